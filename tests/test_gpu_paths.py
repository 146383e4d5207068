"""Every dispatch path of the coordinate-attention ops (csrc/coord.hip) and of the SPPF pool, BiFPN identity add and
layout copy (csrc/pool.hip), each against a plain high-precision reference.

coord.hip picks its pooling kernel, projection kernel, attention kernel, query split and gate tile from the shape.
The first part of this file mirrors those host-side predicates in Python; every case row names the path it is
there for, and a CPU test asserts that the mirror still sends the row down that path.  A retuned heuristic that
moves a row off its path fails there, without a GPU, instead of quietly testing nothing.

The GPU tests then run each row as a drop-in module against the fp64 oracle, five of them again through the C-ABI
on channel-slice views with the fp32 workspace (pooled means, gates) compared with the oracle directly, and the
three pool.hip entry points against exact torch restatements.
"""

import contextlib
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import cases
from fce_yolo_amd import _native as N
from fce_yolo_amd.backend import EagerBackend

OP_TOL = 1e-3  # test_gpu.py: max|ours - ref| <= OP_TOL * max|ref|


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


# =========================================================================== mirror of coord.hip's host side
KG = 16  # lanes per (query, head) of coord_attend_groups_kernel
LDS_MAX = 160 * 1024
CORE_MAX_MACS = 2 << 20
BAND_ROWS = 16


def align_f(n):
    return (n + 63) & ~63


def band_pool_ok(C, W):
    return C >= 256 and C % 64 == 0 and W <= 32 * 8


def ws_layout(inp, oup, mid, n, h, w):
    """ws_layout: ({name: (offset, count)} in floats, total floats); order xh, xw, [part], buf[0..5], g1, g2."""
    L, mx = max(h, w), max(mid, oup)
    off, out = 0, {}

    def take(name, cnt):
        nonlocal off
        out[name] = (off, cnt)
        off += align_f(cnt)

    take("xh", n * h * inp)
    take("xw", n * w * inp)
    if band_pool_ok(inp, w):
        take("part", n * ((h + BAND_ROWS - 1) // BAND_ROWS) * w * inp)
    for i in range(6):
        take(f"buf{i}", n * L * mx)
    take("g1", n * h * oup)
    take("g2", n * w * oup)
    return out, off


def pool_path(N, H, W, C):
    if band_pool_ok(C, W):
        kw = (W + 31) // 32
        NB = (H + BAND_ROWS - 1) // BAND_ROWS
        return f"band KW{3 if kw <= 3 else 5 if kw <= 5 else 8} NB{NB} last{H - BAND_ROWS * (NB - 1)}"
    CG, RG = C // 8, 1
    while RG < 8 and CG * RG * 2 <= 256 and H >= 16 * RG:
        RG *= 2
    XW = 256 // (CG * RG)
    aff = int(N >= 8)
    pad = 8 * ((N + 7) // 8) - N if aff else 0  # images of the padded grid whose blocks must exit
    return f"2pass CG{CG} RG{RG} XW{XW} aff{aff} pad{pad}"


def core_lds_floats(H, W, C, mid, oup):
    L = max(H, W)
    return 2 * L * (C + 4) + 3 * C * mid + mid * oup + 4 * L * (mid + 4) + 4


def use_core(inp, oup, mid, heads, H, W):
    L, dh = max(H, W), mid // heads
    return (dh in (1, 2, 4, 8, 16) and mid % 4 == 0 and oup % 4 == 0 and 3 * L * mid * inp <= CORE_MAX_MACS
            and core_lds_floats(H, W, inp, mid, oup) * 4 <= LDS_MAX)


def qsplit(H, W):
    L, qs = min(H, W), 1
    while qs < 2 and L // (2 * qs) >= 8:
        qs *= 2
    return qs


def attend_grouped(heads):
    return heads <= KG and KG % heads == 0


def proj_kernel(jobs):
    """launch_proj: the register-tiled kernel when every job (K, M) has M % 4 == 0 and K % 4 == 0."""
    m4 = all(M % 4 == 0 and K % 4 == 0 for K, M in jobs)
    return "proj4" if m4 and max(M for _, M in jobs) <= 1024 else "proj1"


def attend_path(mid, heads, oup, Lq, Lk):
    """launch_attend with jobs whose longest query / key axes are Lq / Lk."""
    dh = mid // heads
    if attend_grouped(heads):
        return f"groups<{dh}>"
    QT = max(1, 256 // heads)
    shm = (2 * Lk * mid + QT * mid) * 4
    assert shm <= LDS_MAX
    return f"attend<{dh}> wlds{int(shm + mid * oup * 4 <= LDS_MAX)}"


def coord_path(kind, inp, oup, mid, heads, N, H, W, no_core=False):
    """(pooling, middle, gate) as coord_common dispatches them."""
    L = max(H, W)
    grp = attend_grouped(heads)
    if kind == "Bi" and not no_core and use_core(inp, oup, mid, heads, H, W):
        middle = f"core<{mid // heads}> qs{qsplit(H, W)}"
    elif kind == "Bi":
        middle = [proj_kernel([(inp, mid)] * 6), attend_path(mid, heads, oup, L, L)]
        middle = " + ".join(middle + ([proj_kernel([(mid, oup)] * 2)] if grp else []))
    elif kind == "Att":
        middle = proj_kernel([(inp, mid)] * 2) + " + " + proj_kernel([(mid, oup)] * 2)
    else:
        middle = [proj_kernel([(inp, mid)] * 2), proj_kernel([(mid, mid)] * 3), attend_path(mid, heads, oup, H, W)]
        middle = " + ".join(middle + ([proj_kernel([(mid, oup)])] if grp else []))
    e = W * (oup // 8)  # 8-channel elements of a row
    gpx = 4 if e >= 4096 else 1
    gate = f"gpx{gpx} {'ragged' if e % (256 * gpx) else 'even'}" + (" idconv" if inp != oup else "")
    return pool_path(N, H, W, inp), middle, gate


def mid_heads(kind, args):
    """(mid, heads) of a module's descriptor: modules.BiCoordCrossAtt / CoordAtt / CoordCrossAtt."""
    if kind == "Att":
        return max(8, args[0] // args[2]), 1
    m = max(8, args[0] // args[2])
    return (m // args[3] * args[3], args[3]) if kind == "Bi" else (m, args[3])


# =========================================================================== the case table
# id: (kind, (inp, oup, reduction[, heads]), (N, H, W), no_core, (pooling, middle, gate) the row is there for)
_SPLIT8 = "proj4 + groups<8> + proj4"
COORD = {
    # pool_kernel with the XCD-affine grid (N >= 8): padded to 8 * ceil(N / 8) images, and exact
    "aff_n11": ("Bi", (64, 64, 8, 4), (11, 9, 13), False, ("2pass CG8 RG1 XW32 aff1 pad5", "core<2> qs1", "gpx1 ragged")),
    "aff_n8": ("Bi", (64, 64, 8, 4), (8, 9, 13), False, ("2pass CG8 RG1 XW32 aff1 pad0", "core<2> qs1", "gpx1 ragged")),
    # coord_core_kernel: two query chunks of an odd axis on both branches, and one chunk just below the split
    "core_qs2_odd": ("Bi", (64, 64, 8, 4), (2, 17, 33), False, ("2pass CG8 RG2 XW16 aff0 pad0", "core<2> qs2", "gpx1 ragged")),
    "core_qs1": ("Bi", (64, 64, 8, 4), (2, 16, 15), False, ("2pass CG8 RG2 XW16 aff0 pad0", "core<2> qs1", "gpx1 ragged")),
    # pool_kernel with a channel-group count that does not divide 256, 8 row groups
    "cg3_rg8": ("Bi", (24, 24, 8, 2), (2, 70, 5), False, ("2pass CG3 RG8 XW10 aff0 pad0", "core<4> qs1", "gpx1 ragged")),
    # pool_band_kernel<16, 3 / 5 / 8>: several bands with a short last one, ragged and exact widths
    "band_nb3": ("Bi", (256, 256, 8, 4), (2, 37, 45), False, ("band KW3 NB3 last5", _SPLIT8, "gpx1 ragged")),
    "band_kw5": ("Bi", (256, 256, 8, 4), (1, 18, 100), False, ("band KW5 NB2 last2", _SPLIT8, "gpx1 ragged")),
    "band_kw8": ("Bi", (256, 256, 8, 4), (1, 5, 170), False, ("band KW8 NB1 last5", _SPLIT8, "gpx4 ragged")),
    "band_w256": ("Bi", (256, 256, 8, 4), (1, 4, 256), False, ("band KW8 NB1 last4", _SPLIT8, "gpx4 even")),
    # the fall-back from band pooling to pool_kernel at C >= 256: W > 256, and C % 64 != 0 (CG = 33; K = 264 is
    # projected in chunks of 128 + 128 + 8)
    "w260": ("Bi", (256, 256, 8, 4), (1, 4, 260), False, ("2pass CG32 RG1 XW8 aff0 pad0", _SPLIT8, "gpx4 ragged")),
    "cg33": ("Bi", (264, 264, 8, 4), (2, 19, 21), False, ("2pass CG33 RG2 XW3 aff0 pad0", _SPLIT8, "gpx1 ragged")),
    # gate_apply_kernel<*, 4> with 4160 elements per row against its 1024-element blocks, all three gate modes
    "gpx4": ("Bi", (256, 256, 8, 4), (1, 3, 130), False, ("band KW5 NB1 last3", _SPLIT8, "gpx4 ragged")),
    "gpx4_att": ("Att", (256, 256, 32), (1, 3, 130), False, ("band KW5 NB1 last3", "proj4 + proj4", "gpx4 ragged")),
    "gpx4_cross": ("Cross", (256, 256, 8, 4), (1, 3, 130), False,
                   ("band KW5 NB1 last3", "proj4 + proj4 + groups<8> + proj4", "gpx4 ragged")),
    # coord_attend_kernel (heads not dividing 16, heads > 16) and coord_proj_kernel for its real reason, mid % 4 != 0
    "heads3": ("Bi", (72, 72, 8, 3), (2, 11, 14), False,
               ("2pass CG9 RG1 XW28 aff0 pad0", "proj1 + attend<3> wlds1", "gpx1 ragged")),
    "heads5": ("Bi", (80, 80, 8, 5), (2, 11, 14), False,
               ("2pass CG10 RG1 XW25 aff0 pad0", "proj1 + attend<2> wlds1", "gpx1 ragged")),
    "heads6_core": ("Bi", (96, 96, 8, 6), (2, 11, 14), False, ("2pass CG12 RG1 XW21 aff0 pad0", "core<2> qs1", "gpx1 ragged")),
    "heads6_split": ("Bi", (96, 96, 8, 6), (2, 11, 14), True,
                     ("2pass CG12 RG1 XW21 aff0 pad0", "proj4 + attend<2> wlds1", "gpx1 ragged")),
    # heads 32 > 16: at 6 x 7 it still fits the fused middle (core<1>); at 6 x 13 the middle's LDS need passes
    # 160 KiB (L = 12 is the last that fits) and the row reaches coord_attend_kernel<1>
    "heads32_core": ("Bi", (256, 256, 8, 32), (1, 6, 7), False, ("band KW3 NB1 last6", "core<1> qs1", "gpx1 ragged")),
    "heads32": ("Bi", (256, 256, 8, 32), (1, 6, 13), False, ("band KW3 NB1 last6", "proj4 + attend<1> wlds1", "gpx1 ragged")),
    "heads3_idconv": ("Bi", (64, 96, 8, 3), (2, 11, 14), False,
                      ("2pass CG8 RG1 XW32 aff0 pad0", "proj1 + attend<2> wlds1", "gpx1 ragged idconv")),
    # output projection read from global memory: mid * oup floats do not fit in LDS beside K / V
    "heads3_wlds0": ("Bi", (576, 576, 8, 3), (1, 5, 6), False, ("band KW3 NB1 last5", "proj4 + attend<24> wlds0", "gpx1 ragged")),
    # the head dims that are instantiated and never ran (grouped kernel), with the scalar projection where mid % 4 != 0
    "dh5": ("Bi", (80, 80, 8, 2), (2, 5, 6), False, ("2pass CG10 RG1 XW25 aff0 pad0", "proj1 + groups<5> + proj1", "gpx1 ragged")),
    "dh6": ("Bi", (96, 96, 8, 2), (2, 5, 6), False, ("2pass CG12 RG1 XW21 aff0 pad0", "proj4 + groups<6> + proj4", "gpx1 ragged")),
    "dh7": ("Bi", (112, 112, 8, 2), (2, 5, 6), False, ("2pass CG14 RG1 XW18 aff0 pad0", "proj1 + groups<7> + proj1", "gpx1 ragged")),
    "dh10": ("Bi", (80, 80, 8, 1), (2, 5, 6), False, ("2pass CG10 RG1 XW25 aff0 pad0", "proj1 + groups<10> + proj1", "gpx1 ragged")),
    "dh12": ("Bi", (96, 96, 8, 1), (2, 9, 7), False, ("2pass CG12 RG1 XW21 aff0 pad0", "proj4 + groups<12> + proj4", "gpx1 ragged")),
    "dh20": ("Bi", (160, 160, 8, 1), (2, 5, 6), False, ("2pass CG20 RG1 XW12 aff0 pad0", "proj4 + groups<20> + proj4", "gpx1 ragged")),
    "dh32": ("Bi", (256, 256, 8, 1), (1, 6, 7), False, ("band KW3 NB1 last6", "proj4 + groups<32> + proj4", "gpx1 ragged")),
    "dh48": ("Bi", (384, 384, 8, 1), (1, 5, 6), False, ("band KW3 NB1 last5", "proj4 + groups<48> + proj4", "gpx1 ragged")),
    "dh64": ("Bi", (512, 512, 8, 1), (1, 6, 7), False, ("band KW3 NB1 last6", "proj4 + groups<64> + proj4", "gpx1 ragged")),
    # the other two ops on the same pooling paths
    "att_band_nb3": ("Att", (256, 256, 32), (2, 37, 45), False, ("band KW3 NB3 last5", "proj4 + proj4", "gpx1 ragged")),
    "att_aff": ("Att", (32, 48, 4), (9, 6, 5), False,
                ("2pass CG4 RG1 XW64 aff1 pad7", "proj4 + proj4", "gpx1 ragged idconv")),
    "cross_heads3": ("Cross", (96, 96, 8, 3), (2, 11, 14), False,
                     ("2pass CG12 RG1 XW21 aff0 pad0", "proj4 + proj4 + attend<4> wlds1", "gpx1 ragged")),
    "cross_aff": ("Cross", (64, 64, 4, 2), (10, 7, 9), False,
                  ("2pass CG8 RG1 XW32 aff1 pad6", "proj4 + proj4 + groups<8> + proj4", "gpx1 ragged")),
}
AFF_ROWS = ["aff_n11", "aff_n8"]
ABI_ROWS = ["aff_n11", "band_nb3", "cg33", "heads3_idconv", "cross_heads3"]


@pytest.mark.parametrize("cid", list(COORD))
def test_case_takes_the_path_it_is_there_for(cid):
    kind, args, (n, h, w), no_core, want = COORD[cid]
    mid, heads = mid_heads(kind, args)
    mod = cases.build_coord(kind, args, 0)
    if kind == "Bi":
        assert (mod.mid_dim, mod.num_heads) == (mid, heads)
    elif kind == "Cross":
        assert (mod.mip, mod.num_heads) == (mid, heads)
    else:
        assert mod.cv1.conv.out_channels == mid
    assert coord_path(kind, args[0], args[1], mid, heads, n, h, w, no_core) == want


def test_case_table_covers_every_untested_path():
    """Between them the rows name every coord.hip path that the module fixtures of test_gpu.py never reach."""
    paths = [COORD[c][4] for c in COORD]
    pool, middle, gate = (" | ".join(p[i] for p in paths) for i in range(3))
    for dh in (1, 2, 3, 4, 24):
        assert f"attend<{dh}>" in middle
    assert "wlds0" in middle and "wlds1" in middle and "proj1" in middle
    for dh in (5, 6, 7, 8, 10, 12, 20, 32, 48, 64):
        assert f"groups<{dh}>" in middle
    assert "aff1 pad0" in pool and any("aff1" in p[0] and "pad0" not in p[0] for p in paths)
    for kw in (3, 5, 8):
        assert f"band KW{kw}" in pool
    assert any(p[0].startswith("band") and "NB1" not in p[0] and "last16" not in p[0] for p in paths)
    assert "2pass CG32" in pool and "2pass CG33" in pool and "CG3 RG8" in pool
    assert "core<2> qs2" in middle and COORD["core_qs2_odd"][2][1] % 2 and COORD["core_qs2_odd"][2][2] % 2
    assert any(p[1].startswith("core") and KG % mid_heads(COORD[c][0], COORD[c][1])[1] for c, p in zip(COORD, paths))
    for kind in ("Bi", "Att", "Cross"):
        assert any(COORD[c][0] == kind and "gpx4 ragged" in COORD[c][4][2] for c in COORD)
    assert set(ABI_ROWS) <= set(COORD) and any("idconv" in COORD[c][4][2] for c in ABI_ROWS)


def test_ws_layout_mirror():
    """64-float alignment and the order xh, xw, [part], buf[0..5], g1, g2."""
    lay, total = ws_layout(256, 256, 32, 2, 37, 45)
    assert list(lay) == ["xh", "xw", "part"] + [f"buf{i}" for i in range(6)] + ["g1", "g2"]
    assert all(off % 64 == 0 for off, _ in lay.values()) and total % 64 == 0
    assert lay["part"][1] == 2 * 3 * 45 * 256 and lay["buf0"][1] == 2 * 45 * 256
    lay, total = ws_layout(72, 72, 9, 2, 11, 14)
    assert "part" not in lay and lay["xw"][0] == align_f(2 * 11 * 72) and lay["buf0"][1] == 2 * 14 * 72
    assert total == lay["g2"][0] + align_f(2 * 14 * 72)


@pytest.mark.parametrize("cid", ["aff_n11", "heads3_idconv", "att_aff", "cross_heads3"])
def test_gate_oracle_is_the_oracle(cid):
    """cases.coord_gates restates the oracle functions; its output must be the oracle's, bit for bit."""
    kind, args, shape, _, _ = COORD[cid]
    mod, x = _module_and_input(cid)
    from oracle import fce_oracle as O

    sd = O.cast_sd(O.fuse_state_dict({"m." + k: v for k, v in mod.state_dict().items()}), torch.float64)
    fn = {"Bi": O.bicoordcrossatt, "Att": O.coordatt, "Cross": O.coordcrossatt}[kind]
    with torch.no_grad():
        ref = fn(sd, "m", x.double(), list(args))
    xh, xw, g1, g2, out = cases.coord_oracle(kind, args, mod, x)
    n, h, w = shape
    assert torch.equal(out, ref)
    assert xh.shape == (n, args[0], h) and xw.shape == (n, args[0], w) and g1.shape == (n, args[1], h)
    assert g2 is None if kind == "Cross" else g2.shape == (n, args[1], w)


# =========================================================================== running a case
def _module_and_input(cid):
    kind, args, (n, h, w), _, _ = COORD[cid]
    seed = 1000 + list(COORD).index(cid)
    return cases.build_coord(kind, args, seed), cases.sharpened_input((n, args[0], h, w), seed)


@contextlib.contextmanager
def _no_core(on):
    old = os.environ.get("FCE_COORD_NO_CORE")
    if on:
        os.environ["FCE_COORD_NO_CORE"] = "1"
    try:
        yield
    finally:
        if on:
            if old is None:
                del os.environ["FCE_COORD_NO_CORE"]
            else:
                os.environ["FCE_COORD_NO_CORE"] = old


_RUNS = {}


def _module_run(cid, device):
    """(module on the device, fp16 input, module output on the CPU) of a case, computed once per session."""
    if cid not in _RUNS:
        mod, x = _module_and_input(cid)
        mod = mod.to(device)
        with torch.no_grad(), _no_core(COORD[cid][3]):
            y = mod(x.to(device))
        torch.cuda.synchronize()
        _RUNS[cid] = (mod, x, y.cpu())
    return _RUNS[cid]


class _DescCapture(EagerBackend):
    """Takes the descriptor a module's emit() builds (modules._coord_desc) instead of launching it."""

    def coord(self, kind, desc, x, y):
        self.got = (kind, desc)


def _ws_bytes(cid, device):
    kind, args, (n, h, w), _, _ = COORD[cid]
    mod = _module_run(cid, device)[0]
    be = _DescCapture(device)
    mod.emit(be, be.alloc(n, args[0], h, w))
    k, desc = be.got
    assert k == ["Bi", "Att", "Cross"].index(kind)
    return k, desc, N.lib().fce_coord_workspace_bytes(C.byref(desc), n, h, w)


# =========================================================================== 2. module-level parity on every path
@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(COORD))
def test_coord_module_parity_on_every_path(cid, device):
    """The drop-in module of every row against the fp64 oracle on the same fp16 input, at the project's op bar;
    the mirrored workspace layout must give the library's workspace size."""
    kind, args, (n, h, w), _, _ = COORD[cid]
    mod, x, y = _module_run(cid, device)
    ref = cases.coord_oracle(kind, args, mod, x)[4]
    assert tuple(y.shape) == tuple(ref.shape) and torch.isfinite(y).all()
    err = _rel(y.float(), ref)
    print(f"OPERR {cid} {err:.3e}")
    assert err <= OP_TOL, err
    mid, _ = mid_heads(kind, args)
    assert ws_layout(args[0], args[1], mid, n, h, w)[1] * 4 == _ws_bytes(cid, device)[2]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", AFF_ROWS)
def test_coord_affine_grid_batch_invariance(cid, device):
    """An image of the N >= 8 run (XCD-affine pooling grid) equals the same image run alone and in a batch of two,
    bit for bit: the pooling blocks do the same sums in the same order either way."""
    mod, x, y = _module_run(cid, device)
    n = x.shape[0]
    with torch.no_grad():
        for i in range(n):
            y1 = mod(x[i:i + 1].to(device)).cpu()
            assert torch.equal(y1[0], y[i]), ("alone", i)
        for i in range(0, n, 2):
            pair = [i, (i + 1) % n]
            y2 = mod(x[pair].to(device)).cpu()
            assert torch.equal(y2, y[pair]), ("pair", pair)
    print(f"OPERR {cid} batch-invariant over {n} images")


# =========================================================================== 3. C-ABI on views, workspace vs fp64
GATE_K = 8  # see the docstring of test_coord_c_abi_views_and_workspace


def _nhwc(t):
    return t.permute(0, 2, 1).contiguous()  # oracle [N, C, L] -> workspace [N, L, C]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ABI_ROWS)
def test_coord_c_abi_views_and_workspace(cid, device):
    """fce_bicoordcrossatt / fce_coordatt / fce_coordcrossatt called directly: x a channel slice (offset 16) of a
    buffer 24 channels wider, y a slice (offset 8) of a NaN-filled buffer 16 channels wider.

    * y's slice equals the module-level result bit for bit and y's other channels are still NaN;
    * the pooled means in the workspace are within (L + 2) * 2^-24 * sum|x_i| / L of the fp64 means per element
      (L values averaged: the worst case of an fp32 sum of exactly converted fp16 values in any order, times the
      rounded 1 / L, rounded);
    * the gates in the workspace (fp32: pre-sigmoid logits for BiCoordCrossAtt, sigmoid gates otherwise) deviate from
      the fp64 oracle, relative to max|ref|, by at most GATE_K times what the same oracle run in fp32 on the CPU
      deviates (per array; the fp32 run deviates by 1.8e-7 .. 5.1e-7).  Measured on MI355X, the larger of the g1 and
      g2 ratios of each case: aff_n11 0.78, band_nb3 1.00, cg33 2.33, heads3_idconv 0.79, cross_heads3 1.80.
      GATE_K = 8 is the smallest power of two that holds on all five with a factor 2 to spare (2 * 2.33 = 4.66).
    """
    kind, args, (n, h, w), _, _ = COORD[cid]
    inp, oup = args[0], args[1]
    mod, x, ymod = _module_run(cid, device)
    k, desc, nbytes = _ws_bytes(cid, device)
    g = torch.Generator().manual_seed(5)
    xbuf = torch.randn(n, h, w, inp + 24, generator=g).half()
    xbuf[..., 16:16 + inp] = x.permute(0, 2, 3, 1)
    xbuf = xbuf.to(device)
    ybuf = torch.full((n, h, w, oup + 16), float("nan"), dtype=torch.float16, device=device)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=device)
    xt = N.Tensor(xbuf.data_ptr(), N.F16, N.NHWC, n, inp, h, w, inp + 24, 16)
    yt = N.Tensor(ybuf.data_ptr(), N.F16, N.NHWC, n, oup, h, w, oup + 16, 8)
    fn = ("fce_bicoordcrossatt", "fce_coordatt", "fce_coordcrossatt")[k]
    with _no_core(COORD[cid][3]):
        N.call(fn, C.byref(desc), C.byref(xt), C.byref(yt), ws.data_ptr(), nbytes, torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize()
    yb, wsc = ybuf.cpu(), ws.cpu()

    # the workspace first: a wrong mean or gate is named as such before it shows as a wrong y
    mid, _ = mid_heads(kind, args)
    lay, total = ws_layout(inp, oup, mid, n, h, w)
    assert total * 4 == nbytes

    def read(name, L, c):
        off, cnt = lay[name]
        assert cnt == n * L * c
        return wsc[off:off + cnt].view(n, L, c).double()

    xh, xw, g1, g2, _ = cases.coord_oracle(kind, args, mod, x)
    xa = x.double().abs()
    for name, L, ref, bound in (("xh", h, xh, (w + 2) * 2.0**-24 * xa.sum(3) / w),
                                ("xw", w, xw, (h + 2) * 2.0**-24 * xa.sum(2) / h)):
        got, ref, bound = read(name, L, inp), _nhwc(ref), _nhwc(bound)
        worst = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
        print(f"OPERR {cid} {name} worst |err| / bound {worst:.3f}")
        assert torch.isfinite(got).all() and ((got - ref).abs() <= bound).all(), (name, worst)

    r32 = cases.coord_oracle(kind, args, mod, x, torch.float32)
    ratios = []
    for name, L, ref, ref32 in (("g1", h, g1, r32[2]), ("g2", w, g2, r32[3])):
        if ref is None:
            continue
        got, scale = read(name, L, oup), ref.abs().max()
        assert torch.isfinite(got).all()
        dev = ((got - _nhwc(ref)).abs().max() / scale).item()
        dev32 = ((ref32.double() - ref).abs().max() / scale).item()
        print(f"OPERR {cid} {name} gpu {dev:.3e} fp32-cpu {dev32:.3e} ratio {dev / dev32:.2f}")
        ratios.append(dev / dev32)
    assert max(ratios) <= GATE_K, ratios

    assert torch.equal(yb[..., 8:8 + oup].permute(0, 3, 1, 2), ymod)
    assert torch.isnan(yb[..., :8]).all() and torch.isnan(yb[..., 8 + oup:]).all()


# =========================================================================== 4. pool.hip
def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _pool_values(n, c, h, w, seed):
    """NHWC fp16 randn with -inf, +-65504 sprinkled in and, on maps that hold one, a 7 x 7 all -inf patch (a y1
    window of only -inf); no NaN (the reference model never pools one)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g)
    r = torch.rand(n, h, w, c, generator=g)
    x[r < 0.03] = float("-inf")
    x[(r >= 0.03) & (r < 0.04)] = 65504.0
    x[(r >= 0.04) & (r < 0.05)] = -65504.0
    if h >= 10 and w >= 9:
        x[:, 1:8, 1:8, :3] = float("-inf")
    return x.half()


def _maxpool_chain(x, k, device):
    """fce_maxpool_chain on the SPPF concat layout: x and y1..y3 are the four c-channel slices of one buffer of
    4c + 8 channels; returns the buffer (CPU)."""
    n, h, w, c = x.shape
    buf = torch.full((n, h, w, 4 * c + 8), float("nan"), dtype=torch.float16)
    buf[..., :c] = x
    buf = buf.to(device)
    ts = [N.Tensor(buf.data_ptr(), N.F16, N.NHWC, n, c, h, w, 4 * c + 8, i * c) for i in range(4)]
    N.call("fce_maxpool_chain", *(C.byref(t) for t in ts), k, _stream(device))
    torch.cuda.synchronize()
    return buf.cpu()


def _maxpool_ref(x, k):
    ys, t = [], x.float().permute(0, 3, 1, 2)
    for _ in range(3):
        t = F.max_pool2d(t, k, 1, k // 2)
        ys.append(t.permute(0, 2, 3, 1).half())
    return ys


@pytest.mark.gpu
@pytest.mark.parametrize("n,c,h,w,k", [
    (3, 24, 10, 9, 5),    # 9 blocks: the tail of the XCD remap (grid not a multiple of 8)
    (1, 8, 33, 32, 5),    # H * W = 1056: a second, ragged staging pass
    (1, 8, 4, 3, 5),      # all three windows wider than the map
    (1, 16, 52, 50, 5),   # H * W = 2600: the direct kernel (no LDS plane)
    (2, 16, 13, 17, 3), (2, 16, 13, 17, 9), (2, 16, 13, 17, 13),
])
def test_maxpool_chain_bitwise(n, c, h, w, k, device):
    """y1, y2, y3 against max_pool2d(k, 1, k // 2) applied one, two and three times to the same values (max is
    exact: bit for bit), the input slice and the 8 pad channels of the concat buffer untouched."""
    x = _pool_values(n, c, h, w, 31 * h + w + k)
    buf = _maxpool_chain(x, k, device)
    assert torch.equal(_bits(buf[..., :c]), _bits(x))
    assert torch.isnan(buf[..., 4 * c:]).all()
    for i, ref in enumerate(_maxpool_ref(x, k), 1):
        got = buf[..., i * c:(i + 1) * c]
        bad = int((_bits(got) != _bits(ref)).sum())
        print(f"OPERR maxpool {n}x{c}x{h}x{w} k{k} y{i} mismatches {bad} (-inf outputs {int(torch.isinf(ref).sum())})")
        assert bad == 0, (i, bad)
    if h * w > 2560:
        # the same data through the LDS-plane kernel: a 20 x 20 crop agrees wherever a window lies inside the crop
        crop = _maxpool_chain(x[:, 10:30, 10:30].contiguous(), k, device)
        for i in (1, 2, 3):
            r = i * (k // 2)
            a = crop[:, r:20 - r, r:20 - r, i * c:(i + 1) * c]
            b = buf[:, 10 + r:30 - r, 10 + r:30 - r, i * c:(i + 1) * c]
            assert a.numel() and torch.equal(_bits(a), _bits(b)), i


@pytest.mark.gpu
@pytest.mark.parametrize("up", [0, 1, 2])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_weighted_add_views(up, accumulate, device):
    """fce_weighted_add: y = (accumulate ? y : 0) + relu(w)[fi] / (sum relu(w) + 1e-4) * nearest_up(x) on channel
    slices (offset 8 of 40 channels, both sides) against the same expression in fp64.  Per element
    |err| <= 2^-11 |ref| + 2^-20 (|prev| + |alpha x|) + 2^-25: half an fp16 ulp of the result, the few fp32 ulps of the
    operands that can flip that rounding, and the fp16 subnormal floor.  Without accumulate y starts as NaN and must
    not be read."""
    n, c, hs, ws = 2, 24, 5, 7
    h, w = hs << up, ws << up
    g = torch.Generator().manual_seed(40 + up)
    xbuf = torch.randn(n, hs, ws, 40, generator=g).half()
    prev = torch.randn(n, h, w, c, generator=g).half()
    worst = 0.0
    for fw, fis in (([0.7, -0.2, 1.3], (0, 1, 2)), ([0.5, 1.5], (0, 1))):
        fwt = torch.tensor(fw, dtype=torch.float32)
        fwd = fwt.to(device)
        for fi in fis:
            ybuf = torch.full((n, h, w, 40), float("nan"), dtype=torch.float16)
            if accumulate:
                ybuf[..., 8:8 + c] = prev
            yd, xd = ybuf.to(device), xbuf.to(device)
            xt = N.Tensor(xd.data_ptr(), N.F16, N.NHWC, n, c, hs, ws, 40, 8)
            yt = N.Tensor(yd.data_ptr(), N.F16, N.NHWC, n, c, h, w, 40, 8)
            N.call("fce_weighted_add", C.byref(xt), up, fwd.data_ptr(), len(fw), fi, accumulate, C.byref(yt), _stream(device))
            torch.cuda.synchronize()
            y = yd.cpu()
            assert torch.isnan(y[..., :8]).all() and torch.isnan(y[..., 8 + c:]).all()
            assert torch.equal(_bits(xd.cpu()), _bits(xbuf))
            rw = torch.relu(fwt.double())
            alpha = rw[fi] / (rw.sum() + 1e-4)
            xu = xbuf[..., 8:8 + c].double().repeat_interleave(1 << up, 1).repeat_interleave(1 << up, 2)
            p = prev.double() if accumulate else torch.zeros_like(xu)
            ref = p + alpha * xu
            bound = 2.0**-11 * ref.abs() + 2.0**-20 * (p.abs() + (alpha * xu).abs()) + 2.0**-25
            err = (y[..., 8:8 + c].double() - ref).abs()
            assert torch.isfinite(y[..., 8:8 + c]).all() and (err <= bound).all(), (fw, fi, (err / bound).max().item())
            worst = max(worst, (err / bound).max().item())
            if fw[fi] < 0:  # relu: alpha is exactly 0
                assert torch.equal(y[..., 8:8 + c].double(), p), (fw, fi)
    print(f"OPERR weighted_add up{up} acc{accumulate} worst |err| / bound {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 20, 9, 4)])
@pytest.mark.parametrize("kind", ["u8_nchw->f16_view", "f16_view->f32_nchw", "f32_nchw->f16_nhwc", "f16_slice->f16_slice"])
def test_copy_bitwise(kind, shape, device):
    """fce_copy across the layout / dtype edges a drop-in needs, bit for bit; an NHWC view is channels [8, 8 + c) of a
    buffer of cs channels (16, or c + 12 where c does not fit), and destination channels outside it stay NaN."""
    n, c, h, w = shape
    cs = 16 if c <= 8 else c + 12
    g = torch.Generator().manual_seed(c)
    nan16 = torch.full((n, h, w, cs), float("nan"), dtype=torch.float16)

    def view(buf, cstride=cs, coff=8):
        return N.Tensor(buf.data_ptr(), N.F16, N.NHWC, n, c, h, w, cstride, coff)

    def nchw(buf, dt):
        return N.Tensor(buf.data_ptr(), dt, N.NCHW, n, c, h, w, c, 0)

    if kind == "u8_nchw->f16_view":
        src = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        want, sd, dd = src.permute(0, 2, 3, 1).half(), src.to(device), nan16.to(device)
        st, dt, pick = nchw(sd, N.U8), view(dd), lambda d: d[..., 8:8 + c]
    elif kind == "f16_view->f32_nchw":
        src = torch.randn(n, h, w, cs, generator=g).half()
        want, sd = src[..., 8:8 + c].permute(0, 3, 1, 2).float(), src.to(device)
        dd = torch.full(shape, float("nan"), dtype=torch.float32, device=device)
        st, dt, pick = view(sd), nchw(dd, N.F32), lambda d: d
    elif kind == "f32_nchw->f16_nhwc":
        src = torch.randn(shape, generator=g) * 8
        src.view(-1)[:6] = torch.tensor([65504.0, 65519.9, 70000.0, -1e-7, 3e-6, 2049.0])  # round, overflow, subnormal
        want, sd = src.half().permute(0, 2, 3, 1), src.to(device)
        dd = torch.full((n, h, w, c), float("nan"), dtype=torch.float16, device=device)
        st, dt, pick = nchw(sd, N.F32), view(dd, c, 0), lambda d: d
    else:
        src = torch.randn(n, h, w, cs, generator=g).half()
        want, sd, dd = src[..., 8:8 + c], src.to(device), torch.full((n, h, w, cs + 8), float("nan"), dtype=torch.float16).to(device)
        st, dt, pick = view(sd), view(dd, cs + 8, 16), lambda d: d[..., 16:16 + c]
    N.call("fce_copy", C.byref(st), C.byref(dt), _stream(device))
    torch.cuda.synchronize()
    d = dd.cpu()
    got = pick(d).contiguous()
    want = want.contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape
    same = torch.equal(got.view(torch.int16 if got.dtype == torch.float16 else torch.int32),
                       want.view(torch.int16 if want.dtype == torch.float16 else torch.int32))
    print(f"OPERR copy {kind} {shape} bitwise {same}")
    assert same
    if d.dtype == torch.float16 and d.shape[-1] != c:
        mask = torch.ones(d.shape[-1], dtype=torch.bool)
        lo = 16 if kind == "f16_slice->f16_slice" else 8
        mask[lo:lo + c] = False
        assert torch.isnan(d[..., mask]).all()
