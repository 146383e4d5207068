"""Test-time augmentation on the device: the two kernels of csrc/tta.hip bit for bit against their CPU restatements
(tests/tta_ref.py), the three-pass AugmentedEngine against the reference's DetectionModel._predict_augment
(golden/tta.npz), and augment=True through NMS, Predictor and patch_autobackend."""

from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import tta_ref
from conftest import GOLDEN, _Npz
from fce_yolo_amd import _native as N
from fce_yolo_amd import predict as P
from fce_yolo_amd import tta
from fce_yolo_amd.engine import NMS, Engine
from oracle import nms_oracle

pytestmark = pytest.mark.gpu

BOX_TOL = 1e-3  # the project's forward parity rule (test_gpu.py): box error relative to the reference's max |box|,
CLS_TOL = 1e-3  # class-score error absolute
B = 2
CASES = {"192_b2": (192, 192), "192x160_b2": (192, 160)}
RANGES = {"192_b2": ([756, 525, 525], [(0, 720), (0, 525), (400, 125)]),
          "192x160_b2": ([630, 525, 420], [(0, 600), (0, 525), (320, 100)])}


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def tta_fx():
    return _Npz(GOLDEN / "tta.npz")


@pytest.fixture(scope="module")
def model(tta_fx, device):
    return tta_ref.model_zero_cls_bias(int(tta_fx.z["e2e/model_seed"])).to(device)


@pytest.fixture(scope="module")
def cpu_model(tta_fx):
    """The same model on the host, for the CPU oracle."""
    return tta_ref.model_zero_cls_bias(int(tta_fx.z["e2e/model_seed"]))


@pytest.fixture(scope="module")
def inputs(tta_fx):
    """key -> the fixture's input batch (fp16, host)."""
    out = {}
    for key in CASES:
        fx = tta_fx.group(f"e2e/{key}")
        out[key] = torch.rand(*fx["shape"].tolist(), generator=torch.Generator().manual_seed(int(fx["x_seed"]))).half()
    return out


@pytest.fixture(scope="module")
def augs(model, device):
    """key -> one AugmentedEngine per fixture case, shared by the tests (they pass graph= per call)."""
    engs = {key: tta.AugmentedEngine(model, B, hw, device) for key, hw in CASES.items()}
    yield engs
    for e in engs.values():
        e.close()


def _as(x, dtype):
    """The test image in one of the network input types (u8: quantised first, so the three types differ)."""
    if dtype == torch.uint8:
        return (x.float() * 255).round().to(torch.uint8)
    return x.to(dtype)


# ---------------------------------------------------------------- 1. scale kernel
def _scale_cases(tta_fx):
    imgs = {}
    for name in ("a", "b"):
        fx = tta_fx.group(f"resize/{name}")
        imgs[name] = torch.rand(*fx["shape"].tolist(), generator=torch.Generator().manual_seed(int(fx["seed"])))
    imgs["engine"] = torch.rand(2, 3, 192, 160, generator=torch.Generator().manual_seed(7))
    imgs["wide"] = torch.rand(1, 3, 20, 700, generator=torch.Generator().manual_seed(8))  # three blocks along W
    out = []
    for name, x in imgs.items():
        for r in (0.83, 0.67):
            out.append((name, x, tta.scale_geometry(x.shape[2], x.shape[3], r, 32)))
    # a canvas whose width is no multiple of 4 (the element-wise store path), with padding on both sides
    out.append(("odd", imgs["b"], (30, 43, 31, 45)))
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.uint8], ids=["f16", "f32", "u8"])
def test_scale_img_kernel_bitwise(dtype, tta_fx, device):
    for name, x, (h_s, w_s, H_c, W_c) in _scale_cases(tta_fx):
        xd = _as(x, dtype)
        for flip in (0, 3, 2):
            ref = tta_ref.scale_img_ref(xd, flip, h_s, w_s, H_c, W_c)
            out = torch.full((*x.shape[:2], H_c, W_c), -1.0, dtype=torch.float16, device=device)
            tta.scale_img(xd.to(device), out, flip, h_s, w_s)
            torch.cuda.synchronize()
            got = out.cpu()
            nbad = int((got.view(torch.int16) != ref.view(torch.int16)).sum())
            assert nbad == 0, (name, flip, (h_s, w_s, H_c, W_c), nbad, (got.float() - ref.float()).abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.uint8], ids=["f16", "f32", "u8"])
def test_scale_img_kernel_ratio_one_is_the_converted_copy(dtype, device):
    for shape in ((1, 3, 37, 53), (2, 3, 64, 96)):
        x = _as(torch.rand(*shape, generator=torch.Generator().manual_seed(11)), dtype)
        want = (x.half() / 255) if dtype == torch.uint8 else x.half()
        out = torch.full(shape, -1.0, dtype=torch.float16, device=device)
        tta.scale_img(x.to(device), out, None, shape[2], shape[3])
        assert torch.equal(out.cpu(), want)
        assert torch.equal(tta_ref.scale_img_ref(x, None, shape[2], shape[3], shape[2], shape[3]), want)


def test_scale_img_kernel_refuses_bad_arguments(device):
    x = torch.zeros(1, 3, 16, 16, dtype=torch.float16, device=device)
    out = torch.zeros(1, 3, 32, 32, dtype=torch.float16, device=device)
    with pytest.raises(N.FceError, match="flip"):
        tta.scale_img(x, out, 1, 13, 13)
    with pytest.raises(N.FceError, match="fit the canvas"):
        tta.scale_img(x, out, 0, 33, 13)
    tx = N.Tensor(x.data_ptr(), N.F16, N.NHWC, 1, 3, 16, 16, 3, 0)
    ty = N.Tensor(out.data_ptr(), N.F16, N.NCHW, 1, 3, 32, 32, 3, 0)
    with pytest.raises(N.FceError, match="NCHW"):
        N.call("fce_tta_scale_img", C.byref(tx), C.byref(ty), 0, 13, 13, 0.447, None)
    tx.layout, ty.dtype = N.NCHW, N.F32
    with pytest.raises(N.FceError, match="f16"):
        N.call("fce_tta_scale_img", C.byref(tx), C.byref(ty), 0, 13, 13, 0.447, None)


# ---------------------------------------------------------------- 2. merge kernel
def _random_parts(key, flips, seed, rows=84):
    anchors, ranges = RANGES[key]
    g = torch.Generator().manual_seed(seed)
    H, W = CASES[key]
    parts = []
    for a, (first, count), s, f in zip(anchors, ranges, tta.SCALES, flips):
        p = torch.rand(B, rows, a, generator=g) * 200 - 4
        k = torch.randint(-2 ** 62, 2 ** 62, (B, a), generator=g)
        parts.append((p, k, first, count, s, f, H, W))
    return parts


def _to(parts, device):
    return [(p.to(device), k.to(device), *rest) for p, k, *rest in parts]


@pytest.mark.parametrize("key", list(CASES))
@pytest.mark.parametrize("flips", [tta.FLIPS, (2, None, 3)], ids=["reference", "updown"])
def test_merge_kernel_bitwise(key, flips, device):
    parts = _random_parts(key, flips, 21)
    total = sum(c for _, c in RANGES[key][1])
    ref_p, ref_b = tta_ref.merge_ref(parts)
    for with_best in (True, False):
        out = torch.full((B, 84, total), -7.0, device=device)
        best = torch.full((B, total), -7, dtype=torch.int64, device=device) if with_best else None
        dparts = _to(parts, device)
        if not with_best:
            dparts = [(p, None, *rest) for p, _, *rest in dparts]
        tta.merge(dparts, out, best)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), ref_p.numpy().view(np.uint32))
        if with_best:
            assert torch.equal(best.cpu(), ref_b)


def test_merge_kernel_scale_one_reproduces_the_source_bits(device):
    g = torch.Generator().manual_seed(22)
    bits = torch.randint(-2 ** 31, 2 ** 31, (B, 9, 1370), generator=g, dtype=torch.int64).to(torch.int32)
    p = bits.view(torch.float32)
    p = torch.where(torch.isnan(p), torch.zeros_like(p), p)  # any bit pattern but the NaNs, denormals included
    k = torch.randint(-2 ** 62, 2 ** 62, (B, 1370), generator=g)
    out = torch.empty(B, 9, 1370, device=device)
    best = torch.empty(B, 1370, dtype=torch.int64, device=device)
    tta.merge([(p.to(device), k.to(device), 0, 1370, 1, None, 192, 192)], out, best)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), p.numpy().view(np.uint32))
    assert torch.equal(best.cpu(), k)


def test_merge_kernel_errors_launch_nothing(device):
    p = torch.rand(B, 84, 100, device=device)
    k = torch.zeros(B, 100, dtype=torch.int64, device=device)
    out = torch.full((B, 84, 100), -7.0, device=device)
    best = torch.full((B, 100), -7, dtype=torch.int64, device=device)
    with pytest.raises(N.FceError, match="parts"):  # more than 4
        tta.merge([(p, k, 0, 20, 1, None, 64, 64)] * 5, out, best)
    with pytest.raises(N.FceError, match="outside its anchors"):
        tta.merge([(p, k, 0, 50, 1, None, 64, 64), (p, k, 51, 50, 1, None, 64, 64)], out, best)
    with pytest.raises(N.FceError, match="flip"):
        tta.merge([(p, k, 0, 100, 1, 1, 64, 64)], out, best)
    with pytest.raises(N.FceError, match="every part"):
        tta.merge([(p, k, 0, 50, 1, None, 64, 64), (p, None, 0, 50, 1, None, 64, 64)], out, best)
    torch.cuda.synchronize()
    assert (out == -7).all() and (best == -7).all()


# ---------------------------------------------------------------- 3. per-pass attribution
@pytest.mark.parametrize("key", list(CASES))
def test_each_pass_engine_against_the_oracle(key, cpu_model, inputs, augs, device):
    """Every pass's Engine on scale_img_ref's image against the CPU oracle on the same image: if a later test fails
    while this passes, the forwards are not the cause."""
    aug = augs[key]
    for i, (xi, s, f) in enumerate(tta_ref.pass_images(inputs[key])):
        eng = aug.engines[i]
        assert tuple(xi.shape[2:]) == (eng.H, eng.W)
        y = eng(xi.to(device), graph=False).clone().cpu()
        ref = cases.oracle_model(cpu_model, xi.float(), torch.float32).float()
        box, cls = _rel(y[:, :4], ref[:, :4]), (y[:, 4:] - ref[:, 4:]).abs().max().item()
        print(f"{key} pass {i} ({eng.H}x{eng.W}): box rel {box:.2e} cls abs {cls:.2e}")
        assert box <= BOX_TOL and cls <= CLS_TOL, (i, box, cls)


# ---------------------------------------------------------------- 4. merged tensor
@pytest.mark.parametrize("key", list(CASES))
def test_augmented_engine_against_the_reference(key, tta_fx, inputs, augs, device):
    fx = tta_fx.group(f"e2e/{key}")
    aug = augs[key]
    seg = fx["segments"].tolist()
    assert aug.anchors == sum(seg) and tuple(aug.pred.shape) == (B, 84, sum(seg))
    assert [c for _, c in aug.ranges] == seg and aug.ranges == RANGES[key][1]
    ref = torch.from_numpy(fx["y_rows"])
    x = inputs[key].to(device)
    ys = {}
    for graph in (True, False, True):  # capture, direct launches, replay
        y = aug(x, out=torch.empty_like(aug.pred), graph=graph)
        torch.cuda.synchronize()
        ys.setdefault(graph, []).append(y.cpu())
        got = y.cpu()[:, tta_ref.GOLDEN_KEY_ROWS]
        off = 0
        for k, n in enumerate(seg):
            g, r = got[:, :, off:off + n], ref[:, :, off:off + n]
            box, cls = _rel(g[:, :4], r[:, :4]), (g[:, 4:] - r[:, 4:]).abs().max().item()
            print(f"{key} graph {graph} segment {k}: box rel {box:.2e} cls abs {cls:.2e}")
            assert box <= BOX_TOL and cls <= CLS_TOL, (graph, k, box, cls)
            off += n
    assert torch.equal(ys[True][0], ys[False][0]) and torch.equal(ys[True][0], ys[True][1])


@pytest.mark.parametrize("key", list(CASES))
def test_augmented_engine_is_three_engines_and_the_merge(key, model, inputs, augs, device):
    aug = augs[key]
    x = inputs[key].to(device)
    best = aug.new_best().fill_(-1)
    y = aug(x, out=torch.empty_like(aug.pred), best=best, graph=False)
    H, W = CASES[key]
    parts, engs = [], []
    for s, f in zip(tta.SCALES, tta.FLIPS):
        h_s, w_s, H_c, W_c = tta.scale_geometry(H, W, s, 32)
        eng = Engine(model, B, (H_c, W_c), device)
        engs.append(eng)
        xi = x if s == 1 else tta.scale_img(x, torch.empty(B, 3, H_c, W_c, dtype=torch.float16, device=device), f, h_s, w_s)
        eng(xi, graph=False)
        parts.append([eng.pred, eng.best, s, f])
    ranges = tta.clip_ranges([e.anchors for e in engs], 3)
    y2, best2 = torch.empty_like(y), torch.empty_like(best)
    tta.merge([(p, k, first, count, s, f, H, W) for (p, k, s, f), (first, count) in zip(parts, ranges)], y2, best2)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(best, best2)
    # the scale kernel's images are scale_img_ref's (bitwise), so the merged tensor is merge_ref of the passes
    ref_y, ref_b = tta_ref.merge_ref([(p.cpu(), k.cpu(), first, count, s, f, H, W)
                                      for (p, k, s, f), (first, count) in zip(parts, ranges)])
    assert torch.equal(y.cpu(), ref_y) and torch.equal(best.cpu(), ref_b)
    c = aug.clone()
    assert c.anchors == aug.anchors and c.engines[0] is not aug.engines[0]
    bc = c.new_best().fill_(-1)
    yc = c(x, out=torch.empty_like(aug.pred), best=bc)
    torch.cuda.synchronize()
    assert torch.equal(y, yc) and torch.equal(best, bc)
    c.close()
    for e in engs:
        e.close()


def test_augmented_engine_input_types_and_shape_check(model, inputs, augs, device):
    """u8 input is fp16(v / 255) in every pass (as the stem reads it), f32 is rounded to fp16; a wrong shape raises
    before anything is launched."""
    aug = augs["192x160_b2"]
    x8 = (inputs["192x160_b2"].float() * 255).round().to(torch.uint8)
    a = aug(x8.to(device)).clone()
    b = aug((x8.half() / 255).to(device)).clone()
    c = aug((x8.half() / 255).float().to(device)).clone()
    assert torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(ValueError):
        aug(torch.zeros(B, 3, 160, 192, dtype=torch.float16, device=device))


# ---------------------------------------------------------------- 5. best-class keys and NMS
@pytest.mark.parametrize("key", list(CASES))
def test_merged_best_class_keys_and_nms(key, inputs, augs, device):
    aug = augs[key]
    x = inputs[key].to(device)
    seg = [c for _, c in aug.ranges]
    off = np.concatenate(([0], np.cumsum(seg)))
    for graph in (False, True):
        best = aug.new_best().fill_(-1)
        pred = aug(x, out=torch.empty_like(aug.pred), best=best, graph=graph)
        torch.cuda.synchronize()
        sc, cl = pred[:, 4:].max(1)
        kb = best.cpu().numpy().view(np.uint64)
        assert np.array_equal((kb >> np.uint64(32)).astype(np.uint32), sc.cpu().numpy().view(np.uint32))
        assert np.array_equal((np.uint64(0xFFFFFFFF) - (kb & np.uint64(0xFFFFFFFF))).astype(np.int64), cl.cpu().numpy())
        n1, n2 = NMS(B, aug.anchors, aug.nc, device), NMS(B, aug.anchors, aug.nc, device)
        n1(pred)
        n2(pred, best)
        torch.cuda.synchronize()
        assert torch.equal(n1.buf, n2.buf)
        dets, keep = n2.results()
        od, ok = nms_oracle.non_max_suppression(pred.cpu().numpy())
        for b in range(B):
            kept = keep[b].cpu().numpy()
            assert np.array_equal(kept, ok[b]), (graph, b)
            assert np.array_equal(dets[b].cpu().numpy()[:, 4:], od[b][:, 4:]), (graph, b)
            assert np.array_equal(dets[b].cpu().numpy(), od[b]), (graph, b)
            per_seg = [int(((kept >= off[k]) & (kept < off[k + 1])).sum()) for k in range(3)]
            assert min(per_seg) >= 1, (graph, b, per_seg)  # every pass contributes: the test cannot pass vacuously


# ---------------------------------------------------------------- 6. Predictor
def _images(rng, shapes):
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def _chain_by_hand(eng, imgs, device):
    """Letterbox -> executor -> NMS (with the keys) -> fce_scale_boxes for exactly eng.batch images."""
    lb = P.Letterbox(eng.batch, (eng.H, eng.W), device)
    canvas = lb([torch.from_numpy(im).to(device) for im in imgs])
    best = eng.new_best()
    pred = eng(canvas, out=torch.empty_like(eng.pred), best=best)
    nms = NMS(eng.batch, eng.anchors, eng.nc, device)
    dets, keep, counts = nms(pred, best)
    host = (P.BoxScale * eng.batch)()
    for i, im in enumerate(imgs):
        h0, w0 = im.shape[:2]
        gain, px, py = P.box_scale(eng.H, eng.W, h0, w0)
        host[i] = P.BoxScale(gain, px, py, h0, w0)
    sc = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(device)
    N.call("fce_scale_boxes", C.c_void_p(dets.data_ptr()), C.c_void_p(counts.data_ptr()), eng.batch, 300,
           C.c_void_p(sc.data_ptr()), torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize()
    d, k = nms.results()
    return [t.cpu() for t in d], [t.cpu() for t in k]


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(torch.equal(x, y) for x, y in zip(list(a[0]) + list(a[1]), list(b[0]) + list(b[1])))


@pytest.mark.parametrize("augment", [True, False])
def test_predictor_is_the_chain_composed_by_hand(augment, model, augs, device):
    imgs = _images(np.random.default_rng(31), [(150, 200), (240, 130)])
    pred = P.Predictor(model, B, 192, device, augment=augment)
    assert isinstance(pred.engine, tta.AugmentedEngine if augment else Engine)
    assert all(ln.nms.anchors == pred.engine.anchors for ln in pred.lanes)
    got = pred(imgs, return_idxs=True)
    pred.close()
    eng = augs["192_b2"] if augment else Engine(model, B, 192, device)
    want = _chain_by_hand(eng, imgs, device)
    assert sum(len(k) for k in want[1]) > 0
    assert _same(got, want)
    if augment:  # detections come from every pass
        off = np.concatenate(([0], np.cumsum([c for _, c in eng.ranges])))
        for k in got[1]:
            assert all(((k.numpy() >= off[j]) & (k.numpy() < off[j + 1])).any() for j in range(3))
    else:
        eng.close()


def test_predictor_augment_stream_matches_one_at_a_time(model, device):
    rng = np.random.default_rng(32)
    batches = [_images(rng, [(150, 200), (240, 130)]), _images(rng, [(192, 192)]), _images(rng, [(100, 300), (64, 64)])]
    p1 = P.Predictor(model, B, 192, device, lanes=1, graph=False, augment=True)
    seq = [p1(b, return_idxs=True) for b in batches]
    p1.close()
    p2 = P.Predictor(model, B, 192, device, lanes=2, augment=True)
    n = 0
    for i, r in enumerate(p2.stream(batches, return_idxs=True)):
        assert _same(r, seq[i]), i
        n += 1
    p2.close()
    assert n == 3


# ---------------------------------------------------------------- 7. patch_autobackend
def test_patched_autobackend_augment(model, inputs, augs, device):
    from fce_yolo_amd import integrate

    be = SimpleNamespace(model=model, device=device)
    engines = integrate.patch_autobackend(be)
    x = inputs["192x160_b2"].to(device)
    y = be.forward(x, augment=True).clone()
    assert torch.equal(y, augs["192x160_b2"](x)) and tuple(y.shape) == (B, 84, 1225)
    y0 = be.forward(x).clone()
    eng = Engine(model, B, (192, 160), device)
    assert torch.equal(y0, eng(x)) and tuple(y0.shape) == (B, 84, 630)
    eng.close()
    assert sorted(engines, key=len) == [(B, 192, 160), (B, 192, 160, "augment")]
    assert be.forward(x, augment=True) is engines[(B, 192, 160, "augment")].pred  # cached, not rebuilt
    with pytest.raises(NotImplementedError):
        be.forward(x, visualize=True)
    with pytest.raises(NotImplementedError):
        be.forward(x, embed=[1])
    with pytest.raises(NotImplementedError):
        be.forward(x, augment=True, embed=[1])
