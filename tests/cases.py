"""Shared test-case table: per-op golden fixtures -> (drop-in module, oracle function)."""

from __future__ import annotations

import torch

import fce_pkg

fce_pkg.load()
from fce_yolo_amd import modules as M  # noqa: E402
from fce_yolo_amd.weights import seeded_state_dict  # noqa: E402
from oracle import fce_oracle as O  # noqa: E402

# name: (module class, ctor args, oracle fn(sd, "m", x, args) or None, args for oracle)
OPS = {
    "bicoord_n": (M.BiCoordCrossAtt, (128, 128, 8, 4), O.bicoordcrossatt),
    "bicoord_l_dh16": (M.BiCoordCrossAtt, (512, 512, 8, 4), O.bicoordcrossatt),
    "bicoord_h8": (M.BiCoordCrossAtt, (512, 512, 8, 8), O.bicoordcrossatt),
    "bicoord_oup": (M.BiCoordCrossAtt, (64, 96, 8, 2), O.bicoordcrossatt),
    "bicoord_dh2": (M.BiCoordCrossAtt, (32, 32, 32, 4), O.bicoordcrossatt),
    "bifpn_2": (M.BiFPN_Concat, ([64, 32], 32), O.bifpn_concat),
    "bifpn_3": (M.BiFPN_Concat, ([16, 32, 32], 16), O.bifpn_concat),
    "bifpn_id": (M.BiFPN_Concat, ([32, 32], 32), O.bifpn_concat),
    "bifpn_negw": (M.BiFPN_Concat, ([24, 48, 24], 24), O.bifpn_concat),
    "coordatt_same": (M.CoordAtt, (64, 64, 16), O.coordatt),
    "coordatt_oup": (M.CoordAtt, (32, 48, 4), O.coordatt),
    "coordcross": (M.CoordCrossAtt, (64, 64, 4, 2), O.coordcrossatt),
    "coordcross_h1": (M.CoordCrossAtt, (32, 32, 8, 1), O.coordcrossatt),
    "conv_k1": (M.Conv, (24, 40, 1, 1), lambda sd, p, x, a: O.conv(sd, p, x, 1)),
    "conv_k3s1": (M.Conv, (16, 32, 3, 1), lambda sd, p, x, a: O.conv(sd, p, x, 1)),
    "conv_k3s2": (M.Conv, (16, 24, 3, 2), lambda sd, p, x, a: O.conv(sd, p, x, 2)),
    "conv_c3": (M.Conv, (3, 16, 3, 2), lambda sd, p, x, a: O.conv(sd, p, x, 2)),
    "dwconv": (M.DWConv, (32, 32, 3), lambda sd, p, x, a: O.dwconv(sd, p, x)),
    "sppf": (M.SPPF, (64, 64, 5), lambda sd, p, x, a: O.sppf(sd, p, x, 5)),
    "c2psa": (M.C2PSA, (256, 256, 1), lambda sd, p, x, a: O.c2psa(sd, p, x, list(a))),
    "c3k2_b": (M.C3k2, (32, 64, 1, False, 0.25), lambda sd, p, x, a: O.c3k2(sd, p, x, list(a))),
    "c3k2_c3k": (M.C3k2, (64, 64, 2, True), lambda sd, p, x, a: O.c3k2(sd, p, x, list(a))),
}


def build_op(name, fx):
    """Drop-in module with the fixture's weights (seeded, or stored for the modified case)."""
    cls, args, _ = OPS[name]
    mod = cls(*args)
    sd = mod.state_dict()
    if any(k.startswith("sd::") for k in fx):
        new = {k[4:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("sd::")}
    else:
        new = seeded_state_dict([(k, v.shape) for k, v in sd.items()], int(fx["seed"]))
    mod.load_state_dict(new)
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps = 1e-3
    return mod.eval()


def op_inputs(fx):
    ins = [torch.from_numpy(fx[k]) for k in sorted(k for k in fx if k.startswith("in"))]
    return ins


def oracle_op(name, mod, inputs, dtype=torch.float64):
    """Run the oracle restatement of op `name` on the module's weights."""
    _, args, fn = OPS[name]
    sd = {"m." + k: v for k, v in mod.state_dict().items()}
    sd = O.cast_sd(O.fuse_state_dict(sd), dtype)
    xs = [x.to(dtype) for x in inputs]
    a = list(args)
    if name.startswith("c2psa") or name.startswith("c3k2"):
        a = list(args) if len(args) > 2 else [args[0], args[1], 1]
    x = xs if len(xs) > 1 else xs[0]
    with torch.no_grad():
        return fn(sd, "m", x, a)


def build_detect(fx):
    det = M.Detect(80, (64, 128, 256))
    det.stride = torch.tensor([8.0, 16.0, 32.0])
    sd = det.state_dict()
    det.load_state_dict(seeded_state_dict([(k, v.shape) for k, v in sd.items()], int(fx["seed"])))
    for m in det.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps = 1e-3
    return det.eval()


def seeded_model(cfg_name, seed=0, mutate=None):
    from fce_yolo_amd.parser import DetectionModel, load_cfg

    d = load_cfg(cfg_name)
    if mutate:
        mutate(d)
    model = DetectionModel(d)
    sd = model.state_dict()
    model.load_state_dict(seeded_state_dict([(k, v.shape) for k, v in sd.items()], seed))
    return model.eval()


def heads8(d):
    for row in d["backbone"]:
        if row[2] == "BiCoordCrossAtt":
            row[3] = [512, 8, 8]


E2E = {
    # fixture key: (cfg, mutate)
    "yolo11n-fce_160_b2": ("yolo11n-fce.yaml", None),
    "yolo11n-fce_320_b1": ("yolo11n-fce.yaml", None),
    "yolo11s-bifpn_160_b2": ("yolo11s-bifpn.yaml", None),
    "yolo11m-fce-h8_128_b1": ("yolo11m-fce.yaml", heads8),
    "yolo11l-fce_128_b1": ("yolo11l-fce.yaml", None),
    "yolo11n_160_b1": ("yolo11n.yaml", None),
}


def e2e_input(key, fx):
    s, b = key.split("_")[-2:]
    s, b = int(s), int(b[1:])
    x = torch.rand(b, 3, s, s, generator=torch.Generator().manual_seed(int(fx["x_seed"])))
    return x


def oracle_model(model, x, dtype=torch.float64):
    from oracle.parse import parse

    layers, save, _ = parse(model.yaml)
    sd = O.cast_sd(O.fuse_state_dict(model.state_dict()), dtype)
    with torch.no_grad():
        return O.forward(layers, save, {"model." + k[len("model."):] if k.startswith("model.") else k: v
                                        for k, v in sd.items()}, x.to(dtype))


# ---------------------------------------------------------------- BASELINE-size fixtures (golden/full.npz)
FULL = {
    # fixture key: (cfg, mutate, batch, imgsz) -- make_golden_full.E2E_FULL
    "yolo11n-fce_640_b2": ("yolo11n-fce.yaml", None, 2, 640),
    "yolo11s-bifpn_640_b1": ("yolo11s-bifpn.yaml", None, 1, 640),
    "yolo11l-fce_640_b1": ("yolo11l-fce.yaml", None, 1, 640),
    "yolo11m-fce-h8_1280_b1": ("yolo11m-fce.yaml", heads8, 1, 1280),
}
OPS_FULL = {
    # fixture key: (module class, ctor args, input shape) -- make_golden_full.OPS_FULL
    "bicoord_n_80": (M.BiCoordCrossAtt, (128, 128, 8, 4), (2, 128, 80, 80)),
    "bicoord_l_80": (M.BiCoordCrossAtt, (512, 512, 8, 4), (1, 512, 80, 80)),
    "bicoord_m_160": (M.BiCoordCrossAtt, (512, 512, 8, 8), (1, 512, 160, 160)),
    "c2psa_m_40": (M.C2PSA, (512, 512, 1), (1, 512, 40, 40)),
    "c2psa_n_20": (M.C2PSA, (256, 256, 1), (2, 256, 20, 20)),
}


def full_input(key, fx):
    _, _, b, s = FULL[key]
    return torch.rand(b, 3, s, s, generator=torch.Generator().manual_seed(int(fx["x_seed"])))


def full_op(key, fx):
    """(module with the fixture's seeded weights, input) of a BASELINE-size per-op fixture."""
    cls, args, shape = OPS_FULL[key]
    mod = cls(*args)
    mod.load_state_dict(seeded_state_dict([(k, v.shape) for k, v in mod.state_dict().items()], int(fx["seed"])))
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps = 1e-3
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(int(fx["x_seed"])))
    return mod.eval(), x


def full_op_oracle(key, mod, x, dtype=torch.float32):
    cls, args, _ = OPS_FULL[key]
    sd = O.cast_sd(O.fuse_state_dict({"m." + k: v for k, v in mod.state_dict().items()}), dtype)
    with torch.no_grad():
        if cls is M.C2PSA:
            return O.c2psa(sd, "m", x.to(dtype), list(args))
        return O.bicoordcrossatt(sd, "m", x.to(dtype), list(args))


def op_slice(y):
    """make_golden_full.op_slice."""
    return y[:, ::3, ::5, ::7]


def compare_full(y, fx, anchors=True):
    """Errors of a full output against a BASELINE-size fixture: (slice error, row-sum error), both relative
    to max|ref slice| (row sums: relative to the row's sum of |values| bound A * max|ref|)."""
    y = y.double().cpu()
    ref = torch.from_numpy(fx["slice"]).double()
    ys = y[:, :, ::37] if anchors else op_slice(y)
    scale = ref.abs().max().clamp_min(1e-12)
    e_slice = ((ys - ref).abs().max() / scale).item()
    sums = y.sum(dim=2) if anchors else y.sum(dim=(2, 3))
    n = y.shape[2] if anchors else y.shape[2] * y.shape[3]
    e_sum = ((sums - torch.from_numpy(fx["sum"])).abs().max() / (scale * n)).item()
    return e_slice, e_sum


# ---------------------------------------------------------------- margin-designed end-to-end NMS (golden/e2e_nms.npz)
E2E_NMS = {
    # fixture key: (cfg, batch, imgsz) -- make_golden_e2e_nms.CASES
    "yolo11n-fce_256_b2": ("yolo11n-fce.yaml", 2, 256),
    "yolo11s-bifpn_256_b2": ("yolo11s-bifpn.yaml", 2, 256),
}


E2E_NMS640 = {
    # fixture key: (cfg, batch, imgsz) -- make_golden_e2e_nms640.CASES (per-image input seeds)
    "yolo11n-fce_640_b32": ("yolo11n-fce.yaml", 32, 640),
    "yolo11s-bifpn_640_b4": ("yolo11s-bifpn.yaml", 4, 640),
}


E2E_NMS_ML = {
    # fixture key: (cfg, -h8 BiCoordCrossAtt heads, batch, imgsz) -- make_golden_e2e_nms_ml.CASES: n with designed
    # classes on all three Detect levels; l-fce 640 (the per-rank shard scale of the 8-GPU l256 config) and m-fce-h8
    # 1280 (config 4) on the P3 and P4 levels
    "yolo11n-fce_640_b8_3lvl": ("yolo11n-fce.yaml", False, 8, 640),
    "yolo11l-fce_640_b2": ("yolo11l-fce.yaml", False, 2, 640),
    "yolo11m-fce-h8_1280_b2": ("yolo11m-fce.yaml", True, 2, 1280),
}


def designed_model_ml(key, fx):
    """(model, input) of an all-levels margin-designed case (make_golden_e2e_nms_ml.py)."""
    import re

    from fce_yolo_amd.parser import DetectionModel, load_cfg

    cfg, h8, b, s = E2E_NMS_ML[key]
    d = load_cfg(cfg)
    if h8:
        for row in d["backbone"]:
            if row[2] == "BiCoordCrossAtt":
                row[3] = [512, 8, 8]
    model = DetectionModel(d)
    sd = seeded_state_dict([(k, v.shape) for k, v in model.state_dict().items()], 0, gain=float(fx["gain"]))
    det = len(model.model) - 1
    n = 0
    for k in sd:
        m = re.match(rf"^model\.{det}\.cv3\.(\d+)\.2\.(weight|bias)$", k)
        if m:
            sd[k] = torch.from_numpy(fx[f"cls_{m.group(2)[0]}{m.group(1)}"].copy())
            n += 1
    assert n == 6, n
    model.load_state_dict(sd)
    seeds = [int(v) for v in fx["seeds"]]
    assert len(seeds) == b
    x = torch.cat([torch.rand(1, 3, s, s, generator=torch.Generator().manual_seed(v)) for v in seeds])
    return model.eval(), x


def designed_model640(key, fx):
    """(model, input) of a headline-size margin-designed case (make_golden_e2e_nms640.py): the designed Detect cls
    convs on seeded_state_dict(keys, 0, gain), and the batch of per-image seeded inputs."""
    import re

    from fce_yolo_amd.parser import DetectionModel, load_cfg

    cfg, b, s = E2E_NMS640[key]
    model = DetectionModel(load_cfg(cfg))
    sd = seeded_state_dict([(k, v.shape) for k, v in model.state_dict().items()], 0, gain=float(fx["gain"]))
    det = len(model.model) - 1
    n = 0
    for k in sd:
        m = re.match(rf"^model\.{det}\.cv3\.(\d+)\.2\.(weight|bias)$", k)
        if m:
            sd[k] = torch.from_numpy(fx[f"cls_{m.group(2)[0]}{m.group(1)}"].copy())
            n += 1
    assert n == 6, n
    model.load_state_dict(sd)
    seeds = [int(v) for v in fx["seeds"]]
    assert len(seeds) == b
    x = torch.cat([torch.rand(1, 3, s, s, generator=torch.Generator().manual_seed(v)) for v in seeds])
    return model.eval(), x


def designed_model(key, fx):
    """(model, input) of a margin-designed end-to-end NMS case: seeded_state_dict(keys, 0, gain) with the
    Detect cls head's last 1x1 convs replaced by the fixture's designed weights (make_golden_e2e_nms.py)."""
    import re

    from fce_yolo_amd.parser import DetectionModel, load_cfg

    cfg, b, s = E2E_NMS[key]
    model = DetectionModel(load_cfg(cfg))
    sd = seeded_state_dict([(k, v.shape) for k, v in model.state_dict().items()], 0, gain=float(fx["gain"]))
    det = len(model.model) - 1
    n = 0
    for k in sd:
        m = re.match(rf"^model\.{det}\.cv3\.(\d+)\.2\.(weight|bias)$", k)
        if m:
            sd[k] = torch.from_numpy(fx[f"cls_{m.group(2)[0]}{m.group(1)}"].copy())
            n += 1
    assert n == 6, n
    model.load_state_dict(sd)
    x = torch.rand(b, 3, s, s, generator=torch.Generator().manual_seed(int(fx["x_seed"])))
    return model.eval(), x


# ---------------------------------------------------------------- coordinate-attention path cases (test_gpu_paths.py)
COORD_CLS = {"Bi": M.BiCoordCrossAtt, "Att": M.CoordAtt, "Cross": M.CoordCrossAtt}


def build_coord(kind, args, seed):
    """One of the three coordinate-attention drop-ins with seeded weights, as build_op makes them (BN eps 1e-3)."""
    mod = COORD_CLS[kind](*args)
    mod.load_state_dict(seeded_state_dict([(k, v.shape) for k, v in mod.state_dict().items()], seed))
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps = 1e-3
    return mod.eval()


def sharpened_input(shape, seed):
    """randn fp16 input whose last row, last column and rows 15 / 16 (where they exist) are 4 x larger: a pooled
    mean that drops or double-counts one of them moves by far more than its rounding."""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    h, w = shape[2:]
    for r in sorted({h - 1, 15, 16}):
        if 0 <= r < h:
            x[:, :, r] *= 4
    x[:, :, :, w - 1] *= 4
    return x.half()


def _axial(q, k, v, scale):
    return ((q @ k) * scale).softmax(-1) @ v


def coord_gates(kind, sd, p, x, args):
    """oracle.fce_oracle's bicoordcrossatt / coordatt / coordcrossatt restated to also return what the kernels keep in
    their workspace: (x_h [N,C,H], x_w [N,C,W], g1 [N,oup,H], g2 [N,oup,W] or None, out).  g1 / g2 are the pre-sigmoid
    gate logits of BiCoordCrossAtt, the sigmoid gates a_h / a_w of CoordAtt, and the sigmoid row gate of CoordCrossAtt
    (no g2).  Same operations in the same order as the oracle, so `out` equals the oracle's output bit for bit
    (test_gate_oracle_is_the_oracle)."""
    n, c, h, w = x.shape
    x_h = x.mean(3, keepdim=True)
    if kind == "Bi":
        inp, oup, reduction, heads = args
        dh = max(8, inp // reduction) // heads
        mid, scale = dh * heads, dh**-0.5
        x_w = x.mean(2, keepdim=True)
        q_h = O.conv2d(sd, p + ".proj_q_h", x_h).view(n, heads, dh, h).permute(0, 1, 3, 2)
        k_h = O.conv2d(sd, p + ".proj_k_h", x_w).view(n, heads, dh, w)
        v_h = O.conv2d(sd, p + ".proj_v_h", x_w).view(n, heads, dh, w).permute(0, 1, 3, 2)
        g1 = O.conv2d(sd, p + ".out_h", _axial(q_h, k_h, v_h, scale).permute(0, 1, 3, 2).reshape(n, mid, h, 1))
        q_w = O.conv2d(sd, p + ".proj_q_w", x_w).view(n, heads, dh, w).permute(0, 1, 3, 2)
        k_w = O.conv2d(sd, p + ".proj_k_w", x_h).view(n, heads, dh, h)
        v_w = O.conv2d(sd, p + ".proj_v_w", x_h).view(n, heads, dh, h).permute(0, 1, 3, 2)
        g2 = O.conv2d(sd, p + ".out_w", _axial(q_w, k_w, v_w, scale).permute(0, 1, 3, 2).reshape(n, mid, 1, w))
        ident = O.conv2d(sd, p + ".identity", x) if inp != oup else x
        return x_h[..., 0], x_w[:, :, 0], g1[..., 0], g2[:, :, 0], ident * torch.sigmoid(g1 + g2)
    x_w = x.mean(2, keepdim=True).permute(0, 1, 3, 2)
    if kind == "Att":
        inp, oup, _ = args
        y = O.conv(sd, p + ".cv1", torch.cat([x_h, x_w], dim=2))
        y_h, y_w = torch.split(y, [h, w], dim=2)
        a_h = O.conv2d(sd, p + ".cv_h", y_h).sigmoid()
        a_w = O.conv2d(sd, p + ".cv_w", y_w.permute(0, 1, 3, 2)).sigmoid()
        ident = O.conv2d(sd, p + ".identity", x) if inp != oup else x
        return x_h[..., 0], x_w[..., 0], a_h[..., 0], a_w[:, :, 0], ident * a_h * a_w
    inp, oup, reduction, heads = args
    mip = max(8, inp // reduction)
    scale = (mip // heads) ** -0.5
    y = O.conv2d(sd, p + ".cv1", torch.cat([x_h, x_w], dim=2))
    y_h, y_w = torch.split(y, [h, w], dim=2)
    q = O.conv2d(sd, p + ".q_conv", y_h).view(n, heads, -1, h).permute(0, 1, 3, 2)
    k = O.conv2d(sd, p + ".k_conv", y_w).view(n, heads, -1, w)
    v = O.conv2d(sd, p + ".v_conv", y_w).view(n, heads, -1, w).permute(0, 1, 3, 2)
    z = _axial(q, k, v, scale).permute(0, 1, 3, 2).contiguous().view(n, mip, h, 1)
    g1 = O.conv2d(sd, p + ".proj", z).sigmoid()
    return x_h[..., 0], x_w[..., 0], g1[..., 0], None, x * g1


def coord_oracle(kind, args, mod, x, dtype=torch.float64):
    """coord_gates on the module's weights (BN folded as the oracle folds it) in `dtype`."""
    sd = O.cast_sd(O.fuse_state_dict({"m." + k: v.cpu() for k, v in mod.state_dict().items()}), dtype)
    with torch.no_grad():
        return coord_gates(kind, sd, "m", x.cpu().to(dtype), list(args))
