"""Test-time augmentation, host side: geometry, clip ranges, the CPU restatements of the two kernels against the
reference's own results (golden/tta.npz, make_golden_tta.py), and the public surface.  No GPU."""

from __future__ import annotations

import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import tta_ref
from conftest import GOLDEN, ROOT, _Npz
from fce_yolo_amd import _native as N
from fce_yolo_amd import tta

E2E = {"192_b2": ((192, 192), [(0, 720), (0, 525), (400, 125)]),
       "192x160_b2": ((192, 160), [(0, 600), (0, 525), (320, 100)])}


@pytest.fixture(scope="module")
def tta_fx():
    return _Npz(GOLDEN / "tta.npz")


def test_constants_are_the_references():
    assert tta.SCALES == (1, 0.83, 0.67) and tta.FLIPS == (None, 3, None) and tta.PAD_VALUE == 0.447


def test_scale_geometry_equals_every_recorded_reference_shape(tta_fx):
    table = tta_fx.z["geom/table"]
    assert len(table) == 11 * 11 * 2
    for h, w, r100, h_s, w_s, h_c, w_c in table.tolist():
        assert tta.scale_geometry(h, w, r100 / 100, 32) == (h_s, w_s, h_c, w_c), (h, w, r100)
    assert tta.scale_geometry(640, 480, 1, 32) == (640, 480, 640, 480)


def _anchors(h, w):
    return sum((h // s) * (w // s) for s in (8, 16, 32))


def test_clip_ranges_640_and_fixture_cases(tta_fx):
    canv = [tta.scale_geometry(640, 640, s, 32)[2:] for s in tta.SCALES]
    assert canv == [(640, 640), (544, 544), (448, 448)]
    assert tta.clip_ranges([_anchors(*c) for c in canv], 3) == [(0, 8000), (0, 6069), (3136, 980)]
    for key, ((H, W), ranges) in E2E.items():
        canv = [tta.scale_geometry(H, W, s, 32)[2:] for s in tta.SCALES]
        assert tta.clip_ranges([_anchors(*c) for c in canv], 3) == ranges
        assert [c for _, c in ranges] == tta_fx.group(f"e2e/{key}")["segments"].tolist()


@pytest.mark.parametrize("name", ["a", "b"])
def test_scale_img_ref_against_the_reference(name, tta_fx):
    """Both are fp32 evaluations of the same convex combination of values in [0, 1]: after the fp16 rounding they
    differ by at most one fp16 spacing below 1, 2^-11.  The pad region and the resized size are exact."""
    fx = tta_fx.group(f"resize/{name}")
    shape = tuple(fx["shape"].tolist())
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(int(fx["seed"]))).half()
    for r in (0.83, 0.67):
        h_s, w_s, H_c, W_c = tta.scale_geometry(shape[2], shape[3], r, 32)
        assert [h_s, w_s] == fx[f"r{round(r * 100)}_size"].tolist()
        for flip in (0, 3, 2):
            ref = torch.from_numpy(fx[f"r{round(r * 100)}_f{flip}"])
            assert tuple(ref.shape) == (*shape[:2], H_c, W_c)
            got = tta_ref.scale_img_ref(x, flip, h_s, w_s, H_c, W_c)
            assert got.dtype == torch.float16
            err = (got.float() - ref).abs().max().item()
            print(f"{name} r{r} flip {flip}: max abs {err:.3e}")
            assert err <= 2.0 ** -11
            mask = torch.ones(H_c, W_c, dtype=torch.bool)
            mask[:h_s, :w_s] = False
            assert mask.any()
            assert torch.equal(got[..., mask], ref[..., mask].half())
            assert (ref[..., mask] == np.float32(0.447)).all()
            # the resized region is not pad: the size is pinned from both sides
            assert (got[:, :, :h_s, :w_s].float() - ref[:, :, :h_s, :w_s]).abs().max().item() <= 2.0 ** -11


def test_scale_img_ref_ratio_one_is_the_converted_copy():
    x = torch.rand(1, 3, 9, 13, generator=torch.Generator().manual_seed(5))
    assert torch.equal(tta_ref.scale_img_ref(x, None, 9, 13, 9, 13), x.half())
    u = (x * 255).to(torch.uint8)
    assert torch.equal(tta_ref.scale_img_ref(u, None, 9, 13, 9, 13), u.half() / 255)


@pytest.mark.parametrize("key", list(E2E))
def test_predict_augment_ref_against_the_reference(key, tta_fx):
    """The fp32 restatement (three oracle forwards, de-scale, un-flip, clip, concatenate) against the reference's
    DetectionModel._predict_augment: pins flips, scales and clip ranges without a GPU."""
    fx = tta_fx.group(f"e2e/{key}")
    model = tta_ref.model_zero_cls_bias(int(tta_fx.z["e2e/model_seed"]))
    shape = tuple(fx["shape"].tolist())
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(int(fx["x_seed"]))).half().float()
    y, ranges = tta_ref.predict_augment_ref(model, x, torch.float32)
    assert ranges == E2E[key][1]
    ref = torch.from_numpy(fx["y_rows"])
    assert np.array_equal(fx["rows"], tta_ref.GOLDEN_KEY_ROWS)
    got = y[:, tta_ref.GOLDEN_KEY_ROWS]
    assert got.shape == ref.shape
    box = ((got[:, :4] - ref[:, :4]).abs().max() / ref[:, :4].abs().max()).item()
    cls = (got[:, 4:] - ref[:, 4:]).abs().max().item()
    print(f"{key}: box rel {box:.2e} cls abs {cls:.2e}")
    assert box <= 1e-5 and cls <= 1e-5, (box, cls)


def test_merge_ref_identity_and_flips():
    g = torch.Generator().manual_seed(3)
    p = torch.rand(2, 9, 11, generator=g) * 100
    k = torch.randint(0, 2 ** 62, (2, 11), generator=g)
    y, b = tta_ref.merge_ref([(p, k, 0, 11, 1, None, 50, 70)])
    assert torch.equal(y, p) and torch.equal(b, k)
    y, b = tta_ref.merge_ref([(p, k, 2, 5, 0.5, 3, 50, 70), (p, k, 1, 3, 1, 2, 50, 70)])
    assert y.shape == (2, 9, 8) and b.shape == (2, 8)
    assert torch.equal(y[:, 0, :5], 70 - p[:, 0, 2:7] / 0.5) and torch.equal(y[:, 1, :5], p[:, 1, 2:7] / 0.5)
    assert torch.equal(y[:, 1, 5:], 50 - p[:, 1, 1:4]) and torch.equal(y[:, 4:, :5], p[:, 4:, 2:7])
    assert torch.equal(b, torch.cat([k[:, 2:7], k[:, 1:4]], 1))


def test_tta_part_mirror_has_the_header_size_and_fields():
    """fce_tta_part: two pointers, three ints, a float, three ints -> 44 bytes padded to 48."""
    assert C.sizeof(N.TtaPart) == 48
    header = (ROOT / "include" / "fce_yolo.h").read_text()
    body = re.search(r"typedef struct fce_tta_part \{(.*?)\} fce_tta_part;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == [f[0] for f in N.TtaPart._fields_]
    assert C.sizeof(N.Tensor) == 8 + 8 * 4  # fce_tensor, the scale kernel's argument
    for sym in ("fce_tta_scale_img", "fce_tta_merge"):
        assert sym in N.EXPORTED and re.search(rf"\b{sym}\s*\(", header)


def test_library_exports_the_tta_symbols_and_keeps_the_abi_version():
    L = N.lib()
    assert hasattr(L, "fce_tta_scale_img") and hasattr(L, "fce_tta_merge")
    assert L.fce_abi_version() == 7


def test_public_surface():
    import fce_yolo_amd
    from fce_yolo_amd.predict import Predictor

    p = inspect.signature(Predictor.__init__).parameters
    assert "augment" in p and p["augment"].default is False
    assert fce_yolo_amd.AugmentedEngine is tta.AugmentedEngine
    sig = inspect.signature(tta.AugmentedEngine.__init__).parameters
    assert list(sig)[:7] == ["self", "model", "batch", "imgsz", "device", "graph", "autotune"]
    for name in ("new_best", "clone", "close", "__call__"):
        assert callable(getattr(tta.AugmentedEngine, name))
