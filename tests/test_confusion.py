"""The confusion matrix, host side: the counting rule (tests/confusion_ref.py) against the reference's own
ConfusionMatrix.process_batch results (golden/confusion.npz, make_golden_confusion.py), metrics.ConfusionMatrix against
the reference's tp_fp and normalisation, the C-ABI mirror of the two new symbols and the public surface.  No GPU."""

from __future__ import annotations

import ctypes as C
import inspect
import re

import numpy as np
import pytest

import confusion_ref
import val_ref
from conftest import GOLDEN, ROOT, _Npz
from fce_yolo_amd import _native as N
from fce_yolo_amd import metrics as MT

CASES = ["dense", "many_gt", "batch_mixed", "conf_edge", "near_thr", "contested", "max_det_big", "nc80", "nc1"]


@pytest.fixture(scope="module")
def cm_fx():
    return _Npz(GOLDEN / "confusion.npz")


def _ref(fx, **kw):
    return confusion_ref.confusion(fx["dets"], fx["counts"], fx["gt_boxes"], fx["gt_cls"], fx["gt_off"], int(fx["nc"]), **kw)


@pytest.mark.parametrize("name", CASES)
def test_counting_rule_equals_the_reference_in_every_cell(name, cm_fx):
    fx = cm_fx.group(name)
    nc = int(fx["nc"])
    want = fx["matrix"]
    assert want.shape == (nc + 1, nc + 1) and want.dtype == np.int64 and want[nc, nc] == 0
    got = _ref(fx, conf=confusion_ref.confusion_conf(0.001))  # the fixture was made with the validation default
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    if name == "conf_edge":
        at50 = _ref(fx, conf=confusion_ref.confusion_conf(0.5))
        assert np.array_equal(at50, fx["matrix_conf50"]) and not np.array_equal(at50, want)
    if name == "near_thr":
        for b, m in enumerate(fx["per_image"]):
            one = {**fx, "dets": fx["dets"][b:b + 1], "counts": fx["counts"][b:b + 1], "gt_off": fx["gt_off"][b:b + 2]}
            assert np.array_equal(_ref(one), m), b


def test_fixture_cases_cover_what_they_are_for(cm_fx):
    from fce_yolo_amd import val as V

    assert cm_fx.names() == sorted(CASES)
    for name in ("dense", "many_gt", "max_det_big", "nc80"):  # diagonal, off-diagonal, FP column and FN row
        fx = cm_fx.group(name)
        m, nc = fx["matrix"], int(fx["nc"])
        inner = m[:nc, :nc]
        assert np.trace(inner) > 0 and inner.sum() > np.trace(inner) and m[:nc, nc].sum() > 0 and m[nc, :nc].sum() > 0, name
    assert cm_fx.group("dense")["counts"].tolist() == [300] and len(cm_fx.group("dense")["gt_boxes"]) == 60
    many = cm_fx.group("many_gt")
    assert len(many["gt_boxes"]) == 2 * V.GT_CHUNK + 37
    part = many["dets"][0][many["dets"][0, :, 4] > 0.25]
    iou = val_ref.box_iou(many["gt_boxes"], part[:, :4])
    claimed = iou.argmax(0)[iou.max(0) > np.float32(0.45)]
    assert (claimed < V.GT_CHUNK).any() and (claimed // V.GT_CHUNK == 1).any() and (claimed >= 2 * V.GT_CHUNK).any()
    mixed = cm_fx.group("batch_mixed")
    assert mixed["counts"].tolist() == [0, 7, 300, 1] and np.diff(mixed["gt_off"]).tolist() == [5, 0, 40, 1]
    assert (mixed["dets"][1, :7, 4] > 0.25).all() and (mixed["dets"][0, :, 4] == 1).all()  # padding: conf 1
    big = cm_fx.group("max_det_big")
    assert big["dets"].shape[1] == 1000 and big["counts"].tolist() == [900] and V.DET_LDS < 900
    assert (big["dets"][0, V.DET_LDS:900, 4] > 0.25).any()
    edge = cm_fx.group("conf_edge")["dets"][0, :6, 4]
    q, h = np.float32(0.25), np.float32(0.5)
    assert {q, np.nextafter(q, np.float32(1)), h, np.nextafter(h, np.float32(1))} <= set(edge.tolist())
    near = cm_fx.group("near_thr")
    hits = [int(np.trace(p[:3, :3])) for p in near["per_image"]]
    assert min(hits) == 0 and max(hits) == 10 and near["dets"].shape[:2] == (17, 10)
    for j in range(10):  # detection j of image s sits s - 8 float steps from its GT's crossing of 0.45
        x2 = near["dets"][:, j, 2]
        assert all(np.nextafter(x2[s], np.float32(1e9)) == x2[s + 1] for s in range(16))
    con = cm_fx.group("contested")["matrix"]
    assert con[0, 0] == 1 and con[0, 3] == 3 and con[3, 1] == 2 and con[0, 2] == 1 and con.sum() == 7
    assert cm_fx.group("nc80")["matrix"].shape == (81, 81) and cm_fx.group("nc1")["matrix"].shape == (2, 2)


def test_rule_ties_go_to_the_higher_index():
    """The two spots the reference leaves to numpy's sort, as DESIGN.md states them."""
    box = np.array([[10, 10, 50, 50]], np.float32)
    det = np.array([[10, 10, 50, 50, 0.9, 1]], np.float32)
    m = np.zeros((4, 4), np.int64)  # one detection, two identical GT of classes 0 and 2: the higher GT index
    confusion_ref.confusion_image(m, det, np.repeat(box, 2, 0), np.array([0, 2], np.float32), 3)
    assert m[1, 2] == 1 and m[3, 0] == 1 and m.sum() == 2
    m = np.zeros((4, 4), np.int64)  # one GT, two identical detections of classes 0 and 1: the higher detection index
    confusion_ref.confusion_image(m, np.concatenate([det * [1, 1, 1, 1, 1, 0], det]), box, np.array([2], np.float32), 3)
    assert m[1, 2] == 1 and m[0, 3] == 1 and m.sum() == 2


# ---------------------------------------------------------------- metrics.ConfusionMatrix
def test_confusion_matrix_tp_fp_and_normalized_against_the_reference(cm_fx):
    fx = cm_fx.group("dense")
    cm = MT.ConfusionMatrix({i: f"c{i}" for i in range(3)}, fx["matrix"])
    assert cm.nc == 3 and cm.matrix.dtype == np.float64 and cm.matrix.shape == (4, 4)
    tp, fp = cm.tp_fp()
    assert tp.shape == fp.shape == (3,) and np.array_equal(tp, fx["tp"]) and np.array_equal(fp, fx["fp"])
    norm = cm.normalized()
    assert norm.shape == (4, 4) and np.array_equal(norm, fx["normalized"])
    assert np.allclose(norm.sum(0), 1.0)  # every column of `dense` has counts
    empty = MT.ConfusionMatrix({0: "a", 1: "b"})
    assert empty.matrix.shape == (3, 3) and not empty.matrix.any() and not empty.normalized().any()
    with pytest.raises(ValueError):
        MT.ConfusionMatrix({0: "a"}, np.zeros((3, 3)))


# ---------------------------------------------------------------- C-ABI and surface
def test_ctypes_signatures_agree_with_the_header():
    header = (ROOT / "include" / "fce_yolo.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kinds = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    for sym in ("fce_val_confusion_workspace_bytes", "fce_val_confusion"):
        m = re.search(rf"(\w+)\s+{sym}\s*\((.*?)\)\s*;", header, re.S)
        assert m, sym
        res, args = N._SIGS[sym]
        assert res is kinds[m.group(1)]
        params = [a.strip() for a in m.group(2).split(",")]
        assert len(params) == len(args), (sym, params)
        for a, ct in zip(params, args):
            want = C.c_void_p if "*" in a else kinds[a.split()[0]]
            assert ct is want, (sym, a)
        assert sym in N.EXPORTED
    full = (ROOT / "include" / "fce_yolo.h").read_text()
    assert re.search(r"fce_val_confusion\s+utils/metrics\.py:441-518", full)  # the reference lines it replaces
    L = N.lib()
    assert hasattr(L, "fce_val_confusion") and hasattr(L, "fce_val_confusion_workspace_bytes")
    assert L.fce_abi_version() == 7
    assert L.fce_val_confusion_workspace_bytes(32, 300) == 16  # the error word alone: the state stays in LDS
    assert L.fce_val_confusion_workspace_bytes(2, 1000) == 16 + 2 * 1000 * 8
    assert L.fce_val_confusion_workspace_bytes(0, 300) == 0 and L.fce_val_confusion_workspace_bytes(2, 0) == 0


def test_host_entry_rejects_malformed_arguments_without_a_device():
    """The argument checks come before any HIP call: they answer on a machine without a GPU too."""
    L = N.lib()
    buf = (C.c_int32 * 64)()
    p = C.cast(buf, C.c_void_p)

    def status(nc=3, n=1, max_det=8, conf=0.25, iou=0.45, ws=p, ws_bytes=16, matrix=p, dets=p):
        return L.fce_val_confusion(dets, p, n, max_det, p, p, p, nc, conf, iou, ws, ws_bytes, matrix, None)

    for kw, word in ((dict(nc=0), "nc"), (dict(nc=-1), "nc"), (dict(matrix=None), "null"), (dict(dets=None), "null"),
                     (dict(ws_bytes=15), "workspace"), (dict(ws=None), "workspace"), (dict(n=0), "n / max_det"),
                     (dict(max_det=0), "n / max_det"), (dict(conf=float("nan")), "conf"), (dict(iou=1.5), "iou_thres")):
        assert status(**kw) == 1, kw  # FCE_ERR_INVALID
        assert word in L.fce_last_error().decode(), (kw, L.fce_last_error())
    assert not any(buf)


def test_public_surface():
    import fce_yolo_amd
    from fce_yolo_amd import val as V

    assert fce_yolo_amd.ConfusionMatrix is MT.ConfusionMatrix and "ConfusionMatrix" in fce_yolo_amd.__all__
    assert "Validator" in fce_yolo_amd.__all__ and "AugmentedEngine" in fce_yolo_amd.__all__
    p = inspect.signature(V.Validator.__init__).parameters
    assert list(p) == ["self", "model", "batch", "imgsz", "device", "conf", "iou", "max_det", "lanes", "graph",
                       "single_cls", "agnostic_nms"]
    q = inspect.signature(V.DeviceConfusionMatrix.__init__).parameters
    assert list(q) == ["self", "nc", "batch", "max_det", "device", "conf", "iou_thres"]
    assert q["conf"].default == 0.25 and q["iou_thres"].default == 0.45
    assert list(inspect.signature(V.DeviceConfusionMatrix.__call__).parameters) == ["self", "dets", "counts", "gt_boxes",
                                                                                    "gt_cls", "gt_off", "n"]
    for name in ("zero_", "numpy"):
        assert callable(getattr(V.DeviceConfusionMatrix, name))
    for name in ("tp_fp", "normalized"):
        assert callable(getattr(MT.ConfusionMatrix, name))
    # utils/metrics.py:465: the validation default and None count above 0.25, anything else as given
    assert V.confusion_conf(0.001) == 0.25 and V.confusion_conf(None) == 0.25
    for c in (0.25, 0.5, 0.01, 0.0011, 0.9):
        assert V.confusion_conf(c) == c == confusion_ref.confusion_conf(c)
