"""Validation, host side: the matching rule (tests/val_ref.py) against the reference's own match_predictions results
(golden/val.npz, make_golden_val.py), metrics.py against the reference's ap_per_class / DetMetrics, the GT packing
against the reference's _prepare_batch, the C-ABI mirror and the public surface.  No GPU."""

from __future__ import annotations

import inspect
import re

import numpy as np
import pytest
import torch

import val_ref
from conftest import GOLDEN, ROOT, _Npz
from fce_yolo_amd import _native as N
from fce_yolo_amd import metrics as MT

CASES = ["dense", "many_gt", "batch_mixed", "wrong_class", "near_thr", "max_det_big"]
RESULT_KEYS = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness"]


@pytest.fixture(scope="module")
def val_fx():
    return _Npz(GOLDEN / "val.npz")


def test_thresholds_are_the_references(val_fx):
    from fce_yolo_amd import val as V

    ref = val_fx.z["iouv"]
    assert ref.dtype == np.float32 and ref.shape == (10,)
    assert np.array_equal(V.iou_vector().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(val_ref.IOUV.view(np.uint32), ref.view(np.uint32))
    assert V.iou_vector(1).tolist() == [0.5]


@pytest.mark.parametrize("name", CASES)
def test_matching_rule_equals_the_reference_in_every_cell(name, val_fx):
    fx = val_fx.group(name)
    got = val_ref.match(fx["dets"], fx["counts"], fx["gt_boxes"], fx["gt_cls"], fx["gt_off"])
    assert got.shape == fx["tp"].shape and fx["tp"].dtype == bool
    assert np.array_equal(got, fx["tp"]), int((got != fx["tp"]).sum())
    if name == "wrong_class":
        assert not fx["tp"].any()
    else:
        assert fx["tp"][..., 0].any() and fx["tp"][..., 9].any()


def test_fixture_cases_cover_what_they_are_for(val_fx):
    from fce_yolo_amd import val as V

    src = (ROOT / "fce-yolo_amd" / "csrc" / "val.hip").read_text()
    assert int(re.search(r"VAL_GT_CHUNK = (\d+);", src).group(1)) == V.GT_CHUNK
    assert int(re.search(r"VAL_DET_LDS = (\d+);", src).group(1)) == V.DET_LDS
    many = val_fx.group("many_gt")
    assert len(many["gt_boxes"]) > 2 * V.GT_CHUNK and len(many["gt_boxes"]) % V.GT_CHUNK != 0
    assert many["counts"].tolist() == [300] and val_fx.group("dense")["counts"].tolist() == [300]
    mixed = val_fx.group("batch_mixed")
    assert mixed["counts"].tolist() == [0, 7, 300, 1] and np.diff(mixed["gt_off"]).tolist() == [5, 0, 40, 1]
    big = val_fx.group("max_det_big")
    assert big["dets"].shape[1] == 1000 and big["counts"].tolist() == [900] and V.DET_LDS < 900
    near = val_fx.group("near_thr")
    assert near["dets"].shape[:2] == (17, 10)
    for j in range(10):  # detection j of image s sits s - 8 float steps from threshold j's crossing
        col = near["tp"][:, j, j]
        assert col.any() and not col.all(), j
        x2 = near["dets"][:, j, 2]
        assert all(np.nextafter(x2[s], np.float32(1e9)) == x2[s + 1] for s in range(16))


def test_words_round_trip():
    from fce_yolo_amd import val as V

    tp = np.random.default_rng(1).random((7, 10)) < 0.5
    w = val_ref.words(tp)
    assert w.dtype == np.uint16 and np.array_equal(V.unpack_tp(w), tp)
    assert np.array_equal(V.unpack_tp(w.view(np.int16)), tp)  # the pinned buffer's int16 view


# ---------------------------------------------------------------- metrics
def test_ap_per_class_against_the_reference(val_fx):
    fx = val_fx.group("ap")
    p, r, f1, ap, cls = MT.ap_per_class(fx["tp"], fx["conf"], fx["pred_cls"], fx["target_cls"])
    assert cls.tolist() == fx["unique_classes"].tolist() == [0, 1, 2, 3, 4]
    assert ap.shape == (5, 10) and (ap[4] == 0).all() and (ap[:4, 0] > 0).all()
    for name, got in (("p", p), ("r", r), ("f1", f1), ("ap", ap)):
        err = np.abs(got - fx[name]).max()
        print(f"{name}: max abs {err:.3e}")
        assert got.shape == fx[name].shape and err <= 1e-9, (name, err)


def test_det_metrics_result_dict_against_the_reference(val_fx):
    fx = val_fx.group("ap")
    assert bytes(fx["result_keys"]).decode().split("\n") == RESULT_KEYS
    dm = MT.DetMetrics(names={i: f"c{i}" for i in range(5)})
    assert dm.results_dict == dict.fromkeys(RESULT_KEYS, 0.0)  # nothing processed yet
    target = fx["target_cls"][fx["target_perm"]]
    for i in range(25):
        sel, t = fx["image_of_det"] == i, target[fx["image_of_target"] == i]
        dm.update_stats({"tp": fx["tp"][sel], "conf": fx["conf"][sel], "pred_cls": fx["pred_cls"][sel], "target_cls": t,
                         "target_img": np.unique(t)})
    stats = dm.process()
    assert len(stats["tp"]) == 400
    rd = dm.results_dict
    assert list(rd) == RESULT_KEYS and dm.keys == RESULT_KEYS[:4]
    for k, want in zip(RESULT_KEYS, fx["result_values"]):
        print(f"{k}: {rd[k]!r} reference {want!r}")
        assert isinstance(rd[k], float) and abs(rd[k] - want) <= 1e-9, k
    assert rd["fitness"] == rd["metrics/mAP50-95(B)"]
    assert dm.nt_per_class.tolist() == fx["nt_per_class"].tolist()
    dm.clear_stats()
    assert all(len(v) == 0 for v in dm.stats.values())
    assert dm.results_dict == rd  # the results outlive the statistics, as get_stats returns them after clearing


def test_metrics_module_does_not_import_torch():
    import subprocess
    import sys

    code = ("import sys, importlib.util as u; s = u.spec_from_file_location('m', sys.argv[1]); m = u.module_from_spec(s); "
            "s.loader.exec_module(m); assert 'torch' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(ROOT / "fce-yolo_amd" / "metrics.py")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ---------------------------------------------------------------- GT packing
def test_pack_gt_against_the_references_prepare_batch(val_fx):
    from fce_yolo_amd import val as V

    co, mixed = val_fx.group("collate"), val_fx.group("batch_mixed")
    H, W = co["imgsz"].tolist()
    bi = co["batch_idx"]
    assert (np.diff(bi) < 0).any()  # unsorted
    boxes, cls, off = V.pack_gt(torch.from_numpy(bi), torch.from_numpy(co["cls"]), torch.from_numpy(co["bboxes"]), 4, H, W)
    assert boxes.dtype == torch.float32 and cls.dtype == torch.float32 and off.dtype == torch.int32
    assert off.tolist() == mixed["gt_off"].tolist()
    assert np.array_equal(boxes.numpy().view(np.uint32), mixed["gt_boxes"].view(np.uint32))
    assert np.array_equal(cls.numpy(), mixed["gt_cls"])
    # (M,) classes and numpy inputs are taken too; a non-square canvas scales x by W and y by H
    b2, c2, o2 = V.pack_gt(bi, co["cls"].reshape(-1), co["bboxes"], 4, H, W)
    assert torch.equal(b2, boxes) and torch.equal(c2, cls) and torch.equal(o2, off)
    b3, _, _ = V.pack_gt([0], [1.0], [[0.5, 0.5, 0.5, 0.25]], 1, 100, 200)
    assert b3.tolist() == [[50.0, 37.5, 150.0, 62.5]]
    e, ec, eo = V.pack_gt(np.zeros(0), np.zeros((0, 1)), np.zeros((0, 4)), 3, H, W)
    assert tuple(e.shape) == (0, 4) and ec.numel() == 0 and eo.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        V.pack_gt([4], [0.0], [[0.5, 0.5, 0.1, 0.1]], 4, H, W)


# ---------------------------------------------------------------- C-ABI and surface
def test_ctypes_signatures_agree_with_the_header():
    import ctypes as C

    header = (ROOT / "include" / "fce_yolo.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kinds = {"int": C.c_int, "size_t": C.c_size_t}
    for sym in ("fce_val_match_workspace_bytes", "fce_val_match"):
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
    L = N.lib()
    assert hasattr(L, "fce_val_match") and hasattr(L, "fce_val_match_workspace_bytes")
    assert L.fce_abi_version() == 7
    assert L.fce_val_match_workspace_bytes(32, 300, 640, 10) == 0  # the default max_det needs no workspace
    assert L.fce_val_match_workspace_bytes(2, 1000, 640, 10) == 2 * 1000 * 8


def test_public_surface():
    import fce_yolo_amd
    from fce_yolo_amd import val as V

    assert fce_yolo_amd.Validator is V.Validator and "Validator" in fce_yolo_amd.__all__
    p = inspect.signature(V.Validator.__init__).parameters
    assert list(p) == ["self", "model", "batch", "imgsz", "device", "conf", "iou", "max_det", "lanes", "graph",
                       "single_cls", "agnostic_nms"]
    defaults = {k: v.default for k, v in p.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(imgsz=640, device=None, conf=0.001, iou=0.7, max_det=300, lanes=None, graph=True,
                            single_cls=False, agnostic_nms=False)
    for name in ("update", "stats", "flush", "close", "__enter__", "__exit__"):
        assert callable(getattr(V.Validator, name))
    q = inspect.signature(V.DeviceMatcher.__init__).parameters
    assert list(q)[:5] == ["self", "batch", "max_det", "device", "niou"] and q["niou"].default == 10
    assert list(inspect.signature(V.DeviceMatcher.__call__).parameters)[:6] == ["self", "dets", "counts", "gt_boxes",
                                                                                 "gt_cls", "gt_off"]
    assert list(MT.DetMetrics().results_dict) == RESULT_KEYS
    for name in ("update_stats", "process", "clear_stats"):
        assert callable(getattr(MT.DetMetrics, name))
