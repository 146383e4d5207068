"""Validation on the device: fce_val_match (csrc/val.hip) bit for bit against the reference's own match_predictions
results (golden/val.npz), its argument checks and graph capture, and `Validator` end to end against the same matching
and metrics done on the host (tests/val_ref.py + metrics.py) from the same engine's NMS outputs."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import tta_ref
import val_ref
from conftest import GOLDEN, _Npz
from fce_yolo_amd import _native as N
from fce_yolo_amd import metrics as MT
from fce_yolo_amd import val as V
from fce_yolo_amd.engine import Pipeline

pytestmark = pytest.mark.gpu

CASES = ["dense", "many_gt", "batch_mixed", "wrong_class", "near_thr", "max_det_big"]


@pytest.fixture(scope="module")
def val_fx():
    return _Npz(GOLDEN / "val.npz")


def _inputs(fx, device):
    return [torch.from_numpy(fx[k]).to(device) for k in ("dets", "counts", "gt_boxes", "gt_cls", "gt_off")]


def _match(fx, device, niou=10, out=None):
    n, max_det = fx["dets"].shape[:2]
    m = V.DeviceMatcher(n, max_det, device, niou=niou)
    tp = m(*_inputs(fx, device), out=out)
    torch.cuda.synchronize()
    return tp.cpu().numpy().view(np.uint16).reshape(n, max_det)


# ---------------------------------------------------------------- 1. the kernel against the reference
@pytest.mark.parametrize("name", CASES)
def test_val_match_bitwise_against_the_reference(name, val_fx, device):
    fx = val_fx.group(name)
    want = val_ref.words(fx["tp"])
    got = _match(fx, device)
    bad = got != want
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    for b, k in enumerate(fx["counts"]):
        assert (got[b, k:] == 0).all()
    assert V.unpack_tp(got[0, :fx["counts"][0]]).shape == (fx["counts"][0], 10)
    # one threshold: bit 0 of the ten-threshold result
    one = _match(fx, device, niou=1)
    assert np.array_equal(one, want & 1)


@pytest.mark.parametrize("name", ["batch_mixed", "max_det_big"])
def test_val_match_overwrites_a_dirty_buffer_and_repeats(name, val_fx, device):
    fx = val_fx.group(name)
    n, max_det = fx["dets"].shape[:2]
    want = val_ref.words(fx["tp"])
    out = torch.full((n, max_det), -1, dtype=torch.int16, device=device)
    first = _match(fx, device, out=out).copy()
    out.fill_(0x5555)
    second = _match(fx, device, out=out)
    assert np.array_equal(first, want) and np.array_equal(second, want)


def test_val_match_argument_errors_launch_nothing(val_fx, device):
    fx = val_fx.group("max_det_big")
    dets, counts, gtb, gtc, off = _inputs(fx, device)
    n, max_det = fx["dets"].shape[:2]
    iouv = (C.c_float * 16)(*V.iou_vector().tolist(), *([0.0] * 6))
    nb = N.lib().fce_val_match_workspace_bytes(n, max_det, len(fx["gt_boxes"]), 10)
    assert nb == n * max_det * 8
    ws = torch.zeros(nb, dtype=torch.uint8, device=device)
    out = torch.full((n, max_det), -1, dtype=torch.int16, device=device)

    def call(niou=10, ws_bytes=nb, **null):
        p = dict(dets=dets.data_ptr(), counts=counts.data_ptr(), gtb=gtb.data_ptr(), gtc=gtc.data_ptr(),
                 off=off.data_ptr(), iouv=C.cast(iouv, C.c_void_p), ws=ws.data_ptr(), tp=out.data_ptr())
        p.update(null)
        N.call("fce_val_match", p["dets"], p["counts"], n, max_det, p["gtb"], p["gtc"], p["off"], p["iouv"], niou,
               p["ws"], ws_bytes, p["tp"], None)

    for niou in (0, 17, -1):
        with pytest.raises(N.FceError, match="niou"):
            call(niou=niou)
    for name in ("dets", "counts", "gtb", "gtc", "off", "iouv", "tp"):
        with pytest.raises(N.FceError, match="null"):
            call(**{name: None})
    with pytest.raises(N.FceError, match="workspace"):
        call(ws_bytes=nb - 1)
    with pytest.raises(N.FceError, match="workspace"):
        call(ws=None)
    torch.cuda.synchronize()
    assert (out == -1).all()
    call()  # and the same arguments, complete, run
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), val_ref.words(fx["tp"]))


@pytest.mark.parametrize("name", ["batch_mixed", "max_det_big"])
def test_device_matcher_graph_capture_and_replay(name, val_fx, device):
    fx = val_fx.group(name)
    n, max_det = fx["dets"].shape[:2]
    args = _inputs(fx, device)
    m = V.DeviceMatcher(n, max_det, device)
    tp = m(*args)
    assert tp.dtype == torch.uint16 and tuple(tp.shape) == (n, max_det)
    torch.cuda.synchronize()
    eager = tp.cpu().numpy().copy()
    out = torch.full((n, max_det), -1, dtype=torch.int16, device=device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m(*args, out=out)
    for _ in range(2):
        out.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint16), eager)
    assert np.array_equal(eager, val_ref.words(fx["tp"]))


# ---------------------------------------------------------------- 2. Validator end to end
B, S, NIMG = 2, 192, 5  # three batches, the last one short
NMS_KW = dict(conf=0.001, iou=0.7, max_det=300, multi_label=True)


def _nms_outputs(engine, canvases, device, agnostic=False):
    """The engine's Pipeline NMS outputs per image for the batches of `canvases` (a short batch repeats its last
    canvas): [(k, 6) numpy]."""
    outs = []
    with Pipeline(engine, lanes=1, defer=False, agnostic=agnostic, **NMS_KW) as pipe:
        for i in range(0, len(canvases), B):
            x = canvases[i:i + B]
            n = len(x)
            if n < B:
                x = torch.cat([x, x[-1:].expand(B - n, -1, -1, -1)])
            k = pipe.submit(x.to(device).contiguous())
            dets, _ = pipe.results(k)
            outs += [d.cpu().numpy() for d in dets[:n]]
    return outs


def _host_stats(dets, labels, single_cls=False):
    """val_ref + metrics on the host: DetMetrics with every image's statistics."""
    dm = MT.DetMetrics()
    for d, (gb, gc) in zip(dets, labels):
        d = d.copy()
        if single_cls:
            d[:, 5] = 0
        dm.update_stats({"tp": val_ref.match_image(d[:, :4], d[:, 5], gb, gc), "conf": d[:, 4], "pred_cls": d[:, 5],
                         "target_cls": gc, "target_img": np.unique(gc)})
    return dm


def _batches(canvases, labels_n):
    """The reference collate's dicts (host tensors): img, batch_idx, cls (M, 1), bboxes normalised xywh, the labels
    of a batch in shuffled order."""
    rng = np.random.default_rng(5)
    out = []
    for i in range(0, NIMG, B):
        rows = [(j - i, c, *b) for j in range(i, min(i + B, NIMG)) for b, c in zip(*labels_n[j])]
        rows = np.array(rows, np.float32).reshape(-1, 6)[rng.permutation(len(rows))]
        out.append({"img": canvases[i:i + B], "batch_idx": torch.from_numpy(rows[:, 0].copy()),
                    "cls": torch.from_numpy(rows[:, 1:2].copy()), "bboxes": torch.from_numpy(rows[:, 2:].copy())})
    return out


def _labels(batches):
    """Per image (gt_boxes canvas xyxy, gt_cls) exactly as the Validator packs them."""
    out = []
    for b in batches:
        n = len(b["img"])
        gb, gc, off = V.pack_gt(b["batch_idx"], b["cls"], b["bboxes"], n, S, S)
        gb, gc, off = gb.numpy(), gc.numpy(), off.tolist()
        out += [(gb[off[i]:off[i + 1]], gc[off[i]:off[i + 1]]) for i in range(n)]
    return out


def _feed(v, batches, device_of):
    for bi, b in enumerate(batches):
        v.update({**b, "img": b["img"].to(device_of(bi))})
    v.flush()
    stats = {k: list(x) for k, x in v.metrics.stats.items()}
    return stats, v.stats()


@pytest.fixture(scope="module")
def e2e(device):
    """Model, canvases, labels built from a first plain run's detections, and a Validator (lanes=2) run over them
    with device-resident and host images alternating and the last batch short."""
    model = tta_ref.model_zero_cls_bias(0).to(device)
    canvases = torch.randint(0, 256, (NIMG, 3, S, S), dtype=torch.uint8, generator=torch.Generator().manual_seed(77))
    v = V.Validator(model, B, S, device, lanes=2)
    plain = _nms_outputs(v.engine, canvases, device)
    rng = np.random.default_rng(6)
    labels_n = []  # per image: (normalised xywh (m, 4) fp32, cls (m,) fp32)
    for d in plain:
        assert len(d) >= 20
        _, uniq = np.unique(d[:, :4], axis=0, return_index=True)  # multi_label repeats a box once per class
        m = min(12, len(uniq))
        assert m >= 4
        pick = rng.choice(np.sort(uniq), m, replace=False)
        wh = np.concatenate([d[pick, 2:4] - d[pick, 0:2]] * 2, 1)
        jit = d[pick, :4] + rng.uniform(-1, 1, (m, 4)) * wh * np.geomspace(0.002, 0.08, m)[:, None]
        w, h = rng.uniform(10, 80, 6), rng.uniform(10, 80, 6)
        x1, y1 = rng.uniform(0, S - w), rng.uniform(0, S - h)
        xyxy = np.concatenate([jit, np.stack([x1, y1, x1 + w, y1 + h], 1)]) / S
        xywh = np.concatenate([(xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]], 1).astype(np.float32)
        cls = np.concatenate([d[pick, 5], rng.integers(0, 80, 6)]).astype(np.float32)
        labels_n.append((xywh, cls))
    batches = _batches(canvases, labels_n)
    assert [len(b["img"]) for b in batches] == [2, 2, 1]
    stats, results = _feed(v, batches, lambda bi: device if bi % 2 == 0 else "cpu")
    assert v.seen == NIMG and all(len(x) == 0 for x in v.metrics.stats.values())
    v.close()
    return dict(model=model, canvases=canvases, plain=plain, batches=batches, stats=stats, results=results)


def _assert_same_stats(got: dict, want: dict):
    for k in ("tp", "conf", "pred_cls", "target_cls", "target_img"):
        assert len(got[k]) == len(want[k]) == NIMG, k
        for a, b in zip(got[k], want[k]):
            assert a.dtype == b.dtype and np.array_equal(a, b), k


def _assert_same_results(got: dict, want: dict):
    assert list(got) == list(want)
    for k in got:
        print(f"{k}: {got[k]!r} host {want[k]!r}")
        assert abs(got[k] - want[k]) <= 1e-9, k


def test_validator_equals_host_matching_and_metrics(e2e):
    dm = _host_stats(e2e["plain"], _labels(e2e["batches"]))
    tp = np.concatenate(dm.stats["tp"])
    print("true positives per threshold", tp.sum(0).tolist(), "of", len(tp))
    assert tp[:, 0].any() and tp[:, 5].any()  # thresholds 0.5 and 0.75: the comparison is not vacuous
    _assert_same_stats(e2e["stats"], dm.stats)
    dm.process()
    _assert_same_results(e2e["results"], dm.results_dict)
    assert e2e["results"]["metrics/mAP50(B)"] > 0


def test_validator_one_lane_equals_two(e2e, device):
    with V.Validator(e2e["model"], B, S, device, lanes=1) as v1:
        stats, results = _feed(v1, e2e["batches"], lambda bi: device)
    _assert_same_stats(stats, e2e["stats"])
    assert results == e2e["results"]


def test_validator_single_cls_zeroes_the_predicted_classes(e2e, device):
    batches = [{**b, "cls": torch.zeros_like(b["cls"])} for b in e2e["batches"]]  # such a dataset's classes are all 0
    with V.Validator(e2e["model"], B, S, device, lanes=2, single_cls=True) as v:
        dets = _nms_outputs(v.engine, e2e["canvases"], device, agnostic=True)
        dm = _host_stats(dets, _labels(batches), single_cls=True)
        assert np.concatenate(dm.stats["tp"])[:, 0].any()
        stats, results = _feed(v, batches, lambda bi: device)
    assert all((p == 0).all() for p in stats["pred_cls"])
    _assert_same_stats(stats, dm.stats)
    dm.process()
    _assert_same_results(results, dm.results_dict)
