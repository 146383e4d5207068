"""The confusion matrix on the device: fce_val_confusion (csrc/val.hip) cell for cell against the reference's own
ConfusionMatrix.process_batch results (golden/confusion.npz), its accumulation, argument checks and graph capture, and
`Validator` end to end against the same counting done on the host (tests/confusion_ref.py) from the same engine's NMS
outputs."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import confusion_ref
import tta_ref
from conftest import GOLDEN, _Npz
from fce_yolo_amd import _native as N
from fce_yolo_amd import metrics as MT
from fce_yolo_amd import val as V
from test_gpu_val import NIMG, B, S, _batches, _labels, _nms_outputs

pytestmark = pytest.mark.gpu

CASES = ["dense", "many_gt", "batch_mixed", "conf_edge", "near_thr", "contested", "max_det_big", "nc80", "nc1"]
KEYS = ("dets", "counts", "gt_boxes", "gt_cls", "gt_off")


@pytest.fixture(scope="module")
def cm_fx():
    return _Npz(GOLDEN / "confusion.npz")


def _inputs(fx, device):
    return [torch.from_numpy(np.ascontiguousarray(fx[k])).to(device) for k in KEYS]


def _widened(fx, max_det):
    """The same case with `max_det` rows per image: the new rows repeat row 0 with conf 1 (beyond counts: unread)."""
    d = fx["dets"]
    pad = np.repeat(d[:, :1], max_det - d.shape[1], 1).copy()
    pad[..., 4] = 1
    return {**fx, "dets": np.concatenate([d, pad], 1)}


def _device_matrix(fx, device, conf=0.25, n=None):
    batch, max_det = fx["dets"].shape[:2]
    cm = V.DeviceConfusionMatrix(int(fx["nc"]), batch, max_det, device, conf=conf)
    out = cm(*_inputs(fx, device), n=n)
    assert out is cm.matrix and out.dtype == torch.int32
    return cm.numpy()


# ---------------------------------------------------------------- 1. the kernel against the reference
@pytest.mark.parametrize("name", CASES)
def test_val_confusion_equals_the_reference_in_every_cell(name, cm_fx, device):
    fx = cm_fx.group(name)
    want = fx["matrix"]
    got = _device_matrix(fx, device, conf=V.confusion_conf(0.001))
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5].tolist())
    if name == "conf_edge":
        assert np.array_equal(_device_matrix(fx, device, conf=V.confusion_conf(0.5)), fx["matrix_conf50"])
    if name == "near_thr":  # image by image: a miscount in one image is not made up for by another
        for b in (0, 7, 8, 16):
            assert np.array_equal(_device_matrix(fx, device, n=b + 1) - (_device_matrix(fx, device, n=b) if b else 0),
                                  fx["per_image"][b]), b


@pytest.mark.parametrize("name", ["dense", "many_gt", "batch_mixed", "contested", "nc80"])
def test_val_confusion_workspace_path_equals_the_lds_path(name, cm_fx, device):
    fx = cm_fx.group(name)
    assert fx["dets"].shape[1] <= V.DET_LDS  # the golden run above kept the state in LDS
    wide = _widened(fx, 1000)
    assert N.lib().fce_val_confusion_workspace_bytes(*wide["dets"].shape[:2]) == 16 + wide["dets"].shape[0] * 8000
    assert np.array_equal(_device_matrix(wide, device), fx["matrix"])


def test_val_confusion_accumulates_and_zero_clears(cm_fx, device):
    a, b = cm_fx.group("dense"), cm_fx.group("many_gt")
    cm = V.DeviceConfusionMatrix(3, 1, 300, device)
    cm(*_inputs(a, device))
    cm(*_inputs(b, device))
    assert np.array_equal(cm.numpy(), a["matrix"] + b["matrix"])
    cm(*_inputs(a, device))
    assert np.array_equal(cm.numpy(), 2 * a["matrix"] + b["matrix"])
    cm.zero_()
    assert not cm.numpy().any()
    cm(*_inputs(b, device))
    assert np.array_equal(cm.numpy(), b["matrix"])


def test_val_confusion_counts_only_the_first_n_images(cm_fx, device):
    fx = cm_fx.group("batch_mixed")
    full = fx["matrix"]
    for n in (1, 2, 3):
        want = confusion_ref.confusion(*(fx[k] for k in KEYS), 3, n=n)
        got = _device_matrix(fx, device, n=n)
        assert np.array_equal(got, want) and not np.array_equal(got, full), n
    near = cm_fx.group("near_thr")
    assert np.array_equal(_device_matrix(near, device, n=5), near["per_image"][:5].sum(0))
    cm = V.DeviceConfusionMatrix(3, 4, 300, device)
    for n in (0, 5, -1):
        with pytest.raises(ValueError):
            cm(*_inputs(fx, device), n=n)


@pytest.mark.parametrize("name", ["batch_mixed", "max_det_big"])
def test_device_confusion_matrix_graph_capture_and_replay(name, cm_fx, device):
    fx = cm_fx.group(name)
    batch, max_det = fx["dets"].shape[:2]
    args = _inputs(fx, device)
    eager = V.DeviceConfusionMatrix(3, batch, max_det, device)
    eager(*args)
    eager(*args)
    cm = V.DeviceConfusionMatrix(3, batch, max_det, device)
    cm(*args)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cm(*args)
    g.replay()
    got = cm.numpy()
    assert np.array_equal(got, eager.numpy()) and np.array_equal(got, 2 * fx["matrix"])


GUARD = 64


def test_val_confusion_argument_errors_launch_nothing(cm_fx, device):
    fx = cm_fx.group("max_det_big")
    dets, counts, gtb, gtc, off = _inputs(fx, device)
    n, max_det = fx["dets"].shape[:2]
    nb = N.lib().fce_val_confusion_workspace_bytes(n, max_det)
    assert nb == 16 + n * max_det * 8
    ws = torch.zeros(nb, dtype=torch.uint8, device=device)
    buf = torch.full((16 + 2 * GUARD,), 7, dtype=torch.int32, device=device)
    matrix = buf[GUARD:GUARD + 16]
    matrix.zero_()

    def call(nc=3, ws_bytes=nb, conf=0.25, **null):
        p = dict(dets=dets.data_ptr(), counts=counts.data_ptr(), gtb=gtb.data_ptr(), gtc=gtc.data_ptr(),
                 off=off.data_ptr(), ws=ws.data_ptr(), matrix=matrix.data_ptr())
        p.update(null)
        N.call("fce_val_confusion", p["dets"], p["counts"], n, max_det, p["gtb"], p["gtc"], p["off"], nc, conf, 0.45,
               p["ws"], ws_bytes, p["matrix"], None)

    for nc in (0, -3):
        with pytest.raises(N.FceError, match="nc"):
            call(nc=nc)
    for name in ("dets", "counts", "gtb", "gtc", "off", "matrix"):
        with pytest.raises(N.FceError, match="null"):
            call(**{name: None})
    with pytest.raises(N.FceError, match="workspace"):
        call(ws_bytes=nb - 1)
    with pytest.raises(N.FceError, match="workspace"):
        call(ws=None)
    with pytest.raises(N.FceError, match="conf"):
        call(conf=float("nan"))
    torch.cuda.synchronize()
    assert not matrix.any() and not ws.any()
    call()  # and the same arguments, complete, run
    torch.cuda.synchronize()
    assert np.array_equal(matrix.cpu().numpy().reshape(4, 4), fx["matrix"])
    assert (buf[:GUARD] == 7).all() and (buf[GUARD + 16:] == 7).all()


@pytest.mark.parametrize("max_det", [300, 1000])
def test_val_confusion_class_out_of_range_is_an_error_and_never_an_index(max_det, cm_fx, device):
    """The classes are device data: the host entry cannot see them without a synchronisation.  The kernel counts a
    class outside 0..nc-1 in the workspace's error word and nowhere else, and DeviceConfusionMatrix.numpy() raises."""
    fx = _widened(cm_fx.group("dense"), max_det) if max_det > 300 else cm_fx.group("dense")
    nc = 3
    part = np.nonzero(fx["dets"][0, :300, 4] > 0.25)[0]
    for what, rows, bad in (("gt", np.array([0, 17, 59]), [3.0, -1.0, np.nan]), ("gt", np.array([5]), [1e9]),
                            ("det", part[[0, 3, -1]], [3.0, -1.0, np.inf]), ("det", part[[1]], [-2e9])):
        f = {k: v.copy() for k, v in fx.items()}
        if what == "gt":
            f["gt_cls"][rows] = bad
        else:
            f["dets"][0, rows, 5] = bad
        args = _inputs(f, device)
        cm = V.DeviceConfusionMatrix(nc, 1, max_det, device)
        buf = torch.full(((nc + 1) ** 2 + 2 * GUARD,), 7, dtype=torch.int32, device=device)
        cm.matrix = buf[GUARD:GUARD + (nc + 1) ** 2].view(nc + 1, nc + 1)
        cm.matrix.zero_()
        cm(*args)
        with pytest.raises(N.FceError, match="outside"):
            cm.numpy()
        assert int(cm.ws[:4].view(torch.int32).item()) == len(rows), (what, bad)
        assert (buf[:GUARD] == 7).all() and (buf[GUARD + (nc + 1) ** 2:] == 7).all()
        got = cm.matrix.cpu().numpy()
        assert (got >= 0).all() and got.sum() == fx["matrix"].sum() - len(rows), (what, bad)  # those entries alone
        cm.zero_()
        cm(*_inputs(fx, device))
        assert np.array_equal(cm.numpy(), fx["matrix"])  # zero_ clears the error word too
    # -0.5 and 2.9 truncate to 0 and 2, as .int() does: in range
    f = {k: v.copy() for k, v in fx.items()}
    zero, two = f["gt_cls"] == 0, f["gt_cls"] == 2
    f["gt_cls"][zero], f["gt_cls"][two] = -0.5, 2.9
    assert np.array_equal(_device_matrix(f, device), fx["matrix"])


# ---------------------------------------------------------------- 2. Validator end to end
def _labelled(plain, rng):
    """Per image (normalised xywh (m, 4), cls (m,)): boxes jittered from the image's own confident detections, a third
    of them under another class, and six random boxes nothing detects."""
    labels_n = []
    for d in plain:
        conf = d[d[:, 4] > 0.25]
        _, uniq = np.unique(conf[:, :4], axis=0, return_index=True)
        m = min(12, len(uniq))
        assert m >= 4
        pick = rng.choice(np.sort(uniq), m, replace=False)
        wh = np.concatenate([conf[pick, 2:4] - conf[pick, 0:2]] * 2, 1)
        jit = conf[pick, :4] + rng.uniform(-1, 1, (m, 4)) * wh * np.geomspace(0.002, 0.08, m)[:, None]
        w, h = rng.uniform(10, 80, 6), rng.uniform(10, 80, 6)
        x1, y1 = rng.uniform(0, S - w), rng.uniform(0, S - h)
        xyxy = np.concatenate([jit, np.stack([x1, y1, x1 + w, y1 + h], 1)]) / S
        xywh = np.concatenate([(xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]], 1).astype(np.float32)
        cls = conf[pick, 5].copy()
        cls[::3] = (cls[::3] + 1 + rng.integers(0, 79, len(cls[::3]))) % 80
        labels_n.append((xywh, np.concatenate([cls, rng.integers(0, 80, 6)]).astype(np.float32)))
    return labels_n


def _host_matrix(dets, labels, nc, single_cls=False):
    m = np.zeros((nc + 1, nc + 1), np.int64)
    for d, (gb, gc) in zip(dets, labels):
        d = d.copy()
        if single_cls:
            d[:, 5] = 0
        confusion_ref.confusion_image(m, d, gb, gc, nc)
    return m


def _run(v, batches, device):
    for b in batches:
        v.update({**b, "img": b["img"].to(device)})
    v.flush()
    assert not v.confusion_matrix.matrix.any()  # flush() leaves the device tables alone: nothing is read yet
    stats = {k: list(x) for k, x in v.metrics.stats.items()}
    results = v.stats()
    first = v.confusion_matrix
    again = v.stats()  # no update() in between: an empty run
    assert again == results and not v.confusion_matrix.matrix.any() and v.confusion_matrix is not first
    return stats, results, first


@pytest.fixture(scope="module")
def e2e(device):
    model = tta_ref.model_zero_cls_bias(0).to(device)
    canvases = torch.randint(0, 256, (NIMG, 3, S, S), dtype=torch.uint8, generator=torch.Generator().manual_seed(77))
    with V.Validator(model, B, S, device, lanes=2) as v:
        assert len(v.confusion) == len(v.slots) and all(c.conf == 0.25 and c.nc == 80 for c in v.confusion)
        plain = _nms_outputs(v.engine, canvases, device)
        batches = _batches(canvases, _labelled(plain, np.random.default_rng(8)))
        assert [len(b["img"]) for b in batches] == [2, 2, 1]  # two full batches and a short one
        stats, results, cm = _run(v, batches, device)
    return dict(model=model, canvases=canvases, plain=plain, batches=batches, stats=stats, results=results, cm=cm)


def test_validator_confusion_matrix_equals_host_counting(e2e):
    cm = e2e["cm"]
    assert isinstance(cm, MT.ConfusionMatrix) and cm.nc == 80 and cm.matrix.shape == (81, 81)
    assert cm.matrix.dtype == np.float64
    want = _host_matrix(e2e["plain"], _labels(e2e["batches"]), 80)
    inner = want[:80, :80]
    print("matched", int(inner.sum()), "on the diagonal", int(np.trace(inner)), "FP", int(want[:80, 80].sum()), "FN",
          int(want[80, :80].sum()))
    assert np.trace(inner) > 0 and inner.sum() > np.trace(inner) and want[:80, 80].sum() > 0 and want[80, :80].sum() > 0
    assert np.array_equal(cm.matrix, want), np.argwhere(cm.matrix != want)[:5].tolist()
    # every GT is counted once, and the short batch's repeated canvas not at all
    assert want[:, :80].sum() == sum(len(gc) for _, gc in _labels(e2e["batches"]))
    tp, fp = cm.tp_fp()
    assert tp.sum() == np.trace(inner) and fp.sum() == want[:80].sum() - np.trace(inner)


def test_validator_result_dict_is_what_the_metrics_give_on_the_same_stats(e2e):
    dm = MT.DetMetrics()
    for i in range(NIMG):
        dm.update_stats({k: e2e["stats"][k][i] for k in dm.stats})
    tp, conf, pred_cls, target_cls = (np.concatenate(e2e["stats"][k]) for k in ("tp", "conf", "pred_cls", "target_cls"))
    p, r, _, ap, _ = MT.ap_per_class(tp, conf, pred_cls, target_cls)
    want = dict(zip(MT.KEYS, (p.mean(), r.mean(), ap[:, 0].mean(), ap.mean())))
    want["fitness"] = want["metrics/mAP50-95(B)"]
    got = e2e["results"]
    assert list(got) == list(want)
    for k in got:
        print(f"{k}: {got[k]!r} metrics {want[k]!r}")
        assert abs(got[k] - want[k]) <= 1e-9, k
    dm.process()
    assert dm.results_dict == got and got["metrics/mAP50(B)"] > 0


def test_validator_one_lane_equals_two(e2e, device):
    with V.Validator(e2e["model"], B, S, device, lanes=1) as v1:
        _, results, cm = _run(v1, e2e["batches"], device)
    assert results == e2e["results"]
    assert np.array_equal(cm.matrix, e2e["cm"].matrix)


def test_validator_single_cls_counts_in_class_zero_and_the_background(e2e, device):
    batches = [{**b, "cls": torch.zeros_like(b["cls"])} for b in e2e["batches"]]  # such a dataset's classes are all 0
    with V.Validator(e2e["model"], B, S, device, lanes=2, single_cls=True) as v:
        dets = _nms_outputs(v.engine, e2e["canvases"], device, agnostic=True)
        _, _, cm = _run(v, batches, device)
    m = cm.matrix
    assert not m[1:80].any() and not m[:, 1:80].any()
    assert m[0, 0] > 0 and m[0, 80] > 0 and m[80, 0] > 0 and m[80, 80] == 0
    assert np.array_equal(m, _host_matrix(dets, _labels(batches), 80, single_cls=True))


def test_validator_conf_follows_the_references_rule_and_bad_labels_raise(e2e, device):
    with V.Validator(e2e["model"], B, S, device, lanes=1, conf=0.5) as v:
        assert all(c.conf == 0.5 and c.iou_thres == 0.45 for c in v.confusion)
        b = e2e["batches"][0]
        with pytest.raises(ValueError, match="cls"):
            v.update({**b, "cls": torch.full_like(b["cls"], 80.0)})
        assert v.seen == 0 and not v._fifo
