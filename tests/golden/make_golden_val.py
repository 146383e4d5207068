"""Validation fixtures from the REFERENCE (run where the reference is importable).

    python tests/golden/make_golden_val.py

Writes tests/golden/val.npz (data only), three groups:

  * <case>/...  matching cases: the inputs of fce_val_match (`dets` (n, max_det, 6), `counts`, `gt_boxes`, `gt_cls`,
                `gt_off`) and `tp` (n, max_det, 10) bool from the reference's own utils/metrics.py box_iou +
                BaseValidator.match_predictions (engine/validator.py:266-306) with DetectionValidator's `iouv`, through
                DetectionValidator._process_batch per image; rows >= counts are False.  Rows of `dets` beyond
                `counts` hold copies of matching boxes: a kernel that reads them shows.
  * collate/... the labels of `batch_mixed` as the reference collate delivers them (unsorted `batch_idx`, `cls` (M, 1),
                normalised xywh `bboxes`, `imgsz`); that case's gt_boxes are DetectionValidator._prepare_batch's.
  * ap/...      seeded tp / conf / pred_cls / target_cls over 400 detections and 5 classes (class 4 has GT and no
                detection), the reference ap_per_class outputs and the DetMetrics result dict.

The generator asserts the conditions the tests rely on: no detection with a best class-masked IoU >= 0.5 has its two
largest class-masked IoUs equal; every case but `wrong_class` has true cells at thresholds 0.5 and 0.95; in `near_thr`
every threshold has a true and a false detection among its 17.
Same import recipe as make_golden.py.
"""

from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden  # noqa: E402

S = 640  # canvas
GT_CHUNK = 256  # fce_yolo_amd.val.GT_CHUNK (csrc/val.hip VAL_GT_CHUNK)
NC = 3


def rand_boxes(rng, n, lo=24.0, hi=160.0):
    w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    x1, y1 = rng.uniform(0, S - w), rng.uniform(0, S - h)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)


def jitter(rng, boxes, scale):
    """Every coordinate moved by up to `scale` (per row) of the box's size."""
    wh = np.concatenate([boxes[:, 2:] - boxes[:, :2]] * 2, 1)
    return (boxes + rng.uniform(-1, 1, boxes.shape) * wh * np.asarray(scale)[:, None]).astype(np.float32)


def detections(rng, gt, gcls, src, n_random, wrong=False):
    """Detections jittered from GT rows `src` (jitter from 0.2 % to 12 % of the size: IoUs from ~0.99 down to ~0.6)
    plus `n_random` random boxes, confidences distinct, sorted by confidence descending as the NMS leaves them."""
    scale = np.exp(rng.uniform(np.log(0.002), np.log(0.12), len(src)))
    b = jitter(rng, gt[src], scale)
    c = gcls[src].copy()
    if wrong:
        c = (c + 1 + rng.integers(0, NC - 1, len(src))) % NC
    b = np.concatenate([b, rand_boxes(rng, n_random)])
    c = np.concatenate([c, rng.integers(0, NC, n_random).astype(np.float32)])
    conf = (rng.permutation(len(b)) + 1).astype(np.float32) / np.float32(len(b) + 1)
    o = np.argsort(-conf, kind="stable")
    return np.concatenate([b[o], conf[o, None], c[o, None]], 1).astype(np.float32)


def main():
    torch.set_num_threads(8)
    make_golden.import_reference()
    make_golden._load_pkg()
    # ultralytics/models/__init__.py imports every model family (SAM needs torchvision): the three packages above
    # detect/val.py are entered as bare packages, so only that module's own imports run
    import importlib
    import types

    for pkg in ("ultralytics.models", "ultralytics.models.yolo", "ultralytics.models.yolo.detect"):
        m = types.ModuleType(pkg)
        m.__path__ = [str(make_golden.REF / pkg.replace(".", "/"))]
        sys.modules[pkg] = m
    DetectionValidator = importlib.import_module("ultralytics.models.yolo.detect.val").DetectionValidator
    from ultralytics.utils.metrics import DetMetrics, ap_per_class, box_iou

    from fce_yolo_amd import val as V

    assert V.GT_CHUNK == GT_CHUNK
    # BaseValidator.__init__ imports torchvision only to keep its import time out of a timer (validator.py:103): an
    # empty module object stands in for the constructor and is removed again; nothing is called on it
    sys.modules["torchvision"] = types.ModuleType("torchvision")
    try:
        val = DetectionValidator(save_dir=Path(tempfile.mkdtemp(prefix="fceval_")), args=dict(mode="val", plots=False))
    finally:
        del sys.modules["torchvision"]
    val.device = torch.device("cpu")
    iouv = val.iouv
    assert torch.equal(iouv, torch.linspace(0.5, 0.95, 10)) and iouv.dtype == torch.float32
    out = {"iouv": iouv.numpy()}
    rng = np.random.Generator(np.random.PCG64(2024))

    def reference_tp(dets, counts, gt_boxes, gt_cls, gt_off):
        n, max_det = dets.shape[:2]
        tp = np.zeros((n, max_det, 10), bool)
        for b in range(n):
            k, g0, g1 = int(counts[b]), int(gt_off[b]), int(gt_off[b + 1])
            d = torch.from_numpy(dets[b, :k])
            r = val._process_batch({"bboxes": d[:, :4], "cls": d[:, 5]},
                                   {"bboxes": torch.from_numpy(gt_boxes[g0:g1]), "cls": torch.from_numpy(gt_cls[g0:g1])})
            tp[b, :k] = r["tp"]
            if k and g1 > g0:  # the tie-free condition
                iou = (box_iou(torch.from_numpy(gt_boxes[g0:g1]), d[:, :4]) *
                       (torch.from_numpy(gt_cls[g0:g1])[:, None] == d[:, 5])).numpy()
                top = np.sort(iou, 0)[::-1]
                if top.shape[0] > 1:
                    assert not ((top[0] >= 0.5) & (top[0] == top[1])).any(), "tied best IoUs"
        return tp

    def case(name, dets, counts, gt_boxes, gt_cls, gt_off, expect_true=True):
        dets, gt_boxes, gt_cls = dets.astype(np.float32), gt_boxes.astype(np.float32), gt_cls.astype(np.float32)
        counts, gt_off = np.asarray(counts, np.int32), np.asarray(gt_off, np.int32)
        tp = reference_tp(dets, counts, gt_boxes, gt_cls, gt_off)
        if expect_true:
            assert tp[..., 0].any() and tp[..., 9].any(), name
        else:
            assert not tp.any(), name
        for k, v in dict(dets=dets, counts=counts, gt_boxes=gt_boxes, gt_cls=gt_cls, gt_off=gt_off, tp=tp).items():
            out[f"{name}/{k}"] = v
        print(name, "dets", dets.shape, "gt", len(gt_boxes), "true per threshold", tp.sum((0, 1)).tolist(), flush=True)
        return tp

    def padded(d, max_det, fill):
        """(max_det, 6): d, then rows cycling through `fill` (boxes that would match if they were read)."""
        pad = fill[np.arange(max_det - len(d)) % len(fill)] if len(d) < max_det else fill[:0]
        return np.concatenate([d, pad])[None]

    # ------------------------------------------------------------------ dense
    gt, gc = rand_boxes(rng, 60), rng.integers(0, NC, 60).astype(np.float32)
    d = detections(rng, gt, gc, np.repeat(np.arange(60), 4), 60)
    case("dense", d[None], [300], gt, gc, [0, 60])

    # ------------------------------------------------------------------ many_gt: 2 LDS chunks and a remainder
    M = 2 * GT_CHUNK + 37
    gt, gc = rand_boxes(rng, M, 16, 60), rng.integers(0, NC, M).astype(np.float32)
    d = detections(rng, gt, gc, rng.choice(M, 260, replace=False), 40)
    tp = case("many_gt", d[None], [300], gt, gc, [0, M])
    iou = box_iou(torch.from_numpy(gt), torch.from_numpy(d[:, :4])) * (torch.from_numpy(gc)[:, None] == torch.from_numpy(d[:, 5]))
    best = iou.argmax(0).numpy()[tp[0, :, 0]]
    assert (best < GT_CHUNK).any() and ((best >= GT_CHUNK) & (best < 2 * GT_CHUNK)).any() and (best >= 2 * GT_CHUNK).any()

    # ------------------------------------------------------------------ batch_mixed (+ the collate form of its labels)
    ngt, cnt = [5, 0, 40, 1], [0, 7, 300, 1]
    bidx = np.repeat(np.arange(4), ngt)
    xyxy = rand_boxes(rng, sum(ngt)).astype(np.float64) / S
    xywh = np.concatenate([(xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]], 1).astype(np.float32)
    cls = rng.integers(0, NC, (sum(ngt), 1)).astype(np.float32)
    perm = rng.permutation(sum(ngt))  # the collate's order is by image; a caller's may not be
    batch = {"batch_idx": torch.from_numpy(bidx[perm].astype(np.float32)), "cls": torch.from_numpy(cls[perm]),
             "bboxes": torch.from_numpy(xywh[perm]), "img": torch.zeros(4, 3, S, S, dtype=torch.uint8),
             "ori_shape": [(S, S)] * 4, "ratio_pad": [None] * 4, "im_file": [""] * 4}
    pb = [val._prepare_batch(si, batch) for si in range(4)]
    gt = np.concatenate([p["bboxes"].numpy().reshape(-1, 4) for p in pb])
    gc = np.concatenate([p["cls"].numpy().reshape(-1) for p in pb])
    off = np.concatenate([[0], np.cumsum(ngt)])
    for k in ("batch_idx", "cls", "bboxes"):
        out[f"collate/{k}"] = batch[k].numpy()
    out["collate/imgsz"] = np.array([S, S])
    rows = []
    for b in range(4):
        g = slice(off[b], off[b + 1])
        fill = np.concatenate([gt[:5], np.ones((5, 1), np.float32), gc[:5, None]], 1)  # image 0's GT, exactly
        if b == 2:
            db = detections(rng, gt[g], gc[g], np.repeat(np.arange(40), 6), 60)
        elif b == 3:
            db = detections(rng, gt[g], gc[g], np.arange(1), 0)
            db[:, :4] = jitter(rng, gt[g], [0.004])  # one detection, one GT, IoU > 0.95: the single-match path
        else:
            db = rand_boxes(rng, cnt[b])
            db = np.concatenate([db, np.linspace(0.9, 0.1, cnt[b], dtype=np.float32)[:, None],
                                 rng.integers(0, NC, (cnt[b], 1)).astype(np.float32)], 1)
        rows.append(padded(db[:cnt[b]], 300, fill))
    tp = case("batch_mixed", np.concatenate(rows), cnt, gt, gc, off)
    assert tp[3, 0].all() and not tp[0].any() and not tp[1].any()

    # ------------------------------------------------------------------ wrong_class
    gt, gc = rand_boxes(rng, 30), rng.integers(0, NC, 30).astype(np.float32)
    d = detections(rng, gt, gc, np.repeat(np.arange(30), 3), 0, wrong=True)
    assert (box_iou(torch.from_numpy(gt), torch.from_numpy(d[:, :4])).max(0).values > 0.5).all()
    case("wrong_class", padded(d, 96, d[:1]), [90], gt, gc, [0, 30], expect_true=False)

    # ------------------------------------------------------------------ near_thr
    # image s (17 of them) holds, for every threshold t_j, GT j = (0, 50 j, w_j, 50 j + 30) and one detection sharing
    # x1, y1, y2 with it whose x2 is s - 8 float steps from the first x2 at which the reference's IoU reaches t_j
    widths = (37.3 + 11.7 * np.arange(10)).astype(np.float32)
    gt1 = np.stack([np.zeros(10), 50.0 * np.arange(10), widths, 50.0 * np.arange(10) + 30], 1).astype(np.float32)
    cross = []
    for j in range(10):
        t = iouv[j]
        g = torch.from_numpy(gt1[j:j + 1])

        def reached(x2):
            db = g.clone()
            db[0, 2] = float(x2)
            return bool(box_iou(g, db)[0, 0] >= t)

        x2 = np.float32(np.float64(t) * np.float64(widths[j]))
        while reached(x2):
            x2 = np.nextafter(x2, np.float32(0))
        while not reached(x2):
            x2 = np.nextafter(x2, np.float32(S))
        cross.append(x2)  # the first x2 with IoU >= t_j
    dets = np.zeros((17, 10, 6), np.float32)
    for s in range(17):
        for j in range(10):
            x2 = cross[j]
            for _ in range(abs(s - 8)):
                x2 = np.nextafter(x2, np.float32(S if s > 8 else 0))
            dets[s, j] = [0, gt1[j, 1], x2, gt1[j, 3], 0.9 - 0.01 * j, j % NC]
    gc1 = (np.arange(10) % NC).astype(np.float32)
    tp = case("near_thr", dets, [10] * 17, np.tile(gt1, (17, 1)), np.tile(gc1, 17), np.arange(18) * 10)
    for j in range(10):
        col = tp[:, j, j]
        assert col.any() and not col.all(), (j, col)
        print('near_thr threshold', j, 'true at steps', np.nonzero(col)[0].tolist(), flush=True)

    # ------------------------------------------------------------------ max_det_big: beyond the LDS-resident state
    assert V.DET_LDS < 900
    gt, gc = rand_boxes(rng, 150), rng.integers(0, NC, 150).astype(np.float32)
    d = detections(rng, gt, gc, np.repeat(np.arange(150), 5), 150)
    fill = np.concatenate([gt[:8], np.ones((8, 1), np.float32), gc[:8, None]], 1)
    case("max_det_big", padded(d, 1000, fill), [900], gt, gc, [0, 150])

    # ------------------------------------------------------------------ ap
    D = 400
    pred_cls = rng.integers(0, 4, D).astype(np.float32)
    conf = (rng.permutation(D) + 1).astype(np.float32) / np.float32(D + 1)
    level = rng.integers(0, 14, D)  # thresholds passed: 0 (a false positive) .. 10
    tp = np.arange(10)[None, :] < np.clip(level - 3, 0, 10)[:, None]
    target_cls = np.concatenate([np.full(c, k, np.float32) for k, c in enumerate([70, 55, 90, 40, 12])])
    res = ap_per_class(tp, conf, pred_cls, target_cls)
    for k, v in zip(("tp_count", "fp_count", "p", "r", "f1", "ap", "unique_classes"), res[:7]):
        out[f"ap/{k}"] = np.asarray(v)
    assert res[6].tolist() == [0, 1, 2, 3, 4] and (res[5][4] == 0).all() and (res[5][:4, 0] > 0).all()
    dm = DetMetrics(names={i: f"c{i}" for i in range(5)})
    imgs = np.sort(rng.integers(0, 25, D))  # 25 images, the detections and targets dealt over them
    timg = np.sort(rng.integers(0, 25, len(target_cls)))
    tperm = rng.permutation(len(target_cls))
    for i in range(25):
        sel, t = imgs == i, target_cls[tperm][timg == i]
        dm.update_stats({"tp": tp[sel], "conf": conf[sel], "pred_cls": pred_cls[sel], "target_cls": t,
                         "target_img": np.unique(t)})
    stats = dm.process()
    rd = dm.results_dict
    out["ap/image_of_det"], out["ap/image_of_target"], out["ap/target_perm"] = imgs, timg, tperm
    for k in ("tp", "conf", "pred_cls", "target_cls"):
        out[f"ap/{k}"] = dict(tp=tp, conf=conf, pred_cls=pred_cls, target_cls=target_cls)[k]
    out["ap/result_keys"] = np.frombuffer("\n".join(rd).encode(), np.uint8)
    out["ap/result_values"] = np.array(list(rd.values()), np.float64)
    out["ap/nt_per_class"] = dm.nt_per_class
    assert len(stats["tp"]) == D
    print("ap", rd, flush=True)

    np.savez_compressed(HERE / "val.npz", **out)
    print("val.npz", (HERE / "val.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
