"""Confusion-matrix fixtures from the REFERENCE (run where the reference is importable).

    python tests/golden/make_golden_confusion.py

Writes tests/golden/confusion.npz (data only).  Every case <name>/... holds the inputs of fce_val_confusion (`dets`
(n, max_det, 6), `counts`, `gt_boxes`, `gt_cls`, `gt_off`, `nc`) and `matrix` (nc + 1, nc + 1) int64: the reference's own
ConfusionMatrix.process_batch (utils/metrics.py:441-518) called per image with conf=0.001, the validation default, which
it replaces by 0.25.  `conf_edge` also holds `matrix_conf50` (conf=0.5), `near_thr` the matrices image by image
(`per_image`), `dense` the reference's tp_fp() and its plot's column normalisation.  Rows of `dets` beyond `counts`
hold copies of matching boxes with conf 1: a kernel that reads them shows.

The generator asserts the conditions the tests rely on: among the pairs with IoU > 0.45 of the participating
detections no two of one detection and no two of one GT have equal IoU (the reference's undefined spots), and every
case's matrix has the cells its description names.
Same import recipe as make_golden_val.py.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden  # noqa: E402
from make_golden_val import GT_CHUNK, S, jitter, rand_boxes  # noqa: E402

NC = 3
VAL_CONF = 0.001  # cfg/default.yaml's validation conf, what DetectionValidator passes: counted above 0.25
IOU_THRES = 0.45


def detections(rng, gt, gcls, src, n_random, nc=NC, wrong=1 / 3):
    """Detections jittered from GT rows `src` (0.2 % to 12 % of the size: IoUs from ~0.99 down to ~0.6), a fraction
    `wrong` of them with another class, plus `n_random` random boxes; confidences distinct, sorted descending."""
    scale = np.exp(rng.uniform(np.log(0.002), np.log(0.12), len(src)))
    b = jitter(rng, gt[src], scale)
    c = gcls[src].copy()
    if nc > 1:
        w = rng.random(len(src)) < wrong
        c[w] = (c[w] + 1 + rng.integers(0, nc - 1, int(w.sum()))) % nc
    b = np.concatenate([b, rand_boxes(rng, n_random)])
    c = np.concatenate([c, rng.integers(0, nc, n_random).astype(np.float32)])
    conf = (rng.permutation(len(b)) + 1).astype(np.float32) / np.float32(len(b) + 1)
    o = np.argsort(-conf, kind="stable")
    return np.concatenate([b[o], conf[o, None], c[o, None]], 1).astype(np.float32)


def main():
    torch.set_num_threads(8)
    make_golden.import_reference()
    make_golden._load_pkg()
    from ultralytics.utils.metrics import ConfusionMatrix, box_iou

    from fce_yolo_amd import val as V

    assert V.GT_CHUNK == GT_CHUNK
    out = {}
    rng = np.random.Generator(np.random.PCG64(2025))

    def reference(dets, counts, gt_boxes, gt_cls, gt_off, nc, conf=VAL_CONF):
        """(summed matrix, per-image matrices) of the reference; asserts the tie-free condition."""
        per = []
        thr = 0.25 if conf in {None, 0.001} else conf
        for b in range(len(counts)):
            k, g0, g1 = int(counts[b]), int(gt_off[b]), int(gt_off[b + 1])
            d = torch.from_numpy(dets[b, :k])
            g, gc = torch.from_numpy(gt_boxes[g0:g1]), torch.from_numpy(gt_cls[g0:g1])
            cm = ConfusionMatrix(names={i: f"c{i}" for i in range(nc)})
            cm.process_batch({"bboxes": d[:, :4], "conf": d[:, 4], "cls": d[:, 5]}, {"bboxes": g, "cls": gc}, conf=conf)
            per.append(cm.matrix.copy())
            part = d[d[:, 4] > thr]
            if len(part) and g1 > g0:
                iou = box_iou(g, part[:, :4]).numpy()
                cand = np.where(iou > IOU_THRES, iou, -np.arange(iou.size, dtype=np.float32).reshape(iou.shape) - 1)
                for axis in (0, 1):
                    v = np.sort(cand, axis)
                    a, c = np.swapaxes(v, 0, axis)[1:], np.swapaxes(v, 0, axis)[:-1]
                    assert not ((a == c) & (a > 0)).any(), "tied candidate IoUs"
        per = np.stack(per)
        assert (per == np.round(per)).all()
        return per.sum(0).astype(np.int64), per.astype(np.int64)

    def case(name, dets, counts, gt_boxes, gt_cls, gt_off, nc=NC):
        dets, gt_boxes, gt_cls = dets.astype(np.float32), gt_boxes.astype(np.float32), gt_cls.astype(np.float32)
        counts, gt_off = np.asarray(counts, np.int32), np.asarray(gt_off, np.int32)
        m, per = reference(dets, counts, gt_boxes, gt_cls, gt_off, nc)
        for k, v in dict(dets=dets, counts=counts, gt_boxes=gt_boxes, gt_cls=gt_cls, gt_off=gt_off,
                         nc=np.array(nc, np.int32), matrix=m).items():
            out[f"{name}/{k}"] = v
        print(name, "dets", dets.shape, "gt", len(gt_boxes), "matrix sum", int(m.sum()), "diag", int(np.trace(m)),
              "FP", int(m[:nc, nc].sum()), "FN", int(m[nc, :nc].sum()), flush=True)
        return m, per

    def all_cells(m, nc):
        off = m[:nc, :nc].sum() - np.trace(m[:nc, :nc])
        return np.trace(m[:nc, :nc]) > 0 and off > 0 and m[:nc, nc].sum() > 0 and m[nc, :nc].sum() > 0

    def padded(d, max_det, fill):
        pad = fill[np.arange(max_det - len(d)) % len(fill)] if len(d) < max_det else fill[:0]
        return np.concatenate([d, pad])[None]

    # ------------------------------------------------------------------ dense: every kind of cell
    gt, gc = rand_boxes(rng, 60), rng.integers(0, NC, 60).astype(np.float32)
    d = detections(rng, gt, gc, np.repeat(np.arange(50), 5), 50)
    m, _ = case("dense", d[None], [300], gt, gc, [0, 60])
    assert all_cells(m, NC) and m[NC, NC] == 0
    cm = ConfusionMatrix(names={i: f"c{i}" for i in range(NC)})
    cm.matrix[...] = m
    tp, fp = cm.tp_fp()
    out["dense/tp"], out["dense/fp"] = np.asarray(tp, np.float64), np.asarray(fp, np.float64)
    out["dense/normalized"] = cm.matrix / (cm.matrix.sum(0).reshape(1, -1) + 1e-9)  # metrics.py:585

    # ------------------------------------------------------------------ many_gt: 2 LDS chunks and a remainder
    M = 2 * GT_CHUNK + 37
    gt, gc = rand_boxes(rng, M, 16, 60), rng.integers(0, NC, M).astype(np.float32)
    d = detections(rng, gt, gc, rng.choice(M, 260, replace=False), 40)
    m, _ = case("many_gt", d[None], [300], gt, gc, [0, M])
    part = d[d[:, 4] > 0.25]
    iou = box_iou(torch.from_numpy(gt), torch.from_numpy(part[:, :4])).numpy()
    claimed = iou.argmax(0)[iou.max(0) > IOU_THRES]  # a claimed GT has a winner
    assert (claimed < GT_CHUNK).any() and ((claimed >= GT_CHUNK) & (claimed < 2 * GT_CHUNK)).any()
    assert (claimed >= 2 * GT_CHUNK).any() and all_cells(m, NC)

    # ------------------------------------------------------------------ batch_mixed
    ngt, cnt = [5, 0, 40, 1], [0, 7, 300, 1]
    off = np.concatenate([[0], np.cumsum(ngt)])
    gt, gc = rand_boxes(rng, sum(ngt)), rng.integers(0, NC, sum(ngt)).astype(np.float32)
    rows = []
    for b in range(4):
        g = slice(off[b], off[b + 1])
        fill = np.concatenate([gt[:5], np.ones((5, 1), np.float32), gc[:5, None]], 1)  # image 0's GT, exactly
        if b == 2:
            db = detections(rng, gt[g], gc[g], np.repeat(np.arange(34), 7), 62)  # six GT without a detection
        elif b == 3:
            db = np.concatenate([jitter(rng, gt[g], [0.004]), [[0.8, gc[g][0]]]], 1).astype(np.float32)
        else:
            db = rand_boxes(rng, cnt[b])
            db = np.concatenate([db, np.linspace(0.9, 0.3, cnt[b], dtype=np.float32)[:, None],
                                 rng.integers(0, NC, (cnt[b], 1)).astype(np.float32)], 1)
        rows.append(padded(db[:cnt[b]], 300, fill))
    m, per = case("batch_mixed", np.concatenate(rows), cnt, gt, gc, off)
    assert per[0][NC, :NC].sum() == 5 and per[0].sum() == 5  # all FN
    assert per[1][:NC, NC].sum() == 7 and per[1].sum() == 7  # all FP
    assert per[3].sum() == 1 and np.trace(per[3][:NC, :NC]) == 1 and all_cells(per[2], NC)

    # ------------------------------------------------------------------ conf_edge: strict conf > thres at 0.25 and 0.5
    gt = np.array([[40 + 90 * i, 60, 100 + 90 * i, 140] for i in range(6)], np.float32)
    gc = (np.arange(6) % NC).astype(np.float32)
    confs = np.array([0.9, np.nextafter(np.float32(0.5), np.float32(1)), 0.5, np.nextafter(np.float32(0.25), np.float32(1)),
                      0.25, 0.1], np.float32)
    d = np.concatenate([jitter(rng, gt, [0.01] * 6), confs[:, None], gc[:, None]], 1).astype(np.float32)
    m, _ = case("conf_edge", padded(d, 8, d[:1] * [1, 1, 1, 1, 0, 1] + [0, 0, 0, 0, 1, 0]), [6], gt, gc, [0, 6])
    assert np.trace(m[:NC, :NC]) == 4 and m[NC, :NC].sum() == 2 and m.sum() == 6  # 0.25 itself stays out
    m50, _ = reference(out["conf_edge/dets"], [6], gt, gc, [0, 6], NC, conf=0.5)
    assert np.trace(m50[:NC, :NC]) == 2 and m50[NC, :NC].sum() == 4 and m50.sum() == 6  # 0.5 itself stays out
    out["conf_edge/matrix_conf50"] = m50

    # ------------------------------------------------------------------ near_thr
    # image s (17 of them) holds GT j = (0, 50 j, w_j, 50 j + 30) and one detection sharing x1, y1, y2 with it whose
    # x2 is s - 8 float steps from the first x2 at which the reference's IoU exceeds 0.45
    nj = 10
    widths = (37.3 + 11.7 * np.arange(nj)).astype(np.float32)
    gt1 = np.stack([np.zeros(nj), 50.0 * np.arange(nj), widths, 50.0 * np.arange(nj) + 30], 1).astype(np.float32)
    cross = []
    for j in range(nj):
        g = torch.from_numpy(gt1[j:j + 1])

        def reached(x2):
            db = g.clone()
            db[0, 2] = float(x2)
            return bool((box_iou(g, db) > IOU_THRES)[0, 0])  # the comparison of metrics.py:488

        x2 = np.float32(np.float64(IOU_THRES) * np.float64(widths[j]))
        while reached(x2):
            x2 = np.nextafter(x2, np.float32(0))
        while not reached(x2):
            x2 = np.nextafter(x2, np.float32(S))
        cross.append(x2)
    dets = np.zeros((17, nj, 6), np.float32)
    for s in range(17):
        for j in range(nj):
            x2 = cross[j]
            for _ in range(abs(s - 8)):
                x2 = np.nextafter(x2, np.float32(S if s > 8 else 0))
            dets[s, j] = [0, gt1[j, 1], x2, gt1[j, 3], 0.9 - 0.01 * j, j % NC]
    gc1 = (np.arange(nj) % NC).astype(np.float32)
    m, per = case("near_thr", dets, [nj] * 17, np.tile(gt1, (17, 1)), np.tile(gc1, 17), np.arange(18) * nj)
    out["near_thr/per_image"] = per
    above = np.array([[bool((box_iou(torch.from_numpy(gt1[j:j + 1]), torch.from_numpy(dets[s, j:j + 1, :4])) > IOU_THRES)[0, 0])
                       for j in range(nj)] for s in range(17)])
    assert above.any(0).all() and not above.all(0).any(), above.sum(0)  # every GT's column has both outcomes
    hits = np.array([np.trace(p[:NC, :NC]) for p in per])  # matched pairs per step: classes agree, so the diagonal
    assert np.array_equal(hits, above.sum(1)), (hits, above.sum(1))  # above: a match; else an FN and an FP
    assert all(p[:NC, NC].sum() == nj - h and p[NC, :NC].sum() == nj - h for p, h in zip(per, hits))
    print("near_thr matches per step", hits.tolist(), flush=True)

    # ------------------------------------------------------------------ contested
    # GT A (cls 0) is the best GT of d0..d3 at distinct IoUs: d0 keeps it, the rest are FPs, d3 although it overlaps
    # GT B (cls 1) above 0.45, which nobody claims: an FN.  GT C (cls 2) is matched by a class-0 detection; GT D
    # (cls 1) has no detection.
    gt = np.array([[100, 100, 200, 200], [130, 100, 230, 200], [400, 300, 500, 420], [300, 500, 380, 600]], np.float32)
    gc = np.array([0, 1, 2, 1], np.float32)
    d = np.array([[101, 100, 200, 200, 0.9, 0], [100, 104, 200, 200, 0.8, 0], [95, 100, 200, 200, 0.7, 0],
                  [112, 100, 212, 200, 0.6, 0], [402, 300, 500, 420, 0.5, 0]], np.float32)
    iou = box_iou(torch.from_numpy(gt), torch.from_numpy(d[:, :4])).numpy()
    assert (iou[:, :4].argmax(0) == 0).all() and len(set(iou[0, :4].tolist())) == 4 and iou[0, :4].argmax() == 0
    assert iou[1, 3] > IOU_THRES and (iou[1, :3] < iou[0, :3]).all()
    m, _ = case("contested", padded(d, 8, d[:1]), [5], gt, gc, [0, 4])
    want = np.zeros((4, 4), np.int64)
    want[0, 0], want[0, 3], want[3, 1], want[0, 2] = 1, 3, 2, 1
    assert np.array_equal(m, want), m

    # ------------------------------------------------------------------ max_det_big: beyond the LDS-resident state
    assert V.DET_LDS < 900
    gt, gc = rand_boxes(rng, 150), rng.integers(0, NC, 150).astype(np.float32)
    d = detections(rng, gt, gc, np.repeat(np.arange(130), 6), 120)
    fill = np.concatenate([gt[:8], np.ones((8, 1), np.float32), gc[:8, None]], 1)
    m, _ = case("max_det_big", padded(d, 1000, fill), [900], gt, gc, [0, 150])
    assert all_cells(m, NC)
    part = np.nonzero(d[:, 4] > 0.25)[0]
    assert (part >= V.DET_LDS).any()  # participating detections beyond the LDS-resident range

    # ------------------------------------------------------------------ nc80 / nc1
    gt, gc = rand_boxes(rng, 40), rng.integers(0, 80, 40).astype(np.float32)
    gc[:2] = [0, 79]
    d = detections(rng, gt, gc, np.repeat(np.arange(34), 5), 30, nc=80)
    m, _ = case("nc80", d[None], [200], gt, gc, [0, 40], nc=80)
    assert m.shape == (81, 81) and all_cells(m, 80) and m[:, 79].sum() > 0 and m[:, 0].sum() > 0
    gt, gc = rand_boxes(rng, 20), np.zeros(20, np.float32)
    d = detections(rng, gt, gc, np.repeat(np.arange(16), 5), 20, nc=1)
    m, _ = case("nc1", d[None], [100], gt, gc, [0, 20], nc=1)
    assert m.shape == (2, 2) and m[0, 0] > 0 and m[0, 1] > 0 and m[1, 0] > 0 and m[1, 1] == 0

    np.savez_compressed(HERE / "confusion.npz", **out)
    print("confusion.npz", (HERE / "confusion.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
