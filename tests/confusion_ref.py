"""Numpy restatement of the device confusion matrix (csrc/val.hip val_confusion_kernel), the rule of the reference's
ConfusionMatrix.process_batch (utils/metrics.py:441-518) per image:

    detections with conf > conf_thres take part;  iou = box_iou(gt, det) in fp32, not masked by class
    g*(d) = arg max_g iou[g, d] (of equal maxima the higher g);  d claims g*(d) when iou[g*(d), d] > iou_thres
    w(g) = the claimant of g with the largest IoU (of equal IoUs the higher d)
    GT g with a winner:  matrix[cls(w(g)), cls(g)] += 1       every other GT:  matrix[nc, cls(g)] += 1
    every participating detection that is no winner:          matrix[cls(d), nc] += 1

golden/confusion.npz pins it against the reference's own process_batch (test_confusion.py); the device results are
compared with it where no reference fixture can exist (the engine's own detections).
"""

from __future__ import annotations

import numpy as np

from val_ref import box_iou


def confusion_conf(conf):
    """utils/metrics.py:465."""
    return 0.25 if conf in {None, 0.001} else conf


def confusion_image(matrix, det, gt_boxes, gt_cls, nc, conf=0.25, iou_thres=0.45) -> None:
    """Adds one image to `matrix` (nc + 1, nc + 1).  det (k, 6) xyxy, conf, cls."""
    det = np.asarray(det, np.float32).reshape(-1, 6)
    det = det[det[:, 4] > np.float32(conf)]
    dc, gc = det[:, 5].astype(np.int64), np.asarray(gt_cls, np.float32).astype(np.int64)
    D, M = len(det), len(gc)
    kept = np.zeros(D, bool)
    if D and M:
        iou = box_iou(np.asarray(gt_boxes, np.float32).reshape(-1, 4), det[:, :4])
        g = M - 1 - np.argmax(iou[::-1], axis=0)  # the last (highest-index) maximum
        m = iou[g, np.arange(D)]
        claims = m > np.float32(iou_thres)
        for gi in range(M):
            c = np.nonzero(claims & (g == gi))[0]
            if len(c):
                w = c[len(c) - 1 - np.argmax(m[c][::-1])]  # the largest IoU, of equal ones the higher detection
                kept[w] = True
                matrix[dc[w], gc[gi]] += 1
            else:
                matrix[nc, gc[gi]] += 1
    else:
        for c in gc:
            matrix[nc, c] += 1
    for c in dc[~kept]:
        matrix[c, nc] += 1


def confusion(dets, counts, gt_boxes, gt_cls, gt_off, nc, conf=0.25, iou_thres=0.45, n=None) -> np.ndarray:
    """fce_val_confusion on the host for images 0..n-1: (nc + 1, nc + 1) int64."""
    matrix = np.zeros((nc + 1, nc + 1), np.int64)
    for b in range(len(counts) if n is None else n):
        k, g0, g1 = int(counts[b]), int(gt_off[b]), int(gt_off[b + 1])
        confusion_image(matrix, dets[b, :k], gt_boxes[g0:g1], gt_cls[g0:g1], nc, conf, iou_thres)
    return matrix
