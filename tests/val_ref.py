"""Numpy restatement of the device GT matching (csrc/val.hip): the reference's box_iou in fp32, in its order of
operations (numpy rounds every fp32 operation on its own, as the kernel does with contraction off), masked by class
equality, and the matching rule

    g*(d) = arg max_g iou[g, d] (of equal maxima the higher g),   m(d) = max_g iou[g, d]
    tp[d, i] = m(d) >= iouv[i]  and  no d' < d has g*(d') == g*(d) and m(d') >= iouv[i]

which golden/val.npz pins against the reference's BaseValidator.match_predictions (test_val.py).  The device results
are compared with it bit for bit where no reference fixture can exist (the engine's own detections).
"""

from __future__ import annotations

import numpy as np
import torch

IOUV = torch.linspace(0.5, 0.95, 10).numpy()  # models/yolo/detect/val.py:59, fp32 (golden/val.npz holds the same bits)


def box_iou(gt: np.ndarray, det: np.ndarray) -> np.ndarray:
    """utils/metrics.py:57-77 with box1 = gt (M, 4), box2 = det (D, 4): (M, D) fp32."""
    a, b = gt.astype(np.float32)[:, None, :], det.astype(np.float32)[None, :, :]
    zero, eps = np.float32(0), np.float32(1e-7)
    w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), zero)
    h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), zero)
    inter = w * h
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    out = inter / (((area_a + area_b) - inter) + eps)
    assert out.dtype == np.float32
    return out


def match_image(det_boxes, det_cls, gt_boxes, gt_cls, iouv=IOUV) -> np.ndarray:
    """(D, len(iouv)) bool for one image."""
    D, M = len(det_boxes), len(gt_boxes)
    tp = np.zeros((D, len(iouv)), bool)
    if D == 0 or M == 0:
        return tp
    iou = box_iou(gt_boxes, det_boxes) * (np.asarray(gt_cls, np.float32)[:, None] == np.asarray(det_cls, np.float32)[None, :])
    g = M - 1 - np.argmax(iou[::-1], axis=0)  # the last (highest-index) maximum
    m = iou.max(axis=0)
    for i, t in enumerate(np.asarray(iouv, np.float32)):
        idx = np.nonzero(m >= t)[0]  # ascending detection index
        _, first = np.unique(g[idx], return_index=True)  # the first detection that holds each GT
        tp[idx[first], i] = True
    return tp


def match(dets, counts, gt_boxes, gt_cls, gt_off, iouv=IOUV) -> np.ndarray:
    """fce_val_match on the host: dets (n, max_det, 6), counts (n) -> tp (n, max_det, len(iouv)) bool, rows >= counts
    False."""
    n, max_det = dets.shape[:2]
    tp = np.zeros((n, max_det, len(iouv)), bool)
    for b in range(n):
        k, g0, g1 = int(counts[b]), int(gt_off[b]), int(gt_off[b + 1])
        tp[b, :k] = match_image(dets[b, :k, :4], dets[b, :k, 5], gt_boxes[g0:g1], gt_cls[g0:g1], iouv)
    return tp


def words(tp: np.ndarray) -> np.ndarray:
    """(..., niou) bool -> (...) uint16 with bit i = threshold i (the kernel's output form)."""
    return (tp.astype(np.uint16) << np.arange(tp.shape[-1], dtype=np.uint16)).sum(-1).astype(np.uint16)
