"""Detection metrics on the host: the reference's AP computation restated (ultralytics/utils/metrics.py:785-910
compute_ap / ap_per_class, :913-1076 Metric, :1079-1201 DetMetrics), numpy only.

The device decides which detections are true positives at each IoU threshold (`val.DeviceMatcher`, csrc/val.hip); what
remains is a sort by confidence and a few cumulative sums over all detections of the dataset, float64 numpy exactly as
the reference runs it.  The confusion matrix is counted on the device too (`val.DeviceConfusionMatrix`) and held
here as `ConfusionMatrix` (metrics.py:380-534).  No plots, no COCO JSON.
"""

from __future__ import annotations

import numpy as np

KEYS = ("metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)")

_trapezoid = getattr(np, "trapezoid", None) or np.trapz  # metrics.py:808 (np.trapz is deprecated from numpy 2.0)


def smooth(y: np.ndarray, f: float = 0.05) -> np.ndarray:
    """metrics.py:689-694: box filter of fraction f."""
    nf = round(len(y) * f * 2) // 2 + 1  # number of filter elements (must be odd)
    p = np.ones(nf // 2)  # ones padding
    yp = np.concatenate((p * y[0], y, p * y[-1]), 0)  # y padded
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")  # y-smoothed


def compute_ap(recall, precision):
    """metrics.py:785-814: (AP, precision envelope, recall with sentinels) by the 101-point interpolation (COCO)."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))  # the precision envelope
    x = np.linspace(0, 1, 101)
    ap = _trapezoid(np.interp(x, mrec, mpre), x)
    return ap, mpre, mrec


def ap_per_class(tp: np.ndarray, conf: np.ndarray, pred_cls: np.ndarray, target_cls: np.ndarray, eps: float = 1e-16):
    """metrics.py:817-910 without the plots.  tp (D, niou) bool, conf (D), pred_cls (D), target_cls (T).
    Returns (p, r, f1, ap (nc, niou), unique_classes int): precision, recall and F1 per class with GT at the
    confidence of the maximal mean F1 (1000-point confidence grid), AP per class and threshold."""
    i = np.argsort(-conf)
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes, nt = np.unique(target_cls, return_counts=True)
    nc = unique_classes.shape[0]
    x = np.linspace(0, 1, 1000)
    ap, p_curve, r_curve = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l = nt[ci]  # number of labels
        n_p = i.sum()  # number of predictions
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + eps)
        r_curve[ci] = np.interp(-x, -conf[i], recall[:, 0], left=0)  # negative x, xp because xp decreases
        precision = tpc / (tpc + fpc)
        p_curve[ci] = np.interp(-x, -conf[i], precision[:, 0], left=1)  # p at pr_score
        for j in range(tp.shape[1]):
            ap[ci, j], _, _ = compute_ap(recall[:, j], precision[:, j])
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    i = smooth(f1_curve.mean(0), 0.1).argmax()  # max F1 index
    return p_curve[:, i], r_curve[:, i], f1_curve[:, i], ap, unique_classes.astype(int)


class Metric:
    """metrics.py:913-1076: the per-class results and their means."""

    def __init__(self):
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = [], [], [], [], []
        self.nc = 0

    @property
    def ap50(self):
        return self.all_ap[:, 0] if len(self.all_ap) else []

    @property
    def ap(self):
        return self.all_ap.mean(1) if len(self.all_ap) else []

    @property
    def mp(self):
        return self.p.mean() if len(self.p) else 0.0

    @property
    def mr(self):
        return self.r.mean() if len(self.r) else 0.0

    @property
    def map50(self):
        return self.all_ap[:, 0].mean() if len(self.all_ap) else 0.0

    @property
    def map75(self):
        return self.all_ap[:, 5].mean() if len(self.all_ap) else 0.0

    @property
    def map(self):
        return self.all_ap.mean() if len(self.all_ap) else 0.0

    def mean_results(self):
        return [self.mp, self.mr, self.map50, self.map]

    def class_result(self, i: int):
        return self.p[i], self.r[i], self.ap50[i], self.ap[i]

    def fitness(self) -> float:
        w = [0.0, 0.0, 0.0, 1.0]  # weights for [P, R, mAP@0.5, mAP@0.5:0.95]
        return (np.nan_to_num(np.array(self.mean_results())) * w).sum()

    def update(self, results):
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = results


class DetMetrics:
    """metrics.py:1079-1201: per-image statistics accumulated over a dataset, then `process()` once."""

    def __init__(self, names: dict | None = None):
        self.names = names or {}
        self.box = Metric()
        self.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[], target_img=[])
        self.nt_per_class = self.nt_per_image = None

    def update_stats(self, stat: dict) -> None:
        for k in self.stats:
            self.stats[k].append(stat[k])

    def process(self) -> dict:
        if not self.stats["tp"]:  # no image seen: the results stay as they are (zeros on a fresh object)
            return {}
        stats = {k: np.concatenate(v, 0) for k, v in self.stats.items()}
        self.box.nc = len(self.names)
        self.box.update(ap_per_class(stats["tp"], stats["conf"], stats["pred_cls"], stats["target_cls"]))
        self.nt_per_class = np.bincount(stats["target_cls"].astype(int), minlength=len(self.names))
        self.nt_per_image = np.bincount(stats["target_img"].astype(int), minlength=len(self.names))
        return stats

    def clear_stats(self) -> None:
        for v in self.stats.values():
            v.clear()

    @property
    def keys(self):
        return list(KEYS)

    def mean_results(self):
        return self.box.mean_results()

    def class_result(self, i: int):
        return self.box.class_result(i)

    @property
    def fitness(self) -> float:
        return self.box.fitness()

    @property
    def ap_class_index(self):
        return self.box.ap_class_index

    @property
    def results_dict(self) -> dict:
        keys = [*self.keys, "fitness"]
        values = ((float(x) if hasattr(x, "item") else x) for x in ([*self.mean_results(), self.fitness]))
        return dict(zip(keys, values))


class ConfusionMatrix:
    """metrics.py:380-403, :524-534 and the normalisation of :585 for detection: `matrix` (nc + 1, nc + 1) float64,
    row = predicted class, column = true class, index nc = background.  The counting itself (process_batch) runs on
    the device (`val.DeviceConfusionMatrix`, csrc/val.hip); this object holds a run's counts."""

    def __init__(self, names=(), matrix=None):
        self.names = names
        self.nc = len(names)
        self.matrix = np.zeros((self.nc + 1, self.nc + 1))
        if matrix is not None:
            m = np.asarray(matrix)
            if m.shape != self.matrix.shape:
                raise ValueError(f"ConfusionMatrix: matrix must be {self.matrix.shape}, not {m.shape}")
            self.matrix[...] = m

    def tp_fp(self):
        """metrics.py:524-534: (true positives, false positives) per class, the background dropped."""
        tp = self.matrix.diagonal()
        fp = self.matrix.sum(1) - tp
        return tp[:-1], fp[:-1]

    def normalized(self) -> np.ndarray:
        """metrics.py:585: every column (true class) divided by its sum + 1e-9, as the reference's plot shows it."""
        return self.matrix / (self.matrix.sum(0).reshape(1, -1) + 1e-9)
