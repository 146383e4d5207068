"""Detection validation on the device: precision, recall, mAP50 and mAP50-95 of a model over a labelled dataset.

The MI355X form of the reference's validation loop for detection (ultralytics/engine/validator.py:141-264 and
models/yolo/detect/val.py: preprocess, postprocess, update_metrics, get_stats):

    u8 canvases --(Engine: forward)--> pred --(fce_nms_ex: conf 0.001, multi_label)--> (k, 6) per image, canvas pixels
      --(fce_val_match: box_iou x class equality, match_predictions at the ten thresholds)--> tp words (k) uint16
      --(one D2H copy: packed NMS outputs + tp words)--> host: DetMetrics.update_stats per image
      --(fce_val_confusion, beside the matcher: detections above 0.25, IoU > 0.45)--> resident (nc + 1)^2 int32 counts
    stats(): metrics.ap_per_class over everything accumulated -> results_dict; the counts -> confusion_matrix

The reference syncs once per image (`iou.cpu().numpy()`) and matches in numpy; here the matching runs beside the NMS
on the lane's stream and the host only unpacks bits.  GT boxes are prepared on the host exactly as
`DetectionValidator._prepare_batch` does (xywh2xyxy, times (W, H, W, H), torch fp32) and go up in one H2D copy per
batch.  The NMS outputs are in canvas pixels, the frame the reference matches in: no scale_boxes.

Matching rule and the one tie rule: csrc/val.hip and DESIGN.md ("Validation").
"""

from __future__ import annotations

import ctypes as C
from collections import deque

import numpy as np
import torch

from . import _native as N
from .engine import NMS, Engine, Pipeline
from .metrics import ConfusionMatrix, DetMetrics
from .predict import default_lanes

GT_CHUNK = 256  # csrc/val.hip VAL_GT_CHUNK: GT boxes staged in LDS at a time
DET_LDS = 512  # csrc/val.hip VAL_DET_LDS: detections per image matched without a workspace


def iou_vector(niou: int = 10) -> np.ndarray:
    """models/yolo/detect/val.py:59: torch.linspace(0.5, 0.95, 10) in fp32 (`niou` = 1: [0.5], mAP50 alone)."""
    return torch.linspace(0.5, 0.95, niou).numpy().astype(np.float32)


def unpack_tp(words, niou: int = 10) -> np.ndarray:
    """(k,) uint16 words (bit i = threshold i) -> (k, niou) bool, the reference's `tp` array."""
    w = np.asarray(words).view(np.uint16).reshape(-1)
    return ((w[:, None] >> np.arange(niou, dtype=np.uint16)) & 1).astype(bool)


def pack_gt(batch_idx, cls, bboxes, n: int, H: int, W: int):
    """The collate's labels as the matcher reads them: (gt_boxes (M, 4) canvas xyxy fp32, gt_cls (M,) fp32, gt_off
    (n + 1,) int32), GT stably sorted by image.  Boxes as val.py:145 makes them: ops.xywh2xyxy, then times the
    canvas's (W, H, W, H), in torch fp32 on the host."""
    bi = torch.as_tensor(batch_idx).reshape(-1).cpu()
    cl = torch.as_tensor(cls).cpu().float().reshape(-1)
    bb = torch.as_tensor(bboxes).cpu().float().reshape(-1, 4)
    if not (bi.numel() == cl.numel() == bb.shape[0]):
        raise ValueError("pack_gt: batch_idx, cls and bboxes must have one row per GT box")
    bi = bi.long()
    if bi.numel() and (int(bi.min()) < 0 or int(bi.max()) >= n):
        raise ValueError(f"pack_gt: batch_idx outside 0..{n - 1}")
    xy, wh = bb[:, :2], bb[:, 2:] / 2  # ops.py:224-240 xywh2xyxy
    boxes = torch.cat((xy - wh, xy + wh), 1) * torch.tensor((H, W))[[1, 0, 1, 0]]
    order = torch.argsort(bi, stable=True)
    off = torch.zeros(n + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.bincount(bi, minlength=n), 0)
    return boxes[order].contiguous(), cl[order].contiguous(), off


class DeviceMatcher:
    """`DetectionValidator._process_batch` for a whole batch on the device (fce_val_match):

        tp = matcher(dets, counts, gt_boxes, gt_cls, gt_off)      # (batch, max_det) uint16, bit i = threshold i

    dets (batch, max_det, 6) f32 / counts (batch,) i32: NMS outputs (`engine.NMS`), gt_boxes (M, 4) f32 xyxy in the
    same frame, gt_cls (M,) f32, gt_off (batch + 1,) i32 (`pack_gt`), all on the device.  Rows >= counts[b] are 0.
    Runs on the current stream, allocates nothing per call and can be captured (torch.cuda.graph)."""

    def __init__(self, batch: int, max_det: int, device, niou: int = 10, iouv=None):
        self.batch, self.max_det, self.device = batch, max_det, torch.device(device)
        v = iou_vector(niou) if iouv is None else np.asarray(iouv, np.float32).reshape(-1)
        self.niou = len(v)
        self.iouv = v
        self._iouv = (C.c_float * max(len(v), 1))(*v.tolist())  # host array: passed to the kernel by value
        nb = N.lib().fce_val_match_workspace_bytes(batch, max_det, 0, self.niou)
        self.ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.device)
        self.tp = torch.zeros((batch, max_det), dtype=torch.int16, device=self.device).view(torch.uint16)

    def __call__(self, dets, counts, gt_boxes, gt_cls, gt_off, out: torch.Tensor | None = None) -> torch.Tensor:
        out = self.tp if out is None else out
        assert dets.is_contiguous() and dets.dtype == torch.float32 and tuple(dets.shape) == (self.batch, self.max_det, 6)
        assert counts.is_contiguous() and counts.dtype == torch.int32 and counts.numel() == self.batch
        assert gt_boxes.is_contiguous() and gt_boxes.dtype == torch.float32 and gt_boxes.dim() == 2 and gt_boxes.shape[1] == 4
        assert gt_cls.is_contiguous() and gt_cls.dtype == torch.float32 and gt_cls.numel() == gt_boxes.shape[0]
        assert gt_off.is_contiguous() and gt_off.dtype == torch.int32 and gt_off.numel() == self.batch + 1
        assert out.is_contiguous() and out.element_size() == 2 and out.numel() == self.batch * self.max_det
        stream = torch.cuda.current_stream(self.device).cuda_stream
        N.call("fce_val_match", dets.data_ptr(), counts.data_ptr(), self.batch, self.max_det, gt_boxes.data_ptr(),
               gt_cls.data_ptr(), gt_off.data_ptr(), C.cast(self._iouv, C.c_void_p), self.niou, self.ws.data_ptr(),
               self.ws.numel(), out.data_ptr(), stream)
        return out


def confusion_conf(conf) -> float:
    """utils/metrics.py:465: the confusion matrix counts detections above 0.25 when the validation default conf
    (0.001) or None is passed, above `conf` otherwise."""
    return 0.25 if conf in {None, 0.001} else conf


class DeviceConfusionMatrix:
    """`ConfusionMatrix.process_batch` (utils/metrics.py:441-518) for a whole batch on the device, accumulated in
    one resident (nc + 1, nc + 1) int32 table (fce_val_confusion):

        cm = DeviceConfusionMatrix(nc, batch, max_det, device)
        cm(dets, counts, gt_boxes, gt_cls, gt_off, n=n)           # per batch: adds images 0..n-1, no host work
        counts = cm.numpy()                                       # once, at the end: syncs, returns a copy

    Inputs as `DeviceMatcher`; `conf` and `iou_thres` are used as given (`confusion_conf` is the reference's rule for
    the validator's conf).  Runs on the current stream, allocates nothing per call and can be captured.  A class
    outside 0..nc-1 is counted nowhere but in the workspace's error word; `numpy()` raises if there was one."""

    def __init__(self, nc: int, batch: int, max_det: int, device, conf: float = 0.25, iou_thres: float = 0.45):
        self.nc, self.batch, self.max_det, self.device = int(nc), batch, max_det, torch.device(device)
        self.conf, self.iou_thres = float(conf), float(iou_thres)
        nb = N.lib().fce_val_confusion_workspace_bytes(batch, max_det)
        if self.nc <= 0 or nb == 0:
            raise ValueError("DeviceConfusionMatrix: nc, batch and max_det must be positive")
        self.ws = torch.zeros(nb, dtype=torch.uint8, device=self.device)  # word 0: out-of-range classes met
        self.matrix = torch.zeros((self.nc + 1, self.nc + 1), dtype=torch.int32, device=self.device)

    def __call__(self, dets, counts, gt_boxes, gt_cls, gt_off, n: int | None = None) -> torch.Tensor:
        n = self.batch if n is None else int(n)
        if not 0 < n <= self.batch:
            raise ValueError(f"DeviceConfusionMatrix: n must be 1..{self.batch}")
        assert dets.is_contiguous() and dets.dtype == torch.float32 and tuple(dets.shape) == (self.batch, self.max_det, 6)
        assert counts.is_contiguous() and counts.dtype == torch.int32 and counts.numel() == self.batch
        assert gt_boxes.is_contiguous() and gt_boxes.dtype == torch.float32 and gt_boxes.dim() == 2 and gt_boxes.shape[1] == 4
        assert gt_cls.is_contiguous() and gt_cls.dtype == torch.float32 and gt_cls.numel() == gt_boxes.shape[0]
        assert gt_off.is_contiguous() and gt_off.dtype == torch.int32 and gt_off.numel() >= n + 1
        stream = torch.cuda.current_stream(self.device).cuda_stream
        N.call("fce_val_confusion", dets.data_ptr(), counts.data_ptr(), n, self.max_det, gt_boxes.data_ptr(),
               gt_cls.data_ptr(), gt_off.data_ptr(), self.nc, self.conf, self.iou_thres, self.ws.data_ptr(),
               self.ws.numel(), self.matrix.data_ptr(), stream)
        return self.matrix

    def zero_(self) -> None:
        """Clear the matrix and the error word, in stream order on the current stream."""
        self.matrix.zero_()
        self.ws[:16].zero_()

    def numpy(self) -> np.ndarray:
        """The counts so far, (nc + 1, nc + 1) int32 on the host (synchronises the device)."""
        torch.cuda.synchronize(self.device)
        bad = int(self.ws[:4].view(torch.int32).item())
        if bad:
            raise N.FceError(f"fce_val_confusion: {bad} GT or detection classes outside 0..{self.nc - 1}")
        return self.matrix.cpu().numpy().copy()


class _Slot:
    """What one pipeline slot owns beside its NMS: the canvas of a batch that came from the host or was short, the
    GT staging (pinned host + device: gt_off | gt_cls | gt_boxes) and the pinned copy of its results."""

    def __init__(self, batch: int, nbytes: int):
        self.canvas = None
        self.gt_host = self.gt_dev = None
        self.out_host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.done = torch.cuda.Event()
        self.pending = None  # (images, target_cls per image) of the batch in flight

    def reserve_gt(self, nbytes: int, device):
        if self.gt_host is None or self.gt_host.numel() < nbytes:
            cap = max(nbytes + nbytes // 4, 4096)
            self.gt_host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            self.gt_dev = torch.empty(cap, dtype=torch.uint8, device=device)


class Validator:
    """The reference's `model.val()` for detection on labelled, letterboxed batches:

        with Validator(model, batch=32, imgsz=640) as v:
            for batch in loader:          # the reference collate's dict: img, batch_idx, cls, bboxes
                v.update(batch)
            results = v.stats()           # metrics/precision(B), recall(B), mAP50(B), mAP50-95(B), fitness

    Defaults are the reference's validation defaults (cfg/default.yaml conf 0.001, iou 0.7, max_det 300;
    DetectionValidator.postprocess: multi_label NMS, agnostic = single_cls or agnostic_nms).  `single_cls` zeroes the
    predicted classes as `_prepare_pred` does; the GT classes of such a dataset are already 0 (the dataset does that).
    `lanes` batches are in flight; their results are read in submission order, when a slot is needed again or at
    `stats()`, so the accumulated statistics do not depend on `lanes`.  As under the reference's defaults (plots) the
    confusion matrix is always counted: after `stats()`, `confusion_matrix` (metrics.ConfusionMatrix) holds that run's
    counts (utils/metrics.py:441-518 at conf 0.25 when `conf` is 0.001 or None, else `conf`; IoU 0.45)."""

    def __init__(self, model, batch: int, imgsz=640, device=None, conf=0.001, iou=0.7, max_det=300,
                 lanes: int | None = None, graph: bool = True, single_cls: bool = False, agnostic_nms: bool = False):
        if lanes is None:
            lanes = default_lanes(model)
        lanes = max(1, int(lanes))
        self.engine = Engine(model, batch, imgsz, device, graph=graph)
        self.device, self.batch, self.max_det = self.engine.device, batch, max_det
        self.H, self.W = self.engine.H, self.engine.W
        self.single_cls = bool(single_cls)
        self.tp_bytes = (batch * max_det * 2 + 15) // 16 * 16
        self.pipe = Pipeline(self.engine, depth=max(lanes, 2), defer=False, lanes=lanes, slot_tail=self.tp_bytes,
                             conf=conf, iou=iou, max_det=max_det, multi_label=True,
                             agnostic=bool(single_cls or agnostic_nms))
        self.matcher = DeviceMatcher(batch, max_det, self.device)
        self.niou = self.matcher.niou
        self.slots = [_Slot(batch, self.pipe.slot_bytes) for _ in range(self.pipe.depth)]
        # one table per slot: slots run on different streams, and beyond DET_LDS detections the kernel's state is in
        # the table's workspace.  stats() adds them up (integer counts: the sum does not depend on `lanes`)
        self.confusion = [DeviceConfusionMatrix(self.engine.nc, batch, max_det, self.device, conf=confusion_conf(conf))
                          for _ in self.slots]
        names = getattr(model, "names", None) or {}
        self.cm_names = names if len(names) == self.engine.nc else {i: f"{i}" for i in range(self.engine.nc)}
        self.confusion_matrix = ConfusionMatrix(self.cm_names)  # the last stats()'s run
        self.metrics = DetMetrics(names)
        self.seen = 0
        self._fifo = deque()  # slots in flight, oldest first

    # ------------------------------------------------------------------ device half
    def _canvas(self, sl: _Slot, img: torch.Tensor, n: int) -> torch.Tensor:
        if img.device == self.device and n == self.batch and img.is_contiguous():
            return img
        if sl.canvas is None:
            sl.canvas = torch.empty((self.batch, 3, self.H, self.W), dtype=torch.uint8, device=self.device)
        sl.canvas[:n].copy_(img, non_blocking=True)
        if n < self.batch:  # fixed-shape engine: a short last batch repeats its last canvas (rows dropped later)
            sl.canvas[n:].copy_(sl.canvas[n - 1:n].expand(self.batch - n, -1, -1, -1))
        return sl.canvas

    def update(self, batch: dict) -> None:
        """One batch of the reference collate's dict: `img` uint8 (B', 3, H, W) letterboxed canvases (host or device,
        B' <= batch), `batch_idx` (M,), `cls` (M,) or (M, 1), `bboxes` (M, 4) normalised xywh in the canvas frame."""
        img = batch["img"]
        n = int(img.shape[0])
        if img.dtype != torch.uint8 or tuple(img.shape[1:]) != (3, self.H, self.W) or not 0 < n <= self.batch:
            raise ValueError(f"Validator: img must be uint8 (1..{self.batch}, 3, {self.H}, {self.W})")
        boxes, cls, off = pack_gt(batch["batch_idx"], batch["cls"], batch["bboxes"], n, self.H, self.W)
        if cls.numel() and not (float(cls.min()) > -1 and float(cls.max()) < self.engine.nc):  # as .int() truncates
            raise ValueError(f"Validator: cls outside 0..{self.engine.nc - 1}")
        k = self.pipe.i % self.pipe.depth  # the slot this batch goes to
        sl = self.slots[k]
        if sl.pending is not None:  # the slot's previous batch (and every older one: submission order)
            self._collect_through(k)
        B, M = self.batch, int(boxes.shape[0])
        o_cls = (4 * (B + 1) + 15) // 16 * 16
        o_box = o_cls + (4 * M + 15) // 16 * 16
        total = o_box + 16 * max(M, 1)
        sl.reserve_gt(total, self.device)
        h = sl.gt_host
        hoff = h[:4 * (B + 1)].view(torch.int32)
        hoff[:n + 1] = off
        hoff[n + 1:] = off[n]  # the repeated canvases of a short batch have no GT
        h[o_cls:o_cls + 4 * M].view(torch.float32).copy_(cls)
        h[o_box:o_box + 16 * M].view(torch.float32).copy_(boxes.reshape(-1))
        d = sl.gt_dev
        d[:total].copy_(h[:total], non_blocking=True)  # the batch's GT: one H2D copy
        x = self._canvas(sl, img, n)
        assert self.pipe.submit(x) == k
        nms = self.pipe.nms[k]
        block = self.pipe.slot_block(k)
        with torch.cuda.stream(self.pipe.slot_stream(k)):
            if self.single_cls:
                nms.dets[:, :, 5].zero_()  # val.py:164-165: pred["cls"] *= 0
            gt = (d[o_box:o_box + 16 * max(M, 1)].view(torch.float32).view(-1, 4)[:max(M, 1)],
                  d[o_cls:o_cls + 4 * max(M, 1)].view(torch.float32), d[:4 * (B + 1)].view(torch.int32))
            self.matcher(nms.dets, nms.counts, *gt,
                         out=block[self.pipe.nb:self.pipe.nb + B * self.max_det * 2].view(torch.int16))
            self.confusion[k](nms.dets, nms.counts, *gt, n=n)  # the repeated canvases of a short batch stay out
            sl.out_host.copy_(block, non_blocking=True)  # packed NMS outputs + tp words: one D2H copy
            sl.done.record()
        tcls = cls.numpy()
        o = off.tolist()
        sl.pending = (n, [tcls[o[i]:o[i + 1]].copy() for i in range(n)])
        self._fifo.append(k)
        self.seen += n

    # ------------------------------------------------------------------ host half
    def _collect_through(self, k: int | None) -> None:
        """Read the results of the batches in flight, oldest first, up to and including slot k (None: all)."""
        while self._fifo:
            j = self._fifo.popleft()
            self._collect(self.slots[j])
            if j == k:
                break

    def _collect(self, sl: _Slot) -> None:
        n, tcls = sl.pending
        sl.pending = None
        sl.done.synchronize()
        B, D, nb = self.batch, self.max_det, self.pipe.nb
        host = sl.out_host.numpy()
        _, dets, counts = NMS.unpack(sl.out_host[:nb], B, D)
        dets, counts = dets.numpy(), counts.numpy()
        words = host[nb:nb + B * D * 2].view(np.uint16).reshape(B, D)
        for i in range(n):
            c = int(counts[i])
            t = tcls[i]
            self.metrics.update_stats({
                "tp": unpack_tp(words[i, :c], self.niou),
                "conf": dets[i, :c, 4].copy(),
                "pred_cls": dets[i, :c, 5].copy(),
                "target_cls": t,
                "target_img": np.unique(t),
            })

    def flush(self) -> None:
        """Every submitted batch's statistics are accumulated (`metrics.stats`)."""
        self.pipe.flush()
        self._collect_through(None)

    def stats(self) -> dict:
        """`DetectionValidator.get_stats`: flush, compute, clear; returns `DetMetrics.results_dict`.  The run's
        confusion matrix is left in `self.confusion_matrix` and the device tables are cleared with the statistics."""
        self.flush()
        self.metrics.process()
        self.metrics.clear_stats()
        self.confusion_matrix = ConfusionMatrix(self.cm_names, sum(c.numpy().astype(np.int64) for c in self.confusion))
        for c in self.confusion:
            c.zero_()
        torch.cuda.synchronize(self.device)  # nothing is in flight here: the next run's slot streams see zeros
        return self.metrics.results_dict

    def close(self) -> None:
        try:
            self.pipe.close()
        finally:
            torch.cuda.synchronize(self.device)
            for e in self.pipe.engs:
                e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
