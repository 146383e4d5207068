"""Test-time augmentation: the reference's ``predict(augment=True)`` on the device.

``DetectionModel._predict_augment`` (reference ``nn/tasks.py:422-484``) runs the batch at scale 1, at scale 0.83
flipped left-right and at scale 0.67, de-scales and un-flips each pass's boxes, drops the P5 tail of the large pass
and the P3 head of the small one, and concatenates the three predictions along the anchor axis for one NMS.
``AugmentedEngine`` owns one ``Engine`` per pass at that pass's canvas and presents them as one executor:

    x --------------------------------------------> Engine 0 (H x W) ----------> pred 0, keys 0 --+
    x --(fce_tta_scale_img: flip 3, 0.83, pad)----> Engine 1 (canvas 1) -------> pred 1, keys 1 --+--(fce_tta_merge)--> pred, keys
    x --(fce_tta_scale_img: 0.67, pad)------------> Engine 2 (canvas 2) -------> pred 2, keys 2 --+

The geometry is the reference's Python arithmetic, unchanged (``utils/torch_utils.py:476-495`` scale_img).
"""

from __future__ import annotations

import ctypes as C
import math

import torch

from . import _native as N
from .engine import _DT, Engine

SCALES = (1, 0.83, 0.67)  # tasks.py:435
FLIPS = (None, 3, None)  # tasks.py:436 (2 = up-down, 3 = left-right)
PAD_VALUE = 0.447  # torch_utils.py:495 (the imagenet mean)


def scale_geometry(H: int, W: int, ratio: float, gs: int = 32):
    """torch_utils.py:476-495: (h_s, w_s) the resized size, (H_c, W_c) the padded canvas of a pass at `ratio`."""
    if ratio == 1.0:
        return H, W, H, W
    h_s, w_s = int(H * ratio), int(W * ratio)
    H_c, W_c = (math.ceil(x * ratio / gs) * gs for x in (H, W))
    return h_s, w_s, H_c, W_c


def clip_ranges(anchor_counts, nl: int = 3):
    """tasks.py:468-484 _clip_augmented: the (first, count) anchor range each pass keeps.  The first pass loses its
    last A // g anchors (the P5 level of a square-pyramid count), the last pass its first (A // g) * 4 ** (nl - 1)
    (the P3 level); g = sum of 4 ** x over the levels."""
    counts = list(anchor_counts)
    g = sum(4 ** x for x in range(nl))
    e = 1  # exclude layer count
    ranges = [(0, a) for a in counts]
    i = (counts[0] // g) * sum(4 ** x for x in range(e))
    ranges[0] = (0, ranges[0][1] - i) if i else (0, 0)  # y[..., :-0] is empty
    i = (counts[-1] // g) * sum(4 ** (nl - 1 - x) for x in range(e))
    first, count = ranges[-1]
    ranges[-1] = (first + min(i, count), count - min(i, count))
    return ranges


def scale_img(x: torch.Tensor, out: torch.Tensor, flip, h_s: int, w_s: int, pad: float = PAD_VALUE, stream=None):
    """fce_tta_scale_img: `x` (B, 3, H, W) f16 / f32 / u8 -> `out` (B, 3, H_c, W_c) f16 on the current stream."""
    assert x.is_contiguous() and out.is_contiguous() and out.dtype == torch.float16 and x.dtype in _DT
    b, c, h, w = x.shape
    tx = N.Tensor(x.data_ptr(), _DT[x.dtype], N.NCHW, b, c, h, w, c, 0)
    ty = N.Tensor(out.data_ptr(), N.F16, N.NCHW, out.shape[0], out.shape[1], out.shape[2], out.shape[3], out.shape[1], 0)
    if stream is None:
        stream = torch.cuda.current_stream(x.device).cuda_stream
    N.call("fce_tta_scale_img", C.byref(tx), C.byref(ty), int(flip or 0), h_s, w_s, float(pad), stream)
    return out


def merge(parts, out: torch.Tensor, best: torch.Tensor | None = None, stream=None):
    """fce_tta_merge: `parts` = [(pred (B, R, A_i) f32, best (B, A_i) i64 or None, first, count, scale, flip, img_h,
    img_w)] -> `out` (B, R, sum count) f32 and `best` (B, sum count) i64, on the current stream."""
    arr = (N.TtaPart * max(len(parts), 1))()
    for i, (p, k, first, count, scale, flip, ih, iw) in enumerate(parts):
        assert p.is_contiguous() and p.dtype == torch.float32 and p.shape[:2] == out.shape[:2]
        assert k is None or (k.is_contiguous() and k.dtype == torch.int64 and tuple(k.shape) == (p.shape[0], p.shape[2]))
        arr[i] = N.TtaPart(p.data_ptr(), k.data_ptr() if k is not None else None, p.shape[2], first, count, scale,
                           int(flip or 0), ih, iw)
    total = sum(p[3] for p in parts)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape[2] == total
    assert best is None or (best.is_contiguous() and best.dtype == torch.int64 and tuple(best.shape) == (out.shape[0], total))
    if stream is None:
        stream = torch.cuda.current_stream(out.device).cuda_stream
    N.call("fce_tta_merge", arr, len(parts), out.shape[0], out.shape[1], out.data_ptr(),
           best.data_ptr() if best is not None else None, stream)
    return out


class AugmentedEngine:
    """The three-pass augmented forward as one executor with the `Engine` surface that `NMS`, `Pipeline` lanes and
    `predict.Predictor` use: `.pred` is the merged (B, 4 + nc, A_total) tensor, `.anchors` = A_total.  Each pass has
    its own `Engine` (its own arena, plan and captured hipGraph), also when two passes share a canvas: they run on
    different data in the same call."""

    def __init__(self, model, batch: int, imgsz: int | tuple[int, int], device=None, graph: bool = False,
                 autotune: bool | None = None, _engines=None):
        if isinstance(imgsz, int):
            imgsz = (imgsz, imgsz)
        self.H, self.W = imgsz
        self.batch, self.model, self.graph = batch, model, graph
        gs = int(max(float(s) for s in model.stride))
        self.geom = [scale_geometry(self.H, self.W, s, gs) for s in SCALES]
        if _engines is None:
            _engines = [Engine(model, batch, (hc, wc), device, graph=graph, autotune=autotune)
                        for (_, _, hc, wc) in self.geom]
        self.engines = list(_engines)
        e0 = self.engines[0]
        self.device, self.nc = e0.device, e0.nc
        nl = model.model[-1].nl
        self.ranges = clip_ranges([e.anchors for e in self.engines], nl)
        self.anchors = sum(c for _, c in self.ranges)
        # the scaled passes' network inputs (pass 0 reads the caller's x)
        self.canvas = [None] + [torch.empty((batch, 3, e.H, e.W), dtype=torch.float16, device=self.device)
                                for e in self.engines[1:]]
        self.pred = torch.empty((batch, 4 + self.nc, self.anchors), dtype=torch.float32, device=self.device)
        self.best = self.new_best()

    def new_best(self) -> torch.Tensor:
        return torch.zeros((self.batch, self.anchors), dtype=torch.int64, device=self.device)

    def close(self):
        for e in self.engines:
            e.close()

    def __call__(self, x: torch.Tensor, out: torch.Tensor | None = None, graph: bool | None = None,
                 best: torch.Tensor | None = None) -> torch.Tensor:
        """Augmented forward into `out` (default: self.pred, with the merged best-class keys in self.best), on the
        current stream.  `best`: a new_best() buffer for the keys of this forward."""
        if out is None:
            out, best = self.pred, self.best if best is None else best
        assert tuple(out.shape) == tuple(self.pred.shape)
        g = self.graph if graph is None else graph
        self.engines[0]._in(x)  # dtype, shape and device are right before anything is launched
        parts = []
        for i, (eng, s, f) in enumerate(zip(self.engines, SCALES, FLIPS)):
            xi = x if i == 0 else scale_img(x, self.canvas[i], f, *self.geom[i][:2])
            eng(xi, graph=g)  # into the pass's own pred and keys
            first, count = self.ranges[i]
            parts.append((eng.pred, eng.best if best is not None else None, first, count, s, f, self.H, self.W))
        return merge(parts, out, best)

    def clone(self) -> "AugmentedEngine":
        """A second executor with its own arenas, every pass pinned to this one's kernel variants (`Engine.clone`)."""
        return AugmentedEngine(self.model, self.batch, (self.H, self.W), self.device, graph=self.graph,
                               _engines=[e.clone() for e in self.engines])
