"""CPU restatements of the two test-time-augmentation kernels (csrc/tta.hip) and of the augmented forward.

`scale_img_ref` is fce_tta_scale_img operation by operation (torch CPU ops round every fp32 operation on its own,
as the kernel does with contraction off), so the kernel is compared with it bit for bit; against the reference's own
fp32 `scale_img` it differs by fp32 rounding only (golden/tta.npz).  `merge_ref` is fce_tta_merge in fp32.
`predict_augment_ref` drives `cases.oracle_model` three times and merges: the reference's
DetectionModel._predict_augment (nn/tasks.py:422-484) without a GPU.
"""

from __future__ import annotations

import numpy as np
import torch

import cases
from fce_yolo_amd import tta

GOLDEN_KEY_ROWS = np.r_[0:4, 4:84:4]  # rows of the end-to-end output golden/tta.npz keeps (make_golden_tta.ROWS)


def model_zero_cls_bias(seed: int):
    """cases.seeded_model("yolo11n-fce.yaml", seed) with the Detect cls branches' last conv biases set to 0
    (make_golden_tta.py: the scores then spread around 0.5 instead of sitting under conf 0.25)."""
    model = cases.seeded_model("yolo11n-fce.yaml", seed)
    with torch.no_grad():
        for branch in model.model[-1].cv3:
            branch[2].bias.zero_()
    return model


def fp16_source(x: torch.Tensor) -> torch.Tensor:
    """What the kernel reads: f16 as is, f32 rounded to fp16, u8 as fp16(v / 255); returned as fp32."""
    if x.dtype == torch.uint8:
        return (x.float() / 255).half().float()
    return x.half().float()


def _axis(n_out: int, n_in: int):
    """ATen's align_corners=False source index and weights for an explicit output size, in fp32."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    d = torch.arange(n_out, dtype=torch.float32)
    src = ((d + 0.5) * scale - 0.5).clamp_min(0)
    i0 = src.to(torch.int64).clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l1 = src - i0.float()
    l0 = 1 - l1
    return i0, i1, l0, l1


def scale_img_ref(x: torch.Tensor, flip, h_s: int, w_s: int, H_c: int, W_c: int, pad: float = tta.PAD_VALUE,
                  round_fp16: bool = True) -> torch.Tensor:
    """fce_tta_scale_img: flip (None / 0, 2 up-down, 3 left-right), bilinear resize to (h_s, w_s), pad to (H_c, W_c).
    fp16 result; `round_fp16=False` keeps the fp32 values (and the fp32 pad), the reference's fp32 scale_img."""
    xs = fp16_source(x) if round_fp16 else x.float()
    if flip:
        xs = xs.flip(flip)
    H, W = xs.shape[2:]
    y0, y1, l0h, l1h = _axis(h_s, H)
    x0, x1, l0w, l1w = _axis(w_s, W)
    r0, r1 = xs[:, :, y0], xs[:, :, y1]
    a, b, c, d = r0[..., x0], r0[..., x1], r1[..., x0], r1[..., x1]
    top = l0w * a + l1w * b
    bot = l0w * c + l1w * d
    v = l0h[:, None] * top + l1h[:, None] * bot
    out = torch.full((*xs.shape[:2], H_c, W_c), pad, dtype=torch.float32)
    out[:, :, :h_s, :w_s] = v
    return out.half() if round_fp16 else out


def merge_ref(parts, with_best: bool = True):
    """fce_tta_merge: parts = [(pred (B, R, A_i) f32, best (B, A_i) i64 or None, first, count, scale, flip, img_h,
    img_w)] -> (pred (B, R, sum count), best (B, sum count) or None)."""
    preds, bests = [], []
    for p, k, first, count, scale, flip, ih, iw in parts:
        q = p[:, :, first:first + count].clone()
        q[:, :4] = q[:, :4] / torch.tensor(scale, dtype=torch.float32)
        if flip == 3:
            q[:, 0] = iw - q[:, 0]
        elif flip == 2:
            q[:, 1] = ih - q[:, 1]
        preds.append(q)
        if with_best:
            bests.append(k[:, first:first + count])
    return torch.cat(preds, 2), (torch.cat(bests, 1) if with_best else None)


def pass_images(x: torch.Tensor, gs: int = 32, round_fp16: bool = True):
    """The three passes' network inputs [(image, scale, flip)] for a batch x (pass 0 is x itself)."""
    H, W = x.shape[2:]
    out = []
    for s, f in zip(tta.SCALES, tta.FLIPS):
        if s == 1 and not f:
            out.append((x, s, f))
        else:
            out.append((scale_img_ref(x, f, *tta.scale_geometry(H, W, s, gs), round_fp16=round_fp16), s, f))
    return out


def predict_augment_ref(model, x: torch.Tensor, dtype=torch.float32, round_fp16: bool = False):
    """tasks.py:422-444 on the CPU oracle: (merged pred fp32, [(first, count)] per pass).  `round_fp16`: the scaled
    images are rounded to fp16 as the device path's are (off: the reference's fp32 pipeline)."""
    gs = int(max(float(s) for s in model.stride))
    H, W = x.shape[2:]
    ys = [(cases.oracle_model(model, xi.float(), dtype).float(), s, f) for xi, s, f in pass_images(x, gs, round_fp16)]
    ranges = tta.clip_ranges([y.shape[2] for y, _, _ in ys], model.model[-1].nl)
    parts = [(y, None, first, count, s, f, H, W) for (y, s, f), (first, count) in zip(ys, ranges)]
    return merge_ref(parts, with_best=False)[0], ranges
