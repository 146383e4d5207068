"""Cost of test-time augmentation (tta.AugmentedEngine) on the device, for DESIGN.md "Test-time augmentation".

    python scripts/tta_bench.py [--cfg yolo11n-fce.yaml] [--batch 32] [--imgsz 640] [--iters 200]

Prints one JSON line: the time of one augmented forward (three hipGraph replays, two scale kernels, one merge) beside
the three plain forwards at the passes' canvases timed one by one, and the two new kernels alone against their
algorithmic bytes (scale: one read of the source, one write of the canvas; merge: one read and one write of
(4 + nc) * 4 + 8 bytes per kept anchor).  Times are device events around `iters` back-to-back calls after a warm-up.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import fce_pkg  # noqa: E402

fce_pkg.load()
from fce_yolo_amd import tta  # noqa: E402
from fce_yolo_amd.parser import DetectionModel  # noqa: E402
from fce_yolo_amd.weights import seeded_state_dict  # noqa: E402


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="yolo11n-fce.yaml")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = DetectionModel(a.cfg)
    model.load_state_dict(seeded_state_dict([(k, v.shape) for k, v in model.state_dict().items()], 0))
    model.eval().to(dev)
    B, S = a.batch, a.imgsz
    aug = tta.AugmentedEngine(model, B, S, dev, graph=True)
    x8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev)
    x16 = x8.half() / 255
    res = {"cfg": a.cfg, "batch": B, "imgsz": S, "canvases": [[e.H, e.W] for e in aug.engines],
           "anchors": aug.anchors, "segments": [c for _, c in aug.ranges]}
    for name, x in (("u8", x8), ("f16", x16)):
        res[f"augmented_ms_{name}"] = timed(lambda: aug(x), a.iters)
    plain = []
    for i, e in enumerate(aug.engines):
        xi = x16 if i == 0 else aug.canvas[i]
        plain.append(timed(lambda: e(xi, graph=True), a.iters))
    res["plain_ms"] = plain
    res["plain_sum_ms"] = sum(plain)
    rows = 4 + aug.nc
    for i in (1, 2):
        h_s, w_s, H_c, W_c = aug.geom[i]
        for name, x in (("u8", x8), ("f16", x16)):
            ms = timed(lambda: tta.scale_img(x, aug.canvas[i], tta.FLIPS[i], h_s, w_s), a.iters)
            nbytes = x.numel() * x.element_size() + aug.canvas[i].numel() * 2
            res[f"scale{i}_{name}"] = {"ms": ms, "bytes": nbytes, "GBps": nbytes / ms * 1e-6}
    parts = [(e.pred, e.best, f, c, s, fl, S, S)
             for e, (f, c), s, fl in zip(aug.engines, aug.ranges, tta.SCALES, tta.FLIPS)]
    ms = timed(lambda: tta.merge(parts, aug.pred, aug.best), a.iters)
    nbytes = 2 * B * aug.anchors * (rows * 4 + 8)
    res["merge"] = {"ms": ms, "bytes": nbytes, "GBps": nbytes / ms * 1e-6}
    res["merge_share_of_augmented"] = ms / res["augmented_ms_u8"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
