"""Throughput of validation on the device (val.Validator), for DESIGN.md "Validation".

    python scripts/val_bench.py [--cfg yolo11n-fce.yaml] [--batch 32] [--imgsz 640] [--gt 20] [--batches 60]

Resident u8 canvases, `--gt` GT boxes per image (half of them jittered copies of the model's own detections, so the
matching has true positives).  Prints one JSON line with images/s of
  (a) validator     Validator.update per batch + flush: forward, NMS (conf 0.001, multi_label), fce_val_match, one
                    D2H copy per batch, the host unpacking the tp words;
  (b) pipeline      the same Pipeline (same lanes, same NMS) with no matching and no copy to the host;
  (c) host_match    (b) plus, per batch, the NMS outputs copied to the host and matched per image in numpy
                    (tests/val_ref.py: the reference's per-image loop without its per-image sync);
and the device times of one fce_val_match, of one fce_val_confusion and of one NMS at these settings per batch (events
around back-to-back calls on a finished batch's data).
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import fce_pkg  # noqa: E402

fce_pkg.load()
import val_ref  # noqa: E402
from fce_yolo_amd import val as V  # noqa: E402
from fce_yolo_amd.engine import NMS, Pipeline  # noqa: E402
from fce_yolo_amd.parser import DetectionModel  # noqa: E402
from fce_yolo_amd.predict import default_lanes  # noqa: E402
from fce_yolo_amd.weights import seeded_state_dict  # noqa: E402


def timed(fn, iters, warmup=10):
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
    ap.add_argument("--gt", type=int, default=20)
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--lanes", type=int, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = DetectionModel(a.cfg)
    model.load_state_dict(seeded_state_dict([(k, v.shape) for k, v in model.state_dict().items()], 0))
    model.eval().to(dev)
    B, S, G = a.batch, a.imgsz, a.gt
    lanes = a.lanes or default_lanes(model)
    nms_kw = dict(conf=0.001, iou=0.7, max_det=300, multi_label=True)
    gen = torch.Generator().manual_seed(3)
    canv = [torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, generator=gen).to(dev) for _ in range(4)]
    res = {"cfg": a.cfg, "batch": B, "imgsz": S, "gt_per_image": G, "lanes": lanes, "batches": a.batches}

    with V.Validator(model, B, S, dev, lanes=lanes) as v:
        eng = v.engine
        # labels from a first plain run
        rng = np.random.default_rng(4)
        labels = []
        with Pipeline(eng, lanes=1, defer=False, **nms_kw) as p1:
            for x in canv:
                dets, _ = p1.results(p1.submit(x))
                rows = []
                for i, d in enumerate(dets):
                    d = d.cpu().numpy()
                    k = min(G // 2, len(d))
                    pick = rng.choice(len(d), k, replace=False) if k else np.zeros(0, int)
                    wh = np.concatenate([d[pick, 2:4] - d[pick, 0:2]] * 2, 1)
                    jit = d[pick, :4] + rng.uniform(-0.05, 0.05, (k, 4)) * wh
                    w, h = rng.uniform(16, 200, G - k), rng.uniform(16, 200, G - k)
                    x1, y1 = rng.uniform(0, S - w), rng.uniform(0, S - h)
                    xyxy = np.concatenate([jit, np.stack([x1, y1, x1 + w, y1 + h], 1)]) / S
                    xywh = np.concatenate([(xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]], 1)
                    cls = np.concatenate([d[pick, 5], rng.integers(0, 80, G - k)])
                    rows.append(np.concatenate([np.full((G, 1), i), cls[:, None], xywh], 1))
                r = torch.from_numpy(np.concatenate(rows).astype(np.float32))
                labels.append({"batch_idx": r[:, 0], "cls": r[:, 1:2], "bboxes": r[:, 2:]})
                res.setdefault("detections_per_image", []).append(float(np.mean([len(d) for d in dets])))
        res["detections_per_image"] = float(np.mean(res["detections_per_image"]))

        # (a) the Validator
        def run_a(n):
            for i in range(n):
                v.update({"img": canv[i % 4], **labels[i % 4]})
            v.flush()

        run_a(2 * lanes)
        v.metrics.clear_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_a(a.batches)
        ta = time.perf_counter() - t0
        t0 = time.perf_counter()
        out = v.stats()
        res["stats_s"] = time.perf_counter() - t0
        res["results"] = out
        res["validator_img_s"] = a.batches * B / ta

        # the kernels alone, on the last batch's data
        k = (v.pipe.i - 1) % v.pipe.depth
        nms, sl = v.pipe.nms[k], v.slots[k]
        gt = V.pack_gt(labels[0]["batch_idx"], labels[0]["cls"], labels[0]["bboxes"], B, S, S)
        gb, gc, off = (t.to(dev) for t in gt)
        res["val_match_ms"] = timed(lambda: v.matcher(nms.dets, nms.counts, gb, gc, off), 200)
        # the confusion matrix at the validator's threshold (0.25) and with every detection taking part (0.001)
        cm = v.confusion[k]
        res["val_confusion_ms"] = timed(lambda: cm(nms.dets, nms.counts, gb, gc, off), 200)
        res["participating_per_image"] = float((nms.dets[:, :, 4] > cm.conf).sum().item()) / B
        every = V.DeviceConfusionMatrix(eng.nc, B, 300, dev, conf=0.001)
        res["val_confusion_all_detections_ms"] = timed(lambda: every(nms.dets, nms.counts, gb, gc, off), 200)
        for c in v.confusion:
            c.zero_()
        pred, best = v.pipe.preds[k], v.pipe.bests[k]
        res["nms_conf001_multilabel_ms"] = timed(lambda: nms(pred, best), 50)
        std = NMS(B, eng.anchors, eng.nc, dev)
        res["nms_conf025_ms"] = timed(lambda: std(pred, best), 50)

        # (b) the same pipeline without matching, (c) with the matching on the host
        with Pipeline(eng, depth=max(lanes, 2), defer=False, lanes=lanes, **nms_kw) as pipe:
            def run_b(n):
                for i in range(n):
                    pipe.submit(canv[i % 4])
                pipe.flush()
                torch.cuda.synchronize()

            run_b(2 * lanes)
            t0 = time.perf_counter()
            run_b(a.batches)
            res["pipeline_img_s"] = a.batches * B / (time.perf_counter() - t0)

            host_gt = [V.pack_gt(lb["batch_idx"], lb["cls"], lb["bboxes"], B, S, S) for lb in labels]
            host_gt = [(b.numpy(), c.numpy(), o.tolist()) for b, c, o in host_gt]

            def collect(k, i):
                pipe.check_posted(k)
                pipe.nms_done[k].synchronize()
                _, dets, counts = NMS.unpack(pipe.slot_block(k)[:pipe.nb].cpu(), B, 300)
                dets, counts = dets.numpy(), counts.numpy()
                b, c, o = host_gt[i % 4]
                for j in range(B):
                    d = dets[j, :counts[j]]
                    val_ref.match_image(d[:, :4], d[:, 5], b[o[j]:o[j + 1]], c[o[j]:o[j + 1]])

            def run_c(n):
                q = []
                for i in range(n):
                    if len(q) == pipe.depth:
                        collect(*q.pop(0))
                    q.append((pipe.submit(canv[i % 4]), i))
                pipe.flush()
                for item in q:
                    collect(*item)

            run_c(lanes)
            nb = max(lanes, a.batches // 4)
            t0 = time.perf_counter()
            run_c(nb)
            res["host_match_img_s"] = nb * B / (time.perf_counter() - t0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
