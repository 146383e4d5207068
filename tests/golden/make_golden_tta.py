"""Test-time-augmentation fixtures from the REFERENCE (run where the reference is importable).

    python tests/golden/make_golden_tta.py

Writes tests/golden/tta.npz (data only), three groups:

  * geom/...    the shapes the reference's scale_img (utils/torch_utils.py:476-495) produces for ratios 0.83 and 0.67,
                gs 32: the resized size from F.interpolate and the canvas after the pad, H and W each from SIZES.
  * resize/...  the reference's fp32 scale_img results, with x.flip(3) / x.flip(2) applied first where flipped
                (nn/tasks.py:439), on two seeded random images in [0, 1] pre-rounded to fp16.
  * e2e/...     DetectionModel._predict_augment (nn/tasks.py:422-484) in fp32 on the fused yolo11n-fce with
                seeded_state_dict(keys, SEED) and the Detect cls branches' last conv biases set to 0 (the scores then
                spread around 0.5, so the NMS of the merged tensor has candidates from every pass), inputs pre-rounded
                to fp16.  Rows ROWS of the output are kept (the four box rows and every fourth class row, all
                anchors): the whole tensors would not fit a committed file.
Same import recipe as make_golden.py.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden  # noqa: E402

SIZES = (32, 64, 96, 100, 160, 192, 320, 400, 544, 640, 1280)
RATIOS = (0.83, 0.67)
IMAGES = {"a": ((2, 3, 40, 56), 401), "b": ((1, 3, 37, 53), 402)}  # name: (shape, seed)
SEED = 0  # model weights
E2E = {"192_b2": (2, 192, 192, 1921), "192x160_b2": (2, 192, 160, 1922)}  # key: (batch, H, W, first input seed)
ROWS = np.r_[0:4, 4:84:4]
CONF, MIN_CAND = 0.25, 50


def main():
    torch.set_num_threads(8)
    tasks = make_golden.import_reference()
    make_golden._load_pkg()
    from ultralytics.utils.nms import non_max_suppression
    from ultralytics.utils.torch_utils import scale_img

    from fce_yolo_amd.weights import seeded_state_dict

    out = {}
    # ------------------------------------------------------------------ geometry
    rows = []
    for h in SIZES:
        for w in SIZES:
            x = torch.zeros(1, 1, h, w)
            for r in RATIOS:
                y = scale_img(x, r, gs=32)
                s = torch.nn.functional.interpolate(x, size=(int(h * r), int(w * r)), mode="bilinear", align_corners=False)
                rows.append((h, w, round(r * 100), s.shape[2], s.shape[3], y.shape[2], y.shape[3]))
    out["geom/table"] = np.array(rows, np.int32)  # H, W, ratio * 100, h_s, w_s, H_c, W_c

    # ------------------------------------------------------------------ resize
    for name, (shape, seed) in IMAGES.items():
        x = torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).half().float()
        out[f"resize/{name}/seed"] = np.array(seed)
        out[f"resize/{name}/shape"] = np.array(shape)
        for r in RATIOS:
            for flip in (0, 3, 2):
                y = scale_img(x.flip(flip) if flip else x, r, gs=32)
                out[f"resize/{name}/r{round(r * 100)}_f{flip}"] = y.numpy()
                out[f"resize/{name}/r{round(r * 100)}_size"] = np.array([int(shape[2] * r), int(shape[3] * r)])

    # ------------------------------------------------------------------ end to end
    d = tasks.yaml_model_load(str(make_golden.REF / "ultralytics/cfg/models/11/yolo11n-fce.yaml"))
    model = tasks.DetectionModel(d, ch=3, verbose=False)
    sd = seeded_state_dict([(k, v.shape) for k, v in model.state_dict().items()], seed=SEED)
    det = len(model.model) - 1
    nl = model.model[-1].nl
    for i in range(nl):
        sd[f"model.{det}.cv3.{i}.2.bias"] = torch.zeros_like(sd[f"model.{det}.cv3.{i}.2.bias"])
    model.load_state_dict(sd)
    model.eval()
    model.fuse(verbose=False)
    for key, (bs, H, W, seed0) in E2E.items():
        found = None
        for xs in range(seed0, seed0 + 50):
            x = torch.rand(bs, 3, H, W, generator=torch.Generator().manual_seed(xs)).half().float()
            with torch.inference_mode():
                parts = []
                for si, fi in zip([1, 0.83, 0.67], [None, 3, None]):  # the pass sizes, to know the segments
                    parts.append(scale_img(x.flip(fi) if fi else x, si, gs=32).shape[2:])
                y, _ = model._predict_augment(x)
            # segments of the merged anchor axis (tasks.py:468-484)
            cnt = [sum((h // s) * (w // s) for s in (8, 16, 32)) for h, w in parts]
            g = sum(4 ** k for k in range(nl))
            seg = [cnt[0] - cnt[0] // g, cnt[1], cnt[2] - (cnt[2] // g) * 4 ** (nl - 1)]
            assert sum(seg) == y.shape[2], (seg, y.shape)
            off = np.concatenate(([0], np.cumsum(seg)))
            sc = y[:, 4:].max(1).values.numpy()
            ncand = [[int((sc[b, off[k]:off[k + 1]] > CONF).sum()) for k in range(3)] for b in range(bs)]
            _, keep = non_max_suppression(y.clone(), CONF, 0.7, max_det=300, return_idxs=True)
            kept = [[int(((kb.numpy() >= off[k]) & (kb.numpy() < off[k + 1])).sum()) for k in range(3)] for kb in keep]
            print(key, "x_seed", xs, "segments", seg, "candidates", ncand, "kept per segment", kept, flush=True)
            if min(min(c) for c in ncand) >= MIN_CAND and min(min(c) for c in kept) >= 1:
                found = (xs, y, seg)
                break
        assert found, f"{key}: no input seed gives {MIN_CAND} candidates and a kept detection in every segment"
        xs, y, seg = found
        out[f"e2e/{key}/x_seed"] = np.array(xs)
        out[f"e2e/{key}/shape"] = np.array([bs, 3, H, W])
        out[f"e2e/{key}/segments"] = np.array(seg)
        out[f"e2e/{key}/rows"] = ROWS
        out[f"e2e/{key}/y_rows"] = y.numpy()[:, ROWS].copy()
    out["e2e/model_seed"] = np.array(SEED)
    np.savez_compressed(HERE / "tta.npz", **out)
    print("tta.npz", (HERE / "tta.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
