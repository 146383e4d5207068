"""Per-op autotune report of the bench workload: chosen kernel variant, and every candidate's time.

    python scripts/tune_report.py [--model yolo11n-fce.yaml] [--batch 32] [--imgsz 640] > report.txt
Variant codes: kind = (code >> 8) & 15 names the kernel family, in the order of the kFamilies table of
csrc/conv.hip (which is also the order of the candidates below): 0 implicit GEMM, 3 1x1 streaming, 4 1x1 LDS tile,
5 1x1 ring, 0xB 1x1 256-wide tile, 7 1x1 big tile (K-pipelined), 2 3x3 LDS tile (small cin), 6 3x3 ring,
0xD 3x3 LDS-DMA ring, 9 3x3 32x32x16 ring, 1 3x3 LDS tile (cin % 32 == 0), 8 3x3 LDS-DMA big tile,
0xC 3x3 256-wide implicit GEMM, 0xA 3x3 wide tile; 100 + v is depthwise variant v.  The other bits are the
family's own: the encode / decode pair in the family's file under csrc/ (csrc/conv_variant.h lists them) is the
authority.
"""
import argparse
import ctypes as C
import sys
from collections import defaultdict
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import fce_pkg  # noqa: E402

fce_pkg.load()
from fce_yolo_amd import _native as N  # noqa: E402
from fce_yolo_amd.engine import Engine  # noqa: E402
from fce_yolo_amd.parser import DetectionModel  # noqa: E402
from fce_yolo_amd.weights import seeded_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="yolo11n-fce.yaml")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--imgsz", type=int, default=640)
a = ap.parse_args()
dev = torch.device("cuda:0")
from bench import model_cfg  # noqa: E402  (the "-h8" BASELINE config)

model = DetectionModel(model_cfg(a.model))
model.load_state_dict(seeded_state_dict([(k, v.shape) for k, v in model.state_dict().items()], 0))
model.eval().to(dev)
eng = Engine(model, a.batch, a.imgsz, dev)
L = N.lib()
recs = defaultdict(list)
k = 0
op, code, ms = C.c_int(), C.c_int(), C.c_float()
while L.fce_net_tune_record(eng.net, k, C.byref(op), C.byref(code), C.byref(ms)):
    recs[op.value].append((code.value, ms.value * 1e3))
    k += 1
for i in range(eng.num_ops()):
    name, nbytes, flops = eng.op_info(i)
    ch = L.fce_net_op_variant(eng.net, i)
    cands = " ".join(f"{c:#x}:{t:.1f}" for c, t in sorted(recs.get(i, []), key=lambda r: r[1]))
    print(f"{i:3d} {name:20s} {nbytes / 1e6:7.2f}MB {flops / 1e9:6.2f}GF chosen {ch:#6x} | {cands}", flush=True)
