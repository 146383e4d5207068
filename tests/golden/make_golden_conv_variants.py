"""Record the conv candidate lists (fce_conv_variants, fce_net_op_variants) of a built libfceyolo.so
into tests/golden/conv_variants.json.  The fixture pins the lists a refactor of the conv dispatch must
keep: it is regenerated only on a commit whose lists are meant to change.

    python tests/golden/make_golden_conv_variants.py [--out PATH]      # host grids + the planned net (needs a GPU)
    python tests/golden/make_golden_conv_variants.py --host-only       # host grids, keeps the recorded net lists
    python tests/golden/make_golden_conv_variants.py --full ENV        # print one env set's full lists, for diffing

Host grids (cap 128, det_box 0), one fresh child process per env set (FCE_NO_RING is read once per process):
dense cin x cout x k x stride x up (k = 1) x in_w, depthwise c x in_w x stride.  `lists` is the table of distinct
candidate lists, in full; an env set's `entries` index it, in grid order (host_lists() gives the keys); `truncated`
holds one cap-16 call.
`net_ops` maps every conv / conv-detect op of yolo11n-fce at 160x160, batch 2, planned without autotuning (the only
way to reach the det_box lists) to its full list in `net_lists`.
"""

from __future__ import annotations

import argparse
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
FIXTURE = ROOT / "tests" / "golden" / "conv_variants.json"

ENV_KNOBS = ("FCE_TILE3AL", "FCE_WIDE3", "FCE_RING32", "FCE_NO_GEMM3", "FCE_NO_DRING", "FCE_NO_RING")
ENV_SETS = {
    "default": {},
    "optin": {"FCE_TILE3AL": "1", "FCE_WIDE3": "1", "FCE_RING32": "1"},
    "no_gemm3": {"FCE_NO_GEMM3": "1"},
    "no_dring": {"FCE_NO_DRING": "1"},
    "no_ring": {"FCE_NO_RING": "1"},
}
CAP = 128
TRUNCATED = (64, 64, 3, 1, 0, 80, 16)  # cin, cout, k, stride, up, in_w, cap: more than 16 candidates


def _native():
    """fce_yolo_amd/_native.py alone (ctypes only): the children need neither torch nor the package."""
    spec = importlib.util.spec_from_file_location("fce_native_golden", ROOT / "fce-yolo_amd" / "_native.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dense_grid():
    for cin in (8, 16, 32, 48, 64, 96, 128, 256, 512):
        for cout in (16, 32, 64, 96, 128, 256, 512):
            for k in (1, 3):
                for stride in (1, 2):
                    for up in ((0, 1) if k == 1 else (0,)):
                        for in_w in (20, 80):
                            yield cin, cout, k, stride, up, in_w


def dw_grid():
    for c in (16, 64, 128):
        for in_w in (20, 40, 80, 160):
            for stride in (1, 2):
                yield c, in_w, stride


def variants(N, cin, cout, k, stride, groups, up, in_w, cap=CAP):
    d = N.ConvDesc(cin, cout, k, stride, groups, 1, up, 0, None, 0, 0)
    codes = (C.c_int * cap)()
    nv = N.lib().fce_conv_variants(C.byref(d), in_w, codes, cap)
    return list(codes[:nv])


def host_lists():
    """{key: codes} of both grids, in this process's environment."""
    N = _native()
    out = {}
    for cin, cout, k, stride, up, in_w in dense_grid():
        out[f"{cin},{cout},{k},{stride},{up},{in_w}"] = variants(N, cin, cout, k, stride, 1, up, in_w)
    for c, in_w, stride in dw_grid():
        out[f"dw{c},{in_w},{stride}"] = variants(N, c, c, 3, stride, c, 0, in_w)
    cin, cout, k, stride, up, in_w, cap = TRUNCATED
    out["truncated"] = variants(N, cin, cout, k, stride, 1, up, in_w, cap)
    return out


def child_lists(name):
    """host_lists() of env set `name`, from a fresh child process."""
    env = {k: v for k, v in os.environ.items() if k not in ENV_KNOBS}
    env.update(ENV_SETS[name])
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], capture_output=True, text=True,
                       env=env, timeout=120)
    if r.returncode != 0:
        raise RuntimeError(f"child for env set {name} failed:\n{r.stderr}")
    return json.loads(r.stdout)


def intern(table, item):
    """Index of `item` in `table`, appended if new."""
    if item not in table:
        table.append(item)
    return table.index(item)


def host_record(table):
    rec = {}
    for name in ENV_SETS:
        lists = child_lists(name)
        trunc = lists.pop("truncated")
        rec[name] = {"entries": [intern(table, v) for v in lists.values()], "truncated": trunc}
    return rec


def net_ops():
    """{op index: codes} of the smoke() model, planned without autotuning (GPU)."""
    import torch

    sys.path.insert(0, str(ROOT))
    import fce_pkg

    fce_pkg.load()
    from fce_yolo_amd.engine import Engine
    from fce_yolo_amd.parser import DetectionModel
    from fce_yolo_amd.weights import seeded_state_dict

    dev = torch.device("cuda:0")
    model = DetectionModel("yolo11n-fce.yaml")
    model.load_state_dict(seeded_state_dict([(k, v.shape) for k, v in model.state_dict().items()], 0))
    model.eval().to(dev)
    eng = Engine(model, 2, 160, dev, autotune=False)
    out = {}
    for i in range(eng.num_ops()):
        codes = eng.variants(i)
        if codes:
            out[str(i)] = codes
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="print this process's host lists as JSON")
    ap.add_argument("--full", metavar="ENV", choices=list(ENV_SETS), help="print one env set's full lists")
    ap.add_argument("--host-only", action="store_true", help="keep the recorded net_ops (no GPU)")
    ap.add_argument("--out", type=Path, default=FIXTURE)
    a = ap.parse_args()
    if a.child:
        json.dump(host_lists(), sys.stdout)
        return
    if a.full:
        for k, v in child_lists(a.full).items():
            print(k, " ".join(hex(c) for c in v))
        return
    rec = {"cap": CAP, "truncated_call": list(TRUNCATED), "lists": []}
    rec["host"] = host_record(rec["lists"])
    if a.host_only:
        old = json.loads(FIXTURE.read_text())
        rec["net_lists"], rec["net_ops"] = old["net_lists"], old["net_ops"]
    else:
        rec["net_lists"] = []
        rec["net_ops"] = {i: intern(rec["net_lists"], codes) for i, codes in net_ops().items()}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(rec, separators=(",", ":")) + "\n")
    print(f"wrote {a.out}: {a.out.stat().st_size} bytes, {len(rec['net_ops'])} net ops")


if __name__ == "__main__":
    main()
