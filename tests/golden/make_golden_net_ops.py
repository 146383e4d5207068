"""Record what the fce_net executor of a built libfceyolo.so makes of the shipped models into
tests/golden/net_ops.json.  The fixture pins the op list, the plan's choices and the cost model that a refactor of
the executor must keep: it is regenerated only on a commit whose op lists, plans or costs are meant to change.

    python tests/golden/make_golden_net_ops.py [--out PATH]      # host lists + the planned nets (needs a GPU)
    python tests/golden/make_golden_net_ops.py --host-only       # host lists, keeps the recorded plans

`host`: per env set (one fresh child process each) and per config, the ops of the model lowered into a NetBackend on
the CPU (recorded, never planned): [name, alt_form, c3k2_form, skipped] with the name as an index into `names`.
`plans`: per config at batch 2 and per size, planned without autotuning: [name, bytes, flops, alt_form, skipped,
variant, variants] per op, the variants as an index into `lists`, and `locked`, the ops whose fused form
fce_net_set_alt_form refuses.  `tune`: the (op, code) sequence of fce_net_tune_record after an autotuned plan.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
FIXTURE = ROOT / "tests" / "golden" / "net_ops.json"

FUSE_KNOBS = ("FCE_FUSE_STEM", "FCE_FUSE_DCLS", "FCE_FUSE_C3K2", "FCE_FUSE_BNECK", "FCE_FUSE_PW2")
ENV_SETS = {
    "default": {},
    "unfused": {k: "0" for k in FUSE_KNOBS},
    "no_c3k2": {"FCE_FUSE_C3K2": "0"},
}
HOST_CONFIGS = ("yolo11n-fce.yaml", "yolo11s-bifpn.yaml", "yolo11l-fce.yaml", "yolo11m-fce-h8.yaml")
PLAN_CONFIGS = ("yolo11n-fce.yaml", "yolo11s-bifpn.yaml")
PLAN_BATCH = 2
PLAN_SIZES = (160, 224, 704)  # 704: wider than the fused stem pair is built for
TUNE = ("yolo11n-fce.yaml", 160)


def _imports():
    for p in (ROOT, ROOT / "tests"):
        if str(p) not in sys.path:
            sys.path.insert(0, str(p))
    import cases
    from fce_yolo_amd import _native as N

    return cases, N


def host_ops(cfg):
    """[[name, alt_form, c3k2_form, skipped]] of `cfg` lowered on the CPU, in this process's environment."""
    import torch

    cases, N = _imports()
    from fce_yolo_amd.backend import NetBackend

    h8 = cfg.endswith("-h8.yaml")  # yolo11m-fce.yaml with 8 BiCoordCrossAtt heads (cases.heads8)
    model = cases.seeded_model(cfg.replace("-h8", ""), 0, cases.heads8 if h8 else None)
    be = NetBackend(640, 640, torch.device("cpu"))
    try:
        with torch.no_grad():
            model.emit(be, be.input_view(1, 3))
        L = N.lib()
        out = []
        for i in range(L.fce_net_num_ops(be.net)):
            name = C.create_string_buffer(64)
            nb, fl = C.c_double(), C.c_double()
            N.call("fce_net_op_info", be.net, i, name, 64, C.byref(nb), C.byref(fl))
            out.append([name.value.decode(), L.fce_net_alt_form(be.net, i), L.fce_net_c3k2_form(be.net, i),
                        L.fce_net_op_skipped(be.net, i)])
        return out
    finally:
        be.close()


def child_host(name):
    """{cfg: host_ops(cfg)} of env set `name`, from a fresh child process."""
    env = {k: v for k, v in os.environ.items() if k not in FUSE_KNOBS}
    env.update(ENV_SETS[name])
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], capture_output=True, text=True,
                       env=env, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child for env set {name} failed:\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def plan_ops(model, size, device):
    """(ops, locked) of `model` planned at PLAN_BATCH x size x size without autotuning (GPU)."""
    _imports()
    from fce_yolo_amd.engine import Engine

    eng = Engine(model, PLAN_BATCH, size, device, autotune=False)
    ops, locked = [], []
    for i in range(eng.num_ops()):
        ops.append([*eng.op_info(i), eng.alt_form(i), int(eng.skipped(i)), eng.variant(i), eng.variants(i)])
    for i, op in enumerate(ops):
        if op[3] != 0:
            continue
        try:
            eng.set_alt_form(i, True)
        except RuntimeError:
            locked.append(i)
        else:
            eng.set_alt_form(i, False)
    eng.close()
    return ops, locked


def tune_codes(model, size, device):
    """[(op, code)] of fce_net_tune_record after an autotuned plan (GPU)."""
    _, N = _imports()
    from fce_yolo_amd.engine import Engine

    eng = Engine(model, PLAN_BATCH, size, device, autotune=True)
    out, op, code = [], C.c_int(), C.c_int()
    while N.lib().fce_net_tune_record(eng.net, len(out), C.byref(op), C.byref(code), None):
        out.append([op.value, code.value])
    eng.close()
    return out


def intern(table, item):
    """Index of `item` in `table`, appended if new."""
    if item not in table:
        table.append(item)
    return table.index(item)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="print this process's host lists as JSON")
    ap.add_argument("--host-only", action="store_true", help="keep the recorded plans (no GPU)")
    ap.add_argument("--out", type=Path, default=FIXTURE)
    a = ap.parse_args()
    if a.child:
        print(json.dumps({cfg: host_ops(cfg) for cfg in HOST_CONFIGS}))
        return
    rec = {"names": [], "lists": [], "host": {}}
    for name in ENV_SETS:
        rec["host"][name] = {cfg: [[intern(rec["names"], op[0]), *op[1:]] for op in ops]
                             for cfg, ops in child_host(name).items()}
    if a.host_only:
        old = json.loads(FIXTURE.read_text())
        remap = [intern(rec["names"], n) for n in old["names"]]
        rec["lists"], rec["tune"] = old["lists"], old["tune"]
        rec["plans"] = {cfg: {s: {"ops": [[remap[op[0]], *op[1:]] for op in p["ops"]], "locked": p["locked"]}
                              for s, p in by_size.items()} for cfg, by_size in old["plans"].items()}
    else:
        import torch

        cases, _ = _imports()
        for k in FUSE_KNOBS:
            os.environ.pop(k, None)
        dev = torch.device("cuda:0")
        rec["plans"] = {}
        for cfg in PLAN_CONFIGS:
            model = cases.seeded_model(cfg, 0).to(dev)
            rec["plans"][cfg] = {}
            for size in PLAN_SIZES:
                ops, locked = plan_ops(model, size, dev)
                rec["plans"][cfg][str(size)] = {
                    "ops": [[intern(rec["names"], op[0]), *op[1:6], intern(rec["lists"], op[6])] for op in ops],
                    "locked": locked}
        rec["tune"] = tune_codes(cases.seeded_model(TUNE[0], 0).to(dev), TUNE[1], dev)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(rec, separators=(",", ":")) + "\n")
    print(f"wrote {a.out}: {a.out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
