#!/usr/bin/env python
"""dev: the per-element weight-gradient tables of tests/wgrad_rows_case.py as a record (profiles/wgrad_rows.json is one).

    python tools/wgrad_rows_report.py [--emu] [--cases emu,k4,k3] [--ks 0,2,4] [--faint-ks 3,5] [--out FILE.json]

Muted units (asserted by tests/test_gpu_wgrad_rows.py): per case, k and arithmetic the max E / A of every tensor over its muted and its other rows,
the fp32 oracle's own figure and the ideal restatement's beside it, the rows left out for kinks.  Faint units (rows U of each hidden layer's own
weight and bias x 10^-k: NOT asserted, the cause of what it shows is not established): the same table over all rows, and the forward colour's
distance from float64.  --emu runs the host-emulated kernels (~25 s per backward) instead of the device."""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emu", action="store_true")
    ap.add_argument("--cases", default="emu,k4,k3")
    ap.add_argument("--ks", default="0,2,4")
    ap.add_argument("--faint-ks", default="3,5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import gpu_util
    import wgrad_rows_case as WR
    ints = lambda s: [int(x) for x in s.split(",") if x != ""]
    ctx = contextlib.nullcontext()
    if a.emu:
        from emu_util import emu_backend
        torch.cuda.synchronize = lambda *x, **k: None
        ctx = emu_backend()
    rec = {"muted": {}, "faint": {}, "left_out": {}, "two_plane_factor": WR.TWO_PLANE_FACTOR, "bound": WR.BOUND}
    with ctx:
        for name in a.cases.split(","):
            for k in ints(a.ks):
                ref = WR.Reference(name, k)
                rec["left_out"]["%s k=%d" % (name, k)] = ref.left_out()
                for bits, planes in ((8, 1), (16, 1), (16, 2)):
                    if a.emu and (bits, planes) != (8, 1):
                        continue
                    gm, gp, _ = WR.hip_gradients(ref, gpu_util.hip_render, bits, planes)
                    _, fig = WR.report(ref, "%d-bit cross terms, %d plane(s)" % (bits, planes), gm, None if planes == 1 else WR.two_plane_bound)
                    rec["muted"]["%s k=%d bits=%d planes=%d" % (name, k, bits, planes)] = fig
            if ints(a.faint_ks):
                rec["faint"][name] = {"k=%d" % k: v for k, v in WR.faint_report(name, ints(a.faint_ks), gpu_util.hip_render).items()}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
