"""Timing of the loss-landscape plane (run.py:192-208; SirenEngine.loss_plane, csrc/plane.hip) at the
reference's live size (441 000 coordinates, H = 256): the first SineLayer + 4 Snake layers of the
reference's Snake sweeps, and train()'s default stack (2 sine + 2 Snake).

* `plane_s`: loss_plane(steps=30), HIP events around the whole call (900 grid points, the final copy
  included), median of `rounds`;
* `infer_x900_s`: 900 x the median time of engine.infer(coords) on the same engine and rows -- the only
  way to evaluate a plane without loss_plane (per point it also pays an output allocation and copies,
  and the weights would have to be swapped in on top of that);
* `plane_point_us`: the siren_plane_point launch alone, HIP events around `reps` back-to-back calls;
* `cpu_forward_x900_s` (--cpu): EXTRAPOLATED -- one forward of oracle/torch_cpu_step.py's port of the
  reference module on this host's CPU x 900 (the reference evaluates its plane on the CPU).

    python tools/landscape_bench.py [--rows 441000] [--hidden 256] [--steps 30] [--rounds 3] [--cpu]

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STACKS = {"sine+4snake": (0, 4), "default": (2, 2)}


def _events(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=441000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--omega", type=float, default=22000.0)
    ap.add_argument("--cpu", action="store_true", help="also time one CPU forward of the reference module's port")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(diag=False)
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.landscape import plane_directions
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    dev = torch.device("cuda:0")
    n, H, steps = args.rows, args.hidden, args.steps
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    y = (0.5 * torch.sin(37 * t) + 0.3 * torch.sin(91 * t + 0.5)).reshape(-1)
    out = {"rows": n, "hidden": H, "steps": steps, "cells": steps * steps, "stacks": {}}
    for name, (ns, nk) in STACKS.items():
        torch.manual_seed(0)
        model = SirenWithSnakeTanh(1, 1, H, ns, nk, 0, first_omega_0=args.omega, hidden_omega_0=30.0, a_initial=0.5)
        eng = SirenEngine(model, t, y, device=dev)
        for _ in range(3):
            eng.step()
        d1, d2 = plane_directions([p for _, p in model.named_parameters()], steps=steps,
                                  generator=torch.Generator().manual_seed(0))
        coords = t.to(dev)
        eng.loss_plane(d1, d2, 2)   # warm-up: the scratch network, every kernel once
        eng.infer(coords)
        plane_s = [_events(lambda: eng.loss_plane(d1, d2, steps), dev) for _ in range(args.rounds)]
        infer_s = [_events(lambda: eng.infer(coords), dev) for _ in range(max(args.rounds, 3) * 5)]
        sc = eng._plane_scratch()
        D1, D2 = eng._plane_upload(d1), eng._plane_upload(d2)
        s = eng._stream()

        def points():
            for _ in range(args.reps):
                eng._plane_point(sc, D1, D2, -1.0, 2.0, s)

        point_s = [_events(points, dev) / args.reps for _ in range(args.rounds)]
        r = {"plane_s": statistics.median(plane_s), "plane_s_all": plane_s,
             "infer_s": statistics.median(infer_s), "infer_x900_s": statistics.median(infer_s) * steps * steps,
             "plane_point_us": statistics.median(point_s) * 1e6, "n_micro": eng.n_micro,
             "params": int(eng.layout.n_params)}
        r["plane_over_infer_x900"] = r["plane_s"] / r["infer_x900_s"]
        if args.cpu:
            from oracle import torch_cpu_step as cpu
            ref = cpu.build(1, H, ns, args.omega, 30.0, n_snake=nk)
            x = t.reshape(1, n, 1)
            times = []
            with torch.no_grad():
                for _ in range(3):
                    t0 = time.perf_counter()
                    ref(x)
                    times.append(time.perf_counter() - t0)
            r["cpu_forward_s"] = min(times)
            r["cpu_forward_x900_s"] = min(times) * steps * steps     # extrapolated, not run
            r["cpu_threads"] = torch.get_num_threads()
        out["stacks"][name] = r
        del eng
    print(json.dumps(out))


if __name__ == "__main__":
    main()
