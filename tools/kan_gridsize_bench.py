"""Step times of the KAN fit by grid size on the HIP path.

    python tools/kan_gridsize_bench.py [--rows 441000] [--width 64] [--steps 10] [--grids 10,20,64] [--out FILE]

KAN([1, W, W, 1], grid_size=G) at `rows` coordinates, one whole MSE step (gradients + Adam + scheduler)
replayed from a captured graph, the median of `steps` replays by device events, in ms per step:

  5          the grid-5 kernels (kan.hip: sizes fixed at compile time, one-pass hidden backward)
  5_general  the same net through the any-grid-size kernels (kan_general.hip; SIREN_OPT_KAN_GENERAL)
  10, 20, 64 the any-grid-size kernels at those sizes

and for each row the per-kind launch times of one eager step from the library's own profiling
(SIREN_PROF_KAN_*: kan_fwd, kan_dw -- the head pass and the weight-gradient passes --, kan_dx -- the
input-gradient pass, or the one-pass backward of the grid-5 set --, kan_misc), which say where a
difference between the first two rows goes.  One JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def data(rows):
    g = torch.Generator().manual_seed(1)
    t = torch.arange(rows, dtype=torch.float64)
    y = (0.5 * torch.sin(2 * math.pi * 440 * t / 44100) + 0.2 * torch.sin(2 * math.pi * 3100 * t / 44100 + 1)
         + 0.05 * torch.randn(rows, generator=g, dtype=torch.float64))
    return torch.linspace(-1, 1, rows).reshape(-1, 1), y.float()


def measure(width, rows, grid_size, dev, steps):
    """(ms per replayed step, {kind: ms} of one eager step) for one grid size under the current knobs."""
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd._lib import check
    from inr_for_audio_amd.engine import KanEngine
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(0)
    x, y = data(rows)
    eng = KanEngine(KAN([1, width, width, 1], grid_size=grid_size), x, y, device=dev)
    eng.step()
    torch.cuda.synchronize(dev)
    lib = eng.lib
    check(lib.siren_profile_mask(0xFFFFFFFF))
    check(lib.siren_profile_enable(64 * (steps + 1)))
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize(dev)
    kinds = {k: round(v[0] / steps, 4) for k, v in _lib.profile_read().items() if v[1]}
    check(lib.siren_profile_enable(0))
    eng.capture_graph()
    return median_ms(eng.step, steps), kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=441000)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--grids", default="10,20,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(diag=False)
    from inr_for_audio_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda:0")
    res = {"rows": a.rows, "width": a.width, "device": torch.cuda.get_device_name(0), "step_ms": {}, "kinds_ms": {}}

    def row(name, grid_size):
        res["step_ms"][name], res["kinds_ms"][name] = measure(a.width, a.rows, grid_size, dev, a.steps)

    row("5", 5)
    with _lib.options(lib, {_lib.Opt.KAN_GENERAL: 1}):
        row("5_general", 5)
    for g in [int(v) for v in a.grids.split(",") if v]:
        row(str(g), g)
    res["general_over_grid5"] = res["step_ms"]["5_general"] / res["step_ms"]["5"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
