"""Times of the KAN refit onto a grid of another size (KANLinear.regrid) on the HIP path, per stage.

    python tools/kan_regrid_bench.py [--rows 441000] [--width 256] [--reps 5] [--out FILE]

Per layer of KAN([1, W, W, 1]) at `rows` coordinates and per pair of grid sizes (5 -> 5, 5 -> 10,
10 -> 20, 64 -> 64): knots, Gram sums (with the achieved rate of the one read of the layer input) and
refit, each the median of `reps` timed launches after one warm-up, by device events.  5 -> 5 is
update_grid's case (tools/kan_grid_bench.py times it with its order statistics).  The layers' inputs
are the old model's activations; an input the rank rule refuses is counted, its time stands.  One JSON
line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIRS = ((5, 5), (5, 10), (10, 20), (64, 64))


def timed(fn, reps):
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


def stages(lay, x, g_new, reps):
    """Median ms of each stage of lay.regrid(x, g_new), without touching the layer."""
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd._lib import check, ptr
    lib, dev = _lib.load(), x.device
    s = torch.cuda.current_stream(dev).cuda_stream
    rows, fin, fout, g_old = x.shape[0], lay.in_features, lay.out_features, lay.grid_size
    idx = torch.linspace(0, rows - 1, g_new + 1, dtype=torch.int64).to(dev)
    q = torch.sort(x, dim=0)[0][idx].contiguous()
    grid_new = torch.empty(fin, g_new + 7, dtype=torch.float32, device=dev)
    gram = torch.empty(fin * (g_new + 3) * (g_new + g_old + 6), dtype=torch.float64, device=dev)
    sw = lay.spline_weight.detach()
    sw_new = torch.empty(fout, fin, g_new + 3, dtype=torch.float32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    t = {}
    ws = torch.empty(int(lib.siren_kan_regrid_workspace_bytes(rows, fin, g_old, g_new)), dtype=torch.uint8, device=dev)
    t["knots_ms"] = timed(lambda: check(lib.siren_kan_regrid_knots(ptr(q), fin, g_new, 0.01, lay.grid_eps,
                                                                    ptr(grid_new), s)), reps)
    t["gram_ms"] = timed(lambda: check(lib.siren_kan_regrid_gram(ptr(x), rows, fin, g_old, g_new, ptr(lay.grid),
                                                                  ptr(grid_new), 0, ptr(gram), ptr(ws), s)), reps)
    t["refit_ms"] = timed(lambda: check(lib.siren_kan_regrid_refit(ptr(gram), fin, fout, g_old, g_new, ptr(sw), None,
                                                                    ptr(sw_new), ptr(status), s)), reps)
    t["workspace_MB"] = ws.numel() / 1e6
    t["gram_read_GBps"] = rows * fin * 4 / (t["gram_ms"] * 1e-3) / 1e9
    t["rank_deficient_inputs"] = int(status[0].item())
    t["total_ms"] = t["knots_ms"] + t["gram_ms"] + t["refit_ms"]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=441000)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(diag=False)
    from inr_for_audio_amd.kan import KAN, layer_forward
    dev = torch.device("cuda:0")
    res = {"rows": a.rows, "width": a.width, "device": torch.cuda.get_device_name(0), "pairs": {}}
    with torch.no_grad():
        for g_old, g_new in PAIRS:
            torch.manual_seed(0)
            model = KAN([1, a.width, a.width, 1], grid_size=g_old).to(dev)
            h = torch.linspace(-1, 1, a.rows, device=dev).reshape(-1, 1)
            layers = []
            for lay in model.layers:
                layers.append({"in": lay.in_features, "out": lay.out_features, "regrid": stages(lay, h, g_new, a.reps)})
                h = layer_forward(lay, h)
            res["pairs"][f"{g_old}->{g_new}"] = layers
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
