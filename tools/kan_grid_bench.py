"""Times of the KAN grid update (KANLinear.update_grid, kan.py:168-215) on the HIP path, per stage.

    python tools/kan_grid_bench.py [--rows 441000] [--width 256] [--reps 5] [--out FILE]

Per layer of KAN([1, W, W, 1]) at `rows` coordinates: order statistics (torch.sort + six rows), knots,
Gram sums (with the achieved rate of the one read of the layer input) and refit, each the median of
`reps` timed launches after one warm-up, by device events.  As a yardstick, the reference's algorithm
(the (batch, in, out) curves by bmm, then a batched lstsq on (in, batch, 8)) in torch on the same GPU
at the largest size it fits (--yard-rows x --yard-width), next to the HIP path at that size.  At
441 000 x 256 x 256 the reference's intermediate is 115 GB: it has no timing there.  One JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def stages(lay, x, reps):
    """Median ms of each stage of lay.update_grid(x), without touching the layer."""
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd._lib import check, ptr
    lib, dev = _lib.load(), x.device
    s = torch.cuda.current_stream(dev).cuda_stream
    rows, fin, fout = x.shape[0], lay.in_features, lay.out_features
    idx = torch.linspace(0, rows - 1, 6, dtype=torch.int64).to(dev)
    q = torch.sort(x, dim=0)[0][idx].contiguous()
    grid_new = torch.empty_like(lay.grid)
    ws = torch.empty(int(lib.siren_kan_grid_workspace_bytes(rows, fin)), dtype=torch.uint8, device=dev)
    gram = torch.empty(fin, 2, 8, 8, dtype=torch.float64, device=dev)
    sw_new = torch.empty_like(lay.spline_weight)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    t = {}
    t["order_statistics_ms"] = timed(lambda: torch.sort(x, dim=0)[0][idx].contiguous(), reps)
    t["knots_ms"] = timed(lambda: check(lib.siren_kan_grid_knots(ptr(q), fin, 0.01, lay.grid_eps, ptr(grid_new), s)), reps)
    t["gram_ms"] = timed(lambda: check(lib.siren_kan_grid_gram(ptr(x), rows, fin, ptr(lay.grid), ptr(grid_new), 0,
                                                                ptr(gram), ptr(ws), s)), reps)
    t["refit_ms"] = timed(lambda: check(lib.siren_kan_grid_refit(ptr(gram), fin, fout, ptr(lay.spline_weight.detach()),
                                                                  ptr(lay.spline_scaler.detach()), ptr(sw_new),
                                                                  ptr(status), ptr(ws), s)), reps)
    t["gram_read_GBps"] = rows * fin * 4 / (t["gram_ms"] * 1e-3) / 1e9
    t["rank_deficient_inputs"] = int(status[0].item())
    t["total_ms"] = t["order_statistics_ms"] + t["knots_ms"] + t["gram_ms"] + t["refit_ms"]
    return t


def torch_route(lay, x):
    """The reference's algorithm with torch ops on the device (curves by bmm, batched lstsq), on this
    package's own bspline_bases; the knots are left out (they cost the same sort either way)."""
    curves = torch.bmm(lay.b_splines(x).permute(1, 0, 2), lay.scaled_spline_weight.permute(1, 2, 0))  # (in, batch, out)
    return torch.linalg.lstsq(lay.b_splines(x).transpose(0, 1), curves).solution


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=441000)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--yard-rows", type=int, default=44100)
    ap.add_argument("--yard-width", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(diag=False)
    from inr_for_audio_amd._lib import SirenError
    from inr_for_audio_amd.kan import KAN, layer_forward
    dev = torch.device("cuda:0")
    res = {"rows": a.rows, "width": a.width, "device": torch.cuda.get_device_name(0), "layers": []}
    torch.manual_seed(0)
    with torch.no_grad():
        model = KAN([1, a.width, a.width, 1]).to(dev)
        h = torch.linspace(-1, 1, a.rows, device=dev).reshape(-1, 1)
        for lay in model.layers:
            t = stages(lay, h, a.reps)
            t["in"], t["out"] = lay.in_features, lay.out_features
            res["layers"].append(t)
            try:
                lay.update_grid(h)
            except SirenError as e:  # a rank-deficient input: the layer stays as it was, the times stand
                t["refused"] = str(e)[:120]
            h = layer_forward(lay, h)
        res["update_total_ms"] = sum(t["total_ms"] for t in res["layers"])
        whole = KAN([1, a.width, a.width, 1]).to(dev)
        x0 = torch.linspace(-1, 1, a.rows, device=dev).reshape(-1, 1)
        if not any("refused" in t for t in res["layers"]):
            res["forward_update_grid_ms"] = timed(lambda: whole(x0, update_grid=True), max(1, a.reps // 2))
        # the yardstick: one hidden layer W x W at a size the reference's algorithm fits
        yl = KAN([1, a.yard_width, a.yard_width, 1]).to(dev)
        hy = layer_forward(yl.layers[0], torch.linspace(-1, 1, a.yard_rows, device=dev).reshape(-1, 1))
        lay = yl.layers[1]
        y = {"rows": a.yard_rows, "width": a.yard_width, "hip": stages(lay, hy, a.reps)}
        try:
            y["torch_bmm_lstsq_ms"] = timed(lambda: torch_route(lay, hy), a.reps)
        except Exception as e:  # e.g. no batched gels in this torch build
            y["torch_bmm_lstsq_error"] = f"{type(e).__name__}: {e}"[:200]
        res["yardstick"] = y
        res["reference_at_full_size"] = (f"none: its (batch, in, out) intermediate is "
                                         f"{a.rows * a.width * a.width * 4 / 1e9:.0f} GB")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
