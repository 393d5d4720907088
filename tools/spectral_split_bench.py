"""The split spectral step at the reference's live shape -- 441 000 samples, first sine layer
+ 4 Snake, width 256, mae, alpha = 0.2, both stft_loss kinds -- interleaved rounds in one process on one
GPU (graph replay, device events around `--steps` steps, median of `--rounds` rounds):

  (a) the default one-batch step against split_spectral=True with one micro-batch (the same launches);
  (b) 1 against 2 against 4 micro-batches: the cost of the repeated forward;
  (c) signal forward + backward on a 1/8 window of a 2^23-sample signal against the whole signal: what
      frame sharding saves a rank at 8 GPUs.

    python tools/spectral_split_bench.py [--rounds 5] [--steps 30] [--rows 441000] [--skip-window]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(ts):
    v = sorted(ts)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "all_ms": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=441000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window-rows", type=int, default=1 << 23)
    ap.add_argument("--skip-window", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(diag=False)
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd.engine import SirenEngine, _basis
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, H = args.rows, args.hidden
    out = {"rows": n, "hidden": H, "steps_per_round": args.steps, "rounds": args.rounds, "step": {}, "window": {}}

    def signal(m):
        k = torch.arange(m, dtype=torch.float64)
        g = torch.Generator().manual_seed(0)
        return (0.5 * torch.sin(2 * torch.pi * 440 * k / 44100) + 0.2 * torch.sin(2 * torch.pi * 3100 * k / 44100 + 1)
                + 0.05 * torch.randn(m, generator=g, dtype=torch.float64)).float()

    # ---- (a), (b): whole steps
    t, y = torch.linspace(-1, 1, n).reshape(n, 1), signal(n)

    def engine(kind, **kw):
        torch.manual_seed(0)
        m = SirenWithSnakeTanh(1, 1, H, 0, 4, 0, first_omega_0=22000.0, hidden_omega_0=30.0, a_initial=0.5)
        return SirenEngine(m, t, y, device=dev, loss_mode="mae", alpha=0.2, stft_loss=kind, **kw)

    engines = {}
    for kind in ("stft", "mrstft"):
        engines[f"{kind}_default"] = engine(kind)
        for k in (1, 2, 4):
            mb = -(-(-(-n // k)) // 256) * 256
            engines[f"{kind}_split_{k}mb"] = eng = engine(kind, micro_batch=mb, split_spectral=True)
            assert eng.n_micro == k, (eng.n_micro, k)
    for eng in engines.values():
        eng.step()
        eng.step()
        eng.capture_graph()
    step = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, eng in engines.items():
            eng.step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                eng.step()
            e1.record()
            torch.cuda.synchronize()
            step[name].append(e0.elapsed_time(e1) / args.steps)
    for name, eng in engines.items():
        rec = med(step[name])
        rec["last_loss"] = eng.last_loss()
        rec["overflows"] = eng.guard_state()["overflows"]
        out["step"][name] = rec
    del engines
    torch.cuda.empty_cache()

    # ---- (c): the loss alone on a 1/8 window of a long signal
    if not args.skip_window:
        m = args.window_rows
        yd = signal(m).to(dev)
        xd = (0.8 * yd + 0.05 * torch.randn(m, device=dev)).contiguous()
        g, loss = torch.zeros(m, device=dev), torch.zeros(4, device=dev)
        P = lambda v: v.data_ptr()  # noqa: E731
        s = torch.cuda.current_stream().cuda_stream
        lo, hi = 3 * (m // 8), 4 * (m // 8)
        for kind, nres in (("stft", 1), ("mrstft", 3)):
            fn = lambda name: getattr(lib, f"siren_{kind}_{name}")  # noqa: E731,B023
            basis = _basis(kind, dev)
            ws = torch.zeros(int(fn("workspace_floats")(m, m)), device=dev)
            _lib.check(fn("forward")(P(yd), m, m, P(basis), P(ws), 1, s), "target")
            wins = {}
            for tag, (a, b) in (("whole", (0, m)), ("eighth", (lo, hi))):
                win = (ctypes.c_int32 * 6)()
                for r in range(nres):
                    blk = (ctypes.c_int32 * 4)()
                    rr = (r,) if kind == "mrstft" else ()
                    _lib.check(fn("window")(m, *rr, a, b, blk), "window")
                    win[2 * r], win[2 * r + 1] = blk[0], blk[1]
                wins[tag] = (win, a, b)
            # complete partials and finished scalars for both windows' backwards
            _lib.check(fn("signal_forward")(P(xd), P(yd), m, m, 1, 0.2, P(basis), P(ws), wins["whole"][0], s),
                       "forward")
            _lib.check(fn("signal_finish")(m, m, 1, 0.2, P(ws), P(loss), s), "finish")
            calls = {}
            for tag, (win, a, b) in wins.items():
                calls[f"{tag}_forward"] = lambda win=win: fn("signal_forward")(  # noqa: B023
                    P(xd), P(yd), m, m, 1, 0.2, P(basis), P(ws), win, s)
                calls[f"{tag}_backward"] = lambda win=win, a=a, b=b: fn("signal_backward")(  # noqa: B023
                    P(xd), P(yd), m, m, 1, 0.2, P(basis), P(ws), win, a, b, P(g), s)
            times = {name: [] for name in calls}
            for _ in range(args.rounds):
                for name, call in calls.items():
                    _lib.check(call(), name)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / args.reps)
            out["window"][kind] = {"rows": m, "window": [lo, hi],
                                   "blocks": {tag: list(w[0])[:2 * nres] for tag, w in wins.items()},
                                   **{name: med(v) for name, v in times.items()}}
            del ws, basis
            torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
