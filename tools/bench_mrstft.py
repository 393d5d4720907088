"""Cost of the multi-resolution STFT loss (csrc/stft.hip; run.py:127, :160) at the reference's live
config (run.py:466): a first sine layer + 4 Snake hidden layers, width 256, 441 000 rows (10 s at
44.1 kHz; T = 3676 / 1838 / 8821 frames), beside the single-resolution kernels of the same file
re-measured in the same process as the yardstick.

* the individual entry points (HIP events around `reps` back-to-back calls, rounds interleaved):
  siren_stft_forward / siren_stft_loss_bwd and siren_mrstft_forward / siren_mrstft_loss /
  siren_mrstft_loss_bwd; GEMM rates are 2 T_r win_r 2 bins_r flops per direction, summed over the
  resolutions, over the 157.3 TFLOP/s fp32-MFMA peak.  ``--also NAME=PATH`` times the mrstft entry
  points of another build of the library in the same rounds (an A/B of a blocking choice).
* per resolution: run this file with ``--kernels-only`` under ``rocprofv3 --kernel-trace --stats`` (a run
  of its own); the instantiations carry n_fft / hop / win in their names, and flops() below gives each
  one's work.
* whole steps, each a graph replay with the profiler off, rounds interleaved: ``mae, alpha 0``,
  ``mae, alpha 0.2`` with stft_loss 'stft' and with 'mrstft'; the loss launches' own time from an eager
  run with the per-launch profile (SIREN_PROF_LOSS).

    python tools/bench_mrstft.py [--rows 441000] [--hidden 256] [--rounds 5] [--steps 30] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F32_MFMA = 157.3e12
RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))   # n_fft, hop, win_length
CONFIGS = {"mae_a0": ("mae", 0.0, "stft"), "mae_a0.2_stft": ("mae", 0.2, "stft"),
           "mae_a0.2_mrstft": ("mae", 0.2, "mrstft")}


def flops(n: int, res) -> float:
    """One direction of one resolution: [T][win] x [win][2 bins]."""
    n_fft, hop, win = res
    return 2.0 * (1 + n // hop) * win * 2 * (n_fft // 2 + 1)


def med(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=441000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stack", default="0,4", help="num_sine,num_snake of the hidden stack (run.py:466: 0,4)")
    ap.add_argument("--omega", type=float, default=22000.0)
    ap.add_argument("--kernels-only", action="store_true", help="the entry points only (for a kernel trace)")
    ap.add_argument("--also", action="append", default=[], metavar="NAME=PATH",
                    help="another build of the library whose mrstft entry points are timed in the same rounds")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(diag=False)
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd.engine import SirenEngine, stft_basis
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, H = args.rows, args.hidden
    R = -(-n // 256) * 256
    ns, nk = (int(v) for v in args.stack.split(","))
    P = lambda t: t.data_ptr()  # noqa: E731
    s = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    out = {"rows": n, "padded_rows": R, "hidden": H, "stack": [ns, nk],
           "frames": {"stft": int(lib.siren_stft_frames(n)), "mrstft": [int(lib.siren_mrstft_frames(n, r)) for r in range(3)]},
           "gflop_per_direction": {"stft": 2.0 * (1 + n // 256) * 1024 * 1026 / 1e9,
                                   "mrstft": [flops(n, res) / 1e9 for res in RES]},
           "step": {}, "kernels": {}}

    g = torch.Generator().manual_seed(0)
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    k = torch.arange(n, dtype=torch.float64)
    y = (0.5 * torch.sin(2 * torch.pi * 440 * k / 44100) + 0.2 * torch.sin(2 * torch.pi * 3100 * k / 44100 + 1)
         + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float()
    yd = y.to(dev)
    xd = (0.8 * yd + 0.05 * torch.randn(n, device=dev)).contiguous()
    loss, gbuf = torch.zeros(4, device=dev), torch.zeros(n, device=dev)

    # ---- the individual entry points
    basis = stft_basis(dev)
    ws = torch.zeros(int(lib.siren_stft_workspace_floats(n, R)), device=dev)
    _lib.check(lib.siren_stft_forward(P(yd), n, R, P(basis), P(ws), 1, s()), "stft target")
    _lib.check(lib.siren_stft_forward(P(xd), n, R, P(basis), P(ws), 0, s()), "stft forward")
    _lib.check(lib.siren_stft_loss(n, R, P(ws), P(loss), s()), "stft loss")
    calls = {
        "stft_forward": lambda: lib.siren_stft_forward(P(xd), n, R, P(basis), P(ws), 0, s()),
        "stft_backward_and_gather": lambda: lib.siren_stft_loss_bwd(n, R, P(basis), P(ws), P(gbuf), s()),
    }
    keep = []

    def add_mr(tag, L):
        host = torch.empty(int(L.siren_mrstft_basis_floats()), dtype=torch.float32)
        _lib.check(L.siren_mrstft_basis_fill(host.data_ptr()), "mrstft basis")
        mb = host.to(dev)
        mw = torch.zeros(int(L.siren_mrstft_workspace_floats(n, R)), device=dev)
        keep.extend([mb, mw])
        _lib.check(L.siren_mrstft_forward(P(yd), n, R, P(mb), P(mw), 1, s()), "mrstft target")
        _lib.check(L.siren_mrstft_forward(P(xd), n, R, P(mb), P(mw), 0, s()), "mrstft forward")
        _lib.check(L.siren_mrstft_loss(n, R, P(mw), P(loss), s()), "mrstft loss")
        calls[f"mrstft_forward{tag}"] = lambda: L.siren_mrstft_forward(P(xd), n, R, P(mb), P(mw), 0, s())
        calls[f"mrstft_scalars{tag}"] = lambda: L.siren_mrstft_loss(n, R, P(mw), P(loss), s())
        calls[f"mrstft_backward_and_gather{tag}"] = lambda: L.siren_mrstft_loss_bwd(n, R, P(mb), P(mw), P(gbuf), s())

    add_mr("", lib)
    for spec in args.also:
        name, path = spec.split("=", 1)
        add_mr("@" + name, _lib.bind(path))
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
    for name in calls:
        rec = med(times[name])
        fl = None
        if name.startswith("stft_"):
            fl = 2.0 * (1 + n // 256) * 1024 * 1026
        elif "scalars" not in name:
            fl = sum(flops(n, res) for res in RES)
        if fl is not None:
            rec["gemm_tflops"] = fl / (rec["median_ms"] * 1e-3) / 1e12
            rec["fraction_of_f32_mfma_peak"] = fl / (rec["median_ms"] * 1e-3) / PEAK_F32_MFMA
        out["kernels"][name] = rec
    if args.kernels_only:
        print(json.dumps(out, indent=1))
        return

    # ---- whole steps
    def engine(loss_mode, alpha, stft_loss):
        torch.manual_seed(0)
        m = SirenWithSnakeTanh(1, 1, H, ns, nk, 0, first_omega_0=args.omega, hidden_omega_0=30.0, a_initial=0.5)
        return SirenEngine(m, t, y, device=dev, loss_mode=loss_mode, alpha=alpha, stft_loss=stft_loss)

    engines = {name: engine(*cfg) for name, cfg in CONFIGS.items()}
    prof = {}
    for name, eng in engines.items():       # per-launch profile of eager steps, a run of its own
        eng.step()
        eng.step()
        _lib.check(lib.siren_profile_enable(4096), "profile")
        for _ in range(10):
            eng.step()
        torch.cuda.synchronize()
        prof[name] = {k_: v[0] / 10 for k_, v in _lib.profile_read().items() if v[1]}
        _lib.check(lib.siren_profile_enable(0), "profile off")
    step = {name: [] for name in engines}
    for eng in engines.values():
        eng.capture_graph()
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
    base = med(step["mae_a0"])["median_ms"]
    for name, eng in engines.items():
        rec = med(step[name])
        rec["over_mae_a0_ms"] = rec["median_ms"] - base
        rec["loss_kernels_ms_per_step"] = prof[name].get("loss", 0.0)
        rec["profile_ms_per_step"] = prof[name]
        rec["last_loss"] = eng.last_loss()
        rec["overflows"] = eng.guard_state()["overflows"]
        out["step"][name] = rec
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
