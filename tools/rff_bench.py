"""Timing of the random-Fourier-feature encoded first layer (rff.hip) at the reference's live size
(441 000 coordinates, H = 256, F in {64, 256}; run.py:439-442 fe_snake_*):

* the forward kernel (siren_rff_first_fwd, enc written as in training): HIP events around `reps`
  back-to-back calls, rounds interleaved over the F values; 2 rows 2F H flops over the
  157.3 TFLOP/s fp32-MFMA peak;
* the weight gradient dW0 (split-K GEMM + slice reduce + omega0 finish): the library's per-launch
  profile of whole steps, SIREN_PROF_BWD_DW of the encoded stack minus the same stack without the
  encoding (the hidden layers' dW launches are the same work in both);
* the whole step (graph replay, profiler off) beside the same stack without the encoding.

    python tools/rff_bench.py [--rows 441000] [--hidden 256] [--freqs 64,256] [--rounds 5] [--reps 20]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=441000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--freqs", default="64,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--stack", default="0,4", help="num_sine,num_snake of the hidden stack (fe_snake_*: 0,4)")
    ap.add_argument("--omega", type=float, default=22000.0)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(diag=False)
    from inr_for_audio_amd import GaussianEncoding, _lib
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, H = args.rows, args.hidden
    R = -(-n // 256) * 256
    freqs = [int(f) for f in args.freqs.split(",")]
    ns, nk = (int(v) for v in args.stack.split(","))
    P = lambda t: t.data_ptr()  # noqa: E731
    s = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    import ctypes
    out = {"rows": n, "padded_rows": R, "hidden": H, "stack": [ns, nk], "fwd": {}, "step": {}}

    # ---- forward kernel
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.zeros(R, device=dev)
    x[:n] = torch.linspace(-1, 1, n, device=dev)
    Y, C = (torch.empty(R, H, dtype=torch.float16, device=dev) for _ in range(2))
    bufs = {}
    for F in freqs:
        bufs[F] = (torch.randn(F, device=dev, generator=g) * 10.0,
                   (torch.rand(H, 2 * F, device=dev, generator=g) * 2 - 1) / (2 * F),
                   (torch.rand(H, device=dev, generator=g) * 2 - 1) / (2 * F) ** 0.5,
                   torch.empty(R, lib.siren_rff_kpad(F), dtype=torch.float16, device=dev))
    times = {F: [] for F in freqs}
    for _ in range(args.rounds):
        for F in freqs:
            B, W0, b0, enc = bufs[F]
            call = lambda: lib.siren_rff_first_fwd(P(x), P(B), F, P(W0), P(b0), ctypes.c_float(args.omega), None,  # noqa: E731
                                                   R, H, P(Y), P(C), None, P(enc), s())
            _lib.check(call(), "siren_rff_first_fwd")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            times[F].append(e0.elapsed_time(e1) / args.reps)
    for F in freqs:
        ts = sorted(times[F])
        med = ts[len(ts) // 2]
        fl = 2.0 * R * 2 * F * H
        out["fwd"][F] = {"median_ms": med, "min_ms": ts[0], "max_ms": ts[-1], "tflops": fl / (med * 1e-3) / 1e12,
                         "peak_fraction": fl / (med * 1e-3) / PEAK_F32_MFMA}

    # ---- whole steps: with the encoding and the same stack on the raw coordinate
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    y = 0.5 * torch.sin(37 * t) + 0.3 * torch.sin(91 * t + 0.5)

    def engine(F):
        torch.manual_seed(0)
        m = SirenWithSnakeTanh(2 * F if F else 1, 1, H, ns, nk, 0, first_omega_0=args.omega, hidden_omega_0=30.0,
                               a_initial=0.5)
        return SirenEngine(m, t, y, device=dev, encoding=GaussianEncoding(10.0, 1, F) if F else None)

    engines = {F: engine(F) for F in [0] + freqs}
    prof = {}
    for F, eng in engines.items():       # per-launch profile, eager steps (a run of its own)
        eng.step()
        _lib.check(lib.siren_profile_enable(4096), "profile")
        for _ in range(10):
            eng.step()
        torch.cuda.synchronize()
        prof[F] = {k: v[0] / 10 for k, v in _lib.profile_read().items() if v[1]}
        _lib.check(lib.siren_profile_enable(0), "profile off")
    step = {F: [] for F in engines}
    for eng in engines.values():
        eng.capture_graph()
    for _ in range(args.rounds):
        for F, eng in engines.items():
            eng.step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                eng.step()
            e1.record()
            torch.cuda.synchronize()
            step[F].append(e0.elapsed_time(e1) / args.steps)
    for F in engines:
        ts = sorted(step[F])
        rec = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "profile_ms_per_step": prof[F],
               "overflows": engines[F].guard_state()["overflows"]}
        if F:
            fl = 2.0 * R * 2 * F * H
            dw = prof[F].get("bwd_dw", 0.0) - prof[0].get("bwd_dw", 0.0)
            rec["dw0_ms"] = dw
            rec["dw0_fraction_of_f32_mfma_peak"] = fl / (dw * 1e-3) / PEAK_F32_MFMA if dw > 0 else None
            rec["first_fwd_profile_ms"] = prof[F].get("first_fwd")
        out["step"][F] = rec
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
