"""Cost of the STFT / SNR losses (csrc/stft.hip; run.py:126-128, :160-169) at the reference's live
config (run.py:466): a first sine layer + 4 Snake hidden layers, width 256, 441 000 rows (10 s at 44.1 kHz; T = 1723 frames).

Three engines on the same signal, rounds interleaved, each step a graph replay with the profiler off:

* ``mse, alpha 0``    -- the default step (fused last layer), the yardstick of the same run;
* ``mae, alpha 0.2``  -- unfused head + the two DFT GEMMs + the mix;
* ``snr, alpha 0``    -- unfused head + the SNR sums.

The new kernels' own times come from a separate eager run with the library's per-launch profile
(SIREN_PROF_LOSS: all loss launches of a step), and from HIP events around `reps` back-to-back calls
of the individual entry points (forward GEMM, backward GEMM + gather, SNR); GEMM rates are
2 T 1024 1026 flops per direction over the 157.3 TFLOP/s fp32-MFMA peak.

    python tools/bench_losses.py [--rows 441000] [--hidden 256] [--rounds 5] [--steps 30] [--reps 20]
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
CONFIGS = {"mse_a0": ("mse", 0.0), "mae_a0.2": ("mae", 0.2), "snr_a0": ("snr", 0.0)}


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
    T = int(lib.siren_stft_frames(n))
    out = {"rows": n, "padded_rows": R, "hidden": H, "stack": [ns, nk], "frames": T, "step": {}, "kernels": {}}

    g = torch.Generator().manual_seed(0)
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    k = torch.arange(n, dtype=torch.float64)
    y = (0.5 * torch.sin(2 * torch.pi * 440 * k / 44100) + 0.2 * torch.sin(2 * torch.pi * 3100 * k / 44100 + 1)
         + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float()

    # ---- the individual kernels
    basis = stft_basis(dev)
    ws = torch.zeros(int(lib.siren_stft_workspace_floats(n, R)), device=dev)
    yd = y.to(dev)
    xd = (0.8 * yd + 0.05 * torch.randn(n, device=dev)).contiguous()
    loss, gbuf = torch.zeros(1, device=dev), torch.zeros(n, device=dev)
    _lib.check(lib.siren_stft_forward(P(yd), n, R, P(basis), P(ws), 1, s()), "stft target")
    calls = {
        "stft_forward": lambda: lib.siren_stft_forward(P(xd), n, R, P(basis), P(ws), 0, s()),
        "stft_scalars": lambda: lib.siren_stft_loss(n, R, P(ws), P(loss), s()),
        "stft_backward_and_gather": lambda: lib.siren_stft_loss_bwd(n, R, P(basis), P(ws), P(gbuf), s()),
        "snr_loss_and_grad": lambda: lib.siren_snr_loss(P(xd), P(yd), n, R, P(ws), P(loss), P(gbuf), s()),
    }
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
    fl = 2.0 * T * 1024 * 1026
    for name in calls:
        rec = med(times[name])
        if name in ("stft_forward", "stft_backward_and_gather"):
            rec["gemm_tflops"] = fl / (rec["median_ms"] * 1e-3) / 1e12
            rec["fraction_of_f32_mfma_peak"] = fl / (rec["median_ms"] * 1e-3) / PEAK_F32_MFMA
        out["kernels"][name] = rec

    # ---- whole steps
    def engine(loss_mode, alpha):
        torch.manual_seed(0)
        m = SirenWithSnakeTanh(1, 1, H, ns, nk, 0, first_omega_0=args.omega, hidden_omega_0=30.0, a_initial=0.5)
        return SirenEngine(m, t, y, device=dev, loss_mode=loss_mode, alpha=alpha)

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
    base = med(step["mse_a0"])["median_ms"]
    for name, eng in engines.items():
        rec = med(step[name])
        rec["over_mse_a0_ms"] = rec["median_ms"] - base
        rec["loss_kernels_ms_per_step"] = prof[name].get("loss", 0.0)
        rec["profile_ms_per_step"] = prof[name]
        rec["last_loss"] = eng.last_loss()
        rec["overflows"] = eng.guard_state()["overflows"]
        out["step"][name] = rec
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
