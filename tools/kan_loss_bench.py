"""Step times of the KAN fit under every loss of run.py:124-128, :160-169 on the HIP path.

    python tools/kan_loss_bench.py [--rows 441000] [--width 64] [--wide 256] [--steps 10] [--out FILE]

KAN([1, W, W, 1]) at `rows` coordinates, one whole step (gradients + Adam + scheduler) replayed from a
captured graph, the median of `steps` replays by device events:

  mse, mae           the one-pass steps (siren_kan_train_step_loss)
  each (loss_mode, alpha, stft_loss) of the phased step with 1 and with 2 micro-batches, beside the three
  signal-level loss calls' own time on that engine's signal (so step - loss - mse is what the phasing costs:
  the unfused head forward, the copies, and with 2 micro-batches the second forward)

then `kan_head_bwd` against what it replaces, `kan_bwd_fused` on the same W -> 1 layer and rows, both
bracketed by the library's own launch profiling in KAN([1, W, 1]); then mse / mae / one spectral
combination at --wide, where the head is unfused.  One JSON line.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPECTRAL = [("mse", 0.2, "stft"), ("mae", 0.2, "stft"), ("mae", 1.0, "stft"), ("snr", 0.0, "stft"),
            ("snr", 0.2, "stft"), ("mae", 0.2, "mrstft"), ("snr", 0.2, "mrstft")]


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


def engine(width, rows, dev, **kw):
    from inr_for_audio_amd.engine import KanEngine
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(0)
    x, y = data(rows)
    return KanEngine(KAN([1, width, width, 1]), x, y, device=dev, **kw)


def step_ms(eng, steps):
    eng.step()
    eng.capture_graph()
    return median_ms(eng.step, steps)


def loss_calls_ms(eng, steps):
    """The three signal-level calls of the phased step alone, on the engine's own out_sig."""
    from inr_for_audio_amd._lib import check, ptr
    lib, N, s = eng.lib, eng.n_total, torch.cuda.current_stream(eng.device).cuda_stream
    prefix = "siren_" + eng.stft_loss
    x, y, basis, ws = ptr(eng.out_sig), ptr(eng.target_sig), ptr(eng.stft_basis), ptr(eng.stft_ws)
    mode, alpha = eng.loss_mode_id, eng.alpha
    loss = torch.zeros(4, device=eng.device)

    def calls():
        check(getattr(lib, prefix + "_signal_forward")(x, y, N, N, mode, alpha, basis, ws, eng._sig_win, s))
        check(getattr(lib, prefix + "_signal_finish")(N, N, mode, alpha, ws, ptr(loss), s))
        check(getattr(lib, prefix + "_signal_backward")(x, y, N, N, mode, alpha, basis, ws, eng._sig_win, 0, N,
                                                        ptr(eng.g_sig), s))
    return median_ms(calls, steps)


def head_backward_ms(width, rows, dev, reps):
    """kan_head_bwd (siren_kan_step_backward) and kan_bwd_fused at out = 1 (siren_kan_backward) on the last
    layer of KAN([1, W, 1]): the launches of that layer, slab reduce included, by the library's profiling.
    Both routes share the first layer's kan_dw_fused, which the kan_dw kind of the second route measures."""
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd._lib import check
    from inr_for_audio_amd.engine import KanEngine
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(0)
    x, y = data(rows)
    eng = KanEngine(KAN([1, width, 1]), x, y, device=dev)
    lib, s, b = eng.lib, torch.cuda.current_stream(dev).cuda_stream, eng.batches[0]
    net, gr = ctypes.byref(eng.net), ctypes.byref(eng.grad_struct)
    check(lib.siren_kan_train_step(net, gr, ctypes.byref(b), s))          # a g of the fit's size
    g = eng.g.clone()
    check(lib.siren_kan_forward(net, ctypes.byref(b), s))
    eng.g.copy_(g)
    out = {}
    for name, call in (("step_backward", lambda: lib.siren_kan_step_backward(net, gr, ctypes.byref(b), s)),
                       ("backward", lambda: lib.siren_kan_backward(net, gr, ctypes.byref(b), None, s))):
        check(call())
        torch.cuda.synchronize(dev)
        check(lib.siren_profile_mask(0xFFFFFFFF))
        check(lib.siren_profile_enable(64 * (reps + 1)))
        for _ in range(reps):
            check(call())
        torch.cuda.synchronize(dev)
        out[name] = {k: v[0] / reps for k, v in _lib.profile_read().items() if v[1]}
        check(lib.siren_profile_enable(0))
    first_dw = out["backward"]["kan_dw"]
    return {"kan_head_bwd_ms": out["step_backward"]["kan_dw"] - first_dw, "kan_bwd_fused_out1_ms": out["backward"]["kan_dx"],
            "first_layer_dw_ms": first_dw, "kinds_ms": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=441000)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--wide", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(diag=False)
    dev = torch.device("cuda:0")
    res = {"rows": a.rows, "width": a.width, "device": torch.cuda.get_device_name(0), "step_ms": {}, "spectral": []}
    for mode in ("mse", "mae"):
        res["step_ms"][mode] = step_ms(engine(a.width, a.rows, dev, loss_mode=mode), a.steps)
    for mode, alpha, kind in SPECTRAL:
        row = {"loss_mode": mode, "alpha": alpha, "stft_loss": kind}
        for n_micro in (1, 2):
            eng = engine(a.width, a.rows, dev, loss_mode=mode, alpha=alpha, stft_loss=kind, split_spectral=True,
                         micro_batch=-(-a.rows // n_micro))
            assert eng.n_micro == n_micro
            row[f"step_ms_{n_micro}"] = step_ms(eng, a.steps)
            if n_micro == 1:
                row["loss_calls_ms"] = loss_calls_ms(eng, a.steps)
            del eng
        res["spectral"].append(row)
    res["head_backward"] = head_backward_ms(a.width, a.rows, dev, a.steps)
    wide = {"width": a.wide}
    for mode in ("mse", "mae"):
        wide[mode] = step_ms(engine(a.wide, a.rows, dev, loss_mode=mode), a.steps)
    for n_micro in (1, 2):
        wide[f"mae_0.2_stft_{n_micro}"] = step_ms(engine(a.wide, a.rows, dev, loss_mode="mae", alpha=0.2, split_spectral=True,
                                                         micro_batch=-(-a.rows // n_micro)), a.steps)
    res["wide"] = wide
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
