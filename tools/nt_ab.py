"""Bit-identity of the NT GEMM kernels (gemm_nt.hip) across two builds of the library (tools/build_at.py
makes one from an earlier commit), in ONE process on the same seeded inputs and NaN-filled outputs.

Kernel level: the launches of tests/test_gpu_walk.py, test_gpu_kernels.py (the NT ones), test_gpu_act.py,
test_gpu_headfuse.py, test_gpu_headfuse_act.py and test_gpu_queue.py at R = 2560 rows and H in {256, 512,
1024}, through the C-ABI entry points, under these launch configurations:

    tile 128 (NtSmall) | tile 256 pipe 0 (NtLarge, one tile per block) | pipe 1 (NtLarge, persistent, grids 0 and
    3) | pipe 4 (NtLargePP: static walk at grids 0 and 3, the tile queue at grid 8 with SIREN_OPT_NT_QUEUE 1)

with and without the head partials, with and without the backward scale, Snake at a = 0.5 and 50, the
whole-line Snake / Tanh / dX-Snake epilogues (ACTL) at H <= 512 and the plain ones at 1024, and the fused last
layer of the three kinds (NT_FWD_HB*, ping-pong only).  Step level: one siren_train_step (two launches: a Snake
last layer runs fused from the second) of a sine 3 x 256 stack, the live Snake stack, a Tanh stack and a
first_linear stack at 4096 rows on the 256 tiles with 8 blocks under SIREN_OPT_NT_QUEUE 0 / 1 / 2 (2 sends dX /
dX0 through the queue kernels); the base library runs each step twice ("differing_on_repeat": does the step
repeat at all).  Two kinds of kernel have no C-ABI launch that reaches all their instantiations, so steps reach
them: NT_DX0_SNAKE runs only inside a first_linear step (NtLargePP above; NtSmall in a step on the 128 tile,
NtLarge in steps at pipe 1 and pipe 0), and siren_inner_bwd_dx_act takes no tile queue, so the queued
NT_DX_SNAKE without ACTL runs in a 1024-wide Snake step under SIREN_OPT_NT_QUEUE 2.  Compared as bit patterns
(NaN included).  Prints one JSON object (and writes it to
--out); "differing" must be 0.

    python tools/nt_ab.py --libs parent=inr-for-audio_amd/libsiren_parent.so,this=inr-for-audio_amd/libsiren_hip.so
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

R = 2560
WIDTHS = (256, 512, 1024)
SINE, SNAKE, TANH = 0, 1, 2
F16 = torch.float16


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True, help="base=path,other=path (paths relative to the repo root)")
    ap.add_argument("--out", default="", help="also write the JSON object to this file")
    args = ap.parse_args()
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd._lib import Opt
    libs = {}
    for item in args.libs.split(","):
        nm, path = item.split("=")
        libs[nm] = _lib.bind(os.path.join(ROOT, path), check_abi=False)
    (base, lib_a), (other, lib_b) = libs.items()
    dev = torch.device("cuda:0")
    S = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    f = ctypes.c_float
    tq = _lib.new_tileq(dev)

    def nans(*shape, dtype=F16):
        return torch.full(shape, float("nan"), dtype=dtype, device=dev)

    def inputs(H):
        g = torch.Generator(device=dev).manual_seed(H)
        u = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
        d = {"X": torch.sin(u(R, H) * 6.2831853).to(F16),
             "W": ((u(H, H) * 2 - 1) * (6 / H) ** 0.5 / 30).to(F16),
             "Wa": ((u(H, H) * 2 - 1) * (1 / H) ** 0.5).to(F16),  # Snake / Tanh layers: Linear's own scale
             "b": (u(H) - 0.5) * 0.06, "hw": (u(H) - 0.5) * 0.02, "bh": (u(1) - 0.5) * 0.1,
             "Cp": torch.cos(u(R, H) * 6.2831853).to(F16), "D": (u(R, H) * 2).to(F16),
             "Ep": ((u(R, H) - 0.5) * 2).to(F16),
             "dZ": (torch.randn(R, H, device=dev, generator=g) * 1e-3).to(F16),
             "t": u(R, 2) * 2 - 1, "y": (u(R) - 0.5),
             "a": {0.5: 0.5 * (0.5 + u(H)), 50.0: 50.0 * (0.5 + u(H))}}
        d["WT"] = d["W"].t().contiguous()
        return d

    scales = {None: None, **{k: torch.tensor([2.0 ** k, 2.0 ** -k], device=dev) for k in (5, 9)}}
    gscale = scales.__getitem__  # the tensors outlive every launch that reads them

    # every case: (name, fn(lib, inputs, H) -> output tensors, NaN-filled before the launch)
    def fwd(head):
        def run(lib, d, H):
            Y, C, hp = nans(R, H), nans(R, H), nans(H // 128, R, dtype=torch.float32)
            _lib.check(lib.siren_inner_fwd(P(d["X"]), P(d["W"]), P(d["b"]), f(30.0), R, H, P(Y), P(C),
                                           P(d["hw"]) if head else None, P(hp) if head else None, P(tq), S()), "fwd")
            return Y, C, hp
        return run

    def fwd_act(act, amag, head):
        def run(lib, d, H):
            Y, C, E, hp = nans(R, H), nans(R, H), nans(R, H), nans(H // 128, R, dtype=torch.float32)
            _lib.check(lib.siren_inner_fwd_act(P(d["X"]), P(d["Wa"]), P(d["b"]), act, f(30.0), P(d["a"][amag]), R, H,
                                               P(Y), P(C), P(E), P(d["hw"]) if head else None,
                                               P(hp) if head else None, P(tq), S()), "fwd_act")
            return Y, C, E, hp
        return run

    def dx(k):
        def run(lib, d, H):
            out, part = nans(R, H), nans(R // 128, H, dtype=torch.float32)
            _lib.check(lib.siren_inner_bwd_dx(P(d["dZ"]), P(d["WT"]), P(d["Cp"]), f(30.0), R, H, P(gscale(k)), P(out),
                                              P(part), S()), "dx")
            return out, part
        return run

    def dx_act(act, k):
        def run(lib, d, H):
            out, part = nans(R, H), nans(R // 128, 2, H, dtype=torch.float32)
            _lib.check(lib.siren_inner_bwd_dx_act(P(d["dZ"]), P(d["WT"]), P(d["D"]), P(d["Ep"]) if act == SNAKE else None,
                                                  act, f(30.0), R, H, P(gscale(k)), P(out), P(part), S()), "dx_act")
            return out, part
        return run

    def dx0(in_dim, k):
        def run(lib, d, H):
            part = nans(R // 128, 1 + in_dim, H, dtype=torch.float32)
            t = d["t"][:, :in_dim].contiguous()
            _lib.check(lib.siren_first_bwd_dx(P(d["dZ"]), P(d["WT"]), P(d["Cp"]), P(t), in_dim, f(1000.0), R, H,
                                              P(gscale(k)), P(part), S()), "dx0")
            return (part,)
        return run

    def hb(act, amag, head_omega, loss_mode, n_valid):
        def run(lib, d, H):
            o = {"hp": nans(H // 128, R, dtype=torch.float32), "out": nans(R, dtype=torch.float32),
                 "g": nans(R, dtype=torch.float32), "sse": nans(R // 256, dtype=torch.float32),
                 "gsum": nans(R // 256, dtype=torch.float32), "gmax": nans(R // 256, dtype=torch.float32),
                 "dZ": nans(R, H), "part": nans(R // 256, 3, H, dtype=torch.float32), "E": nans(R, H)}
            _lib.check(lib.siren_head_fused_fwd_act(
                P(d["X"]), P(d["W"] if act == SINE else d["Wa"]), P(d["b"]), act, f(30.0), P(d["a"][amag]), R, H,
                P(d["hw"]), P(d["bh"]), f(head_omega), P(d["y"]), n_valid, float(n_valid), loss_mode, P(gscale(9)),
                P(o["hp"]), P(o["out"]), P(o["g"]), P(o["sse"]), P(o["gsum"]), P(o["gmax"]), P(o["dZ"]), P(o["part"]),
                P(o["E"]), S()), "hb")
            # head_part is hand-off scratch (every word published): compared as well
            return tuple(o.values())
        return run

    plain = [(f"fwd[head={h}]", fwd(h)) for h in (False, True)]
    plain += [(f"fwd_act[{a},{m},head={h}]", fwd_act(a, m, h))
              for a, m in ((SNAKE, 0.5), (SNAKE, 50.0), (TANH, 0.5)) for h in (False, True)]
    plain += [(f"dx[k={k}]", dx(k)) for k in (None, 9)]
    plain += [(f"dx_act[{a},k={k}]", dx_act(a, k)) for a in (SNAKE, TANH) for k in (None, 9)]
    plain += [(f"dx0[in={i},k={k}]", dx0(i, k)) for i, k in ((1, None), (2, 5))]
    fused = [(f"hb[{a},{m},ho={ho},loss={lm},n={nv}]", hb(a, m, ho, lm, nv))
             for a, m in ((SINE, 0.5), (SNAKE, 0.5), (SNAKE, 50.0), (TANH, 0.5))
             for ho, lm, nv in ((0.0, 0, R), (30.0, 0, R - 60), (0.0, 1, R - 60))]
    configs = [("tile128", {Opt.NT_TILE: 128}, plain),
               ("tile256/pipe0", {Opt.NT_TILE: 256, Opt.NT_PIPE: 0}, plain),
               ("tile256/pipe1/grid0", {Opt.NT_TILE: 256, Opt.NT_PIPE: 1}, plain),
               ("tile256/pipe1/grid3", {Opt.NT_TILE: 256, Opt.NT_PIPE: 1, Opt.NT_GRID: 3}, plain),
               ("tile256/pipe4/grid0/queue0", {Opt.NT_TILE: 256, Opt.NT_PIPE: 4, Opt.NT_QUEUE: 0}, plain + fused),
               ("tile256/pipe4/grid3/queue0", {Opt.NT_TILE: 256, Opt.NT_PIPE: 4, Opt.NT_GRID: 3, Opt.NT_QUEUE: 0},
                plain + fused),
               ("tile256/pipe4/grid8/queue1", {Opt.NT_TILE: 256, Opt.NT_PIPE: 4, Opt.NT_GRID: 8, Opt.NT_QUEUE: 1},
                plain + fused)]

    res = {"libs": dict(i.split("=") for i in args.libs.split(",")), "rows": R, "widths": list(WIDTHS), "cases": {},
           "launches": 0, "compared": 0, "differing": 0, "differing_on_repeat": 0}

    def compare(name, a, b):
        bad = [int((_bits(x) != _bits(y)).sum()) for x, y in zip(a, b)]
        res["compared"] += sum(x.numel() for x in a)
        res["differing"] += sum(bad)
        res["cases"][name] = bad if any(bad) else 0

    for H in WIDTHS:
        d = inputs(H)
        for cname, opts, cases in configs:
            with _lib.options(lib_a, opts), _lib.options(lib_b, opts):
                for name, run in cases:
                    a = run(lib_a, d, H)
                    b = run(lib_b, d, H)
                    torch.cuda.synchronize()
                    res["launches"] += 1
                    compare(f"H{H}/{cname}/{name}", a, b)
        del d

    # ---- whole steps: the engine is built on the package's library, then launched through each build
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.models import SirenWithSnakeTanh

    def stack(kind, hidden):
        torch.manual_seed(3)
        cfg, a0, fl, ll = {"sine": ((3, 0, 0), 50.0, False, True), "snake_live": ((0, 4, 0), 50.0, False, True),
                           "tanh": ((1, 0, 3), 0.5, False, True), "first_linear": ((1, 1, 1), 0.5, True, False)}[kind]
        return SirenWithSnakeTanh(1, 1, hidden, *cfg, first_linear=fl, last_linear=ll, first_omega_0=1000.0,
                                  hidden_omega_0=30.0, a_initial=a0)

    n = 4096
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    y = 0.5 * torch.sin(37 * t) + 0.3 * torch.sin(91 * t + 0.5)

    def step(lib, kind, hidden):
        eng = SirenEngine(stack(kind, hidden), t, y, lr=1e-3, device=dev)
        eng.lib = lib
        got = []
        for _ in range(2):
            eng._launch_grads()
            torch.cuda.synchronize()
            got += [eng.grads.clone(), eng.ws.out.clone(), eng.ws.g.clone()]
        return got

    large = {Opt.NT_TILE: 256, Opt.TN_TILE: 256, Opt.NT_GRID: 8}
    steps = [(f"step/{kind}/queue{q}", kind, 256, {**large, Opt.NT_QUEUE: q})
             for kind in ("sine", "snake_live", "tanh", "first_linear") for q in (0, 1, 2)]
    steps += [("step/first_linear/tile128", "first_linear", 256, {Opt.NT_TILE: 128}),
              ("step/first_linear/pipe1", "first_linear", 256, {**large, Opt.NT_PIPE: 1}),
              ("step/first_linear/pipe0", "first_linear", 256, {**large, Opt.NT_PIPE: 0}),
              ("step/snake_live/H1024/queue2", "snake_live", 1024, {**large, Opt.NT_QUEUE: 2})]
    for name, kind, hidden, opts in steps:
        with _lib.options(lib_a, opts), _lib.options(lib_b, opts):
            a, b, a2 = step(lib_a, kind, hidden), step(lib_b, kind, hidden), step(lib_a, kind, hidden)
        res["launches"] += 3
        compare(name, a, b)
        res["step_nonfinite"] = res.get("step_nonfinite", 0) + sum(int((~torch.isfinite(x)).sum()) for x in a)
        res["differing_on_repeat"] += sum(int((_bits(x) != _bits(z)).sum()) for x, z in zip(a, a2))
    res["n_cases"] = len(res["cases"])
    text = json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, args.out)) or ".", exist_ok=True)
        with open(os.path.join(ROOT, args.out), "w") as fh:
            fh.write(text + "\n")
    return 1 if res["differing"] else 0


if __name__ == "__main__":
    sys.exit(main())
