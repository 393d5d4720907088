"""Bit-identity of the KAN kernels across two builds of the library (tools/build_at.py makes one
from an earlier commit), kernel by kernel, in ONE process on the same seeded inputs and NaN-filled
workspaces: every (in, out, rows, splits) case of tests/test_gpu_kan_kernels.py through
siren_kan_forward and siren_kan_backward with and without grad_coords, and the [1, h, 1]
siren_kan_train_step cases of test_head_train_vs_unfused_route, and one whole step of
KAN([1, H, H, 1]), H = 64 and 128, at bench.py cfg5's 441 000 rows (the base library twice there:
"differing_on_repeat" tells whether the step repeats at all).  Compared as bit patterns (NaN
included): out, g, the flat gradient vector, dX and the whole workspace (W, W^T, X[l], dW, slabs,
Gin).  Prints one JSON object; "differing" must be 0.  --general runs the comparison through the
any-grid-size kernel set instead: grid_size 1, 11, 64, and 5 under SIREN_OPT_KAN_GENERAL, on the layer
cases of tests/test_gpu_kan_grids.py (_fwd_cases, _bwd_cases) and [1, 3, 1] and [1, 64, 1] steps under
MSE and L1 (a few hundred rows each).

    python tools/kan_ab.py --libs parent=inr-for-audio_amd/libsiren_parent.so,this=inr-for-audio_amd/libsiren_hip.so
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _params(fn, k=1):
    """The argvalues of a test's (first) pytest.mark.parametrize."""
    return [m for m in fn.pytestmark if m.name == "parametrize"][-1].args[k]


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()  # stays on its device: a workspace is up to 1 GB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True, help="base=path,other=path (paths relative to the repo root)")
    ap.add_argument("--step-rows", type=int, default=441_000, help="rows of the whole-step cases (bench.py cfg5's)")
    ap.add_argument("--general", action="store_true", help="compare through the any-grid-size kernel set")
    args = ap.parse_args()
    if args.general:
        return general_main(args)
    import test_gpu_kan_kernels as T
    from inr_for_audio_amd import _lib
    libs = {}
    for item in args.libs.split(","):
        nm, path = item.split("=")
        libs[nm] = _lib.bind(os.path.join(ROOT, path), check_abi=False)
    (base, lib_a), (other, lib_b) = libs.items()
    dev = torch.device("cuda:0")

    layer_cases = {(fin, fout, rows, 1) for fin, fout, rows in T.FWD_CASES}
    layer_cases |= {c[:4] for c in T.BWD_CASES}
    layer_cases |= {(fin, 8 * fin, 2060, 1) for fin in _params(T.test_fused_forward_bases_bit_exact)}
    layer_cases |= {(fin, 8 * fin, 1760, 4) for fin, _ in _params(T.test_basis_derivative_value_fused)}
    layer_cases |= {(1, 16, 4161, 66)}  # test_slab_reduce_16_via_layer_backward

    def layer_run(lib, case):
        fin, fout, rows, splits = case
        _, _, _, G, net = T._layer_case(lib, dev, fin, fout, rows, splits)
        net.b.zero_grads = 1
        got = {"out": _bits(torch.from_numpy(net.forward()))}
        for want_dx in (True, False):
            net.flat.fill_(float("nan"))
            _, dx = net.backward(G, want_dx)
            tag = "dx" if want_dx else "nodx"
            got[f"grads_{tag}"] = _bits(net.flat)
            got[f"ws_{tag}"] = _bits(net.ws)
            if want_dx:
                got["dX"] = _bits(torch.from_numpy(dx))
        return got

    def head_run(lib, case):
        h, rows, n_valid = case
        data, make = T._two_layer(lib, dev, h, rows, 3, h)
        y = data[5].copy()
        y[n_valid:] = np.nan
        net = make().bind(data[4], 3, target=y, n_valid=n_valid, n_total=1234.0)
        net.flat.fill_(float("nan"))
        net.b.zero_grads = 1
        out, g = net.train_step()
        return {"out": _bits(torch.from_numpy(out)), "g": _bits(torch.from_numpy(g)), "grads": _bits(net.flat),
                "ws": _bits(net.ws)}

    def step_run(lib, case):
        """siren_kan_train_step of KAN([1, H, H, 1]) at bench.py cfg5's rows and KanEngine's splits."""
        H, rows = case
        widths = [1, H, H, 1]
        layers = [(T.kr.kan_knots(widths[l], 700 + l), *T._weights(widths[l], widths[l + 1], 710 + l)) for l in range(3)]
        y = np.random.default_rng(H).normal(size=rows).astype(T.F32)
        net = T.Net(lib, dev, widths, layers).bind(T._inputs(layers[0][0], rows, H), max(1, min(256, rows // 2048)),
                                                   target=y, n_valid=rows, n_total=float(rows))
        net.flat.fill_(float("nan"))
        net.b.zero_grads = 1
        out, g = net.train_step()
        return {"out": _bits(torch.from_numpy(out)), "g": _bits(torch.from_numpy(g)), "grads": _bits(net.flat),
                "ws": _bits(net.ws)}

    res = {"libs": {nm: p for nm, p in (i.split("=") for i in args.libs.split(","))}, "cases": {}, "compared": 0,
           "differing": 0, "differing_on_repeat": 0}
    for kind, run, cases in (("layer", layer_run, sorted(layer_cases)),
                             ("head_train", head_run, list(_params(T.test_head_train_vs_unfused_route))),
                             ("step", step_run, [(h, args.step_rows) for h in (64, 128)])):
        for case in cases:
            a, b = run(lib_a, tuple(case)), run(lib_b, tuple(case))
            bad = {k: int((a[k] != b[k]).sum()) for k in a}
            if kind == "step":  # the base library once more: is the step repeatable at all
                a2 = run(lib_a, tuple(case))
                res["differing_on_repeat"] += sum(int((a[k] != a2[k]).sum()) for k in a)
            res["compared"] += sum(v.numel() for v in a.values())
            res["differing"] += sum(bad.values())
            res["cases"][f"{kind}{tuple(case)}"] = {k: v for k, v in bad.items() if v} or 0
    print(json.dumps(res))
    return 1 if res["differing"] else 0


def general_main(args):
    import test_gpu_kan_grids as T
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd._lib import Opt, options
    (base, lib_a), (other, lib_b) = [(nm, _lib.bind(os.path.join(ROOT, path), check_abi=False))
                                     for nm, path in (i.split("=") for i in args.libs.split(","))]
    dev = torch.device("cuda:0")

    def layer_run(lib, case):
        G, fin, fout, rows, splits = case
        _, _, _, up, net = T._layer_case(lib, dev, G, fin, fout, rows, splits)
        net.b.zero_grads = 1
        got = {"out": _bits(torch.from_numpy(net.forward()))}
        for want_dx in (True, False):
            net.flat.fill_(float("nan"))
            _, dx = net.backward(up, want_dx)
            tag = "dx" if want_dx else "nodx"
            got[f"grads_{tag}"] = _bits(net.flat)
            got[f"ws_{tag}"] = _bits(net.ws)
            if want_dx:
                got["dX"] = _bits(torch.from_numpy(dx))
        return got

    def step_run(lib, case):
        G, h, loss_mode = case
        rows = 300
        data, make = T._two_layer(lib, dev, G, h, rows, 3, h + G)
        y = data[5].copy()
        y[270:] = np.nan
        net = make().bind(data[4], 3, target=y, n_valid=270, n_total=1234.0)
        net.flat.fill_(float("nan"))
        net.b.zero_grads = 1
        out, g = net.train_step(loss_mode)
        got = {"out": _bits(torch.from_numpy(out)), "g": _bits(torch.from_numpy(g)), "grads": _bits(net.flat),
               "ws": _bits(net.ws)}
        net.flat.fill_(float("nan"))
        net.step_backward(g)
        got["grads_step_backward"] = _bits(net.flat)
        return got

    res = {"libs": {base: None, other: None}, "set": "general", "cases": {}, "compared": 0, "differing": 0}
    res["libs"] = {nm: p for nm, p in (i.split("=") for i in args.libs.split(","))}
    for G in (1, 5, 11, 64):
        layers = sorted({(G, fin, fout, rows, 1) for fin, fout, rows in T._fwd_cases(G)} | {(G, *c) for c in T._bwd_cases(G)})
        steps = [(G, h, mode) for h in (3, 64) for mode in (0, 1)]
        for kind, run, cases in (("layer", layer_run, layers), ("step", step_run, steps)):
            for case in cases:
                got = []
                for lib in (lib_a, lib_b):
                    with options(lib, {Opt.KAN_GENERAL: 1}):
                        got.append(run(lib, case))
                a, b = got
                bad = {k: int((a[k] != b[k]).sum()) for k in a}
                res["compared"] += sum(v.numel() for v in a.values())
                res["differing"] += sum(bad.values())
                res["cases"][f"{kind}{case}"] = {k: v for k, v in bad.items() if v} or 0
    print(json.dumps(res))
    return 1 if res["differing"] else 0


if __name__ == "__main__":
    sys.exit(main())
