"""Generate tests/golden/kan_regrid.npz from the REFERENCE's kan.py, for the refit of a KANLinear
onto a grid of another size (KANLinear.regrid / KAN.regrid of the HIP path).

Runs where the reference (senyuanfan/inr-for-audio) is mounted, on the CPU; imports its own kan.py
and writes data only.  The reference has no regrid, so a case drives its methods alone:

  equal sizes    lay = KANLinear(in, out, grid_size=G) with spline_scaler set to ones;
                 lay.update_grid(x) -- the reference's own refit (with a unit scaler its stored
                 result is the plain least-squares refit, which is what regrid computes)
  unequal sizes  new = KANLinear(in, out, grid_size=Gn); new.update_grid(x) sets the knots;
                 new.curve2coeff(x, bmm(old.b_splines(x), old.scaled_spline_weight)) the coefficients

Old grids are non-uniform: one prior reference update on uniform random data.  Each case stores the
inputs, the old layer, the reference's knots and coefficients, and the reference's own coefficient
error against the fp64 restatement tests/kan_regrid_ref.py on the same knots (``ref_err``).

    python tests/golden/make_golden_kan_regrid.py [--ref /root/reference]

Asserted here, with the reference alone: every new knot row is non-decreasing; every solvable case
has ref_err <= 1e-4 and a worst Cholesky pivot ratio above 2^-24 (below about that the reference's
fp32 lstsq falls back to a minimum-norm answer, its error becomes 1 and a gate of 4 x ref_err would
hide anything); the refusal cases (Gn + 2 rows) fail the factorisation.
"""
import argparse
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import kan_regrid_ref as rr  # noqa: E402

F32 = np.float32
GEN = {
    "randn": lambda n, i: torch.randn(n, i),
    "linspace": lambda n, i: torch.linspace(-1, 1, n).reshape(n, 1).repeat(1, i),
    "ties": lambda n, i: torch.round(torch.randn(n, i) * 8) / 8,
    "tanh": lambda n, i: torch.tanh(3 * torch.randn(n, i)),
}
# name: (Go, Gn, input kind, rows, in, out); the pairs are kan_regrid_ref.PAIRS
CASES = {
    "p5_5": (5, 5, "randn", 2049, 4, 3),
    "p5_10": (5, 10, "randn", 2049, 5, 3),
    "p1_2": (1, 2, "linspace", 20, 3, 2),
    "p4_11": (4, 11, "ties", 2049, 4, 2),
    "p11_4": (11, 4, "tanh", 2049, 17, 8),
    "p16_64": (16, 64, "randn", 268, 3, 4),
    "p64_64": (64, 64, "linspace", 2049, 2, 3),
    "p64_1": (64, 1, "randn", 2049, 5, 2),
    "p6_6": (6, 6, "ties", 36, 3, 2),
    "exact5_10": (5, 10, "linspace", 13, 2, 2),     # exactly Gn + 3 rows
    # Gn + 2 rows: refused.  Small Gn only: the last pivot of such a G_nn is rounding noise of the fp64
    # sums magnified by the pivots before it, and at Gn = 11 (13 rows, normal or equispaced) that noise
    # lands above the 2^-40 of the rank rule for some inputs, in numpy and on the device alike
    "rank11_4": (11, 4, "randn", 6, 2, 2),
    "rank64_1": (64, 1, "randn", 3, 3, 2),
    "rank6_6": (6, 6, "randn", 8, 2, 2),
}
STACK_WIDTHS, STACK_ROWS, PRIOR_ROWS = [1, 8, 8, 1], 3001, 512
# (Go, Gn): (seed, KAN keywords).  The hidden layers' inputs are activations, clustered and of a small
# range, and under most seeds the reference's fp32 lstsq breaks on one of them (its error against fp64
# is 0.1 to 1): these seeds keep every layer inside the caps of the layer cases, asserted below.
STACKS = {(5, 10): (20, {"scale_noise": 1.0}), (4, 11): (20, {})}


def np32(t):
    return t.detach().numpy().astype(F32).copy()


def layer_state(lay):
    return np32(lay.grid), np32(lay.base_weight), np32(lay.spline_weight), np32(lay.spline_scaler)


def ref_regrid(ref_kan, old, x, Gn, scaled=True):
    """(new knots, coefficients) from the reference's methods alone (module docstring); scaled=False
    fits the curves of the unscaled spline_weight, the target KANLinear.regrid uses."""
    new = ref_kan.KANLinear(old.in_features, old.out_features, grid_size=Gn)
    with torch.no_grad():
        new.update_grid(x)
        coeff = (old.scaled_spline_weight if scaled else old.spline_weight).permute(1, 2, 0)
        curves = torch.bmm(old.b_splines(x).permute(1, 0, 2), coeff).permute(1, 0, 2)
        return new, new.curve2coeff(x, curves)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import kan as ref_kan  # noqa: E402  (the reference's own module)

    out, report = {}, []
    for k, (name, (Go, Gn, kind, rows, fin, fout)) in enumerate(CASES.items()):
        torch.manual_seed(300 + k)
        old = ref_kan.KANLinear(fin, fout, grid_size=Go)
        with torch.no_grad():
            old.update_grid(torch.rand(PRIOR_ROWS, fin) * 2 - 1)  # the non-uniform starting grid
            if Go == Gn:
                old.spline_scaler.fill_(1.0)
        x = GEN[kind](rows, fin).float()
        grid, bw, sw, sc = layer_state(old)
        assert (np.diff(grid, axis=1) > 0).all()
        out.update({f"{name}_x": np32(x), f"{name}_grid": grid, f"{name}_base_weight": bw,
                    f"{name}_spline_weight": sw, f"{name}_spline_scaler": sc, f"{name}_sizes": np.array([Go, Gn])})
        if Go == Gn:
            with torch.no_grad():
                old.update_grid(x)
            new_grid, new_sw = np32(old.grid), np32(old.spline_weight)
        else:
            new, coeff = ref_regrid(ref_kan, old, x, Gn)
            new_grid, new_sw = np32(new.grid), np32(coeff)
        assert (np.diff(new_grid, axis=1) >= 0).all(), name
        assert np.array_equal(new_grid, rr.knots32(np32(x), Gn, old.grid_eps, 0.01)), \
            f"{name}: knots32 is not the reference's knot arithmetic"
        out[f"{name}_new_grid"] = new_grid
        g_nn, _ = rr.gram(np32(x), grid, new_grid)
        worst = min(rr.pivot_ratios(g_nn[i]).min() for i in range(fin))
        if name.startswith("rank"):
            assert rows == Gn + 2 and len(rr.rank_deficient(g_nn)) == fin, name
            report.append(f"{name}: refused, worst pivot ratio 2^{np.log2(max(worst, 1e-300)):.1f}")
            continue
        c64 = rr.refit(np32(x), grid, new_grid, sw * sc[..., None])
        err = rr.coeff_error(new_sw, c64)
        assert err <= 1e-4 and worst > 2.0 ** -24, (name, err, worst)
        out.update({f"{name}_new_spline_weight": new_sw, f"{name}_ref_err": np.float64(err)})
        report.append(f"{name}: {Go} -> {Gn} {kind} {rows} x {fin}: reference error {err:.2e}, worst pivot ratio "
                      f"2^{np.log2(worst):.1f}")

    # the stacks: KAN([1, 8, 8, 1]) on 3001 coordinates, per layer the reference's knots and fit of the
    # unscaled curves, base_weight and spline_scaler carried over (KAN.regrid's definition)
    x = torch.linspace(-1, 1, STACK_ROWS).reshape(-1, 1)
    out["stack_x"] = np32(x)
    for (Go, Gn), (seed, kw) in STACKS.items():
        torch.manual_seed(seed)
        model = ref_kan.KAN(STACK_WIDTHS, grid_size=Go, **kw)
        with torch.no_grad():
            model(torch.rand(PRIOR_ROWS, 1) * 2 - 1, update_grid=True)
            y_old = model(x)
        olds = [layer_state(lay) for lay in model.layers]
        h = x
        for lay, st in zip(model.layers, olds):
            new, coeff = ref_regrid(ref_kan, lay, h, Gn, scaled=False)
            g_nn, _ = rr.gram(np32(h), st[0], np32(new.grid))
            worst = min(rr.pivot_ratios(g_nn[i]).min() for i in range(len(g_nn)))
            lerr = rr.coeff_error(np32(coeff), rr.refit(np32(h), st[0], np32(new.grid), st[2]))
            assert lerr <= 1e-4 and worst > 2.0 ** -24, (Go, Gn, lerr, worst)
            with torch.no_grad():
                new.base_weight.copy_(lay.base_weight)
                new.spline_scaler.copy_(lay.spline_scaler)
                new.spline_weight.copy_(coeff)
                h = new(h)
        y64, _ = rr.stack_regrid(np32(x), olds, Gn)
        tag = f"stack{Go}_{Gn}"
        err = float(np.abs(np32(h) - y64).max() / np.abs(y64).max())
        for l, st in enumerate(olds):
            for nm, a in zip(("grid", "base_weight", "spline_weight", "spline_scaler"), st):
                out[f"{tag}_l{l}_{nm}"] = a
        out[f"{tag}_out"], out[f"{tag}_out_ref_err"] = np32(h), np.float64(err)
        change = float(np.abs(np32(h) - np32(y_old)).max() / np.abs(np32(y_old)).max())
        report.append(f"{tag}: output reference error {err:.2e}; the regrid changes the output by {change:.2e}")

    path = os.path.join(OUT, "kan_regrid.npz")
    np.savez_compressed(path, **out)
    print("\n".join(report))
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
