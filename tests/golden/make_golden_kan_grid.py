"""Generate tests/golden/kan_grid_update.npz from the REFERENCE's update_grid (kan.py:168-215).

Runs where the reference (senyuanfan/inr-for-audio) is mounted, on the CPU; imports its own kan.py
and writes data only: per case the inputs, the layer before the update (a non-uniform grid, made by
one prior reference update on uniform random data), the reference's new grid and spline_weight, and
the reference's own error against the fp64 restatement tests/kan_grid_ref.py on the same new knots.

    python tests/golden/make_golden_kan_grid.py [--ref /root/reference]

Asserted here, with the reference alone: every new knot row is strictly increasing; every solvable
case's worst Cholesky pivot ratio is above 2^-30 (2^10 clear of the kernels' refusal threshold
2^-40); the 7-row case fails the factorisation.
"""
import argparse
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import kan_grid_ref as gr  # noqa: E402

F32 = np.float32
# name: (rows, in, out, input generator)
CASES = {
    "normal": (257, 5, 3, lambda n, i: torch.randn(n, i)),
    "coords": (2049, 1, 16, lambda n, i: torch.linspace(-1, 1, n).reshape(n, i)),
    "clustered": (1000, 17, 65, lambda n, i: torch.tanh(3 * torch.randn(n, i))),
    "ties": (600, 4, 2, lambda n, i: torch.round(torch.randn(n, i) * 8) / 8),
    "outside": (300, 3, 4, lambda n, i: 3 * torch.randn(n, i) + 1),
    "few": (9, 2, 2, lambda n, i: torch.randn(n, i)),
    "rank": (7, 2, 2, lambda n, i: torch.randn(n, i)),
}
STACK_WIDTHS, STACK_ROWS, PRIOR_ROWS = [1, 8, 8, 1], 3001, 512
REG_ARGS = (0.7, 1.3)


def np32(t):
    return t.detach().numpy().astype(F32).copy()


def layer_state(lay):
    return np32(lay.grid), np32(lay.base_weight), np32(lay.spline_weight), np32(lay.spline_scaler)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import kan as ref_kan  # noqa: E402  (the reference's own module)

    out, report = {}, []
    for k, (name, (rows, fin, fout, gen)) in enumerate(CASES.items()):
        torch.manual_seed(100 + k)
        lay = ref_kan.KANLinear(fin, fout)
        lay.update_grid(torch.rand(PRIOR_ROWS, fin) * 2 - 1)  # the non-uniform starting grid
        x = gen(rows, fin).float()
        grid, bw, sw, sc = layer_state(lay)
        assert (np.diff(grid, axis=1) > 0).all()
        out.update({f"{name}_x": np32(x), f"{name}_grid": grid, f"{name}_base_weight": bw,
                    f"{name}_spline_weight": sw, f"{name}_spline_scaler": sc})
        grid_new = gr.knots32(np32(x), lay.grid_eps, 0.01)
        g64 = gr.gram(np32(x), grid, grid_new)
        worst = min(gr.pivot_ratios(g64[i, 0]).min() for i in range(fin))
        lay.update_grid(x)  # the rank case too: the CPU's gelsy returns a minimum-norm answer there
        new_grid, new_sw = np32(lay.grid), np32(lay.spline_weight)
        assert (np.diff(new_grid, axis=1) > 0).all(), name
        assert np.array_equal(new_grid, grid_new), f"{name}: knots32 is not the reference's knot arithmetic"
        if name == "rank":
            assert gr.rank_deficient(g64), "the 7-row case must fail the Cholesky factorisation"
            out[f"{name}_new_grid"] = new_grid
            report.append(f"{name}: refused, worst pivot ratio 2^{np.log2(max(worst, 1e-300)):.1f}")
            continue
        assert worst > 2.0 ** -30, (name, worst)
        _, c64 = gr.update_grid(np32(x), grid, sw, sc, grid_new=new_grid)
        err = gr.coeff_error(new_sw, c64)
        out.update({f"{name}_new_grid": new_grid, f"{name}_new_spline_weight": new_sw,
                    f"{name}_ref_err": np.float64(err)})
        report.append(f"{name}: reference error {err:.2e}, worst pivot ratio 2^{np.log2(worst):.1f}, "
                      f"cond(G) {max(np.linalg.cond(g64[i, 0]) for i in range(fin)):.1e}")

    # the stack: KAN([1, 8, 8, 1]) on 3001 coordinates
    torch.manual_seed(7)
    model = ref_kan.KAN(STACK_WIDTHS)
    with torch.no_grad():
        model(torch.rand(PRIOR_ROWS, 1) * 2 - 1, update_grid=True)
    x = torch.linspace(-1, 1, STACK_ROWS).reshape(-1, 1)
    old = [layer_state(lay) for lay in model.layers]
    with torch.no_grad():
        y = model(x, update_grid=True)
        y_again = model(x)
    assert torch.equal(y, y_again)
    y64, new64 = gr.stack_update(np32(x), old)
    out["stack_x"], out["stack_out"] = np32(x), np32(y)
    out["stack_out_ref_err"] = np.float64(np.abs(np32(y) - y64).max() / np.abs(y64).max())
    for l, lay in enumerate(model.layers):
        for nm, a in zip(("grid", "base_weight", "spline_weight", "spline_scaler"), old[l]):
            out[f"stack_l{l}_{nm}"] = a
        out[f"stack_l{l}_new_grid"], out[f"stack_l{l}_new_spline_weight"] = np32(lay.grid), np32(lay.spline_weight)
        assert (np.diff(np32(lay.grid), axis=1) > 0).all()
        out[f"stack_l{l}_ref_err"] = np.float64(gr.coeff_error(np32(lay.spline_weight), new64[l][2]))
    assert np.array_equal(out["stack_l0_new_grid"], gr.knots32(np32(x)))
    # regularization_loss (kan.py:217-237, :281-285) of the updated stack and its gradients
    model.zero_grad()
    reg = model.regularization_loss(*REG_ARGS)
    reg.backward()
    out["stack_reg_args"], out["stack_reg"] = np.array(REG_ARGS), np.float64(reg.item())
    for l, lay in enumerate(model.layers):
        out[f"stack_l{l}_reg_grad"] = np32(lay.spline_weight.grad)
    report.append(f"stack: output reference error {float(out['stack_out_ref_err']):.2e}, per-layer coefficient errors "
                  + ", ".join(f"{float(out[f'stack_l{l}_ref_err']):.2e}" for l in range(len(model.layers))))

    path = os.path.join(OUT, "kan_grid_update.npz")
    np.savez_compressed(path, **out)
    print("\n".join(report))
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
