"""fp64 numpy restatement of a KANLinear refit from a grid of Go intervals onto one of Gn (the HIP
path's ``KANLinear.regrid``, csrc/kan_general.hip kan_regrid_*), for any pair of sizes: kan_grid_ref.py
with the sizes taken from the arrays (knots [in][G + 7], coefficients [out][in][G + 3]).

Everything is fp64 -- the bases (kan.py:94-104), the curves, the knots and the least-squares fit
(``numpy.linalg.lstsq``) -- except ``knots32``: kan.py:183-212 op for op in fp32 as torch evaluates
it on the CPU, which the kernel must match bit for bit.  ``gram`` / ``refit_from_gram`` restate the
route the kernels take (normal equations through G_nn (Gn+3)^2 and G_no (Gn+3) x (Go+3)), so that the
identity they rest on is itself under test.  ``refit`` takes the coefficients it is given: the
reference's update_grid passes spline_weight * spline_scaler, ``KANLinear.regrid`` the unscaled
spline_weight.
"""
import numpy as np

F32, F64 = np.float32, np.float64
ORDER = 3
PIVOT_RATIO = 2.0 ** -40  # the kernels' rank rule: a Cholesky pivot at or below this x max diagonal
PAIRS = ((5, 5), (5, 10), (1, 2), (4, 11), (11, 4), (16, 64), (64, 64), (64, 1), (6, 6))  # (Go, Gn)


def bases(x, grid):
    """x [N][in], knots [in][G+7] -> [N][in][G+3], all fp64 (order-0 predicate g[j] <= x < g[j+1])."""
    x = np.asarray(x, F64)[:, :, None]
    g = np.asarray(grid, F64)[None]
    b = ((x >= g[..., :-1]) & (x < g[..., 1:])).astype(F64)
    for k in range(1, ORDER + 1):
        with np.errstate(divide="ignore", invalid="ignore"):
            left = (x - g[..., :-(k + 1)]) / (g[..., k:-1] - g[..., :-(k + 1)])
            right = (g[..., k + 1:] - x) / (g[..., k + 1:] - g[..., 1:(-k)])
        b = left * b[..., :-1] + right * b[..., 1:]
    return b


def order_index(rows, G):
    """The G + 1 row indices of kan.py:185-187: torch.linspace(0, rows - 1, G + 1, dtype=int64)."""
    import torch
    return torch.linspace(0, rows - 1, G + 1, dtype=torch.int64).numpy()


def knots64(x, G, grid_eps=0.02, margin=0.01):
    """kan.py:183-212 in fp64 at grid size G: new knots [in][G+7] of inputs x [N][in]."""
    xs = np.sort(np.asarray(x, F64), axis=0)
    adaptive = xs[order_index(xs.shape[0], G)]
    step = (xs[-1] - xs[0] + 2 * margin) / G
    uniform = np.arange(G + 1, dtype=F64)[:, None] * step + xs[0] - margin
    g = grid_eps * uniform + (1 - grid_eps) * adaptive
    lo = g[:1] - step * np.arange(ORDER, 0, -1, dtype=F64)[:, None]
    hi = g[-1:] + step * np.arange(1, ORDER + 1, dtype=F64)[:, None]
    return np.concatenate([lo, g, hi], 0).T.copy()


def knots32(x, G, grid_eps=0.02, margin=0.01):
    """The same formula in fp32, each operation rounded once in the reference's order (host scalars
    are rounded to fp32 where torch rounds them: 2 * margin and 1 - grid_eps are formed in double)."""
    xs = np.sort(np.asarray(x, F32), axis=0)
    q = xs[order_index(xs.shape[0], G)]
    m, m2, eps, one_eps = F32(margin), F32(2 * margin), F32(grid_eps), F32(1 - grid_eps)
    step = ((q[G] - q[0]) + m2) / F32(G)
    uniform = (np.arange(G + 1, dtype=F32)[:, None] * step + q[0]) - m
    g = eps * uniform + one_eps * q
    lo = g[:1] - step * np.arange(ORDER, 0, -1).astype(F32)[:, None]
    hi = g[-1:] + step * np.arange(1, ORDER + 1).astype(F32)[:, None]
    out = np.concatenate([lo, g, hi], 0).T.copy()
    assert out.dtype == F32
    return out


def refit(x, grid_old, grid_new, coeff):
    """The lstsq route: coeff [out][in][Go+3] on grid_old -> [out][in][Gn+3] on grid_new, per input
    the least-squares fit over the rows of x of the curves the old coefficients draw."""
    x, coeff = np.asarray(x, F64), np.asarray(coeff, F64)
    a_old, a_new = bases(x, grid_old), bases(x, grid_new)
    new = np.empty(coeff.shape[:2] + (a_new.shape[-1],), F64)
    for i in range(x.shape[1]):
        curves = a_old[:, i, :] @ coeff[:, i, :].T  # [N][out]
        new[:, i, :] = np.linalg.lstsq(a_new[:, i, :], curves, rcond=None)[0].T
    return new


def gram(x, grid_old, grid_new):
    """(G_nn [in][Gn+3][Gn+3], G_no [in][Gn+3][Go+3]) = sum_r b_new b_new^T, sum_r b_new b_old^T, fp64."""
    a_old, a_new = bases(x, grid_old), bases(x, grid_new)
    return np.einsum("nic,nid->icd", a_new, a_new), np.einsum("nic,nid->icd", a_new, a_old)


def pack(g_nn, g_no):
    """The C-ABI's dense layout: per input G_nn then G_no, one flat fp64 array."""
    fin = g_nn.shape[0]
    return np.concatenate([g_nn.reshape(fin, -1), g_no.reshape(fin, -1)], 1).reshape(-1)


def unpack(flat, fin, Go, Gn):
    a = np.asarray(flat).reshape(fin, (Gn + 3) * (Gn + Go + 6))
    return (a[:, :(Gn + 3) ** 2].reshape(fin, Gn + 3, Gn + 3).copy(),
            a[:, (Gn + 3) ** 2:].reshape(fin, Gn + 3, Go + 3).copy())


def pivot_ratios(g_nn):
    """Cholesky pivots of one G_nn over its largest diagonal entry, up to and including the first
    that breaks the rank rule (the factorisation stops there)."""
    g = np.asarray(g_nn, F64)
    n, dmax = len(g), g.diagonal().max()
    L, out = np.zeros((n, n)), []
    for j in range(n):
        p = g[j, j] - (L[j, :j] ** 2).sum()
        out.append(p / dmax if dmax > 0 else 0.0)
        if not p > PIVOT_RATIO * dmax:
            break
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (g[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return np.array(out)


def rank_deficient(g_nn):
    """Indices of the inputs of G_nn [in][Gn+3][Gn+3] that the rank rule refuses."""
    return [i for i in range(len(g_nn)) if pivot_ratios(g_nn[i]).min() <= PIVOT_RATIO]


def refit_from_gram(g_nn, g_no, coeff):
    """The Gram route: [out][in][Gn+3] = G_nn^-1 G_no coeff per input."""
    coeff = np.asarray(coeff, F64)
    new = np.empty(coeff.shape[:2] + (g_nn.shape[-1],), F64)
    for i in range(len(g_nn)):
        new[:, i, :] = np.linalg.solve(g_nn[i], g_no[i] @ coeff[:, i, :].T).T
    return new


def spans(x, grid):
    """[N][in] span index s with g[s] <= x < g[s+1], -1 where there is none."""
    x, g = np.asarray(x, F32)[:, :, None], np.asarray(grid, F32)[None]
    hit = (x >= g[..., :-1]) & (x < g[..., 1:])
    return np.where(hit.any(-1), hit.argmax(-1), -1)


def overlapping_pairs(go, gn):
    """The (new span s, old span r) pairs of one input whose half-open intervals overlap."""
    return [(s, r) for s in range(len(gn) - 1) for r in range(len(go) - 1)
            if max(gn[s], go[r]) < min(gn[s + 1], go[r + 1])]


def layer_forward(x, grid, base_weight, spline_weight, spline_scaler):
    """kan.py:153-166 in fp64: [N][in] -> [N][out]."""
    x = np.asarray(x, F64)
    w = (np.asarray(spline_weight, F64) * np.asarray(spline_scaler, F64)[..., None]).reshape(len(base_weight), -1)
    return (x / (1.0 + np.exp(-x))) @ np.asarray(base_weight, F64).T + bases(x, grid).reshape(len(x), -1) @ w.T


def stack_regrid(x, layers, Gn, grid_eps=0.02, margin=0.01):
    """KAN.regrid in fp64 over layers [(grid, base_weight, spline_weight, spline_scaler), ...]: per
    layer new knots from its input, the unscaled coefficients refitted, then its forward.  Returns
    (output, new layers)."""
    h, new = np.asarray(x, F64), []
    for grid, bw, sw, sc in layers:
        g = knots64(h, Gn, grid_eps, margin)
        c = refit(h, grid, g, sw)
        new.append((g, bw, c, sc))
        h = layer_forward(h, g, bw, c, sc)
    return h, new


def stack_forward(x, layers):
    h = np.asarray(x, F64)
    for grid, bw, sw, sc in layers:
        h = layer_forward(h, grid, bw, sw, sc)
    return h


def coeff_error(got, want):
    """Largest coefficient error relative to the layer's largest coefficient."""
    want = np.asarray(want, F64)
    return float(np.abs(np.asarray(got, F64) - want).max() / np.abs(want).max())
