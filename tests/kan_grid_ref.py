"""fp64 numpy restatement of efficient-KAN's ``KANLinear.update_grid`` (kan.py:168-215) and of the
layer forward (kan.py:153-166), for judging the HIP grid update (csrc/kan_general.hip kan_regrid_* at 5 -> 5).

Everything is fp64: the bases (the Cox-de Boor recursion of kan.py:94-104), the curves, the knots and
the least-squares fit (``numpy.linalg.lstsq``, an SVD).  ``knots32`` is the one fp32 routine: the
knot formula op for op as torch evaluates it on the CPU, which the kernel must match bit for bit.
``gram`` / ``refit_from_gram`` restate the route the kernels take (normal equations through the
8 x 8 Gram matrices), so that the identity they rest on is itself under test.
"""
import numpy as np

F32, F64 = np.float32, np.float64
NB, NG, ORDER, GRID_SIZE = 8, 12, 3, 5
PIVOT_RATIO = 2.0 ** -40  # the kernels' rank rule: a Cholesky pivot at or below this x max diagonal


def bases(x, grid):
    """x [N][in], knots [in][12] -> [N][in][8], all fp64 (order-0 predicate g[j] <= x < g[j+1])."""
    x = np.asarray(x, F64)[:, :, None]
    g = np.asarray(grid, F64)[None]
    b = ((x >= g[..., :-1]) & (x < g[..., 1:])).astype(F64)
    for k in range(1, ORDER + 1):
        left = (x - g[..., :-(k + 1)]) / (g[..., k:-1] - g[..., :-(k + 1)])
        right = (g[..., k + 1:] - x) / (g[..., k + 1:] - g[..., 1:(-k)])
        b = left * b[..., :-1] + right * b[..., 1:]
    return b


def order_index(rows):
    """The six row indices of kan.py:185-187: torch.linspace(0, rows - 1, 6, dtype=int64)."""
    import torch
    return torch.linspace(0, rows - 1, GRID_SIZE + 1, dtype=torch.int64).numpy()


def knots64(x, grid_eps=0.02, margin=0.01):
    """kan.py:183-212 in fp64: new knots [in][12] of inputs x [N][in]."""
    xs = np.sort(np.asarray(x, F64), axis=0)
    adaptive = xs[order_index(xs.shape[0])]
    step = (xs[-1] - xs[0] + 2 * margin) / GRID_SIZE
    uniform = np.arange(GRID_SIZE + 1, dtype=F64)[:, None] * step + xs[0] - margin
    g = grid_eps * uniform + (1 - grid_eps) * adaptive
    lo = g[:1] - step * np.arange(ORDER, 0, -1, dtype=F64)[:, None]
    hi = g[-1:] + step * np.arange(1, ORDER + 1, dtype=F64)[:, None]
    return np.concatenate([lo, g, hi], 0).T.copy()


def knots32(x, grid_eps=0.02, margin=0.01):
    """The same formula in fp32, each operation rounded once in the reference's order (host scalars
    are rounded to fp32 where torch rounds them: 2 * margin and 1 - grid_eps are formed in double)."""
    xs = np.sort(np.asarray(x, F32), axis=0)
    q = xs[order_index(xs.shape[0])]
    m, m2, eps, one_eps = F32(margin), F32(2 * margin), F32(grid_eps), F32(1 - grid_eps)
    step = ((q[5] - q[0]) + m2) / F32(GRID_SIZE)
    uniform = (np.arange(GRID_SIZE + 1, dtype=F32)[:, None] * step + q[0]) - m
    g = eps * uniform + one_eps * q
    lo = g[:1] - step * np.arange(ORDER, 0, -1).astype(F32)[:, None]
    hi = g[-1:] + step * np.arange(1, ORDER + 1).astype(F32)[:, None]
    out = np.concatenate([lo, g, hi], 0).T.copy()
    assert out.dtype == F32
    return out


def update_grid(x, grid_old, spline_weight, spline_scaler, grid_eps=0.02, margin=0.01, grid_new=None):
    """kan.py:168-215 in fp64.  Returns (grid_new [in][12], spline_weight_new [out][in][8]).  With
    grid_new given (the reference's fp32 knots) only the refit is restated, on exactly those knots.
    The refit targets the scaled curves and is returned undivided, like the reference."""
    x = np.asarray(x, F64)
    if grid_new is None:
        grid_new = knots64(x, grid_eps, margin)
    coeff = np.asarray(spline_weight, F64) * np.asarray(spline_scaler, F64)[..., None]  # [out][in][8]
    a_old, a_new = bases(x, grid_old), bases(x, grid_new)
    new = np.empty_like(coeff)
    for i in range(x.shape[1]):
        curves = a_old[:, i, :] @ coeff[:, i, :].T  # [N][out]
        new[:, i, :] = np.linalg.lstsq(a_new[:, i, :], curves, rcond=None)[0].T
    return np.asarray(grid_new, F64), new


def gram(x, grid_old, grid_new):
    """[in][2][8][8]: G_nn = sum_r b_new b_new^T and G_no = sum_r b_new b_old^T, in fp64."""
    a_old, a_new = bases(x, grid_old), bases(x, grid_new)
    return np.stack([np.einsum("nic,nid->icd", a_new, a_new), np.einsum("nic,nid->icd", a_new, a_old)], 1)


def pivot_ratios(g_nn):
    """Cholesky pivots of one 8 x 8 G_nn over its largest diagonal entry, up to and including the
    first that breaks the rank rule (the factorisation stops there)."""
    g = np.asarray(g_nn, F64)
    dmax = g.diagonal().max()
    L, out = np.zeros((NB, NB)), []
    for j in range(NB):
        p = g[j, j] - (L[j, :j] ** 2).sum()
        out.append(p / dmax if dmax > 0 else 0.0)
        if not p > PIVOT_RATIO * dmax:
            break
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (g[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return np.array(out)


def rank_deficient(g):
    """Indices of the inputs of gram [in][2][8][8] that the rank rule refuses."""
    return [i for i in range(g.shape[0]) if pivot_ratios(g[i, 0]).min() <= PIVOT_RATIO]


def refit_from_gram(g, spline_weight, spline_scaler):
    """spline_weight_new [out][in][8] = G_nn^-1 G_no (spline_weight * spline_scaler) per input."""
    coeff = np.asarray(spline_weight, F64) * np.asarray(spline_scaler, F64)[..., None]
    new = np.empty_like(coeff)
    for i in range(g.shape[0]):
        new[:, i, :] = np.linalg.solve(g[i, 0], g[i, 1] @ coeff[:, i, :].T).T
    return new


def layer_forward(x, grid, base_weight, spline_weight, spline_scaler):
    """kan.py:153-166 in fp64: [N][in] -> [N][out]."""
    x = np.asarray(x, F64)
    w = (np.asarray(spline_weight, F64) * np.asarray(spline_scaler, F64)[..., None]).reshape(len(base_weight), -1)
    return (x / (1.0 + np.exp(-x))) @ np.asarray(base_weight, F64).T + bases(x, grid).reshape(len(x), -1) @ w.T


def stack_update(x, layers, grid_eps=0.02, margin=0.01):
    """kan.py:274-279 with update_grid=True in fp64 over layers [(grid, base_weight, spline_weight,
    spline_scaler), ...]: per layer the update, then its forward.  Returns (output, new layers)."""
    h, new = np.asarray(x, F64), []
    for grid, bw, sw, sc in layers:
        g, c = update_grid(h, grid, sw, sc, grid_eps, margin)
        new.append((g, bw, c, sc))
        h = layer_forward(h, g, bw, c, sc)
    return h, new


def coeff_error(got, want):
    """Largest coefficient error relative to the layer's largest coefficient."""
    want = np.asarray(want, F64)
    return float(np.abs(np.asarray(got, F64) - want).max() / np.abs(want).max())
