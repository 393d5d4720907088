"""tests/kan_ref.py for any grid size: the fp64 restatement of one ``KANLinear`` whose sizes come
from its arrays (grid [in][G + 7], spline_weight [out][in][G + 3]), and a knot family per grid size.

``bases64``, ``outside``, ``probe_inputs``, ``kan_div_emulated`` and ``recursion_quotients`` of
kan_ref take their shapes from the knot rows they are given and are re-exported unchanged."""
import numpy as np

from kan_ref import (DERIV_C, F32, F64, ORACLE_ERR_B, ORACLE_ERR_DB, _silu, bases64, kan_div_emulated,  # noqa: F401
                     outside, probe_inputs, recursion_quotients)

GRIDS = (1, 2, 4, 6, 11, 16, 64)   # the grid sizes the host and GPU tests run


def dims(G):
    """(NB bases, NG knots, K1 A-columns per input, IC inputs per chunk) of the any-grid-size kernels."""
    return G + 3, G + 7, G + 4, min(16, 144 // (G + 4))


def layer(x, grid, base_weight, spline_weight, spline_scaler, G=None, G_terms=None):
    """kan_ref.layer with NB = spline_weight.shape[-1]: forward and autograd of one KANLinear in
    fp64 as a dict of (value, terms) pairs -- ``out``; with an upstream G also ``dW`` (combined
    weight [out][(NB + 1) in]), ``base_weight``, ``spline_weight``, ``spline_scaler`` and ``dX``."""
    x64 = np.asarray(x, F32).astype(F64)
    n, fin = x64.shape
    bw = np.asarray(base_weight, F32).astype(F64)
    sw = np.asarray(spline_weight, F32).astype(F64)
    sc = np.asarray(spline_scaler, F32).astype(F64)
    fout, nb = bw.shape[0], sw.shape[-1]
    assert np.asarray(grid).shape == (fin, nb + 4) and sw.shape == (fout, fin, nb)
    b, db, sb, sdb = bases64(x, grid)
    sl, dsl, sdsl = _silu(x64)
    A = np.concatenate([sl, b.reshape(n, -1)], 1)
    aA = np.concatenate([np.abs(sl), sb.reshape(n, -1)], 1)
    W = np.concatenate([bw, (sw * sc[..., None]).reshape(fout, -1)], 1)
    res = {"out": (A @ W.T, aA @ np.abs(W).T)}
    if G is None:
        return res
    G = np.asarray(G).astype(F64).reshape(n, fout)
    aG = np.abs(G) if G_terms is None else np.asarray(G_terms, F64).reshape(n, fout)
    dW, tW = G.T @ A, aG.T @ aA
    res["dW"] = (dW, tW)
    dS, tS = dW[:, fin:].reshape(fout, fin, nb), tW[:, fin:].reshape(fout, fin, nb)
    res["base_weight"] = (dW[:, :fin], tW[:, :fin])
    res["spline_weight"] = (dS * sc[..., None], tS * np.abs(sc)[..., None])
    res["spline_scaler"] = ((dS * sw).sum(-1), (tS * np.abs(sw)).sum(-1))
    dA, tA = G @ W, aG @ np.abs(W)
    dAs, tAs = dA[:, fin:].reshape(n, fin, nb), tA[:, fin:].reshape(n, fin, nb)
    res["dX"] = (dsl * dA[:, :fin] + (db * dAs).sum(-1), sdsl * tA[:, :fin] + (sdb * tAs).sum(-1))
    return res


def kan_knots_g(fin, G, seed):
    """[fin][G + 7] fp32 knot rows by kan_ref.kan_knots' law at grid size G: the constructor's row
    arange(-3, G + 4) * (2 / G) - 1, stretched by 0.6 .. 1.6 and shifted by -0.5 .. 0.5 per input,
    every knot jittered by up to +-30 % of its input's step.  The smallest gap is
    0.6 * (1 - 0.6) = 0.24 steps before rounding; at least 0.1 steps is asserted."""
    rng = np.random.default_rng(seed)
    step = 2.0 / G
    base = np.arange(-3, G + 4, dtype=F64) * step - 1.0
    stretch = rng.uniform(0.6, 1.6, (fin, 1))
    shift = rng.uniform(-0.5, 0.5, (fin, 1))
    jitter = rng.uniform(-0.3, 0.3, (fin, G + 7)) * step
    g = ((base[None] + jitter) * stretch + shift).astype(F32)
    assert np.all(np.diff(g.astype(F64), axis=1) >= 0.1 * step), "kan_knots_g: a knot gap under 0.1 steps"
    return g


def workspace_floats(widths, rows, splits, G):
    """capi.hip kan_layout restated with K1 = G + 4: (float offsets of X[l], offset of G[0], total)."""
    k1 = G + 4
    al = lambda v: (v + 63) // 64 * 64  # noqa: E731
    L = len(widths) - 1
    off, wk = 0, 1
    for l in range(L):
        kw = widths[l + 1] * k1 * widths[l]
        off += 2 * al(kw)
        wk = max(wk, kw)
    X = {}
    for l in range(1, L + 1):
        X[l] = off
        off += al(rows * widths[l])
    off += al(wk)
    slab = wk * splits
    for l in range(L):
        if widths[l + 1] == 1:
            slab = max(slab, 4 * splits * k1 * widths[l])
    off += al(slab)
    G0 = off
    off += 2 * al(rows * max(widths[:L])) + 3 * al((rows + 255) // 256) + al(1)
    return X, G0, off
