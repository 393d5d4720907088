"""fp64 restatement of one efficient-KAN ``KANLinear`` (kan.py:94-104, 145-166) and its autograd,
in plain numpy, for judging the HIP kernels of csrc/kan.hip element by element.

Inputs are the fp32 arrays the kernels read (x [N][in], grid [in][12], base_weight [out][in],
spline_weight [out][in][8], spline_scaler [out][in], upstream G [N][out]); everything is widened
to fp64 first, so the only rounding in a reference value is fp64's.  Every result comes with
``terms``: per element, the sum of the absolute values of the products that make it up, the scale
an fp32 summation error is measured against (tests/test_gpu_kernels.py's 1e-5 * sum|terms|).
"""
import numpy as np

F32, F64 = np.float32, np.float64
NB, NG, ORDER = 8, 12, 3
# Largest error of the fp32 recursion with IEEE divisions (oracle.siren_oracle.kan_bases) against
# bases64, in units of 2^-24 * scale, measured by tests/test_kan_host.py on 18 kan_knots inputs and
# 40 000 draws plus knots each: 7.94 for B, 6.66 for B'; rounded up.
ORACLE_ERR_B, ORACLE_ERR_DB = 8.0, 7.0
# Gate of a kernel's B' as a value: 4 x the oracle's error.  The backward kernels trade each 0.5-ulp
# IEEE division for a 1-ulp v_rcp_f32 and a rounded product, three levels deep.
DERIV_C = 4.0 * ORACLE_ERR_DB


def bases64(x, grid, deriv=True):
    """Cox-de Boor recursion of kan.py:94-104 in fp64 on fp32 inputs x [N][in] and knots [in][12].

    Order-0 bases are the predicate g[j] <= x < g[j+1] (so the span at a knot is the kernels').
    Returns (B, sB) or, with deriv, (B, dB, sB, sdB), each [N][in][8]: the bases, their
    x-derivatives (the recursion differentiated), and their scales -- the same recursions with
    every term replaced by its absolute value.  sB == B inside the support (all terms there are
    non-negative); sdB measures rounding error where B' cancels to near zero."""
    x = np.asarray(x, F32).astype(F64)[:, :, None]
    g = np.asarray(grid, F32).astype(F64)[None]
    b = ((x >= g[..., :-1]) & (x < g[..., 1:])).astype(F64)
    sb, db, sdb = b.copy(), np.zeros_like(b), np.zeros_like(b)
    for k in range(1, ORDER + 1):
        dl = g[..., k:-1] - g[..., :-(k + 1)]
        dr = g[..., k + 1:] - g[..., 1:(-k)]
        left = (x - g[..., :-(k + 1)]) / dl
        right = (g[..., k + 1:] - x) / dr
        if deriv:
            db = b[..., :-1] / dl + left * db[..., :-1] - b[..., 1:] / dr + right * db[..., 1:]
            sdb = (sb[..., :-1] / np.abs(dl) + np.abs(left) * sdb[..., :-1]
                   + sb[..., 1:] / np.abs(dr) + np.abs(right) * sdb[..., 1:])
        b = left * b[..., :-1] + right * b[..., 1:]
        sb = np.abs(left) * sb[..., :-1] + np.abs(right) * sb[..., 1:]
    return (b, db, sb, sdb) if deriv else (b, sb)


def outside(x, grid):
    """[N][in] bool: x lies in no knot span of its input (below the first knot or at / past the last)."""
    x, g = np.asarray(x, F32), np.asarray(grid, F32)
    return (x < g[None, :, 0]) | (x >= g[None, :, -1])


def _silu(x):
    """SiLU(x), SiLU'(x) = s + s x (1 - s) with s = sigmoid(x), and the scale of SiLU': the same sum
    with both terms made absolute.  SiLU' crosses zero at x = -1.278, where the two terms cancel
    and a rounding error of either (a few 2^-24 of the term, whatever the evaluation order) is
    large against the value itself -- as with a basis derivative and its scale."""
    s = 1.0 / (1.0 + np.exp(-x))
    return x * s, s * (1.0 + x * (1.0 - s)), s * (1.0 + np.abs(x) * (1.0 - s))


def layer(x, grid, base_weight, spline_weight, spline_scaler, G=None, G_terms=None):
    """Forward and autograd of one KANLinear in fp64.  Returns a dict of (value, terms) pairs:
    ``out`` [N][out]; with an upstream G [N][out] also ``dW`` (combined weight [out][9 in]),
    ``base_weight``, ``spline_weight``, ``spline_scaler`` (their gradients) and ``dX`` [N][in].
    In the terms of dX the derivative factors B'_c and SiLU' enter by their scales (bases64, _silu).
    G_terms (default |G|) is the magnitude G enters the terms with."""
    x64 = np.asarray(x, F32).astype(F64)
    n, fin = x64.shape
    bw = np.asarray(base_weight, F32).astype(F64)
    sw = np.asarray(spline_weight, F32).astype(F64)
    sc = np.asarray(spline_scaler, F32).astype(F64)
    fout = bw.shape[0]
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
    dS, tS = dW[:, fin:].reshape(fout, fin, NB), tW[:, fin:].reshape(fout, fin, NB)
    res["base_weight"] = (dW[:, :fin], tW[:, :fin])
    res["spline_weight"] = (dS * sc[..., None], tS * np.abs(sc)[..., None])
    res["spline_scaler"] = ((dS * sw).sum(-1), (tS * np.abs(sw)).sum(-1))
    dA, tA = G @ W, aG @ np.abs(W)
    dAs, tAs = dA[:, fin:].reshape(n, fin, NB), tA[:, fin:].reshape(n, fin, NB)
    res["dX"] = (dsl * dA[:, :fin] + (db * dAs).sum(-1), sdsl * tA[:, :fin] + (sdb * tAs).sum(-1))
    return res


def kan_knots(fin, seed):
    """[fin][12] fp32 knot rows, strictly increasing, different for every input and non-uniform:
    the constructor's row (arange(-3, 9) * 0.4 - 1), stretched by 0.6 .. 1.6 and shifted by
    -0.5 .. 0.5 per input, every knot jittered by up to +-30 % of its input's step.  The smallest
    gap is 0.4 * 0.6 * (1 - 0.6) = 0.096 before rounding; at least 0.05 is asserted, so no
    denominator of the recursion vanishes or comes near fp32's underflow."""
    rng = np.random.default_rng(seed)
    base = np.arange(-3, 9, dtype=F64) * 0.4 - 1.0
    stretch = rng.uniform(0.6, 1.6, (fin, 1))
    shift = rng.uniform(-0.5, 0.5, (fin, 1))
    jitter = rng.uniform(-0.3, 0.3, (fin, NG)) * 0.4
    g = ((base[None] + jitter) * stretch + shift).astype(F32)
    assert np.all(np.diff(g.astype(F64), axis=1) >= 0.05), "kan_knots: a knot gap under 0.05"
    return g


def probe_inputs(grid, n, seed=0):
    """[n + 40][in] fp32 inputs for knots [in][12]: n uniform draws per input from half a unit
    below the lowest knot of any input to half a unit above the highest (a large share falls
    outside an input's own knot range), every knot of that input, the floats one ulp either side
    of each, and +-0, +-1e-30.  Column i is rolled by 7 i rows so a row mixes the kinds."""
    g = np.asarray(grid, F32)
    rng = np.random.default_rng(seed)
    lo, hi = float(g.min()) - 0.5, float(g.max()) + 0.5
    cols = []
    for i in range(g.shape[0]):
        col = np.concatenate([rng.uniform(lo, hi, n).astype(F32), g[i], np.nextafter(g[i], F32(np.inf)),
                              np.nextafter(g[i], F32(-np.inf)), np.array([0.0, -0.0, 1e-30, -1e-30], F32)])
        cols.append(np.roll(col.astype(F32), 7 * i))
    return np.stack(cols, 1)


def _rn32(v):
    return np.asarray(v, F64).astype(F32).astype(F64)


def kan_div_emulated(a, d):
    """csrc/kan_tiles.h kan_div on fp32 arrays a, d, emulated in fp64: y = RN(1/d), q = RN(a y),
    r = fma(-q, d, a), q' = fma(r, y, q).  Products of two fp32 numbers and r are exact in fp64;
    the last sum is not always, so its fp64 rounding error (two-sum) nudges the sum one fp64 ulp
    towards the true value before the rounding to fp32 -- the result is the single rounding an
    fp32 fma makes."""
    a32, d32 = np.asarray(a, F32), np.asarray(d, F32)
    a, d = a32.astype(F64), d32.astype(F64)
    y = (F32(1.0) / d32).astype(F64)
    q = _rn32(a * y)
    r = _rn32(a - d * q)
    t = r * y
    s = q + t
    err = t - (s - q)  # exact: |q| >= |t| wherever t != 0
    s = np.where(err > 0, np.nextafter(s, np.inf), np.where(err < 0, np.nextafter(s, -np.inf), s))
    return s.astype(F32)


def recursion_quotients(x, grid):
    """Every (numerator, denominator) fp32 pair the full recursion forms for x [N][in] on knots
    [in][12] (all j, k = 1..3, left and right), as two flat fp32 arrays."""
    x = np.asarray(x, F32)[:, :, None]
    g = np.asarray(grid, F32)[None]
    num, den = [], []
    for k in range(1, ORDER + 1):
        dl = g[..., k:-1] - g[..., :-(k + 1)]
        dr = g[..., k + 1:] - g[..., 1:(-k)]
        a_l = x - g[..., :-(k + 1)]
        a_r = g[..., k + 1:] - x
        for a, dd in ((a_l, dl), (a_r, dr)):
            num.append(a.ravel())
            den.append(np.broadcast_to(dd, a.shape).ravel())
    return np.concatenate(num).astype(F32), np.concatenate(den).astype(F32)
