"""fp64 references and bounds of the NT GEMM kernel tests (a plain module like gpu_util.py: no
fixtures, nothing collected).

One definition of what "within one fp16 rounding of the fp64 answer computed from the same fp16
inputs" means for every epilogue mode of the hidden-layer GEMM, shared by the per-kernel tests
(test_gpu_kernels.py, test_gpu_act.py) and the multi-tile walk tests (test_gpu_walk.py): the
input generators whose ranges the bounds were set on, the fp64 reference of each mode, and the
assertions themselves.  `got` arguments are host arrays (any float type); inputs are the fp16-
rounded fp32 arrays that went to the device.  A `tag` logs the measured column-sum errors
through errlog.log.

same_bits / first_difference: the bit-identity comparison of the walk-depth tests, on lists of
buffers that were pre-filled with NaN (an element a launch failed to write stays NaN on one side
only, or on both -- see first_difference)."""
import math

import numpy as np

from errlog import log
from gpu_util import within_f16
from oracle import siren_oracle as orc

F32 = np.float32
F64 = np.float64
SINE, SNAKE, TANH = 0, 1, 2


# ------------------------------------------------------------------ input generators
def inner_inputs(rng, R, H):
    """A sine layer's X (fp16 values), fp32 W in the SIREN init range and b."""
    X = orc.f16_round(rng.uniform(-1, 1, (R, H)).astype(F32))
    lim = math.sqrt(6 / H) / 30
    W = rng.uniform(-lim, lim, (H, H)).astype(F32)
    b = rng.uniform(-1 / math.sqrt(H), 1 / math.sqrt(H), H).astype(F32)
    return X, W, b


def act_inputs(rng, R, H):
    """A Snake / Tanh layer's X, W (both fp16 values) and b."""
    X = orc.f16_round(rng.uniform(-1, 1, (R, H)).astype(F32))
    lim = 1 / math.sqrt(H)     # nn.Linear default init range of the Snake / Tanh Linears
    W = orc.f16_round(rng.uniform(-lim, lim, (H, H)).astype(F32))
    b = rng.uniform(-lim, lim, H).astype(F32)
    return X, W, b


def snake_ref(z, a):
    """Snake y, dy/dz, dy/da at pre-activation z (models.py:241 and its autograd)."""
    s, c = np.sin(a * z), np.cos(a * z)
    return z + s * s / a, 1.0 + 2.0 * s * c, (z * 2.0 * s * c) / a - s * s / (a * a)


def _f64(x):
    return np.asarray(x, F64)


# ------------------------------------------------------------------ forward modes
def _check_head(hp, y, hw):
    """Head partials [parts][R] summed over the parts against y @ w_head (a sum over the H
    columns of one row: independent of the row count)."""
    ref = y @ _f64(hw)
    got = _f64(hp).sum(0)
    assert np.max(np.abs(got - ref)) < 1e-4 * max(1.0, np.max(np.abs(ref)))


def check_inner_fwd(Y, C, hp, X, Wh, b, hw):
    """siren_inner_fwd: Y = sin a, C = cos a, a = 30 (X Wh^T + b); hp None: no head partials."""
    a = 30.0 * (_f64(X) @ _f64(Wh).T + b)
    assert within_f16(Y, np.sin(a), 2e-5) <= 0
    assert within_f16(C, np.cos(a), 2e-5) <= 0
    if hp is not None:
        _check_head(hp, np.sin(a), hw)


def check_inner_fwd_act(act, Y, C, E, hp, X, W, b, a, hw, amag):
    """siren_inner_fwd_act, SNAKE (Y, C = dY/dz, E = dY/da) or TANH (Y, C = 1 - Y^2; E ignored);
    amag: the magnitude the Snake a was drawn around; hp None: no head partials."""
    z = _f64(X) @ _f64(W).T + b
    # fp32 accumulation of z: |dz| ~ 1e-6; through sin(a z) that is a*|dz|
    slack = 2e-6 * max(1.0, float(amag)) * 4
    if act == SNAKE:
        y, d, e = snake_ref(z, _f64(a))
        assert within_f16(Y, y, slack) <= 0
        assert within_f16(C, d, 2 * slack) <= 0
        assert within_f16(E, e, 2 * slack * (np.max(np.abs(z)) + 1) / float(np.min(a))) <= 0
    else:
        y = np.tanh(z)
        assert within_f16(Y, y, 1e-6) <= 0
        assert within_f16(C, 1.0 - y * y, 2e-6) <= 0
    if hp is not None:
        _check_head(hp, y, hw)


# ------------------------------------------------------------------ backward modes
def _colsum(tag, name, got, terms, tol):
    """Column sums over the rows: |got - sum(terms)| < tol, the measured worst logged beside the
    tolerance and beside the cancellation-aware scale sum |terms| (test_head_bwd's)."""
    ref = terms.sum(0)
    err = float(np.max(np.abs(got - ref)))
    if tag:
        log(tag, what=name, err=err, tol=float(tol),
            rel_abs_terms=float(np.max(np.abs(got - ref) / np.maximum(np.abs(terms).sum(0), 1e-300))))
    assert err < tol, (name, err, tol)


def check_inner_bwd_dx(out, dbp, dZ, Wh, Cp, k, tag=None):
    """siren_inner_bwd_dx: dZprev = 30 Cp (dZ Wh) (carries dZ's scale), db partials x 1/S with
    S = 2^k (k None: unscaled); dbp: the written partial rows [R/tile][H]."""
    ref = (_f64(dZ) @ _f64(Wh)) * Cp * 30.0
    scale = np.max(np.abs(ref))
    assert within_f16(out, ref, 1e-5 * scale) <= 0
    db = _f64(dbp).sum(0) * 2.0 ** (k or 0)
    _colsum(tag, "db", db, ref, 1e-4 * np.max(np.abs(ref.sum(0))) + 1e-6 * scale)


def check_inner_bwd_dx_act(act, out, part, dZ, W, D, Ep, k, tag=None):
    """siren_inner_bwd_dx_act into a SNAKE (part [R/tile][2][H]: db, da) or TANH (part
    [R/tile][H]: db) layer: dZprev = D (dZ W); part holds the written partial rows only."""
    R = dZ.shape[0]
    dY = _f64(dZ) @ _f64(W)
    ref = dY * D
    scale = np.max(np.abs(ref))
    assert within_f16(out, ref, 1e-5 * scale) <= 0
    p = _f64(part)
    db, da = (p[:, 0].sum(0), p[:, 1].sum(0)) if act == SNAKE else (p.sum(0), None)
    sc = 2.0 ** (k or 0)
    _colsum(tag, "db", db * sc, ref, 1e-4 * np.max(np.abs(ref.sum(0))) + 1e-6 * scale * math.sqrt(R))
    if da is not None:
        terms = dY * Ep
        _colsum(tag, "da", da * sc, terms,
                1e-4 * np.max(np.abs(terms.sum(0))) + 1e-6 * np.max(np.abs(dY)) * math.sqrt(R))


def check_first_bwd_dx(part, dZ1, Wh, C0, t, omega0, k, tag=None):
    """siren_first_bwd_dx: column partials [R/tile][1 + in][H] of dZ0 = omega0 C0 (dZ1 Wh) and of
    dZ0 t_j, x 1/S (dZ0 itself is never stored)."""
    R, in_dim = t.shape
    dz0 = (_f64(dZ1) @ _f64(Wh)) * C0 * omega0
    got = _f64(part).sum(0) * 2.0 ** (k or 0)
    scale = np.max(np.abs(dz0)) * math.sqrt(R)
    _colsum(tag, "db0", got[0], dz0, 1e-4 * scale)
    for j in range(in_dim):
        _colsum(tag, f"dW0[{j}]", got[1 + j], dz0 * t[:, j:j + 1], 1e-4 * scale)


# ------------------------------------------------------------------ bit identity
def first_difference(a, b):
    """Where two lists of equally shaped buffers differ bit for bit, NaN counting as a value of its
    own (torch.nan_to_num to 7, as test_gpu_queue._same): None when they agree, else (buffer index,
    flat element index, got, expected).  Buffers the launches were to fill completely are checked
    with `written` below; this one only says the two runs left the same bits everywhere -- inside
    the tiles and outside them."""
    import torch
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, (i, x.shape, y.shape)
        xs, ys = torch.nan_to_num(x.float(), 7.0), torch.nan_to_num(y.float(), 7.0)
        if not torch.equal(xs, ys):
            j = int(torch.nonzero((xs != ys).reshape(-1))[0])
            return i, j, float(x.reshape(-1)[j]), float(y.reshape(-1)[j])
    return None


def same_bits(a, b):
    return first_difference(a, b) is None


def unwritten(bufs):
    """Indices of the buffers that still hold a NaN of their pre-fill (a launch must overwrite
    every element of the buffers it owns; none of these kernels' results is NaN on finite input)."""
    import torch
    return [i for i, x in enumerate(bufs) if bool(torch.isnan(x).any())]
