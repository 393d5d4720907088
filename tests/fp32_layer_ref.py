"""fp64 restatement of the unfused fp32 layers of csrc/layer_fp32.hip (include/siren_hip.h, "unfused
fp32 layers") and their autograd, in plain numpy, for judging the kernels element by element (a plain
module like kan_ref.py: no fixtures, nothing collected).

Inputs are the fp32 arrays the kernels read; everything is widened to fp64 first, so the only
rounding in a reference value is fp64's.  Every result comes as a pair (value, scale):
  * for the linear layer, `scale` is per element the sum of the absolute values of the terms that
    form it -- what a first-order fp32 summation bound  chain * 2^-24 * sum|terms|  multiplies;
  * for an activation, `scale` is the natural size of the result: the sum of the absolute values of
    the terms of its formula plus, for Snake, what one rounding of the sine's argument fl(a v)
    moves the result by (|a v| times the derivative with respect to the argument).  An evaluation
    error is expressed in units of 2^-24 * scale.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                                   # fp32 unit roundoff
IDENTITY, SIN, TANH, SNAKE = 0, 1, 2, 3          # enum siren_fp32_act


def _w(a):
    return np.asarray(a, F32).astype(F64)


# ---- linear: pre = omega (x W^T + b) ------------------------------------------------------------
def linear(x, W, b, omega):
    """x [rows][in], W [out][in], b [out] or None -> (pre [rows][out], sum|terms|)."""
    x, W, om = _w(x), _w(W), float(F32(omega))
    z, t = x @ W.T, np.abs(x) @ np.abs(W).T
    if b is not None:
        z, t = z + _w(b)[None], t + np.abs(_w(b))[None]
    return om * z, abs(om) * t


def linear_bwd(x, W, omega, gpre):
    """Autograd of linear() for dL/dpre = gpre [rows][out]: gz = omega gpre, gW = gz^T x [out][in],
    gb = column sums of gz [out], gx = gz W [rows][in]; each but gz as (value, sum|terms|)."""
    x, W, gz = _w(x), _w(W), float(F32(omega)) * _w(gpre)
    az = np.abs(gz)
    return {"gz": gz,
            "gW": (gz.T @ x, az.T @ np.abs(x)),
            "gb": (gz.sum(0), az.sum(0)),
            "gx": (gz @ W, az @ np.abs(W))}


def split_k(rows, splits):
    """kan_gemm's split-K structure over K = rows: (kchunk, z) -- the rows per slab, a multiple of the
    16-row K-tile, and the slabs actually written (z <= splits; the slab buffer is sized for splits)."""
    kchunk = -(-rows // splits)
    kchunk = -(-kchunk // 16) * 16
    return kchunk, -(-rows // kchunk)


# ---- activations -----------------------------------------------------------------------------------
def _snake_parts(x, a):
    v, a = _w(x), _w(a).reshape(1, -1)
    arg = a * v
    return v, a, arg, np.sin(arg), np.cos(arg)


def act(kind, x, a=None):
    """y = act(x) over x [rows][cols] (a [cols] for Snake) -> (y, scale)."""
    v = _w(x)
    if kind == IDENTITY:
        return v, np.abs(v)
    if kind == SIN:                               # judged absolutely, in units of 2^-24 (|sin| <= 1)
        return np.sin(v), np.ones_like(v)
    if kind == TANH:
        t = np.tanh(v)
        return t, np.abs(t)
    v, a, arg, s, c = _snake_parts(x, a)          # v + sin^2(a v) / a
    y = v + s * s / a
    #        |terms|                      d/d arg [sin^2(arg) / a] * |arg|
    return y, np.abs(v) + s * s / np.abs(a) + np.abs(2 * s * c / a) * np.abs(arg)


def act_deriv(kind, x, a=None):
    """dy/dx -> (d, scale); Snake: (d, scale, dy/da, its scale)."""
    v = _w(x)
    if kind == IDENTITY:
        return np.ones_like(v), np.ones_like(v)
    if kind == SIN:
        return np.cos(v), np.ones_like(v)
    if kind == TANH:                              # 1 - t^2: both terms count where they cancel
        t = np.tanh(v)
        return 1.0 - t * t, 1.0 + t * t
    v, a, arg, s, c = _snake_parts(x, a)
    c2 = c * c - s * s                            # cos(2 arg)
    d = 1.0 + 2 * s * c                           # 1 + sin(2 a v)
    sd = 1.0 + np.abs(2 * s * c) + np.abs(2 * c2) * np.abs(arg)
    da = (2 * v * s * c - s * s / a) / a          # dy/da = (2 v s c - s^2 / a) / a
    sda = (np.abs(2 * v * s * c) + s * s / np.abs(a)
           + (np.abs(2 * v * c2) + np.abs(2 * s * c / a)) * np.abs(arg)) / np.abs(a)
    return d, sd, da, sda


def act_bwd(kind, x, gy, a=None):
    """Autograd of act() for dL/dy = gy: {"gx": (gy dy/dx, scale)} and, for Snake, "da_prod":
    (gy dy/da per element, scale) whose column sums are da."""
    g = _w(gy)
    r = act_deriv(kind, x, a)
    out = {"gx": (g * r[0], np.abs(g) * r[1])}
    if kind == SNAKE:
        out["da_prod"] = (g * r[2], np.abs(g) * r[3])
    return out


def units(got, ref, scale):
    """Largest |got - ref| in units of 2^-24 * scale over the elements with scale > 0, and whether
    every element with scale == 0 equals its reference exactly (NaN counts as infinitely far)."""
    got = np.asarray(got, F64).reshape(ref.shape)
    err = np.abs(got - ref)
    err = np.where(np.isnan(err), np.inf, err)
    pos = scale > 0
    worst = float(np.max(err[pos] / (U * scale[pos]), initial=0.0))
    return worst, bool(np.all(err[~pos] == 0))
