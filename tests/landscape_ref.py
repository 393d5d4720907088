"""The loss-landscape plane restated in numpy, independent of inr_for_audio_amd.landscape (a plain
module like errlog.py: no fixtures, nothing collected).

directions(): the definition of the plane's two grid-step vectors in fp64 (raw draws ->
Gram-Schmidt -> filter normalisation -> scale), rounded to fp32 once.  cell_params(): theta_ij with the
oracle's fp32 fma.  cell_loss(): the MSE of theta_ij through the oracle's forward, in fp64 or with the
HIP path's fp16 storage emulated (half=True)."""
import numpy as np

from oracle import siren_oracle as orc

F32, F64 = np.float32, np.float64


def _dot(xs, ys):
    return float(sum(np.sum(x * y) for x, y in zip(xs, ys)))


def orthogonalise(r1, r2):
    d1 = [np.asarray(r, F64) for r in r1]
    r2 = [np.asarray(r, F64) for r in r2]
    c = _dot(r2, d1) / _dot(d1, d1)
    return d1, [b - c * a for a, b in zip(d1, r2)]


def filter_normalise(d, theta):
    out = []
    for x, t in zip(d, theta):
        if x.ndim <= 1:
            out.append(np.sign(x) * np.abs(t))
            continue
        y = np.zeros_like(x)
        for f in range(x.shape[0]):
            dn = np.sqrt(np.sum(x[f] * x[f]))
            if dn > 0:
                y[f] = x[f] * (np.sqrt(np.sum(t[f] * t[f])) / dn)
        out.append(y)
    return out


def directions(theta, r1, r2, distance=2.0, steps=30, stage="final"):
    """(d1, d2) as lists of arrays.  stage 'orth': after Gram-Schmidt (fp64); 'filter': after filter
    normalisation (fp64); 'final': scaled to one grid step and rounded to fp32."""
    theta = [np.asarray(np.asarray(t, F32), F64) for t in theta]
    ds = orthogonalise([np.asarray(r, F32) for r in r1], [np.asarray(r, F32) for r in r2])
    if stage == "orth":
        return ds
    ds = [filter_normalise(d, theta) for d in ds]
    if stage == "filter":
        return ds
    tn = np.sqrt(_dot(theta, theta))
    out = []
    for d in ds:
        dn = np.sqrt(_dot(d, d))
        s = (tn * distance / steps) / dn if dn > 0 else 0.0
        out.append([(x * s).astype(F32) for x in d])
    return out


def coeff(k, steps):
    return k - steps / 2


def cell_params(theta, d1, d2, steps, i, j):
    """theta_ij = fma(b_j, d2, fma(a_i, d1, theta)) in fp32, one array per parameter."""
    a, b = F32(coeff(i, steps)), F32(coeff(j, steps))
    return [orc.fma32(b, np.asarray(v, F32), orc.fma32(a, np.asarray(u, F32), np.asarray(t, F32)))
            for t, u, v in zip(theta, d1, d2)]


def oracle_params(names, values, counts, first_linear=False, last_linear=True, hidden_omega=30.0):
    """orc.Params of a {name: value} parameter list; counts = (num_sine, num_snake, num_tanh)."""
    return orc.Params.from_state_dict(dict(zip(names, values)), counts[0], counts[1], counts[2],
                                      first_linear=first_linear, last_linear=last_linear, hidden_omega=hidden_omega)


def cell_loss(p, t, y, omega0, omega, half=False):
    """mean (f_theta(t) - y)^2 through the oracle: fp64 arithmetic, or (half=True) the fp16 storage of
    the HIP path emulated."""
    out, _ = orc.forward(p, np.asarray(t, F32), omega0, omega, half=half, dtype=F64)
    return orc.mse(out, y)


def min_abs_snake_a(names, theta, d1, d2, steps):
    """min over the grid's cells of |a| over every Snake a (names ending in '.a'); inf without one."""
    worst = np.inf
    for i in range(steps):
        for j in range(steps):
            cell = cell_params(theta, d1, d2, steps, i, j)
            for n, v in zip(names, cell):
                if n.endswith(".a"):
                    worst = min(worst, float(np.min(np.abs(v))))
    return worst
