"""The loss-landscape plane of run.py:192-208 (``visualization=True``): host side.

The reference hands the fitted model to ``loss_landscapes.random_plane(model, metric, distance=2,
steps=30, normalization='filter')``.  That package is not a dependency of this project, so the plane
is restated here from its published definition (Li et al. 2018, "Visualizing the Loss Landscape of
Neural Nets", filter normalisation) and parity is to this formula, not to an installed module:

theta is the list of model parameters in named_parameters() order.

1. raw draws r1, r2: torch.rand (U[0, 1), fp32, CPU), one tensor per parameter in order, all of r1
   before all of r2, from one generator;
2. d1 = r1, d2 = r2 - (<r2, r1> / <r1, r1>) r1 (inner products over all parameters);
3. filter normalisation of each direction: a tensor of 2 or more dimensions has one filter per slice
   along dim 0, d[f] *= |theta[f]| / |d[f]|; every element of a 1-D tensor is its own filter,
   d[f] = sign(d[f]) |theta[f]|; a filter of d with zero norm stays zero.  The directions are not
   orthogonalised again afterwards (nor are they in the package);
4. scale: d *= (|theta| distance / steps) / |d| over all parameters: the vectors hold one grid step.

Everything is computed in fp64 from the fp32 inputs and rounded to fp32 once.  The grid itself
(theta_ij = fma(b_j, d2, fma(a_i, d1, theta)), a_i = i - steps / 2, b_j = j - steps / 2) and its 900
forward passes run on the device: engine.SirenEngine.loss_plane (csrc/plane.hip).

One thing the package does is deliberately not reproduced: its in-place walk over the grid is
remembered to evaluate every other column one step further along d2.  The plane here is the regular
grid of the definition above.
"""
from __future__ import annotations

import warnings

import torch


def draw_raw(shapes, generator=None):
    """(r1, r2): torch.rand per parameter shape, all of r1 first, then all of r2 (step 1)."""
    r1 = [torch.rand(tuple(s), generator=generator, dtype=torch.float32) for s in shapes]
    r2 = [torch.rand(tuple(s), generator=generator, dtype=torch.float32) for s in shapes]
    return r1, r2


def _dot(xs, ys) -> torch.Tensor:
    return sum(((x * y).sum() for x, y in zip(xs, ys)), torch.zeros((), dtype=torch.float64))


def orthogonalise(r1, r2):
    """(d1, d2) of step 2 as fp64 lists: d1 = r1, d2 = r2 minus its component along r1."""
    d1 = [r.detach().to("cpu", torch.float64) for r in r1]
    r2 = [r.detach().to("cpu", torch.float64) for r in r2]
    c = _dot(r2, d1) / _dot(d1, d1)
    return d1, [b - c * a for a, b in zip(d1, r2)]


def filter_normalise(d, theta):
    """Step 3 on one direction (fp64 lists; returns a new list)."""
    out = []
    for x, t in zip(d, theta):
        if x.dim() <= 1:   # every element its own filter: sign(d) |theta| (sign(0) = 0: a zero filter stays zero)
            out.append(torch.sign(x) * t.abs())
            continue
        xf, tf = x.reshape(x.shape[0], -1), t.reshape(t.shape[0], -1)
        dn, tn = xf.norm(dim=1), tf.norm(dim=1)
        s = torch.where(dn > 0, tn / torch.where(dn > 0, dn, torch.ones_like(dn)), torch.zeros_like(dn))
        out.append((xf * s[:, None]).reshape(x.shape))
    return out


def plane_directions(params, *, distance=2.0, steps=30, generator=None, raw=None, normalization="filter"):
    """The two grid-step vectors (d1, d2) of the plane around `params` (run.py:194-198: distance=2,
    steps=30, normalization='filter'), as lists of fp32 CPU tensors in the parameters' own shapes.

    `params`: the model parameters in named_parameters() order.  `generator`: the torch.Generator of
    the draws (None: the global RNG).  `raw=(r1, r2)` replaces the draws."""
    if normalization != "filter":
        raise NotImplementedError(f"normalization={normalization!r}: only 'filter' (run.py:198) is implemented")
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"steps={steps!r} must be at least 1")
    params = list(params)
    theta = [p.detach().to("cpu", torch.float32).to(torch.float64) for p in params]
    r1, r2 = draw_raw([t.shape for t in theta], generator) if raw is None else raw
    if len(r1) != len(theta) or len(r2) != len(theta) or \
            any(tuple(a.shape) != tuple(t.shape) or tuple(b.shape) != tuple(t.shape) for a, b, t in zip(r1, r2, theta)):
        raise ValueError("raw=(r1, r2): one tensor per parameter, in the parameters' shapes")
    tnorm = _dot(theta, theta).sqrt()
    out = []
    for d in orthogonalise(r1, r2):
        d = filter_normalise(d, theta)
        dnorm = _dot(d, d).sqrt()
        s = (tnorm * float(distance) / steps) / dnorm if dnorm > 0 else torch.zeros((), dtype=torch.float64)
        out.append([(x * s).to(torch.float32) for x in d])
    return out[0], out[1]


def grid_coefficient(k: int, steps: int) -> float:
    """a_k = b_k = k - steps / 2 (float division): with even steps, cell steps / 2 is theta itself."""
    return float(k) - steps / 2


def save_plane(plane, folder: str) -> list:
    """Write landscape.npy ([steps][steps] float64) into `folder` and, when matplotlib is importable,
    landscape.png: the 3-D surface of run.py:200-208 (column index on x, row index on y, z range
    0 .. 0.15, the reference's title).  Returns the paths written."""
    import numpy as np
    plane = np.asarray(plane, dtype=np.float64)
    paths = [f"{folder}/landscape.npy"]
    np.save(paths[0], plane)
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        warnings.warn("matplotlib is not importable: landscape.png is skipped (landscape.npy holds the plane)",
                      RuntimeWarning, stacklevel=2)
        return paths
    steps = plane.shape[0]
    X, Y = np.meshgrid(np.arange(plane.shape[1]), np.arange(steps))
    fig = plt.figure()
    ax = fig.add_subplot(projection="3d")
    ax.plot_surface(X, Y, plane, rstride=1, cstride=1, cmap="viridis", edgecolor="none")
    ax.set_title("Surface Plot of Loss Landscape")
    ax.set_zlim(0, 0.15)
    paths.append(f"{folder}/landscape.png")
    fig.savefig(paths[1])
    plt.close(fig)
    return paths
