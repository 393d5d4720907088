"""The any-grid-size KAN kernels (csrc/kan_general.hip) through the C-ABI, the way
tests/test_gpu_kan_kernels.py drives the grid-5 kernels: one-layer nets select the kernel by shape,
judged against tests/kan_grids_ref.py (fp64, element by element) on per-input non-uniform knots
(kan_knots_g), with a NaN-filled workspace.

  kang_head_fwd    L = 1, out = 1, in <= 64, forward       kang_fwd_fused   any other forward
  kang_dw_fused    every backward                          kang_dx_fused    backward with grad_coords
  kang_head_train  siren_kan_train_step_loss (MSE, L1) and siren_kan_step_backward (a given g)
There is no one-pass backward in this set: out <= 64 with grad_coords runs kang_dw_fused + kang_dx_fused.

Grid sizes: 1 (NB = 4: the window is the whole row and clamps at both ends), 2, 4 and 6 (the
neighbours of 5, where a left-over literal 8, 9 or 12 shows), 11 (K1 = 15, 9 inputs per chunk, 135
columns padded to 144), 16 (7 inputs per chunk), 64 (2 inputs per chunk, the largest tables).

Gates, as in test_gpu_kan_kernels.py: 1e-5 * sum|terms| + 1e-12 per element -- a row has 5 non-zero
terms per input at any grid size and the added columns contribute exact zeros, so the summation
error per input is what it is at grid 5; the basis derivative as a value within kan_ref.DERIV_C = 28
units of 2^-24 * scale', 4 x the fp32 oracle's bound, which tests/test_kan_grids_host.py re-asserts
on these knots; the forward bases bit for bit torch's CPU recursion (kan_div is the IEEE quotient
on these knots: the same host module)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import kan_grids_ref as kg

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRIDS = kg.GRIDS


def IC(G):
    return kg.dims(G)[3]


class Net:
    """A KANLinear stack of grid size G on the device, with the C-ABI structs; layers =
    [(grid, bw, sw, sc), ...] as fp32 numpy arrays."""

    def __init__(self, lib, dev, widths, layers, G):
        from inr_for_audio_amd._lib import SirenKanGrads, SirenKanNet, ptr
        self.lib, self.dev, self.widths, self.L, self.G = lib, dev, list(widths), len(layers), G
        self.p = [[torch.from_numpy(np.ascontiguousarray(a, F32)).to(dev) for a in lay] for lay in layers]
        self.net = SirenKanNet()
        self.net.n_layers, self.net.grid_size = self.L, G
        for l, w in enumerate(widths):
            self.net.width[l] = w
        sizes = []
        for l, (g, bw, sw, sc) in enumerate(self.p):
            assert g.shape == (widths[l], G + 7) and bw.shape == (widths[l + 1], widths[l])
            assert sw.shape == (widths[l + 1], widths[l], G + 3) and sc.shape == bw.shape
            n = self.net
            n.grid[l], n.base_w[l], n.spline_w[l], n.scaler[l] = (ptr(t) for t in (g, bw, sw, sc))
            sizes += [bw.numel(), sw.numel(), sc.numel()]
        self.flat = torch.zeros(sum(sizes) + 1, dtype=torch.float32, device=dev)
        self.views, o = [], 0
        for s in sizes:
            self.views.append(self.flat[o:o + s])
            o += s
        self.sse = self.flat[o:o + 1]
        self.gr = SirenKanGrads()
        for l in range(self.L):
            self.gr.base_w[l], self.gr.spline_w[l], self.gr.scaler[l] = (ptr(v) for v in self.views[3 * l:3 * l + 3])
        self.gr.sse, self.gr.flat, self.gr.flat_len = ptr(self.sse), ptr(self.flat), self.flat.numel()

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def bind(self, x, splits, target=None, n_valid=0, n_total=1.0, zero_grads=0):
        """A batch over coords x [rows][width[0]] with a fresh NaN-filled workspace."""
        from inr_for_audio_amd._lib import SirenKanBatch, ptr
        rows = x.shape[0]
        self.x = torch.from_numpy(np.ascontiguousarray(x, F32)).to(self.dev)
        self.rows, self.splits = rows, splits
        nws = int(self.lib.siren_kan_workspace_floats(ctypes.byref(self.net), rows, splits))
        self.X_off, self.G0_off, total = kg.workspace_floats(self.widths, rows, splits, self.G)
        assert total == nws, (total, nws)
        self.ws = torch.full((nws,), float("nan"), dtype=torch.float32, device=self.dev)
        self.out = torch.full((rows, self.widths[-1]), float("nan"), dtype=torch.float32, device=self.dev)
        self.g = torch.zeros(rows, self.widths[-1], dtype=torch.float32, device=self.dev)
        self.target = None if target is None else torch.from_numpy(np.ascontiguousarray(target, F32)).to(self.dev)
        b = self.b = SirenKanBatch()
        b.rows, b.n_valid, b.n_total, b.splits, b.zero_grads = rows, n_valid, float(n_total), splits, zero_grads
        b.coords, b.target, b.out, b.g, b.ws = ptr(self.x), ptr(self.target), ptr(self.out), ptr(self.g), ptr(self.ws)
        return self

    def forward(self):
        from inr_for_audio_amd._lib import check
        check(self.lib.siren_kan_forward(ctypes.byref(self.net), ctypes.byref(self.b), self._stream()),
              "siren_kan_forward")
        torch.cuda.synchronize()
        return self.out.cpu().numpy()

    def backward(self, G, want_dx):
        """siren_kan_backward after forward() on the same batch; returns (grads per layer, dX or None)."""
        from inr_for_audio_amd._lib import check, ptr
        self.g.copy_(torch.from_numpy(np.ascontiguousarray(G, F32)).reshape(self.g.shape))
        gx = None
        if want_dx:
            gx = torch.full((self.rows, self.widths[0]), float("nan"), dtype=torch.float32, device=self.dev)
        check(self.lib.siren_kan_backward(ctypes.byref(self.net), ctypes.byref(self.gr), ctypes.byref(self.b), ptr(gx),
                                          self._stream()), "siren_kan_backward")
        torch.cuda.synchronize()
        return self.grads(), None if gx is None else gx.cpu().numpy()

    def train_step(self, loss_mode=0):
        from inr_for_audio_amd._lib import check
        check(self.lib.siren_kan_train_step_loss(ctypes.byref(self.net), ctypes.byref(self.gr), ctypes.byref(self.b),
                                                 loss_mode, self._stream()), "siren_kan_train_step_loss")
        torch.cuda.synchronize()
        return self.out.cpu().numpy().reshape(-1), self.g.cpu().numpy().reshape(-1)

    def step_backward(self, g):
        from inr_for_audio_amd._lib import check
        self.g.copy_(torch.from_numpy(np.ascontiguousarray(g, F32)).reshape(self.g.shape))
        check(self.lib.siren_kan_step_backward(ctypes.byref(self.net), ctypes.byref(self.gr), ctypes.byref(self.b),
                                               self._stream()), "siren_kan_step_backward")
        torch.cuda.synchronize()
        return self.grads()

    def grads(self):
        names = ("base_weight", "spline_weight", "spline_scaler")
        return [{nm: self.views[3 * l + k].cpu().numpy().reshape(self.p[l][1 + k].shape) for k, nm in enumerate(names)}
                for l in range(self.L)]

    def ws_piece(self, off, shape):
        return self.ws[off:off + int(np.prod(shape))].cpu().numpy().reshape(shape)


def _inputs(grid, rows, seed=0):
    """rows probe inputs: with room, uniform draws, every knot and its two neighbours, +-0, +-1e-30."""
    extra = 3 * grid.shape[1] + 4
    if rows >= extra:
        return kg.probe_inputs(grid, rows - extra, seed)
    return kg.probe_inputs(grid, 24, seed)[-(rows + 8):][:rows]


def _weights(fin, fout, G, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(fout, fin)).astype(F32), rng.normal(size=(fout, fin, G + 3)).astype(F32),
            rng.normal(size=(fout, fin)).astype(F32))


def _one_hot_layer(fin, G):
    """out = NB in, base_weight 0, spline_scaler 1, spline_weight[NB i + c][i][c] = 1."""
    nb = G + 3
    sw = np.zeros((nb * fin, fin, nb), F32)
    for i in range(fin):
        for c in range(nb):
            sw[nb * i + c, i, c] = 1.0
    return np.zeros((nb * fin, fin), F32), sw, np.ones((nb * fin, fin), F32)


def _close(got, ref_terms, what):
    """|got - ref| <= 1e-5 * terms + 1e-12 for every element (NaN fails)."""
    ref, terms = ref_terms
    got = np.asarray(got, np.float64).reshape(ref.shape)
    lim = 1e-5 * terms + 1e-12
    err = np.abs(got - ref)
    bad = np.argwhere(~(err <= lim))
    print(f"{what}: worst |err| / (1e-5 terms + 1e-12) = {np.nanmax(err / lim):.3g}")
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[:4].T)], ref[tuple(bad[:4].T)])


def _check_grads(got, ref, what, scale=1.0):
    for nm in ("base_weight", "spline_weight", "spline_scaler"):
        r, t = ref[nm]
        _close(got[nm], (scale * r, scale * t), f"{what} d {nm}")


def _torch_bases(x, grid):
    from inr_for_audio_amd.kan import bspline_bases
    return bspline_bases(torch.from_numpy(x), torch.from_numpy(grid), 3).numpy()


# ---- a. forward bases, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("G", GRIDS)
def test_fused_forward_bases_bit_exact(lib, dev, G):
    """kang_fwd_fused with in = IC + 1 (one full chunk and a ragged one of one input) and a one-hot
    spline_weight of NB in outputs (more than 64: two or more out tiles): output column NB i + c is
    B_c(x_i) bit for bit as torch's CPU recursion gives it -- every other product is an exact 0."""
    fin = IC(G) + 1
    assert (G + 3) * fin > 64
    grid = kg.kan_knots_g(fin, G, 20 + G)
    x = kg.probe_inputs(grid, 600, G)
    out = Net(lib, dev, [fin, (G + 3) * fin], [(grid, *_one_hot_layer(fin, G))], G).bind(x, 1).forward()
    ref = _torch_bases(x, grid).reshape(x.shape[0], -1)
    bad = np.argwhere(out != ref)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), out[tuple(bad[:5].T)], ref[tuple(bad[:5].T)])


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("fin", [3, 64])
def test_head_forward_bases_bit_exact(lib, dev, G, fin):
    """kang_head_fwd (lane = input, weights and tables in LDS): out = 1 and a one-hot spline_weight
    at (i, c) output exactly B_c(x_i), for every basis of lane 0, a middle lane and lane in - 1."""
    grid = kg.kan_knots_g(fin, G, 30 + fin + G)
    x = kg.probe_inputs(grid, 200, fin)
    ref = _torch_bases(x, grid)
    nb = G + 3
    net = Net(lib, dev, [fin, 1], [(grid, np.zeros((1, fin), F32), np.zeros((1, fin, nb), F32), np.ones((1, fin), F32))], G)
    net.bind(x, 1)
    sw = net.p[0][2]
    for i in sorted({0, fin // 2, fin - 1}):
        for c in range(nb):
            sw.zero_()
            sw[0, i, c] = 1.0
            out = net.forward().reshape(-1)
            bad = np.flatnonzero(out != ref[:, i, c])
            assert bad.size == 0, (i, c, bad[:5], x[bad[:5], i], out[bad[:5]], ref[bad[:5], i, c])


# ---- b. forward against fp64, per element -----------------------------------------------------
def _fwd_cases(G):
    ic = IC(G)
    return [(1, 1, 1), (3, 1, 65), (64, 1, 300),                                    # kang_head_fwd
            (1, 16, 63), (ic + 1, 5, 64), (2 * ic + 1, 70, 300), (64, 16, 1)]       # kang_fwd_fused


@pytest.mark.parametrize("G,fin,fout,rows", [(G, *c) for G in GRIDS for c in _fwd_cases(G)])
def test_forward_vs_fp64(lib, dev, G, fin, fout, rows):
    grid = kg.kan_knots_g(fin, G, 100 + fin + G)
    x = _inputs(grid, rows, fout)
    w = _weights(fin, fout, G, 7 * fin + fout)
    out = Net(lib, dev, [fin, fout], [(grid, *w)], G).bind(x, 1).forward()
    _close(out, kg.layer(x, grid, *w)["out"], f"G {G} out")


# ---- c. the basis derivative as a value -------------------------------------------------------
def _deriv_gate(dx, x, grid, basis_of_row, what):
    """dx[n][i] must be B'_{basis_of_row[n]}(x[n][i]) within DERIV_C * 2^-24 * scale', and exactly
    0 where x[n][i] lies outside input i's knot range."""
    _, db, _, sdb = kg.bases64(x, grid)
    idx = np.asarray(basis_of_row)[:, None, None]
    ref = np.take_along_axis(db, np.broadcast_to(idx, db.shape[:2] + (1,)), 2)[..., 0]
    scale = np.take_along_axis(sdb, np.broadcast_to(idx, db.shape[:2] + (1,)), 2)[..., 0]
    lim = kg.DERIV_C * 2.0 ** -24 * scale
    err = np.abs(dx.astype(np.float64) - ref)
    worst = np.max(err[scale > 0] / (2.0 ** -24 * scale[scale > 0]), initial=0.0)
    print(f"{what}: worst B' error {worst:.2f} x 2^-24 scale' (gate {kg.DERIV_C:g})")
    bad = np.argwhere(~(err <= lim))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), dx[tuple(bad[:4].T)], ref[tuple(bad[:4].T)])
    assert np.all(dx[kg.outside(x, grid)] == 0), what


@pytest.mark.parametrize("G", [1, 11, 64])
def test_basis_derivative_value_dx(lib, dev, G):
    """B' as kang_dx_fused computed it (v_rcp_f32 quotients), one value per element of dX: one-hot
    combined weight with an output per (input, basis) pair, G[n][NB i + c] = (c == n % NB), each
    probe input repeated over NB rows, so dX[n][i] = B'_{n % NB}(x[n][i]) -- selection by 1 and 0 is
    exact through the MFMA chain and the window's contraction.  in = IC + 1: both chunks."""
    nb, fin = G + 3, IC(G) + 1
    grid = kg.kan_knots_g(fin, G, 40 + G)
    x = np.repeat(kg.probe_inputs(grid, 60, G), nb, axis=0)
    rows, fout = x.shape[0], nb * fin
    c_of = np.arange(rows) % nb
    up = np.zeros((rows, fout), F32)
    for i in range(fin):
        up[np.arange(rows), nb * i + c_of] = 1.0
    net = Net(lib, dev, [fin, fout], [(grid, *_one_hot_layer(fin, G))], G).bind(x, 4)
    net.forward()
    _, dx = net.backward(up, True)
    _deriv_gate(dx, x, grid, c_of, f"G {G} kang_dx_fused")


def _scaled_first_layer(h, G, seed, flip):
    """Layer 0 of a [1, h, 1] net that hands t >= 18 to lane i as t * s_i exactly, s_i = +-2^-6
    (even lanes positive, odd negative; the other way round with flip): t is outside layer 0's knot
    range (every basis an exact 0) and SiLU(t) = t in fp32 there, so X[1][n][i] = t_n s_i."""
    g0 = kg.kan_knots_g(1, G, seed)
    assert g0.max() < 17
    s = np.where(np.arange(h) % 2 == int(flip), 1.0, -1.0).astype(F32) * F32(2.0 ** -6)
    _, sw, sc = _weights(1, h, G, seed)
    return (g0, s.reshape(h, 1), sw, sc), s


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("G,h,lanes", [(1, 3, (0, 1, 2)), (1, 64, (0, 17, 63)), (11, 3, (0, 1, 2)), (11, 64, (0, 17, 63)),
                                       (64, 3, (0, 1, 2)), (64, 64, (0, 63))])
def test_basis_derivative_value_head_train(lib, dev, G, h, lanes, flip):
    """kang_head_train's B' (IEEE quotients through kan_div) as a value: [1, h, 1] with the last
    layer's weight one-hot at (i, c), targets -2^25 and n_total = 2, so g = 2^25 exactly for every
    row and Gin[n][i] = 2^25 B'_c(X[1][n][i]).  Layer 0 scales the coordinates by +-2^-6 exactly, so
    lane i meets its own knots and their one-ulp neighbours (those of its sign with
    |knot| >= 18 / 64; the other sign with flip) as well as points inside and outside its range."""
    nb = G + 3
    lay0, s = _scaled_first_layer(h, G, 50 + h, flip)
    g1 = kg.kan_knots_g(h, G, 60 + h)
    p = kg.probe_inputs(g1, 40, h)
    t = np.concatenate([64.0 * np.abs(p[:, i][(np.sign(p[:, i]) == np.sign(s[i])) & (np.abs(p[:, i]) >= 18 / 64)])
                        for i in lanes]).astype(F32).reshape(-1, 1)
    rows = t.shape[0]
    x1 = t * s[None, :]
    hit = sum(int(np.sum(x1[:, i][:, None] == g1[i][None, :])) for i in lanes)
    assert hit >= 2 * len(lanes), hit     # the lanes do meet knots of their own
    net = Net(lib, dev, [1, h, 1],
              [lay0, (g1, np.zeros((1, h), F32), np.zeros((1, h, nb), F32), np.ones((1, h), F32))], G)
    net.bind(t, 2, target=np.full(rows, -2.0 ** 25, F32), n_valid=rows, n_total=2.0)
    sw = net.p[1][2]
    worst = 0.0
    for i in lanes:
        _, db, _, sdb = kg.bases64(x1[:, i:i + 1], g1[i:i + 1])
        out_i = kg.outside(x1[:, i:i + 1], g1[i:i + 1])[:, 0]
        for c in range(nb):
            sw.zero_()
            sw[0, i, c] = 1.0
            _, g = net.train_step()
            if c == 0:
                assert np.array_equal(net.ws_piece(net.X_off[1], (rows, h)), x1)
            assert np.all(g == F32(2.0 ** 25))
            gin = net.ws_piece(net.G0_off, (rows, h))
            assert np.all(gin[:, np.delete(np.arange(h), i)] == 0)
            got = gin[:, i].astype(np.float64) * 2.0 ** -25
            ref, scale = db[:, 0, c], sdb[:, 0, c]
            err = np.abs(got - ref)
            assert np.all(err <= kg.DERIV_C * 2.0 ** -24 * scale), (i, c)
            assert np.all(got[out_i] == 0), (i, c)
            worst = max(worst, np.max(err[scale > 0] / (2.0 ** -24 * scale[scale > 0]), initial=0.0))
    print(f"G {G} kang_head_train h {h}: worst B' error {worst:.2f} x 2^-24 scale' (gate {kg.DERIV_C:g})")


# ---- d. gradients against fp64, per element ---------------------------------------------------
def _bwd_cases(G):
    ic = IC(G)
    return [(1, 16, 200, 3), (ic + 1, 48, 300, 1), (2 * ic + 1, 70, 300, 2), (64, 1, 300, 2)]


def _layer_case(lib, dev, G, fin, fout, rows, splits, seed=0):
    grid = kg.kan_knots_g(fin, G, 200 + fin + G + seed)
    x = _inputs(grid, rows, fout + seed)
    w = _weights(fin, fout, G, 3 * fin + fout + seed)
    up = np.random.default_rng(rows + fout).normal(size=(rows, fout)).astype(F32)
    return grid, x, w, up, Net(lib, dev, [fin, fout], [(grid, *w)], G).bind(x, splits)


@pytest.mark.parametrize("want_dx", [True, False])
@pytest.mark.parametrize("G,fin,fout,rows,splits", [(G, *c) for G in GRIDS for c in _bwd_cases(G)])
def test_backward_vs_fp64(lib, dev, G, fin, fout, rows, splits, want_dx):
    grid, x, w, up, net = _layer_case(lib, dev, G, fin, fout, rows, splits)
    net.forward()
    grads, dx = net.backward(up, want_dx)
    ref = kg.layer(x, grid, *w, up)
    _check_grads(grads[0], ref, f"G {G} grad")
    if want_dx:
        _close(dx, ref["dX"], f"G {G} dX")


@pytest.mark.parametrize("want_dx", [True, False])
def test_backward_accumulates_and_zero_grads(lib, dev, want_dx):
    """A second backward into the same buffers without zero_grads gives twice the reference; with
    zero_grads and `flat` set, NaN-filled gradient buffers are cleared first."""
    G = 11
    grid, x, w, up, net = _layer_case(lib, dev, G, 2 * IC(G) + 1, 70, 300, 2, seed=1)
    ref = kg.layer(x, grid, *w, up)
    net.forward()
    net.backward(up, want_dx)
    grads, dx = net.backward(up, want_dx)
    _check_grads(grads[0], ref, "twice", scale=2.0)
    if want_dx:
        _close(dx, ref["dX"], "dX (not accumulated)")
    net.flat.fill_(float("nan"))
    net.b.zero_grads = 1
    grads, _ = net.backward(up, want_dx)
    _check_grads(grads[0], ref, "zero_grads")


def test_backward_is_deterministic(lib, dev):
    """Two calls of the (2 IC + 1, 70, 300 rows, 2 splits) backward at grid 11 agree bit for bit."""
    G = 11
    _, _, _, up, net = _layer_case(lib, dev, G, 2 * IC(G) + 1, 70, 300, 2)
    net.b.zero_grads = 1
    net.forward()
    g1, dx1 = net.backward(up, True)
    net.forward()
    g2, dx2 = net.backward(up, True)
    assert np.array_equal(dx1, dx2)
    for nm in g1[0]:
        assert np.array_equal(g1[0][nm], g2[0][nm]), nm


@pytest.mark.parametrize("want_dx", [False, True])
def test_slab_reduce_16_via_layer_backward(lib, dev, want_dx):
    """[1 -> 16] at grid 11, 4161 rows, 66 splits: 66 one-tile slabs of 16 x 15 columns (more than 64
    slabs, under 16 384 columns: kan_slab_reduce_kernel<16>; every other case here runs <64>)."""
    grid, x, w, up, net = _layer_case(lib, dev, 11, 1, 16, 4161, 66, seed=2)
    net.forward()
    grads, dx = net.backward(up, want_dx)
    ref = kg.layer(x, grid, *w, up)
    _check_grads(grads[0], ref, "grad")
    if want_dx:
        _close(dx, ref["dX"], "dX")


# ---- e. the fused step ------------------------------------------------------------------------
def _two_layer(lib, dev, G, h, rows, splits, seed):
    g0, g1 = kg.kan_knots_g(1, G, 400 + seed), kg.kan_knots_g(h, G, 500 + seed)
    w0, w1 = _weights(1, h, G, seed), _weights(h, 1, G, seed + 1)
    t = _inputs(g0, rows, seed)
    y = np.random.default_rng(seed).normal(size=rows).astype(F32)
    return (g0, g1, w0, w1, t, y), lambda: Net(lib, dev, [1, h, 1], [(g0, *w0), (g1, *w1)], G)


def _check_two_layer(net, data, out, g, grads, what):
    """out, Gin and every gradient of a [1, h, 1] step against kan_grids_ref, stage by stage: each
    stage's reference starts from the fp32 arrays the device handed it (X[1], g, Gin)."""
    g0, g1, w0, w1, t, _ = data
    rows, h = t.shape[0], g1.shape[0]
    x1 = net.ws_piece(net.X_off[1], (rows, h))
    _close(x1, kg.layer(t, g0, *w0)["out"], f"{what} X[1]")
    r1 = kg.layer(x1, g1, *w1, g.reshape(rows, 1))
    _close(out, r1["out"], f"{what} out")
    _check_grads(grads[1], r1, f"{what} layer 1")
    gin = net.ws_piece(net.G0_off, (rows, h))
    _close(gin, r1["dX"], f"{what} Gin")
    _check_grads(grads[0], kg.layer(t, g0, *w0, gin), f"{what} layer 0")


@pytest.mark.parametrize("loss_mode", [0, 1])
@pytest.mark.parametrize("G", [1, 11, 64])
@pytest.mark.parametrize("h", [3, 64])
def test_fused_step(lib, dev, G, h, loss_mode):
    """siren_kan_train_step_loss on [1, h, 1] (kang_fwd_fused, kang_head_train, kang_dw_fused) with
    n_valid < rows: out is siren_kan_forward's bit for bit; g is exact -- (out - y) fp32(2 / N) for
    MSE, sign(out - y) fp32(1 / N) for L1 with sign(0) = 0 (four targets are set to the output
    itself), 0 on the pad rows (their targets are NaN); the loss sum and every gradient agree with
    the fp64 reference; siren_kan_step_backward fed that g reproduces the gradients bit for bit."""
    rows, n_valid, n_total = 300, 270, 1234.0
    data, make = _two_layer(lib, dev, G, h, rows, 3, h + G)
    t, y = data[4], data[5].copy()
    out_f = make().bind(t, 3).forward().reshape(-1)
    y[:4] = out_f[:4]
    y[n_valid:] = np.nan
    a = make().bind(t, 3, target=y, n_valid=n_valid, n_total=n_total)
    a.flat.fill_(float("nan"))
    a.b.zero_grads = 1
    out, g = a.train_step(loss_mode)
    grads, loss_sum = a.grads(), float(a.sse.cpu())
    assert np.array_equal(out, out_f)
    err = out[:n_valid] - y[:n_valid]
    g_ref = np.zeros(rows, F32)
    g_ref[:n_valid] = np.sign(err) * F32(1.0 / n_total) if loss_mode else err * F32(2.0 / n_total)
    assert np.array_equal(g, g_ref) and np.all(g[:4] == 0)
    ref_sum = float(np.sum(np.abs(err.astype(np.float64)) if loss_mode else err.astype(np.float64) ** 2))
    assert abs(loss_sum - ref_sum) <= 1e-5 * ref_sum, (loss_sum, ref_sum)
    _check_two_layer(a, data, out, g, grads, f"G {G} h {h} mode {loss_mode}")
    b = make().bind(t, 3)
    b.forward()
    b.flat.fill_(float("nan"))
    b.b.zero_grads = 1
    again = b.step_backward(g)
    for l in range(2):
        for nm in grads[l]:
            assert np.array_equal(grads[l][nm], again[l][nm]), (l, nm)


def test_slab_reduce_16_via_head_train(lib, dev):
    """[1, 8, 1] at grid 11, 16 700 rows, splits 17: kang_head_train runs 66 blocks of 254 rows (slab
    room 4 * 17 = 68 rows of 15 * 8 columns)."""
    rows = 16700
    data, make = _two_layer(lib, dev, 11, 8, rows, 17, 8)
    net = make().bind(data[4], 17, target=data[5], n_valid=rows, n_total=float(rows))
    out, g = net.train_step()
    _check_two_layer(net, data, out, g, net.grads(), "A")


# ---- f. the knob: grid 5 through both kernel sets -----------------------------------------------
def _both_sets(lib, run):
    from inr_for_audio_amd._lib import Opt, options
    own = run()
    with options(lib, {Opt.KAN_GENERAL: 1}):
        general = run()
    return own, general


def _same(a, b):
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


def test_knob_bases_bit_identical(lib, dev):
    """SIREN_OPT_KAN_GENERAL at grid 5: the any-grid-size forward's bases are the grid-5 kernels'
    bit for bit (and torch's), fused forward (in = 17: both chunks) and head forward."""
    G, fin = 5, 17
    grid = kg.kan_knots_g(fin, G, 25)
    x = kg.probe_inputs(grid, 600, G)
    own, general = _both_sets(lib, lambda: Net(lib, dev, [fin, 8 * fin], [(grid, *_one_hot_layer(fin, G))], G).bind(x, 1).forward())
    assert np.array_equal(own, general)
    assert np.array_equal(general, _torch_bases(x, grid).reshape(x.shape[0], -1))
    w = _weights(fin, 1, G, 3)
    own, general = _both_sets(lib, lambda: Net(lib, dev, [fin, 1], [(grid, *w)], G).bind(x, 1).forward())
    _close(own, kg.layer(x, grid, *w)["out"], "head out, grid-5 set")
    _close(general, kg.layer(x, grid, *w)["out"], "head out, general set")
    print(f"knob: head forward bit-identical: {_same(own, general)}")


def test_knob_selects_the_kernel_set(lib, dev):
    """The knob does switch sets: a (17 -> 48) backward with grad_coords is one launch of the kan_dx
    kind in the grid-5 set (the one-pass kernel) and a kan_dw plus a kan_dx launch in the general set."""
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd._lib import check

    def run():
        _, _, _, up, net = _layer_case(lib, dev, 5, 17, 48, 300, 1)
        net.forward()
        check(lib.siren_profile_mask(0xFFFFFFFF))
        check(lib.siren_profile_enable(64))
        try:
            net.backward(up, True)
            return {k: v[1] for k, v in _lib.profile_read().items() if v[1]}
        finally:
            check(lib.siren_profile_enable(0))

    own, general = _both_sets(lib, run)
    assert own.get("kan_dw", 0) == 0 and own["kan_dx"] == 1, own
    assert general["kan_dw"] == 1 and general["kan_dx"] == 1, general


@pytest.mark.parametrize("prefill", [False, True])
def test_knob_combine_and_param_grads_bit_identical(lib, dev, prefill):
    """One kan_combine and one kan_param_grads kernel (run-time NB) serve both sets: at grid 5 the
    combined W and W^T in the workspace and siren_kan_backward's three parameter gradients of a
    (17 -> 48) layer at 300 rows are bit-equal with the knob off and on -- from zeroed gradient
    buffers and, with prefill, accumulated onto the same non-zero contents."""
    G, fin, fout, rows = 5, 17, 48, 300
    wlen = fout * (G + 4) * fin
    pre = np.random.default_rng(5).normal(size=fout * fin * (G + 5) + 1).astype(F32)

    def run():
        _, _, _, up, net = _layer_case(lib, dev, G, fin, fout, rows, 1)
        net.forward()
        if prefill:
            net.flat.copy_(torch.from_numpy(pre))
        else:
            net.b.zero_grads = 1
        grads, _ = net.backward(up, True)
        return net.ws_piece(0, (wlen,)), net.ws_piece((wlen + 63) // 64 * 64, (wlen,)), grads[0]

    (w_a, wt_a, g_a), (w_b, wt_b, g_b) = _both_sets(lib, run)
    assert not np.isnan(w_a).any() and not np.isnan(wt_a).any()
    assert np.array_equal(w_a.reshape(fout, -1).T, wt_a.reshape(-1, fout))
    assert np.array_equal(w_a, w_b) and np.array_equal(wt_a, wt_b)
    for nm in g_a:
        assert not np.isnan(g_a[nm]).any(), nm
        assert np.array_equal(g_a[nm], g_b[nm]), nm


@pytest.mark.parametrize("rows,splits,blocks", [(256, 1, 1), (500, 1, 2), (1100, 1, 4), (1100, 2, 5)])
@pytest.mark.parametrize("G,general", [(5, 0), (5, 1), (11, 0)])
def test_head_partition_reproduces_step(lib, dev, G, general, rows, splits, blocks):
    """The head pass's block partition is one host function for both sets and the three sources of
    g: on [1, 64, 1], siren_kan_step_backward fed the step's own g reproduces the step's gradients
    bit for bit, at grid 5 (both sets) and 11, for 1, 2, 4 and 5 blocks (the count of loss partials
    the step wrote).  Through the C-ABI a pass has 4 * splits slab rows and ceil(rows / 256) loss
    partials, so at 1100 rows only 4 and 5 blocks can be had; 1 and 2 blocks take fewer rows."""
    from inr_for_audio_amd._lib import Opt, options
    h = 64
    data, make = _two_layer(lib, dev, G, h, rows, splits, 11 + G)
    with options(lib, {Opt.KAN_GENERAL: general}):
        a = make().bind(data[4], splits, target=data[5], n_valid=rows - 7, n_total=float(rows))
        a.flat.fill_(float("nan"))
        a.b.zero_grads = 1
        _, g = a.train_step()
        grads = a.grads()
        parts = a.ws_piece(a.G0_off + 2 * ((rows * h + 63) // 64 * 64), ((rows + 255) // 256,))
        assert int(np.sum(~np.isnan(parts))) == blocks
        b = make().bind(data[4], splits)
        b.forward()
        b.flat.fill_(float("nan"))
        b.b.zero_grads = 1
        again = b.step_backward(g)
    for l in range(2):
        for nm in grads[l]:
            assert not np.isnan(grads[l][nm]).any(), (l, nm)
            assert np.array_equal(grads[l][nm], again[l][nm]), (l, nm)


@pytest.mark.parametrize("fin,fout,rows,splits", [(17, 48, 300, 1), (33, 70, 300, 2), (64, 1, 300, 2)])
def test_knob_layer_within_gate(lib, dev, fin, fout, rows, splits):
    """Outputs and gradients of both sets at grid 5 within the gate of fp64; whether they are
    bit-identical is printed (the general set adds the same non-zero terms in the same order, but
    out <= 64 with grad_coords runs dW + dX there and the one-pass kernel in the grid-5 set)."""
    G = 5

    def run():
        grid, x, w, up, net = _layer_case(lib, dev, G, fin, fout, rows, splits)
        out = net.forward()
        grads, dx = net.backward(up, True)
        return grid, x, w, up, out, grads[0], dx

    own, general = _both_sets(lib, run)
    grid, x, w, up = own[:4]
    ref = kg.layer(x, grid, *w, up)
    for name, r in (("grid-5 set", own), ("general set", general)):
        _close(r[4], ref["out"], f"{name} out")
        _check_grads(r[5], ref, name)
        _close(r[6], ref["dX"], f"{name} dX")
    same = {"out": _same(own[4], general[4]), "dX": _same(own[6], general[6]),
            **{nm: _same(own[5][nm], general[5][nm]) for nm in own[5]}}
    print(f"knob ({fin}, {fout}): bit-identical to the grid-5 set: {same}")


@pytest.mark.parametrize("loss_mode", [0, 1])
def test_knob_fused_step_within_gate(lib, dev, loss_mode):
    G, h, rows = 5, 64, 300
    data, make = _two_layer(lib, dev, G, h, rows, 3, 7)

    def run():
        net = make().bind(data[4], 3, target=data[5], n_valid=rows - 30, n_total=float(rows))
        net.b.zero_grads = 1
        out, g = net.train_step(loss_mode)
        return net, out, g, net.grads()

    own, general = _both_sets(lib, run)
    for name, (net, out, g, grads) in (("grid-5 set", own), ("general set", general)):
        _check_two_layer(net, data, out, g, grads, name)
    same = {"out": _same(own[1], general[1]), "g": _same(own[2], general[2]),
            **{f"{l}.{nm}": _same(own[3][l][nm], general[3][l][nm]) for l in range(2) for nm in own[3][l]}}
    print(f"knob fused step mode {loss_mode}: bit-identical to the grid-5 set: {same}")


# ---- g. engine and API --------------------------------------------------------------------------
def _data(n_sub=None):
    g = np.load(os.path.join(GOLDEN, "gt_bach_1s.npz"))
    t, y = g["coords"].reshape(-1, 1), g["target"]
    if n_sub:
        idx = np.arange(0, 44100, 44100 // n_sub)[:n_sub]
        t, y = t[idx], y[idx]
    return t, y


def _kan(widths, G, seed=0):
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(seed)
    return KAN(widths, grid_size=G)


def _engine_grads(eng):
    return {k: v.detach().cpu().numpy() for k, v in zip(eng.layout.names, eng.grad_views())}


def test_engine_step_vs_oracle_and_micro_batches(dev):
    """KanEngine on KAN([1, 16, 16, 1], grid_size=11) over 2 000 coordinates: one step against the
    oracle (which takes its shapes from the state dict), Adam bit-exact against oracle.adam_step on
    the device gradients, and the same step in two micro-batches."""
    from inr_for_audio_amd.engine import KanEngine
    from oracle import siren_oracle as orc
    widths = [1, 16, 16, 1]
    m = _kan(widths, 11)
    sd = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    assert sd["layers.1.spline_weight"].shape == (16, 16, 14) and sd["layers.0.grid"].shape == (1, 18)
    t, y = _data(2000)
    out, xs = orc.kan_forward(sd, t, 3)
    ref = orc.kan_backward(sd, xs, orc.mse_grad(out, y), 3)
    for mb in (1 << 20, 1000):
        mm = _kan(widths, 11)
        mm.load_state_dict(m.state_dict())
        eng = KanEngine(mm, torch.from_numpy(t), torch.from_numpy(y), micro_batch=mb, device=dev)
        assert eng.net.grid_size == 11 and eng.n_micro == (1 if mb > 2000 else 2)
        eng.step()
        torch.cuda.synchronize()
        got = _engine_grads(eng)
        assert set(ref) == set(got)
        for k, r in ref.items():
            rel = np.linalg.norm(got[k].reshape(r.shape) - r) / np.linalg.norm(r)
            assert rel < 1e-4, (mb, k, rel)
        assert abs(eng.last_loss() - orc.mse(out, y)) < 1e-5 * orc.mse(out, y)
        for i, k in enumerate(eng.layout.names):
            p1, _, _ = orc.adam_step(sd[k].astype(np.float32), got[k], np.zeros_like(sd[k]), np.zeros_like(sd[k]), 1, 1e-3)
            assert np.array_equal(eng.layout.view(eng.params, i).cpu().numpy(), p1), (mb, k)


def test_engine_graph_replay_is_the_eager_step(dev):
    from inr_for_audio_amd.engine import KanEngine
    t, y = _data(2000)
    ma, mb = _kan([1, 16, 16, 1], 11), _kan([1, 16, 16, 1], 11)
    mb.load_state_dict(ma.state_dict())
    a = KanEngine(ma, torch.from_numpy(t), torch.from_numpy(y), device=dev)
    for _ in range(4):
        a.step()
    b = KanEngine(mb, torch.from_numpy(t), torch.from_numpy(y), device=dev)
    b.capture_graph()
    for _ in range(4):
        b.step()
    assert torch.equal(a.params, b.params)
    (la, ra), (lb, rb) = a.history(), b.history()
    assert len(la) == 4 and np.array_equal(la, lb) and np.array_equal(ra, rb)
    with pytest.raises(NotImplementedError, match="checked against the reference at grid_size=5 only"):
        a.update_grid()


def test_capture_before_any_step_at_the_largest_tables(dev):
    """KAN([1, 64, 64, 1], grid_size=64): the head pass takes 159 504 B of dynamic LDS, and with no
    step before capture_graph() its first launch is the captured one.  Replay equals eager bit for bit."""
    from inr_for_audio_amd.engine import KanEngine
    t, y = _data(1000)
    ma, mb = _kan([1, 64, 64, 1], 64), _kan([1, 64, 64, 1], 64)
    mb.load_state_dict(ma.state_dict())
    b = KanEngine(mb, torch.from_numpy(t), torch.from_numpy(y), device=dev)
    b.capture_graph()
    for _ in range(2):
        b.step()
    a = KanEngine(ma, torch.from_numpy(t), torch.from_numpy(y), device=dev)
    for _ in range(2):
        a.step()
    assert torch.equal(a.params, b.params) and np.array_equal(a.history()[0], b.history()[0])
    assert np.all(np.isfinite(a.history()[0]))


def test_module_forward_and_autograd(dev):
    """KAN(grid_size=6) as a module: inference and loss.backward() against the oracle."""
    from oracle import siren_oracle as orc
    m = _kan([1, 12, 20, 1], 6)
    sd = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    t, y = _data(1500)
    m = m.to(dev)
    x = torch.from_numpy(t).to(dev).reshape(1, -1, 1)
    with torch.no_grad():
        inf = m(x).cpu().numpy().reshape(-1)
    ref_out, xs = orc.kan_forward(sd, t, 3)
    assert np.max(np.abs(inf - ref_out)) < 1e-5 * max(1.0, np.max(np.abs(ref_out)))
    loss = torch.nn.MSELoss()(m(x), torch.from_numpy(y).to(dev).reshape(1, -1, 1))
    loss.backward()
    ref = orc.kan_backward(sd, xs, orc.mse_grad(ref_out, y), 3)
    for k, p in m.named_parameters():
        r = ref[k]
        rel = np.linalg.norm(p.grad.cpu().numpy().reshape(r.shape) - r) / np.linalg.norm(r)
        assert rel < 1e-4, (k, rel)
    with pytest.raises(NotImplementedError, match="checked against the reference at grid_size=5 only"):
        m(x, update_grid=True)


def test_train_with_a_grid_size_and_resume(dev, tmp_path):
    from scipy.io import wavfile

    from inr_for_audio_amd.run import train
    g = np.load(os.path.join(GOLDEN, "gt_bach_1s.npz"))
    wav = tmp_path / "clip.wav"
    wavfile.write(wav, int(g["fs"]), g["raw"])
    kw = dict(arch="kan", num_hidden_features=16, total_steps=3, filename=str(wav), seed=0, kan_grid_size=11)
    ckpt = train(str(tmp_path), "k", "clip", 1, **kw)
    folder = os.path.dirname(ckpt)
    params = json.load(open(os.path.join(folder, "parameters.json")))
    assert params["kan_grid_size"] == 11 and np.isfinite(params["SNR"])
    sd = torch.load(ckpt, weights_only=True)["model_state_dict"]
    assert tuple(sd["layers.0.spline_weight"].shape) == (16, 1, 14) and tuple(sd["layers.1.grid"].shape) == (16, 18)
    again = train(str(tmp_path), "k2", "clip", 1, prev_ckpt_path=ckpt, **kw)
    assert tuple(torch.load(again, weights_only=True)["model_state_dict"]["layers.2.spline_weight"].shape) == (1, 16, 14)
    with pytest.raises(RuntimeError, match="size mismatch"):
        train(str(tmp_path), "k3", "clip", 1, prev_ckpt_path=ckpt, **{**kw, "kan_grid_size": 4})


@pytest.mark.parametrize("G", [4, 11])
def test_fit_tracks_reference(dev, G):
    """30 full-batch MSE steps of KAN([1, 16, 16, 1], grid_size=G) on gt_bach 1 s from the reference's
    own init (tests/golden/kan_grids_init.npz) against the reference's own loop
    (trajectory_kan_grids.json): every loss within 1e-3 relative, the learning rates equal -- the gate
    of test_gpu_kan.py::test_kan_fit_tracks_reference.  The reference's own two-half-batch loop moves
    its losses by `spread` (recorded beside them)."""
    from inr_for_audio_amd.engine import KanEngine
    tr = json.load(open(os.path.join(GOLDEN, "trajectory_kan_grids.json")))
    init = np.load(os.path.join(GOLDEN, "kan_grids_init.npz"))
    m = _kan(tr["widths"], G, tr["seed"])
    m.load_state_dict({k: torch.from_numpy(init[f"g{G}_{k}"]) for k in m.state_dict()})
    t, y = _data()
    eng = KanEngine(m, torch.from_numpy(t), torch.from_numpy(y), device=dev)
    for _ in range(tr["steps"]):
        eng.step()
    losses, lrs = eng.history()
    ref = np.array(tr["grids"][str(G)]["loss"])
    print(f"G {G}: worst relative loss error {np.max(np.abs(losses - ref) / ref):.3g} (gate 1e-3; "
          f"reference spread {tr['grids'][str(G)]['spread']:.3g})")
    assert np.max(np.abs(losses - ref) / ref) < 1e-3, (losses[:5], ref[:5])
    assert np.array_equal(lrs, np.array(tr["grids"][str(G)]["lr"]))
