"""Each kernel of csrc/kan.hip through the C-ABI (siren_kan_forward / _backward / _train_step, driven
as kan.py's _KanFunction drives them) against tests/kan_ref.py: fp64, element by element, on
per-input non-uniform knots (kan_ref.kan_knots -- no two inputs share a knot row and no two gaps of
a row are equal, so a wrong knot row, reciprocal slot or il / ir swap changes the values).

A single-layer net selects the kernel by shape (capi.hip kan_run_forward / kan_run_backward):
  kan_head_fwd    L = 1, out = 1, in <= 64, forward        kan_fwd_fused   any other forward
  kan_bwd_fused   backward, out <= 64, grad_coords given   kan_dw_fused    backward, grad_coords NULL
  kan_dw_fused + kan_dx_fused   backward, out > 64, grad_coords given
  kan_head_train  siren_kan_train_step, L = 2, width[1] <= 64, last width 1
Loader / store variants and the cases that reach them ((in, out, rows, splits) below):
  kan_fwd_fused  vec (in % 16 == 0: register-prefetched float4 W and X, float4 kf_put_pair): (16, 64),
                 (32, 128) two chunks i0 = 16, (64, 16), (16, 128) bit-exact; scalar loaders with
                 float4 kf_put_pair stores (ic & 3 == 0): (8, 64), (20, 48) both chunks; scalar
                 stores (ic & 3 != 0): (1, 16), (3, 5), (18, 70) second chunk ic = 2, (3, 24) and
                 (18, 144) bit-exact; out tiles 64 + 6: (18, 70), 64 + 64 + 16: (18, 144)
  kan_head_fwd   in = 1, 3, 64 (the last lane); bit-exact at in = 3 and 64
  kan_bwd_fused  vec (ic == 16, in % 4 == 0, out == 64): (16, 64), (32, 64); the first chunk of
                 (20, 64) vec and its tail chunk ic = 4 scalar; scalar: the rest; kf_stage_x float4
                 (full chunk, in % 4 == 0, out != 64): (16, 16); one tile, several tiles and a
                 ragged last split: 2100 rows at 16 splits (11 splits of 192 rows) and at 1 split
  kan_dw_fused   float4 G (out % 4 == 0, full out tile): (16, 64), (32, 128), (8, 128), (20, 48) not
                 (48 < 64: scalar); scalar G: (3, 5), (18, 70) second out tile of 6, (1, 16);
                 kf_stage_x float4: in = 16, 32; scalar: in = 1, 3, 8, 18, 20 tail, 64 with out 1
  kan_dx_fused   vec G and W^T (out % 4 == 0, full out tile, full chunk): (16, 128), (32, 128);
                 vec G with scalar W^T: (3, 128), (20, 128) tail chunk; scalar both: (1, 70), (18, 70),
                 (64, 70); derivative values at (16, 128) and (18, 144)
  kan_slab_reduce_kernel<16> (more than 64 slabs, under 16 384 columns): test_slab_reduce_16
  kan_slab_reduce_kernel<64>: every other backward case
Bounds: 1e-5 * sum|terms| + 1e-12 per element (the suite's fp32-summation bound, test_gpu_kernels.py);
the basis derivative as a value within kan_ref.DERIV_C = 28 units of 2^-24 * scale' (4 x the fp32
IEEE-division oracle's own measured error of 6.66, tests/test_kan_host.py); the forward bases bit
for bit against torch's CPU recursion (tests/test_kan_host.py checks on the host that kan_div is
the IEEE quotient on these knots and inputs).  The workspace starts NaN-filled, so a read of a slab
row or tile no kernel wrote shows."""
import ctypes

import numpy as np
import pytest
import torch

import kan_ref as kr

pytestmark = pytest.mark.gpu
F32 = np.float32


def _al(v):
    return (v + 63) // 64 * 64


def ws_layout(widths, rows, splits):
    """capi.hip kan_layout restated: float offsets of the pieces the tests read (X[l], G[0]) and
    the total, which must equal siren_kan_workspace_floats."""
    L = len(widths) - 1
    off, wk = 0, 1
    for l in range(L):
        kw = widths[l + 1] * 9 * widths[l]
        off += 2 * _al(kw)
        wk = max(wk, kw)
    X = {}
    for l in range(1, L + 1):
        X[l] = off
        off += _al(rows * widths[l])
    off += _al(wk)
    slab = wk * splits
    for l in range(L):
        if widths[l + 1] == 1:
            slab = max(slab, 4 * splits * 9 * widths[l])
    off += _al(slab)
    wmax = max(widths[:L])
    G0 = off
    off += 2 * _al(rows * wmax) + 3 * _al((rows + 255) // 256) + _al(1)
    return X, G0, off


class Net:
    """A KANLinear stack on the device, with the C-ABI structs; layers = [(grid, bw, sw, sc), ...]
    as fp32 numpy arrays."""

    def __init__(self, lib, dev, widths, layers):
        from inr_for_audio_amd._lib import SirenKanGrads, SirenKanNet, ptr
        self.lib, self.dev, self.widths, self.L = lib, dev, list(widths), len(layers)
        self.p = [[torch.from_numpy(np.ascontiguousarray(a, F32)).to(dev) for a in lay] for lay in layers]
        self.net = SirenKanNet()
        self.net.n_layers = self.L
        for l, w in enumerate(widths):
            self.net.width[l] = w
        sizes = []
        for l, (g, bw, sw, sc) in enumerate(self.p):
            assert g.shape == (widths[l], 12) and bw.shape == (widths[l + 1], widths[l])
            assert sw.shape == (widths[l + 1], widths[l], 8) and sc.shape == bw.shape
            n = self.net
            n.grid[l], n.base_w[l], n.spline_w[l], n.scaler[l] = (ptr(t) for t in (g, bw, sw, sc))
            sizes += [bw.numel(), sw.numel(), sc.numel()]
        # one flat gradient vector (+ the squared-error slot), viewed per parameter
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
        self.X_off, self.G0_off, total = ws_layout(self.widths, rows, splits)
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

    def train_step(self):
        from inr_for_audio_amd._lib import check
        check(self.lib.siren_kan_train_step(ctypes.byref(self.net), ctypes.byref(self.gr), ctypes.byref(self.b),
                                            self._stream()), "siren_kan_train_step")
        torch.cuda.synchronize()
        return self.out.cpu().numpy().reshape(-1), self.g.cpu().numpy().reshape(-1)

    def grads(self):
        names = ("base_weight", "spline_weight", "spline_scaler")
        return [{nm: self.views[3 * l + k].cpu().numpy().reshape(self.p[l][1 + k].shape) for k, nm in enumerate(names)}
                for l in range(self.L)]

    def ws_piece(self, off, shape):
        return self.ws[off:off + int(np.prod(shape))].cpu().numpy().reshape(shape)


def _inputs(grid, rows, seed=0):
    """rows probe inputs: with room, uniform draws, every knot and its two neighbours, +-0, +-1e-30."""
    if rows >= 40:
        return kr.probe_inputs(grid, rows - 40, seed)
    return kr.probe_inputs(grid, 24, seed)[-(rows + 8):][:rows]


def _weights(fin, fout, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(fout, fin)).astype(F32), rng.normal(size=(fout, fin, 8)).astype(F32),
            rng.normal(size=(fout, fin)).astype(F32))


def _one_hot_layer(fin):
    """out = 8 in, base_weight 0, spline_scaler 1, spline_weight[o(i, c)][i][c] = 1 with o(i, c) = 8 i + c."""
    fout = 8 * fin
    sw = np.zeros((fout, fin, 8), F32)
    for i in range(fin):
        for c in range(8):
            sw[8 * i + c, i, c] = 1.0
    return np.zeros((fout, fin), F32), sw, np.ones((fout, fin), F32)


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


# ---- a. forward bases, bit for bit ------------------------------------------------------------
def _torch_bases(x, grid):
    from inr_for_audio_amd.kan import bspline_bases
    return bspline_bases(torch.from_numpy(x), torch.from_numpy(grid), 3).numpy()


@pytest.mark.parametrize("fin", [16, 18, 3])
def test_fused_forward_bases_bit_exact(lib, dev, fin):
    """kan_fwd_fused (count-and-gather window, kf_put_pair's float4 and scalar stores, the vec and
    scalar W loaders, out tiles 64 + 64 (+ 16)): with base_weight 0, spline_scaler 1 and a one-hot
    spline_weight of 8 in outputs, output column 8 i + c is B_c(x_i) bit for bit as torch's CPU
    recursion (kan.bspline_bases) gives it -- every other product the MFMA chain adds is an exact 0."""
    grid = kr.kan_knots(fin, 20 + fin)
    x = kr.probe_inputs(grid, 2060, fin)
    out = Net(lib, dev, [fin, 8 * fin], [(grid, *_one_hot_layer(fin))]).bind(x, 1).forward()
    ref = _torch_bases(x, grid).reshape(x.shape[0], -1)
    bad = np.argwhere(out != ref)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), out[tuple(bad[:5].T)], ref[tuple(bad[:5].T)])


@pytest.mark.parametrize("fin,lanes", [(3, (0, 1, 2)), (64, (0, 17, 31, 32, 63))])
def test_head_forward_bases_bit_exact(lib, dev, fin, lanes):
    """kan_head_fwd (select window, lane = input) on non-uniform per-input knots: out = 1 and a
    one-hot spline_weight at (i, c) output exactly B_c(x_i), for every basis of the listed lanes."""
    grid = kr.kan_knots(fin, 30 + fin)
    x = kr.probe_inputs(grid, 660, fin)
    ref = _torch_bases(x, grid)
    net = Net(lib, dev, [fin, 1], [(grid, np.zeros((1, fin), F32), np.zeros((1, fin, 8), F32), np.ones((1, fin), F32))])
    net.bind(x, 1)
    sw = net.p[0][2]
    for i in lanes:
        for c in range(8):
            sw.zero_()
            sw[0, i, c] = 1.0
            out = net.forward().reshape(-1)
            bad = np.flatnonzero(out != ref[:, i, c])
            assert bad.size == 0, (i, c, bad[:5], x[bad[:5], i], out[bad[:5]], ref[bad[:5], i, c])


# ---- b. forward against fp64, per element -----------------------------------------------------
FWD_CASES = [(1, 1, 1), (3, 1, 65), (64, 1, 700),                              # kan_head_fwd
             (1, 16, 63), (3, 5, 64), (8, 64, 65), (16, 64, 700), (18, 70, 2100), (20, 48, 700),
             (32, 128, 2100), (64, 16, 1), (16, 128, 65), (1, 70, 1)]          # kan_fwd_fused


@pytest.mark.parametrize("fin,fout,rows", FWD_CASES)
def test_forward_vs_fp64(lib, dev, fin, fout, rows):
    grid = kr.kan_knots(fin, 100 + fin)
    x = _inputs(grid, rows, fout)
    w = _weights(fin, fout, 7 * fin + fout)
    out = Net(lib, dev, [fin, fout], [(grid, *w)]).bind(x, 1).forward()
    _close(out, kr.layer(x, grid, *w)["out"], "out")


# ---- c. the basis derivative as a value -------------------------------------------------------
def _deriv_gate(dx, x, grid, basis_of_row, what):
    """dx[n][i] must be B'_{basis_of_row[n]}(x[n][i]) within DERIV_C * 2^-24 * scale', and exactly
    0 where x[n][i] lies outside input i's knot range."""
    _, db, _, sdb = kr.bases64(x, grid)
    idx = np.asarray(basis_of_row)[:, None, None]
    ref = np.take_along_axis(db, np.broadcast_to(idx, db.shape[:2] + (1,)), 2)[..., 0]
    scale = np.take_along_axis(sdb, np.broadcast_to(idx, db.shape[:2] + (1,)), 2)[..., 0]
    lim = kr.DERIV_C * 2.0 ** -24 * scale
    err = np.abs(dx.astype(np.float64) - ref)
    worst = np.max(err[scale > 0] / (2.0 ** -24 * scale[scale > 0]), initial=0.0)
    print(f"{what}: worst B' error {worst:.2f} x 2^-24 scale' (gate {kr.DERIV_C:g})")
    bad = np.argwhere(~(err <= lim))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), dx[tuple(bad[:4].T)], ref[tuple(bad[:4].T)])
    assert np.all(dx[kr.outside(x, grid)] == 0), what


@pytest.mark.parametrize("fin,kernel", [(8, "kan_bwd_fused"), (16, "kan_dx_fused"), (18, "kan_dx_fused")])
def test_basis_derivative_value_fused(lib, dev, fin, kernel):
    """B' as the kernel computed it (v_rcp_f32 quotients), one value per element of dX: one-hot
    combined weight with an output per (input, basis) pair, G[n][o(i, c)] = (c == n % 8), each probe
    input repeated over 8 rows, so dX[n][i] = B'_{n % 8}(x[n][i]) -- selection by 1 and 0 is exact
    through both MFMA chains and the contraction.
    Gate: kan_ref.DERIV_C = 28 units of 2^-24 * scale' = 4 x 7, the fp32 IEEE-division oracle's own
    error against bases64 (measured on the host, tests/test_kan_host.py: 7.94 units for B, 6.66 for
    B', rounded up to 8 and 7).  Measured on an MI355X: 5.04 (kan_bwd_fused), 5.23 and 5.83
    (kan_dx_fused at in = 16 and 18); kan_head_train below, on IEEE quotients: 4.09."""
    grid = kr.kan_knots(fin, 40 + fin)
    x = np.repeat(kr.probe_inputs(grid, 220, fin), 8, axis=0)
    rows, fout = x.shape[0], 8 * fin
    c_of = np.arange(rows) % 8
    G = np.zeros((rows, fout), F32)
    for i in range(fin):
        G[np.arange(rows), 8 * i + c_of] = 1.0
    net = Net(lib, dev, [fin, fout], [(grid, *_one_hot_layer(fin))]).bind(x, 4)
    assert (fout <= 64) == (kernel == "kan_bwd_fused")
    net.forward()
    _, dx = net.backward(G, True)
    _deriv_gate(dx, x, grid, c_of, kernel)


def _scaled_first_layer(h, seed, flip):
    """Layer 0 of a [1, h, 1] net that hands t >= 18 to lane i as t * s_i exactly, s_i = +-2^-6
    (even lanes positive, odd negative; the other way round with flip):
    t is outside layer 0's knot range (every basis an exact 0) and SiLU(t) = t / (1 + exp(-t)) = t
    in fp32 there, so X[1][n][i] = RN(t_n s_i) = t_n s_i."""
    g0 = kr.kan_knots(1, seed)
    assert g0.max() < 17
    s = np.where(np.arange(h) % 2 == int(flip), 1.0, -1.0).astype(F32) * F32(2.0 ** -6)
    _, sw, sc = _weights(1, h, seed)
    return (g0, s.reshape(h, 1), sw, sc), s


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("h,lanes", [(3, (0, 1, 2)), (64, (0, 17, 63))])
def test_basis_derivative_value_head_train(lib, dev, h, lanes, flip):
    """kan_head_train's B' (IEEE quotients through kan_div) as a value: [1, h, 1] with the last
    layer's weight one-hot at (i, c), targets -2^25 and n_total = 2, so g = 2^25 exactly for every
    row and the kernel's Gin[n][i] = 2^25 B'_c(X[1][n][i]).  Layer 0 scales the coordinates by
    +-2^-6 exactly, so lane i meets its own knots and their one-ulp neighbours (those of its sign
    with |knot| >= 18 / 64; the other sign with flip) as well as points inside and outside its
    range.  A basis whose support a lane's sign never reaches prints 0.00 and checks the exact 0."""
    lay0, s = _scaled_first_layer(h, 50 + h, flip)
    g1 = kr.kan_knots(h, 60 + h)
    p = kr.probe_inputs(g1, 60, h)
    t = np.concatenate([64.0 * np.abs(p[:, i][(np.sign(p[:, i]) == np.sign(s[i])) & (np.abs(p[:, i]) >= 18 / 64)])
                        for i in lanes]).astype(F32).reshape(-1, 1)
    rows = t.shape[0]
    x1 = t * s[None, :]
    hit = sum(int(np.sum(x1[:, i][:, None] == g1[i][None, :])) for i in lanes)
    assert hit >= 3 * len(lanes), hit     # the lanes do meet knots of their own
    net = Net(lib, dev, [1, h, 1], [lay0, (g1, np.zeros((1, h), F32), np.zeros((1, h, 8), F32), np.ones((1, h), F32))])
    net.bind(t, 2, target=np.full(rows, -2.0 ** 25, F32), n_valid=rows, n_total=2.0)
    sw = net.p[1][2]
    for i in lanes:
        for c in range(8):
            sw.zero_()
            sw[0, i, c] = 1.0
            _, g = net.train_step()
            assert np.array_equal(net.ws_piece(net.X_off[1], (rows, h)), x1)
            assert np.all(g == F32(2.0 ** 25))
            gin = net.ws_piece(net.G0_off, (rows, h))
            others = np.delete(np.arange(h), i)
            assert np.all(gin[:, others] == 0)
            _deriv_gate(gin[:, i:i + 1] * F32(2.0 ** -25), x1[:, i:i + 1], g1[i:i + 1], np.full(rows, c),
                        f"kan_head_train lane {i} basis {c}")


# ---- d. gradients against fp64, per element ---------------------------------------------------
BWD_CASES = [
    # kan_bwd_fused (out <= 64, grad_coords given)
    (1, 1, 1, 1, True), (3, 5, 63, 1, True), (8, 16, 64, 1, True), (16, 64, 700, 3, True), (32, 64, 2100, 16, True),
    (18, 48, 2100, 1, True), (20, 64, 65, 1, True), (64, 1, 700, 2, True), (16, 16, 2100, 16, True),
    # kan_dw_fused + kan_dx_fused (out > 64, grad_coords given)
    (1, 70, 1, 1, True), (3, 128, 63, 1, True), (16, 128, 700, 3, True), (18, 70, 2100, 16, True),
    (20, 128, 65, 1, True), (32, 128, 2100, 1, True), (64, 70, 64, 2, True),
    # kan_dw_fused alone (grad_coords NULL)
    (1, 16, 2100, 16, False), (3, 5, 65, 1, False), (16, 64, 700, 3, False), (18, 70, 2100, 1, False),
    (32, 128, 64, 1, False), (20, 48, 1, 1, False), (64, 1, 63, 1, False), (8, 128, 2100, 16, False),
]


def _layer_case(lib, dev, fin, fout, rows, splits, seed=0):
    grid = kr.kan_knots(fin, 200 + fin + seed)
    x = _inputs(grid, rows, fout + seed)
    w = _weights(fin, fout, 3 * fin + fout + seed)
    G = np.random.default_rng(rows + fout).normal(size=(rows, fout)).astype(F32)
    return grid, x, w, G, Net(lib, dev, [fin, fout], [(grid, *w)]).bind(x, splits)


@pytest.mark.parametrize("fin,fout,rows,splits,want_dx", BWD_CASES)
def test_backward_vs_fp64(lib, dev, fin, fout, rows, splits, want_dx):
    grid, x, w, G, net = _layer_case(lib, dev, fin, fout, rows, splits)
    net.forward()
    grads, dx = net.backward(G, want_dx)
    ref = kr.layer(x, grid, *w, G)
    _check_grads(grads[0], ref, "grad")
    if want_dx:
        _close(dx, ref["dX"], "dX")


@pytest.mark.parametrize("fin,fout,want_dx", [(18, 48, True), (18, 70, True), (18, 70, False)])
def test_backward_accumulates_and_zero_grads(lib, dev, fin, fout, want_dx):
    """A second backward into the same buffers without zero_grads gives twice the reference; with
    zero_grads and `flat` set, NaN-filled gradient buffers are cleared first."""
    grid, x, w, G, net = _layer_case(lib, dev, fin, fout, 700, 3, seed=1)
    ref = kr.layer(x, grid, *w, G)
    net.forward()
    net.backward(G, want_dx)
    grads, dx = net.backward(G, want_dx)
    _check_grads(grads[0], ref, "twice", scale=2.0)
    if want_dx:
        _close(dx, ref["dX"], "dX (not accumulated)")
    net.flat.fill_(float("nan"))
    net.b.zero_grads = 1
    grads, _ = net.backward(G, want_dx)
    _check_grads(grads[0], ref, "zero_grads")


@pytest.mark.parametrize("fin,fout", [(3, 1), (18, 48), (18, 70)])
def test_all_inputs_outside_knot_range(lib, dev, fin, fout):
    """Every input of every row outside its knot range and base_weight 0: out, dX, d spline_weight
    and d spline_scaler are exactly 0 (kan_head_fwd / kan_fwd_fused, kan_bwd_fused, kan_dw_fused +
    kan_dx_fused)."""
    rows = 700
    grid = kr.kan_knots(fin, 300 + fin)
    rng = np.random.default_rng(fout)
    d = rng.uniform(0.0, 2.0, (rows, fin)).astype(F32)
    x = np.where(rng.random((rows, fin)) < 0.5, grid[None, :, -1] + d, np.nextafter(grid[None, :, 0], F32(-np.inf)) - d)
    x = x.astype(F32)
    x[:12] = grid[:, -1][None]     # at the last knot: outside
    assert kr.outside(x, grid).all()
    _, sw, sc = _weights(fin, fout, 9)
    G = rng.normal(size=(rows, fout)).astype(F32)
    net = Net(lib, dev, [fin, fout], [(grid, np.zeros((fout, fin), F32), sw, sc)]).bind(x, 3)
    out = net.forward()
    grads, dx = net.backward(G, True)
    assert np.all(out == 0) and np.all(dx == 0)
    assert np.all(grads[0]["spline_weight"] == 0) and np.all(grads[0]["spline_scaler"] == 0)
    ref = kr.layer(x, grid, np.zeros((fout, fin), F32), sw, sc, G)
    _close(grads[0]["base_weight"], ref["base_weight"], "d base_weight")


# ---- e. kan_head_train against the unfused route -----------------------------------------------
def _two_layer(lib, dev, h, rows, splits, seed):
    g0, g1 = kr.kan_knots(1, 400 + seed), kr.kan_knots(h, 500 + seed)
    w0, w1 = _weights(1, h, seed), _weights(h, 1, seed + 1)
    t = _inputs(g0, rows, seed)
    y = np.random.default_rng(seed).normal(size=rows).astype(F32)
    return (g0, g1, w0, w1, t, y), lambda: Net(lib, dev, [1, h, 1], [(g0, *w0), (g1, *w1)])


def _check_two_layer(net, data, out, g, grads, what):
    """out, Gin and every gradient of a [1, h, 1] step against kan_ref, stage by stage: each
    stage's reference starts from the fp32 arrays the device handed it (X[1], g, Gin)."""
    g0, g1, w0, w1, t, _ = data
    rows, h = t.shape[0], g1.shape[0]
    x1 = net.ws_piece(net.X_off[1], (rows, h))
    _close(x1, kr.layer(t, g0, *w0)["out"], f"{what} X[1]")
    r1 = kr.layer(x1, g1, *w1, g.reshape(rows, 1))
    _close(out, r1["out"], f"{what} out")
    _check_grads(grads[1], r1, f"{what} layer 1")
    gin = net.ws_piece(net.G0_off, (rows, h))
    _close(gin, r1["dX"], f"{what} Gin")
    _check_grads(grads[0], kr.layer(t, g0, *w0, gin), f"{what} layer 0")
    return r1


@pytest.mark.parametrize("h,rows,n_valid",
                         [(3, 700, 650), (20, 700, 650), (64, 700, 650), (20, 700, 700), (20, 700, 0)])
def test_head_train_vs_unfused_route(lib, dev, h, rows, n_valid):
    """Route A: siren_kan_train_step (kan_fwd_fused, kan_head_train, kan_dw_fused).  Route B:
    siren_kan_forward (kan_fwd_fused, kan_head_fwd), then siren_kan_backward on route A's g
    (kan_bwd_fused for the last layer, kan_dw_fused for the first).  out is bit-identical; g is
    (out - y) * fp32(2 / n_total) in fp32 below n_valid and 0 from there on (those targets are
    NaN); the squared error and every gradient of both routes agree with kan_ref per element."""
    n_total = 1234.0
    data, make = _two_layer(lib, dev, h, rows, 3, h)
    t, y = data[4], data[5].copy()
    y[n_valid:] = np.nan
    a = make().bind(t, 3, target=y, n_valid=n_valid, n_total=n_total)
    a.flat.fill_(float("nan"))
    a.b.zero_grads = 1
    out_a, g_a = a.train_step()
    grads_a, sse = a.grads(), float(a.sse.cpu())
    b = make().bind(t, 3)
    out_b = b.forward().reshape(-1)
    grads_b, _ = b.backward(g_a, False)
    assert np.array_equal(out_a, out_b)
    g_ref = np.zeros(rows, F32)
    g_ref[:n_valid] = (out_a[:n_valid] - y[:n_valid]) * F32(2.0 / n_total)
    assert np.array_equal(g_a, g_ref)
    sse_ref = float(np.sum((out_a[:n_valid].astype(np.float64) - y[:n_valid]) ** 2))
    assert abs(sse - sse_ref) <= 1e-5 * sse_ref, (sse, sse_ref)
    r1 = _check_two_layer(a, data, out_a, g_a, grads_a, "A")
    _check_two_layer(b, data, out_b, g_a, grads_b, "B")
    for l in range(2):
        for nm in grads_a[l]:
            if l == 1:  # the same upstream g on both routes: one bound on the difference
                diff = np.abs(grads_a[l][nm].astype(np.float64) - grads_b[l][nm])
                assert np.all(diff <= 1e-5 * r1[nm][1] + 1e-12), nm
            if n_valid == 0:
                assert np.all(grads_a[l][nm] == 0) and np.all(grads_b[l][nm] == 0), nm


# ---- f. kan_slab_reduce_kernel<16> ------------------------------------------------------------
@pytest.mark.parametrize("want_dx", [False, True])
def test_slab_reduce_16_via_layer_backward(lib, dev, want_dx):
    """[1 -> 16], 4161 rows, 66 splits: 66 one-tile slabs of 144 columns (more than 64 slabs, under
    16 384 columns), through kan_dw_fused (grad_coords NULL) and kan_bwd_fused."""
    grid, x, w, G, net = _layer_case(lib, dev, 1, 16, 4161, 66, seed=2)
    net.forward()
    grads, dx = net.backward(G, want_dx)
    ref = kr.layer(x, grid, *w, G)
    _check_grads(grads[0], ref, "grad")
    if want_dx:
        _close(dx, ref["dX"], "dX")


def test_slab_reduce_16_via_head_train(lib, dev):
    """[1, 8, 1], 16 700 rows, splits 17: kan_head_train runs 66 blocks of 254 rows (slab room
    4 * 17 = 68 rows of 72 columns)."""
    rows = 16700
    data, make = _two_layer(lib, dev, 8, rows, 17, 8)
    net = make().bind(data[4], 17, target=data[5], n_valid=rows, n_total=float(rows))
    out, g = net.train_step()
    _check_two_layer(net, data, out, g, net.grads(), "A")
