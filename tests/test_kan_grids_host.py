"""The KAN at grid sizes other than 5, on the host: the numerics the any-grid-size kernels
(csrc/kan_general.hip) rest on, checked on the knot family the GPU tests use
(kan_grids_ref.kan_knots_g), and the host side of the interface: what the modules accept and refuse,
the net struct's grid_size, the workspace layout and the C-ABI's validation."""
import ctypes

import numpy as np
import pytest
import torch

import kan_grids_ref as kg
from oracle import siren_oracle as orc

F32 = np.float32
PROBE_FIN, PROBE_N = 6, 20000


def _probe(G):
    g = kg.kan_knots_g(PROBE_FIN, G, 11 + G)
    return g, kg.probe_inputs(g, PROBE_N, G)


@pytest.mark.parametrize("G", kg.GRIDS)
def test_oracle_error_zero_outside_and_four_bases(G):
    """oracle.siren_oracle.kan_bases (fp32, IEEE divisions, kan.py's op order) against bases64 on
    kan_knots_g grids, in units of 2^-24 * scale: under the bounds recorded for grid 5
    (kan_ref.ORACLE_ERR_B = 8, ORACLE_ERR_DB = 7), which the GPU gate DERIV_C = 4 x 7 rests on.
    Exact zeros where the scale is 0 (outside the knot range), and at most 4 non-zero bases a row:
    the window the kernels keep in registers is the whole row."""
    g, x = _probe(G)
    assert g.shape == (PROBE_FIN, G + 7)
    b32, db32 = orc.kan_bases(x, g, deriv=True)
    assert b32.shape == x.shape + (G + 3,)
    b, db, sb, sdb = kg.bases64(x, g)
    u = 2.0 ** -24
    out = kg.outside(x, g)
    for v32, v64, s in ((b32, b, sb), (db32, db, sdb)):
        assert np.all(v32[s == 0] == 0) and np.all(v64[s == 0] == 0)
    assert np.all(b32[out] == 0) and np.all(db32[out] == 0)
    assert np.max((b32 != 0).sum(-1)) <= 4 and np.max((db32 != 0).sum(-1)) <= 4
    assert np.max((b != 0).sum(-1)) <= 4
    eb = np.max(np.abs(b32 - b)[sb > 0] / (u * sb[sb > 0]))
    ed = np.max(np.abs(db32 - db)[sdb > 0] / (u * sdb[sdb > 0]))
    print(f"G = {G}: oracle error in 2^-24 * scale: B {eb:.2f}  B' {ed:.2f}")
    assert eb <= kg.ORACLE_ERR_B and ed <= kg.ORACLE_ERR_DB, (G, eb, ed)


@pytest.mark.parametrize("G", kg.GRIDS)
def test_kan_div_is_the_ieee_quotient_on_these_grids(G):
    """kan_div (reciprocal, product, two fmas) equals the fp32 quotient on every quotient the
    recursion forms on these knots and probe inputs: the forward's bit-exactness carries over."""
    g = kg.kan_knots_g(PROBE_FIN, G, 11 + G)
    a, d = kg.recursion_quotients(kg.probe_inputs(g, 1500, G), g)
    got, ref = kg.kan_div_emulated(a, d), a / d
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (G, bad.size, a[bad[:3]], d[bad[:3]], got[bad[:3]], ref[bad[:3]])


def test_span_by_bisection_equals_span_predicate():
    """kan_bases_window's KAN_SPAN_BISECT span: bisection for the first knot above x on non-decreasing knots gives
    #{j : g[j] <= x}, so s = count - 1 (count 1 .. NG - 1) is the span of the predicate
    g[j] <= x < g[j+1] -- on, beside and outside the knots, with repeated knots, +-inf and NaN."""
    rng = np.random.default_rng(0)
    for ng in (8, 9, 12, 18, 71):
        for rep in range(6):
            g = np.sort(rng.normal(size=ng).astype(F32))
            if rep % 2:
                k = int(rng.integers(0, ng - 1))
                g[k + 1] = g[k]
            xs = np.concatenate([g, np.nextafter(g, F32(np.inf)), np.nextafter(g, F32(-np.inf)),
                                 rng.uniform(g[0] - 1, g[-1] + 1, 100).astype(F32),
                                 np.array([np.inf, -np.inf, np.nan], F32)])
            for x in xs:
                s_pred = -1
                for j in range(ng - 1):
                    if g[j] <= x < g[j + 1]:
                        s_pred = j
                lo, hi = 0, ng
                while lo < hi:
                    mid = (lo + hi) >> 1
                    if x >= g[mid]:
                        lo = mid + 1
                    else:
                        hi = mid
                assert (lo - 1 if 1 <= lo <= ng - 1 else -1) == s_pred, (g, x)


@pytest.mark.parametrize("G,fin,fout", [(1, 3, 5), (11, 4, 3)])
def test_layer_equals_torch_fp64_autograd(G, fin, fout):
    """kan_grids_ref.layer (values) against torch fp64 autograd of kan.py:153-166: 1e-12 relative."""
    from inr_for_audio_amd.kan import bspline_bases
    rng = np.random.default_rng(G)
    g = kg.kan_knots_g(fin, G, 5)
    x = kg.probe_inputs(g, 200)
    n = x.shape[0]
    bw, sw = rng.normal(size=(fout, fin)).astype(F32), rng.normal(size=(fout, fin, G + 3)).astype(F32)
    sc, up = rng.normal(size=(fout, fin)).astype(F32), rng.normal(size=(n, fout)).astype(F32)
    ref = kg.layer(x, g, bw, sw, sc, up)
    t = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in
         {"x": x, "base_weight": bw, "spline_weight": sw, "spline_scaler": sc}.items()}
    bases = bspline_bases(t["x"], torch.from_numpy(g).double(), 3)
    W = t["spline_weight"] * t["spline_scaler"].unsqueeze(-1)
    out = torch.nn.functional.silu(t["x"]) @ t["base_weight"].t() + bases.reshape(n, -1) @ W.reshape(fout, -1).t()
    (out * torch.from_numpy(up).double()).sum().backward()
    got = {"out": out.detach(), "dX": t["x"].grad,
           **{k: t[k].grad for k in ("base_weight", "spline_weight", "spline_scaler")}}
    for k, v in got.items():
        r, terms = ref[k]
        assert r.shape == tuple(v.shape) == terms.shape, k
        assert np.max(np.abs(v.numpy() - r)) <= 1e-12 * max(1.0, np.max(np.abs(r))), k
        assert np.all(terms >= np.abs(r) * (1 - 1e-12)), k


# ---- the interface ----------------------------------------------------------------------------
def test_make_net_carries_the_grid_size():
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(0)
    m = KAN([1, 8, 1], grid_size=11)
    assert m.layers[0].spline_weight.shape == (8, 1, 14) and m.layers[1].grid.shape == (8, 18)
    assert m.make_net().grid_size == 11
    assert KAN([1, 8, 1]).make_net().grid_size == 5
    assert KAN([1, 4, 1], grid_size=1).make_net().grid_size == 1
    assert KAN([1, 4, 1], grid_size=64).make_net().grid_size == 64


def test_what_stays_refused_names_its_limit():
    from inr_for_audio_amd import kan as hk
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError, match="spline_order=3 only"):
        hk.KAN([1, 4, 1], spline_order=2).hip_check()
    with pytest.raises(NotImplementedError, match="grid_size from 1 to 64"):
        hk.KAN([1, 4, 1], grid_size=65).hip_check()
    with pytest.raises(NotImplementedError, match="grid_size from 1 to 64"):
        hk._hip_check_layer(hk.KANLinear(2, 3, grid_size=65))
    with pytest.raises(NotImplementedError, match="spline_order=3 only"):
        hk._hip_check_layer(hk.KANLinear(2, 3, spline_order=2))
    x = torch.zeros(16, 1)
    # update_grid off the default grid: refused before the device is looked at
    with pytest.raises(NotImplementedError, match="checked against the reference at grid_size=5 only"):
        hk.KANLinear(1, 3, grid_size=4).update_grid(x)
    with pytest.raises(NotImplementedError, match="checked against the reference at grid_size=5 only"):
        hk._update_grid_check(11)
    hk._update_grid_check(5)


def test_train_refuses_a_grid_size_without_the_kan(tmp_path):
    from inr_for_audio_amd.run import train
    with pytest.raises(ValueError, match="kan_grid_size"):
        train(str(tmp_path), "t", "bach", 1, arch="mlp", kan_grid_size=8)


def _net(widths, G):
    from inr_for_audio_amd._lib import SirenKanNet
    n = SirenKanNet()
    n.n_layers, n.grid_size = len(widths) - 1, G
    for l, w in enumerate(widths):
        n.width[l] = w
    for l in range(len(widths) - 1):   # never dereferenced on the host
        n.grid[l] = n.base_w[l] = n.spline_w[l] = n.scaler[l] = 64
    return n


@pytest.mark.parametrize("widths,rows,splits", [([1, 64, 64, 1], 5000, 2), ([3, 70], 300, 3), ([64, 1], 300, 2)])
def test_workspace_floats_follow_the_grid_size(lib, widths, rows, splits):
    from inr_for_audio_amd import _lib
    assert _lib.KAN_MAX_GRID == 64
    ws = lambda G: int(lib.siren_kan_workspace_floats(ctypes.byref(_net(widths, G)), rows, splits))  # noqa: E731
    for G in kg.GRIDS + (5,):
        assert ws(G) == kg.workspace_floats(widths, rows, splits, G)[2], G
    # 0 is the default grid: the value a zero-initialised struct got before grid_size existed
    assert ws(0) == ws(5) == kg.workspace_floats(widths, rows, splits, 5)[2]
    assert ws(65) == -1 and ws(-1) == -1


def test_grid_size_is_validated_before_any_launch(lib):
    from inr_for_audio_amd._lib import SirenKanBatch, SirenKanGrads
    for G in (65, -1, 1 << 20):
        net = _net([1, 8, 1], G)
        assert lib.siren_kan_forward(ctypes.byref(net), ctypes.byref(SirenKanBatch()), None) == 1003
        assert lib.siren_kan_train_step(ctypes.byref(net), ctypes.byref(SirenKanGrads()),
                                        ctypes.byref(SirenKanBatch()), None) == 1003
    for G in (0, 1, 5, 64):            # accepted: the next check (NULL batch pointers) answers
        assert lib.siren_kan_forward(ctypes.byref(_net([1, 8, 1], G)), ctypes.byref(SirenKanBatch()), None) == 1002


def test_kan_general_option(lib):
    from inr_for_audio_amd._lib import Opt, options
    assert lib.siren_set_option(Opt.KAN_GENERAL, 2) == 1003 and lib.siren_set_option(Opt.KAN_GENERAL, -1) == 1003
    with options(lib, {Opt.KAN_GENERAL: 1}):
        pass
