"""KAN variant on the host: the module mirror's init and the CPU oracle against
the reference's own numbers (tests/golden/kan_fwd_bwd.npz from /root/reference's kan.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import siren_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def load(name):
    return np.load(os.path.join(G, name))


def _sd(name):
    f = load("kan_fwd_bwd.npz")
    pre = f"{name}_init_"
    return {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}


@pytest.mark.parametrize("name,widths,seed", [("k64", [1, 64, 64, 1], 0), ("k128", [1, 128, 128, 1], 3)])
def test_kan_init_bit_exact(name, widths, seed):
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(seed)
    m = KAN(widths)
    ref = _sd(name)
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k, v in sd.items():
        if k.endswith("spline_weight"):
            # torch.linalg.lstsq (kan.py:126-128) is not bit-reproducible run to run: the
            # reference itself, re-run, differs from its own fixture by a few ulps here
            assert np.max(np.abs(v.numpy() - ref[k])) < 1e-7, k
        else:
            assert np.array_equal(v.numpy(), ref[k]), k


def test_kan_bases_bit_exact_vs_torch_recursion():
    """The oracle's fp32 bases equal the module's torch recursion (kan.py:94-104 op order)."""
    from inr_for_audio_amd.kan import bspline_bases
    sd = _sd("k64")
    x = np.random.default_rng(0).uniform(-1.2, 1.2, (500, 64)).astype(np.float32)
    x[:5, 0] = [-1.0, 1.0, 0.2, -0.6, 1.4]
    ref = bspline_bases(torch.from_numpy(x), torch.from_numpy(sd["layers.1.grid"]), 3).numpy()
    assert np.array_equal(orc.kan_bases(x, sd["layers.1.grid"]), ref)


def test_kan_oracle_matches_reference():
    f = load("kan_fwd_bwd.npz")
    g = load("gt_bach_1s.npz")
    idx = f["subset_idx"]
    t, y = g["coords"][idx].reshape(-1, 1), g["target"][idx]
    sd = _sd("k64")
    out, xs = orc.kan_forward(sd, t, 3)
    ref = f["k64_out"]
    assert np.max(np.abs(out - ref)) < 1e-5 * max(1.0, np.max(np.abs(ref)))
    assert abs(orc.mse(out, y) - float(f["k64_loss"][0])) < 1e-5 * float(f["k64_loss"][0])
    grads = orc.kan_backward(sd, xs, orc.mse_grad(out, y), 3)
    for k, gr in grads.items():
        r = f[f"k64_grad_{k}"]
        rel = np.linalg.norm(gr.reshape(r.shape) - r) / np.linalg.norm(r)
        assert rel < 1e-4, (k, rel)


def test_span_by_count_equals_span_predicate():
    """kan_tiles.h kan_bases_window (KAN_WINDOW_GATHER): for non-decreasing knots the span found by
    counting, s = #{j : g[j] <= x} - 1 if that count is 1 .. 11 else -1, equals the span of the
    per-span predicate g[j] <= x < g[j+1] (kan.py:94-96's order-0 bases), for x on, between and
    outside the knots, +-inf and NaN, on uniform grids (efficient-KAN init) and on sorted grids
    with repeated knots (what update_grid can produce)."""
    rng = np.random.default_rng(0)
    grids = [(np.arange(-3, 9, dtype=np.float32) * np.float32(0.4) - np.float32(1.0))]
    for _ in range(40):
        g = np.sort(rng.normal(size=12).astype(np.float32))
        if rng.random() < 0.5:  # repeated knots
            k = rng.integers(0, 11)
            g[k + 1] = g[k]
        grids.append(g)
    for g in grids:
        xs = np.concatenate([g, np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf)),
                             rng.uniform(g[0] - 1, g[-1] + 1, 200).astype(np.float32),
                             np.array([np.inf, -np.inf, np.nan], dtype=np.float32)])
        for x in xs:
            s_pred = -1
            for j in range(11):
                if g[j] <= x < g[j + 1]:
                    s_pred = j
            cnt = int(np.sum(x >= g))
            s_cnt = cnt - 1 if 1 <= cnt <= 11 else -1
            assert s_cnt == s_pred, (g, x)


def test_hip_path_rejects_unsorted_knots():
    """The HIP KAN path counts knots to find a span, which needs non-decreasing knots: a grid
    that is not is rejected before any launch; after the grid is restored the layer passes."""
    from inr_for_audio_amd import kan as hk
    torch.manual_seed(0)
    lay = hk.KANLinear(4, 3)
    hk._hip_check_layer(lay)
    keep = lay.grid.clone()
    with torch.no_grad():
        lay.grid[2, 5], lay.grid[2, 6] = lay.grid[2, 6].item(), lay.grid[2, 5].item()
    with pytest.raises(NotImplementedError, match="non-decreasing"):
        hk._hip_check_layer(lay)
    with torch.no_grad():
        lay.grid.copy_(keep)
    hk._hip_check_layer(lay)


# ---- tests/kan_ref.py (the fp64 reference of tests/test_gpu_kan_kernels.py), pinned on the host ----
PROBE_FIN, PROBE_SEED, PROBE_N = 18, 11, 40000


def _probe():
    import kan_ref as kr
    g = kr.kan_knots(PROBE_FIN, PROBE_SEED)
    return g, kr.probe_inputs(g, PROBE_N)


def test_kan_knots_are_per_input_and_non_uniform():
    import kan_ref as kr
    g = kr.kan_knots(64, 3)
    assert g.dtype == np.float32 and g.shape == (64, 12)
    gaps = np.diff(g.astype(np.float64), axis=1)
    assert gaps.min() >= 0.05
    assert np.all(gaps.max(1) / gaps.min(1) > 1.05)                 # no row is uniform
    assert len({r.tobytes() for r in g}) == 64                      # no two inputs share a row
    assert np.array_equal(g, kr.kan_knots(64, 3))                   # a function of the seed alone
    x = kr.probe_inputs(g[:18], 4000)
    share = kr.outside(x, g[:18]).mean()
    assert 0.2 < share < 0.6, share                                 # a large share outside the knot range


@pytest.mark.parametrize("fin,fout", [(1, 1), (3, 5), (18, 7)])
def test_kan_ref_equals_torch_fp64_autograd(fin, fout):
    """kan_ref.layer (values, not terms) against torch fp64 autograd of the plain formula
    (kan.py:153-166 on bspline_bases), on kan_knots grids and probe inputs: 1e-12 relative."""
    import kan_ref as kr
    from inr_for_audio_amd.kan import bspline_bases
    rng = np.random.default_rng(fin)
    g = kr.kan_knots(fin, 5)
    x = kr.probe_inputs(g, 300)
    n = x.shape[0]
    bw, sw = rng.normal(size=(fout, fin)).astype(np.float32), rng.normal(size=(fout, fin, 8)).astype(np.float32)
    sc, G = rng.normal(size=(fout, fin)).astype(np.float32), rng.normal(size=(n, fout)).astype(np.float32)
    ref = kr.layer(x, g, bw, sw, sc, G)
    t = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in
         {"x": x, "base_weight": bw, "spline_weight": sw, "spline_scaler": sc}.items()}
    bases = bspline_bases(t["x"], torch.from_numpy(g).double(), 3)
    W = t["spline_weight"] * t["spline_scaler"].unsqueeze(-1)
    out = torch.nn.functional.silu(t["x"]) @ t["base_weight"].t() + bases.reshape(n, -1) @ W.reshape(fout, -1).t()
    (out * torch.from_numpy(G).double()).sum().backward()
    got = {"out": out.detach(), "dX": t["x"].grad, **{k: t[k].grad for k in ("base_weight", "spline_weight",
                                                                               "spline_scaler")}}
    for k, v in got.items():
        r, terms = ref[k]
        assert r.shape == tuple(v.shape) == terms.shape, k
        assert np.max(np.abs(v.numpy() - r)) <= 1e-12 * max(1.0, np.max(np.abs(r))), k
        assert np.all(terms >= np.abs(r) * (1 - 1e-12)), k          # terms bound their own sum


def test_kan_oracle_error_measured_and_zero_outside():
    """The fp32 oracle's bases and derivatives (oracle.siren_oracle.kan_bases, IEEE divisions in
    kan.py's op order) against kan_ref.bases64 on the probe inputs, in units of 2^-24 * scale:
    measured here 7.94 for B and 6.66 for B' (18 inputs, 40 000 draws plus knots each), asserted
    under kan_ref.ORACLE_ERR_B = 8 and ORACLE_ERR_DB = 7 (the measurements rounded up).  These are
    the error of the operation order itself; the GPU gate for B' is 4 x ORACLE_ERR_DB
    (kan_ref.DERIV_C = 28, tests/test_gpu_kan_kernels.py).  Where the scale is 0 (x outside its input's knot
    range) B and B' are exactly 0 in both."""
    import kan_ref as kr
    g, x = _probe()
    b32, db32 = orc.kan_bases(x, g, deriv=True)
    b, db, sb, sdb = kr.bases64(x, g)
    u = 2.0 ** -24
    out = kr.outside(x, g)
    at_first = x == g[None, :, 0]    # every cubic term there carries the factor x - g[0] = 0
    assert np.array_equal(sb.sum(-1) == 0, out | at_first) and np.array_equal(sdb.sum(-1) == 0, out | at_first)
    for v32, v64, s in ((b32, b, sb), (db32, db, sdb)):
        assert np.all(v32[s == 0] == 0) and np.all(v64[s == 0] == 0)
    eb = np.max(np.abs(b32 - b)[sb > 0] / (u * sb[sb > 0]))
    ed = np.max(np.abs(db32 - db)[sdb > 0] / (u * sdb[sdb > 0]))
    print(f"oracle error in 2^-24 * scale: B {eb:.2f}  B' {ed:.2f}")
    assert eb <= kr.ORACLE_ERR_B and ed <= kr.ORACLE_ERR_DB, (eb, ed)


def test_kan_div_emulated_is_the_ieee_quotient():
    """kan_tiles.h kan_div (a reciprocal, a product and two fmas; Markstein) equals the fp32 IEEE
    quotient a / D on every quotient the recursion forms for the kan_knots grids and probe inputs
    the GPU tests use, so the forward's bit-exactness claim holds on those non-default grids."""
    import kan_ref as kr
    for fin, seed, n in ((PROBE_FIN, PROBE_SEED, 4000), (64, 3, 500), (3, 7, 4000)):
        g = kr.kan_knots(fin, seed)
        a, d = kr.recursion_quotients(kr.probe_inputs(g, n), g)
        got, ref = kr.kan_div_emulated(a, d), a / d
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (fin, bad.size, a[bad[:3]], d[bad[:3]], got[bad[:3]], ref[bad[:3]])
