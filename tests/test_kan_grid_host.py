"""Host side of the KAN grid update (kan.py:168-215): the fixture tests/golden/kan_grid_update.npz
(written by tests/golden/make_golden_kan_grid.py from the reference on the CPU) against the fp64
restatement tests/kan_grid_ref.py, the Gram identity the kernels rest on, and the C-ABI's argument
checks.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kan_grid_ref as gr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kan_grid_update.npz")
SOLVABLE = ["normal", "coords", "clustered", "ties", "outside", "few"]
ENTRY_POINTS = ["siren_kan_grid_pass_rows", "siren_kan_grid_workspace_bytes", "siren_kan_grid_knots",
                "siren_kan_grid_gram", "siren_kan_grid_refit"]


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def case(fx, name):
    return {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "_")}


@pytest.mark.parametrize("name", SOLVABLE)
def test_restatement_matches_reference(fx, name):
    """The reference's new spline_weight lies within its stored error of the fp64 restatement on the
    reference's knots (the error was measured against this very computation; 0.1 % of slack for
    another machine's LAPACK, whose fp64 result moves by ~1e-16 against an error of ~1e-6), and the
    fp32 knot arithmetic of kan_grid_ref.knots32 gives the reference's grid bit for bit."""
    c = case(fx, name)
    assert np.array_equal(gr.knots32(c["x"]), c["new_grid"])
    _, c64 = gr.update_grid(c["x"], c["grid"], c["spline_weight"], c["spline_scaler"], grid_new=c["new_grid"])
    err = gr.coeff_error(c["new_spline_weight"], c64)
    print(f"{name}: reference error {err:.3e} (stored {float(c['ref_err']):.3e})")
    assert err <= float(c["ref_err"]) * 1.001
    # the fp64 knots agree with the fp32 ones to fp32 rounding of a knot (a few ulps of the range)
    g64 = gr.knots64(c["x"])
    assert np.abs(g64 - c["new_grid"]).max() <= 8 * 2.0 ** -24 * np.abs(g64).max()


@pytest.mark.parametrize("name", SOLVABLE)
def test_gram_identity(fx, name):
    """c_new[i] = G_nn[i]^-1 G_no[i] coeff_old[i] is the least-squares refit: in fp64 numpy the two
    routes agree to the normal equations' conditioning, n^2 cond(G) 2^-53 with n = 8 (a backward-stable
    solve of an 8 x 8 system; the SVD route's own error, ~sqrt(cond(G)) 2^-53, is far inside it),
    relative to the layer's largest coefficient.  Out-of-band entries of G_nn are exact zeros."""
    c = case(fx, name)
    g = gr.gram(c["x"], c["grid"], c["new_grid"])
    for a in range(8):
        for b in range(8):
            if abs(a - b) > 3:
                assert (g[:, 0, a, b] == 0).all()
    assert not gr.rank_deficient(g)
    via_gram = gr.refit_from_gram(g, c["spline_weight"], c["spline_scaler"])
    _, via_lstsq = gr.update_grid(c["x"], c["grid"], c["spline_weight"], c["spline_scaler"], grid_new=c["new_grid"])
    cond = max(np.linalg.cond(g[i, 0]) for i in range(g.shape[0]))
    err = gr.coeff_error(via_gram, via_lstsq)
    print(f"{name}: normal equations vs lstsq {err:.3e}, cond(G) {cond:.2e}")
    assert err <= 64 * cond * 2.0 ** -53


@pytest.mark.parametrize("name", SOLVABLE)
def test_kernel_route_on_the_host(fx, name):
    """The kernels' arithmetic emulated on the CPU -- fp32 bases (bspline_bases, torch's recursion),
    their exact products summed in fp64, an fp64 solve, the result rounded to fp32 -- stays within 4 x
    the reference's own error of the fp64 restatement, the bound the GPU test holds the device to."""
    from inr_for_audio_amd.kan import bspline_bases
    c = case(fx, name)
    x = torch.from_numpy(c["x"])
    b_old = bspline_bases(x, torch.from_numpy(c["grid"]), 3).double().numpy()
    b_new = bspline_bases(x, torch.from_numpy(c["new_grid"]), 3).double().numpy()
    g = np.stack([np.einsum("nic,nid->icd", b_new, b_new), np.einsum("nic,nid->icd", b_new, b_old)], 1)
    scaled = (c["spline_weight"] * c["spline_scaler"][..., None]).astype(np.float32)  # fp32 product, like the kernel
    got = gr.refit_from_gram(g, scaled, np.ones_like(c["spline_scaler"])).astype(np.float32)
    _, c64 = gr.update_grid(c["x"], c["grid"], c["spline_weight"], c["spline_scaler"], grid_new=c["new_grid"])
    err = gr.coeff_error(got, c64)
    print(f"{name}: emulated route {err:.3e} = {err / float(c['ref_err']):.2f} x the reference's {float(c['ref_err']):.3e}")
    assert err <= 4 * float(c["ref_err"])


def test_rank_case_is_refused(fx):
    """Seven rows cannot determine eight coefficients: the Cholesky pivot rule refuses both inputs."""
    c = case(fx, "rank")
    g = gr.gram(c["x"], c["grid"], gr.knots32(c["x"]))
    assert gr.rank_deficient(g) == [0, 1]


def test_stack_fixture_consistent(fx):
    """Layer 0 of the stack sees the coordinates themselves, so its knots are knots32 of them."""
    assert np.array_equal(fx["stack_l0_new_grid"], gr.knots32(fx["stack_x"]))
    for l in range(3):
        assert (np.diff(fx[f"stack_l{l}_new_grid"], axis=1) > 0).all()


def test_binding_lists_entry_points():
    from inr_for_audio_amd import _lib
    for name in ENTRY_POINTS:
        assert name in _lib._SIGS, name


def test_validation_without_device(lib):
    """NULL pointers and bad shapes are refused on the host, before any launch."""
    NULL, SHAPE = 1002, 1001
    assert lib.siren_kan_grid_knots(None, 4, 0.01, 0.02, 1, None) == NULL
    assert lib.siren_kan_grid_knots(1, 4, 0.01, 0.02, None, None) == NULL
    assert lib.siren_kan_grid_knots(1, 0, 0.01, 0.02, 1, None) == SHAPE
    assert lib.siren_kan_grid_knots(1, 4097, 0.01, 0.02, 1, None) == SHAPE
    G = lambda x=1, rows=8, fin=4, go=1, gn=1, gram=1, ws=1: lib.siren_kan_grid_gram(  # noqa: E731
        x, rows, fin, go, gn, 0, gram, ws, None)
    for kw in ("x", "go", "gn", "gram", "ws"):
        assert G(**{kw: None}) == NULL, kw
    assert G(rows=0) == SHAPE and G(fin=0) == SHAPE and G(fin=4097) == SHAPE
    R = lambda gram=1, fin=4, out=2, sw=1, sc=1, new=1, st=1, ws=1: lib.siren_kan_grid_refit(  # noqa: E731
        gram, fin, out, sw, sc, new, st, ws, None)
    for kw in ("gram", "sw", "sc", "new", "st", "ws"):
        assert R(**{kw: None}) == NULL, kw
    assert R(fin=0) == SHAPE and R(out=0) == SHAPE and R(out=4097) == SHAPE
    assert lib.siren_kan_grid_workspace_bytes(0, 4) == -1 and lib.siren_kan_grid_workspace_bytes(8, 0) == -1
    assert lib.siren_kan_grid_pass_rows(0) == -1


def test_workspace_and_pass_sizes(lib):
    """One pass of the Gram grid covers 8 rows per slice; the slices shrink as the 64-input column
    groups grow (about 1024 one-wave blocks), between 8 and 256; the scratch holds one [128][in]
    fp64 partial per slice, and at least the refit's [in][8][8] solution."""
    assert lib.siren_kan_grid_pass_rows(1) == lib.siren_kan_grid_pass_rows(256) == 8 * 256
    assert lib.siren_kan_grid_pass_rows(512) == 8 * 128 and lib.siren_kan_grid_pass_rows(4096) == 8 * 16
    assert lib.siren_kan_grid_workspace_bytes(1, 5) == 8 * 128 * 5            # one slice
    assert lib.siren_kan_grid_workspace_bytes(65, 17) == 8 * 9 * 128 * 17     # ceil(65 / 8) slices
    assert lib.siren_kan_grid_workspace_bytes(441000, 256) == 8 * 256 * 128 * 256
