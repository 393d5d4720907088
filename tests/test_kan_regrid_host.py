"""The KAN refit onto a grid of another size, on the host: the identities the kernels of
csrc/kan_general.hip (kan_regrid_*) rest on, checked with the fp64 restatement tests/kan_regrid_ref.py
on the fixture tests/golden/kan_regrid.npz, and the host side of the interface (the C-ABI's argument
types and validation, train()'s refusals, and what stays refused)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kan_grids_ref as kg
import kan_regrid_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kan_regrid.npz")
SOLVABLE = ["p5_5", "p5_10", "p1_2", "p4_11", "p11_4", "p16_64", "p64_64", "p64_1", "p6_6", "exact5_10"]
REFUSED = ["rank11_4", "rank64_1", "rank6_6"]
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def case(fx, name):
    return {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "_")}


def test_fixture_covers_every_pair(fx):
    assert sorted(tuple(int(v) for v in fx[f"{n}_sizes"]) for n in SOLVABLE[:-1]) == sorted(rr.PAIRS)


@pytest.mark.parametrize("name", SOLVABLE)
def test_gram_route_equals_lstsq_route(fx, name):
    """c = G_nn^-1 G_no c_old is the least-squares fit of the old curves on the new bases, in fp64, for
    sizes that differ: the identity the kernels rest on.  The normal equations square the condition
    number, so the bound is the Gram matrix's: 64 eps cond(G_nn) of the largest coefficient."""
    c = case(fx, name)
    Go, Gn = (int(v) for v in c["sizes"])
    assert c["grid"].shape[1] == Go + 7 and c["new_grid"].shape[1] == Gn + 7
    coeff = c["spline_weight"].astype(F64)
    g_nn, g_no = rr.gram(c["x"], c["grid"], c["new_grid"])
    assert g_nn.shape[1:] == (Gn + 3, Gn + 3) and g_no.shape[1:] == (Gn + 3, Go + 3)
    a, b = rr.refit_from_gram(g_nn, g_no, coeff), rr.refit(c["x"], c["grid"], c["new_grid"], coeff)
    cond = max(np.linalg.cond(g) for g in g_nn)
    err = rr.coeff_error(a, b)
    print(f"{name}: Gram route vs lstsq route {err:.2e}, cond(G_nn) {cond:.1e}")
    assert err <= 64 * 2.0 ** -52 * cond
    assert not rr.rank_deficient(g_nn)
    # pack / unpack are the C-ABI's layout
    p_nn, p_no = rr.unpack(rr.pack(g_nn, g_no), len(g_nn), Go, Gn)
    assert np.array_equal(p_nn, g_nn) and np.array_equal(p_no, g_no)


@pytest.mark.parametrize("name", REFUSED)
def test_refused_cases_fail_the_rank_rule(fx, name):
    c = case(fx, name)
    assert c["x"].shape[0] == int(c["sizes"][1]) + 2
    g_nn, _ = rr.gram(c["x"], c["grid"], c["new_grid"])
    assert rr.rank_deficient(g_nn) == list(range(len(g_nn)))


@pytest.mark.parametrize("name", SOLVABLE + REFUSED)
def test_knots32_is_the_references_arithmetic(fx, name):
    c = case(fx, name)
    got = rr.knots32(c["x"], int(c["sizes"][1]))
    assert np.array_equal(got.view(np.int32), c["new_grid"].view(np.int32))
    assert np.abs(rr.knots64(c["x"], int(c["sizes"][1])) - got).max() <= 1e-5


def _check_staircase(x, go, gn):
    """Per input: the span pairs the rows hit lie among the overlapping pairs, and no two overlapping
    pairs share s + r, so the slot s + r addresses a 4 x 4 block of G_no without collisions; there are
    at most Gn + Go + 11 slots."""
    so, sn = rr.spans(x, go), rr.spans(x, gn)
    for i in range(x.shape[1]):
        pairs = rr.overlapping_pairs(go[i], gn[i])
        slots = [s + r for s, r in pairs]
        assert len(set(slots)) == len(slots)
        assert max(slots) <= (gn.shape[1] - 2) + (go.shape[1] - 2) < (gn.shape[1] - 7) + (go.shape[1] - 7) + 11
        hit = {(int(s), int(r)) for s, r in zip(sn[:, i], so[:, i]) if s >= 0 and r >= 0}
        assert hit <= set(pairs)


@pytest.mark.parametrize("Go,Gn", rr.PAIRS)
def test_span_sums_are_unique(fx, Go, Gn):
    """On the knots of the GPU Gram test (kan_grids_ref.kan_knots_g, two seeds), on the fixture's, and
    on knots with ties."""
    go, gn = kg.kan_knots_g(7, Go, 21), kg.kan_knots_g(7, Gn, 22)
    _check_staircase(kg.probe_inputs(np.concatenate([go, gn], 1), 500), go, gn)
    name = next(n for n in SOLVABLE if tuple(fx[f"{n}_sizes"]) == (Go, Gn))
    _check_staircase(fx[f"{name}_x"], fx[f"{name}_grid"], fx[f"{name}_new_grid"])
    tied = gn.copy()
    tied[:, 4] = tied[:, 3]
    _check_staircase(kg.probe_inputs(np.concatenate([go, tied], 1), 500), go, tied)


# ---- the interface ----------------------------------------------------------------------------
def test_lib_argtypes(lib):
    from inr_for_audio_amd import _lib
    p, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    want = {
        "siren_kan_regrid_pass_rows": (i64, [i32, i32, i32]),
        "siren_kan_regrid_workspace_bytes": (i64, [i64, i32, i32, i32]),
        "siren_kan_regrid_knots": (ctypes.c_int, [p, i32, i32, dbl, dbl, p, p]),
        "siren_kan_regrid_gram": (ctypes.c_int, [p, i64, i32, i32, i32, p, p, i32, p, p, p]),
        "siren_kan_regrid_refit": (ctypes.c_int, [p, i32, i32, i32, i32, p, p, p, p, p]),
    }
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # the grid-5 entry points keep their signatures
    assert list(lib.siren_kan_grid_gram.argtypes) == [p, i64, i32, p, p, i32, p, p, p]
    assert list(lib.siren_kan_grid_refit.argtypes) == [p, i32, i32, p, p, p, p, p, p]
    assert _lib.KAN_MAX_GRID == 64


def test_sizes_are_validated_before_any_launch(lib):
    """A size outside 1 .. 64 is SIREN_ERR_CONFIG (1003) whatever the other arguments (NULL pointers
    here, which a valid size answers with SIREN_ERR_NULL, 1002); the size queries return -1."""
    for bad in (0, 65, -3):
        assert lib.siren_kan_regrid_knots(None, 4, bad, 0.01, 0.02, None, None) == 1003
        for go, gn in ((bad, 5), (5, bad)):
            assert lib.siren_kan_regrid_gram(None, 10, 4, go, gn, None, None, 0, None, None, None) == 1003
            assert lib.siren_kan_regrid_refit(None, 4, 4, go, gn, None, None, None, None, None) == 1003
            assert lib.siren_kan_regrid_workspace_bytes(10, 4, go, gn) == -1
            assert lib.siren_kan_regrid_pass_rows(4, go, gn) == -1
    for g in (1, 5, 64):
        assert lib.siren_kan_regrid_knots(None, 4, g, 0.01, 0.02, None, None) == 1002
        assert lib.siren_kan_regrid_gram(None, 10, 4, g, 65 - g, None, None, 0, None, None, None) == 1002
        assert lib.siren_kan_regrid_refit(None, 4, 4, g, 65 - g, None, None, None, None, None) == 1002
    # `in` and `out` as the grid-5 calls
    assert lib.siren_kan_regrid_workspace_bytes(10, 0, 5, 5) == -1 and lib.siren_kan_regrid_workspace_bytes(0, 4, 5, 5) == -1
    assert lib.siren_kan_regrid_pass_rows(4097, 5, 5) == -1


def test_workspace_holds_what_can_be_non_zero(lib):
    """The scratch cap: at the default chunk (2^20 rows of 256 inputs) and 64 -> 64 the scratch is no
    larger than the 1 GiB of x the call reads; it is slices x inputs x the compact entry count
    4 (Gn + 3) + 16 (Gn + Go + 11) doubles, or at 5 -> 5 the dense pair of 8 x 8 matrices, 128."""
    rows, fin = 1 << 20, 256
    assert rows * fin * 4 == 1 << 30
    for Go, Gn in rr.PAIRS + ((64, 64),):
        nws = int(lib.siren_kan_regrid_workspace_bytes(rows, fin, Go, Gn))
        slices = int(lib.siren_kan_regrid_pass_rows(fin, Go, Gn)) // 8
        print(f"{Go} -> {Gn}: workspace {nws / 2 ** 20:.1f} MiB in {slices} slices")
        assert 0 < nws <= 1 << 30
        assert nws == 8 * slices * fin * (128 if (Go, Gn) == (5, 5) else 4 * (Gn + 3) + 16 * (Gn + Go + 11))
    assert lib.siren_kan_regrid_workspace_bytes(1, 1, 1, 1) == 8 * (16 + 16 * 13)


def test_train_refuses_a_previous_grid_size_without_its_checkpoint(tmp_path):
    from inr_for_audio_amd.run import train
    with pytest.raises(ValueError, match="kan_prev_grid_size"):
        train(str(tmp_path), "t", "bach", 1, arch="kan", kan_grid_size=10, kan_prev_grid_size=5)
    with pytest.raises(ValueError, match="kan_prev_grid_size"):
        train(str(tmp_path), "t", "bach", 1, arch="mlp", prev_ckpt_path="x.pt", kan_prev_grid_size=5)


def test_regrid_refuses_before_the_device_is_looked_at():
    from inr_for_audio_amd import kan as hk
    torch.manual_seed(0)
    lay = hk.KANLinear(2, 3, grid_size=4)
    state = {k: v.clone() for k, v in lay.state_dict().items()}
    x = torch.zeros(16, 2)
    for bad in (0, 65, 2.5):
        with pytest.raises(NotImplementedError, match="grid_size from 1 to 64"):
            lay.regrid(x, bad)
        with pytest.raises(NotImplementedError, match="grid_size from 1 to 64"):
            hk.KAN([2, 3, 1], grid_size=4).regrid(x, bad)
    with pytest.raises(RuntimeError, match="HIP path only"):
        lay.regrid(x, 8)
    assert all(torch.equal(v, lay.state_dict()[k]) for k, v in state.items())
    # the constructor's random init of the blank layer leaves the caller's generator alone
    torch.manual_seed(3)
    a = torch.rand(4)
    torch.manual_seed(3)
    blank = hk._blank_layer(lay, 9)
    assert torch.equal(a, torch.rand(4))
    assert blank.grid.shape == (2, 16) and blank.spline_weight.shape == (3, 2, 12) and blank.grid_eps == lay.grid_eps


def test_update_grid_off_grid_5_stays_refused():
    """update_grid runs the regrid kernels at equal sizes, and off grid 5 it still raises its refusal
    (lifting it needs reference fixtures with a non-unit scaler at other sizes)."""
    from inr_for_audio_amd import kan as hk
    torch.manual_seed(0)
    x = torch.zeros(16, 1)
    with pytest.raises(NotImplementedError, match="checked against the reference at grid_size=5 only"):
        hk.KANLinear(1, 3, grid_size=4).update_grid(x)
    with pytest.raises(NotImplementedError, match="checked against the reference at grid_size=5 only"):
        hk.KANLinear(1, 3, grid_size=10).update_grid(x)
    with pytest.raises(NotImplementedError, match="checked against the reference at grid_size=5 only"):
        hk._update_grid_check(64)
    hk._update_grid_check(5)
