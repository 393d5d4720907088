"""The KAN refit onto a grid of another size on the HIP path: each kernel through the C-ABI
(siren_kan_regrid_knots / _gram / _refit), KANLinear.regrid, KAN.regrid and
train(kan_prev_grid_size=...), against tests/golden/kan_regrid.npz (the reference's own results,
tests/golden/make_golden_kan_regrid.py) and the fp64 restatement tests/kan_regrid_ref.py.

Sizes are the (Go, Gn) pairs kan_regrid_ref.PAIRS.  Bounds.  Knots: bit for bit.  Gram: the fp64 sums
of the exact products of the fp32 bases, each entry within rows * 2^-52 * sum|terms| whatever the
order of the adds; out-of-band entries of G_nn exact zeros, G_nn symmetric; two runs bit-identical.
Refit: one fp32 ulp at the row's largest coefficient against an fp64 numpy solve of the device's own
Gram sums.  Layer and stack: 4 x the reference's own error against the fp64 restatement, as stored in
the fixture.  All scratch starts NaN-filled and has exactly the size the library asks for, so a read
of something no kernel wrote shows.  The Gram test's knots are kan_grids_ref.kan_knots_g, which is
kan_ref.kan_knots' law at any grid size."""
import json
import os

import numpy as np
import pytest
import torch

import kan_grids_ref as kg
import kan_regrid_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SOLVABLE = ["p5_5", "p5_10", "p1_2", "p4_11", "p11_4", "p16_64", "p64_64", "p64_1", "p6_6", "exact5_10"]
REFUSED = ["rank11_4", "rank64_1", "rank6_6"]
GRID5_SOLVABLE = ["normal", "coords", "clustered", "ties", "outside", "few"]  # of kan_grid_update.npz
F32, F64 = np.float32, np.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "kan_regrid.npz")))


@pytest.fixture(scope="module")
def fx5():
    return dict(np.load(os.path.join(GOLDEN, "kan_grid_update.npz")))


def case(fx, name):
    c = {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "_")}
    if "sizes" in c:
        c["Go"], c["Gn"] = (int(v) for v in c["sizes"])
    return c


def _s(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32 if a.dtype == F32 else np.int64)


def dev_knots(lib, dev, x, Gn, grid_eps=0.02, margin=0.01):
    from inr_for_audio_amd._lib import check, ptr
    xs = _t(x.astype(F32), dev)
    q = torch.sort(xs, dim=0)[0][torch.from_numpy(rr.order_index(x.shape[0], Gn)).to(dev)].contiguous()
    grid = torch.full((x.shape[1], Gn + 7), NAN, dtype=torch.float32, device=dev)
    check(lib.siren_kan_regrid_knots(ptr(q), x.shape[1], Gn, margin, grid_eps, ptr(grid), _s(dev)), "knots")
    return grid.cpu().numpy()


def dev_gram(lib, dev, x, grid_old, grid_new, pieces=1):
    """(G_nn [in][Gn+3][Gn+3], G_no [in][Gn+3][Go+3]) over x in `pieces` row pieces (accumulate from the
    second on); NaN-filled scratch of exactly the size the library asks for, and a NaN-filled result."""
    from inr_for_audio_amd._lib import check, ptr
    rows, fin = x.shape
    Go, Gn = grid_old.shape[1] - 7, grid_new.shape[1] - 7
    xs, go, gn = _t(x.astype(F32), dev), _t(grid_old.astype(F32), dev), _t(grid_new.astype(F32), dev)
    out = torch.full((fin * (Gn + 3) * (Gn + Go + 6),), NAN, dtype=torch.float64, device=dev)
    cuts = [rows * k // pieces for k in range(pieces + 1)]
    for k in range(pieces):
        lo, hi = cuts[k], cuts[k + 1]
        nws = int(lib.siren_kan_regrid_workspace_bytes(hi - lo, fin, Go, Gn))
        assert nws % 8 == 0 and nws > 0
        ws = torch.full((nws // 8,), NAN, dtype=torch.float64, device=dev)
        check(lib.siren_kan_regrid_gram(ptr(xs[lo:hi]), hi - lo, fin, Go, Gn, ptr(go), ptr(gn), int(k > 0), ptr(out),
                                        ptr(ws), _s(dev)), "gram")
    return rr.unpack(out.cpu().numpy(), fin, Go, Gn)


def dev_refit(lib, dev, g_nn, g_no, sw, sc):
    """(spline_w_new [out][in][Gn+3] from a NaN-filled buffer, status [2]); sc None: the NULL scaler"""
    from inr_for_audio_amd._lib import check, ptr
    fout, fin, nbo = sw.shape
    nbn = g_nn.shape[-1]
    g, w = _t(rr.pack(g_nn, g_no), dev), _t(sw.astype(F32), dev)
    s = None if sc is None else _t(sc.astype(F32), dev)
    new = torch.full((fout, fin, nbn), NAN, dtype=torch.float32, device=dev)
    status = torch.full((2,), -7, dtype=torch.int32, device=dev)
    check(lib.siren_kan_regrid_refit(ptr(g), fin, fout, nbo - 3, nbn - 3, ptr(w), ptr(s), ptr(new), ptr(status),
                                     _s(dev)), "refit")
    return new.cpu().numpy(), status.cpu().tolist()


# ---- knots ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOLVABLE + REFUSED)
def test_knots_bit_exact(lib, dev, fx, name):
    """The reference's new grid bit for bit, for every Gn of the pairs."""
    c = case(fx, name)
    got = dev_knots(lib, dev, c["x"], c["Gn"])
    assert np.array_equal(bits(got), bits(c["new_grid"]))


@pytest.mark.parametrize("Gn", sorted({gn for _, gn in rr.PAIRS}))
def test_knots_honour_margin_and_eps(lib, dev, fx, Gn):
    x = fx["p5_10_x"]
    for eps, margin in ((0.3, 0.05), (1.0, 0.0), (0.0, 0.25)):
        assert np.array_equal(bits(dev_knots(lib, dev, x, Gn, eps, margin)), bits(rr.knots32(x, Gn, eps, margin))), \
            (eps, margin)


# ---- Gram ----------------------------------------------------------------------------------------
def gram_inputs(rows, fin, Go, Gn):
    """Per-input non-uniform old and new knots (two seeds), x uniform over half a unit beyond either
    grid (so some lie outside the old grid, some outside the new), every fifth row on a knot of the
    old grid and every seventh on one of the new."""
    go, gn = kg.kan_knots_g(fin, Go, 21), kg.kan_knots_g(fin, Gn, 22)
    rng = np.random.default_rng(1000 * fin + rows)
    x = rng.uniform(min(go.min(), gn.min()) - 0.5, max(go.max(), gn.max()) + 0.5, (rows, fin)).astype(F32)
    i = np.arange(fin)
    for r in range(0, rows, 5):
        x[r] = go[i, (r + i) % (Go + 7)]
    for r in range(3, rows, 7):
        x[r] = gn[i, (r + i) % (Gn + 7)]
    return x, go, gn


def gram_reference(x, go, gn):
    """((G_nn, G_no) sums, (G_nn, G_no) sum|terms|) in fp64 from the fp32 bases of bspline_bases on the
    CPU: the reference covers only the summation."""
    from inr_for_audio_amd.kan import bspline_bases
    xt = torch.from_numpy(x)
    bo = bspline_bases(xt, torch.from_numpy(go), 3).double()
    bn = bspline_bases(xt, torch.from_numpy(gn), 3).double()
    ein = lambda a, b: torch.einsum("nic,nid->icd", a, b).numpy()  # noqa: E731
    return (ein(bn, bn), ein(bn, bo)), (ein(bn.abs(), bn.abs()), ein(bn.abs(), bo.abs()))


ALL_ROWS, ALL_FIN = [1, 63, 65, 2049, "pass+77"], [1, 5, 64, 65]
GRAM_CASES = [(go, gn, rows, fin) for go, gn in ((5, 10), (64, 64)) for rows in ALL_ROWS for fin in ALL_FIN]
GRAM_CASES += [(go, gn, rows, fin) for go, gn in rr.PAIRS if (go, gn) not in ((5, 10), (64, 64))
               for rows, fin in ((2049, 65), (1, 1))]
# either side of the dense 5 -> 5 kernel, on the compact one: two column groups, row and input tails
GRAM_CASES += [(5, 6, 65, 65), (6, 5, 65, 65)]


@pytest.mark.parametrize("Go,Gn,rows,fin", GRAM_CASES)
def test_gram(lib, dev, Go, Gn, rows, fin):
    if rows == "pass+77":  # one full pass of the kernel's grid, and 77 rows of the second
        rows = int(lib.siren_kan_regrid_pass_rows(fin, Go, Gn)) + 77
    x, go, gn = gram_inputs(rows, fin, Go, Gn)
    ref, terms = gram_reference(x, go, gn)
    if rows >= 2049:
        assert kg.outside(x, go).any() and kg.outside(x, gn).any()
    got = dev_gram(lib, dev, x, go, gn)
    again = dev_gram(lib, dev, x, go, gn)
    halves = dev_gram(lib, dev, x, go, gn, pieces=2) if rows >= 2 else got
    for k, nm in enumerate(("G_nn", "G_no")):
        bound = rows * 2.0 ** -52 * terms[k]
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all()
        worst = float((np.abs(got[k] - ref[k]) / np.maximum(bound, 1e-300)).max())
        print(f"gram {Go} -> {Gn} rows {rows} in {fin} {nm}: worst error {worst:.3f} of the bound")
        assert (np.abs(got[k] - ref[k]) <= bound).all()
        assert np.array_equal(bits(got[k]), bits(again[k]))
        # two halves, the second accumulating: the same bound of the one sum
        assert (np.abs(halves[k] - ref[k]) <= bound).all()
    a, b = np.indices((Gn + 3, Gn + 3))
    assert (got[0][:, np.abs(a - b) > 3] == 0).all() and (halves[0][:, np.abs(a - b) > 3] == 0).all()
    assert np.array_equal(got[0], got[0].transpose(0, 2, 1))


# ---- at 5 -> 5 against the grid-5 entry points, which forward here ------------------------------
def grid5_gram(lib, dev, x, go, gn):
    from inr_for_audio_amd._lib import check, ptr
    rows, fin = x.shape
    xs, gos, gns = _t(x.astype(F32), dev), _t(go.astype(F32), dev), _t(gn.astype(F32), dev)  # alive over the launch
    out = torch.full((fin, 2, 8, 8), NAN, dtype=torch.float64, device=dev)
    ws = torch.full((int(lib.siren_kan_grid_workspace_bytes(rows, fin)) // 8,), NAN, dtype=torch.float64, device=dev)
    check(lib.siren_kan_grid_gram(ptr(xs), rows, fin, ptr(gos), ptr(gns), 0, ptr(out), ptr(ws), _s(dev)), "grid gram")
    torch.cuda.synchronize(dev)
    return out, ws


@pytest.mark.parametrize("rows,fin", [(2049, 65), (63, 5)])
def test_gram_5_to_5_equals_grid_gram(lib, dev, rows, fin):
    """siren_kan_grid_* is siren_kan_regrid_* at (5, 5): the same sums bit for bit, the same sizes."""
    x, go, gn = gram_inputs(rows, fin, 5, 5)
    g5 = grid5_gram(lib, dev, x, go, gn)[0].cpu().numpy()
    got = dev_gram(lib, dev, x, go, gn)
    for k in range(2):
        assert np.array_equal(bits(got[k]), bits(g5[:, k]))
    for n_in in (1, 65, 256, 512, 4096):
        assert lib.siren_kan_grid_pass_rows(n_in) == lib.siren_kan_regrid_pass_rows(n_in, 5, 5) > 0
        for n in (1, rows, 441000):
            assert lib.siren_kan_grid_workspace_bytes(n, n_in) == lib.siren_kan_regrid_workspace_bytes(n, n_in, 5, 5) > 0


@pytest.mark.parametrize("name", GRID5_SOLVABLE)
def test_refit_5_to_5_equals_grid_refit(lib, dev, fx5, name):
    """On the solvable cases of kan_grid_update.npz, with the scaler (siren_kan_grid_refit always has
    one): bit for bit."""
    from inr_for_audio_amd._lib import check, ptr
    c = case(fx5, name)
    fout, fin = c["spline_scaler"].shape
    g5, ws = grid5_gram(lib, dev, c["x"], c["grid"], c["new_grid"])
    want = torch.full((fout, fin, 8), NAN, dtype=torch.float32, device=dev)
    status = torch.full((2,), -7, dtype=torch.int32, device=dev)
    sw, sc = _t(c["spline_weight"], dev), _t(c["spline_scaler"], dev)
    check(lib.siren_kan_grid_refit(ptr(g5), fin, fout, ptr(sw), ptr(sc), ptr(want), ptr(status), ptr(ws), _s(dev)),
          "grid refit")
    assert status.cpu().tolist()[0] == 0
    g_nn, g_no = dev_gram(lib, dev, c["x"], c["grid"], c["new_grid"])
    got, st = dev_refit(lib, dev, g_nn, g_no, c["spline_weight"], c["spline_scaler"])
    assert st[0] == 0
    assert np.array_equal(bits(got), bits(want))


# ---- refit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [True, False], ids=["scaler", "null"])
@pytest.mark.parametrize("name", SOLVABLE)
def test_refit_vs_fp64_solve(lib, dev, fx, name, scaled):
    c = case(fx, name)
    g_nn, g_no = dev_gram(lib, dev, c["x"], c["grid"], c["new_grid"])
    got, status = dev_refit(lib, dev, g_nn, g_no, c["spline_weight"], c["spline_scaler"] if scaled else None)
    assert status[0] == 0
    # the kernel forms the fp32 product spline_weight * spline_scaler, the reference's scaled_spline_weight
    coeff = (c["spline_weight"] * c["spline_scaler"][..., None]).astype(F32) if scaled else c["spline_weight"]
    want = rr.refit_from_gram(g_nn, g_no, coeff)
    bound = 2.0 ** -23 * np.abs(want).max(-1, keepdims=True)
    worst = float((np.abs(got - want) / bound).max())
    print(f"refit {name}: worst error {worst:.3f} ulp of the row's largest coefficient")
    assert got.shape == want.shape and (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("name", REFUSED)
def test_refit_refuses_rank_deficiency(lib, dev, fx, name):
    """Gn + 2 rows: every input fails the pivot rule; the status word counts them and names the first,
    and nothing is written to the output."""
    c = case(fx, name)
    fin = c["x"].shape[1]
    g_nn, g_no = dev_gram(lib, dev, c["x"], c["grid"], c["new_grid"])
    got, status = dev_refit(lib, dev, g_nn, g_no, c["spline_weight"], c["spline_scaler"])
    assert status == [fin, 0]
    assert np.isnan(got).all()


@pytest.mark.parametrize("name,bad", [("p5_10", 3), ("p64_1", 0), ("p11_4", 16)])
def test_refit_refuses_one_input_among_good_ones(lib, dev, fx, name, bad):
    """Only the zeroed input's rows stay unwritten, and it is the one named."""
    c = case(fx, name)
    g_nn, g_no = dev_gram(lib, dev, c["x"], c["grid"], c["new_grid"])
    g_nn[bad], g_no[bad] = 0.0, 0.0
    got, status = dev_refit(lib, dev, g_nn, g_no, c["spline_weight"], None)
    assert status == [1, bad]
    assert np.isnan(got[:, bad]).all() and np.isfinite(np.delete(got, bad, axis=1)).all()


# ---- the layer -----------------------------------------------------------------------------------
def make_layer(c, dev, scaler=None):
    from inr_for_audio_amd.kan import KANLinear
    fout, fin = c["spline_scaler"].shape
    lay = KANLinear(fin, fout, grid_size=c["Go"])
    lay.load_state_dict({"grid": torch.from_numpy(c["grid"]), "base_weight": torch.from_numpy(c["base_weight"]),
                         "spline_weight": torch.from_numpy(c["spline_weight"]),
                         "spline_scaler": torch.from_numpy(c["spline_scaler"] if scaler is None else scaler)})
    return lay.to(dev)


@pytest.mark.parametrize("name", SOLVABLE)
def test_layer_regrid(lib, dev, fx, name):
    c = case(fx, name)
    lay = make_layer(c, dev)
    before = {k: v.clone() for k, v in lay.state_dict().items()}
    new = lay.regrid(_t(c["x"], dev), c["Gn"])
    assert new is not lay and new.grid_size == c["Gn"] and new.grid.shape == (lay.in_features, c["Gn"] + 7)
    assert new.spline_weight.shape == (lay.out_features, lay.in_features, c["Gn"] + 3)
    assert all(np.array_equal(bits(v), bits(lay.state_dict()[k])) for k, v in before.items())  # the source layer
    assert np.array_equal(bits(new.grid), bits(c["new_grid"]))
    assert np.array_equal(bits(new.base_weight), bits(c["base_weight"]))
    assert np.array_equal(bits(new.spline_scaler), bits(c["spline_scaler"]))
    # the unscaled coefficients refitted, in fp64 on the same knots
    c64 = rr.refit(c["x"], c["grid"], c["new_grid"], c["spline_weight"])
    err, ref_err = rr.coeff_error(npy(new.spline_weight), c64), float(c["ref_err"])
    print(f"regrid {name}: error {err:.3e} = {err / ref_err:.2f} x the reference's {ref_err:.3e}")
    assert err <= 4 * ref_err
    # the chunked Gram accumulation (three chunks) gives the same refit to the same bound
    new3 = lay.regrid(_t(c["x"], dev), c["Gn"], chunk=max(1, c["x"].shape[0] // 3))
    assert rr.coeff_error(npy(new3.spline_weight), c64) <= 4 * ref_err
    # the new layer's forward, on the new knots
    y = new(_t(c["x"], dev)).detach().cpu().numpy()
    y64 = rr.layer_forward(c["x"], c["new_grid"], c["base_weight"], c64, c["spline_scaler"])
    assert y.shape == y64.shape and np.abs(y - y64).max() <= 1e-5 * max(1.0, np.abs(y64).max())
    if c["Go"] == c["Gn"]:
        # equal sizes and a spline_scaler of ones (the fixture's, for these cases): the reference's update_grid
        assert (c["spline_scaler"] == 1).all()
        assert rr.coeff_error(npy(new.spline_weight), c["new_spline_weight"].astype(F64)) <= 4 * ref_err


@pytest.mark.parametrize("name", REFUSED)
def test_layer_rank_deficiency_raises(lib, dev, fx, name):
    from inr_for_audio_amd._lib import SirenError
    c = case(fx, name)
    lay = make_layer(c, dev)
    new = None
    with pytest.raises(SirenError, match="input 0"):
        new = lay.regrid(_t(c["x"], dev), c["Gn"])
    assert new is None
    assert np.array_equal(bits(lay.grid), bits(c["grid"])) and np.array_equal(bits(lay.spline_weight), bits(c["spline_weight"]))


# ---- the stack -----------------------------------------------------------------------------------
NAMES = ("grid", "base_weight", "spline_weight", "spline_scaler")


def make_stack(fx, dev, Go, Gn):
    from inr_for_audio_amd.kan import KAN
    m = KAN([1, 8, 8, 1], grid_size=Go)
    m.load_state_dict({f"layers.{l}.{nm}": torch.from_numpy(fx[f"stack{Go}_{Gn}_l{l}_{nm}"])
                       for l in range(3) for nm in NAMES})
    return m.to(dev)


@pytest.mark.parametrize("Go,Gn", [(5, 10), (4, 11)])
def test_stack_regrid(lib, dev, fx, Go, Gn):
    from inr_for_audio_amd.engine import KanEngine
    m = make_stack(fx, dev, Go, Gn)
    x = _t(fx["stack_x"], dev)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    y_old = m(x).detach().cpu().numpy()
    new = m.regrid(x, Gn)
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in before.items())
    assert new.grid_size == Gn and new.widths == [1, 8, 8, 1] and new.make_net().grid_size == Gn
    assert sorted(new.state_dict()) == sorted(before)
    assert all(p.is_leaf and p.grad_fn is None for p in new.parameters())  # nothing of the refit is recorded
    with torch.no_grad():
        y = new(x)
    assert y.shape == (x.shape[0], 1)
    y = y.cpu().numpy()
    olds = [tuple(fx[f"stack{Go}_{Gn}_l{l}_{nm}"] for nm in NAMES) for l in range(3)]
    y64, _ = rr.stack_regrid(fx["stack_x"], olds, Gn)
    err, ref_err = float(np.abs(y - y64).max() / np.abs(y64).max()), float(fx[f"stack{Go}_{Gn}_out_ref_err"])
    print(f"stack {Go} -> {Gn}: error {err:.3e} = {err / ref_err:.2f} x the reference's {ref_err:.3e}")
    print(f"stack {Go} -> {Gn}: the regrid changes the model's output by "
          f"{float(np.abs(y - y_old).max() / np.abs(y_old).max()):.3e} of its largest value")
    assert err <= 4 * ref_err
    # the returned model trains: three engine steps eager, and the same three with the last two replayed
    # from a captured graph, bit for bit (the losses themselves are not judged)
    t = fx["stack_x"]
    target = torch.from_numpy((0.5 * np.sin(37 * t) + 0.2 * np.sin(91 * t * t)).reshape(-1).astype(F32))
    state = {k: v.detach().cpu().clone() for k, v in new.state_dict().items()}
    runs = []
    for graph in (False, True):
        from inr_for_audio_amd.kan import KAN
        mm = KAN([1, 8, 8, 1], grid_size=Gn)
        mm.load_state_dict(state)
        eng = KanEngine(mm, torch.from_numpy(t), target, lr=1e-3, device=dev)
        eng.step()
        if graph:
            eng.capture_graph(warmup=0)
        eng.step()
        eng.step()
        torch.cuda.synchronize()
        assert graph == (eng.graph is not None) and eng.steps_applied() == 3
        runs.append((eng.params.clone(), eng.history()[0].copy()))
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(runs[0][1], runs[1][1])
    assert np.isfinite(runs[0][1]).all()


# ---- train() -------------------------------------------------------------------------------------
def test_train_continues_on_a_finer_grid(dev, tmp_path):
    """1 s of the shipped clip, KAN([1, 16, 16, 1]): a few steps at grid 5, then
    train(prev_ckpt_path=..., kan_prev_grid_size=5, kan_grid_size=10).

    The bound on the second run's first loss.  The checkpoint holds the parameters after the first
    run's last update, so the loss the second run starts from is the checkpointed model's, L = mean
    (y - t)^2, evaluated here from the checkpoint (the history's last entry is the loss before that
    update and is printed beside it).  The regrid moves the output by d with |d| <= D, the printed
    largest change over the run's coordinates, so L' = mean (y + d - t)^2 differs from L by
    |mean(2 (y - t) d + d^2)| <= 2 sqrt(L) D + D^2 (Cauchy-Schwarz).  The fp32 evaluation of either
    loss adds 1e-5 L (sums of 44100 fp32 squares in blocks, a few 2^-24 each, taken generously).

    The refit runs at kan_regrid_margin=0.  kan.py:169's margin of 0.01 is an absolute pad of the knot
    range, and four steps from the init the hidden activations of this model span 0.005 to 0.05: the
    uniform part of the last interior knot then lies above the largest sample, the last knot span is
    empty and the input is refused as rank deficient (measured on an MI355X: seeds 0, 2, 3, 5, 8 and 9
    of 0 .. 9 are refused at 0.01, none at 0).  Which seeds those are hangs on the last bits of KAN's
    least-squares init, which torch.linalg.lstsq does not reproduce from run to run."""
    from scipy.io import wavfile

    from inr_for_audio_amd.kan import KAN
    from inr_for_audio_amd.run import train
    from inr_for_audio_amd.utils import WaveformFitting
    g = np.load(os.path.join(GOLDEN, "gt_bach_1s.npz"))
    wav = tmp_path / "clip.wav"
    wavfile.write(wav, int(g["fs"]), g["raw"])
    kw = dict(arch="kan", num_hidden_features=16, filename=str(wav), seed=5)
    first = train(str(tmp_path), "g5", "clip", 1, total_steps=4, **kw)
    p1 = json.load(open(os.path.join(os.path.dirname(first), "parameters.json")))
    assert "kan_prev_grid_size" not in p1 and "kan_grid_size" not in p1
    coords, target = WaveformFitting(str(wav), duration=1, decimation=1)[0]
    m = KAN([1, 16, 16, 1])
    m.load_state_dict(torch.load(first, weights_only=True)["model_state_dict"])
    m = m.to(dev)
    x = coords.to(dev)
    t64 = target.numpy().reshape(-1).astype(F64)
    y_old = m(x).detach().cpu().numpy().reshape(-1).astype(F64)
    with torch.no_grad():
        y_new = m.regrid(x, 10, margin=0.0)(x).cpu().numpy().reshape(-1).astype(F64)
    L, D = float(np.mean((y_old - t64) ** 2)), float(np.abs(y_new - y_old).max())
    bound = 2 * np.sqrt(L) * D + D * D + 1e-5 * L
    second = train(str(tmp_path), "g10", "clip", 1, total_steps=1, prev_ckpt_path=first, kan_prev_grid_size=5,
                   kan_grid_size=10, kan_regrid_margin=0.0, **kw)
    p2 = json.load(open(os.path.join(os.path.dirname(second), "parameters.json")))
    assert p2["kan_prev_grid_size"] == 5 and p2["kan_grid_size"] == 10 and p2["prev_ckpt_path"] == first
    assert p2["kan_regrid_margin"] == 0.0
    sd = torch.load(second, weights_only=True)["model_state_dict"]
    assert tuple(sd["layers.1.spline_weight"].shape) == (16, 16, 13) and tuple(sd["layers.2.grid"].shape) == (16, 17)
    L2 = p2["final_loss"]  # total_steps = 1: the first loss
    print(f"train 5 -> 10: the regrid changes the output by at most D = {D:.3e} (largest output {np.abs(y_old).max():.3e}); "
          f"first run's last recorded loss {p1['final_loss']:.6e}, its checkpoint's loss L = {L:.6e}, second run's "
          f"first loss {L2:.6e}: |L2 - L| = {abs(L2 - L):.3e}, bound 2 sqrt(L) D + D^2 + 1e-5 L = {bound:.3e}")
    assert np.isfinite(L2) and abs(L2 - L) <= bound
    # without the argument the old path runs, shape error included
    with pytest.raises(RuntimeError, match="size mismatch"):
        train(str(tmp_path), "g10b", "clip", 1, total_steps=1, prev_ckpt_path=first, kan_grid_size=10, **kw)
