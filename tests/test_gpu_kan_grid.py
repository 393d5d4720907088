"""The KAN grid update (kan.py:168-215) on the HIP path: each kernel through the C-ABI's (5, 5) forwards
(siren_kan_grid_knots / _gram / _refit), KANLinear.update_grid, KAN.forward(x, update_grid=True),
KanEngine.update_grid and regularization_loss, against tests/golden/kan_grid_update.npz (the
reference's own results, tests/golden/make_golden_kan_grid.py) and the fp64 restatement
tests/kan_grid_ref.py.

Bounds.  Knots: bit for bit.  Gram: the fp64 sums of the exact products of the fp32 bases, each
entry within rows * 2^-52 * sum|terms| whatever the order of the adds; out-of-band entries of G_nn
exact zeros; two runs bit-identical.  Refit: one fp32 ulp at the row's magnitude against an fp64
numpy solve of the device's own Gram sums (on the fp32 product spline_weight * spline_scaler, the
reference's scaled_spline_weight, which the kernel forms the same way).  Layer and stack: 4 x the
reference's own error against the fp64 restatement, as stored in the fixture.  All scratch starts
NaN-filled, so a read of something no kernel wrote shows."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

import kan_grid_ref as gr
import kan_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kan_grid_update.npz")
SOLVABLE = ["normal", "coords", "clustered", "ties", "outside", "few"]
F32, F64 = np.float32, np.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def case(fx, name):
    return {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "_")}


def _s(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def dev_knots(lib, dev, x, grid_eps=0.02, margin=0.01):
    from inr_for_audio_amd._lib import check, ptr
    xs = _t(x.astype(F32), dev)
    q = torch.sort(xs, dim=0)[0][torch.from_numpy(gr.order_index(x.shape[0])).to(dev)].contiguous()
    grid = torch.full((x.shape[1], 12), NAN, dtype=torch.float32, device=dev)
    check(lib.siren_kan_grid_knots(ptr(q), x.shape[1], margin, grid_eps, ptr(grid), _s(dev)), "knots")
    return grid.cpu().numpy()


def dev_gram(lib, dev, x, grid_old, grid_new, pieces=1, gram=None):
    """gram [in][2][8][8] over x in `pieces` row pieces (accumulate from the second on); NaN-filled
    scratch of exactly the size the library asks for, and a NaN-filled result."""
    from inr_for_audio_amd._lib import check, ptr
    rows, fin = x.shape
    xs, go, gn = _t(x.astype(F32), dev), _t(grid_old.astype(F32), dev), _t(grid_new.astype(F32), dev)
    out = torch.full((fin, 2, 8, 8), NAN, dtype=torch.float64, device=dev)
    cuts = [rows * k // pieces for k in range(pieces + 1)]
    for k in range(pieces):
        lo, hi = cuts[k], cuts[k + 1]
        nws = int(lib.siren_kan_grid_workspace_bytes(hi - lo, fin))
        assert nws % 8 == 0 and nws > 0
        ws = torch.full((nws // 8,), NAN, dtype=torch.float64, device=dev)
        check(lib.siren_kan_grid_gram(ptr(xs[lo:hi]), hi - lo, fin, ptr(go), ptr(gn), int(k > 0), ptr(out), ptr(ws),
                                      _s(dev)), "gram")
    return out.cpu().numpy()


def dev_refit(lib, dev, gram, sw, sc):
    """(spline_w_new [out][in][8] from a NaN-filled buffer, status [2])"""
    from inr_for_audio_amd._lib import check, ptr
    fout, fin = sc.shape
    g, w, s = _t(gram.astype(F64), dev), _t(sw.astype(F32), dev), _t(sc.astype(F32), dev)
    new = torch.full((fout, fin, 8), NAN, dtype=torch.float32, device=dev)
    status = torch.full((2,), -7, dtype=torch.int32, device=dev)
    ws = torch.full((int(lib.siren_kan_grid_workspace_bytes(1, fin)) // 8,), NAN, dtype=torch.float64, device=dev)
    check(lib.siren_kan_grid_refit(ptr(g), fin, fout, ptr(w), ptr(s), ptr(new), ptr(status), ptr(ws), _s(dev)), "refit")
    return new.cpu().numpy(), status.cpu().tolist()


# ---- knots ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOLVABLE + ["rank", "stack"])
def test_knots_bit_exact(lib, dev, fx, name):
    """The reference's new grid bit for bit (the stack: layer 0, whose input is the coordinates)."""
    x, want = (fx["stack_x"], fx["stack_l0_new_grid"]) if name == "stack" else (fx[f"{name}_x"], fx[f"{name}_new_grid"])
    got = dev_knots(lib, dev, x)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_knots_honour_margin_and_eps(lib, dev, fx):
    x = fx["normal_x"]
    for eps, margin in ((0.3, 0.05), (1.0, 0.0), (0.0, 0.25)):
        assert np.array_equal(dev_knots(lib, dev, x, eps, margin), gr.knots32(x, eps, margin)), (eps, margin)


# ---- Gram ----------------------------------------------------------------------------------------
def gram_inputs(rows, fin):
    """Per-input non-uniform old and new knots (kan_ref.kan_knots, two seeds), x uniform over half a
    unit beyond either grid (so some lie outside the old grid, some outside the new), every fifth
    row on a knot of the old grid and every seventh on one of the new."""
    go, gn = kr.kan_knots(fin, 21), kr.kan_knots(fin, 22)
    rng = np.random.default_rng(1000 * fin + rows)
    x = rng.uniform(min(go.min(), gn.min()) - 0.5, max(go.max(), gn.max()) + 0.5, (rows, fin)).astype(F32)
    i = np.arange(fin)
    for r in range(0, rows, 5):
        x[r] = go[i, (r + i) % 12]
    for r in range(3, rows, 7):
        x[r] = gn[i, (r + i) % 12]
    return x, go, gn


def gram_reference(x, go, gn):
    """(sums, sum|terms|) [in][2][8][8] in fp64 from the fp32 bases of bspline_bases on the CPU: the
    reference covers only the summation."""
    from inr_for_audio_amd.kan import bspline_bases
    xt = torch.from_numpy(x)
    bo = bspline_bases(xt, torch.from_numpy(go), 3).double().numpy()
    bn = bspline_bases(xt, torch.from_numpy(gn), 3).double().numpy()
    ref = np.stack([np.einsum("nic,nid->icd", bn, bn), np.einsum("nic,nid->icd", bn, bo)], 1)
    terms = np.stack([np.einsum("nic,nid->icd", np.abs(bn), np.abs(bn)),
                      np.einsum("nic,nid->icd", np.abs(bn), np.abs(bo))], 1)
    return ref, terms


@pytest.mark.parametrize("fin", [1, 5, 16, 17, 64, 65, 256])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 2049, "pass+77"])
def test_gram(lib, dev, rows, fin):
    if rows == "pass+77":  # one full pass of the kernel's grid, and 77 rows of the second
        rows = int(lib.siren_kan_grid_pass_rows(fin)) + 77
    x, go, gn = gram_inputs(rows, fin)
    ref, terms = gram_reference(x, go, gn)
    if rows >= 257:
        assert kr.outside(x, go).any() and kr.outside(x, gn).any()
    got = dev_gram(lib, dev, x, go, gn)
    bound = rows * 2.0 ** -52 * terms
    assert np.isfinite(got).all()
    worst = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    print(f"gram rows {rows} in {fin}: worst error {worst:.3f} of the bound")
    assert (np.abs(got - ref) <= bound).all()
    for a in range(8):
        for b in range(8):
            if abs(a - b) > 3:
                assert (got[:, 0, a, b] == 0).all()
    assert np.array_equal(got[:, 0], got[:, 0].transpose(0, 2, 1))
    again = dev_gram(lib, dev, x, go, gn)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))
    if rows >= 2:  # two halves, the second accumulating: the same bound of the one sum
        halves = dev_gram(lib, dev, x, go, gn, pieces=2)
        assert (np.abs(halves - ref) <= bound).all()


# ---- refit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOLVABLE)
def test_refit_vs_fp64_solve(lib, dev, fx, name):
    c = case(fx, name)
    g = dev_gram(lib, dev, c["x"], c["grid"], c["new_grid"])
    got, status = dev_refit(lib, dev, g, c["spline_weight"], c["spline_scaler"])
    assert status[0] == 0
    scaled = (c["spline_weight"] * c["spline_scaler"][..., None]).astype(F32)
    want = gr.refit_from_gram(g, scaled, np.ones_like(c["spline_scaler"]))
    bound = 2.0 ** -23 * np.abs(want).max(-1, keepdims=True)
    worst = float((np.abs(got - want) / bound).max())
    print(f"refit {name}: worst error {worst:.3f} ulp of the row's largest coefficient")
    assert (np.abs(got - want) <= bound).all()


def test_refit_refuses_rank_deficiency(lib, dev, fx):
    """Seven rows: both inputs fail the pivot rule; the status word counts them and names the first,
    and nothing is written to the output."""
    c = case(fx, "rank")
    g = dev_gram(lib, dev, c["x"], c["grid"], c["new_grid"])
    got, status = dev_refit(lib, dev, g, c["spline_weight"], c["spline_scaler"])
    assert status == [2, 0]
    assert np.isnan(got).all()
    # one deficient input among good ones: only its rows stay unwritten, and it is the one named
    n = case(fx, "normal")
    g = dev_gram(lib, dev, n["x"], n["grid"], n["new_grid"])
    g[3] = 0.0
    got, status = dev_refit(lib, dev, g, n["spline_weight"], n["spline_scaler"])
    assert status == [1, 3]
    assert np.isnan(got[:, 3]).all() and np.isfinite(np.delete(got, 3, axis=1)).all()


# ---- the layer -----------------------------------------------------------------------------------
def make_layer(c, dev):
    from inr_for_audio_amd.kan import KANLinear
    fout, fin = c["spline_scaler"].shape
    lay = KANLinear(fin, fout)
    lay.load_state_dict({"grid": torch.from_numpy(c["grid"]), "base_weight": torch.from_numpy(c["base_weight"]),
                         "spline_weight": torch.from_numpy(c["spline_weight"]),
                         "spline_scaler": torch.from_numpy(c["spline_scaler"])})
    return lay.to(dev)


@pytest.mark.parametrize("name", SOLVABLE)
def test_layer_update_grid(lib, dev, fx, name):
    c = case(fx, name)
    lay = make_layer(c, dev)
    ptrs = (lay.grid.data_ptr(), lay.spline_weight.data_ptr())
    lay.update_grid(_t(c["x"], dev))
    assert (lay.grid.data_ptr(), lay.spline_weight.data_ptr()) == ptrs
    assert np.array_equal(lay.grid.cpu().numpy().view(np.int32), c["new_grid"].view(np.int32))
    _, c64 = gr.update_grid(c["x"], c["grid"], c["spline_weight"], c["spline_scaler"], grid_new=c["new_grid"])
    err, ref_err = gr.coeff_error(lay.spline_weight.detach().cpu().numpy(), c64), float(c["ref_err"])
    print(f"update_grid {name}: error {err:.3e} = {err / ref_err:.2f} x the reference's {ref_err:.3e}")
    assert err <= 4 * ref_err
    # the chunked Gram accumulation (three chunks) gives the same refit to the same bound
    lay2 = make_layer(c, dev)
    lay2.update_grid(_t(c["x"], dev), chunk=max(1, c["x"].shape[0] // 3))
    assert gr.coeff_error(lay2.spline_weight.detach().cpu().numpy(), c64) <= 4 * ref_err
    # the forward runs on the new knots (the knot check re-ran by itself: its key is the buffer version)
    y = lay(_t(c["x"], dev)).detach().cpu().numpy()
    y64 = gr.layer_forward(c["x"], c["new_grid"], c["base_weight"], c64, c["spline_scaler"])
    assert np.abs(y - y64).max() <= 1e-5 * max(1.0, np.abs(y64).max())


def test_layer_update_grid_in_small_chunks(lib, dev, fx):
    """chunk smaller than the batch (257 rows in chunks of 100): the refit of the Gram sums accumulated
    over the same row pieces in the same order, bit for bit, and inside the layer test's gate."""
    from inr_for_audio_amd._lib import check, ptr
    c = case(fx, "normal")
    rows, fin = c["x"].shape
    assert rows > 200 and rows % 100
    lay = make_layer(c, dev)
    lay.update_grid(_t(c["x"], dev), chunk=100)
    assert np.array_equal(bits(lay.grid), c["new_grid"].view(np.int32))
    xs, go, gn = _t(c["x"], dev), _t(c["grid"], dev), _t(c["new_grid"], dev)
    gram = torch.full((fin, 2, 8, 8), NAN, dtype=torch.float64, device=dev)
    ws = torch.full((int(lib.siren_kan_grid_workspace_bytes(100, fin)) // 8,), NAN, dtype=torch.float64, device=dev)
    for lo in range(0, rows, 100):
        hi = min(rows, lo + 100)
        check(lib.siren_kan_grid_gram(ptr(xs[lo:hi]), hi - lo, fin, ptr(go), ptr(gn), int(lo > 0), ptr(gram), ptr(ws),
                                      _s(dev)), "gram")
    want, status = dev_refit(lib, dev, gram.cpu().numpy(), c["spline_weight"], c["spline_scaler"])
    assert status[0] == 0
    assert np.array_equal(bits(lay.spline_weight), want.view(np.int32))
    _, c64 = gr.update_grid(c["x"], c["grid"], c["spline_weight"], c["spline_scaler"], grid_new=c["new_grid"])
    assert gr.coeff_error(lay.spline_weight.detach().cpu().numpy(), c64) <= 4 * float(c["ref_err"])


def test_layer_rank_deficiency_raises(lib, dev, fx):
    from inr_for_audio_amd._lib import SirenError
    c = case(fx, "rank")
    lay = make_layer(c, dev)
    with pytest.raises(SirenError, match="input 0"):
        lay.update_grid(_t(c["x"], dev))
    assert np.array_equal(lay.grid.cpu().numpy().view(np.int32), c["grid"].view(np.int32))
    assert np.array_equal(lay.spline_weight.detach().cpu().numpy().view(np.int32), c["spline_weight"].view(np.int32))


# ---- the stack -----------------------------------------------------------------------------------
def make_stack(fx, dev, new=False):
    from inr_for_audio_amd.kan import KAN
    m = KAN([1, 8, 8, 1])
    sd = {}
    for l in range(3):
        for nm in ("grid", "base_weight", "spline_weight", "spline_scaler"):
            key = f"stack_l{l}_new_{nm}" if new and nm in ("grid", "spline_weight") else f"stack_l{l}_{nm}"
            sd[f"layers.{l}.{nm}"] = torch.from_numpy(fx[key])
    m.load_state_dict(sd)
    return m.to(dev)


def test_stack_update_grid(lib, dev, fx):
    m = make_stack(fx, dev)
    x = _t(fx["stack_x"], dev)
    y = m(x, update_grid=True)
    assert y.shape == (x.shape[0], 1)
    assert np.array_equal(m.layers[0].grid.cpu().numpy().view(np.int32), fx["stack_l0_new_grid"].view(np.int32))
    old = [tuple(fx[f"stack_l{l}_{nm}"] for nm in ("grid", "base_weight", "spline_weight", "spline_scaler"))
           for l in range(3)]
    y64, _ = gr.stack_update(fx["stack_x"], old)
    err, ref_err = float(np.abs(y.cpu().numpy() - y64).max() / np.abs(y64).max()), float(fx["stack_out_ref_err"])
    print(f"stack output: error {err:.3e} = {err / ref_err:.2f} x the reference's {ref_err:.3e}")
    assert err <= 4 * ref_err
    again = m(x).detach()
    assert not y.requires_grad
    assert np.array_equal(y.cpu().numpy().view(np.int32), again.cpu().numpy().view(np.int32))


def test_regularization_loss(lib, dev, fx):
    """kan.py:217-237, :281-285 on the updated stack: value and gradients at 1e-6 relative to torch's
    CPU values.  A gradient is measured against the layer's largest entry, not entry by entry: an entry is
    sign(w) / 8 * (a + e * (H - log p_oi) / S), and where log p_oi comes near the entropy H the two O(1)
    terms, each carrying fp32's 6e-8, cancel, so two correct fp32 evaluations (torch on the CPU and on
    the device: another log, another summation order) differ by an unbounded factor of such an entry
    itself (measured: 5.9e-6 of the entry on layer 0) while staying at fp32 rounding of the gradient."""
    m = make_stack(fx, dev, new=True)
    ra, re = (float(v) for v in fx["stack_reg_args"])
    loss = m.regularization_loss(ra, re)
    loss.backward()
    assert abs(loss.item() - float(fx["stack_reg"])) <= 1e-6 * abs(float(fx["stack_reg"]))
    for l, lay in enumerate(m.layers):
        want = fx[f"stack_l{l}_reg_grad"]
        got = lay.spline_weight.grad.cpu().numpy()
        diff = np.abs(got.astype(F64) - want.astype(F64))
        print(f"reg grad layer {l}: worst error {float(diff.max() / np.abs(want).max()):.2e} of the largest entry, "
              f"{float((diff / np.abs(want)).max()):.2e} of the entry itself")
        assert diff.max() <= 1e-6 * np.abs(want).max()
        assert lay.base_weight.grad is None and lay.spline_scaler.grad is None


# ---- the engine ----------------------------------------------------------------------------------
E_WIDTHS, E_N, E_STEPS = [1, 16, 16, 1], 3001, 3


def engine_data():
    t = torch.linspace(-1, 1, E_N).reshape(-1, 1)
    return t, (0.5 * torch.sin(37 * t) + 0.2 * torch.sin(91 * t * t)).reshape(-1)


def new_engine(dev, state=None, seed=5):
    from inr_for_audio_amd.engine import KanEngine
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(seed)
    m = KAN(E_WIDTHS)
    if state is not None:
        m.load_state_dict(state)
    t, y = engine_data()
    return KanEngine(m, t, y, lr=1e-3, device=dev)


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def test_engine_update_grid(lib, dev):
    # every engine starts from one state dict: KAN's least-squares init (torch.linalg.lstsq on the CPU)
    # is not bit-reproducible under one seed
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(5)
    init = {k: v.clone() for k, v in KAN(E_WIDTHS).state_dict().items()}
    a = new_engine(dev, init)
    for _ in range(E_STEPS):
        a.step()
    adam = (a.exp_avg.clone(), a.exp_avg_sq.clone())
    hist, opt = a.history(), bytes(a.opt_state())
    pointers = [p.data_ptr() for p in a.model.parameters()] + [lay.grid.data_ptr() for lay in a.model.layers]
    grids = [lay.grid.clone() for lay in a.model.layers]
    out = a.update_grid()
    assert out.shape == (E_N, 1)
    assert pointers == [p.data_ptr() for p in a.model.parameters()] + [lay.grid.data_ptr() for lay in a.model.layers]
    assert all(not torch.equal(g, lay.grid) for g, lay in zip(grids, a.model.layers))   # the knots moved
    assert torch.equal(adam[0], a.exp_avg) and torch.equal(adam[1], a.exp_avg_sq)
    assert bytes(a.opt_state()) == opt and a.steps_applied() == E_STEPS
    for h0, h1 in zip(hist, a.history()):
        assert np.array_equal(h0, h1)
    assert np.array_equal(bits(out), bits(a.infer(a.coords).reshape(-1, 1)))
    state = {k: v.detach().cpu().clone() for k, v in a.model.state_dict().items()}
    a.step()
    # a fresh engine built from the updated state_dict: its first step sees the same loss and gradients
    b = new_engine(dev, state)
    b.step()
    nparam = a.layout.n_params
    assert np.array_equal(bits(a.grads[:nparam]), bits(b.grads[:nparam]))
    assert np.float32(a.last_loss()).view(np.int32) == np.float32(b.last_loss()).view(np.int32)
    # a captured graph replays across the update: the same parameters as the eager engine, bit for bit
    c = new_engine(dev, init)
    c.capture_graph(warmup=1)
    for _ in range(E_STEPS - 1):
        c.step()
    c.update_grid()
    c.step()
    torch.cuda.synchronize()
    assert c.graph is not None
    assert np.array_equal(bits(a.params), bits(c.params)) and np.array_equal(bits(a.grads[:nparam]), bits(c.grads[:nparam]))
    for la, lc in zip(a.model.layers, c.model.layers):
        assert np.array_equal(bits(la.grid), bits(lc.grid))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    import sys
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = new_engine(torch.device("cuda:0"))
    before = eng.params.clone()
    try:
        eng.update_grid()
        q.put((rank, "no error"))
    except NotImplementedError as e:
        q.put((rank, "raised" if torch.equal(before, eng.params) else "raised, parameters changed", str(e)))
    dist.destroy_process_group()


def test_engine_update_grid_two_ranks_raises(lib):
    """Each rank sees only its shard; global order statistics are out of scope, so a process group of
    two ranks (gloo, sharing the GPU) refuses the update and leaves the parameters alone."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == [0, 1]
    assert all(r[1] == "raised" and "one process" in r[2] for r in res), res
