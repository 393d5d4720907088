"""The KAN fit under the mae, snr and STFT losses (run.py:124-128, :160-169 with arch='kan').

1. the L1 step (siren_kan_train_step_loss, loss_mode 1) against the oracle;
2. kan_head_bwd (siren_kan_step_backward) against the MSE pass it shares its rows and sums with;
3. the phased spectral step against the fp64 references on the engine's own signal;
4. that step against its launches called by hand, and across micro-batches;
5. graph replay;  6. train();  7. the L1 fit against the reference's own trajectory.

Gates are the model family's (test_gpu_kan.py: 1e-4 relative L2 per gradient, 1e-5 on the loss, 1e-3 on
a trajectory) and the spectral losses' (test_gpu_spectral_split.py: 1e-5 on the loss, e <= 8 e_torch32)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import kan_loss_cases as kc
import mrstft_ref as mr
import spectral_ref as sr
from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
FUSED = [[1, 64, 64, 1], [1, 32, 30, 1], [1, 32, 16, 1]]   # last-layer in: a full wave, lanes past in, no multiple of 16
UNFUSED = [1, 128, 128, 1]
# (rows, micro_batch, n_valid): nine 256-row blocks with a ragged last one; 1000 + 1000 + 100; pad rows
LAYOUTS = [(2100, 1 << 20, None), (2100, 1000, None), (2100, 1 << 20, 2050)]
_ORACLE = {}


def _data(n_sub):
    g = np.load(os.path.join(G, "gt_bach_1s.npz"))
    t, y = g["coords"].reshape(-1, 1), g["target"]
    idx = np.arange(0, 44100, 44100 // n_sub)[:n_sub]
    return t[idx], y[idx]


def _kan(widths, seed=0):
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(seed)
    return KAN(widths)


def _sd(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def _shared(key, make, x, L):
    """One state dict per case family and its oracle forward (sd, out, per-layer inputs), computed once:
    KAN's least-squares init is not bit-reproducible under one seed, so every engine of the family loads
    these numbers."""
    if key not in _ORACLE:
        sd = _sd(make())
        _ORACLE[key] = (sd,) + tuple(orc.kan_forward(sd, x, L))
    return _ORACLE[key]


def _load(m, sd):
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _refs(eng):
    return ctypes.byref(eng.net), ctypes.byref(eng.grad_struct)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _rel(got, ref):
    return float(np.linalg.norm(np.asarray(got, np.float64).reshape(ref.shape) - ref) / np.linalg.norm(ref))


# ------------------------------------------------------------------ 1. the L1 step
@pytest.mark.parametrize("widths,layout", [(FUSED[0], LAYOUTS[0]), (FUSED[0], LAYOUTS[1]), (FUSED[0], LAYOUTS[2]),
                                           (FUSED[1], LAYOUTS[0]), (FUSED[2], LAYOUTS[1]), (UNFUSED, LAYOUTS[0]),
                                           (UNFUSED, LAYOUTS[2])])
def test_l1_step_vs_oracle(dev, widths, layout):
    """loss_mode='mae' on the gt_bach subset.  The reference gradient is evaluated on the engine's own
    output (g_ref = l1_grad(out_readback, y)): one sample whose err changes sign between fp32 and fp64
    would move a gradient by about 2 / sqrt(N) relative."""
    from inr_for_audio_amd.engine import KanEngine
    n, mb, n_valid = layout
    L = len(widths) - 1
    t, y = _data(n)
    sd, _, xs = _shared(("l1", tuple(widths)), lambda: _kan(widths), t, L)
    m = _load(_kan(widths), sd)
    eng = KanEngine(m, torch.from_numpy(t), torch.from_numpy(y), micro_batch=mb, device=dev, loss_mode="mae")
    assert eng.n_micro == (1 if mb > n else 3) and not eng.split_spectral
    lib, s = eng.lib, _stream(dev)
    net, gr = _refs(eng)
    nv = n if n_valid is None else n_valid
    if n_valid is not None:
        eng.batches[0].n_valid = n_valid

    # a first forward; a dozen targets are set to its output, where torch's sign is 0
    out0 = torch.empty(n, device=dev)
    for k, b in enumerate(eng.batches):
        assert lib.siren_kan_forward(net, ctypes.byref(b), s) == 0
        out0[k * eng.rows:k * eng.rows + b.rows] = eng.out[:b.rows]
    ties = torch.arange(37, nv, nv // 12, device=dev)[:12]
    eng.target[ties] = out0[ties]
    y = eng.target.cpu().numpy()

    # the step's launches by hand, to read every micro-batch's out and g
    out, g = torch.empty(n, device=dev), torch.empty(n, device=dev)
    for k, b in enumerate(eng.batches):
        assert lib.siren_kan_train_step_loss(net, gr, ctypes.byref(b), 1, s) == 0
        out[k * eng.rows:k * eng.rows + b.rows] = eng.out[:b.rows]
        g[k * eng.rows:k * eng.rows + b.rows] = eng.g[:b.rows]
    torch.cuda.synchronize(dev)
    by_hand = eng.grads.clone()
    out_h, g_h = out.cpu().numpy(), g.cpu().numpy()
    assert torch.equal(bits(out), bits(out0))                              # siren_kan_forward's, bit for bit
    g_ref = orc.l1_grad(out_h, y)
    g_ref[nv:] = 0
    assert np.array_equal(g_h, g_ref)                                       # sign(out - y) fp32(1 / N)
    assert np.all(g_h[ties.cpu().numpy()] == 0) and np.all(g_h[nv:] == 0)
    assert np.count_nonzero(g_h[:nv]) == nv - 12

    eng.step()
    torch.cuda.synchronize(dev)
    assert torch.equal(bits(eng.grads), bits(by_hand))
    ref = orc.kan_backward(sd, xs, g_ref, L)
    got = {k: v.detach().cpu().numpy() for k, v in zip(eng.layout.names, eng.grad_views())}
    assert set(ref) == set(got)
    for k, r in ref.items():
        rel = _rel(got[k], r)
        print(f"{widths} {layout} {k}: rel {rel:.2e}")
        assert rel < 1e-4, (k, rel)
    want = orc.l1(out_h[:nv], y[:nv]) * nv / n   # the valid rows' sum over n_total
    assert abs(eng.last_loss() - want) < 1e-5 * want
    for i, k in enumerate(eng.layout.names):   # Adam on the device gradients: bit-exact with the oracle's
        p1, _, _ = orc.adam_step(sd[k].astype(F32), got[k], np.zeros_like(sd[k]), np.zeros_like(sd[k]), 1, 1e-3)
        assert np.array_equal(eng.layout.view(eng.params, i).cpu().numpy(), p1), k


# ------------------------------------------------------------------ 2. kan_head_bwd against the MSE pass
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("widths", FUSED + [UNFUSED])
def test_step_backward_reproduces_the_mse_pass(dev, widths, layout):
    """siren_kan_train_step's gradients and g; then NaN gradients, siren_kan_forward, that g, and
    siren_kan_step_backward: every gradient word is equal (same blocks, same order of sums).  The
    unfused head takes siren_kan_backward's route, so that call gives the same words too."""
    from inr_for_audio_amd.engine import KanEngine
    n, mb, n_valid = layout
    t, y = _data(n)
    eng = KanEngine(_kan(widths), torch.from_numpy(t), torch.from_numpy(y), micro_batch=mb, device=dev)
    lib, s, npar = eng.lib, _stream(dev), eng.layout.n_params
    net, gr = _refs(eng)
    if n_valid is not None:
        eng.batches[0].n_valid = n_valid
    for b in eng.batches:
        b.zero_grads = 1   # each micro-batch on its own
        assert lib.siren_kan_train_step(net, gr, ctypes.byref(b), s) == 0
        want, g = eng.grads[:npar].clone(), eng.g[:b.rows].clone()
        assert bool(torch.isfinite(want).all()) and bool(want.any())
        assert bool((g[b.n_valid:] == 0).all())
        routes = ["siren_kan_step_backward"] + (["siren_kan_backward"] if widths == UNFUSED else [])
        for route in routes:
            eng.grads.fill_(float("nan"))
            assert lib.siren_kan_forward(net, ctypes.byref(b), s) == 0
            eng.g[:b.rows] = g
            extra = (None,) if route == "siren_kan_backward" else ()
            assert getattr(lib, route)(net, gr, ctypes.byref(b), *extra, s) == 0
            torch.cuda.synchronize(dev)
            assert torch.equal(bits(eng.grads[:npar]), bits(want)), (route, b.rows)
    # gradients accumulate when zero_grads is off
    b = eng.batches[-1]
    b.zero_grads = 0
    assert lib.siren_kan_step_backward(net, gr, ctypes.byref(b), s) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(bits(eng.grads[:npar]), bits(want + want))


# ------------------------------------------------------------------ 3. the spectral step
def _spectral_engine(dev, widths, loss_mode, alpha, kind, **kw):
    from inr_for_audio_amd.engine import KanEngine
    sd, _, xs = _shared(("spectral", tuple(widths)), lambda: kc.recorded_model(widths), kc.coords().numpy(), len(widths) - 1)
    m = _load(kc.model(widths), sd)
    kw.setdefault("split_spectral", True)
    eng = KanEngine(m, kc.coords(), kc.target(), device=dev, loss_mode=loss_mode, alpha=alpha, stft_loss=kind, **kw)
    return eng, sd, xs


def clamp_ok(kind, out):
    return mr.clamp_margin_ok(out.double()) if kind == "mrstft" else sr.clamp_margin_ok(out.double())


@pytest.mark.parametrize("widths", kc.WIDTHS)
@pytest.mark.parametrize("loss_mode,alpha,kind", kc.CASES)
def test_spectral_step_vs_reference(dev, widths, loss_mode, alpha, kind):
    """One phased step on the broadband recipe (kan_loss_cases): the finished loss within 1e-5 of the fp64
    reference at the engine's own out_sig, g_sig under e <= 8 e_torch32, the parameter gradients within
    1e-4 of the oracle's backward fed the read-back g_sig.

    Measured on an MI355X from the recorded initial states (kan_loss_cases; two processes gave the same
    digits), 14 cases: loss rel 8e-10 .. 5.3e-8; every parameter gradient 3e-8 .. 5.3e-7; g: e / e_torch32 =
    0.48 .. 0.97 on the ten 'stft' cases, 0.83 on [1, 32, 16, 1] with 'mrstft', and 7.43 on [1, 64, 64, 1] with
    'mrstft' (('mae', 0.2) e 7.91e-4 against 1.065e-4, ('snr', 0.2) 3.99e-4 against 5.37e-5): inside the bound
    of 8, with little room.  That statistic is the max-norm of a heavy-tailed error and moves with the
    init's last bits: before the states were recorded, three processes' own seed-0 inits gave 9.2, 17.7
    (both a miss) and a pass on those two cases, with 0.66 on [1, 32, 16, 1].  The KAN's part is not in
    it: the loss calls are the MLP's, unchanged, and see only out_sig.  This signal's bins span nine
    decades of power (a DC bin of 2e4 beside bins of 2e-5), and the loss kernels evaluate the transform
    as an fp32 dot product per bin where torch.stft runs an fp32 FFT: on the CPU, torch's own fp32 matmul
    against the same windowed cos / sin tables gives e 1.15e-4 against the FFT's 2.57e-5 (4.5 x) on the
    oracle's [1, 64, 64, 1] signal and 4.9e-5 against 1.29e-4 (0.4 x) on the [1, 32, 16, 1] one."""
    eng, sd, xs = _spectral_engine(dev, widths, loss_mode, alpha, kind)
    assert eng.split_spectral and eng.n_micro == 1
    eng.step()
    torch.cuda.synchronize(dev)
    assert eng.steps_applied() == 1
    y, out = kc.target(), eng.out_sig.cpu()
    assert clamp_ok(kind, out)                     # the references' precondition, on the engine's own output
    loss64, g64 = mr.loss_and_grad(mr.mixed_loss, out.double(), y.double(), loss_mode, alpha, kind)
    _, g32 = mr.loss_and_grad(mr.mixed_loss, out, y, loss_mode, alpha, kind)
    got = float(eng.loss_hist[0].item())
    rel = abs(got - float(loss64)) / abs(float(loss64))
    e, e32 = mr.grad_err(eng.g_sig.cpu(), g64), mr.grad_err(g32, g64)
    print(f"{widths} {kind} {loss_mode} alpha {alpha}: loss {got:.7f} vs {float(loss64):.7f} (rel {rel:.2e}); "
          f"g: e {e:.3e}, e_torch32 {e32:.3e}")
    assert rel <= 1e-5
    assert e <= 8 * e32
    L = len(widths) - 1
    ref = orc.kan_backward(sd, xs, eng.g_sig.cpu().numpy(), L)
    for k, v in zip(eng.layout.names, eng.grad_views()):
        r = _rel(v.detach().cpu().numpy(), ref[k])
        print(f"  {k}: rel {r:.2e}")
        assert r < 1e-4, (k, r)


# ------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("widths", [[1, 64, 64, 1], UNFUSED])
@pytest.mark.parametrize("loss_mode,alpha,kind", [("mae", 0.2, "stft"), ("snr", 0.2, "mrstft")])
def test_phased_step_is_its_launches(dev, widths, loss_mode, alpha, kind):
    """One micro-batch: the step's gradients, loss and g equal siren_kan_forward, the three signal calls
    and siren_kan_step_backward called by hand.  Three micro-batches (2048 + 2048 + 904): out_sig, the loss
    and g_sig are the one-micro-batch step's bit for bit; the gradients agree to 1e-4 (their split-K
    order differs)."""
    from inr_for_audio_amd.engine import LOSS_MODES
    one, _, _ = _spectral_engine(dev, widths, loss_mode, alpha, kind)
    lib, s, npar, N = one.lib, _stream(dev), one.layout.n_params, kc.N
    one._launch_grads()
    torch.cuda.synchronize(dev)
    grads, out_sig, g_sig = one.grads.clone(), one.out_sig.clone(), one.g_sig.clone()
    assert bool(torch.isfinite(grads).all()) and bool(grads[:npar].any())

    net, gr = _refs(one)
    b, prefix, mode = one.batches[0], f"siren_{kind}", LOSS_MODES[loss_mode]
    one.grads.zero_()
    assert lib.siren_kan_forward(net, ctypes.byref(b), s) == 0
    x, g, loss = one.out[:N].clone(), torch.full((N,), float("nan"), device=dev), torch.zeros(4, device=dev)
    yp, basis, ws = one.target_sig.data_ptr(), one.stft_basis.data_ptr(), one.stft_ws.data_ptr()
    assert getattr(lib, prefix + "_signal_forward")(x.data_ptr(), yp, N, N, mode, alpha, basis, ws, one._sig_win, s) == 0
    assert getattr(lib, prefix + "_signal_finish")(N, N, mode, alpha, ws, loss.data_ptr(), s) == 0
    assert getattr(lib, prefix + "_signal_backward")(x.data_ptr(), yp, N, N, mode, alpha, basis, ws, one._sig_win,
                                                     0, N, g.data_ptr(), s) == 0
    one.g[:N] = g
    assert lib.siren_kan_step_backward(net, gr, ctypes.byref(b), s) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(bits(x), bits(out_sig)) and torch.equal(bits(g), bits(g_sig))
    assert torch.equal(bits(loss[0]), bits(grads[one.layout.sse_offset]))
    assert torch.equal(bits(one.grads[:npar]), bits(grads[:npar]))

    three, _, _ = _spectral_engine(dev, widths, loss_mode, alpha, kind, micro_batch=2048)
    assert three.n_micro == 3 and three.batches[-1].rows == 904
    three._launch_grads()
    torch.cuda.synchronize(dev)
    assert torch.equal(bits(three.out_sig), bits(out_sig))
    assert torch.equal(bits(three.g_sig), bits(g_sig))
    assert torch.equal(bits(three.grads[three.layout.sse_offset]), bits(grads[one.layout.sse_offset]))
    for i, k in enumerate(one.layout.names):
        a, r = three.layout.view(three.grads, i).cpu().numpy(), one.layout.view(grads, i).cpu().numpy()
        rel = _rel(a, r.astype(np.float64))
        print(f"{widths} {k}: three vs one micro-batch rel {rel:.2e}")
        assert rel < 1e-4, (k, rel)


# ------------------------------------------------------------------ 5. graph replay
@pytest.mark.parametrize("loss_mode,alpha,kind", [("mae", 0.0, "stft"), ("snr", 0.2, "mrstft")])
def test_graph_replay_matches_eager(dev, loss_mode, alpha, kind):
    """Three replayed steps are three eager ones bit for bit (no host synchronisation in either step);
    two micro-batches.  Both engines start from one state dict."""
    eager, _, _ = _spectral_engine(dev, [1, 64, 64, 1], loss_mode, alpha, kind, micro_batch=3000)
    graph, _, _ = _spectral_engine(dev, [1, 64, 64, 1], loss_mode, alpha, kind, micro_batch=3000)
    assert eager.n_micro == 2 and eager.split_spectral == (loss_mode == "snr")
    for _ in range(3):
        eager.step()
    graph.capture_graph()
    for _ in range(3):
        graph.step()
    torch.cuda.synchronize(dev)
    he, hg = eager.history()[0], graph.history()[0]
    assert len(he) == len(hg) == 3 and np.isfinite(he).all()
    assert np.array_equal(he.view(np.int32), hg.view(np.int32))
    assert torch.equal(bits(eager.params), bits(graph.params))


def test_update_grid_between_steps(dev):
    """update_grid() between steps keeps the phased step running on the same pointers: a captured graph
    replays on the new knots, and the loss stays finite."""
    eng, _, _ = _spectral_engine(dev, [1, 32, 16, 1], "mae", 0.2, "stft")
    eng.step()
    eng.capture_graph()
    eng.step()
    eng.update_grid()
    eng.step()
    torch.cuda.synchronize(dev)
    h = eng.history()[0]
    assert len(h) == 3 and np.isfinite(h).all()
    assert bool(torch.isfinite(eng.out_sig).all()) and bool(torch.isfinite(eng.params).all())


# ------------------------------------------------------------------ 6. train()
@pytest.mark.parametrize("kw", [dict(loss_mode="mae"),
                                dict(loss_mode="mae", alpha=0.2, restated_losses=True, split_spectral=True)])
def test_train_kan_with_the_losses(dev, tmp_path, kw):
    """train(arch='kan') for 25 steps on the 1 s clip, width 64.  The run resumes from a checkpoint made of the
    recorded seed-0 state (kan_64_mae_init.npz) with an empty optimizer state, so that it is the same run in
    every process, and takes learning_rate 1e-4: on the linspace grid a KAN's upper STFT bins hold rounding
    noise, the mixed loss answers the init's last bits with +-0.5 %, and at 1e-3 the 25 steps' descent is
    inside that (measured: 9 to 12 of the 24 steps rise, with or without the STFT term; at 1e-4, 3 to 8)."""
    from inr_for_audio_amd.run import train
    g = np.load(os.path.join(G, "gt_bach_1s.npz"))
    wav = tmp_path / "clip.wav"
    wavfile.write(wav, int(g["fs"]), g["raw"])
    init = np.load(os.path.join(G, "kan_64_mae_init.npz"))
    start = tmp_path / "start.pt"
    torch.save({"model_state_dict": {k: torch.from_numpy(init[k]) for k in init.files},
                "optimizer_state_dict": {"state": {}, "param_groups": [{"lr": 1e-4}]}}, start)
    ckpt = train(str(tmp_path), "k", "clip", 1, arch="kan", num_hidden_features=64, total_steps=25,
                 filename=str(wav), seed=0, learning_rate=1e-4, prev_ckpt_path=str(start), **kw)
    folder = os.path.dirname(ckpt)
    _, out = wavfile.read(os.path.join(folder, "output.wav"))
    assert out.shape[0] == 44100 and np.all(np.isfinite(out))
    params = json.load(open(os.path.join(folder, "parameters.json")))
    assert params["arch"] == "kan" and params["loss_mode"] == "mae" and params["alpha"] == kw.get("alpha", 0.0)
    assert params.get("split_spectral", False) == kw.get("split_spectral", False)
    assert np.isfinite(params["SNR"]) and params["final_loss"] > 0
    losses = train.last_history[0]
    print(f"{kw}: first {losses[0]:.6f} last {losses[-1]:.6f} min {np.min(losses):.6f} max {np.max(losses):.6f}")
    assert len(losses) == 25 and np.isfinite(losses).all() and losses[-1] < losses[0]


# ------------------------------------------------------------------ 7. the L1 fit
def test_l1_fit_tracks_reference(dev):
    """30 full-batch steps of KAN([1, 64, 64, 1]) with nn.L1Loss on gt_bach 1 s against the reference's
    own loop (tests/golden/trajectory_kan_64_mae.json, from the recorded initial state).  The gate is the
    MSE trajectory's 1e-3 relative, provided the reference's own sensitivity to the summation order
    (`spread`: its loop with the mean accumulated over two half-batches) lies within a quarter of it;
    otherwise 4 x that spread."""
    from inr_for_audio_amd.engine import KanEngine
    tr = json.load(open(os.path.join(G, "trajectory_kan_64_mae.json")))
    spread = float(np.max(np.abs(np.array(tr["loss_chunked"]) - np.array(tr["loss"])) / np.array(tr["loss"])))
    gate = 1e-3 if spread <= 0.25e-3 else 4 * spread
    g = np.load(os.path.join(G, "gt_bach_1s.npz"))
    t, y = g["coords"].reshape(-1, 1), g["target"]
    m = _kan(tr["widths"], tr["seed"])
    init = np.load(os.path.join(G, "kan_64_mae_init.npz"))
    m.load_state_dict({k: torch.from_numpy(init[k]) for k in init.files})
    eng = KanEngine(m, torch.from_numpy(t), torch.from_numpy(y), device=dev, loss_mode="mae")
    for _ in range(tr["steps"]):
        eng.step()
    losses, lrs = eng.history()
    ref = np.array(tr["loss"])
    dev_rel = float(np.max(np.abs(losses - ref) / ref))
    print(f"L1 fit: deviation {dev_rel:.3e}, reference spread {spread:.3e}, gate {gate:.3e}")
    assert dev_rel < gate, (losses[:5], ref[:5])
    assert np.array_equal(lrs, np.array(tr["lr"]))
