"""SirenEngine / train() with the STFT term and the SNR loss (run.py:126-128, :160-169): one step
against tests/spectral_ref.py evaluated on the engine's own output, the composition of the step
checked bit for bit against siren_forward + siren_backward, graph replay, the plateau scheduler on
negative losses, the refusals, and train(restated_losses=True).

Engine: H = 128, two sine layers, n = 5000 (rows pad to 5120; T = 20 frames).  The first layer's
omega is 10000 (up to 4 rad per sample over this grid, i.e. aliased): the untrained output is then
broadband and every bin's power lies some 250 x above the clamp band [eps / 4, 4 eps] -- at a small
omega the output is smooth, its upper bins hold only rounding noise around the clamp, and whether an
fp32 evaluation clamps such a bin is arbitrary (the precondition below, asserted per case)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import spectral_ref as sr

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, H = 5000, 128
CASES = [("mse", 0.2, True), ("mae", 0.2, True), ("mae", 1.0, True), ("snr", 0.0, True), ("snr", 0.2, True),
         ("mae", 0.2, False)]   # (loss_mode, alpha, last_linear)
_DATA = {}


def data():
    if not _DATA:
        _, y = sr.signals(N)
        _DATA["t"] = torch.linspace(-1, 1, N).reshape(N, 1)
        _DATA["y"] = y.float()
    return _DATA["t"], _DATA["y"]


def make_model(last_linear=True, seed=3):
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(seed)
    return SirenWithSnakeTanh(1, 1, H, 2, 0, 0, last_linear=last_linear, first_omega_0=10000.0, hidden_omega_0=30.0)


def make_engine(dev, loss_mode, alpha, last_linear=True, **kw):
    from inr_for_audio_amd.engine import SirenEngine
    t, y = data()
    return SirenEngine(make_model(last_linear), t, y, lr=1e-4, device=dev, loss_mode=loss_mode, alpha=alpha, **kw)


@pytest.mark.parametrize("loss_mode,alpha,last_linear", CASES)
def test_one_step_vs_reference_and_composition(dev, loss_mode, alpha, last_linear):
    """After one step(): loss_hist[0] is the reference mixed loss of the engine's own ws.out within
    1e-5 relative; ws.g is the reference gradient there under the bound rule of test_gpu_stft
    (e <= 8 e_torch32, e_torch32 = the error of torch's own fp32 autograd of the same loss), zero on
    pad rows.  Then, with no tolerance: a second siren_train_step_spectral's parameter gradients equal, bit
    for bit, siren_forward + that step's g written back + siren_backward on the same workspace."""
    eng = make_engine(dev, loss_mode, alpha, last_linear)
    lib, ws = eng.lib, eng.ws
    _, y = data()
    eng.step()
    torch.cuda.synchronize(dev)
    assert eng.steps_applied() == 1
    out = ws.out[:N].cpu()
    assert sr.clamp_margin_ok(out.double())
    loss64, g64 = sr.loss_and_grad(sr.mixed_loss, out.double(), y.double(), loss_mode, alpha)
    _, g32 = sr.loss_and_grad(sr.mixed_loss, out, y, loss_mode, alpha)
    got = float(eng.loss_hist[0].item())
    rel = abs(got - float(loss64)) / abs(float(loss64))
    e, e32 = sr.grad_err(ws.g[:N].cpu(), g64), sr.grad_err(g32, g64)
    print(f"{loss_mode} alpha {alpha} last_linear {last_linear}: loss {got:.7f} vs {float(loss64):.7f} "
          f"(rel {rel:.2e}); g: e {e:.3e}, e_torch32 {e32:.3e}, ratio {e / max(e32, 1e-300):.2f}")
    assert rel <= 1e-5
    assert e <= 8 * e32
    assert not ws.g[N:].any()

    # composition: the same launches as siren_forward -> g -> siren_backward
    net, gr, b = ctypes.byref(eng.net), ctypes.byref(eng.grad_struct), ctypes.byref(eng.batches[0])
    s = torch.cuda.current_stream(dev).cuda_stream
    npar = eng.layout.n_params
    assert lib.siren_train_step_spectral(net, gr, b, ctypes.byref(eng.spectral_struct), s) == 0
    torch.cuda.synchronize(dev)
    grads_step, g_step, out_step = eng.grads[:npar].clone(), ws.g.clone(), ws.out.clone()
    assert bool(grads_step.any()) and bool(torch.isfinite(grads_step).all())
    eng.grads.fill_(float("nan"))
    assert lib.siren_forward(net, b, s) == 0
    assert torch.equal(ws.out, out_step)
    ws.g.copy_(g_step)
    assert lib.siren_backward(net, gr, b, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(eng.grads[:npar].view(torch.int32), grads_step.view(torch.int32))


@pytest.mark.parametrize("loss_mode,alpha,last_linear", [("mae", 0.2, True), ("snr", 0.2, False)])
def test_graph_replay_matches_eager(dev, loss_mode, alpha, last_linear):
    """Three steps replayed from a captured graph give the loss history of three eager steps, bit
    for bit (the loss scalars stay on the device: the step takes no host synchronisation)."""
    eager = make_engine(dev, loss_mode, alpha, last_linear)
    graph = make_engine(dev, loss_mode, alpha, last_linear)
    for _ in range(3):
        eager.step()
    graph.capture_graph()
    for _ in range(3):
        graph.step()
    torch.cuda.synchronize(dev)
    he, hg = eager.history()[0], graph.history()[0]
    assert len(he) == len(hg) == 3 and np.isfinite(he).all()
    assert np.array_equal(he.view(np.int32), hg.view(np.int32))
    assert torch.equal(eager.params, graph.params)


def test_plateau_on_negative_losses_matches_torch(lib, dev):
    """ReduceLROnPlateau's relative rule cur < best (1 - threshold) on an all-negative trace (the SNR
    loss): lr and num_bad_epochs equal torch's scheduler step for step."""
    from inr_for_audio_amd._lib import SirenOptState, check, ptr
    from inr_for_audio_amd.engine import _opt_state_tensor
    rng = np.random.default_rng(0)
    trace = [-1.0]
    for k in range(59):   # improvements, plateaus, tiny gains inside the threshold, set-backs
        step = rng.choice([-0.5, 0.0, -5e-5, 0.3, -1e-3])
        trace.append(min(trace[-1] + step, -0.01))
    trace = np.asarray(trace, np.float32)
    assert (trace < 0).all()
    lr0, min_lr, factor, patience = 1e-3, 3e-4, 0.8, 2
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr0)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=factor, patience=patience, min_lr=min_lr)
    state = _opt_state_tensor(lr0, min_lr, factor, patience, dev)
    sse = torch.zeros(2, device=dev)
    lh, lrh = torch.zeros(64, device=dev), torch.zeros(64, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    reduced = 0
    for k, v in enumerate(trace):
        sse[0] = float(v)
        check(lib.siren_plateau_step(ptr(state), ptr(sse), 1.0, ptr(lh), ptr(lrh), 64, s), "plateau")
        sch.step(float(v))
        st = SirenOptState.from_buffer_copy(bytes(state.cpu().numpy().tobytes()))
        assert st.lr == opt.param_groups[0]["lr"], (k, st.lr, opt.param_groups[0]["lr"])
        assert st.num_bad == sch.num_bad_epochs and st.best == sch.best, k
        reduced += st.lr != lr0
    assert reduced and st.lr < lr0            # the trace did drive reductions
    assert np.array_equal(lh[:len(trace)].cpu().numpy(), trace)


def test_refusals(dev, monkeypatch):
    from inr_for_audio_amd import engine as E
    t, y = data()
    with pytest.raises(NotImplementedError, match="one micro-batch"):
        make_engine(dev, "mae", 0.2, micro_batch=1024)
    with pytest.raises(NotImplementedError, match="one micro-batch"):
        make_engine(dev, "snr", 0.0, micro_batch=1024)
    with pytest.raises(ValueError, match="512"):
        E.SirenEngine(make_model(), t[:512], y[:512], device=dev, loss_mode="mae", alpha=0.2)
    E.SirenEngine(make_model(), t[:512], y[:512], device=dev, loss_mode="snr")      # no frames: fine
    with pytest.raises(ValueError, match="alpha"):
        make_engine(dev, "mae", 1.5)
    with pytest.raises(NotImplementedError, match="MSELoss only"):
        E.KanEngine(None, t, y, device=dev, loss_mode="snr")
    with pytest.raises(NotImplementedError, match="MSELoss only"):
        E.KanEngine(None, t, y, device=dev, alpha=0.2)
    monkeypatch.setattr(E, "_dist", lambda: object())     # a process group of more than one rank
    with pytest.raises(NotImplementedError, match="one rank"):
        make_engine(dev, "mae", 0.2)


def test_train_with_restated_losses(dev, tmp_path):
    """train(restated_losses=True, loss_mode='mae', alpha=0.2) on the 1 s golden clip: checkpoint and
    parameters.json (alpha and loss_mode recorded), and the mixed loss falls."""
    from inr_for_audio_amd.run import train
    d = tmp_path / "data"
    d.mkdir()
    g = np.load(os.path.join(G, "gt_bach_1s.npz"))
    wavfile.write(str(d / "bach.wav"), int(g["fs"]), g["raw"])
    ck = train(str(tmp_path / "exp"), "s", "bach", 1, loss_mode="mae", alpha=0.2, total_steps=20,
               num_hidden_features=128, omega=1000, data_dir=str(d), seed=1, restated_losses=True)
    assert os.path.exists(ck)
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    assert {"model_state_dict", "optimizer_state_dict"} <= set(sd)
    params = json.load(open(os.path.join(os.path.dirname(ck), "parameters.json")))
    assert params["alpha"] == 0.2 and params["loss_mode"] == "mae" and params["total_steps"] == 20
    losses = train.last_history[0]
    assert len(losses) == 20 and np.isfinite(losses).all()
    assert losses[-1] < losses[0] and params["final_loss"] > 0
