"""End-to-end parity of the fused HIP path (C-ABI siren_train_step / siren_apply_update /
siren_forward / siren_backward) against the CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import siren_oracle as orc
from errlog import check_grads, log
from gpu_util import rel_np as _rel

pytestmark = pytest.mark.gpu


def _model(H, L, w0, w=30.0, in_dim=1, seed=0):
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(seed)
    return SirenWithSnakeTanh(in_dim, 1, H, L, 0, 0, first_omega_0=w0, hidden_omega_0=w)


def _sd(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _signal(n, in_dim=1):
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    if in_dim == 2:
        ch = torch.where(torch.arange(n) % 2 == 0, -1.0, 1.0).reshape(n, 1)
        t = torch.cat([t, ch], 1)
    y = 0.5 * torch.sin(37 * t[:, :1]) + 0.3 * torch.sin(91 * t[:, :1] + 0.5)
    return t, y


@pytest.mark.parametrize("H,L,n,w0,in_dim,mb", [
    (256, 2, 1000, 1000.0, 1, 1 << 20),
    (256, 2, 44100, 22000.0, 1, 1 << 20),
    (512, 3, 3000, 3000.0, 2, 1024),     # stereo (t, ch) grid, 3 micro-batches
    (1024, 4, 2048, 3000.0, 1, 1 << 20),  # SIREN 5x1024
])
def test_train_step_grads_vs_oracle(dev, H, L, n, w0, in_dim, mb):
    from inr_for_audio_amd.engine import SirenEngine
    model = _model(H, L, w0, in_dim=in_dim)
    sd0 = _sd(model)
    t, y = _signal(n, in_dim)
    eng = SirenEngine(model, t, y, lr=1e-3, micro_batch=mb, device=dev)
    eng.step()
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy() for k, v in zip(eng.layout.names, eng.grad_views())}
    p = orc.Params.from_state_dict(sd0, L)
    out, cache = orc.forward(p, t.numpy(), w0, 30.0, half=True, dtype=np.float64)
    ref = orc.backward(p, t.numpy(), cache, orc.mse_grad(out, y.numpy()), w0, 30.0, half=True)
    check_grads(f"engine_step[{H}x{L}x{n}x{in_dim}x{mb}]", got, ref)
    # loss of step 0 and the fp32 (no-fp16-storage) oracle loss agree to storage accuracy
    out32, _ = orc.forward(p, t.numpy(), w0, 30.0)
    l32 = orc.mse(out32, y.numpy())
    log(f"engine_loss_vs_fp32[{H}x{L}x{n}]", rel=abs(eng.last_loss() - l32) / l32)
    assert abs(eng.last_loss() - l32) < 1e-4 * l32  # measured <= 2.2e-6
    # Adam applied with the device gradients is bit-exact with the oracle Adam on them
    flat = [sd0[k].astype(np.float32) for k in eng.layout.names]
    for i, k in enumerate(eng.layout.names):
        pnew, _, _ = orc.adam_step(flat[i], got[k], np.zeros_like(flat[i]), np.zeros_like(flat[i]), 1, 1e-3)
        dev_p = eng.layout.view(eng.params, i).detach().cpu().numpy()
        assert np.array_equal(dev_p, pnew), k


@pytest.mark.parametrize("tile", [128, 256])
def test_train_step_forced_tiles(lib, dev, tile):
    """The fused step with the NT and TN GEMM tile edge forced (256 is what the 2^20-coord
    bench uses) against the oracle, SIREN 5x512 on 2048 rows."""
    from inr_for_audio_amd._lib import Opt, options
    from inr_for_audio_amd.engine import SirenEngine
    # persistent NT grid of 3 blocks: multi-tile walks
    with options(lib, {Opt.NT_TILE: tile, Opt.TN_TILE: tile, Opt.NT_GRID: 3}):
        L, H, w0 = 4, 512, 3000.0
        model = _model(H, L, w0)
        sd0 = _sd(model)
        t, y = _signal(2000)
        eng = SirenEngine(model, t, y, device=dev)
        eng.step()
        torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy() for k, v in zip(eng.layout.names, eng.grad_views())}
    p = orc.Params.from_state_dict(sd0, L)
    out, cache = orc.forward(p, t.numpy(), w0, 30.0, half=True, dtype=np.float64)
    ref = orc.backward(p, t.numpy(), cache, orc.mse_grad(out, y.numpy()), w0, 30.0, half=True)
    check_grads(f"forced_tiles[{tile}]", got, ref)


def test_micro_batching_matches_full_batch(dev):
    from inr_for_audio_amd.engine import SirenEngine
    t, y = _signal(5000)
    grads = []
    for mb in (1 << 20, 1024, 640):
        eng = SirenEngine(_model(256, 2, 2000.0), t, y, micro_batch=mb, device=dev)
        eng.step()
        grads.append(eng.grads.cpu().numpy().copy())
    for g in grads[1:]:
        assert _rel(g, grads[0]) < 1e-4


def test_graph_replay_matches_eager(dev):
    from inr_for_audio_amd.engine import SirenEngine
    t, y = _signal(4096)
    a = SirenEngine(_model(256, 2, 2000.0), t, y, device=dev)
    b = SirenEngine(_model(256, 2, 2000.0), t, y, device=dev)
    for _ in range(5):
        a.step()
    b.step()
    b.capture_graph()
    for _ in range(4):
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    la, _ = a.history()
    lb, _ = b.history()
    assert np.array_equal(la, lb)


def test_graph_replay_with_tile_queue(dev, lib):
    """At 65 536 rows x 512 the forward GEMMs take the 256-tile ping-pong kernel with the dynamic
    tile queue (256 tiles, grid % 8 == 0): a captured step replays the queue kernels (their
    counters re-zero themselves at the end of every launch) and stays bit-identical to eager."""
    from inr_for_audio_amd.engine import SirenEngine
    assert lib.siren_nt_tile(65536, 512) == 256
    t, y = _signal(65536)
    a = SirenEngine(_model(512, 2, 2000.0), t, y, device=dev)
    b = SirenEngine(_model(512, 2, 2000.0), t, y, device=dev)
    for _ in range(4):
        a.step()
    b.step()
    b.capture_graph()
    for _ in range(3):
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)


def test_determinism(dev):
    from inr_for_audio_amd.engine import SirenEngine
    t, y = _signal(3000)
    runs = []
    for _ in range(2):
        e = SirenEngine(_model(512, 2, 2000.0), t, y, device=dev)
        for _ in range(3):
            e.step()
        runs.append(e.params.cpu().numpy().copy())
    assert np.array_equal(runs[0], runs[1])


def test_forward_and_autograd_vs_oracle(dev):
    L, H, w0 = 2, 256, 1500.0
    model = _model(H, L, w0).to(dev)
    sd0 = _sd(model)
    t, y = _signal(777)
    out = model(t.reshape(1, -1, 1).to(dev))
    assert out.shape == (1, 777, 1)
    loss = torch.nn.functional.mse_loss(out, y.reshape(1, -1, 1).to(dev))
    loss.backward()
    p = orc.Params.from_state_dict(sd0, L)
    o_ref, cache = orc.forward(p, t.numpy(), w0, 30.0, half=True, dtype=np.float64)
    assert _rel(out.detach().cpu().numpy().reshape(-1), o_ref) < 1e-2
    ref = orc.backward(p, t.numpy(), cache, orc.mse_grad(o_ref, y.numpy()), w0, 30.0, half=True)
    for (k, prm) in model.named_parameters():
        assert _rel(prm.grad.cpu().numpy().reshape(ref[k].shape), ref[k]) < 3e-2, k


def test_infer_chunks(dev):
    from inr_for_audio_amd.engine import SirenEngine
    t, y = _signal(3000)
    eng = SirenEngine(_model(256, 2, 2000.0), t, y, device=dev)
    o1 = eng.infer(t.to(dev))
    o2 = eng.infer(t.to(dev), chunk=256)
    assert torch.allclose(o1, o2, atol=1e-6)


def test_cpu_tensors_raise(lib):
    model = _model(256, 2, 1000.0)
    with pytest.raises(RuntimeError):
        model(torch.zeros(1, 10, 1))


@pytest.mark.parametrize("n", [1, 7, 129])
def test_tiny_and_ragged_inputs(dev, n):
    """Fewer coordinates than one 128-row tile (padding rows carry g = 0) and one row past a
    tile: the fused step still equals the oracle, and KAN (no padding) too."""
    from inr_for_audio_amd.engine import KanEngine, SirenEngine
    from inr_for_audio_amd.kan import KAN
    t, y = _signal(n)
    m = _model(128, 2, 1000.0)
    sd0 = _sd(m)
    eng = SirenEngine(m, t, y, device=dev)
    eng.step()
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy() for k, v in zip(eng.layout.names, eng.grad_views())}
    p = orc.Params.from_state_dict(sd0, 2)
    out, cache = orc.forward(p, t.numpy(), 1000.0, 30.0, half=True, dtype=np.float64)
    ref = orc.backward(p, t.numpy(), cache, orc.mse_grad(out, y.numpy()), 1000.0, 30.0, half=True)
    check_grads(f"tiny[{n}]", got, ref)
    torch.manual_seed(0)
    km = KAN([1, 16, 16, 1])
    ksd = {k: v.detach().numpy().copy() for k, v in km.state_dict().items()}
    keng = KanEngine(km, t, y, device=dev)
    keng.step()
    torch.cuda.synchronize()
    kgot = {k: v.detach().cpu().numpy() for k, v in zip(keng.layout.names, keng.grad_views())}
    kout, xs = orc.kan_forward(ksd, t.numpy(), 3)
    kref = orc.kan_backward(ksd, xs, orc.mse_grad(kout, y.numpy()), 3)
    for k, r in kref.items():
        assert _rel(kgot[k].reshape(r.shape), r) < 1e-4, k


@pytest.mark.parametrize("H,cfg,n,fl,ll", [
    (100, (2, 0, 0), 1500, False, True),     # a width the reference accepts (models.py:310), padded to 128
    (200, (1, 1, 0), 1500, True, False),     # Linear + Snake first, Snake a padded with 1, final SineLayer
    (384, (1, 0, 1), 1024, False, True),     # padded to 512, Tanh last
    (1500, (2, 0, 0), 1024, False, True),    # padded to 2048: two 1024-column windows per GEMM, unfused head
    (2100, (1, 1, 1), 512, False, True),     # padded to 3072 (three windows), sine + Snake + Tanh last
])
def test_padded_hidden_width_vs_oracle(dev, H, cfg, n, fl, ll):
    """hidden_features that is not 128/256/512/1024 runs zero-padded to the next kernel width: the
    step's gradients in the model's own shapes equal the oracle's for the unpadded network, every
    pad entry's gradient is exactly 0, and after three Adam steps the pads still hold their fill
    (0, or 1 for a Snake a)."""
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(3)
    model = SirenWithSnakeTanh(1, 1, H, *cfg, first_linear=fl, last_linear=ll, first_omega_0=1000.0,
                               hidden_omega_0=30.0, a_initial=0.5)
    sd0 = _sd(model)
    t, y = _signal(n)
    eng = SirenEngine(model, t, y, lr=1e-3, device=dev)
    assert eng.spec.hidden == model.hip_width() > H
    eng.step()
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy() for k, v in zip(eng.layout.names, eng.grad_views())}
    p = orc.Params.from_state_dict(sd0, *cfg, fl, ll)
    out, cache = orc.forward(p, t.numpy(), 1000.0, 30.0, half=True, dtype=np.float64)
    ref = orc.backward(p, t.numpy(), cache, orc.mse_grad(out, y.numpy()), 1000.0, 30.0, half=True)
    assert set(ref) == set(got)
    check_grads(f"padded_width_step[{H}x{cfg}x{fl}x{ll}]", got, ref)
    lay = eng.layout
    for _ in range(2):
        eng.step()
    torch.cuda.synchronize()
    for i, name in enumerate(lay.names):
        if lay.shapes[i] == lay.true_shapes[i]:
            continue
        mask = torch.ones(lay.shapes[i], dtype=torch.bool, device=dev)
        mask[tuple(slice(0, d) for d in lay.true_shapes[i])] = False
        assert bool((lay.view(eng.grads, i)[mask] == 0).all()), name
        fill = 1.0 if name.endswith(".a") else 0.0
        assert bool((lay.view(eng.params, i)[mask] == fill).all()), name
    # the module's parameters are the model-shaped blocks, and the state_dict round-trips
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: v.shape for k, v in sd0.items()}
    # inference through the padded network = the model's own forward (autograd drop-in, also padded)
    with torch.no_grad():
        a = eng.infer(t.to(dev)).cpu()
        b = model(t.to(dev)).reshape(-1).cpu()
    assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()) + 1e-7


def test_padded_width_autograd_dropin(dev):
    """model(x) / loss.backward() at hidden_features=100: HIP forward and backward through the
    padded kernels, gradients in the model's shapes vs the oracle."""
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(5)
    model = SirenWithSnakeTanh(1, 1, 100, 2, 0, 0, first_omega_0=1000.0, hidden_omega_0=30.0)
    sd0 = _sd(model)
    t, y = _signal(1200)
    model = model.to(dev)
    out = model(t.to(dev))
    loss = torch.nn.MSELoss()(out, y.to(dev))
    loss.backward()
    p = orc.Params.from_state_dict(sd0, 2)
    ref_out, cache = orc.forward(p, t.numpy(), 1000.0, 30.0, half=True, dtype=np.float64)
    ref = orc.backward(p, t.numpy(), cache, orc.mse_grad(ref_out, y.numpy()), 1000.0, 30.0, half=True)
    got = {k: v.grad.detach().cpu().numpy() for k, v in model.named_parameters()}
    check_grads("padded_width_autograd", got, ref)


@pytest.mark.parametrize("H,n", [(2048, 16384), (4096, 2048)])
def test_wide_hidden_windows_vs_oracle(dev, H, n):
    """Hidden widths above 1024 (the reference takes any, models.py:310-311) run every GEMM, the
    first layer and the head backward over 1024-column windows (gemm_nt, first_fwd, head_bwd):
    one step's gradients equal the oracle's.  16384 rows x 2048 takes the 256x256 ping-pong tiles
    (512 tiles), 2048 rows x 4096 the 128x128 ones."""
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(5)
    model = SirenWithSnakeTanh(1, 1, H, 2, 0, 0, first_linear=False, last_linear=True, first_omega_0=1000.0,
                               hidden_omega_0=30.0)
    sd0 = _sd(model)
    t, y = _signal(n)
    eng = SirenEngine(model, t, y, lr=1e-3, device=dev)
    assert eng.spec.hidden == H
    with torch.no_grad():  # inference at the initial weights (the step below updates them)
        a = eng.infer(t.to(dev)).cpu().numpy().reshape(-1)
    eng.step()
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy() for k, v in zip(eng.layout.names, eng.grad_views())}
    p = orc.Params.from_state_dict(sd0, 2, 0, 0, False, True)
    out, cache = orc.forward(p, t.numpy(), 1000.0, 30.0, half=True, dtype=np.float64)
    ref = orc.backward(p, t.numpy(), cache, orc.mse_grad(out, y.numpy()), 1000.0, 30.0, half=True)
    check_grads(f"wide_hidden_step[{H}x{n}]", got, ref)
    err = float(np.max(np.abs(a - out.reshape(-1))))
    log(f"wide_hidden_infer[{H}x{n}]", err=err, scale=float(np.max(np.abs(out))))
    assert err <= 1e-3 * float(np.max(np.abs(out))) + 1e-5
