"""The Gaussian random-Fourier-feature encoding (run.py:141-144) on the HIP path: the encoded
first layer's kernels against fp64, whole steps of SirenEngine(..., encoding=...) against the
oracle fed the fp64-encoded [N][2F] matrix, graph replay, infer, two ranks, and train(num_freq=F).

Reference arithmetic: enc64(x) = cat(cos(2 pi x b^T), sin(2 pi x b^T)) in fp64 numpy from the fp32
x and b; the oracle's first_preact (K <= 2 only) is patched to omega0 (t W0^T + b0) in fp64, its
backward is general in K."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from scipy.io import wavfile

from errlog import STEP_TOL, check_grads, log, rel
from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu
F64 = np.float64
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def enc64(x, b):
    ph = 2.0 * np.pi * np.asarray(x, F64).reshape(-1, 1) @ np.asarray(b, F64).reshape(1, -1)
    return np.concatenate([np.cos(ph), np.sin(ph)], 1)


def enc_torch32(x, b):
    """The reference's own fp32 evaluation on the CPU (rff.functional.gaussian_encoding)."""
    vp = 2 * np.pi * x.reshape(-1, 1) @ b.reshape(-1, 1).T
    return torch.cat((torch.cos(vp), torch.sin(vp)), dim=-1)


_INPUTS = {}


def _inputs(rows, H, F):
    """x, b, W0, b0, a of one shape: drawn once, shared by every case of that shape, never modified."""
    key = (rows, H, F)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * rows + 10 * H + F)
        x = torch.linspace(-1, 1, rows)
        b = torch.randn(F, 1, generator=g) * 10.0
        W0 = (torch.rand(H, 2 * F, generator=g) * 2 - 1) / (2 * F)     # SineLayer is_first init
        b0 = (torch.rand(H, generator=g) * 2 - 1) / np.sqrt(2 * F)       # nn.Linear bias init
        a = 0.5 + torch.rand(H, generator=g)
        _INPUTS[key] = (x, b, W0, b0, a)
    return _INPUTS[key]


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("snake", [False, True])
@pytest.mark.parametrize("w0", [30.0, 22000.0])
@pytest.mark.parametrize("F", [1, 5, 24, 64, 256])
@pytest.mark.parametrize("H", [128, 256, 1024])
@pytest.mark.parametrize("rows", [384, 1024])
def test_first_fwd_vs_fp64(lib, dev, rows, H, F, w0, snake):
    """siren_rff_first_fwd: |got - ref64| <= 2^-11 |ref64| + 2^-25 + 2 e32 on Y0 and C0, e32 = the
    max error of the reference's own fp32 evaluation of the pre-activation on the same inputs (the
    factor 2: another summation order).  Snake epilogue: the pre-activation is z + b0 (no omega0),
    e32 its fp32 error, the same bound on Y0 and C0.  E0 (not bounded by the issue): |dE/dz| <= 2 |z|,
    plus the hardware sin / cos absolute error (~1e-7 at a = 0.5, siren_common.h snake_epi) over
    a^2 >= 1/4."""
    from inr_for_audio_amd._lib import ptr
    x, b, W0, b0, a = _inputs(rows, H, F)
    om = 1.0 if snake else w0
    a32 = (torch.nn.functional.linear(enc_torch32(x, b), W0, b0) * om).numpy()
    a64 = om * (enc64(x.numpy(), b.numpy()) @ W0.numpy().astype(F64).T + b0.numpy().astype(F64))
    e32 = float(np.max(np.abs(a32 - a64)))
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    xd, bd, Wd, b0d, ad = d(x), d(b.reshape(-1)), d(W0), d(b0), d(a)
    Y0, C0, E0 = (torch.empty(rows, H, dtype=torch.float16, device=dev) for _ in range(3))
    KP = lib.siren_rff_kpad(F)
    enc = torch.full((rows, KP), float("nan"), dtype=torch.float16, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    st = lib.siren_rff_first_fwd(ptr(xd), ptr(bd), F, ptr(Wd), ptr(b0d), w0, ptr(ad) if snake else None, rows, H,
                                 ptr(Y0), ptr(C0), ptr(E0) if snake else None, ptr(enc), s)
    assert st == 0
    torch.cuda.synchronize()
    got_y, got_c = Y0.cpu().numpy().astype(F64), C0.cpu().numpy().astype(F64)
    if snake:
        av = a.numpy().astype(F64)[None, :]
        sn, cs = np.sin(av * a64), np.cos(av * a64)
        ref_y, ref_c = a64 + sn * sn / av, 1.0 + 2.0 * sn * cs
        ref_e = (a64 * 2.0 * sn * cs) / av - sn * sn / (av * av)
    else:
        ref_y, ref_c = np.sin(a64), np.cos(a64)
    base = lambda r: 2.0 ** -11 * np.abs(r) + 2.0 ** -25  # noqa: E731
    ey, ec = np.abs(got_y - ref_y), np.abs(got_c - ref_c)
    log(f"rff_fwd[{rows}x{H}x{F}x{w0}x{snake}]", e32=e32, y=float(ey.max()), c=float(ec.max()))
    print(f"rff_fwd rows={rows} H={H} F={F} w0={w0} snake={snake}: e32={e32:.3e} max|dY|={ey.max():.3e} "
          f"max|dC|={ec.max():.3e} over 2^-11|ref|+2^-25: y {np.max(ey - base(ref_y)):.3e} "
          f"c {np.max(ec - base(ref_c)):.3e}")
    assert np.all(ey <= base(ref_y) + 2 * e32)
    assert np.all(ec <= base(ref_c) + 2 * e32)
    if snake:
        ee = np.abs(E0.cpu().numpy().astype(F64) - ref_e)
        assert np.all(ee <= base(ref_e) + 2 * np.abs(a64) * 2 * e32 + 4e-7 * (1 + np.abs(a64)))
    # enc written once as fp16 [rows][KP]: the fp64 encoding to fp16 accuracy, zero pad columns
    ge = enc.cpu().numpy().astype(F64)
    assert np.all(np.abs(ge[:, :2 * F] - enc64(x.numpy(), b.numpy())) <= 2.0 ** -11 + 2e-6)
    assert np.all(ge[:, 2 * F:] == 0)


@pytest.mark.parametrize("F", [1, 5, 24, 64, 256])
def test_encode_kernel_vs_fp64(lib, dev, F):
    """GaussianEncoding on CUDA tensors (siren_rff_encode): max error vs fp64 <= 2 x the error of the
    reference's fp32 torch evaluation on the same inputs."""
    from inr_for_audio_amd import GaussianEncoding
    x, b, _, _, _ = _inputs(1024, 128, F)
    x = x[:1000]
    ref = enc64(x.numpy(), b.numpy())
    e_torch = float(np.max(np.abs(enc_torch32(x, b).numpy() - ref)))
    mod = GaussianEncoding(b=b).to(dev)
    got = mod(x.reshape(1, -1, 1).to(dev))
    assert got.shape == (1, 1000, 2 * F) and got.dtype == torch.float32
    e_dev = float(np.max(np.abs(got.cpu().numpy().reshape(1000, 2 * F) - ref)))
    log(f"rff_encode[{F}]", dev=e_dev, torch32=e_torch)
    print(f"rff_encode F={F}: device {e_dev:.3e}, torch fp32 {e_torch:.3e}")
    assert e_dev <= 2 * e_torch


def _bwd_case(lib, dev, rows, H, F, w0, snake, n_valid, pad_garbage=False):
    from inr_for_audio_amd._lib import ptr
    x, b, _, _, _ = _inputs(rows, H, F)
    g = torch.Generator().manual_seed(7 + rows + H + F)
    S = 64.0
    dZ1 = ((torch.rand(rows, H, generator=g) * 2 - 1) * S).half()           # S = 2^6-scale inputs
    dZ1[n_valid:] = 0                                                       # pad rows: g = 0
    WT = ((torch.rand(H, H, generator=g) * 2 - 1) * np.sqrt(6 / H) / 30).half()
    C0 = (torch.rand(rows, H, generator=g) * 2 - 1 + (1.0 if snake else 0.0)).half()
    E0 = (torch.rand(rows, H, generator=g) * 2 - 1).half()
    x = x.clone()
    if pad_garbage:  # whatever the pad rows hold besides their zero gradient
        x[n_valid:] = torch.randn(rows - n_valid, generator=g) * 1e3
        C0[n_valid:] = 60000.0
        E0[n_valid:] = -60000.0
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    dZ1d, WTd, C0d, E0d, xd, bd = d(dZ1), d(WT), d(C0), d(E0), d(x), d(b.reshape(-1))
    gscale = torch.tensor([S, 1.0 / S], device=dev)
    KP = lib.siren_rff_kpad(F)
    dZ0 = torch.empty(rows, H, dtype=torch.float16, device=dev)
    enc = torch.empty(rows, KP, dtype=torch.float16, device=dev)
    part = torch.empty(rows // 128, 3, H, device=dev)
    red = torch.empty(4, 64, H, device=dev)
    slab = torch.empty(lib.siren_rff_slab_floats(rows, H, F), device=dev)
    gW0, gb0, ga0 = torch.zeros(H, 2 * F, device=dev), torch.zeros(H, device=dev), torch.zeros(H, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    st = lib.siren_rff_first_bwd(ptr(dZ1d), ptr(WTd), ptr(C0d), ptr(E0d) if snake else None, ptr(xd), ptr(bd), F, w0,
                                 rows, H, ptr(gscale), ptr(dZ0), ptr(enc), ptr(part), ptr(red), ptr(slab), ptr(gW0),
                                 ptr(gb0), ptr(ga0) if snake else None, s)
    assert st == 0
    torch.cuda.synchronize()
    got = {"W0": gW0.cpu().numpy(), "b0": gb0.cpu().numpy(), "a0": ga0.cpu().numpy()}
    acc = dZ1.numpy().astype(F64) @ WT.numpy().astype(F64).T / S
    dz0 = acc * C0.numpy().astype(F64) * (1.0 if snake else w0)
    nv = n_valid
    ref = {"W0": dz0[:nv].T @ enc64(x[:nv].numpy(), b.numpy()), "b0": dz0[:nv].sum(0)}
    if snake:
        ref["a0"] = (acc * E0.numpy().astype(F64))[:nv].sum(0)
    return got, ref


@pytest.mark.parametrize("rows,H,F,w0,snake", [
    (384, 128, 1, 30.0, False), (384, 256, 5, 22000.0, False), (1024, 256, 24, 22000.0, False),
    (1024, 128, 256, 22000.0, False), (1024, 1024, 64, 22000.0, False), (384, 1024, 256, 30.0, True),
    (1024, 256, 64, 22000.0, True), (1024, 128, 5, 30.0, True),
])
def test_first_bwd_vs_fp64(lib, dev, rows, H, F, w0, snake):
    """dW0 / db0 (/ da0) of siren_rff_first_bwd against fp64 from the same fp16 inputs (relative L2 <
    STEP_TOL), finite at S = 2^6-scale inputs with omega0 = 22000."""
    got, ref = _bwd_case(lib, dev, rows, H, F, w0, snake, rows)
    for k, r in ref.items():
        assert np.all(np.isfinite(got[k])), k
        e = rel(got[k], r)
        log(f"rff_bwd[{rows}x{H}x{F}x{w0}x{snake}]", key=k, rel=e)
        print(f"rff_bwd rows={rows} H={H} F={F} w0={w0} snake={snake} {k}: rel {e:.3e}")
        assert e < STEP_TOL, (k, e)


@pytest.mark.parametrize("snake", [False, True])
def test_first_bwd_pad_rows_contribute_nothing(lib, dev, snake):
    """n_valid = 1000 in 1024 rows.  In the fused step g = 0 on pad rows makes their dZ exactly zero in
    every layer above, while their enc is (1, ..., 0, ...) and their C0 whatever the forward left:
    the zero travels through dZ1.  So the entry point is run with zero pad-row dZ1 twice -- with
    ordinary pad-row inputs, and with garbage pad-row x / C0 / E0 -- and both must give the same
    bits, equal to the fp64 gradients of the 1000 valid rows."""
    a, ref = _bwd_case(lib, dev, 1024, 256, 24, 22000.0, snake, 1000)
    b, _ = _bwd_case(lib, dev, 1024, 256, 24, 22000.0, snake, 1000, pad_garbage=True)
    for k, r in ref.items():
        assert np.array_equal(a[k], b[k]), k
        assert rel(a[k], r) < STEP_TOL, k


# ------------------------------------------------------------------ whole steps
def _model(H, cfg, F, w0, fl=False, seed=0):
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(seed)
    return SirenWithSnakeTanh(2 * F, 1, H, *cfg, first_linear=fl, first_omega_0=w0, hidden_omega_0=30.0,
                              a_initial=0.5)


def _encoding(F, seed=5):
    from inr_for_audio_amd import GaussianEncoding
    torch.manual_seed(seed)
    return GaussianEncoding(10.0, 1, F)


def _signal(n):
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    return t, 0.5 * torch.sin(37 * t) + 0.3 * torch.sin(91 * t + 0.5)


def _patch_oracle(monkeypatch):
    monkeypatch.setattr(orc, "first_preact", lambda t, W0, b0, omega0: float(omega0) * (
        np.asarray(t, F64) @ np.asarray(W0, F64).T + np.asarray(b0, F64)[None, :]))


@pytest.mark.parametrize("H,cfg,F,n,mb,w0,fl", [
    (256, (2, 0, 0), 24, 1000, 1 << 20, 30.0, False),
    (256, (2, 0, 0), 24, 1000, 1 << 20, 300.0, False),
    (256, (0, 2, 0), 64, 3000, 1024, 30.0, False),         # three micro-batches
    (256, (0, 2, 0), 64, 3000, 1024, 300.0, False),
    (1024, (2, 0, 0), 256, 2048, 1 << 20, 30.0, False),
    (1024, (2, 0, 0), 256, 2048, 1 << 20, 300.0, False),
    (200, (1, 1, 0), 5, 1000, 1 << 20, 30.0, False),        # hidden width padded to 256
    (200, (1, 1, 0), 5, 1000, 1 << 20, 300.0, False),
    (256, (1, 1, 0), 24, 1500, 1 << 20, 300.0, True),       # first_linear: Linear(2F, H) + Snake
])
def test_engine_step_vs_oracle(dev, monkeypatch, H, cfg, F, n, mb, w0, fl):
    from inr_for_audio_amd.engine import SirenEngine
    _patch_oracle(monkeypatch)
    model, enc = _model(H, cfg, F, w0, fl), _encoding(F)
    sd0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    t, y = _signal(n)
    eng = SirenEngine(model, t, y, lr=1e-3, micro_batch=mb, device=dev, encoding=enc)
    assert eng.n_micro == -(-n // eng.rows) and (mb > n or eng.n_micro == 3)
    eng.step()
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy() for k, v in zip(eng.layout.names, eng.grad_views())}
    te = enc64(t.numpy(), enc.b.detach().numpy())
    p = orc.Params.from_state_dict(sd0, *cfg, fl)
    out, cache = orc.forward(p, te, w0, 30.0, half=True, dtype=F64)
    ref = orc.backward(p, te, cache, orc.mse_grad(out, y.numpy()), w0, 30.0, half=True)
    assert set(ref) == set(got)
    check_grads(f"rff_step[{H}x{cfg}x{F}x{n}x{mb}x{w0}x{fl}]", got, ref)
    out32, _ = orc.forward(p, te, w0, 30.0)
    l32 = orc.mse(out32, y.numpy())
    log(f"rff_step_loss[{H}x{cfg}x{F}x{n}x{w0}]", rel=abs(eng.last_loss() - l32) / l32)
    assert abs(eng.last_loss() - l32) < 1e-4 * l32
    # Adam applied with the device gradients is bit-exact with the oracle Adam on them
    for i, k in enumerate(eng.layout.names):
        p0 = sd0[k].astype(np.float32)
        pnew, _, _ = orc.adam_step(p0, got[k], np.zeros_like(p0), np.zeros_like(p0), 1, 1e-3)
        assert np.array_equal(eng.layout.true_view(eng.params, i).detach().cpu().numpy(), pnew), k
    assert eng.guard_state()["overflows"] == 0


def test_step_at_omega_22000_is_finite(dev):
    """The reference's default first omega: dZ0 is stored without omega0, so nothing overflows fp16 at
    the S chosen for the hidden layers (a step against an oracle is not meaningful here: the
    reference's own fp32 first-layer rounding moves the gradients by more than STEP_TOL)."""
    from inr_for_audio_amd.engine import SirenEngine
    t, y = _signal(4096)
    eng = SirenEngine(_model(256, (2, 2, 0), 64, 22000.0), t, y, device=dev, encoding=_encoding(64))
    eng.step()
    torch.cuda.synchronize()
    assert torch.isfinite(eng.grads).all() and float(eng.grads.abs().max()) > 0
    assert eng.guard_state()["overflows"] == 0 and eng.steps_applied() == 1


def test_graph_replay_matches_eager(dev):
    from inr_for_audio_amd.engine import SirenEngine
    t, y = _signal(4096)
    a = SirenEngine(_model(256, (2, 0, 0), 24, 300.0), t, y, device=dev, encoding=_encoding(24))
    b = SirenEngine(_model(256, (2, 0, 0), 24, 300.0), t, y, device=dev, encoding=_encoding(24))
    for _ in range(5):
        a.step()
    b.step()
    b.capture_graph()
    for _ in range(4):
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    assert np.array_equal(a.history()[0], b.history()[0])


def test_infer_is_the_forward_of_the_step(dev):
    """infer() encodes too: on the training coordinates it returns the outputs the step's forward
    left in the workspace, whole or in chunks, and the loss they give is the step's."""
    from inr_for_audio_amd.engine import SirenEngine
    n = 3000
    t, y = _signal(n)
    eng = SirenEngine(_model(256, (1, 1, 0), 24, 300.0), t, y, lr=0.0, min_lr=0.0, device=dev,
                      encoding=_encoding(24))
    eng.step()                                    # lr 0: the weights stay those of the forward
    step_out = eng.ws.out[:n].clone()
    o1 = eng.infer(t.to(dev))
    assert torch.allclose(o1, step_out, atol=1e-6)
    o2 = eng.infer(t.to(dev), chunk=256)
    assert o1.shape == (n,) and torch.allclose(o1, o2, atol=1e-6)
    loss = float(torch.mean((o1.cpu() - y.reshape(-1)) ** 2))
    assert abs(loss - eng.last_loss()) < 1e-5 * loss


# ------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    import sys
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from inr_for_audio_amd.engine import SirenEngine
    t, y = _signal(5001)
    enc = _encoding(24, seed=5 + 17 * rank)       # every rank draws its own: rank 0's must win
    eng = SirenEngine(_model(256, (2, 0, 0), 24, 300.0), t, y, device=torch.device("cuda:0"), encoding=enc)
    eng.step()
    torch.cuda.synchronize()
    q.put((rank, eng.n_local, eng.grads.cpu().numpy().copy(), enc.b.detach().cpu().numpy().copy(),
           eng.rff_B.cpu().numpy().copy()))
    dist.destroy_process_group()


def test_two_rank_engine_matches_single(lib, dev):
    from inr_for_audio_amd.engine import SirenEngine
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r[0], r[1:]) for r in (q.get(timeout=300) for _ in range(2)))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    t, y = _signal(5001)
    enc = _encoding(24, seed=5)
    eng = SirenEngine(_model(256, (2, 0, 0), 24, 300.0), t, y, device=dev, encoding=enc)
    eng.step()
    torch.cuda.synchronize()
    g_full = eng.grads.cpu().numpy()
    assert res[0][0] + res[1][0] == 5001
    b0 = enc.b.detach().numpy()
    for r in (0, 1):
        _, g1, b_mod, b_dev = res[r]
        assert np.array_equal(b_mod, b0) and np.array_equal(b_dev.reshape(b0.shape), b0)
        assert rel(g1, g_full.astype(F64)) < 1e-3


# ------------------------------------------------------------------ train(num_freq=F)
@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("data")
    g = np.load(os.path.join(G, "gt_bach_1s.npz"))
    wavfile.write(str(d / "bach.wav"), int(g["fs"]), g["raw"])
    return str(d)


def test_train_num_freq_artifacts_and_resume(dev, tmp_path, data_dir):
    from inr_for_audio_amd.run import RFF_KEY, train
    exp = str(tmp_path)
    kw = dict(num_freq=16, num_sine=0, num_snake=2, num_hidden_features=128, total_steps=30, data_dir=data_dir)
    ck1 = train(exp, "a", "bach", 1, seed=3, **kw)
    folder = os.path.dirname(ck1)
    fs, out = wavfile.read(os.path.join(folder, "output.wav"))
    assert fs == 44100 and out.dtype == np.float32 and out.reshape(-1).shape == (44100,)
    params = json.load(open(os.path.join(folder, "parameters.json")))
    assert params["num_freq"] == 16 and params["fp16_overflow_steps"] == 0
    ck = torch.load(ck1, map_location="cpu", weights_only=True)
    b = ck[RFF_KEY]
    assert b.shape == (16, 1) and b.dtype == torch.float32
    assert ck["model_state_dict"]["net.0.linear.weight"].shape == (128, 32)
    torch.manual_seed(3)                          # drawn after the model, sigma 10 (run.py:142)
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    SirenWithSnakeTanh(32, 1, 128, 0, 2, 0, first_omega_0=22000, hidden_omega_0=30, a_initial=0.5)
    assert torch.equal(b, torch.randn(16, 1) * 10.0)
    l1 = 10 ** (np.asarray(train.last_history[0]) / 10)          # dB -> loss
    assert l1[-1] < l1[0]
    # resuming reuses the saved b: the loss continues from the saved level, not from the initial one
    ck2 = train(exp, "b", "bach", 1, seed=99, prev_ckpt_path=ck1, **kw)
    assert torch.equal(torch.load(ck2, map_location="cpu", weights_only=True)[RFF_KEY], b)
    l2 = 10 ** (np.asarray(train.last_history[0]) / 10)
    print(f"train(num_freq=16): loss {l1[0]:.4e} -> {l1[-1]:.4e}; resumed at {l2[0]:.4e} -> {l2[-1]:.4e}")
    assert abs(l2[0] - l1[-1]) < 0.5 * (l1[0] - l1[-1])
    # a checkpoint without the key draws a fresh encoding, as the reference does
    del ck[RFF_KEY]
    bare = os.path.join(exp, "bare.pt")
    torch.save(ck, bare)
    ck3 = train(exp, "c", "bach", 1, seed=99, prev_ckpt_path=bare, **dict(kw, total_steps=2))
    assert not torch.equal(torch.load(ck3, map_location="cpu", weights_only=True)[RFF_KEY], b)
