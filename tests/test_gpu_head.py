"""head_loss_kernel in its four modes ({MSE, L1} x {linear head, final sine}) and siren_grad_scale_bound.

siren_head_loss exposes only MSE with a linear head; the other modes run inside siren_train_step when
SIREN_OPT_HEAD_FUSE is 0, and that call leaves the kernel's input (head_part, b_head) and all of its
outputs in the workspace.  The reference is fp64 arithmetic on the read-back head_part -- the kernel's
input, not its output: o = sum_j part_j + b.

Tolerances, u = 2^-24 (one fp32 rounding), all per element:
  o (linear head)   (nparts + 1) u (sum|part_j| + |b|)                       =: B_o
  a = omega o       omega B_o + |omega o| u                                  =: B_a
  out = sin a       B_a + EPS_SIN u
  g (MSE)           gfac (B_out [omega |cos a|] + |err| omega (B_a + EPS_COS u)) + 4 u |g|
  g (L1)            exactly +-fp32(1/N); through the final sine gfac omega (B_a + EPS_COS u) + 4 u |g|
  sse / gsum partials   16 u sum|terms| against the fp64 sum over the block's valid rows
EPS_SIN / EPS_COS are the only figures not derivable here: the error of the device library's sinf /
cosf at these arguments (|a| <= 40), measured on an MI355X against fp64 at 2^22 arguments uniform in
[-40, 40]: sinf 1.142 u, cosf 1.185 u (MEASURED_*); the gates are 4 x the measured value, rounded up
(4.57 -> 5 and 4.74 -> 5)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from inr_for_audio_amd._lib import Opt, options
from oracle import siren_oracle as orc
from gpu_util import ok, ptr, release, stream as S, to_dev

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
MEASURED_SIN, MEASURED_COS = 1.142, 1.185    # units of 2^-24, |a| <= 40
EPS_SIN = float(math.ceil(4 * MEASURED_SIN))    # 5
EPS_COS = float(math.ceil(4 * MEASURED_COS))    # 5
NAN = float("nan")


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


# ------------------------------------------------------------------ head_loss_kernel
N, H, L, W0 = 1000, 128, 2, 30.0


def _engine(dev, ll, loss):
    """A 2 x 128 SIREN on 1000 coordinates (rows = 1024: 24 pad rows); the targets are the CPU
    oracle's output +- a random offset in [0.01, 1], so |out - y| stays far above every tolerance
    and the L1 sign is determined on every row."""
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(0)
    model = SirenWithSnakeTanh(1, 1, H, L, 0, 0, last_linear=ll, first_omega_0=W0, hidden_omega_0=30.0)
    sd0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    t = torch.linspace(-1, 1, N).reshape(N, 1)
    p = orc.Params.from_state_dict(sd0, L, 0, 0, False, ll)
    out, _ = orc.forward(p, t.numpy(), W0, 30.0, half=True, dtype=np.float64)
    rng = np.random.default_rng(5)
    y = (out + rng.choice([-1.0, 1.0], N) * rng.uniform(0.01, 1.0, N)).astype(F32)
    eng = SirenEngine(model, t, torch.from_numpy(y), device=dev, loss_mode=loss)
    return eng, p.head_omega


def _run(eng, lib):
    with options(lib, {Opt.HEAD_FUSE: 0}):
        eng._launch_grads()
    torch.cuda.synchronize()
    ws = eng.ws
    host = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
    return {"part": host(ws.head_part), "b": host(eng.layout.view(eng.params, eng.ix["bh"])).reshape(-1)[0],
            "out": host(ws.out), "g": host(ws.g), "sse": host(ws.sse_part), "gsum": host(ws.gsum_part),
            "gmax": host(eng._gmax[0]), "y": host(eng.target)}


def _check(d, R, n_valid, nparts, omega, loss, zero_rows=()):
    """All of head_loss_kernel's outputs against fp64 from its inputs.  zero_rows: rows whose target
    was set to the device's own output bits -- err == 0 exactly there."""
    l1 = loss == "mae"
    part = d["part"].astype(np.float64)[:nparts]
    b = float(d["b"])
    o = part.sum(0) + b
    B_o = (nparts + 1) * U * (np.abs(part).sum(0) + abs(b))
    if omega > 0:
        a = omega * o
        B_a = omega * B_o + np.abs(a) * U
        out64, B_out = np.sin(a), B_a + EPS_SIN * U
    else:
        out64, B_out = o, B_o
    e_out = np.abs(d["out"].astype(np.float64) - out64)
    print(f"head_loss {loss} omega={omega}: out err/bound {float((e_out / B_out).max()):.3f}")
    assert np.all(e_out <= B_out)

    valid = np.arange(R) < n_valid
    zero = np.zeros(R, bool)
    zero[list(zero_rows)] = True
    gfac = float(F32((1.0 if l1 else 2.0) / N))
    err = np.where(valid & ~zero, out64 - d["y"].astype(np.float64), 0.0)
    assert np.all(np.abs(err[valid & ~zero]) > 1e3 * B_out[valid & ~zero])      # the sign is determined
    lin = np.sign(err) if l1 else err
    chain = omega * np.cos(a) if omega > 0 else 1.0
    g64 = gfac * lin * chain
    tol = 4 * U * np.abs(g64)
    if not l1:
        tol = tol + gfac * B_out * np.abs(chain)
    if omega > 0:
        dc = B_a + EPS_COS * U
        tol = tol + gfac * omega * dc * (np.abs(lin) + (0.0 if l1 else B_out))
    g = d["g"]
    e_g = np.abs(g.astype(np.float64) - g64)
    live = valid & ~zero
    print(f"head_loss {loss} omega={omega}: g err/bound {float((e_g[live] / tol[live]).max()):.3f}")
    assert np.all(e_g[live] <= tol[live])
    if l1 and omega == 0:
        want = (np.sign(err) * np.float64(F32(1.0 / N))).astype(F32)
        assert np.array_equal(g[live].view(np.uint32), want[live].view(np.uint32))
    assert not g[~valid].view(np.uint32).any()                  # pad rows: exact +0
    assert np.all(g[zero] == 0.0)                               # sign(0) = 0, err = 0

    nb = (R + 255) // 256
    terms = np.abs(err) if l1 else err * err
    for name, got, tm in (("sse", d["sse"], terms), ("gsum", d["gsum"], g64)):
        tb = tm.reshape(nb, 256)
        e = np.abs(got.astype(np.float64) - tb.sum(1))
        bound = 16 * U * np.abs(tb).sum(1)
        ratio = float(np.max(e[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
        print(f"head_loss {loss} omega={omega}: {name} partial err/bound {ratio:.3f}")
        assert np.all(e <= bound), name
        empty = ~valid.reshape(nb, 256).any(1)
        assert not got[empty].view(np.uint32).any(), name        # a block of pad rows only: exact zeros
    gmax = np.abs(g).reshape(nb, 256).max(1)
    assert np.array_equal(d["gmax"].view(np.uint32), gmax.view(np.uint32))


@pytest.mark.parametrize("n_valid", [1000, 700], ids=["pad24", "padblock"])
@pytest.mark.parametrize("ll", [True, False], ids=["linear", "sine"])
@pytest.mark.parametrize("loss", ["mse", "mae"])
def test_head_loss_modes(lib, dev, loss, ll, n_valid):
    """n_valid 1000 ends inside the last 256-row block; 700 leaves that block all pad rows."""
    eng, omega = _engine(dev, ll, loss)
    assert (omega > 0) == (not ll)
    R = eng.rows
    assert R == 1024 and eng.n_micro == 1
    nparts = H // int(lib.siren_nt_tile(R, H))
    eng.batches[0].n_valid = n_valid
    for buf in (eng.ws.out, eng.ws.g, eng.ws.sse_part, eng.ws.gsum_part, eng._gmax, eng.ws.head_part):
        buf.fill_(NAN)
    first = _run(eng, lib)
    _check(first, R, n_valid, nparts, omega, loss)
    # the sign(0) branch: the step is deterministic, so a target equal to the first run's output bits
    # makes err exactly 0 on those rows -- g = 0 in both loss modes, nothing added to the partials
    rows = [0, 1, 63, 64, 255, 256, 257, 300, 511, 512, 600, 650, 690, 697, 698, n_valid - 1]
    assert len(set(rows)) == 16 and max(rows) < n_valid
    idx = torch.tensor(rows, device=dev)
    eng.target[idx] = eng.ws.out[idx]
    second = _run(eng, lib)
    assert np.array_equal(second["out"].view(np.uint32), first["out"].view(np.uint32))
    _check(second, R, n_valid, nparts, omega, loss, zero_rows=rows)


# ------------------------------------------------------------------ siren_grad_scale_bound
N_TOTAL = 5000.0
ACT_BOUND = 30.0


def _bound64(y, n_valid, w, b, head_omega, loss_mode):
    gfac = (1.0 if loss_mode == 1 else 2.0) / N_TOTAL
    ym = float(np.abs(y[:n_valid]).max()) if n_valid else 0.0
    wa = np.abs(w.astype(np.float64))
    gb = gfac if loss_mode == 1 else gfac * ((1.0 if head_omega > 0 else wa.sum() + abs(float(b))) + ym)
    if head_omega > 0:
        gb *= head_omega
    return gb * wa.max() * ACT_BOUND * (1.0 + 2.0 ** -10), gb


def _bound_inputs(n_valid, Hh, head_omega, loss_mode):
    """Inputs whose fp64 bound has a frexp mantissa in [0.55, 0.95]: its octave cannot then depend
    on the order of the fp32 sums.  A target of 1e6 sits at row n_valid, which the maximum over the
    n_valid rows must not see."""
    rows = (n_valid // 256 + 2) * 256
    for seed in range(1000):
        rng = np.random.default_rng(1000 * n_valid + seed)
        y = (rng.normal(size=rows) * 0.7).astype(F32)
        y[n_valid] = 1e6
        w = rng.uniform(-1, 1, Hh).astype(F32) * F32(10.0 ** rng.uniform(-3, 0))
        b = F32(rng.uniform(-0.5, 0.5))
        bound, _ = _bound64(y, n_valid, w, b, head_omega, loss_mode)
        if 0.55 <= math.frexp(bound)[0] <= 0.95:
            return y, w, b, bound
    raise AssertionError("no input found")


@pytest.mark.parametrize("Hh", [128, 1024])
@pytest.mark.parametrize("n_valid", [0, 1, 255, 256, 257, 1000])
@pytest.mark.parametrize("head_omega", [0.0, 30.0])
@pytest.mark.parametrize("loss_mode", [0, 1])
def test_grad_scale_bound(lib, dev, loss_mode, head_omega, n_valid, Hh):
    y, w, b, bound = _bound_inputs(n_valid, Hh, head_omega, loss_mode)
    nb = (n_valid + 255) // 256
    ymax = torch.full((nb + 2,), NAN, device=dev)
    gscale = torch.full((4,), NAN, device=dev)
    ok(lib.siren_grad_scale_bound(ptr(to_dev(y, dev)), n_valid, ptr(ymax), ptr(to_dev(w, dev)),
                                  ptr(to_dev(np.array([b], F32), dev)), Hh, ctypes.c_double(N_TOTAL),
                                  ctypes.c_float(head_omega), loss_mode, ctypes.c_float(ACT_BOUND), ptr(gscale),
                                  S()), lib)
    gs = gscale.cpu().numpy()
    S_dev, inv = float(gs[0]), float(gs[1])
    assert np.isnan(gs[2:]).all()
    # gscale is exactly {2^k, 2^-k}
    assert math.frexp(S_dev)[0] == 0.5 and S_dev * inv == 1.0 and math.frexp(inv)[0] == 0.5
    e = math.frexp(bound)[1]                                    # bound in [2^(e-1), 2^e)
    assert S_dev == 2.0 ** (6 - e)
    assert S_dev == orc.grad_scale_bound(y, n_valid, w, float(b), N_TOTAL, ACT_BOUND, head_omega, loss_mode)
    # the per-256-row maxima of |y| over the n_valid rows, nothing after them
    ym = ymax.cpu().numpy()
    pad = np.zeros(nb * 256, F32)
    pad[:n_valid] = np.abs(y[:n_valid])
    assert np.array_equal(ym[:nb].view(np.uint32), pad.reshape(nb, 256).max(1).view(np.uint32))
    assert np.isnan(ym[nb:]).all()

    # the guarantee: whatever the forward produces within its range, the scaled dZ_L bound stays
    # below 2^6.  |out| <= sum|w| + |b| (<= 1 under the final sine); the worst case is out at that
    # limit with the sign against the largest target, and cos = 1 through the final sine.
    if n_valid == 0:
        return
    rng = np.random.default_rng(7)
    wa = np.abs(w.astype(np.float64))
    lim = 1.0 if head_omega > 0 else wa.sum() + abs(float(b))
    yv = y[:n_valid].astype(np.float64)
    gfac = (1.0 if loss_mode == 1 else 2.0) / N_TOTAL
    worst = 0.0
    for out in (rng.uniform(-lim, lim, n_valid), np.full(n_valid, lim), np.full(n_valid, -lim), -np.sign(yv) * lim):
        err = out - yv
        g = gfac * (np.sign(err) if loss_mode == 1 else err)
        if head_omega > 0:
            g = g * head_omega                                  # |cos| <= 1
        worst = max(worst, float(np.abs(g).max()))
    assert worst * wa.max() * ACT_BOUND * S_dev < 2.0 ** 6
