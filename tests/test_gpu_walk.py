"""Multi-tile walks of the persistent 256 x 256 ping-pong NT GEMM, in every epilogue mode.

The production kernel (gemm_nt.hip, NtLargePP) runs min(tiles, CUs) persistent blocks, each
walking several tiles with the LDS ring, the epilogue scratch (NtLds LINES / HALF / RED / EARLY)
and the next tile's prefetch running across tile boundaries: 441 000 x 256 is 1723 tiles on 256
blocks, about 7 per block, at the shortest K loop (K = 256, four K-tiles).  A race or a stale
scratch read there shows only from the second tile a block computes.

Kernel level (test_walk_*): a tile's arithmetic does not depend on which block computes it or
when, so with SIREN_OPT_NT_TILE 256 and the automatic pipe every output of a launch is
bit-identical for every SIREN_OPT_NT_GRID; the flat launch (grid 0: one tile per block here) also
meets the fp64 bounds of the per-kernel tests (kernel_ref.py: the same definitions).  Together
these put the deep walks within those bounds.  R = 2560 rows (10 row bands):

    H     tiles  grids (tiles per block)
    256   10     0 (1 each), 3 (4, 3, 3), 5 (2 each)
    512   20     0, 6 (4, 4, 3, 3, 3, 3), 3 (7, 7, 6)
    1024  40     0, 7 (6 x5, 5 x2), 16 (3 x8, 2 x8)

Every output buffer is pre-filled with NaN before every launch and whole buffers are compared,
so an element a walk failed to write, or wrote outside its tile, fails.

Step level: the whole fused step at width 256 on the forced 256-tile kernels with a grid of 3
against the fp16-storage oracle (the reference's live stack, run.py:466, train()'s default stack
and a first_linear / last_linear=False stack, which reaches NT_DX0_SNAKE), and the tile queue in
every mode (SIREN_OPT_NT_QUEUE 0 / 1 / 2) on Snake / Tanh stacks.
"""
import ctypes

import numpy as np
import pytest
import torch

from inr_for_audio_amd._lib import Opt, options
from oracle import siren_oracle as orc
from errlog import check_grads, log
from gpu_util import grads as _grads, ok, option_setter, ptr, release, stream as S, to_dev
from kernel_ref import (SNAKE, TANH, act_inputs, check_first_bwd_dx, check_inner_bwd_dx, check_inner_bwd_dx_act,
                        check_inner_fwd, check_inner_fwd_act, first_difference, inner_inputs, same_bits, unwritten)

gpu = pytest.mark.gpu

F32 = np.float32
H16 = torch.float16
R = 2560
GRIDS = {256: (0, 3, 5), 512: (0, 6, 3), 1024: (0, 7, 16)}
WIDTHS = sorted(GRIDS)


@pytest.fixture
def walk(lib, dev):
    """walk(H, launch): run launch() -- which allocates its NaN-filled outputs, launches and returns
    (every output buffer, the parts of them the launch owns) -- once per grid of GRIDS[H] on the
    256 x 256 tiles with the automatic pipe; every deep walk must leave the bits of the flat launch
    in every buffer, and the flat launch must have written all it owns.  Returns the flat
    launch's buffers for the fp64 check."""
    def run(H, launch):
        flat = None
        for grid in GRIDS[H]:
            with options(lib, {Opt.NT_TILE: 256, Opt.NT_GRID: grid}):
                assert lib.siren_nt_tile(R, H) == 256
                bufs, owned = launch()
                torch.cuda.synchronize()
            holes = unwritten(owned)
            assert holes == [], (grid, holes)
            if flat is None:
                flat = bufs
            else:
                diff = first_difference(bufs, flat)  # (buffer, element, deep walk's value, flat launch's)
                assert diff is None, (grid, diff)
        return flat
    yield run
    release()


def nans(dev, *shape, dtype=H16):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def f16_np(t):
    return t.float().cpu().numpy().astype(np.float64)


def gscale_dev(dev, k):
    """{S, 1/S} with S = 2^k, or None (NULL: unscaled)."""
    return None if k is None else to_dev(np.array([2.0 ** k, 2.0 ** -k], F32), dev)


# ------------------------------------------------------------------ 1. per mode
@gpu
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("H", WIDTHS)
def test_walk_inner_fwd(lib, dev, walk, H, head):
    rng = np.random.default_rng(2)
    X, W, b = inner_inputs(rng, R, H)
    Wh = orc.f16_round(W)
    hw = rng.uniform(-0.01, 0.01, H).astype(F32)
    Xd, Wd, bd, hwd = to_dev(X, dev, H16), to_dev(Wh, dev, H16), to_dev(b, dev), to_dev(hw, dev)

    def launch():
        Y, C, hp = nans(dev, R, H), nans(dev, R, H), nans(dev, H // 128, R, dtype=torch.float32)
        ok(lib.siren_inner_fwd(ptr(Xd), ptr(Wd), ptr(bd), ctypes.c_float(30.0), R, H, ptr(Y), ptr(C),
                               ptr(hwd) if head else None, ptr(hp) if head else None, None, S()), lib)
        # the 256-tile launches write H/256 partial rows; the rest stays NaN in every run
        return [Y, C, hp], [Y, C] + ([hp[:H // 256]] if head else [])
    Y, C, hp = walk(H, launch)
    check_inner_fwd(f16_np(Y), f16_np(C), hp[:H // 256].cpu().numpy() if head else None, X, Wh, b, hw)


@gpu
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("act,amag", [(SNAKE, 0.5), (SNAKE, 50.0), (TANH, 0.5)])
@pytest.mark.parametrize("H", WIDTHS)
def test_walk_inner_fwd_act(lib, dev, walk, H, act, amag, head):
    """H <= 512 without the head partials takes the whole-line epilogue (ACTL; the Snake with them
    the 8-row passes, HALF), H = 1024 the plain path; a = 50 is the reference's __main__ value."""
    rng = np.random.default_rng(21)
    X, W, b = act_inputs(rng, R, H)
    a = (amag * rng.uniform(0.5, 1.5, H)).astype(F32)
    hw = rng.uniform(-0.01, 0.01, H).astype(F32)
    Xd, Wd, bd = to_dev(X, dev, H16), to_dev(W, dev, H16), to_dev(b, dev)
    ad, hwd = to_dev(a, dev), to_dev(hw, dev)

    def launch():
        Y, C, E = nans(dev, R, H), nans(dev, R, H), nans(dev, R, H)
        hp = nans(dev, H // 128, R, dtype=torch.float32)
        ok(lib.siren_inner_fwd_act(ptr(Xd), ptr(Wd), ptr(bd), act, ctypes.c_float(30.0), ptr(ad), R, H, ptr(Y),
                                   ptr(C), ptr(E), ptr(hwd) if head else None, ptr(hp) if head else None, None,
                                   S()), lib)
        # E is the Snake's alone: a Tanh launch must leave it untouched (NaN in every run)
        return [Y, C, E, hp], [Y, C] + ([E] if act == SNAKE else []) + ([hp[:H // 256]] if head else [])
    Y, C, E, hp = walk(H, launch)
    if act == TANH:
        assert bool(torch.isnan(E).all())
    check_inner_fwd_act(act, f16_np(Y), f16_np(C), f16_np(E), hp[:H // 256].cpu().numpy() if head else None,
                        X, W, b, a, hw, amag)


@gpu
@pytest.mark.parametrize("k", [None, 9])
@pytest.mark.parametrize("H", WIDTHS)
def test_walk_inner_bwd_dx(lib, dev, walk, H, k):
    """The db column sums run over 2560 rows here (256-768 in test_inner_bwd_dx); their tolerance
    is relative to the largest column sum, which grows with the rows as the fp32 error does."""
    rng = np.random.default_rng(5)
    dZ = orc.f16_round((rng.normal(size=(R, H)) * 1e-3).astype(F32))
    _, W, _ = inner_inputs(rng, R, H)
    Wh = orc.f16_round(W)
    Cp = orc.f16_round(rng.uniform(-1, 1, (R, H)).astype(F32))
    dZd, WTd, Cd = to_dev(dZ, dev, H16), to_dev(np.ascontiguousarray(Wh.T), dev, H16), to_dev(Cp, dev, H16)
    gs = gscale_dev(dev, k)

    def launch():
        out, dbp = nans(dev, R, H), nans(dev, R // 128, H, dtype=torch.float32)
        ok(lib.siren_inner_bwd_dx(ptr(dZd), ptr(WTd), ptr(Cd), ctypes.c_float(30.0), R, H, ptr(gs), ptr(out),
                                  ptr(dbp), S()), lib)
        return [out, dbp], [out, dbp[:R // 256]]
    out, dbp = walk(H, launch)
    check_inner_bwd_dx(f16_np(out), dbp[:R // 256].cpu().numpy(), dZ, Wh, Cp, k, tag=f"walk_dx[{H},{k}]")


@gpu
@pytest.mark.parametrize("act", [SNAKE, TANH])
@pytest.mark.parametrize("H,k", [(256, None), (512, 9), (1024, 3)])
def test_walk_inner_bwd_dx_act(lib, dev, walk, H, k, act):
    """dX into a Snake layer (whole-line stores, ACTL, at H <= 512) with the db / da partials, and
    into a Tanh layer (NT_DX with omega 1).  Column sums over 2560 rows: as test_walk_inner_bwd_dx,
    the tolerances are test_inner_bwd_dx_act's, which scale with sqrt(rows) and the column sums."""
    rng = np.random.default_rng(22)
    dZ = orc.f16_round((rng.normal(size=(R, H)) * 1e-3).astype(F32))
    _, W, _ = act_inputs(rng, R, H)
    D = orc.f16_round(rng.uniform(0, 2, (R, H)).astype(F32))
    Ep = orc.f16_round(rng.normal(size=(R, H)).astype(F32))
    dZd, WTd = to_dev(dZ, dev, H16), to_dev(np.ascontiguousarray(W.T), dev, H16)
    Dd, Ed = to_dev(D, dev, H16), to_dev(Ep, dev, H16)
    gs = gscale_dev(dev, k)
    nrow = R // 256

    def written(part):  # Snake [R/256][2][H] (db, da), Tanh [R/256][H] (db), from the buffer's start
        return part[:nrow] if act == SNAKE else part.reshape(-1)[:nrow * H].reshape(nrow, H)

    def launch():
        out, part = nans(dev, R, H), nans(dev, R // 128, 2, H, dtype=torch.float32)
        ok(lib.siren_inner_bwd_dx_act(ptr(dZd), ptr(WTd), ptr(Dd), ptr(Ed) if act == SNAKE else None, act,
                                      ctypes.c_float(30.0), R, H, ptr(gs), ptr(out), ptr(part), S()), lib)
        return [out, part], [out, written(part)]
    out, part = walk(H, launch)
    check_inner_bwd_dx_act(act, f16_np(out), written(part).cpu().numpy(), dZ, W, D, Ep, k,
                           tag=f"walk_dx_act[{H},{k},{act}]")


@gpu
@pytest.mark.parametrize("in_dim,omega0", [(1, 22000.0), (2, 1000.0)])
@pytest.mark.parametrize("H", WIDTHS)
def test_walk_first_bwd_dx(lib, dev, walk, H, in_dim, omega0):
    """dX0 (EARLY: the next tile's first K-tile is staged before this tile's partial stores); its
    only outputs are the column partials of dZ0 and dZ0 t_j.  test_first_bwd_dx's tolerance is
    relative to max|dZ0| sqrt(rows)."""
    rng = np.random.default_rng(6)
    k = 5 if in_dim == 2 else None
    dZ1 = orc.f16_round((rng.normal(size=(R, H)) * 1e-3).astype(F32))
    _, W, _ = inner_inputs(rng, R, H)
    Wh = orc.f16_round(W)
    t = rng.uniform(-1, 1, (R, in_dim)).astype(F32)
    W0 = rng.uniform(-1 / in_dim, 1 / in_dim, (H, in_dim)).astype(F32)
    b0 = rng.uniform(-1, 1, H).astype(F32)
    C0 = orc.f16_round(orc.cos32(orc.first_preact(t, W0, b0, omega0)))  # as siren_first_fwd stores it
    dZd, WTd = to_dev(dZ1, dev, H16), to_dev(np.ascontiguousarray(Wh.T), dev, H16)
    Cd, td = to_dev(C0, dev, H16), to_dev(t, dev)
    gs = gscale_dev(dev, k)

    def launch():
        part = nans(dev, R // 128, 1 + in_dim, H, dtype=torch.float32)
        ok(lib.siren_first_bwd_dx(ptr(dZd), ptr(WTd), ptr(Cd), ptr(td), in_dim, ctypes.c_float(omega0), R, H,
                                  ptr(gs), ptr(part), S()), lib)
        return [part], [part[:R // 256]]
    part, = walk(H, launch)
    check_first_bwd_dx(part[:R // 256].cpu().numpy(), dZ1, Wh, C0, t, omega0, k, tag=f"walk_dx0[{H},{in_dim}]")


# ------------------------------------------------------------------ 3. whole step, width 256
def _model(H, cfg, a0, in_dim=1, fl=False, ll=True, seed=0):
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(seed)
    return SirenWithSnakeTanh(in_dim, 1, H, *cfg, first_linear=fl, last_linear=ll, first_omega_0=1000.0,
                              hidden_omega_0=30.0, a_initial=a0)


def _signal(n, in_dim=1):
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    if in_dim == 2:
        ch = torch.where(torch.arange(n) % 2 == 0, -1.0, 1.0).reshape(n, 1)
        t = torch.cat([t, ch], 1)
    y = 0.5 * torch.sin(37 * t[:, :1]) + 0.3 * torch.sin(91 * t[:, :1] + 0.5)
    return t, y


@gpu
@pytest.mark.parametrize("cfg,a0,in_dim,fl,ll", [
    ((0, 4, 0), 50.0, 1, False, True),    # the reference's __main__ run (run.py:466)
    ((2, 2, 0), 0.5, 1, False, True),     # run.py train() default architecture
    ((1, 1, 1), 0.5, 2, True, False),     # Linear + Snake first, final SineLayer: NT_DX0_SNAKE
])
def test_step_width_256_on_production_kernels(lib, dev, cfg, a0, in_dim, fl, ll):
    """The fused step at width 256 on the 256 x 256 NT and TN kernels with 3 persistent blocks (10
    row bands: walks of 4, 3 and 3 tiles; 2500 coordinates, so 60 pad rows carry g = 0) against the
    fp16-storage oracle.  A Snake last layer runs unfused on its first launch and fused with the
    head on the second, which is compared at the scale it used."""
    from inr_for_audio_amd.engine import SirenEngine
    n, H = 2500, 256
    with option_setter(lib) as set_:
        set_(Opt.NT_TILE, 256)
        set_(Opt.TN_TILE, 256)
        set_(Opt.NT_GRID, 3)
        model = _model(H, cfg, a0, in_dim, fl, ll)
        sd0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
        t, y = _signal(n, in_dim)
        eng = SirenEngine(model, t, y, lr=1e-3, device=dev)
        assert eng.rows == R and lib.siren_nt_tile(eng.rows, H) == 256 and lib.siren_dw_tile(eng.rows, H) == 256
        snake_last = cfg[2] == 0 and cfg[1] > 0
        launches = [_grads(eng, lib)]
        if snake_last:
            launches.append(_grads(eng, lib))
            assert launches[0][3]["head_fwd"] == 0 and launches[1][3]["head_fwd"] == 1
            S_fused = float(eng.ws.gscale[0])
            g_fused = eng.ws.g.cpu().numpy()
        eng.step()  # the same weights again (nothing was applied yet): the loss of step 0
        torch.cuda.synchronize()
    p = orc.Params.from_state_dict(sd0, *cfg, fl, ll)
    out, cache = orc.forward(p, t.numpy(), 1000.0, 30.0, half=True, dtype=np.float64)
    gl = orc.mse_grad(out, y.numpy())
    name = f"walk_step[{cfg}x{in_dim}x{fl}x{ll}]"
    views = lambda g: {k: eng.layout.view(g, i).cpu().numpy() for i, k in enumerate(eng.layout.names)}  # noqa: E731
    ref = orc.backward(p, t.numpy(), cache, gl, 1000.0, 30.0, half=True)
    got = views(launches[0][0])
    assert set(ref) == set(got)
    check_grads(name, got, ref)
    if snake_last:
        # grad_scale on the previous launch's max|g| (= this launch's: no update in between)
        assert S_fused == orc.grad_scale(g_fused, p.wf, 2.0)
        ref = orc.backward(p, t.numpy(), cache, gl, 1000.0, 30.0, half=True, scale=S_fused)
        check_grads(name + "fused", views(launches[1][0]), ref)
    out32, _ = orc.forward(p, t.numpy(), 1000.0, 30.0)
    l32 = orc.mse(out32, y.numpy())
    log(name + "loss", loss=abs(eng.last_loss() - l32) / l32)
    assert abs(eng.last_loss() - l32) < 5e-4 * l32


# ------------------------------------------------------------------ 4. the queue in every mode
@gpu
@pytest.mark.parametrize("cfg,a0,fl", [((1, 2, 1), 0.5, True), ((0, 4, 0), 50.0, False)])
def test_queue_every_mode_on_act_stacks(lib, dev, cfg, a0, fl):
    """SIREN_OPT_NT_QUEUE 2 sends the dX / dX0 launches of siren_train_step through the batch's
    counter set as well (the backward C-ABI entry points take none), 1 the forward modes only, 0
    none: on Snake / Tanh stacks at width 256 (16 tiles on 8 blocks: the queue kernel runs, two
    tiles per block) the step's gradients are bit-identical across the three, on the first launch
    and on the second, where a Snake last layer runs fused with the head."""
    from inr_for_audio_amd.engine import SirenEngine
    n, H = 4096, 256
    runs = []
    for q in (0, 1, 2):
        with options(lib, {Opt.NT_TILE: 256, Opt.NT_GRID: 8, Opt.NT_QUEUE: q}):
            t, y = _signal(n)
            eng = SirenEngine(_model(H, cfg, a0, fl=fl), t, y, device=dev)
            assert lib.siren_nt_tile(eng.rows, H) == 256
            first, second = _grads(eng, lib), _grads(eng, lib)
            assert second[3]["head_fwd"] == 1
            runs.append([first[0], first[1], first[2], second[0], second[1], second[2]])
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][3]).all())
    for q in (1, 2):
        diff = first_difference(runs[q], runs[0])
        assert diff is None, (q, diff)


# ------------------------------------------------------------------ 5. the comparison itself (host)
def test_bit_identity_helper_reports_one_ulp_and_one_nan():
    """The walk tests stand on first_difference / unwritten: two buffer lists as test_walk_* hold
    them (fp16 outputs and fp32 partials with their unwritten rows still NaN on both sides) compare
    equal; one fp16 ulp in one element of one tile, or one element left NaN, is reported."""
    g = torch.Generator().manual_seed(0)
    Y = torch.rand(512, 256, generator=g).to(H16)
    part = torch.full((4, 256), float("nan"))
    part[:2] = torch.rand(2, 256, generator=g)
    a, b = [Y, part], [Y.clone(), part.clone()]
    assert same_bits(a, b) and first_difference(a, b) is None
    assert unwritten([Y, part[:2]]) == [] and unwritten([Y, part]) == [1]
    ulp = Y.clone()
    at = 300 * 256 + 17     # row 300, column 17: inside the second 256-row tile
    ulp.view(torch.int16).reshape(-1)[at] += 1
    assert abs(float(ulp.reshape(-1)[at]) - float(Y.reshape(-1)[at])) <= 2.0 ** -11
    d = first_difference([ulp, part], b)
    assert not same_bits([ulp, part], b) and d is not None and d[:2] == (0, at)
    hole = Y.clone()
    hole.reshape(-1)[at] = float("nan")
    d = first_difference([hole, part], b)
    assert not same_bits([hole, part], b) and d[:2] == (0, at)
    assert unwritten([hole, part[:2]]) == [0]
    lost = part.clone()
    lost[1, 5] = float("nan")     # a partial a walk skipped
    assert first_difference([Y, lost], b)[:2] == (1, 256 + 5) and unwritten([Y, lost[:2]]) == [1]
