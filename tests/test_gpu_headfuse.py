"""The fused head backward (gemm_nt.hip NT_FWD_HB; SIREN_OPT_HEAD_FUSE, default on).

siren_train_step runs a sine last layer, the head (models.py:374-381), the MSE / L1 gradient
(run.py:161-169) and the head backward as ONE launch: the column tiles of a row band run in
lockstep on consecutive blocks and hand their head partials to each other (DESIGN §4 "fused
head backward").  Checked against the unfused launches (SIREN_OPT_HEAD_FUSE 0: the same loss,
outputs and dLoss/dout bit for bit, gradients to fp32 summation order) and against the oracle
with the fused path's backward scale (grad_scale_bound).  The NT tile is forced to 256 so that
4k-8k-row cases take the path; small persistent grids make every block walk many bands."""
import numpy as np
import pytest
import torch

from inr_for_audio_amd._lib import Opt, options
from errlog import check_grads, log
from gpu_util import grads as _grads, option_setter, rel as _rel
from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture
def opts(lib):
    """opts(Opt.X, v): set a knob for the rest of the test."""
    with option_setter(lib) as set_:
        yield set_


def _engine(dev, H, L, n, *, w0=3000.0, ll=True, loss="mse", mb=1 << 20, seed=0):
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(seed)
    model = SirenWithSnakeTanh(1, 1, H, L, 0, 0, last_linear=ll, first_omega_0=w0, hidden_omega_0=30.0)
    sd0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    y = 0.5 * torch.sin(37 * t) + 0.3 * torch.sin(91 * t + 0.5)
    eng = SirenEngine(model, t, y, micro_batch=mb, loss_mode=loss, device=dev)
    return eng, sd0, t, y


@pytest.mark.parametrize("H,L,n,grid,ll,loss,mb", [
    (1024, 4, 8192, 0, True, "mse", 1 << 20),    # 4 column tiles per band, 32 bands on 128 blocks
    (1024, 4, 8192, 8, True, "mse", 1 << 20),    # 2 band groups walking 16 bands each
    (1024, 4, 8000, 12, True, "mse", 1 << 20),   # pad rows (g = 0), 3 band groups
    (512, 3, 4096, 6, True, "mae", 1 << 20),     # L1Loss, 2 column tiles per band
    (256, 2, 4096, 0, False, "mse", 1 << 20),    # last_linear=False (final sine), 1 tile per band
    (1024, 2, 6000, 4, True, "mse", 2048),       # 3 micro-batches accumulating
])
def test_fused_matches_unfused(dev, lib, opts, H, L, n, grid, ll, loss, mb):
    opts(Opt.NT_TILE, 256)
    opts(Opt.NT_GRID, grid)
    eng, _, _, _ = _engine(dev, H, L, n, ll=ll, loss=loss, mb=mb)
    ga, oa, gga, ka = _grads(eng, lib)
    opts(Opt.HEAD_FUSE, 0)
    gb, ob, ggb, kb = _grads(eng, lib)
    # the fused path ran (one launch per micro-batch, no head_loss / head_bwd), the other did not
    assert ka["head_fwd"] == eng.n_micro and kb["head_fwd"] == 0
    assert ka["inner_fwd"] == (L - 1) * eng.n_micro and kb["inner_fwd"] == L * eng.n_micro
    assert ka["head"] == 2 * eng.n_micro and kb["head"] == 3 * eng.n_micro
    # head_loss's arithmetic on the same head partials: bit-identical outputs, dLoss/dout, loss
    assert torch.equal(oa, ob) and torch.equal(gga, ggb)
    sse = eng.layout.sse_offset
    assert torch.equal(ga[sse], gb[sse])
    lay = eng.layout
    errs = {k: _rel(lay.view(ga, i), lay.view(gb, i)) for i, k in enumerate(lay.names)}
    log(f"headfuse_vs_unfused[{H}x{L}x{n}x{grid}x{ll}x{loss}x{mb}]", errs=errs)
    # only the S of the dZ storage (a different power of two: bits differ only below fp16's normal
    # range) and the fp32 order of the db_L / dw_head column sums differ
    for k, e in errs.items():
        assert e < 2e-5, (k, e)


@pytest.mark.parametrize("H,L,n,ll,loss", [
    (1024, 4, 4000, True, "mse"),
    (512, 3, 4096, True, "mae"),
    (256, 2, 4096, False, "mse"),
])
def test_fused_vs_oracle(dev, lib, opts, H, L, n, ll, loss):
    opts(Opt.NT_TILE, 256)
    eng, sd0, t, y = _engine(dev, H, L, n, ll=ll, loss=loss)
    got_g, _, _, kinds = _grads(eng, lib)
    assert kinds["head_fwd"] == 1
    p = orc.Params.from_state_dict(sd0, L, 0, 0, False, ll)
    S = orc.grad_scale_bound(y.numpy(), n, p.wf, float(np.asarray(p.bf).reshape(-1)[0]), n, 30.0,
                             head_omega=p.head_omega, loss_mode=1 if loss == "mae" else 0)
    assert float(eng.ws.gscale[0]) == S and float(eng.ws.gscale[1]) == 1.0 / S
    out, cache = orc.forward(p, t.numpy(), 3000.0, 30.0, half=True, dtype=np.float64)
    gl = orc.l1_grad(out, y.numpy()) if loss == "mae" else orc.mse_grad(out, y.numpy())
    ref = orc.backward(p, t.numpy(), cache, gl, 3000.0, 30.0, half=True, scale=S)
    got = {k: eng.layout.view(got_g, i).cpu().numpy() for i, k in enumerate(eng.layout.names)}
    check_grads(f"headfuse_vs_oracle[{H}x{L}x{n}x{ll}x{loss}]", got, ref)
    lref = orc.l1(out, y.numpy()) if loss == "mae" else orc.mse(out, y.numpy())
    lgot = float(got_g[eng.layout.sse_offset]) / n
    assert abs(lgot - lref) <= 1e-4 * lref, (lgot, lref)


def test_fused_step_graph_and_determinism(dev, opts):
    """Eager steps, a captured step replayed, and a second engine: bit-identical parameters and
    losses (the hand-off's partial order is fixed, so no run-to-run drift)."""
    opts(Opt.NT_TILE, 256)
    a, _, _, _ = _engine(dev, 1024, 3, 8192)
    b, _, _, _ = _engine(dev, 1024, 3, 8192)
    for _ in range(4):
        a.step()
    b.step()
    b.capture_graph()
    for _ in range(3):
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    la, _ = a.history()
    lb, _ = b.history()
    assert np.array_equal(la, lb)


@pytest.mark.parametrize("H,R,n_valid,grid", [
    (1024, 4096, 4096, 0),
    (1024, 4096, 3000, 8),    # pad rows; 2 band groups walking 8 bands each
    (512, 2048, 2048, 2),
    (256, 2048, 1500, 0),
    (256, 2560, 2300, 3),     # width 256 (K = 256: 4 K-tiles), 10 bands on 3 blocks: walks of 4, 3, 3
])
def test_kernel_vs_unfused_launches(dev, lib, opts, H, R, n_valid, grid):
    """siren_head_fused_fwd against siren_inner_fwd (+ head) -> siren_head_loss -> siren_head_bwd
    with the same backward scale: outputs, dLoss/dout, the 256-row loss partials and the stored
    dZ_L bit-identical; the db_L / dw_head column partials (256- instead of 128-row blocks) agree
    to fp32 summation order."""
    import ctypes
    from inr_for_audio_amd._lib import new_tileq
    opts(Opt.NT_TILE, 256)
    opts(Opt.NT_GRID, grid)
    g_ = torch.Generator(device=dev).manual_seed(H + R)
    f16 = torch.float16
    P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    X = torch.sin(torch.rand(R, H, device=dev, generator=g_) * 6.2831853).to(f16)
    W = ((torch.rand(H, H, device=dev, generator=g_) * 2 - 1) * (6 / H) ** 0.5 / 30).to(f16)
    b = (torch.rand(H, device=dev, generator=g_) - 0.5) * 0.06
    wh = (torch.rand(H, device=dev, generator=g_) - 0.5) * 2 / H ** 0.5
    bh = torch.tensor([0.01], device=dev)
    y = (torch.rand(R, device=dev, generator=g_) - 0.5)
    gs = torch.tensor([2.0 ** 9, 2.0 ** -9], device=dev)
    e = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=dev)  # noqa: E731
    hp1, out1, g1, sse1, gsum1, dZ1, part1 = e(H // 256, R), e(R), e(R), e(R // 256), e(R // 256), e(R, H, dt=f16), \
        e(R // 256, 2, H)
    st = lib.siren_head_fused_fwd(P(X), P(W), P(b), ctypes.c_float(30.0), R, H, P(wh), P(bh), ctypes.c_float(0.0),
                                  P(y), n_valid, float(n_valid), 0, P(gs), P(hp1), P(out1), P(g1), P(sse1), P(gsum1),
                                  P(dZ1), P(part1), s)
    assert st == 0, lib.siren_status_string(st)
    Y, C, hp2 = e(R, H, dt=f16), e(R, H, dt=f16), e(H // 256, R)
    out2, g2, sse2, gsum2, dZ2 = e(R), e(R), e(R // 256), e(R // 256), e(R, H, dt=f16)
    db2, dw2 = e(R // 128, H), e(R // 128, H)
    tq = new_tileq(dev)
    for st in (lib.siren_inner_fwd(P(X), P(W), P(b), ctypes.c_float(30.0), R, H, P(Y), P(C), P(wh), P(hp2), P(tq), s),
               lib.siren_head_loss(P(hp2), H // 256, R, P(bh), P(y), n_valid, float(n_valid), P(out2), P(g2), P(sse2),
                                   P(gsum2), None, s),
               lib.siren_head_bwd(P(C), P(Y), P(g2), P(wh), ctypes.c_float(30.0), R, H, P(gs), P(dZ2), P(db2), P(dw2),
                                  None, None, s)):
        assert st == 0, lib.siren_status_string(st)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2) and torch.equal(g1, g2)
    assert torch.equal(sse1, sse2) and torch.equal(gsum1, gsum2)
    assert torch.equal(dZ1, dZ2)
    for got, ref in ((part1[:, 0].double().sum(0), db2.double().sum(0)), (part1[:, 1].double().sum(0),
                                                                          dw2.double().sum(0))):
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-12


def test_fused_head_needs_a_coresident_grid(dev, lib, opts):
    """The fused last layer's bands wait for each other's head partials, so its grid must be
    co-resident: a persistent grid larger than the device can hold (forced through
    SIREN_OPT_NT_GRID) is not fused -- siren_train_step falls back to the unfused launches and
    computes the same step; siren_head_fused_fwd refuses it with an error instead of launching."""
    import ctypes
    opts(Opt.NT_TILE, 256)
    eng, _, _, _ = _engine(dev, 1024, 2, 65536)   # 1 024 tiles of 256^2
    ga, oa, gga, ka = _grads(eng, lib)
    assert ka["head_fwd"] == 1
    opts(Opt.NT_GRID, 1024)                        # more blocks than CUs x occupancy (1 per CU)
    gb, ob, ggb, kb = _grads(eng, lib)
    assert kb["head_fwd"] == 0 and kb["inner_fwd"] == 2
    assert torch.equal(oa, ob) and torch.equal(gga, ggb)
    lay = eng.layout
    for i, k in enumerate(lay.names):
        assert _rel(lay.view(ga, i), lay.view(gb, i)) < 2e-5, k
    # the entry point itself: real buffers (a launch, were it to happen, would be well-formed)
    R, H = 65536, 1024
    P = lambda t: t.data_ptr()  # noqa: E731
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=dev)  # noqa: E731
    X, W, dZ = z(R, H, dt=torch.float16), z(H, H, dt=torch.float16), z(R, H, dt=torch.float16)
    b, wh, bh, y, gs = z(H), z(H), z(1), z(R), torch.tensor([1.0, 1.0], device=dev)
    hp, out, g, sse, gsum, part = z(H // 256, R), z(R), z(R), z(R // 256), z(R // 256), z(R // 256, 2, H)
    st = lib.siren_head_fused_fwd(P(X), P(W), P(b), ctypes.c_float(30.0), R, H, P(wh), P(bh), ctypes.c_float(0.0),
                                  P(y), R, float(R), 0, P(gs), P(hp), P(out), P(g), P(sse), P(gsum), P(dZ), P(part),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st != 0, "a grid larger than the device holds must not launch the fused kernel"


@pytest.mark.parametrize("cfg", ["sine", "snake"])
def test_handoff_timeout_voids_the_step(dev, monkeypatch, cfg):
    """A band partner that never publishes its head partial (SIREN_OPT_HB_FAULT bit 0, a hook of the
    -DSIREN_DIAG library: column tile 1 keeps its partial to itself; poll limit 64) drives the wait's
    timeout branch.  The step must fail loudly and leave the model untouched: the kernel counts the
    timeout in the guard's stall word (and in the reduced sse[1] slot), siren_apply_update skips Adam
    and the scheduler, and the engine raises SirenError at its next guard read.  Parameters, Adam
    moments and the optimizer state are bit-identical to before the step; no NaN reaches them.
    Cleared, the engine trains on normally (ADVICE r4 medium / VERDICT r4 item 4)."""
    import __graft_entry__ as ge
    from inr_for_audio_amd import _lib
    diag = _lib.bind(ge.DIAG_LIB, expect_build_id=_lib.expected_build_id(ge.DIAG_DEFINES))
    monkeypatch.setattr(_lib, "_lib", diag)  # the engine below runs on the SIREN_DIAG library
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(0)
    n = 65536  # 256 bands x 4 column tiles
    cfgs = {"sine": (2, 0, 0), "snake": (1, 1, 0)}
    model = SirenWithSnakeTanh(1, 1, 1024, *cfgs[cfg], first_omega_0=3000.0, hidden_omega_0=30.0)
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    y = 0.5 * torch.sin(37 * t)
    eng = SirenEngine(model, t, y, device=dev)
    assert eng.lib is diag
    eng.step()  # a normal step (a Snake last layer's first one is unfused)
    eng.step()  # ... fused from here on
    assert eng.steps_applied() == 2
    fused = eng.lib.siren_profile_enable(64) == 0
    before = [x.clone() for x in (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.state, eng.loss_hist)]
    try:
        with options(diag, {Opt.HB_FAULT: (64 << 8) | 1}):
            eng.step()
            torch.cuda.synchronize()
    finally:
        prof = _lib.profile_read()
        diag.siren_profile_enable(0)
    assert fused and prof["head_fwd"][1] == 1, prof  # the fused last layer ran
    with pytest.raises(_lib.SirenError, match="hand-off"):
        eng.steps_applied()
    after = (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.state, eng.loss_hist)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(eng.params).all())
    assert float(eng.grads[eng.layout.sse_offset + 1]) >= 1.0           # the reduced stall slot
    assert not bool(torch.isfinite(eng.ws.out).all())                     # the voided band's NaN
    g = eng.guard.cpu().tolist()
    assert g[5] >= 1 and g[3] == 0 and g[1] == 6                          # stalls; headroom untouched
    eng.clear_stalls()
    eng.step()
    assert eng.steps_applied() == 3
    assert bool(torch.isfinite(eng.params).all()) and not torch.equal(eng.params, before[0])
    log(f"handoff_timeout[{cfg}]", stalls=g[5])


def test_handoff_timeout_fails_fast(dev, monkeypatch):
    """Once one hand-off wait of a step has given up, every other wait of the step stops within
    kStallCheck (256) polls instead of spending its own whole limit: with the
    fault hook on and a 2^20-poll limit (~0.17 s per wait, tools/handoff_timeout.py), a step of 4
    micro-batches whose blocks each walk 4 bands per launch would otherwise wait 16 limits in a
    row (~2.7 s); it must come in under 4 limits.  The step is voided as in the test above."""
    import time
    import __graft_entry__ as ge
    from inr_for_audio_amd import _lib
    diag = _lib.bind(ge.DIAG_LIB, expect_build_id=_lib.expected_build_id(ge.DIAG_DEFINES))
    monkeypatch.setattr(_lib, "_lib", diag)
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(0)
    n = 4 * 16384  # 4 micro-batches of 64 bands x 4 column tiles
    model = SirenWithSnakeTanh(1, 1, 1024, 2, 0, 0, first_omega_0=3000.0, hidden_omega_0=30.0)
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    eng = SirenEngine(model, t, 0.5 * torch.sin(37 * t), micro_batch=16384, device=dev)
    assert eng.lib is diag and eng.n_micro == 4
    # 256 x 256 tiles at 16 384 rows (the fused path's tile); 16 blocks: each walks 16 band tiles per launch
    with options(diag, {Opt.NT_TILE: 256, Opt.NT_GRID: 16}):
        eng.step()
        torch.cuda.synchronize()
        fused = diag.siren_profile_enable(64 * eng.n_micro) == 0
        t0 = time.perf_counter()
        eng.step()
        torch.cuda.synchronize()
        clean = time.perf_counter() - t0
        prof = _lib.profile_read()
        diag.siren_profile_enable(0)
        assert fused and prof["head_fwd"][1] == eng.n_micro, prof  # the fused last layer runs per micro-batch
        limit = 1 << 20
        with options(diag, {Opt.HB_FAULT: (limit << 8) | 1}):
            t0 = time.perf_counter()
            eng.step()
            torch.cuda.synchronize()
            voided = time.perf_counter() - t0
    per_limit = limit * 0.16e-6
    with pytest.raises(_lib.SirenError, match="hand-off"):
        eng.steps_applied()
    log("handoff_fail_fast", clean_s=clean, voided_s=voided, per_limit_s=per_limit)
    assert voided < clean + 4 * per_limit, (voided, per_limit)
    eng.clear_stalls()
