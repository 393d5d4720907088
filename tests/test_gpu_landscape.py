"""The loss-landscape plane on the device (run.py:192-208, visualization=True; csrc/plane.hip):
siren_plane_point bit for bit, SirenEngine.loss_plane against the engine's own infer() and against the
fp64 formula of landscape_ref.py, no side effects on a running fit, and train(visualization=True)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import errlog
import landscape_ref as ref
from gpu_util import ok, ptr, release, stream
from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = np.float32, np.float64

# loss_plane against host fp64 MSE of the same kernels' outputs: only the fp32 block sums of at most 256
# non-negative terms differ (worst case 255 * 2^-24 = 1.5e-5; across blocks the sum is fp64)
SELF_GATE = 2e-5
# loss_plane against the fp64 formula: DESIGN 3's loss gates, 1e-4 for sine stacks and 5e-4 for Snake / Tanh
# stacks.  last_linear=False misses the sine gate at the far cells: measured worst 2.98e-4 (5-step grid, weights
# up to three times theta's; 1.97e-4 on the 4-step grid), where the half=True oracle is 2.88e-4 (1.82e-4) from
# fp64 on the same cell -- the fp16 storage's own error, which the final SineLayer's omega = 30 multiplies --
# so its gate is 4 x the measured worst
GATE = {"sine": 1e-4, "default": 5e-4, "tanh": 5e-4, "sinehead": 1.2e-3}


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


def _model(in_dim, H, ns, nk, nt, seed=0, **kw):
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(seed)
    return SirenWithSnakeTanh(in_dim, 1, H, ns, nk, nt, first_omega_0=kw.pop("w0", 1000.0), hidden_omega_0=30.0,
                              a_initial=0.5, **kw)


# ------------------------------------------------------------------ siren_plane_point
# name: (in_features, hidden, num_sine, num_snake, num_tanh, model kwargs)
POINT_CASES = {
    "h128_1": (1, 128, 1, 0, 0, {}),
    "h128_3": (1, 128, 1, 1, 1, {}),
    "h100_pad": (1, 100, 1, 2, 0, {}),            # padded to 128: zero pads, Snake a pads at 1
    "in2": (2, 128, 2, 0, 0, {}),
    "rff3": (6, 128, 1, 1, 0, {}),                # W0 [H][2 F], F = 3
    "first_linear": (1, 128, 1, 1, 0, {"first_linear": True}),
    "h1100_pad": (1, 1100, 1, 0, 0, {}),          # padded to 2048
}
AB = [(0.0, 0.0), (-2.5, 1.5), (3.0, -2.0)]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


@pytest.mark.parametrize("case", list(POINT_CASES))
def test_plane_point_bit_for_bit(lib, dev, case):
    from inr_for_audio_amd.engine import ParamLayout
    in_dim, H, ns, nk, nt, kw = POINT_CASES[case]
    model = _model(in_dim, H, ns, nk, nt, **kw)
    lay, ix, Hp, L = ParamLayout(model, model.hip_padding()), model.param_index(), model.hip_width(), ns + nk + nt
    g = torch.Generator().manual_seed(3)
    theta = torch.zeros(lay.flat_len)
    lay.fill_pads(theta)
    d1, d2 = torch.zeros(lay.flat_len), torch.zeros(lay.flat_len)
    for i in range(len(lay.names)):       # N(0, 1) in every true entry; pads and gaps as the engine's
        for v in (theta, d1, d2):
            lay.true_view(v, i).copy_(torch.randn(lay.true_shapes[i], generator=g))
    if H != Hp:   # the pads this case is about
        if nk:
            a_pad = lay.view(theta, ix["a"][1])
            assert float(a_pad[H:].min()) == 1.0 and float(a_pad[H:].max()) == 1.0
        assert not lay.view(theta, ix["W"][0])[H:].any() and not lay.view(d1, ix["W"][0])[:, H:].any()
    pads = torch.ones(lay.flat_len, dtype=torch.bool)     # pad entries and alignment gaps: outside every true view
    for i in range(len(lay.names)):
        lay.true_view(pads, i).zero_()
    pads = pads.numpy() & (np.arange(lay.flat_len) < lay.n_params)
    assert not d1.numpy()[pads].any() and not d2.numpy()[pads].any()
    T, D1, D2 = theta.to(dev), d1.to(dev), d2.to(dev)
    nan32 = lambda n: torch.full((n,), float("nan"), device=dev)  # noqa: E731
    nan16 = lambda: torch.full((Hp, Hp), float("nan"), dtype=torch.float16, device=dev)  # noqa: E731
    arr = lambda ts: (ctypes.c_void_p * L)(*[ptr(t) for t in ts])  # noqa: E731
    for a, b in AB:
        out = nan32(lay.flat_len)
        Wh, WTh = [nan16() for _ in range(L)], [nan16() for _ in range(L)]
        Wout = [lay.view(out, k) for k in ix["W"]]
        ok(lib.siren_plane_point(ptr(T), ptr(D1), ptr(D2), a, b, ptr(out), lay.n_params, Hp, L, arr(Wout), arr(Wh),
                                 arr(WTh), stream()), lib)
        torch.cuda.synchronize()
        want = orc.fma32(F32(b), d2.numpy(), orc.fma32(F32(a), d1.numpy(), theta.numpy()))
        got = out.cpu().numpy()
        assert np.array_equal(got[:lay.n_params].view(np.int32), want[:lay.n_params].view(np.int32)), (case, a, b)
        assert np.isnan(got[lay.n_params:]).all()       # nothing past the parameters
        if H != Hp:   # pads keep their fill whatever (a, b)
            assert np.array_equal(got.view(np.int32)[pads], theta.numpy().view(np.int32)[pads])
            if nk:
                assert (lay.view(out, ix["a"][1])[H:] == 1.0).all()
        for l in range(L):
            Wh2, WTh2 = nan16(), nan16()
            ok(lib.siren_cast_weight(ptr(Wout[l]), Hp, Hp, ptr(Wh2), ptr(WTh2), stream()), lib)
            assert torch.equal(_bits(Wh[l]), _bits(Wh2)) and torch.equal(_bits(WTh[l]), _bits(WTh2)), (case, a, b, l)
            assert torch.equal(WTh[l], Wh[l].t()) and not torch.isnan(Wh[l]).any()
            if (a, b) == (0.0, 0.0):   # the live parameters and their shadows
                Wl, WTl = nan16(), nan16()
                ok(lib.siren_cast_weight(ptr(lay.view(T, ix["W"][l])), Hp, Hp, ptr(Wl), ptr(WTl), stream()), lib)
                assert torch.equal(_bits(Wh[l]), _bits(Wl)) and torch.equal(_bits(WTh[l]), _bits(WTl))
        if (a, b) == (0.0, 0.0):
            assert np.array_equal(got[:lay.n_params].view(np.int32), theta.numpy()[:lay.n_params].view(np.int32))


# ------------------------------------------------------------------ SirenEngine.loss_plane
# name: ((num_sine, num_snake, num_tanh), hidden, model kwargs, distance).  Snake stacks take a shorter
# distance: a 1-D parameter's direction is +-|theta| times the grid step's relative length distance / steps,
# so at distance 2 and 4 steps the corner coefficients (-2, -2) put every Snake a at exactly 0
STACKS = {
    "sine": ((3, 0, 0), 128, {}, 2.0),
    "default": ((2, 2, 0), 256, {}, 0.5),
    "tanh": ((1, 0, 2), 128, {}, 2.0),
    "sinehead": ((2, 0, 0), 128, {"last_linear": False}, 2.0),
}
# (rows, micro_batch, steps): one micro-batch; two whose second is mostly padding
GRIDS = [(1000, 1 << 20, 4), (700, 512, 5)]


def _data(n):
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    return t, (0.5 * torch.sin(37 * t) + 0.2 * torch.sin(91 * t)).reshape(-1)


@functools.lru_cache(maxsize=None)
def _plane_case(stack, grid):
    """Everything the engine tests of one (stack, grid) share, computed once: the plane, per cell the
    fp64 MSE of infer() at plane_state_dict's weights, the fp64 and the half=True formula values."""
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.landscape import plane_directions
    counts, H, kw, distance = STACKS[stack]
    n, mb, steps = GRIDS[grid]
    dev = torch.device("cuda:0")
    t, y = _data(n)
    model = _model(1, H, *counts, **kw)
    eng = SirenEngine(model, t, y, micro_batch=mb, device=dev)
    assert eng.n_micro == (1 if grid == 0 else 2)
    for _ in range(3):      # a few steps: not the initial weights
        eng.step()
    names = [k for k, _ in model.named_parameters()]
    theta = [p.detach().cpu().numpy().copy() for _, p in model.named_parameters()]
    d1, d2 = plane_directions([p for _, p in model.named_parameters()], distance=distance, steps=steps,
                              generator=torch.Generator().manual_seed(11))
    min_a = ref.min_abs_snake_a(names, theta, [x.numpy() for x in d1], [x.numpy() for x in d2], steps)
    plane = eng.loss_plane(d1, d2, steps).numpy()
    # a second engine on a fresh model: plane_state_dict's weights are loaded into it cell by cell
    model2 = _model(1, H, *counts, seed=5, **kw)
    eng2 = SirenEngine(model2, t, y, micro_batch=mb, device=dev)
    own, f64, f16, same = np.zeros_like(plane), np.zeros_like(plane), np.zeros_like(plane), True
    yn = y.numpy()
    for i in range(steps):
        for j in range(steps):
            sd = eng.plane_state_dict(d1, d2, steps, i, j)
            cell = ref.cell_params(theta, [x.numpy() for x in d1], [x.numpy() for x in d2], steps, i, j)
            same = same and all(np.array_equal(sd[k].numpy().view(np.int32), c.view(np.int32))
                                for k, c in zip(names, cell))
            model2.load_state_dict(sd)
            eng2._refresh_shadows()
            own[i, j] = orc.mse(eng2.infer(t.to(dev)).cpu().numpy(), yn)
            p = ref.oracle_params(names, cell, counts, last_linear=kw.get("last_linear", True))
            f64[i, j] = ref.cell_loss(p, t.numpy(), yn, 1000.0, 30.0)
            f16[i, j] = ref.cell_loss(p, t.numpy(), yn, 1000.0, 30.0, half=True)
    live = orc.mse(eng.infer(t.to(dev)).cpu().numpy(), yn)
    return {"plane": plane, "own": own, "f64": f64, "f16": f16, "same": same, "min_a": min_a, "live": live,
            "steps": steps}


CASES = [(s, g) for s in STACKS for g in range(len(GRIDS))]


@pytest.mark.parametrize("stack,grid", CASES)
def test_plane_against_own_infer(lib, dev, stack, grid):
    """Each cell == the host fp64 MSE of infer() on a fresh model holding plane_state_dict(i, j)."""
    c = _plane_case(stack, grid)
    assert c["same"]        # plane_state_dict is the formula's theta_ij bit for bit
    err = np.abs(c["plane"] - c["own"]) / c["own"]
    errlog.log("landscape_self", stack=stack, grid=grid, worst=float(err.max()))
    print(f"landscape self {stack}/{grid}: worst {err.max():.3e}")
    assert np.isfinite(c["plane"]).all() and err.max() <= SELF_GATE, (stack, grid, err.max())
    k = c["steps"] // 2
    if c["steps"] % 2 == 0:  # theta itself
        assert abs(c["plane"][k, k] - c["live"]) <= SELF_GATE * c["live"]


@pytest.mark.parametrize("stack,grid", CASES)
def test_plane_against_formula(lib, dev, stack, grid):
    """Each cell against the fp64 formula at the same theta_ij; the half=True oracle's error against fp64
    on the same cells is logged beside it (the storage format's share)."""
    c = _plane_case(stack, grid)
    assert c["min_a"] >= 1e-3, c["min_a"]      # no Snake a near 0 anywhere on the grid: no cell is skipped
    err = np.abs(c["plane"] - c["f64"]) / c["f64"]
    half = np.abs(c["f16"] - c["f64"]) / c["f64"]
    errlog.log("landscape_formula", stack=stack, grid=grid, worst=float(err.max()), half_worst=float(half.max()),
               cells=err.tolist(), half_cells=half.tolist())
    print(f"landscape formula {stack}/{grid}: worst {err.max():.3e} (half=True oracle {half.max():.3e})")
    assert err.max() <= GATE[stack], (stack, grid, err.max(), half.max())


# ------------------------------------------------------------------ no side effects
def _fit_state(eng):
    torch.cuda.synchronize()
    return [eng.params, eng.exp_avg, eng.exp_avg_sq, eng.state, eng.loss_hist, eng.lr_hist, eng.guard,
            *eng.Wh, *eng.WTh]


@pytest.mark.parametrize("spectral", [False, True])
def test_loss_plane_leaves_the_fit_alone(lib, dev, spectral):
    """Two engines from one seed, step -> capture -> steps; one evaluates a plane between steps.  Parameters,
    shadows, Adam state, history and guard are bit-identical afterwards.

    loss_plane captures the step's graph again after its launches (engine._recapture): replayed as it was, the
    old graph's first step after a plane found a stray word in the gradients' stall slot and was voided, with
    parameters, guard and gradients bit-identical before and after the plane itself."""
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.landscape import plane_directions
    t, y = _data(1000)
    kw = dict(loss_mode="mae", alpha=0.2) if spectral else {}
    engs = [SirenEngine(_model(1, 256, 2, 2, 0), t, y, device=dev, **kw) for _ in range(2)]
    planes, snaps, guards = [], [], [[], []]
    tail = lambda e: e.grads[e.layout.sse_offset:e.layout.sse_offset + 2].clone()  # noqa: E731
    for k, eng in enumerate(engs):
        eng.step()
        eng.capture_graph()
        for _ in range(3):
            eng.step()
        guards[k].append((eng.guard.clone(), tail(eng)))       # stream-ordered copies: no host synchronisation
        if k == 0:
            d1, d2 = plane_directions([p for _, p in eng.model.named_parameters()], distance=0.5, steps=4,
                                      generator=torch.Generator().manual_seed(2))
            snaps.append(eng.params.clone())
            planes.append(eng.loss_plane(d1, d2, 4))
            guards[k].append((eng.guard.clone(), tail(eng)))
        for _ in range(3):
            eng.step()
        guards[k].append((eng.guard.clone(), tail(eng)))
        if k == 0:
            snaps.append(eng.params.clone())
            planes.append(eng.loss_plane(d1, d2, 4))
    state = [_fit_state(e) for e in engs]
    # every figure before any assertion: [flag, headroom, clean, overflows, headroom0, stalls] and the gradients'
    # [sse, stall slot] after 4 steps, (engine 0: after the plane,) after 7 steps
    for k in range(2):
        print(f"landscape side effects spectral={spectral} engine {k}: "
              f"{[(g.cpu().tolist(), t.cpu().tolist()) for g, t in guards[k]]}, "
              f"scheduler steps {engs[k].opt_state().last_epoch}")
    print(f"  params moved between the planes {not torch.equal(snaps[0], snaps[1])}, "
          f"planes differ {not torch.equal(planes[0], planes[1])}, "
          f"|params0 - params1| {float((engs[0].params - engs[1].params).norm()):.3e}")
    for a, b in zip(*state):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    applied = [e.steps_applied() for e in engs]
    assert applied == [7, 7]
    # the plane follows the live weights: three steps later it is another plane
    assert np.isfinite(planes[0].numpy()).all() and not torch.equal(planes[0], planes[1])


# ------------------------------------------------------------------ train(visualization=True)
def test_train_visualization(dev, tmp_path):
    """train(visualization=True, seed=0, total_steps=3) on the golden clip's first second.  A sine stack:
    with the run's 30 steps and distance 2 a 1-D parameter's direction is +-|theta| / 15, so row 0 / column
    15 (and half of the anti-diagonal) put a Snake a at 0 up to rounding -- the reference formula's own NaN
    cell, which passes through -- and this test asserts a finite plane."""
    from inr_for_audio_amd.run import train
    g = np.load(os.path.join(G, "gt_bach_1s.npz"))
    d = tmp_path / "data"
    d.mkdir()
    wavfile.write(str(d / "bach.wav"), int(g["fs"]), g["raw"])
    kw = dict(num_hidden_features=128, num_sine=3, num_snake=0, omega=1000, data_dir=str(d), seed=0, total_steps=3,
              visualization=True)
    planes = []
    for tag in ("a", "b"):
        folder = os.path.dirname(train(str(tmp_path / "exp"), tag, "bach", 1, **kw))
        plane = np.load(os.path.join(folder, "landscape.npy"))
        assert plane.shape == (30, 30) and plane.dtype == np.float64 and np.isfinite(plane).all()
        params = json.load(open(os.path.join(folder, "parameters.json")))
        assert params["visualization"] is True and params["landscape_time_s"] > 0
        try:
            import matplotlib  # noqa: F401
            have = True
        except ImportError:
            have = False
        assert os.path.exists(os.path.join(folder, "landscape.png")) == have
        fs, out = wavfile.read(os.path.join(folder, "output.wav"))
        target = orc.waveform_target(g["raw"], 1, int(g["fs"]))
        want = orc.mse(out.reshape(-1), target)
        assert abs(plane[15, 15] - want) <= GATE["sine"] * want, (plane[15, 15], want)
        planes.append(plane)
    assert np.array_equal(planes[0].view(np.int64), planes[1].view(np.int64))
    folder = os.path.dirname(train(str(tmp_path / "exp"), "c", "bach", 1, **dict(kw, visualization=False)))
    assert not os.path.exists(os.path.join(folder, "landscape.npy"))
    assert "landscape_time_s" not in json.load(open(os.path.join(folder, "parameters.json")))
