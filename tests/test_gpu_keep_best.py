"""keep_best=True on the device (run.py:171-174 as the reference meant it): siren_best_keep
called directly, bit for bit; SirenEngine and KanEngine fits that oscillate, against a twin engine without
the feature stopped at the best step; load_best(); and train(keep_best=True).

The fits' learning rates, step counts and seeds were picked on the GPU so that the loss goes up and down
(the figures stand beside each case below); every engine test asserts that its own run did: at least 3
snapshots, the best step not step 0 and at least 5 steps before the last."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from inr_for_audio_amd._lib import SirenOptState
from inr_for_audio_amd.engine import _opt_state_tensor, new_guard
from gpu_util import ok, ptr, release, stream as S

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = np.float32, np.float64

GRID_CAP = 2048                      # kBestKeepGridCap (csrc/siren_kernels.h): the copy's grid cap, blocks
PASS_FLOATS = GRID_CAP * 256 * 4     # 256 threads a block, one float4 each: floats of the first grid pass
SIZES = [4, 252, 260, PASS_FLOATS + 4]
PAD = 64                             # sentinel floats on either side of best_params (keeps it 256-B aligned)
INF_BITS = 0x7F800000
LAST_EPOCH = 7
SENTINEL = -1234.5


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


def _f32_bits(x) -> int:
    return int(np.array([x], F32).view(np.int32)[0])


def _loss(sse0, n_total) -> np.float32:
    """(float)((double)sse[0] / n_total): IEEE double division, one rounding to fp32."""
    return F32(F64(F32(sse0)) / F64(n_total))


def _raw(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


class Rig:
    """The buffers of one siren_best_keep caller: params with recognisable ends, best_params inside a
    sentinel-filled buffer that is read back whole, the optimizer state at last_epoch 7."""

    def __init__(self, lib, dev, n):
        self.lib, self.dev, self.n = lib, dev, n
        p = np.random.default_rng(n).normal(size=n).astype(F32)
        p[0], p[-1] = 1.25, -7.5
        self.p = torch.from_numpy(p).to(dev)
        self.buf = torch.empty(n + 2 * PAD, device=dev)
        self.bp = self.buf[PAD:PAD + n]
        assert self.p.data_ptr() % 16 == 0 and self.bp.data_ptr() % 16 == 0
        self.state = _opt_state_tensor(1e-3, 1e-6, 0.8, 200, dev)
        st = SirenOptState.from_buffer_copy(_raw(self.state))
        st.last_epoch = LAST_EPOCH
        self.state.copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8))
        self.state0 = _raw(self.state)
        self.sse = torch.zeros(2, device=dev)
        self.best = torch.zeros(4, dtype=torch.int32, device=dev)

    def call(self, best0, sse0, n_total=1.0, stall=0.0, guard=None, fill=SENTINEL):
        """From best_params = `fill` everywhere and best = best0: one call; (whole buffer bytes, best).
        Run twice from the same start: the two runs agree bit for bit.  params, state, sse and the guard
        are read-only to the call."""
        runs = []
        for _ in range(2):
            self.buf.fill_(fill)
            self.best.copy_(torch.tensor(best0, dtype=torch.int32))
            self.sse.copy_(torch.tensor([sse0, stall], dtype=torch.float32))
            before = (_raw(self.p), _raw(self.sse), None if guard is None else _raw(guard))
            ok(self.lib.siren_best_keep(ptr(self.p), ptr(self.bp), self.n, ptr(self.state), ptr(self.sse),
                                        ctypes.c_double(n_total), ptr(guard), ptr(self.best), S()), self.lib)
            torch.cuda.synchronize()
            assert before == (_raw(self.p), _raw(self.sse), None if guard is None else _raw(guard))
            assert _raw(self.state) == self.state0
            runs.append((_raw(self.buf), self.best.cpu().tolist()))
        assert runs[0] == runs[1]
        return runs[0]

    def expect(self, taken: bool, fill=SENTINEL):
        want = torch.full((self.n + 2 * PAD,), fill)
        if taken:
            want[PAD:PAD + self.n] = self.p.cpu()
        return _raw(want)

    def plateau_loss_bits(self, sse0, n_total):
        """The loss_hist entry siren_plateau_step writes for the same sse / n_total, at last_epoch."""
        st = self.state.clone()
        hist = torch.full((LAST_EPOCH + 2,), float("nan"), device=self.dev)
        lrs = torch.zeros(LAST_EPOCH + 2, dtype=torch.float64, device=self.dev)
        self.sse.copy_(torch.tensor([sse0, 0.0], dtype=torch.float32))
        ok(self.lib.siren_plateau_step(ptr(st), ptr(self.sse), ctypes.c_double(n_total), ptr(hist), ptr(lrs),
                                       LAST_EPOCH + 2, S()), self.lib)
        torch.cuda.synchronize()
        h = hist.cpu().numpy()
        assert np.isnan(h[:LAST_EPOCH]).all() and np.isnan(h[LAST_EPOCH + 1:]).all()
        return int(h[LAST_EPOCH:LAST_EPOCH + 1].view(np.int32)[0])


@pytest.fixture(scope="module", params=SIZES, ids=[f"n{n}" for n in SIZES])
def rig(request, lib, dev):
    return Rig(lib, dev, request.param)


@pytest.mark.parametrize("n_total", [1.0, 441000.0])
def test_improving_loss_copies_and_commits(rig, n_total):
    """From (+inf, -1, 0): the whole vector is copied bit for bit -- both ends, nothing outside -- and the
    state becomes (the float plateau_kernel records, last_epoch, 1); a smaller loss then takes again."""
    sse0 = 123.456
    bits = _f32_bits(_loss(sse0, n_total))
    buf, best = rig.call([INF_BITS, -1, 0, 0], sse0, n_total)
    assert buf == rig.expect(True)
    assert best == [bits, LAST_EPOCH, 1, 0]
    assert bits == rig.plateau_loss_bits(sse0, n_total)
    # one fp32 step below the recorded best: strictly smaller, taken
    lower = float(np.nextafter(F32(sse0), F32(0)))
    bits2 = _f32_bits(_loss(lower, n_total))
    buf, best = rig.call([bits, 3, 1, 0], lower, n_total)
    if bits2 != bits:       # (the division may round the two to one float at n_total = 441 000)
        assert buf == rig.expect(True) and best == [bits2, LAST_EPOCH, 2, 0]
        assert bits2 == rig.plateau_loss_bits(lower, n_total)
    else:
        assert buf == rig.expect(False) and best == [bits, 3, 1, 0]


@pytest.mark.parametrize("what,sse0", [("equal", 2.5), ("worse", 2.5000002), ("much worse", 1e30),
                                      ("nan", float("nan")), ("inf", float("inf")), ("-nan", -float("nan"))])
def test_not_taken_leaves_everything(rig, what, sse0):
    """An equal loss (the earlier step stays), a worse one, NaN and +inf: best_params -- the whole buffer --
    and the state stay as they were."""
    best0 = [_f32_bits(2.5), 3, 5, 0]
    buf, best = rig.call(best0, sse0, 1.0)
    assert buf == rig.expect(False) and best == best0
    if what == "inf":       # +inf is not below the initial +inf either
        buf, best = rig.call([INF_BITS, -1, 0, 0], sse0, 1.0)
        assert buf == rig.expect(False) and best == [INF_BITS, -1, 0, 0]


def test_stall_slot_and_guard(rig, dev):
    """sse[1] != 0 and a stalled guard are not taken; the guard's overflow flag alone IS (the loss of such a
    step is the true loss of the weights, and its recomputation cannot take again: strict <); no guard works."""
    best0, sse0 = [_f32_bits(2.5), 3, 5, 0], 1.5
    took = (rig.expect(True), [_f32_bits(1.5), LAST_EPOCH, 6, 0])
    left = (rig.expect(False), best0)
    assert rig.call(best0, sse0, guard=None) == took
    assert rig.call(best0, sse0, stall=1.0) == left
    assert rig.call(best0, sse0, stall=4.2e-41) == left          # any non-zero word voids the step
    clean, flagged, stalled = new_guard(dev), new_guard(dev), new_guard(dev)
    flagged[0] = 1
    stalled[5] = 2
    assert rig.call(best0, sse0, guard=clean) == took
    assert rig.call(best0, sse0, guard=flagged) == took
    assert rig.call(best0, sse0, guard=stalled) == left
    both = new_guard(dev)
    both[0], both[5] = 1, 1
    assert rig.call(best0, sse0, guard=both) == left
    # the recomputed overflow step: same loss, same last_epoch -- not taken a second time
    assert rig.call(took[1], sse0, guard=flagged) == (rig.expect(False), took[1])


# ------------------------------------------------------------------ engines
import keep_best_cases as kc  # noqa: E402

STEPS = kc.STEPS
SINE_GATE = 1e-4   # DESIGN 3's loss gate of a sine stack: infer()'s fp64 MSE against the step's own loss
# the KAN's step output is bit-identical to inference: only the fp32 sums of at most 256 non-negative terms per
# block differ from the fp64 mean (worst case 255 * 2^-24 = 1.5e-5; test_gpu_landscape.py's SELF_GATE)
KAN_GATE = 2e-5


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _live(eng):
    """Everything a step writes that the next one reads, and the histories."""
    torch.cuda.synchronize()
    out = [eng.params, eng.exp_avg, eng.exp_avg_sq, eng.state, eng.loss_hist, eng.lr_hist]
    if eng.guard is not None:
        out += [eng.guard, *eng.Wh, *eng.WTh]
    return out


def _fit(make, tag):
    """The checks every oscillating fit gets; returns (the eager engine, the graph-replayed one, best_info)."""
    keep = make(True)
    for _ in range(STEPS):
        keep.step()
    loss, step, taken = keep.best_info()
    h, _ = keep.history()
    print(f"keep_best {tag}: taken {taken}, best step {step} of {STEPS} (argmin {int(np.argmin(h))}), best loss "
          f"{loss:.6e}, first {h[0]:.6e}, last {h[-1]:.6e}")
    # the run is a valid subject: it went up and down, and the best step is neither end
    assert keep.steps_applied() == STEPS and len(h) == STEPS
    assert taken >= 3 and step != 0 and step <= STEPS - 1 - 5, (taken, step)
    assert step == int(np.argmin(h))
    assert _f32_bits(loss) == _f32_bits(h[step])
    n = keep.layout.n_params

    # a twin without the feature, stopped at the best step: its weights are the snapshot
    twin = make(False)
    assert twin.best_params is None and not twin.keep_best
    for _ in range(step):
        twin.step()
    torch.cuda.synchronize()
    assert _same(twin.params[:n], keep.best_params[:n])
    want = {k: p.detach().cpu().clone() for k, p in twin.model.named_parameters()}
    got = keep.best_state_dict()
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float32 and _same(got[k], want[k]), k
    # ... and run on to the end: the snapshots did not disturb the fit
    for _ in range(STEPS - step):
        twin.step()
    for a, b in zip(_live(keep), _live(twin)):
        assert _same(a, b)

    # the same fit with the step replayed as a graph: the pair is captured with the rest of the update
    graph = make(True)
    graph.step()
    graph.capture_graph()
    for _ in range(STEPS - 1):
        graph.step()
    assert graph.best_info() == (loss, step, taken)
    assert _same(graph.best_params, keep.best_params)
    for a, b in zip(_live(graph), _live(keep)):
        assert _same(a, b)
    return keep, graph, (loss, step, taken)


def _after_load_best(eng, info, coords, target, gate, tag, mse):
    """load_best() on an engine that replays its step: the weights are the snapshot, nothing else moved,
    infer() reproduces the best loss, and one more step runs, replays and sees that loss again."""
    loss, step, taken = info
    n = eng.layout.n_params
    before = [t.clone() for t in (eng.exp_avg, eng.exp_avg_sq, eng.state, eng.loss_hist, eng.lr_hist)]
    ptrs = (eng.params.data_ptr(), eng.best_params.data_ptr())
    eng.load_best()
    torch.cuda.synchronize()
    assert ptrs == (eng.params.data_ptr(), eng.best_params.data_ptr())
    assert _same(eng.params[:n], eng.best_params[:n])
    for a, b in zip(before, (eng.exp_avg, eng.exp_avg_sq, eng.state, eng.loss_hist, eng.lr_hist)):
        assert _same(a, b)
    assert eng.best_info() == info
    if mse:
        out = eng.infer(coords.to(eng.device)).cpu().double().reshape(-1)
        mse64 = float(((out - target.double().reshape(-1)) ** 2).mean())
        print(f"keep_best {tag}: infer() fp64 MSE / best loss = {mse64 / loss:.8f} (gate {gate:g})")
        assert abs(mse64 - loss) <= gate * loss, (mse64, loss)
    assert eng.graph is not None
    eng.step()
    assert eng.steps_applied() == STEPS + 1
    h, _ = eng.history()
    # the same weights through the same kernels: the step after load_best() records the best loss again
    assert _f32_bits(h[STEPS]) == _f32_bits(loss), (h[STEPS], loss)
    assert eng.best_info() == info      # an equal loss keeps the earlier step


@pytest.mark.parametrize("case", list(kc.SIREN_CASES))
def test_siren_fit_keeps_the_best_step(lib, dev, case):
    """plain: 1000 coordinates in one micro-batch; micro: two micro-batches (micro_batch=384 runs as 512 rows);
    spectral: loss_mode='mae', alpha=0.2 at 2048 samples -- the sse slot holds the finished loss, n_total = 1.0."""
    keep, graph, info = _fit(lambda kb: kc.siren_engine(case, dev, kb), f"siren {case}")
    assert keep.n_micro == (2 if case == "micro" else 1) and keep.spectral == (case == "spectral")
    n, kw, _, _ = kc.SIREN_CASES[case]
    t, y = kc.data(n)
    _after_load_best(graph, info, t, y, SINE_GATE, f"siren {case}", mse=case != "spectral")
    # the fp16 shadows the forward reads are siren_cast_weight of the restored weights, bit for bit
    keep.load_best()
    for W, Wh, WTh in zip(keep.W, keep.Wh, keep.WTh):
        a, b = torch.full_like(Wh, float("nan")), torch.full_like(WTh, float("nan"))
        ok(lib.siren_cast_weight(ptr(W), kc.H, kc.H, ptr(a), ptr(b), S()), lib)
        torch.cuda.synchronize()
        assert not torch.isnan(a).any() and _same(a, Wh) and _same(b, WTh)


@pytest.mark.parametrize("case", list(kc.KAN_CASES))
def test_kan_fit_keeps_the_best_step(lib, dev, case):
    """g5 / g11: the compile-time grid and a general one; micro: three micro-batches of 384 rows; spectral: the
    phased step (split_spectral=True) with loss_mode='mae', alpha=0.2 at 2048 samples -- n_total = 1.0."""
    keep, graph, info = _fit(lambda kb: kc.kan_engine(case, dev, kb), f"kan {case}")
    assert keep.n_micro == (3 if case == "micro" else 1) and keep.spectral == (case == "spectral")
    n = kc.KAN_CASES[case][0]
    t, y = kc.data(n)
    _after_load_best(graph, info, t, y, KAN_GATE, f"kan {case}", mse=case != "spectral")


def test_no_snapshot_raises(lib, dev):
    for make in (kc.siren_engine, kc.kan_engine):
        case = "plain" if make is kc.siren_engine else "g5"
        eng = make(case, dev, True)
        loss, step, taken = eng.best_info()
        assert (loss, step, taken) == (float("inf"), -1, 0)
        assert not eng.best_params.any()
        with pytest.raises(RuntimeError, match="no snapshot"):
            eng.load_best()
        with pytest.raises(RuntimeError, match="no snapshot"):
            eng.best_state_dict()
        off = make(case, dev, False)
        for call in (off.best_info, off.best_state_dict, off.load_best):
            with pytest.raises(RuntimeError, match="keep_best"):
                call()


def test_kan_update_grid_resets_the_best(lib, dev):
    """update_grid() moves the knots, which live outside the flat vector: the snapshot from before belongs to
    other knots, so the state returns to (+inf, -1) -- `taken` keeps counting -- and the next step takes."""
    eng = kc.kan_engine("g5", dev, True)
    for _ in range(10):
        eng.step()
    loss, step, taken = eng.best_info()
    assert step >= 0 and taken >= 1
    eng.update_grid()
    assert eng.best_info() == (float("inf"), -1, taken)
    with pytest.raises(RuntimeError, match="no snapshot"):
        eng.load_best()
    n = eng.layout.n_params
    before = eng.params[:n].clone()
    eng.step()
    h, _ = eng.history()
    loss2, step2, taken2 = eng.best_info()
    assert (step2, taken2) == (10, taken + 1) and _f32_bits(loss2) == _f32_bits(h[10])
    assert _same(eng.best_params[:n], before)


# ------------------------------------------------------------------ train(keep_best=True)
def _spy(monkeypatch, name):
    """train()'s engine, caught as it is built: the test reads the device state train() leaves behind."""
    from inr_for_audio_amd import run
    made = []

    class Spy(getattr(run, name)):
        def __init__(self, model, coords, target, **kw):
            super().__init__(model, coords, target, **kw)
            self.coords_in = coords
            self.final_params = None
            made.append(self)

        def load_best(self):
            self.final_params = self.params.clone()
            super().load_best()

    monkeypatch.setattr(run, name, Spy)
    return made


@pytest.mark.parametrize("arch", ["mlp", "kan"])
def test_train_keep_best(dev, tmp_path, monkeypatch, arch):
    """train(keep_best=True) on the golden clip's first second: the checkpoint's model_state_dict, output.wav
    and parameters.json are the best step's; optimizer_state_dict is the final Adam state.  Without the
    keyword none of the new keys is written.  Measured over the 30 steps: the MLP (lr 2.5e-3) fell all the way,
    18 snapshots with the best at step 29; the KAN (lr 0.05) 9 snapshots with the best at step 26."""
    from inr_for_audio_amd.run import train
    g = np.load(os.path.join(G, "gt_bach_1s.npz"))
    d = tmp_path / "data"
    d.mkdir()
    wavfile.write(str(d / "bach.wav"), int(g["fs"]), g["raw"])
    steps = 30
    if arch == "mlp":
        kw = dict(num_hidden_features=128, num_sine=3, num_snake=0, omega=1000, learning_rate=2.5e-3)
    else:
        kw = dict(arch="kan", num_hidden_features=8, learning_rate=0.05)
    kw.update(data_dir=str(d), seed=0, total_steps=steps)
    made = _spy(monkeypatch, "SirenEngine" if arch == "mlp" else "KanEngine")
    ckpt_path = train(str(tmp_path / "exp"), "a", "bach", 1, keep_best=True, **kw)
    folder = os.path.dirname(ckpt_path)
    eng, = made
    assert eng.keep_best and eng.final_params is not None          # load_best() ran
    loss, step, taken = eng.best_info()
    h, _ = eng.history()
    n = eng.layout.n_params
    print(f"train keep_best {arch}: taken {taken}, best step {step} of {steps}, best {loss:.6e}, last {h[-1]:.6e}, "
          f"final weights differ from best: {not _same(eng.final_params[:n], eng.best_params[:n])}")
    params = json.load(open(os.path.join(folder, "parameters.json")))
    assert params["keep_best"] is True and params["best_loss"] == loss == float(h[step])
    assert params["best_iter"] == step == int(np.argmin(h)) and params["final_loss"] == float(h[-1])
    assert eng.steps_applied() == steps
    # the live weights are the snapshot, not the final weights (even the last step's snapshot is the
    # weights its loss was computed with, before its update)
    assert _same(eng.params[:n], eng.best_params[:n])
    assert not _same(eng.final_params[:n], eng.best_params[:n])
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    best = eng.best_state_dict()
    sd = ckpt["model_state_dict"]
    assert set(best) <= set(sd)                                     # (a KAN's state_dict also holds its knots)
    for k, v in best.items():
        assert _same(sd[k], v), k
    adam = eng.adam_state_dict()
    assert float(ckpt["optimizer_state_dict"]["state"][0]["step"]) == steps
    for i, s in adam["state"].items():
        assert _same(ckpt["optimizer_state_dict"]["state"][i]["exp_avg"], s["exp_avg"])
    fs, out = wavfile.read(os.path.join(folder, "output.wav"))
    want = eng.infer(eng.coords_in.to(eng.device)).cpu().numpy().astype(np.float32)
    assert out.dtype == np.float32 and np.array_equal(out.reshape(-1).view(np.int32), want.reshape(-1).view(np.int32))

    made.clear()
    folder = os.path.dirname(train(str(tmp_path / "exp"), "b", "bach", 1, **kw))
    eng, = made
    assert not eng.keep_best and eng.best_params is None and eng.final_params is None
    plain = json.load(open(os.path.join(folder, "parameters.json")))
    assert "keep_best" not in plain and "best_loss" not in plain
    assert set(params) - set(plain) == {"keep_best", "best_loss"}
    # the same fit: its history is the keep_best run's, and its checkpoint holds the last step's weights
    assert plain["best_iter"] == step and plain["final_loss"] == params["final_loss"]
