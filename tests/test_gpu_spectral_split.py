"""The split spectral step (run.py:126-128, :160-169 across micro-batches and ranks).

Kernel level: siren_{stft,mrstft}_signal_forward / _finish / _backward run over the windows of a
partition of a 12 301-sample signal (4 / 7 / 4 / 16 frame blocks), the partials of the blocks a window
does not own zeroed and the arrays summed as the all-reduce would.  The reference is the existing
whole-signal calls (siren_*_forward -> _loss -> _loss_bwd, siren_snr_loss); what they expose -- the
partial arrays, every finished scalar, the spectral loss and its gradient -- must come out bit for bit,
and the mixed g is rebuilt from them with loss_mix's own two roundings.

Engine level: test_gpu_mrstft_engine.py's setup (N = 5003, H = 128, omega0 = 30000, seed 6)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import mrstft_ref as mr
import spectral_ref as sr

pytestmark = pytest.mark.gpu
NS = 12301
MODES = {"mse": 0, "mae": 1, "snr": 2}
NRES = {"stft": 1, "mrstft": 3}
NAN = float("nan")
_REF = {}


def partitions(n):
    return ([0, n // 2, n], [0, 700, 9000, n], [0, n - 1, n])


class Sig:
    """One loss kind's entry points on an n-sample signal with rows = n."""

    def __init__(self, lib, kind, n, dev):
        from inr_for_audio_amd.engine import _basis
        self.lib, self.kind, self.n, self.dev, self.nres = lib, kind, n, dev, NRES[kind]
        self.basis = _basis(kind, dev)
        self.floats = int(self.fn("workspace_floats")(n, n))
        self.s = torch.cuda.current_stream(dev).cuda_stream
        rr = self.rr
        self.off = [[int(self.fn("ws_offset")(n, n, *rr(r), k)) for k in range(6)] for r in range(self.nres)]
        self.parts = [[int(self.fn("signal_parts")(n, n, *rr(r), k)) for k in range(6)] for r in range(self.nres)]
        self.T = [int(self.fn("frames")(n, *rr(r))) for r in range(self.nres)]
        self.scal = self.off[0][5]                               # the transform scalars [32]
        self.pscal = self.parts[0][4] + 8 * self.parts[0][5]     # the point loss's scalars [32]

    def fn(self, name):
        return getattr(self.lib, f"siren_{self.kind}_{name}")

    def rr(self, r):
        return (r,) if self.kind == "mrstft" else ()

    def new_ws(self, y):
        ws = torch.zeros(self.floats, device=self.dev)
        assert self.fn("forward")(y.data_ptr(), self.n, self.n, self.basis.data_ptr(), ws.data_ptr(), 1, self.s) == 0
        return ws

    def window(self, lo, hi):
        """(win array of the compute ranges, [(owned lo, owned hi)] per transform)."""
        win, owned = (ctypes.c_int32 * 6)(), []
        for r in range(self.nres):
            b = (ctypes.c_int32 * 4)()
            assert self.fn("window")(self.n, *self.rr(r), lo, hi, b) == 0
            win[2 * r], win[2 * r + 1] = b[0], b[1]
            owned.append((b[2], b[3]))
        return win, owned

    def part_index(self, r, b0, b1):
        """ws indices of the partials (both rows) of transform r's frame blocks [b0, b1)."""
        off, npart, nblk, gy = self.parts[r][:4]
        return torch.tensor([off + row * npart + y * nblk + b for row in range(2) for y in range(gy)
                             for b in range(b0, b1)], dtype=torch.long, device=self.dev)

    def rows_index(self, r, t0, t1, which):
        """ws indices of the frames [t0, t1) of transform r's re (0) / im (1) / dF (4)."""
        kwp = {"stft": (1024,), "mrstft": (608, 1200, 240)}[self.kind][r]     # the window's support, padded to 16
        width = (self.off[r][1] - self.off[r][0]) // self.T[r] if which < 4 else kwp
        t0, t1 = min(t0, self.T[r]), min(t1, self.T[r])
        return torch.arange(self.off[r][which] + t0 * width, self.off[r][which] + t1 * width, device=self.dev)

    def poison(self, ws):
        """NaN in every model-side region: re, im, dF and all partial arrays."""
        for r in range(self.nres):
            for which in (0, 1, 4):
                ws[self.rows_index(r, 0, self.T[r], which)] = NAN
            ws[self.parts[r][0]:self.parts[r][0] + 2 * self.parts[r][1]] = NAN
        ws[self.parts[0][4]:self.parts[0][4] + 8 * self.parts[0][5]] = NAN
        return ws

    def forward(self, x, y, mode, alpha, ws, win):
        assert self.fn("signal_forward")(x.data_ptr(), y.data_ptr(), self.n, self.n, mode, alpha,
                                         self.basis.data_ptr(), ws.data_ptr(), win, self.s) == 0

    def finish(self, mode, alpha, ws):
        loss = torch.full((4,), NAN, device=self.dev)
        assert self.fn("signal_finish")(self.n, self.n, mode, alpha, ws.data_ptr(), loss.data_ptr(), self.s) == 0
        return loss[0].cpu()

    def backward(self, x, y, mode, alpha, ws, win, lo, hi, g):
        assert self.fn("signal_backward")(x.data_ptr(), y.data_ptr(), self.n, self.n, mode, alpha,
                                          self.basis.data_ptr(), ws.data_ptr(), win, lo, hi, g.data_ptr(), self.s) == 0


def reference(lib, kind, dev):
    """The whole-signal calls, once per loss kind: x, y, the Sig, the finished workspace, L_spec, g_spec,
    and the SNR loss's workspace (a siren_stft_* one), loss and gradient."""
    if kind not in _REF:
        x64, y64 = mr.signals(NS)
        x, y = x64.float().to(dev), y64.float().to(dev)
        sg = Sig(lib, kind, NS, dev)
        ws = sg.new_ws(y)
        n, s = NS, sg.s
        assert sg.fn("forward")(x.data_ptr(), n, n, sg.basis.data_ptr(), ws.data_ptr(), 0, s) == 0
        loss, g = torch.zeros(4, device=dev), torch.zeros(n, device=dev)
        assert sg.fn("loss")(n, n, ws.data_ptr(), loss.data_ptr(), s) == 0
        assert sg.fn("loss_bwd")(n, n, sg.basis.data_ptr(), ws.data_ptr(), g.data_ptr(), s) == 0
        snr_ws = torch.zeros(int(lib.siren_stft_workspace_floats(n, n)), device=dev)
        snr_loss, snr_g = torch.zeros(4, device=dev), torch.zeros(n, device=dev)
        assert lib.siren_snr_loss(x.data_ptr(), y.data_ptr(), n, n, snr_ws.data_ptr(), snr_loss.data_ptr(),
                                  snr_g.data_ptr(), s) == 0
        torch.cuda.synchronize(dev)
        assert [p[2] for p in sg.parts] == ([4] if kind == "stft" else [7, 4, 16])
        _REF[kind] = dict(x=x, y=y, sg=sg, ws=ws, loss=loss[0].cpu(), g=g.cpu(), snr_ws=snr_ws,
                          snr_loss=snr_loss[0].cpu(), snr_g=snr_g.cpu())
    return _REF[kind]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def expected_g(ref, mode, alpha):
    """loss_mix's g from the reference calls' pieces: v = wp gp, then v += ws g_spec (two fp32 roundings)."""
    x, y, n = ref["x"].cpu(), ref["y"].cpu(), NS
    if mode == "snr":
        gp = ref["snr_g"]
    else:
        err = x - y
        gp = torch.sign(err) * np.float32(1.0 / n) if mode == "mae" else err * np.float32(2.0 / n)
    v = torch.tensor(np.float32(1.0 - alpha)) * gp
    if alpha != 0.0:
        v = v + torch.tensor(np.float32(alpha)) * ref["g"]
    return v


def check_scalars(ref, ws, mode, alpha):
    sg = ref["sg"]
    if alpha != 0.0:   # per transform {S1, sum|dlog|, Sy, L_r, c1, c2}; mrstft: also their mean
        k = 6 if sg.kind == "stft" else 25
        assert torch.equal(bits(ws[sg.scal:sg.scal + k]), bits(ref["ws"][sg.scal:sg.scal + k]))
    if mode == "snr":   # the SNR sums' partial rows and {mean x, mean y, Syc, Sr, L_snr, its gradient factor}
        lib, nb = sg.lib, (NS + 255) // 256
        so = int(lib.siren_stft_ws_offset(NS, NS, 5))
        po, pn = int(lib.siren_stft_signal_parts(NS, NS, 4)), int(lib.siren_stft_signal_parts(NS, NS, 5))
        assert torch.equal(bits(ws[sg.pscal + 6:sg.pscal + 12]), bits(ref["snr_ws"][so + 6:so + 12]))
        for row in range(2, 8):
            a = sg.parts[0][4] + row * sg.parts[0][5]
            assert torch.equal(bits(ws[a:a + nb]), bits(ref["snr_ws"][po + row * pn:po + row * pn + nb])), row


CASES = [(k, m, a) for k in ("stft", "mrstft") for m in ("mse", "mae", "snr") for a in (0.2, 1.0)] + \
    [("stft", "snr", 0.0), ("mrstft", "snr", 0.0)]


@pytest.mark.parametrize("kind,mode,alpha", CASES)
def test_windows_reproduce_the_whole_signal(lib, dev, kind, mode, alpha):
    ref = reference(lib, kind, dev)
    sg, x, y, m = ref["sg"], ref["x"], ref["y"], MODES[mode]
    g_want = expected_g(ref, mode, alpha)
    # the mixed loss in fp64 from the reference calls' fp32 scalars: each carries one fp32 rounding, the
    # point loss's 256-term fp32 partials a few more (the finish itself sums in fp64): 16 x 2^-24 of the terms
    p64 = float(sr.mixed_loss(x.cpu().double(), y.cpu().double(), mode, 0.0))
    want = (1.0 - alpha) * p64 + alpha * float(ref["loss"])
    tol = 1e-6 * (abs((1.0 - alpha) * p64) + abs(alpha * float(ref["loss"])))
    ws = sg.poison(sg.new_ws(y))
    full, _ = sg.window(0, NS)
    sg.forward(x, y, m, alpha, ws, full)
    loss_full = sg.finish(m, alpha, ws)
    for cuts in partitions(NS):
        ws = sg.poison(sg.new_ws(y))
        g = torch.full((NS,), NAN, device=dev)
        acc = torch.zeros_like(ws)
        ranges = list(zip(cuts[:-1], cuts[1:]))
        for lo, hi in ranges:
            win, owned = sg.window(lo, hi)
            sg.forward(x, y, m, alpha, ws, win)
            if alpha != 0.0:
                for r, (o0, o1) in enumerate(owned):   # the owned blocks' partials; zeros elsewhere; summed
                    ix = sg.part_index(r, o0, o1)
                    acc[ix] += ws[ix]
        if alpha != 0.0:
            for r in range(sg.nres):
                a, cnt = sg.parts[r][0], 2 * sg.parts[r][1]
                ix = sg.part_index(r, 0, sg.parts[r][2])
                assert torch.equal(bits(acc[ix]), bits(ref["ws"][ix])), (cuts, r)     # the partial arrays
                ws[a:a + cnt] = acc[a:a + cnt]
        loss = sg.finish(m, alpha, ws)
        for lo, hi in ranges:
            sg.backward(x, y, m, alpha, ws, sg.window(lo, hi)[0], lo, hi, g)
        torch.cuda.synchronize(dev)
        check_scalars(ref, ws, mode, alpha)
        print(f"{kind} {mode} alpha {alpha} cuts {cuts}: loss {float(loss):.8f} want {want:.8f} tol {tol:.2e}")
        assert torch.equal(bits(loss), bits(loss_full))
        assert abs(float(loss) - want) <= tol
        if alpha == 1.0:
            assert torch.equal(bits(loss), bits(ref["loss"]))
        if mode == "snr" and alpha == 0.0:
            assert torch.equal(bits(loss), bits(ref["snr_loss"]))
        assert bool(torch.isfinite(g).all())
        assert torch.equal(g.cpu(), g_want), cuts


@pytest.mark.parametrize("lo,hi", [(700, 9000), (9000, NS)])
@pytest.mark.parametrize("kind", ["stft", "mrstft"])
def test_a_window_writes_its_own_rows_only(lib, dev, kind, lo, hi):
    """One window alone -- [700, 9000) or [9000, n) of the 12 301 samples -- on a workspace whose model
    side is NaN: after its forward only its blocks' re / im rows and partials are numbers; with the
    complete partial arrays in place (the all-reduce) its backward writes its dF rows and g[lo..hi)
    alone, and that g is the whole-signal one: a rank needs nothing outside its window."""
    ref = reference(lib, kind, dev)
    sg, x, y = ref["sg"], ref["x"], ref["y"]
    mode, alpha = "mae", 0.2
    ws = sg.poison(sg.new_ws(y))
    g = torch.full((NS,), NAN, device=dev)
    win, _ = sg.window(lo, hi)
    sg.forward(x, y, MODES[mode], alpha, ws, win)
    torch.cuda.synchronize(dev)
    inside = torch.zeros(ws.numel(), dtype=torch.bool, device=dev)
    for r in range(sg.nres):
        b0, b1 = win[2 * r], win[2 * r + 1]
        assert b0 < b1 and (b0 > 0 or b1 < sg.parts[r][2])        # a proper sub-window
        inside[sg.part_index(r, b0, b1)] = True
        for which in (0, 1):
            inside[sg.rows_index(r, 16 * b0, 16 * b1, which)] = True
    model = torch.zeros_like(inside)
    for r in range(sg.nres):
        for which in (0, 1, 4):
            model[sg.rows_index(r, 0, sg.T[r], which)] = True
        model[sg.parts[r][0]:sg.parts[r][0] + 2 * sg.parts[r][1]] = True
    assert bool(torch.isfinite(ws[inside]).all())
    assert bool(torch.isnan(ws[model & ~inside]).all())
    for r in range(sg.nres):   # the all-reduce's result
        a, cnt = sg.parts[r][0], 2 * sg.parts[r][1]
        ws[a:a + cnt] = ref["ws"][a:a + cnt]
    sg.finish(MODES[mode], alpha, ws)
    sg.backward(x, y, MODES[mode], alpha, ws, win, lo, hi, g)
    torch.cuda.synchronize(dev)
    for r in range(sg.nres):
        inside[sg.rows_index(r, 16 * win[2 * r], 16 * win[2 * r + 1], 4)] = True
        inside[sg.parts[r][0]:sg.parts[r][0] + 2 * sg.parts[r][1]] = True
    assert bool(torch.isfinite(ws[model & inside]).all())
    assert bool(torch.isnan(ws[model & ~inside]).all())
    assert bool(torch.isnan(g[:lo]).all()) and bool(torch.isnan(g[hi:]).all())
    assert torch.equal(g[lo:hi].cpu(), expected_g(ref, mode, alpha)[lo:hi])


# ------------------------------------------------------------------ engine level
N, H, OMEGA0, SEED = 5003, 128, 30000.0, 6
_DATA = {}


def data():
    if not _DATA:
        _, y = mr.signals(N)
        _DATA["t"] = torch.linspace(-1, 1, N).reshape(N, 1)
        _DATA["y"] = y.float()
    return _DATA["t"], _DATA["y"]


def make_model(last_linear=True):
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(SEED)
    return SirenWithSnakeTanh(1, 1, H, 2, 0, 0, last_linear=last_linear, first_omega_0=OMEGA0, hidden_omega_0=30.0)


def make_engine(dev, kind, loss_mode, alpha, last_linear=True, **kw):
    from inr_for_audio_amd.engine import SirenEngine
    t, y = data()
    return SirenEngine(make_model(last_linear), t, y, lr=1e-4, device=dev, loss_mode=loss_mode, alpha=alpha,
                       stft_loss=kind, **kw)


def clamp_ok(kind, out):
    return mr.clamp_margin_ok(out.double()) if kind == "mrstft" else sr.clamp_margin_ok(out.double())


@pytest.mark.parametrize("kind", ["stft", "mrstft"])
@pytest.mark.parametrize("loss_mode,alpha,last_linear", [("mse", 0.2, True), ("mae", 1.0, True), ("snr", 0.2, False)])
def test_one_micro_batch_is_the_default_step(dev, kind, loss_mode, alpha, last_linear):
    """split_spectral=True with the whole signal in one micro-batch: the launches of the default step,
    so three steps leave the same loss history and parameters, bit for bit."""
    a = make_engine(dev, kind, loss_mode, alpha, last_linear)
    b = make_engine(dev, kind, loss_mode, alpha, last_linear, split_spectral=True)
    assert b.split_spectral and b.n_micro == 1 and not a.split_spectral
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize(dev)
    assert a.steps_applied() == b.steps_applied() == 3
    assert clamp_ok(kind, b.out_sig.cpu())
    ha, hb = a.history()[0], b.history()[0]
    assert np.isfinite(ha).all() and np.array_equal(ha.view(np.int32), hb.view(np.int32))
    assert torch.equal(bits(a.params), bits(b.params))


@pytest.mark.parametrize("kind,loss_mode,alpha,last_linear", [("mrstft", "mae", 0.2, True), ("stft", "snr", 0.2, False),
                                                              ("stft", "mse", 0.2, True)])
def test_five_micro_batches(dev, kind, loss_mode, alpha, last_linear):
    """micro_batch=1024: 5 micro-batches, the last with 907 valid rows.  One step against the fp64
    reference on the engine's own out_sig and against the one-batch default engine; then the parameter
    gradients against a host composition of siren_forward + g slice + siren_backward, bit for bit."""
    _, y = data()
    eng = make_engine(dev, kind, loss_mode, alpha, last_linear, micro_batch=1024, split_spectral=True)
    one = make_engine(dev, kind, loss_mode, alpha, last_linear)
    assert eng.n_micro == 5 and eng.batches[-1].n_valid == 907 and one.n_micro == 1
    eng.step()
    one.step()
    torch.cuda.synchronize(dev)
    assert eng.steps_applied() == 1
    out = eng.out_sig.cpu()
    assert clamp_ok(kind, out)
    loss64, g64 = mr.loss_and_grad(mr.mixed_loss, out.double(), y.double(), loss_mode, alpha, kind)
    _, g32 = mr.loss_and_grad(mr.mixed_loss, out, y, loss_mode, alpha, kind)
    got = float(eng.loss_hist[0].item())
    rel = abs(got - float(loss64)) / abs(float(loss64))
    e, e32 = mr.grad_err(eng.g_sig.cpu(), g64), mr.grad_err(g32, g64)
    npar = eng.layout.n_params
    grel = float(torch.linalg.norm(eng.grads[:npar] - one.grads[:npar]) / torch.linalg.norm(one.grads[:npar]))
    print(f"{kind} {loss_mode} alpha {alpha}: loss {got:.7f} vs {float(loss64):.7f} (rel {rel:.2e}); g: e {e:.3e}, "
          f"e_torch32 {e32:.3e}; grads vs one batch rel {grel:.2e}, loss {float(one.loss_hist[0].item()):.7f}")
    assert rel <= 1e-5
    assert e <= 8 * e32
    assert grel < 1e-3
    assert np.allclose(got, float(one.loss_hist[0].item()), rtol=1e-4)

    # composition: a second evaluation of the gradients, then the same launches from the host
    lib, ws = eng.lib, eng.ws
    net, gr = ctypes.byref(eng.net), ctypes.byref(eng.grad_struct)
    s = torch.cuda.current_stream(dev).cuda_stream
    eng._launch_grads()
    torch.cuda.synchronize(dev)
    grads_step, g_sig = eng.grads[:npar].clone(), eng.g_sig.clone()
    assert bool(grads_step.any()) and bool(torch.isfinite(grads_step).all())
    eng.grads.zero_()
    for k, b in enumerate(eng.batches):
        assert lib.siren_forward(net, ctypes.byref(b), s) == 0
        ws.g.zero_()
        ws.g[:b.n_valid] = g_sig[k * 1024:k * 1024 + b.n_valid]
        assert lib.siren_backward(net, gr, ctypes.byref(b), s) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(bits(eng.grads[:npar]), bits(grads_step))


def test_graph_replay_matches_eager(dev):
    """With 5 micro-batches, three steps replayed from a captured graph give the loss history and the
    parameters of three eager steps, bit for bit (the split step takes no host synchronisation)."""
    eager = make_engine(dev, "mrstft", "mae", 0.2, micro_batch=1024, split_spectral=True)
    graph = make_engine(dev, "mrstft", "mae", 0.2, micro_batch=1024, split_spectral=True)
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


def test_refusals(dev, monkeypatch):
    from inr_for_audio_amd import engine as E
    t, y = data()
    with pytest.raises(NotImplementedError, match="one micro-batch"):
        make_engine(dev, "mrstft", "mae", 0.2, micro_batch=1024)
    with pytest.raises(NotImplementedError, match="whole signal"):
        make_engine(dev, "stft", "mae", 0.2, n_total=2 * N, split_spectral=True)
    # no spectral term: the plain step
    assert not make_engine(dev, "stft", "mae", 0.0, split_spectral=True).split_spectral
    monkeypatch.setattr(E, "_dist", lambda: object())     # a process group of more than one rank
    with pytest.raises(NotImplementedError, match="one rank"):
        make_engine(dev, "stft", "mae", 0.2)
    with pytest.raises(NotImplementedError, match="whole signal"):
        make_engine(dev, "stft", "mae", 0.2, n_total=N, split_spectral=True)


def test_train_with_the_switch(dev, tmp_path):
    """train(restated_losses=True, split_spectral=True) on the 1 s golden clip in micro-batches of 8192
    rows (graph replay after the first step): a finite loss history that falls, and parameters.json
    records the switch only when it is set."""
    from inr_for_audio_amd.run import train
    d = tmp_path / "data"
    d.mkdir()
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_bach_1s.npz"))
    wavfile.write(str(d / "bach.wav"), int(g["fs"]), g["raw"])
    kw = dict(loss_mode="mae", alpha=0.2, num_hidden_features=128, omega=1000, data_dir=str(d), seed=1,
              restated_losses=True)
    ck = train(str(tmp_path / "exp"), "s", "bach", 1, total_steps=20, micro_batch=8192, split_spectral=True, **kw)
    params = json.load(open(os.path.join(os.path.dirname(ck), "parameters.json")))
    assert params["split_spectral"] is True and params["alpha"] == 0.2
    losses = train.last_history[0]
    assert len(losses) == 20 and np.isfinite(losses).all() and losses[-1] < losses[0]
    ck2 = train(str(tmp_path / "exp"), "s1", "bach", 1, total_steps=3, **kw)
    assert "split_spectral" not in json.load(open(os.path.join(os.path.dirname(ck2), "parameters.json")))
    with pytest.raises(NotImplementedError, match="micro-batch"):
        train(str(tmp_path / "exp"), "s2", "bach", 1, total_steps=3, micro_batch=8192, **kw)
