"""siren_apply_update called directly (guard check -> Adam -> shadow cast -> plateau scheduler), on a
minimal valid siren_net: hidden 128, one inner layer whose fp32 weight is a view at a 16-byte-aligned
offset inside the flat vector.  n_params = 2 * 262 144 + 77, so guard_check (cap 1024 x 256 elements a
pass) takes three passes and Adam's loop is entered by every thread; the gradients are synthetic host
arrays and `sse` is the reduced [value, stall slot] pair.  Every buffer the call may write is read back
whole after each call: p / m / v against siren_adam_step on copies (bit for bit), the shadows against
siren_cast_weight, the optimizer state and the guard field by field, both histories against
NaN-prefilled expectations."""
import ctypes

import numpy as np
import pytest
import torch

from inr_for_audio_amd._lib import HEADROOM0, SirenGuard, SirenNet, SirenOptState
from inr_for_audio_amd.engine import _opt_state_tensor, new_guard
from gpu_util import ok, ptr, release, stream as S

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 2 * 262144 + 77
H = 128
W_OFF = 1000            # floats: a 16-byte-aligned offset that is no multiple of the 64-element tile
N_TOTAL = 1000.0
LR = 1e-3
K_MIN, K_DROP, K_GROW = -14, 4, 1000   # kHeadroomMin, kHeadroomDrop, kHeadroomGrowAfter (siren_kernels.h)


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def _grad(seed=1):
    return (np.random.default_rng(seed).normal(size=N) * 1e-3).astype(F32)


class Rig:
    """The buffers of one siren_apply_update caller, as SirenEngine lays them out."""

    def __init__(self, lib, dev, hist_cap=8, hist_len=8, guard=True, headroom=HEADROOM0):
        self.lib, self.dev, self.hist_cap = lib, dev, hist_cap
        rng = np.random.default_rng(0)
        self.p = torch.from_numpy((rng.normal(size=N) * 0.05).astype(F32)).to(dev)
        self.p0 = self.p.clone()
        self.m = torch.zeros(N, device=dev)
        self.v = torch.zeros(N, device=dev)
        self.g = torch.zeros(N, device=dev)
        self.W = self.p[W_OFF:W_OFF + H * H]
        assert self.W.data_ptr() % 16 == 0
        self.Wh = torch.full((H, H), float("nan"), dtype=torch.float16, device=dev)
        self.WTh = torch.full((H, H), float("nan"), dtype=torch.float16, device=dev)
        self.state = _opt_state_tensor(LR, 1e-6, 0.8, 200, dev)
        self.guard = new_guard(dev) if guard else None
        if guard:
            self.guard[1] = headroom
        self.loss_hist = torch.full((hist_len,), float("nan"), device=dev)
        self.lr_hist = torch.full((hist_len,), float("nan"), dtype=torch.float64, device=dev)
        self.sse = torch.zeros(2, device=dev)
        net = SirenNet()
        net.in_dim, net.hidden, net.n_inner = 1, H, 1
        net.omega0, net.omega = 30.0, 30.0
        # the update reads none of these; check_net wants them present
        net.W0 = net.b0 = net.w_head = net.b_head = ptr(self.p)
        net.b[0], net.Wh[0], net.WTh[0] = ptr(self.p), ptr(self.Wh), ptr(self.WTh)
        self.net = net
        self._Wp = (ctypes.c_void_p * 1)(ptr(self.W))
        self._Whp = (ctypes.c_void_p * 1)(ptr(self.Wh))
        self._WThp = (ctypes.c_void_p * 1)(ptr(self.WTh))

    def call(self, g, sse0=123.456, stall=0.0):
        """One siren_apply_update with the gradient vector g (host array or None: as last call); the
        shadows are NaN before it, so a cast that did not run shows."""
        if g is not None:
            self.g.copy_(torch.from_numpy(g))
        self.sse.copy_(torch.tensor([sse0, stall], dtype=torch.float32))
        self.Wh.fill_(float("nan"))
        self.WTh.fill_(float("nan"))
        ok(self.lib.siren_apply_update(ctypes.byref(self.net), ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), N,
                                       self._Wp, self._Whp, self._WThp, ptr(self.state), ptr(self.sse),
                                       ctypes.c_double(N_TOTAL), ptr(self.loss_hist), ptr(self.lr_hist),
                                       self.hist_cap, ptr(self.guard), S()), self.lib)

    def with_grad(self, g):
        self.g.copy_(torch.from_numpy(g))
        return self

    def adam_ref(self):
        """(p, m, v) that siren_adam_step makes of copies of the current vectors, gradient and state."""
        p, m, v, st = self.p.clone(), self.m.clone(), self.v.clone(), self.state.clone()
        ok(self.lib.siren_adam_step(ptr(p), ptr(self.g), ptr(m), ptr(v), N, ptr(st), S()), self.lib)
        torch.cuda.synchronize()
        return p, m, v

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: _bits(getattr(self, k)) for k in ("p", "m", "v", "state", "loss_hist", "lr_hist")}

    def st(self):
        return SirenOptState.from_buffer_copy(_bits(self.state))

    def gd(self):
        return SirenGuard.from_buffer_copy(_bits(self.guard))

    def check_shadows(self):
        """Wh / WTh equal siren_cast_weight of the fp32 weight as it stands now."""
        Wh = torch.full_like(self.Wh, float("nan"))
        WTh = torch.full_like(self.WTh, float("nan"))
        ok(self.lib.siren_cast_weight(ptr(self.W), H, H, ptr(Wh), ptr(WTh), S()), self.lib)
        torch.cuda.synchronize()
        assert not torch.isnan(Wh).any() or torch.isnan(self.W).any()
        assert _bits(self.Wh) == _bits(Wh) and _bits(self.WTh) == _bits(WTh)

    def check_applied(self, ref, before, k, sse0=123.456):
        """After a call that applied: vectors equal `ref` (adam_ref taken before the call) bit for bit,
        step and last_epoch one past `before`, history slot k written."""
        torch.cuda.synchronize()
        for name, r in zip(("p", "m", "v"), ref):
            assert _bits(getattr(self, name)) == _bits(r), name
        self.check_shadows()
        st = self.st()
        assert st.step == before.step + 1.0 and st.last_epoch == before.last_epoch + 1
        assert k == before.last_epoch
        loss = F32(np.float64(F32(sse0)) / N_TOTAL)
        if k < self.hist_cap:
            got = self.loss_hist.cpu().numpy()[k]
            assert got.tobytes() == loss.tobytes() or (np.isnan(got) and np.isnan(loss))
            assert self.lr_hist.cpu().numpy()[k] == st.lr


def _guard(gd):
    return {"flag": gd.flag, "headroom": gd.headroom, "clean": gd.clean, "overflows": gd.overflows,
            "headroom0": gd.headroom0, "stalls": gd.stalls}


def _hist_expect(n, vals, dtype):
    e = np.full(n, np.nan, dtype)
    e[:len(vals)] = vals
    return e


def test_clean_step(lib, dev):
    r = Rig(lib, dev)
    sses = [123.456, 120.0, 119.5]
    for k, sse0 in enumerate(sses):
        ref, before = r.with_grad(_grad(10 + k)).adam_ref(), r.st()
        r.call(None, sse0)
        r.check_applied(ref, before, k, sse0)
        assert _guard(r.gd()) == {"flag": 0, "headroom": 6, "clean": k + 1, "overflows": 0, "headroom0": 6,
                                  "stalls": 0}
    st = r.st()
    assert st.step == 3.0 and st.last_epoch == 3 and st.lr == LR and st.num_bad == 0
    assert st.best == float(F32(np.float64(F32(sses[-1])) / N_TOTAL))
    losses = [F32(np.float64(F32(s)) / N_TOTAL) for s in sses]
    assert np.array_equal(r.loss_hist.cpu().numpy(), _hist_expect(8, losses, F32), equal_nan=True)
    assert np.array_equal(r.lr_hist.cpu().numpy(), _hist_expect(8, [LR] * 3, np.float64), equal_nan=True)
    assert int((r.p != r.p0).sum()) > N // 2      # the steps did move the parameters


@pytest.mark.parametrize("index", [0, 262144 + 3, N - 1], ids=["first", "pass2", "last"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "pinf", "ninf"])
def test_overflow_step(lib, dev, index, bad):
    r = Rig(lib, dev)
    g = _grad()
    r.call(g)                                      # a clean step first: clean = 1, one history entry
    snap = r.snapshot()
    assert _guard(r.gd())["clean"] == 1
    g_bad = g.copy()
    g_bad[index] = bad
    r.call(g_bad)
    assert r.snapshot() == snap                     # p, m, v, the state bytes and both histories untouched
    r.check_shadows()                               # the cast ran, on the unchanged W
    assert _guard(r.gd()) == {"flag": 1, "headroom": 6 - K_DROP, "clean": 0, "overflows": 1, "headroom0": 6,
                              "stalls": 0}
    ref, before = r.with_grad(g).adam_ref(), r.st()
    r.call(g)                                      # the flag is cleared by the next call
    r.check_applied(ref, before, 1)
    assert _guard(r.gd()) == {"flag": 0, "headroom": 6 - K_DROP, "clean": 1, "overflows": 1, "headroom0": 6,
                              "stalls": 0}


def test_floor_at_headroom_min(lib, dev):
    """From headroom 6 with every call overflowing: five calls are skipped (6 -> 2 -> -2 -> -6 -> -10 -> -14),
    the sixth is passed through -- the NaN reaches p as the fp32 reference would let it."""
    r = Rig(lib, dev)
    g = _grad()
    g[5] = np.nan
    snap = r.snapshot()
    for i in range(5):
        r.call(g)
        assert r.snapshot() == snap, i
        assert _guard(r.gd()) == {"flag": 1, "headroom": 6 - K_DROP * (i + 1), "clean": 0, "overflows": i + 1,
                                  "headroom0": 6, "stalls": 0}
    assert r.gd().headroom == K_MIN
    ref, before = r.adam_ref(), r.st()
    r.call(g)
    r.check_applied(ref, before, 0)
    assert torch.isnan(r.p[5]) and int(torch.isnan(r.p).sum()) == 1
    assert _guard(r.gd()) == {"flag": 1, "headroom": K_MIN, "clean": 1, "overflows": 5, "headroom0": 6, "stalls": 0}


def test_regrowth_after_clean_steps(lib, dev):
    r = Rig(lib, dev)
    g = _grad()
    g_bad = g.copy()
    g_bad[7] = np.inf
    r.call(g_bad)
    assert _guard(r.gd())["headroom"] == 2
    r.with_grad(g)
    for _ in range(K_GROW - 1):
        r.call(None)
    assert _guard(r.gd()) == {"flag": 0, "headroom": 2, "clean": K_GROW - 1, "overflows": 1, "headroom0": 6,
                              "stalls": 0}
    assert r.st().step == K_GROW - 1
    r.call(None)
    assert _guard(r.gd()) == {"flag": 0, "headroom": 3, "clean": 0, "overflows": 1, "headroom0": 6, "stalls": 0}
    assert r.st().step == K_GROW and r.st().last_epoch == K_GROW
    # the cap: at headroom0 the thousandth clean step resets the count and grows nothing
    r.guard[1] = HEADROOM0
    r.guard[2] = K_GROW - 1
    r.call(None)
    assert _guard(r.gd()) == {"flag": 0, "headroom": HEADROOM0, "clean": 0, "overflows": 1, "headroom0": 6,
                              "stalls": 0}


@pytest.mark.parametrize("sse0", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_diverged_loss_is_applied(lib, dev, sse0):
    """A non-finite loss with non-finite gradients is a diverged fit, not an fp16 overflow: applied."""
    r = Rig(lib, dev)
    g = _grad()
    g[3], g[262144 + 9], g[N - 2] = np.nan, np.inf, -np.inf
    ref, before = r.with_grad(g).adam_ref(), r.st()
    r.call(None, sse0)
    r.check_applied(ref, before, 0, sse0)
    assert _guard(r.gd()) == {"flag": 1, "headroom": 6, "clean": 1, "overflows": 0, "headroom0": 6, "stalls": 0}
    assert r.st().step == 1.0


def test_stall_skips_until_cleared(lib, dev):
    r = Rig(lib, dev)
    g = _grad()
    r.call(g)
    snap = r.snapshot()
    quiet = {"flag": 0, "headroom": 6, "clean": 1, "overflows": 0, "headroom0": 6, "stalls": 1}
    r.call(g, stall=1.0)                           # the reduced stall slot a data-parallel rank receives
    assert r.snapshot() == snap and _guard(r.gd()) == quiet
    r.check_shadows()
    r.call(g, stall=0.0)                           # sticky
    assert r.snapshot() == snap and _guard(r.gd()) == quiet
    g_bad = g.copy()
    g_bad[262144 + 3] = np.nan
    r.call(g_bad, stall=0.0)                       # the stall takes precedence: headroom untouched
    assert r.snapshot() == snap and _guard(r.gd()) == dict(quiet, flag=1)
    r.guard[5] = 0
    ref, before = r.with_grad(g).adam_ref(), r.st()
    r.call(g)
    r.check_applied(ref, before, 1)
    assert _guard(r.gd()) == {"flag": 0, "headroom": 6, "clean": 2, "overflows": 0, "headroom0": 6, "stalls": 0}


def test_null_guard_makes_no_check(lib, dev):
    r = Rig(lib, dev, guard=False)
    g = _grad()
    g[262144 + 3] = np.nan
    ref, before = r.with_grad(g).adam_ref(), r.st()
    r.call(None)
    r.check_applied(ref, before, 0)
    assert torch.isnan(r.p[262144 + 3]) and int(torch.isnan(r.p).sum()) == 1


def test_history_bound(lib, dev):
    r = Rig(lib, dev, hist_cap=3, hist_len=8)
    g = _grad()
    sses = [50.0, 49.0, 48.5, 48.25, 48.0]
    for s in sses:
        r.call(g, s)
    torch.cuda.synchronize()
    losses = [F32(np.float64(F32(s)) / N_TOTAL) for s in sses[:3]]
    assert np.array_equal(r.loss_hist.cpu().numpy(), _hist_expect(8, losses, F32), equal_nan=True)
    assert np.array_equal(r.lr_hist.cpu().numpy(), _hist_expect(8, [LR] * 3, np.float64), equal_nan=True)
    assert r.st().last_epoch == 5 and r.st().step == 5.0
