"""The KAN fit under the mae, snr and STFT losses, without a device: the new entry points' binding and
validation (every code comes back before any launch), the struct and ABI they leave alone, the
refusals that stay, and the spectral tests' broadband recipe on the oracle's output."""
import ctypes

import pytest
import torch

import kan_loss_cases as kc
import mrstft_ref as mr
import spectral_ref as sr
from oracle import siren_oracle as orc

OK, SHAPE, NULL, CONFIG = 0, 1001, 1002, 1003
_i32, _i64, _p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


def test_entry_points_are_bound(lib):
    from inr_for_audio_amd import _lib
    P = ctypes.POINTER
    triple = [P(_lib.SirenKanNet), P(_lib.SirenKanGrads), P(_lib.SirenKanBatch)]
    assert _lib._SIGS["siren_kan_train_step_loss"] == (ctypes.c_int, triple + [_i32, _p])
    assert _lib._SIGS["siren_kan_step_backward"] == (ctypes.c_int, triple + [_p])
    for name in ("siren_kan_train_step_loss", "siren_kan_step_backward"):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib._SIGS[name][1]


def test_batch_struct_and_abi_are_unchanged(lib):
    from inr_for_audio_amd import _lib
    assert [f[0] for f in _lib.SirenKanBatch._fields_] == ["rows", "n_valid", "n_total", "splits", "zero_grads",
                                                           "coords", "target", "out", "g", "ws"]
    assert lib.siren_struct_size(6) == ctypes.sizeof(_lib.SirenKanBatch) == 64
    assert lib.siren_struct_size(4) == ctypes.sizeof(_lib.SirenKanNet)
    assert lib.siren_struct_size(5) == ctypes.sizeof(_lib.SirenKanGrads)
    assert lib.siren_abi_version() == _lib.ABI_VERSION == 12


def _structs(widths=(1, 8, 8, 1)):
    """A net, gradients and a batch whose pointers are non-null but never followed: every call below
    returns from its checks."""
    from inr_for_audio_amd import _lib
    net, gr, b = _lib.SirenKanNet(), _lib.SirenKanGrads(), _lib.SirenKanBatch()
    net.n_layers = len(widths) - 1
    for l, w in enumerate(widths):
        net.width[l] = w
    for l in range(net.n_layers):
        net.grid[l] = net.base_w[l] = net.spline_w[l] = net.scaler[l] = 64
        gr.base_w[l] = gr.spline_w[l] = gr.scaler[l] = 64
    gr.sse = 64
    b.rows, b.n_valid, b.n_total, b.splits = 100, 100, 100.0, 1
    b.coords = b.target = b.out = b.g = b.ws = 64
    return net, gr, b


def test_train_step_loss_validation(lib):
    R = ctypes.byref
    net, gr, b = _structs()
    step = lib.siren_kan_train_step_loss
    for mode in (2, 3, -1):      # 'snr' is no point loss of this entry point
        assert step(R(net), R(gr), R(b), mode, None) == CONFIG
    assert step(None, R(gr), R(b), 1, None) == NULL
    assert step(R(net), None, R(b), 1, None) == NULL
    assert step(R(net), R(gr), None, 1, None) == NULL
    for field in ("coords", "target", "out", "g", "ws"):
        net, gr, b = _structs()
        setattr(b, field, None)
        assert step(R(net), R(gr), R(b), 1, None) == NULL, field
    net, gr, b = _structs()
    gr.sse = None
    assert step(R(net), R(gr), R(b), 1, None) == NULL
    net, gr, b = _structs()
    gr.spline_w[1] = None
    assert step(R(net), R(gr), R(b), 1, None) == NULL
    for field, bad in (("rows", 0), ("splits", 0), ("n_valid", 101), ("n_valid", -1), ("n_total", 0.0)):
        net, gr, b = _structs()
        setattr(b, field, bad)
        assert step(R(net), R(gr), R(b), 1, None) == SHAPE, field
    net, gr, b = _structs((1, 8, 2))
    assert step(R(net), R(gr), R(b), 1, None) == SHAPE          # a point loss on a scalar output
    net, gr, b = _structs()
    net.n_layers = 9
    assert step(R(net), R(gr), R(b), 1, None) == CONFIG


def test_step_backward_validation(lib):
    R = ctypes.byref
    bwd = lib.siren_kan_step_backward
    net, gr, b = _structs()
    assert bwd(None, R(gr), R(b), None) == NULL
    assert bwd(R(net), None, R(b), None) == NULL
    assert bwd(R(net), R(gr), None, None) == NULL
    for field in ("coords", "g", "ws"):
        net, gr, b = _structs()
        setattr(b, field, None)
        assert bwd(R(net), R(gr), R(b), None) == NULL, field
    net, gr, b = _structs()
    gr.base_w[0] = None
    assert bwd(R(net), R(gr), R(b), None) == NULL
    for field in ("rows", "splits"):
        net, gr, b = _structs()
        setattr(b, field, 0)
        assert bwd(R(net), R(gr), R(b), None) == SHAPE, field
    for widths in ((1, 8, 2), (1, 128, 128, 3)):    # last width 1, fused head or not
        net, gr, b = _structs(widths)
        assert bwd(R(net), R(gr), R(b), None) == SHAPE, widths
    net, gr, b = _structs()
    net.width[1] = 0
    assert bwd(R(net), R(gr), R(b), None) == SHAPE


# ------------------------------------------------------------------ refusals
def test_engine_refuses_without_the_switch():
    """Before the model is touched (it is None here) and before any device is asked for."""
    from inr_for_audio_amd.engine import KanEngine
    t, y = kc.coords(), kc.target()
    for kw in (dict(loss_mode="snr"), dict(alpha=0.2), dict(loss_mode="mae", alpha=0.2, stft_loss="mrstft")):
        with pytest.raises(NotImplementedError, match="MSELoss only") as e:
            KanEngine(None, t, y, **kw)
        assert "split_spectral=True" in str(e.value)


def test_engine_shape_refusals_are_the_mlps():
    from inr_for_audio_amd.engine import KanEngine
    t, y = kc.coords(), kc.target()
    sw = dict(split_spectral=True)
    with pytest.raises(ValueError, match="alpha"):
        KanEngine(None, t, y, alpha=1.5, **sw)
    with pytest.raises(ValueError, match="512"):
        KanEngine(None, t[:512], y[:512], alpha=0.2, **sw)
    with pytest.raises(ValueError, match="1024"):
        KanEngine(None, t[:1024], y[:1024], alpha=0.2, stft_loss="mrstft", **sw)
    with pytest.raises(NotImplementedError, match="whole signal"):
        KanEngine(None, t, y, alpha=0.2, n_total=2 * kc.N, **sw)
    with pytest.raises(ValueError, match="stft_loss"):
        KanEngine(None, t, y, alpha=0.2, stft_loss="cqt", **sw)
    with pytest.raises(NotImplementedError, match="loss_mode"):
        KanEngine(None, t, y, loss_mode="huber")


@pytest.mark.parametrize("kw,match", [
    (dict(alpha=0.2, restated_losses=True), "split_spectral"),
    (dict(loss_mode="snr", restated_losses=True), "split_spectral"),
    (dict(alpha=0.2, restated_losses=True, stft_loss="mrstft"), "split_spectral"),
    (dict(alpha=0.2), "restated_losses"),
    (dict(method="mdct", loss_mode="mae"), "1-D"),
    (dict(method="mdct", alpha=0.2, restated_losses=True, split_spectral=True), "1-D"),
    (dict(visualization=True, loss_mode="mae"), "plane"),
])
def test_train_refusals(tmp_path, kw, match):
    from inr_for_audio_amd.run import train
    with pytest.raises(NotImplementedError, match=match):
        train(str(tmp_path), "t", "clip", 1, arch="kan", **kw)
    assert not list(tmp_path.iterdir())             # refused before the experiment folder exists


def test_train_still_refuses_multichannel_with_these_losses(tmp_path):
    from inr_for_audio_amd.run import train
    with pytest.raises(NotImplementedError, match="multichannel"):
        train(str(tmp_path), "t", "clip", 1, alpha=0.2, restated_losses=True, split_spectral=True, multichannel=True)
    assert not list(tmp_path.iterdir())


# ------------------------------------------------------------------ the spectral tests' recipe
@pytest.mark.parametrize("widths", kc.WIDTHS + [[1, 128, 128, 1]])
def test_recipe_clears_the_clamp(widths):
    """The broadband KAN signal passes both references' clamp-margin precondition on the oracle's output,
    with room: no bin's power below 16 eps (the band that fails ends at 4 eps)."""
    m = kc.recorded_model(widths)
    sd = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    out, _ = orc.kan_forward(sd, kc.coords().numpy(), len(widths) - 1)
    x = torch.from_numpy(out).double().reshape(-1)
    assert x.numel() == kc.N and bool(torch.isfinite(x).all())
    assert sr.clamp_margin_ok(x) and mr.clamp_margin_ok(x)
    floor = min(float(sr.power(x).min()), *(float(mr.power(x, res).min()) for res in mr.RES))
    print(f"{widths}: smallest bin power {floor:.2e}")
    assert floor > 16 * sr.EPS
