"""Multi-resolution STFT loss (run.py:127, :160), the parts that need no GPU: the fp64 reference
against its own single-resolution pieces and recorded values, the three transforms' tables against
an fp64 DFT of the padded window, sizing, host-side argument validation of the new entry points, and
train()'s switch."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import mrstft_ref as mr
import spectral_ref as sr

# per resolution: table rows (win rounded up to 16), padded bins
KWP, NBP = (608, 1200, 240), (528, 1040, 272)


def inputs(n=5003, clamp=False):
    """The fp32 roundings of spectral_ref.signals(n) (seed 1), as fp64 tensors."""
    x, y = sr.signals(n)
    if clamp:
        x[:2048] = 0
    return x.float().double(), y.float().double()


# ------------------------------------------------------------------ the reference itself
def test_reference_identical_signals_give_zero():
    x, y = inputs()
    assert float(mr.mrstft_loss(y, y)) == 0.0
    assert float(mr.mrstft_loss(x, y)) > 0.1


def test_reference_is_the_mean_of_three_single_resolution_terms():
    x, y = inputs()
    t = [float(mr.stft_loss(x, y, res)) for res in mr.RES]
    assert abs(float(mr.mrstft_loss(x, y)) - sum(t) / 3) < 1e-15
    assert [tuple(mr.stft(x, res).shape) for res in mr.RES] == [(513, 42), (1025, 21), (257, 101)]
    l1 = float((x - y).abs().mean())
    assert abs(float(mr.mixed_loss(x, y, "mae", 0.2)) - (0.8 * l1 + 0.2 * sum(t) / 3)) < 1e-15
    assert float(mr.mixed_loss(x, y, "mae", 0.2, stft_loss="stft")) == float(sr.mixed_loss(x, y, "mae", 0.2))
    assert float(mr.mixed_loss(x, y, "snr", 0.0)) == float(sr.snr_loss(x, y))


def test_reference_at_the_single_resolution_is_spectral_ref():
    x, y = inputs()
    assert float(mr.stft_loss(x, y, (1024, 256, 1024))) == float(sr.stft_loss(x, y))
    assert mr.clamp_margin_ok(x, (1024, 256, 1024)) == sr.clamp_margin_ok(x)


def test_reference_reproduces_the_recorded_values():
    """n = 5003 (seed 1, fp32 roundings): L_mrstft 0.8389569 = mean(0.8380588, 0.8529485, 0.8258634); with
    x[:2048] = 0: 4.2340820, 7695 / 7175 / 10023 bins on the clamp and an fp64 gradient that is exactly
    0.0 at 1081 samples.  The GPU tests' four inputs pass the clamp-margin precondition at all three
    resolutions; n = 1025 fails it at resolution 0."""
    x, y = inputs()
    t = [float(v) for v in mr.terms(x, y)]
    assert abs(float(mr.mrstft_loss(x, y)) - 0.8389569) < 1e-6
    assert max(abs(a - b) for a, b in zip(t, (0.8380588, 0.8529485, 0.8258634))) < 1e-6
    xc, _ = inputs(clamp=True)
    assert abs(float(mr.mrstft_loss(xc, y)) - 4.2340820) < 1e-6
    assert [int((mr.power(xc, res) <= mr.EPS).sum()) for res in mr.RES] == [7695, 7175, 10023]
    _, g = mr.loss_and_grad(mr.mrstft_loss, xc, y)
    assert int((g == 0).sum()) == 1081
    for n in (1536, 5003, 8448):
        assert mr.clamp_margin_ok(inputs(n)[0])
    assert mr.clamp_margin_ok(xc)
    x1025 = inputs(1025)[0]
    assert not mr.clamp_margin_ok(x1025, mr.RES[0]) and not mr.clamp_margin_ok(x1025)


# ------------------------------------------------------------------ the tables
@pytest.fixture(scope="module")
def basis(lib):
    nb = int(lib.siren_mrstft_basis_floats())
    assert nb == sum(2 * 2 * k * b for k, b in zip(KWP, NBP))
    host = torch.full((nb,), float("nan"), dtype=torch.float32)
    assert lib.siren_mrstft_basis_fill(host.data_ptr()) == 0
    return host.numpy()


@pytest.mark.parametrize("r", [0, 1, 2])
def test_basis_tables_vs_fp64_dft_of_the_padded_window(basis, r):
    """Row k' of resolution r's table is the windowed DFT of the unit impulse at tap pad + k':
    w_k' exp(-2 pi i (pad + k') bin / n_fft), here from an fp64 rfft of diag(padded window).  Only the
    rows of the window's support are kept.  Both fragment layouts hold the same fp32 values, each the
    correctly rounded fp64 value up to the fp64 evaluation's own error; the rows past win_length, the
    row of tap 0 (where the periodic Hann is exactly 0) and the pad bins are zero."""
    n_fft, _, win = mr.RES[r]
    kwp, nbp, nb, pad = KWP[r], NBP[r], n_fft // 2 + 1, (n_fft - win) // 2
    off = sum(2 * 2 * k * b for k, b in zip(KWP[:r], NBP[:r]))
    half = 2 * kwp * nbp
    fwd = basis[off:off + half].reshape(2, kwp // 16, nbp, 16).transpose(0, 2, 1, 3).reshape(2, nbp, kwp)
    bwd = basis[off + half:off + 2 * half].reshape(2, nbp // 16, kwp, 16).transpose(0, 1, 3, 2).reshape(2, nbp, kwp)
    assert np.array_equal(fwd, bwd)                                                 # [c][bin][k']
    assert not fwd[:, nb:].any() and not fwd[:, :, win:].any() and not fwd[:, :, 0].any()
    wpad = torch.zeros(n_fft, dtype=torch.float64)
    wpad[pad:pad + win] = torch.hann_window(win, periodic=True, dtype=torch.float64)
    D = torch.fft.rfft(torch.diag(wpad), dim=1).numpy()[pad:pad + win]              # [k'][bin]
    ref = np.stack([D.real.T, D.imag.T])                                            # [c][bin][k']
    err = np.abs(fwd[:, :nb, :win].astype(np.float64) - ref)
    assert err.max() <= 2.0 ** -25 + 1e-14, err.max()    # half an ulp of values below 1, plus the FFT's error
    assert np.abs(fwd).max() > 0.99


# ------------------------------------------------------------------ sizing and validation without a device
def test_sizing_helpers(lib):
    assert [lib.siren_mrstft_frames(5003, r) for r in range(3)] == [42, 21, 101]
    assert [lib.siren_mrstft_frames(441000, r) for r in range(3)] == [3676, 1838, 8821]
    assert [lib.siren_mrstft_frames(1024, r) for r in range(3)] == [0, 0, 0]      # reflect needs n > 1024
    assert all(lib.siren_mrstft_frames(1025, r) > 0 for r in range(3))
    assert lib.siren_mrstft_frames(5003, 3) == 0 and lib.siren_mrstft_frames(5003, -1) == 0
    assert lib.siren_mrstft_workspace_floats(5003, 4096) == -1                     # rows < n
    assert lib.siren_mrstft_workspace_floats(0, 256) == -1
    ws = lib.siren_mrstft_workspace_floats(5003, 5120)
    offs = [[lib.siren_mrstft_ws_offset(5003, 5120, r, k) for k in range(6)] for r in range(3)]
    flat = [o for row in offs for o in row[:5]]
    assert flat == sorted(flat) and flat[0] == 0 and len(set(flat)) == 15
    for r, T in enumerate((42, 21, 101)):
        o = offs[r]
        assert [o[k + 1] - o[k] for k in range(4)] == [T * NBP[r]] * 4
        if r < 2:
            assert offs[r + 1][0] >= o[4] + T * KWP[r]
    assert offs[0][5] == offs[1][5] == offs[2][5] >= offs[2][4] + 101 * 240          # one set of scalars
    assert offs[0][5] + 32 + 5120 <= ws
    assert all(o % 4 == 0 for row in offs for o in row)                             # 16-byte pieces
    assert lib.siren_mrstft_ws_offset(5003, 5120, 0, 6) == -1
    assert lib.siren_mrstft_ws_offset(5003, 5120, 3, 0) == -1
    # the SNR loss alone has no frame: a short signal still sizes its workspace
    assert lib.siren_mrstft_workspace_floats(300, 512) > 0


def test_validation_without_device(lib):
    NULL, SHAPE, CONFIG = 1002, 1001, 1003
    assert lib.siren_mrstft_basis_fill(None) == NULL
    assert lib.siren_mrstft_forward(None, 5003, 5120, 1, 1, 0, None) == NULL
    assert lib.siren_mrstft_forward(1, 5003, 5120, None, 1, 0, None) == NULL
    assert lib.siren_mrstft_forward(1, 5003, 5120, 1, None, 0, None) == NULL
    assert lib.siren_mrstft_forward(1, 1024, 1024, 1, 1, 0, None) == SHAPE        # n <= 1024
    assert lib.siren_mrstft_forward(1, 5003, 4096, 1, 1, 0, None) == SHAPE        # rows < n
    assert lib.siren_mrstft_forward(1, 5003, 5120, 1, 1, 2, None) == CONFIG       # target is 0 or 1
    assert lib.siren_mrstft_loss(5003, 5120, None, 1, None) == NULL
    assert lib.siren_mrstft_loss(5003, 5120, 1, None, None) == NULL
    assert lib.siren_mrstft_loss(1000, 1024, 1, 1, None) == SHAPE
    assert lib.siren_mrstft_loss_bwd(5003, 5120, None, 1, 1, None) == NULL
    assert lib.siren_mrstft_loss_bwd(5003, 5120, 1, None, 1, None) == NULL
    assert lib.siren_mrstft_loss_bwd(5003, 5120, 1, 1, None, None) == NULL
    assert lib.siren_mrstft_loss_bwd(1024, 1024, 1, 1, 1, None) == SHAPE


def _valid_batch():
    """A net / grads / batch whose every required pointer is set (never dereferenced: validation
    returns before any launch)."""
    from inr_for_audio_amd._lib import SirenBatch, SirenGrads, SirenNet
    net, gr, b = SirenNet(), SirenGrads(), SirenBatch()
    net.in_dim, net.hidden, net.n_inner = 1, 128, 1
    net.W0 = net.b0 = net.w_head = net.b_head = 1
    net.b[0] = net.Wh[0] = net.WTh[0] = 1
    b.rows, b.n_valid, b.n_total, b.splits = 5120, 5003, 5003.0, 1
    for k in ("coords", "target", "out", "g", "head_part", "sse_part", "gsum_part", "gmax_part", "gscale",
              "col_part", "col_part2", "red_tmp", "slab"):
        setattr(b, k, 1)
    b.Y[0] = b.Y[1] = b.C[0] = b.C[1] = b.dZ[0] = b.dZ[1] = 1
    return net, gr, b


def test_train_step_mrstft_validates_its_arguments(lib):
    """siren_train_step_mrstft refuses as siren_train_step_spectral does, with n > 1024 for the
    transforms -- all before the gradient destinations are looked at (grads is empty here)."""
    from inr_for_audio_amd._lib import SirenSpectralMR
    step = lambda net, gr, b, sp: lib.siren_train_step_mrstft(ctypes.byref(net), ctypes.byref(gr), ctypes.byref(b),  # noqa: E731
                                                              None if sp is None else ctypes.byref(sp), None)
    net, gr, b = _valid_batch()
    sp = SirenSpectralMR()
    assert step(net, gr, b, None) == 1002           # no loss struct
    assert step(net, gr, b, sp) == 1002             # alpha 0, mse: the plain step (NULL grads)
    b.loss_mode = 3
    assert step(net, gr, b, sp) == 1003
    b.loss_mode = 2
    assert step(net, gr, b, sp) == 1002             # 'snr' without its workspace
    sp.ws = 1
    b.n_total = 10000.0
    assert step(net, gr, b, sp) == 1003             # a shard of a larger signal
    b.n_total, b.loss_mode, sp.alpha = 5003.0, 0, 0.2
    assert step(net, gr, b, sp) == 1002             # alpha without the tables
    sp.basis = 1
    for bad in (-0.1, 1.5, float("nan")):
        sp.alpha = bad
        assert step(net, gr, b, sp) == 1003
    for n in (512, 1024):
        sp.alpha, b.n_valid, b.n_total, b.rows = 0.2, n, float(n), 1024
        assert step(net, gr, b, sp) == 1001         # reflect padding undefined at n <= 1024
    b.n_valid, b.n_total, b.rows = 1025, 1025.0, 1152
    assert step(net, gr, b, sp) == 1002             # n = 1025 passes the shape check (then: NULL grads)
    b.n_valid, b.n_total, b.rows = 1024, 1024.0, 1024
    b.loss_mode, sp.alpha = 2, 0.0
    assert step(net, gr, b, sp) == 1002             # 'snr' alone takes a short signal (then: NULL grads)


def test_the_struct_of_its_own(lib):
    """siren_spectral_mr is registered as struct 9; siren_spectral (8) and the ABI version stay."""
    from inr_for_audio_amd import _lib
    assert [f[0] for f in _lib.SirenSpectralMR._fields_] == ["alpha", "basis", "ws"]
    assert lib.siren_struct_size(9) == ctypes.sizeof(_lib.SirenSpectralMR) == 24
    assert lib.siren_struct_size(8) == 24 and lib.siren_struct_size(10) == -1
    assert lib.siren_abi_version() == 12
    assert lib.siren_stft_basis_floats() == 2 * 2 * 1024 * 528 and lib.siren_stft_ws_offset(5000, 5120, 6) == -1


# ------------------------------------------------------------------ the engine's and train()'s switch
def test_engine_refuses_before_it_touches_a_device():
    from inr_for_audio_amd.engine import SirenEngine
    t, y = torch.linspace(-1, 1, 1024).reshape(-1, 1), torch.zeros(1024)
    with pytest.raises(ValueError, match="stft_loss"):
        SirenEngine(None, t, y, alpha=0.2, stft_loss="mr")
    with pytest.raises(ValueError, match="1024"):
        SirenEngine(None, t, y, loss_mode="mae", alpha=0.2, stft_loss="mrstft")


def test_train_without_the_switch_still_refuses(tmp_path):
    from inr_for_audio_amd.run import train
    with pytest.raises(NotImplementedError, match="restated_losses"):
        train(str(tmp_path), "t", "clip", 1, alpha=0.2, stft_loss="mrstft")
    assert not list(tmp_path.iterdir())


def test_train_refuses_an_unknown_stft_loss(tmp_path):
    from inr_for_audio_amd.run import train
    with pytest.raises(ValueError, match="stft_loss"):
        train(str(tmp_path), "t", "clip", 1, alpha=0.2, restated_losses=True, stft_loss="multi")
    assert not list(tmp_path.iterdir())
    import inspect
    p = inspect.signature(train).parameters["stft_loss"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "stft"


def test_train_refuses_a_clip_of_1024_samples(tmp_path):
    from inr_for_audio_amd.run import train
    d = tmp_path / "data"
    d.mkdir()
    rng = np.random.default_rng(0)
    wavfile.write(str(d / "short.wav"), 1024, (rng.standard_normal(2048) * 3000).astype(np.int16))
    with pytest.raises(ValueError, match="1024"):
        train(str(tmp_path / "exp"), "t", "short", 1, loss_mode="mae", alpha=0.2, data_dir=str(d),
              restated_losses=True, stft_loss="mrstft")
