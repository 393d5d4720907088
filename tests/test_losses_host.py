"""STFT / SNR losses (run.py:126-128, :160-169), the parts that need no GPU: the fp64 reference
against closed forms, the transform's tables against an fp64 DFT of unit impulses, host-side
argument validation of the new entry points, and train()'s opt-in switch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import spectral_ref as sr


# ------------------------------------------------------------------ the reference itself
def test_reference_identical_signals_give_zero_stft_loss():
    x, y = sr.signals(5000)
    assert float(sr.stft_loss(y, y)) == 0.0
    assert float(sr.stft_loss(x, y)) > 0.1


def test_reference_scaled_copy_gives_the_analytic_snr():
    """x = a y: r = (a - 1) yc, so L_snr = -10 log10(1 / (a - 1)^2) up to the two eps."""
    _, y = sr.signals(5000)
    for a in (0.5, 0.9, 1.25):
        want = -10.0 * math.log10(1.0 / (a - 1.0) ** 2)
        assert abs(float(sr.snr_loss(a * y + 0.3, y)) - want) < 1e-6    # the DC offset drops out
    assert float(sr.snr_loss(0.99 * y, y)) < 0                          # negative for any useful fit


def test_reference_frames_and_clamp_case():
    """T = 1 + n // 256 frames of 513 bins; the clamp case of the GPU tests (x[:2048] = 0 at n = 5000:
    seven silent frames) has 3591 clamped bins and a loss of about 4.24; the precondition holds for
    the four inputs and fails for the one the issue names (n = 1536, seed 0)."""
    for n in (1536, 5000, 8448):
        x, _ = sr.signals(n)
        assert tuple(sr.stft(x).shape) == (513, 1 + n // 256)
        assert sr.clamp_margin_ok(x)
    x, y = sr.signals(5000)
    x[:2048] = 0
    assert sr.clamp_margin_ok(x)
    assert int((sr.power(x) <= sr.EPS).sum()) == 7 * 513 == 3591
    assert abs(float(sr.stft_loss(x, y)) - 4.24) < 0.01
    _, g = sr.loss_and_grad(sr.stft_loss, x, y)
    assert float(g[:1024].abs().max()) == 0.0
    assert not sr.clamp_margin_ok(sr.signals(1536, seed=0)[0])


def test_reference_mix():
    x, y = sr.signals(1536)
    l1, ls = float((x - y).abs().mean()), float(sr.stft_loss(x, y))
    assert abs(float(sr.mixed_loss(x, y, "mae", 0.2)) - (0.8 * l1 + 0.2 * ls)) < 1e-15
    assert float(sr.mixed_loss(x, y, "snr", 0.0)) == float(sr.snr_loss(x, y))
    assert float(sr.mixed_loss(x, y, "mse", 0.0)) == float(((x - y) ** 2).mean())


# ------------------------------------------------------------------ the tables
@pytest.fixture(scope="module")
def basis(lib):
    nb = int(lib.siren_stft_basis_floats())
    assert nb == 2 * 2 * 1024 * 528
    host = torch.full((nb,), float("nan"), dtype=torch.float32)
    assert lib.siren_stft_basis_fill(host.data_ptr()) == 0
    return host.numpy()


def test_basis_tables_vs_fp64_dft_of_unit_impulses(basis):
    """Row k of the table is the windowed DFT of the unit impulse at k: w_k exp(-2 pi i k bin / 1024),
    here from an fp64 rfft of diag(hann).  Both fragment layouts hold the same fp32 values, each the
    correctly rounded fp64 value up to the fp64 evaluation's own error; pad bins are zero."""
    half = basis.size // 2
    fwd = basis[:half].reshape(2, 64, 528, 16).transpose(0, 2, 1, 3).reshape(2, 528, 1024)   # [c][bin][k]
    bwd = basis[half:].reshape(2, 33, 1024, 16).transpose(0, 1, 3, 2).reshape(2, 528, 1024)  # [c][bin][k]
    assert np.array_equal(fwd, bwd)
    assert not fwd[:, 513:].any()
    w = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    D = torch.fft.rfft(torch.diag(w), dim=1).numpy()                                          # [k][bin]
    ref = np.stack([D.real.T, D.imag.T])                                                      # [c][bin][k]
    err = np.abs(fwd[:, :513].astype(np.float64) - ref)
    assert err.max() <= 2.0 ** -25 + 1e-14, err.max()     # half an ulp of values below 1, plus the FFT's error
    # exact zeros: the window vanishes at k = 0, the imaginary part at bin 0
    assert not fwd[:, :, 0].any() and not fwd[1, 0].any()


# ------------------------------------------------------------------ validation without a device
def test_sizing_helpers(lib):
    assert lib.siren_stft_frames(5000) == 20 and lib.siren_stft_frames(1536) == 7
    assert lib.siren_stft_frames(441000) == 1723
    assert lib.siren_stft_frames(512) == 0 and lib.siren_stft_frames(513) == 3   # reflect needs n > 512
    assert lib.siren_stft_workspace_floats(5000, 4096) == -1                     # rows < n
    assert lib.siren_stft_workspace_floats(0, 256) == -1
    ws = lib.siren_stft_workspace_floats(5000, 5120)
    offs = [lib.siren_stft_ws_offset(5000, 5120, k) for k in range(6)]
    assert offs[:5] == [0, 20 * 528, 2 * 20 * 528, 3 * 20 * 528, 4 * 20 * 528]
    assert offs[5] > offs[4] + 20 * 1024 and offs[5] + 32 + 5120 <= ws
    assert all(o % 4 == 0 for o in offs)                                         # 16-byte pieces
    assert lib.siren_stft_ws_offset(5000, 5120, 6) == -1
    # the SNR loss alone has no frame: a short signal still sizes its workspace
    assert lib.siren_stft_workspace_floats(300, 512) > 0


def test_validation_without_device(lib):
    NULL, SHAPE, CONFIG = 1002, 1001, 1003
    assert lib.siren_stft_basis_fill(None) == NULL
    assert lib.siren_stft_forward(None, 5000, 5120, 1, 1, 0, None) == NULL
    assert lib.siren_stft_forward(1, 5000, 5120, None, 1, 0, None) == NULL
    assert lib.siren_stft_forward(1, 5000, 5120, 1, None, 0, None) == NULL
    assert lib.siren_stft_forward(1, 512, 512, 1, 1, 0, None) == SHAPE          # n <= 512
    assert lib.siren_stft_forward(1, 5000, 4096, 1, 1, 0, None) == SHAPE        # rows < n
    assert lib.siren_stft_forward(1, 5000, 5120, 1, 1, 2, None) == CONFIG       # target is 0 or 1
    assert lib.siren_stft_loss(5000, 5120, None, 1, None) == NULL
    assert lib.siren_stft_loss(5000, 5120, 1, None, None) == NULL
    assert lib.siren_stft_loss(400, 512, 1, 1, None) == SHAPE
    assert lib.siren_stft_loss_bwd(5000, 5120, None, 1, 1, None) == NULL
    assert lib.siren_stft_loss_bwd(5000, 5120, 1, 1, None, None) == NULL
    assert lib.siren_stft_loss_bwd(512, 512, 1, 1, 1, None) == SHAPE
    assert lib.siren_snr_loss(None, 1, 5000, 5120, 1, 1, 1, None) == NULL
    assert lib.siren_snr_loss(1, 1, 5000, 5120, 1, 1, None, None) == NULL
    assert lib.siren_snr_loss(1, 1, 0, 256, 1, 1, 1, None) == SHAPE
    assert lib.siren_snr_loss(1, 1, 5000, 4999, 1, 1, 1, None) == SHAPE


def _valid_batch():
    """A net / grads / batch whose every required pointer is set (never dereferenced: validation
    returns before any launch)."""
    from inr_for_audio_amd._lib import SirenBatch, SirenGrads, SirenNet
    net, gr, b = SirenNet(), SirenGrads(), SirenBatch()
    net.in_dim, net.hidden, net.n_inner = 1, 128, 1
    net.W0 = net.b0 = net.w_head = net.b_head = 1
    net.b[0] = net.Wh[0] = net.WTh[0] = 1
    b.rows, b.n_valid, b.n_total, b.splits = 5120, 5000, 5000.0, 1
    for k in ("coords", "target", "out", "g", "head_part", "sse_part", "gsum_part", "gmax_part", "gscale",
              "col_part", "col_part2", "red_tmp", "slab"):
        setattr(b, k, 1)
    b.Y[0] = b.Y[1] = b.C[0] = b.C[1] = b.dZ[0] = b.dZ[1] = 1
    return net, gr, b


def test_train_step_spectral_validates_its_arguments(lib):
    """siren_train_step_spectral: the loss struct, its workspace and (alpha != 0) the tables are
    required, the batch must hold the whole signal, alpha lies in [0, 1], and the STFT term needs
    n > 512 -- all refused before the gradient destinations are even looked at (grads is empty here).
    siren_train_step itself keeps its behaviour and has no workspace for loss_mode 2."""
    from inr_for_audio_amd._lib import SirenSpectral
    plain = lambda net, gr, b: lib.siren_train_step(ctypes.byref(net), ctypes.byref(gr), ctypes.byref(b), None)  # noqa: E731
    step = lambda net, gr, b, sp: lib.siren_train_step_spectral(ctypes.byref(net), ctypes.byref(gr), ctypes.byref(b),  # noqa: E731
                                                                None if sp is None else ctypes.byref(sp), None)
    net, gr, b = _valid_batch()
    sp = SirenSpectral()
    assert plain(net, gr, b) == 1002                # plain batch: passes check_batch, grads are NULL
    assert step(net, gr, b, None) == 1002           # no loss struct
    assert step(net, gr, b, sp) == 1002             # alpha 0, mse: the plain step (NULL grads)
    b.loss_mode = 3
    assert step(net, gr, b, sp) == 1003 and plain(net, gr, b) == 1003
    b.loss_mode = 2
    assert plain(net, gr, b) == 1002                # 'snr' through siren_train_step: no workspace
    assert step(net, gr, b, sp) == 1002             # 'snr' without its workspace
    sp.stft_ws = 1
    b.n_total = 10000.0
    assert step(net, gr, b, sp) == 1003             # a shard of a larger signal
    b.n_total, b.loss_mode, sp.alpha = 5000.0, 0, 0.2
    assert step(net, gr, b, sp) == 1002             # alpha without the tables
    sp.stft_basis = 1
    for bad in (-0.1, 1.5, float("nan")):
        sp.alpha = bad
        assert step(net, gr, b, sp) == 1003
    sp.alpha, b.n_valid, b.n_total, b.rows = 0.2, 512, 512.0, 512
    assert step(net, gr, b, sp) == 1001             # reflect padding undefined at n <= 512
    b.loss_mode, sp.alpha = 2, 0.0
    assert step(net, gr, b, sp) == 1002             # 'snr' alone takes a short signal (then: NULL grads)


def test_the_batch_struct_is_untouched(lib):
    """The loss options travel in a struct of their own: siren_batch keeps its layout."""
    from inr_for_audio_amd import _lib
    assert [f[0] for f in _lib.SirenBatch._fields_][-2:] == ["enc", "rff_slab"]
    assert [f[0] for f in _lib.SirenSpectral._fields_] == ["alpha", "stft_basis", "stft_ws"]
    assert lib.siren_struct_size(8) == ctypes.sizeof(_lib.SirenSpectral) == 24


# ------------------------------------------------------------------ train()'s switch
@pytest.mark.parametrize("kw", [{"loss_mode": "snr"}, {"alpha": 0.5}, {"loss_mode": "mae", "alpha": 0.01}])
def test_train_without_the_switch_still_refuses(tmp_path, kw):
    from inr_for_audio_amd.run import train
    with pytest.raises(NotImplementedError, match="restated_losses"):
        train(str(tmp_path), "t", "clip", 1, **kw)


@pytest.mark.parametrize("kw", [{"multichannel": True}, {"arch": "kan"}])
def test_train_with_the_switch_refuses_what_it_does_not_cover(tmp_path, kw):
    from inr_for_audio_amd.run import train
    with pytest.raises(NotImplementedError):
        train(str(tmp_path), "t", "clip", 1, alpha=0.2, restated_losses=True, **kw)
    assert not list(tmp_path.iterdir())             # refused before the experiment folder exists
