"""Reference of the multi-resolution STFT loss (run.py:127, :160), written with torch.stft and
autograd on the CPU: auraloss 0.4.0's MultiResolutionSTFTLoss() defaults as published
(perceptual_weighting=False, so sample_rate has no effect).

  r = 0, 1, 2: n_fft 1024 / 2048 / 512, hop 120 / 240 / 50, win_length 600 / 1200 / 240
  X_r = stft(x, n_fft, hop, win_length, periodic Hann, center, reflect), x_mag = sqrt(clamp(|X_r|^2, 1e-8))
  L_r = ||y_mag - x_mag||_F / ||y_mag||_F + mean |log x_mag - log y_mag|
  L_mrstft = (L_0 + L_1 + L_2) / 3,  loss = (1 - alpha) {L1 | L_snr | MSE} + alpha L_mrstft

torch.stft zero-pads the window to n_fft, centred.  Inputs, loss_and_grad and grad_err are
spectral_ref's; everything takes and returns tensors of the dtype it is given."""
import torch

import spectral_ref as sr
from spectral_ref import grad_err, loss_and_grad, signals  # noqa: F401  (re-exported for the tests)

RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))   # (n_fft, hop, win_length)
EPS = sr.EPS


def stft(x: torch.Tensor, res) -> torch.Tensor:
    """[n_fft / 2 + 1][1 + n // hop] complex."""
    n_fft, hop, win = res
    w = torch.hann_window(win, periodic=True, dtype=x.dtype)
    return torch.stft(x.reshape(-1), n_fft, hop_length=hop, win_length=win, window=w, center=True,
                      pad_mode="reflect", return_complex=True)


def power(x: torch.Tensor, res) -> torch.Tensor:
    X = stft(x, res)
    return X.real ** 2 + X.imag ** 2


def mag(x: torch.Tensor, res) -> torch.Tensor:
    return torch.sqrt(torch.clamp(power(x, res), min=EPS))


def stft_loss(x: torch.Tensor, y: torch.Tensor, res) -> torch.Tensor:
    """One resolution's term; at (1024, 256, 1024) it is spectral_ref.stft_loss."""
    xm, ym = mag(x, res), mag(y, res)
    sc = torch.linalg.norm(ym - xm) / torch.linalg.norm(ym)
    return sc + (torch.log(xm) - torch.log(ym)).abs().mean()


def terms(x: torch.Tensor, y: torch.Tensor):
    return [stft_loss(x, y, res) for res in RES]


def mrstft_loss(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    t = terms(x, y)
    return (t[0] + t[1] + t[2]) / 3


def mixed_loss(x: torch.Tensor, y: torch.Tensor, loss_mode: str, alpha: float, stft_loss: str = "mrstft") -> torch.Tensor:
    """run.py:161-169 with the spectral term of run.py:127 ('mrstft') or :128 ('stft')."""
    if stft_loss == "stft" or alpha == 0.0:
        return sr.mixed_loss(x, y, loss_mode, alpha)
    if stft_loss != "mrstft":
        raise ValueError(stft_loss)
    x, y = x.reshape(-1), y.reshape(-1)
    point = sr.mixed_loss(x, y, loss_mode, 0.0)
    return (1.0 - alpha) * point + alpha * mrstft_loss(x, y)


def clamp_margin_ok(x: torch.Tensor, res=None) -> bool:
    """The tests' precondition on the fp64 reference, per resolution (res None: all three): no bin's
    unclamped power lies in [eps / 4, 4 eps], where an fp32 evaluation could land on the other side
    of the clamp."""
    if res is None:
        return all(clamp_margin_ok(x, r) for r in RES)
    p = power(x.double(), res)
    return not bool(((p >= EPS / 4) & (p <= 4 * EPS)).any())
