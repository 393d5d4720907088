"""Reference of the STFT and SNR losses (run.py:126-128, :160-169), written with torch.stft and
autograd on the CPU: auraloss 0.4.0's STFTLoss() and SNRLoss() defaults as published.

  X = stft(x, 1024, hop 256, win 1024, periodic Hann, center, reflect), x_mag = sqrt(clamp(|X|^2, 1e-8))
  L_stft = ||y_mag - x_mag||_F / ||y_mag||_F + mean |log x_mag - log y_mag|
  L_snr  = -10 log10(sum yc^2 / (sum (xc - yc)^2 + 1e-8) + 1e-8), xc / yc mean-removed
  loss   = (1 - alpha) {L1 | L_snr | MSE} + alpha L_stft

Everything takes and returns torch tensors of the dtype it is given (fp64 for the reference proper,
fp32 for the "what torch itself achieves in fp32" yardstick of the gradient bound)."""
import math

import torch

N_FFT, HOP, BINS, EPS = 1024, 256, 513, 1e-8


def signals(n: int, seed: int = 1):
    """The tests' input recipe: (x, y) in fp64; y two sines plus noise, x = 0.8 y + noise."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    y = (0.5 * torch.sin(2 * math.pi * 440 * t / 44100) + 0.2 * torch.sin(2 * math.pi * 3100 * t / 44100 + 1)
         + 0.05 * torch.randn(n, generator=g, dtype=torch.float64))
    x = 0.8 * y + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
    return x, y


def stft(x: torch.Tensor) -> torch.Tensor:
    """[513][T] complex, T = 1 + n // 256."""
    w = torch.hann_window(N_FFT, periodic=True, dtype=x.dtype)
    return torch.stft(x.reshape(-1), N_FFT, hop_length=HOP, win_length=N_FFT, window=w, center=True,
                      pad_mode="reflect", return_complex=True)


def power(x: torch.Tensor) -> torch.Tensor:
    X = stft(x)
    return X.real ** 2 + X.imag ** 2


def mag(x: torch.Tensor) -> torch.Tensor:
    return torch.sqrt(torch.clamp(power(x), min=EPS))


def stft_loss(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    xm, ym = mag(x), mag(y)
    sc = torch.linalg.norm(ym - xm) / torch.linalg.norm(ym)
    return sc + (torch.log(xm) - torch.log(ym)).abs().mean()


def snr_loss(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    x = x.reshape(-1) - x.mean()
    y = y.reshape(-1) - y.mean()
    r = x - y
    return -10.0 * torch.log10((y ** 2).sum() / ((r ** 2).sum() + EPS) + EPS)


def mixed_loss(x: torch.Tensor, y: torch.Tensor, loss_mode: str, alpha: float) -> torch.Tensor:
    """run.py:161-169."""
    x, y = x.reshape(-1), y.reshape(-1)
    if loss_mode == "mae":
        point = (x - y).abs().mean()
    elif loss_mode == "snr":
        point = snr_loss(x, y)
    else:
        point = ((x - y) ** 2).mean()
    if alpha == 0.0:
        return point
    return (1.0 - alpha) * point + alpha * stft_loss(x, y)


def loss_and_grad(fn, x: torch.Tensor, *args):
    """(fn(x, *args), d fn / d x) by autograd."""
    x = x.detach().clone().requires_grad_(True)
    loss = fn(x, *args)
    loss.backward()
    return loss.detach(), x.grad.detach()


def clamp_margin_ok(x: torch.Tensor) -> bool:
    """The tests' precondition on the fp64 reference: no bin's unclamped power lies in
    [eps / 4, 4 eps], where an fp32 evaluation could land on the other side of the clamp."""
    p = power(x.double())
    return not bool(((p >= EPS / 4) & (p <= 4 * EPS)).any())


def grad_err(g: torch.Tensor, g64: torch.Tensor) -> float:
    """max|g - g64| / max|g64|."""
    return float((g.double() - g64).abs().max() / g64.abs().max())
