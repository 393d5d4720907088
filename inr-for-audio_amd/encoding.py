"""Gaussian random-Fourier-feature input encoding -- run.py:141-144.

The reference draws ``rff.layers.GaussianEncoding(10.0, 1, num_freq)`` after building the model
and feeds the network ``encoding(model_input)``.  The ``rff`` package is only this formula:

* ``b = torch.randn(encoded_size, input_size) * sigma`` (not trained);
* ``v -> cat(cos(2 pi v b^T), sin(2 pi v b^T), dim=-1)``, cosines first.

``GaussianEncoding`` mirrors that class (same constructor, same draw under the same seed).
Called on a CUDA tensor it runs siren_rff_encode (the stand-alone HIP kernel, fp32 out); inside
``SirenEngine(..., encoding=enc)`` the encoding is built in the first layer's kernel instead and
the [N][2F] matrix never reaches memory.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib

MAX_FREQ = 256  # kRffMaxFreq: the encoded first layer's K = 2F <= 512


class GaussianEncoding(nn.Module):
    """rff.layers.GaussianEncoding(sigma, input_size, encoded_size, b=None); input_size must be 1
    (the reference passes 1: waveform fitting only, run.py:142)."""

    def __init__(self, sigma=None, input_size=None, encoded_size=None, b=None):
        super().__init__()
        if b is None:
            if sigma is None or input_size is None or encoded_size is None:
                raise ValueError('Arguments "sigma," "input_size," and "encoded_size" are required.')
            b = torch.randn(int(encoded_size), int(input_size)) * sigma
        elif sigma is not None or input_size is not None or encoded_size is not None:
            raise ValueError('Only specify the "b" argument when using it.')
        b = torch.as_tensor(b, dtype=torch.float32)
        if b.dim() != 2 or b.shape[1] != 1:
            raise NotImplementedError(f"HIP path: input_size must be 1 (run.py:142), got b of shape {tuple(b.shape)}")
        if not 1 <= b.shape[0] <= MAX_FREQ:
            raise NotImplementedError(f"HIP path: encoded_size must be in 1..{MAX_FREQ}, got {b.shape[0]}")
        self.b = nn.Parameter(b.clone(), requires_grad=False)

    @property
    def encoded_size(self) -> int:
        return int(self.b.shape[0])

    def forward(self, v: torch.Tensor) -> torch.Tensor:
        """[..., 1] CUDA coordinates -> [..., 2 encoded_size] fp32 (cosines, then sines)."""
        if not v.is_cuda:
            raise RuntimeError("GaussianEncoding runs on the HIP path only (CUDA tensors)")
        if v.shape[-1] != 1:
            raise ValueError(f"expected coordinates [..., 1], got {tuple(v.shape)}")
        lib = _lib.load()
        x = v.detach().reshape(-1).contiguous().float()
        bd = self.b.detach().to(v.device, torch.float32).reshape(-1).contiguous()
        F = self.encoded_size
        out = torch.empty(x.numel(), 2 * F, dtype=torch.float32, device=v.device)
        s = torch.cuda.current_stream(v.device).cuda_stream
        _lib.check(lib.siren_rff_encode(_lib.ptr(x), _lib.ptr(bd), F, x.numel(), _lib.ptr(out), s),
                   "siren_rff_encode")
        return out.reshape(*v.shape[:-1], 2 * F)
