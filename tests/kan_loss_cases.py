"""The broadband KAN signal of the spectral-loss tests (test_gpu_kan_losses.py, test_kan_losses_host.py).

A KAN's output on the linspace grid is a smooth curve: its upper STFT bins hold rounding noise around
the losses' clamp (|X|^2 = 1e-8), where an fp32 evaluation can land on the other side of it, and the
references' clamp_margin_ok precondition fails.  So the coordinates are uniform draws in [-1, 1), not
sorted, and the last layer's base_weight and spline_scaler are multiplied by 40: consecutive samples are
unrelated, and every bin's power lies far above the clamp (at seed 0 the smallest is at least 8e-7
against the band's upper edge 4e-8).

The models of WIDTHS start from a recorded state (tests/golden/kan_spectral_init.npz, written once by
`python tests/kan_loss_cases.py` from model(widths) under seed 0): KAN's least-squares init is not
bit-reproducible under one seed, and the gradient bound's statistic (a max-norm dominated by the weakest
bins) moved between 0.7 and 18 x e_torch32 from one process's init to the next.  With the recorded state
every figure of the GPU tests is the same in every run."""
import os

import numpy as np
import torch

import spectral_ref as sr

N = 5000          # the size of the MLP's loss tests
HEAD_GAIN = 40.0
SEED = 0
CASES = [("mse", 0.2, "stft"), ("mae", 0.2, "stft"), ("mae", 1.0, "stft"), ("snr", 0.0, "stft"),
         ("snr", 0.2, "stft"), ("mae", 0.2, "mrstft"), ("snr", 0.2, "mrstft")]
WIDTHS = [[1, 64, 64, 1], [1, 32, 16, 1]]


def coords():
    return torch.rand(N, 1, generator=torch.Generator().manual_seed(7)) * 2 - 1


def target():
    return sr.signals(N)[1].float()


def model(widths, seed=SEED):
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(seed)
    m = KAN(widths)
    with torch.no_grad():
        m.layers[-1].base_weight.mul_(HEAD_GAIN)
        m.layers[-1].spline_scaler.mul_(HEAD_GAIN)
    return m


INIT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kan_spectral_init.npz")


def _key(widths):
    return "x".join(str(w) for w in widths)


def recorded_model(widths):
    """model(widths) on the recorded state where there is one (WIDTHS), the seeded model otherwise."""
    m = model(widths)
    if list(widths) in WIDTHS:
        z = np.load(INIT)
        pre = _key(widths) + "/"
        m.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)})
    return m


if __name__ == "__main__":   # writes the recorded states (CPU; the package's own KAN)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    for w in WIDTHS:
        for k, v in model(w).state_dict().items():
            out[f"{_key(w)}/{k}"] = v.detach().numpy().astype(np.float32).copy()
    np.savez_compressed(INIT, **out)
    print(f"{INIT}: {os.path.getsize(INIT)} bytes, {len(out)} arrays")
