"""The oscillating fits of the keep_best tests (test_gpu_keep_best.py, test_gpu_keep_best_dist.py): models,
data and the learning rate / step count of every case.

SIREN: width 128, 3 sine layers, the two-sine target of test_gpu_landscape_dist.py.  KAN: KAN([1, 8, 8, 1]) at
grid 5 and 11, started from a recorded state (tests/golden/kan_keep_best_init.npz, written once by
`python tests/keep_best_cases.py` under seed 0): KAN's least-squares init is not bit-reproducible under one
seed (kan_loss_cases.py), and whether a fit oscillates depends on where it starts.

The learning rates were picked on the GPU (60 steps each; "taken" snapshots, best step):
on the CPU in plain fp32 torch the SIREN at lr 2.5e-3 gave 8 snapshots with the best at step 42 and was
monotone at 1e-3; the fp16 path at 2.5e-3 gives 8 snapshots with the best at step 27.  Each test asserts its
own run's figures (at least 3 snapshots, best step not 0 and at least 5 steps before the last)."""
import os

import numpy as np
import torch

H, COUNTS, W0, W = 128, (3, 0, 0), 1000.0, 30.0
KAN_WIDTHS = [1, 8, 8, 1]
STEPS = 60
INIT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kan_keep_best_init.npz")

# case: (coordinates, engine keywords, seed, lr) -- measured (taken, best step) in the comment
SIREN_CASES = {
    "plain": (1000, {}, 0, 2.5e-3),                                   # 8, 27
    "micro": (1000, {"micro_batch": 384}, 0, 5e-3),                   # two micro-batches of 512 rows: 4, 23
    "spectral": (2048, {"loss_mode": "mae", "alpha": 0.2}, 1, 1e-3),  # n_total = 1.0: 6, 37
}
# case: (coordinates, grid size, engine keywords, lr); at grid 5 lr 0.1 .. 0.2 fell to the last step, 1.0 never improved
KAN_CASES = {
    "g5": (1000, 5, {}, 0.05),                                                                # 32, 49
    "g11": (1000, 11, {}, 0.3),                                                               # 7, 44
    "micro": (1000, 5, {"micro_batch": 384}, 0.05),                                           # 32, 49
    "spectral": (2048, 5, {"loss_mode": "mae", "alpha": 0.2, "split_spectral": True}, 0.2),   # n_total = 1.0: 8, 45
}


def data(n):
    t = torch.linspace(-1, 1, n).reshape(n, 1)
    return t, (0.5 * torch.sin(37 * t) + 0.2 * torch.sin(91 * t)).reshape(-1)


def siren_model(seed):
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(seed)
    return SirenWithSnakeTanh(1, 1, H, *COUNTS, first_omega_0=W0, hidden_omega_0=W)


def kan_model(grid):
    from inr_for_audio_amd.kan import KAN
    torch.manual_seed(0)
    m = KAN(KAN_WIDTHS, grid_size=grid)
    z = np.load(INIT)
    pre = f"g{grid}/"
    m.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)})
    return m


def siren_engine(case, dev, keep_best, lr=None):
    from inr_for_audio_amd.engine import SirenEngine
    n, kw, seed, lr0 = SIREN_CASES[case]
    t, y = data(n)
    return SirenEngine(siren_model(seed), t, y, lr=lr or lr0, device=dev, keep_best=keep_best, **kw)


def kan_engine(case, dev, keep_best, lr=None):
    from inr_for_audio_amd.engine import KanEngine
    n, grid, kw, lr0 = KAN_CASES[case]
    t, y = data(n)
    return KanEngine(kan_model(grid), t, y, lr=lr or lr0, device=dev, keep_best=keep_best, **kw)


if __name__ == "__main__":   # writes the recorded states (CPU; the package's own KAN)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from inr_for_audio_amd.kan import KAN
    out = {}
    for g in (5, 11):
        torch.manual_seed(0)
        for k, v in KAN(KAN_WIDTHS, grid_size=g).state_dict().items():
            out[f"g{g}/{k}"] = v.detach().numpy().astype(np.float32).copy()
    np.savez_compressed(INIT, **out)
    print(f"{INIT}: {os.path.getsize(INIT)} bytes, {len(out)} arrays")
