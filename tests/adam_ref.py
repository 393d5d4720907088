"""The Adam reference shared by tests/test_gpu_elementwise.py and tests/test_host.py (a plain module:
no fixtures, nothing collected).

The reference of the bit-for-bit Adam test is torch.optim.Adam(fused=True) on the CPU: on this input
its p, exp_avg and exp_avg_sq equal oracle.siren_oracle.adam_step word for word over all five steps
(test_host.py asserts that identity).  The unfused CPU Adam rounds p differently in about 0.05 % of
the elements per step, so it is not the reference."""
import numpy as np
import torch

F32 = np.float32

# written at both ends of every gradient vector: zeros, the smallest subnormal, values whose square
# underflows, values whose square overflows after a few steps (3e20: v = +inf by step 4, so the
# update there is 0), and fp16's maximum
LATTICE = np.array([0.0, 0.0, 1e-45, -1e-45, 1e-38, -1e-38, 1e-30, -1e-30, 1e19, -1e19, 1e20, 3e20, -3e20,
                    1.0, -1.0, 65504.0], F32)
STEPS = 5
N_BIG = (1 << 20) + 3 * 256 + 5      # past adam_flat's grid cap of 4096 x 256 = 2^20 elements


def lr_at(step: int) -> float:
    return 1e-3 * step


def adam_case(n: int):
    """(p0, [g_1 .. g_5]) for n elements: test_adam_bit_exact's parameters and gradients (normal x
    10^U(-6, 0)) with LATTICE over both ends (as much of it as fits)."""
    rng = np.random.default_rng(9)
    p0 = (rng.normal(size=n) * 0.05).astype(F32)
    k = min(LATTICE.size, n)
    gs = []
    for _ in range(STEPS):
        g = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, 0, n)).astype(F32)
        g[n - k:] = LATTICE[:k][::-1]
        g[:k] = LATTICE[:k]
        gs.append(g)
    return p0, gs


def torch_fused_adam(p0: np.ndarray, gs):
    """[(p, exp_avg, exp_avg_sq)] after each step of torch.optim.Adam(fused=True) on the CPU with
    lr = lr_at(step), torch's default betas and eps."""
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=lr_at(1), fused=True)
    out = []
    for step, g in enumerate(gs, 1):
        opt.param_groups[0]["lr"] = lr_at(step)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out
