"""Generate tests/golden/kan_grids_init.npz and trajectory_kan_grids.json from the REFERENCE's KAN.

Runs where the reference (senyuanfan/inr-for-audio) is mounted, on the CPU; imports its own kan.py and
writes data only.  For grid_size G in 4 and 11: the initial state_dict of KAN([1, 16, 16, 1], grid_size=G)
under seed 0 (keys ``g{G}_<state dict key>``; the least-squares init is not bit-reproducible under one
seed, so the test loads these very numbers) and two traces of 30 full-batch steps on gt_bach 1 s
(tests/golden/gt_bach_1s.npz) with nn.MSELoss, Adam(1e-3) and ReduceLROnPlateau as run.py:116-117,
:125, :156-187 set them up:

  loss / lr      the reference's loop as it stands (one forward, one backward per step)
  loss_chunked   the same loop with the mean taken as two half-batch backward passes accumulated:
                 the reference's own sensitivity to the summation order

    python tests/golden/make_golden_kan_grids.py [--ref /root/reference]

Printed and stored per grid size as `spread`: max |loss_chunked - loss| / loss over the steps.  The
GPU test holds every loss within 1e-3 relative of `loss`; a spread above 1e-4 would leave that gate
little room.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
WIDTHS, SEED, STEPS, GRIDS = [1, 16, 16, 1], 0, 30, (4, 11)


def loop(model, x, y, steps, chunks):
    """run.py:156-187 with loss_mode='mse', alpha = 0; `chunks` > 1 accumulates the mean's gradient over
    that many contiguous slices of the batch."""
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.8, patience=200, min_lr=1e-6)
    n = x.shape[0]
    bounds = [n * k // chunks for k in range(chunks + 1)]
    losses, lrs = [], []
    for _ in range(steps):
        opt.zero_grad()
        if chunks == 1:
            loss = torch.nn.MSELoss()(model(x.reshape(1, n, 1)), y.reshape(1, n, 1))
            loss.backward()
        else:
            loss = torch.zeros(())
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                part = torch.nn.MSELoss(reduction="sum")(model(x[lo:hi].reshape(1, -1, 1)), y[lo:hi].reshape(1, -1, 1)) / n
                part.backward()
                loss = loss + part.detach()
        losses.append(float(loss.item()))
        opt.step()
        sched.step(loss)
        lrs.append(float(sched.get_last_lr()[0]))
    return np.array(losses), np.array(lrs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import kan as ref_kan  # noqa: E402  (the reference's own module)

    g = np.load(os.path.join(OUT, "gt_bach_1s.npz"))
    x = torch.from_numpy(g["coords"].reshape(-1, 1).astype(np.float32))
    y = torch.from_numpy(g["target"].reshape(-1).astype(np.float32))
    init, traj = {}, {"steps": STEPS, "widths": WIDTHS, "seed": SEED, "grids": {}}
    for G in GRIDS:
        torch.manual_seed(SEED)
        model = ref_kan.KAN(WIDTHS, grid_size=G)
        for k, v in model.state_dict().items():
            init[f"g{G}_{k}"] = v.detach().numpy().astype(np.float32).copy()
        twin = copy.deepcopy(model)
        loss, lr = loop(model, x, y, STEPS, 1)
        loss_chunked, lr_chunked = loop(twin, x, y, STEPS, 2)
        assert np.array_equal(lr, lr_chunked)
        spread = float(np.max(np.abs(loss_chunked - loss) / loss))
        traj["grids"][str(G)] = {"loss": loss.tolist(), "lr": lr.tolist(), "loss_chunked": loss_chunked.tolist(),
                                 "spread": spread}
        print(f"kan grid_size {G}: losses {loss[:3]} ... {loss[-1]:.6e}; chunked spread {spread:.3e}")
    np.savez_compressed(os.path.join(OUT, "kan_grids_init.npz"), **init)
    json.dump(traj, open(os.path.join(OUT, "trajectory_kan_grids.json"), "w"))


if __name__ == "__main__":
    main()
