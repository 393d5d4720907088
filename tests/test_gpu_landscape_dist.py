"""SirenEngine.loss_plane in a process group: 2 ranks (one process each) sharing the box's GPU, gloo
carrying the broadcast of rank 0's directions and the SUM all-reduce of the cells' fp64 sums (as
test_gpu_dist.py does for the gradients).  Both ranks return one plane, and it meets the fp64 formula."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import landscape_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, H, COUNTS = 1000, 4, 128, (3, 0, 0)
GATE = 1e-4   # DESIGN 3's loss gate of a sine stack (test_gpu_landscape.py)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup():
    import sys
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(0)
    m = SirenWithSnakeTanh(1, 1, H, *COUNTS, first_omega_0=1000.0, hidden_omega_0=30.0)
    t = torch.linspace(-1, 1, N).reshape(N, 1)
    return m, t, (0.5 * torch.sin(37 * t) + 0.2 * torch.sin(91 * t)).reshape(-1)


def _rank(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from inr_for_audio_amd.engine import SirenEngine
    from inr_for_audio_amd.landscape import plane_directions
    m, t, y = _setup()
    eng = SirenEngine(m, t, y, device=torch.device("cuda:0"))
    eng.step()
    # each rank draws its own directions: rank 0's are the ones every rank must use
    d1, d2 = plane_directions([p for _, p in m.named_parameters()], steps=STEPS,
                              generator=torch.Generator().manual_seed(20 + rank))
    plane = eng.loss_plane(d1, d2, STEPS)
    theta = [p.detach().cpu().numpy().copy() for _, p in m.named_parameters()]
    q.put((rank, eng.n_local, plane.numpy(), theta, [x.numpy() for x in d1], [x.numpy() for x in d2]))
    dist.destroy_process_group()


def test_two_rank_plane(lib):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r[0], r[1:]) for r in (q.get(timeout=300) for _ in range(2)))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res[0][0] + res[1][0] == N
    plane = res[0][1]
    assert plane.shape == (STEPS, STEPS) and plane.dtype == np.float64
    assert np.array_equal(plane.view(np.int64), res[1][1].view(np.int64))
    m, t, y = _setup()
    names = [k for k, _ in m.named_parameters()]
    _, _, theta, d1, d2 = res[0]      # rank 0's directions: the ones both ranks used
    assert all(np.array_equal(a, b) for a, b in zip(theta, res[1][2]))
    assert not all(np.array_equal(a, b) for a, b in zip(d1, res[1][3]))
    worst = 0.0
    for i in range(STEPS):
        for j in range(STEPS):
            p = ref.oracle_params(names, ref.cell_params(theta, d1, d2, STEPS, i, j), COUNTS)
            want = ref.cell_loss(p, t.numpy(), y.numpy(), 1000.0, 30.0)
            worst = max(worst, abs(plane[i, j] - want) / want)
    print(f"landscape dist: worst {worst:.3e}")
    assert worst <= GATE, worst
