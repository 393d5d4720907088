"""keep_best=True in a process group: 2 ranks (one process each) sharing the box's GPU, gloo carrying the
gradient all-reduce (as test_gpu_landscape_dist.py).  siren_best_keep runs after the all-reduce, on the
reduced sse slot, so both ranks take the same decisions: one (loss, step, taken) and bit-identical
best_params, and the step is the argmin of each rank's history."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 40


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    import sys
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import keep_best_cases as kc
    eng = kc.siren_engine("plain", torch.device("cuda:0"), True)
    for _ in range(STEPS):
        eng.step()
    info = eng.best_info()
    h, _ = eng.history()
    n = eng.layout.n_params
    sd = {k: v.numpy() for k, v in eng.best_state_dict().items()}
    q.put((rank, eng.n_local, info, h, eng.best_params[:n].cpu().numpy(), eng.params[:n].cpu().numpy(), sd))
    dist.destroy_process_group()


def test_two_ranks_keep_one_best(lib):
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
    assert res[0][0] + res[1][0] == 1000
    (loss, step, taken), h = res[0][1], res[0][2]
    print(f"keep_best dist: taken {taken}, best step {step} of {STEPS}, best loss {loss:.6e}, last {h[-1]:.6e}")
    assert res[1][1] == res[0][1]
    assert taken >= 3 and 0 < step <= STEPS - 1 - 5
    for r in range(2):
        hr = res[r][2]
        assert len(hr) == STEPS and step == int(np.argmin(hr)) and np.float32(loss) == hr[step]
    assert np.array_equal(h.view(np.int32), res[1][2].view(np.int32))
    assert np.array_equal(res[0][3].view(np.int32), res[1][3].view(np.int32))
    assert np.array_equal(res[0][4].view(np.int32), res[1][4].view(np.int32))        # the live weights too
    assert not np.array_equal(res[0][3].view(np.int32), res[0][4].view(np.int32))    # ... which moved on
    for k, v in res[0][5].items():
        assert np.array_equal(v.view(np.int32), res[1][5][k].view(np.int32)), k
