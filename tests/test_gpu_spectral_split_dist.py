"""The split spectral step data-parallel: 2 ranks (one process each) sharing the box's GPU
over gloo, as test_gpu_dist.py.  The ranks' out shards are gathered by a SUM all-reduce of a buffer that
is zero outside the own shard, each rank runs the loss on its window of frame blocks, and one SUM
all-reduce completes the partial arrays.  Sharded step == the single-process one-batch default step."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, OMEGA0, SEED = 5003, 128, 30000.0, 6
# name: (loss_mode, alpha, stft_loss, micro_batch, micro-batches per rank)
CFGS = {"mae_mrstft": ("mae", 0.2, "mrstft", 1 << 20, 1), "snr_stft_mb": ("snr", 0.2, "stft", 1024, 3)}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup():
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mrstft_ref as mr
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(SEED)
    m = SirenWithSnakeTanh(1, 1, H, 2, 0, 0, first_omega_0=OMEGA0, hidden_omega_0=30.0)
    _, y = mr.signals(N)
    return m, torch.linspace(-1, 1, N).reshape(N, 1), y.float()


def _engine(cfg, **kw):
    from inr_for_audio_amd.engine import SirenEngine
    loss_mode, alpha, kind, mb, _ = CFGS[cfg]
    m, t, y = _setup()
    return SirenEngine(m, t, y, lr=1e-4, device=torch.device("cuda:0"), loss_mode=loss_mode, alpha=alpha,
                       stft_loss=kind, **kw)


def _rank(rank, world, port, q, cfg):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = _engine(cfg, micro_batch=CFGS[cfg][3], split_spectral=True)
    assert eng._buckets is not None and eng.n_micro == CFGS[cfg][4] and eng.split_spectral
    eng.step()
    g1 = eng.grads.cpu().numpy().copy()
    eng.step()
    torch.cuda.synchronize()
    q.put((rank, eng.n_local, g1, eng.params.cpu().numpy().copy(), eng.history()[0]))
    dist.destroy_process_group()


@pytest.mark.parametrize("cfg", list(CFGS))
def test_two_rank_split_step_matches_single(lib, cfg):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, cfg)) for r in range(2)]
    for p in procs:
        p.start()
    try:   # each process under a time limit, its exit code checked; none outlives the test
        res = dict((r[0], r[1:]) for r in (q.get(timeout=300) for _ in range(2)))
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    eng = _engine(cfg)
    eng.step()
    g_full = eng.grads.cpu().numpy().copy()
    eng.step()
    torch.cuda.synchronize()
    npar = eng.layout.n_params
    assert res[0][0] + res[1][0] == N
    for r in (0, 1):
        n_local, g1, p2, losses = res[r]
        rel = np.linalg.norm(g1[:npar] - g_full[:npar]) / np.linalg.norm(g_full[:npar])
        print(f"{cfg} rank {r}: grads rel {rel:.2e}, losses {losses} vs {eng.history()[0]}")
        assert rel < 1e-3
        assert np.allclose(losses, eng.history()[0], rtol=1e-4)
    assert np.array_equal(res[0][2], res[1][2])  # replicated optimizer stays in lockstep
