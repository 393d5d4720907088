"""The KAN's phased spectral step data-parallel: 2 ranks (one process each) sharing the box's GPU over
gloo, as test_gpu_spectral_split_dist.py.  The ranks' out shards are gathered by a SUM all-reduce, each
rank runs the loss on its window of frame blocks, one SUM all-reduce completes the partial arrays: the
loss and every rank's slice of g_sig are the single-process phased step's bit for bit, and the
gradients and parameters agree to that file's tolerance (the ranks' split-K slices differ)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS, CASE = [1, 64, 64, 1], ("mae", 0.2, "stft")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _engine(sd_path):
    """Every process loads one state dict: KAN's least-squares init is not bit-reproducible."""
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kan_loss_cases as kc
    from inr_for_audio_amd.engine import KanEngine
    m = kc.model(WIDTHS)
    m.load_state_dict(torch.load(sd_path, weights_only=True))
    loss_mode, alpha, kind = CASE
    return KanEngine(m, kc.coords(), kc.target(), device=torch.device("cuda:0"), loss_mode=loss_mode, alpha=alpha,
                     stft_loss=kind, split_spectral=True)


def _rank(rank, world, port, q, sd_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = _engine(sd_path)
    assert eng.split_spectral and eng.n_micro == 1
    eng.step()
    torch.cuda.synchronize()
    q.put((rank, eng._sig_lo, eng._sig_hi, eng.g_sig.cpu().numpy().copy(), eng.grads.cpu().numpy().copy(),
           eng.params.cpu().numpy().copy(), eng.history()[0]))
    dist.destroy_process_group()


def test_two_rank_phased_step_matches_single(lib, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kan_loss_cases as kc
    sd_path = str(tmp_path / "kan_sd.pt")
    torch.save(kc.recorded_model(WIDTHS).state_dict(), sd_path)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, sd_path)) for r in range(2)]
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
    eng = _engine(sd_path)
    eng.step()
    torch.cuda.synchronize()
    npar = eng.layout.n_params
    g_sig, grads, params, losses = (eng.g_sig.cpu().numpy(), eng.grads.cpu().numpy(), eng.params.cpu().numpy(),
                                    eng.history()[0])
    assert (res[0][0], res[0][1], res[1][1]) == (0, res[1][0], kc.N)
    for r in (0, 1):
        lo, hi, g_r, gr_r, p_r, loss_r = res[r]
        assert np.array_equal(g_r[lo:hi].view(np.int32), g_sig[lo:hi].view(np.int32))
        assert np.array_equal(loss_r.view(np.int32), losses.view(np.int32))
        rel = np.linalg.norm(gr_r[:npar] - grads[:npar]) / np.linalg.norm(grads[:npar])
        prel = np.linalg.norm(p_r[:npar] - params[:npar]) / np.linalg.norm(params[:npar])
        print(f"rank {r}: grads rel {rel:.2e}, params rel {prel:.2e}, loss {loss_r} vs {losses}")
        assert rel < 1e-3 and prel < 1e-3
    assert np.array_equal(res[0][4], res[1][4])  # replicated optimizer stays in lockstep
