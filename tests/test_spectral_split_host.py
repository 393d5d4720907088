"""The split spectral step (run.py:126-128, :160-169 across micro-batches and ranks), the
parts that need no GPU: the new C-ABI symbols and their validation, the frame-block window against a
brute-force enumeration of covering frames, and the engine's / train()'s switch."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "siren_hip.h")
NULL, SHAPE, CONFIG = 1002, 1001, 1003
NEW = [f"siren_{k}_{f}" for k in ("stft", "mrstft")
       for f in ("window", "signal_parts", "signal_forward", "signal_finish", "signal_backward")]
# the trait table of csrc/stft.hip's header: (n_fft, hop, win); the first is the single transform
TRAITS = ((1024, 256, 1024), (1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
FT = 16   # frames per block


def test_symbols_are_declared_bound_and_exported(lib):
    from inr_for_audio_amd import _lib
    text = open(HEADER).read()
    for name in NEW:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|int64_t) " + name + r"\(", text, re.S)
        assert m and "run.py:" in m.group(1), name     # declared under a comment that cites the reference
        assert name in _lib._SIGS and hasattr(lib, name), name
    assert lib.siren_abi_version() == 12 == _lib.ABI_VERSION
    assert lib.siren_struct_size(10) == -1 and lib.siren_stft_ws_offset(5000, 5120, 6) == -1


def _win(*v):
    return (ctypes.c_int32 * 6)(*v)


@pytest.mark.parametrize("kind,blocks", [("stft", (2,)), ("mrstft", (3, 2, 7))])
def test_validation_without_device(lib, kind, blocks):
    """Dummy pointers: every refusal comes before a launch.  n = 5003: 2 / 3 / 2 / 7 frame blocks."""
    fwd, fin, bwd = (getattr(lib, f"siren_{kind}_signal_{f}") for f in ("forward", "finish", "backward"))
    n = 5003
    full = _win(*[v for b in blocks for v in (0, b)])
    ok_f = [1, 1, n, n, 1, 0.2, 1, 1, full, None]
    ok_b = [1, 1, n, n, 1, 0.2, 1, 1, full, 0, n, 1, None]
    for args, fn, ptrs in ((ok_f, fwd, (0, 1, 6, 7, 8)), (ok_b, bwd, (0, 1, 6, 7, 8, 11))):
        for k in ptrs:
            a = list(args)
            a[k] = None
            assert fn(*a) == NULL, (kind, k)
        for mode, alpha in ((3, 0.2), (-1, 0.2), (1, -0.1), (1, 1.5), (1, float("nan"))):
            a = list(args)
            a[4], a[5] = mode, alpha
            assert fn(*a) == CONFIG, (mode, alpha)
        for j, b in enumerate(blocks):          # a window outside [0, blocks], or reversed
            for lo, hi in ((-1, b), (0, b + 1), (2, 1)):
                w = _win(*full)
                w[2 * j], w[2 * j + 1] = lo, hi
                a = list(args)
                a[8] = w
                assert fn(*a) == SHAPE, (j, lo, hi)
        a = list(args)
        a[2] = a[3] = 1024 if kind == "mrstft" else 512     # too short for the transforms
        assert fn(*a) == SHAPE
        a = list(args)
        a[3] = n - 1                                        # rows < n
        assert fn(*a) == SHAPE
    for lo, hi in ((-1, 5), (7, 5), (0, n + 1)):
        a = list(ok_b)
        a[9], a[10] = lo, hi
        assert bwd(*a) == SHAPE, (lo, hi)
    assert fin(n, n, 1, 0.2, None, 1, None) == NULL and fin(n, n, 1, 0.2, 1, None, None) == NULL
    assert fin(n, n, 3, 0.2, 1, 1, None) == CONFIG and fin(n, n, 1, 2.0, 1, 1, None) == CONFIG
    assert fin(n, n - 1, 1, 0.2, 1, 1, None) == SHAPE
    # the window function and the partial locator
    rr = (0,) if kind == "mrstft" else ()
    window, parts = getattr(lib, f"siren_{kind}_window"), getattr(lib, f"siren_{kind}_signal_parts")
    out = (ctypes.c_int32 * 4)()
    assert window(n, *rr, 0, n, None) == NULL
    assert window(n, *rr, 0, n, out) == 0 and list(out) == [0, blocks[0], 0, blocks[0]]
    for lo, hi in ((-1, 5), (7, 5), (0, n + 1)):
        assert window(n, *rr, lo, hi, out) == SHAPE
    assert window(512, *rr, 0, 512, out) == SHAPE
    if kind == "mrstft":
        assert window(n, 3, 0, n, out) == SHAPE and parts(n, n, 3, 0) == -1
    assert parts(n, n, *rr, 6) == -1 and parts(n, n - 1, *rr, 0) == -1
    assert parts(n, n, *rr, 2) == blocks[0] and parts(n, n, *rr, 1) >= blocks[0] * parts(n, n, *rr, 3)
    assert parts(n, n, *rr, 0) % 4 == 0 and parts(n, n, *rr, 4) % 4 == 0


def _covering_blocks(n, lo, hi, n_fft, hop, win):
    """Brute force: the blocks of every frame t < T that covers the padded index of sample i or of one
    of its two reflected images (gather_sample's three), for lo <= i < hi."""
    T, H, pad = 1 + n // hop, n_fft // 2, (n_fft - win) // 2
    blocks = set()
    for i in range(lo, hi):
        js = [i + H]
        if 1 <= i <= H:
            js.append(H - i)
        if n - H - 1 <= i <= n - 2:
            js.append(2 * (n - 1) - i + H)
        for j in js:
            a = j - pad          # frame t holds the padded indices t hop + pad .. t hop + pad + win - 1
            if a < 0:
                continue
            for t in range(max(0, a // hop - win // hop - 1), min(T - 1, a // hop) + 1):
                if t * hop <= a < t * hop + win:
                    blocks.add(t // FT)
    return blocks


def _partitions(n):
    """Two equal parts, three unequal ones (the middle cut at 9000, or 3000 where n is shorter), and a
    1-sample last shard."""
    return ([0, n // 2, n], [0, 700, 9000, n] if n > 9000 else [0, 700, 3000, n], [0, n - 1, n])


@pytest.mark.parametrize("n", [5003, 12301])
@pytest.mark.parametrize("trait", range(4))
def test_window_vs_brute_force(lib, n, trait):
    n_fft, hop, win = TRAITS[trait]
    nblk = -(-(1 + n // hop) // FT)
    out = (ctypes.c_int32 * 4)()

    def window(lo, hi):
        st = lib.siren_stft_window(n, lo, hi, out) if trait == 0 else lib.siren_mrstft_window(n, trait - 1, lo, hi, out)
        assert st == 0
        return tuple(out)

    for cuts in _partitions(n):
        owned = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            c0, c1, o0, o1 = window(lo, hi)
            cover = _covering_blocks(n, lo, hi, n_fft, hop, win)
            assert cover and (c0, c1) == (min(cover), max(cover) + 1), (lo, hi)   # the smallest aligned cover
            assert 0 <= c0 <= o0 <= o1 <= c1 <= nblk, (lo, hi)                    # compute contains owned
            want = [b for b in range(nblk) if lo <= min(b * FT * hop, n - 1) < hi]
            assert list(range(o0, o1)) == want, (lo, hi)
            owned.append((o0, o1))
        assert owned[0][0] == 0 and owned[-1][1] == nblk                           # the owned ranges partition
        assert all(a[1] == b[0] for a, b in zip(owned[:-1], owned[1:]))
    assert window(100, 100)[2:] in [(b, b) for b in range(nblk + 1)] and window(100, 100)[:2] == (0, 0)


def test_engine_refuses_before_it_touches_a_device():
    from inr_for_audio_amd.engine import SirenEngine
    assert inspect.signature(SirenEngine.__init__).parameters["split_spectral"].default is False
    t, y = torch.linspace(-1, 1, 1024).reshape(-1, 1), torch.zeros(1024)
    with pytest.raises(ValueError, match="512"):
        SirenEngine(None, t[:512], y[:512], alpha=0.2, split_spectral=True)
    with pytest.raises(ValueError, match="1024"):
        SirenEngine(None, t, y, loss_mode="mae", alpha=0.2, stft_loss="mrstft", split_spectral=True)
    with pytest.raises(NotImplementedError, match="n_total"):
        SirenEngine(None, t, y, alpha=0.2, n_total=4096, split_spectral=True)


def test_train_switch(tmp_path):
    from inr_for_audio_amd.run import train
    p = inspect.signature(train).parameters["split_spectral"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    with pytest.raises(NotImplementedError, match="restated_losses"):
        train(str(tmp_path), "t", "clip", 1, alpha=0.2, split_spectral=True)
    assert not list(tmp_path.iterdir())
