"""The memory-bound kernels of csrc/elementwise.hip past their first grid pass and at ragged sizes.

Every grid here is capped (grid_for), so production sizes loop: Adam at 4096 x 256 = 2^20 elements a
pass, the coordinate fills at 2^21 rows, the first layer at 4096 x (2048 / H) rows with the next row's
coordinates loaded one pass ahead.  Each test sizes its input just past one pass, pre-fills every
output with NaN and compares the whole buffer.  References: torch.optim.Adam(fused=True) on the CPU
(adam_ref.py), oracle.linspace_f32 / torch.linspace + meshgrid, the fp32 first-layer restatement
with fp64 sin / cos, int64 and fp64 column sums, torch's ReduceLROnPlateau."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adam_ref
from inr_for_audio_amd._lib import SirenOptState
from inr_for_audio_amd.engine import _opt_state_tensor
from oracle import siren_oracle as orc
from gpu_util import col_reduce_chain as _chain, ok, ptr, release, stream as S, to_dev, within_f16

pytestmark = pytest.mark.gpu

F32 = np.float32
H16 = torch.float16
NAN = float("nan")


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------ Adam
@functools.lru_cache(maxsize=None)
def _adam_reference(n):
    p0, gs = adam_ref.adam_case(n)
    return p0, gs, adam_ref.torch_fused_adam(p0, gs)


@pytest.mark.parametrize("n", [adam_ref.N_BIG, 0, 1, 255, 257])
def test_adam_second_pass_vs_torch_fused(lib, dev, n):
    """Five siren_adam_step calls (lr = 1e-3 x step) against torch.optim.Adam(fused=True) on the CPU:
    p, exp_avg and exp_avg_sq bit for bit, at n past the grid cap (every block loops; the edge lattice
    sits in the first and in the second pass) and at the smallest sizes.  16 NaN floats follow each
    vector: nothing is written past n."""
    pad = 16
    p0, gs, ref = _adam_reference(n)
    dv = lambda a: torch.from_numpy(np.concatenate([a, np.full(pad, np.nan, F32)])).to(dev)  # noqa: E731
    pd, md, vd = dv(p0), dv(np.zeros(n, F32)), dv(np.zeros(n, F32))
    for step, g in enumerate(gs, 1):
        st = _opt_state_tensor(adam_ref.lr_at(step), 1e-6, 0.8, 200, dev)
        st_host = SirenOptState.from_buffer_copy(bytes(st.cpu().numpy().tobytes()))
        st_host.step = float(step - 1)
        st = torch.frombuffer(bytearray(bytes(st_host)), dtype=torch.uint8).to(dev)
        ok(lib.siren_adam_step(ptr(pd), ptr(dv(g)), ptr(md), ptr(vd), n, ptr(st), S()), lib)
        for name, got, want in zip("pmv", (pd, md, vd), ref[step - 1]):
            got = got.cpu().numpy()
            bad = np.flatnonzero(_u32(got[:n]) != _u32(want))
            assert bad.size == 0, (step, name, bad[:8], got[bad[:8]], want[bad[:8]])
            assert np.isnan(got[n:]).all(), (step, name)
    if n >= 32:
        v = vd.cpu().numpy()[:n]
        assert np.isinf(v).sum() == 4            # 3e20: v = +inf by step 4, so the update there is 0
        assert np.array_equal(_u32(pd.cpu().numpy()[:n][np.isinf(v)]), _u32(ref[3][0][np.isinf(v)]))


# ------------------------------------------------------------------ coordinate fills
ROWS2 = (1 << 21) + 777      # one grid pass covers 8192 x 256 = 2^21 rows


@pytest.mark.parametrize("n,offset", [(ROWS2, 0), (3 * (1 << 20) + 11, (1 << 20) - 5)])
def test_coords_fill_second_pass(lib, dev, n, offset):
    t = torch.full((ROWS2 + 8,), NAN, device=dev)
    ok(lib.siren_coords_fill(ptr(t), ROWS2, offset, n, S()), lib)
    got = t.cpu().numpy()
    valid = min(ROWS2, n - offset)
    want = np.concatenate([orc.linspace_f32(n)[offset:offset + valid], np.zeros(ROWS2 - valid, F32)])
    assert np.array_equal(_u32(got[:ROWS2]), _u32(want))       # pad rows are exact (+0) zeros
    assert np.isnan(got[ROWS2:]).all()
    assert (n - offset < ROWS2) == (offset > 0)                 # the second case has pad rows


@pytest.mark.parametrize("width", [1, 2, 3])
def test_coords_fill_grid_second_pass(lib, dev, width):
    offset = 1000003                                            # no multiple of 2 or 3
    height = (offset + ROWS2 - 300) // width
    n = height * width
    xy = torch.full((ROWS2 + 4, 2), NAN, device=dev)
    ok(lib.siren_coords_fill_grid(ptr(xy), ROWS2, offset, height, width, S()), lib)
    got = xy.cpu()
    t = torch.linspace(-1, 1, steps=height)
    ch = torch.linspace(0, 0, steps=1) if width == 1 else torch.linspace(-1, 1, steps=width)
    hg, wg = torch.meshgrid(t, ch, indexing="ij")
    grid = torch.stack((hg, wg), dim=-1).reshape(n, 2)
    want = torch.zeros(ROWS2, 2)
    want[:n - offset] = grid[offset:]
    assert 0 < ROWS2 - (n - offset) < 400
    assert torch.equal(got[:ROWS2].view(torch.int32), want.view(torch.int32))
    assert torch.isnan(got[ROWS2:]).all()


# ------------------------------------------------------------------ first layer
def _f16_gate(got, ref):
    """test_first_fwd's gate: within one fp16 rounding of the fp64 sin / cos of the fp32
    pre-activation, and more than 0.995 of the elements exactly the rounded reference."""
    worst = within_f16(got, ref, abs_slack=1e-6)
    exact = float(np.mean(got == orc.f16_round(ref)))
    return worst, exact


@pytest.mark.parametrize("in_dim", [1, 2])
@pytest.mark.parametrize("H,R", [(256, 32768 + 13), (1024, 8192 + 3), (2048, 4096 + 1), (4096, 8192 + 3)])
def test_first_fwd_second_pass(lib, dev, H, R, in_dim):
    """Rows past one grid pass of 4096 x (2048 / window) rows: the row loop prefetches the next pass's
    coordinates under `m + stride < R`, and the widths above 2048 run as 1024-column windows at row
    stride H.  The gate holds for the whole buffer, for the rows of the second pass and for the last
    row on their own."""
    omega0 = 22000.0
    win = H if H <= 2048 else 1024
    pass_rows = 4096 * (2048 // win)
    assert pass_rows < R < 2 * pass_rows
    rng = np.random.default_rng(100 + H + in_dim)
    t = rng.uniform(-1, 1, (R, in_dim)).astype(F32)
    W0 = rng.uniform(-1, 1, (H, in_dim)).astype(F32)
    b0 = rng.uniform(-1, 1, H).astype(F32)
    Y0 = torch.full((R + 1, H), NAN, dtype=H16, device=dev)
    C0 = torch.full((R + 1, H), NAN, dtype=H16, device=dev)
    ok(lib.siren_first_fwd(ptr(to_dev(t, dev)), in_dim, ptr(to_dev(W0, dev)), ptr(to_dev(b0, dev)),
                           ctypes.c_float(omega0), R, H, ptr(Y0), ptr(C0), S()), lib)
    a0 = orc.first_preact(t, W0, b0, omega0)
    for name, buf, fn in (("Y0", Y0, orc.sin32), ("C0", C0, orc.cos32)):
        got = buf.float().cpu().numpy()
        assert np.isnan(got[R]).all(), name                    # nothing past row R
        got, ref = got[:R], fn(a0)
        for part, sl in (("all", slice(None)), ("pass2", slice(pass_rows, R)), ("last", slice(R - 1, R))):
            worst, exact = _f16_gate(got[sl], ref[sl])
            print(f"first_fwd H={H} in={in_dim} {name} {part}: worst {worst:.3e} exact {exact:.5f}")
            assert worst <= 0, (name, part, worst)
            assert exact > 0.995, (name, part, exact)


# ------------------------------------------------------------------ column reduction
NROWS = [1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 258, 4097, 8199]
NCOLS = [1, 63, 64, 65, 259]
U = 2.0 ** -24


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("data", ["int", "normal"])
def test_col_reduce_shapes(lib, dev, data, accumulate):
    """Every nrows x ncols of the lists above (the 256 / 257 switch between one and two passes, tails
    of the 8-deep unrolled row loop, column counts off a multiple of 64), row_stride 3 ncols + 1 with
    NaN in the columns that are not part of the reduction, out_stride 1 and 3 alternating.
    int: integer-valued floats in [-8, 8] -- every fp32 partial sum is exact in any order, so the
    result equals the int64 sum; a dropped or doubled row shows outright.  normal: per element within
    d 2^-24 sum|terms|, d = _chain(nrows)."""
    rng = np.random.default_rng(8 + accumulate)
    pre = 0.5 if accumulate else NAN
    for i, nrows in enumerate(NROWS):
        for j, ncols in enumerate(NCOLS):
            out_stride = 3 if (i + j) % 2 else 1
            rs = 3 * ncols + 1
            part = np.full((nrows, rs), np.nan, F32)
            if data == "int":
                part[:, :ncols] = rng.integers(-8, 9, (nrows, ncols)).astype(F32)
            else:
                part[:, :ncols] = rng.normal(size=(nrows, ncols)).astype(F32)
            n_out = ncols * out_stride + 5
            written = np.zeros(n_out, bool)
            written[np.arange(ncols) * out_stride] = True
            out0 = np.full(n_out, np.nan, F32)
            out0[written] = pre
            out = torch.from_numpy(out0.copy()).to(dev)
            tmp = torch.full((64, ncols), NAN, device=dev)
            ok(lib.siren_col_reduce(ptr(to_dev(part, dev)), rs, nrows, ncols, ptr(out), out_stride, accumulate,
                                    ptr(tmp), S()), lib)
            got = out.cpu().numpy()
            where = (data, accumulate, nrows, ncols, out_stride)
            assert np.isnan(got[~written]).all(), where         # between the strides and past the end
            terms = part[:, :ncols].astype(np.float64)
            if data == "int":
                want = terms.astype(np.int64).sum(0) + (0.5 if accumulate else 0.0)
                assert np.array_equal(got[written].astype(np.float64), want), where
            else:
                want = terms.sum(0) + (0.5 if accumulate else 0.0)
                bound = _chain(nrows) * U * (np.abs(terms).sum(0) + (0.5 if accumulate else 0.0))
                err = np.abs(got[written].astype(np.float64) - want)
                assert not np.isnan(got[written]).any() and np.all(err <= bound), (where, float((err / bound).max()))
        release()


# ------------------------------------------------------------------ plateau scheduler
def _torch_plateau(lr, min_lr, factor, patience):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr)
    return opt, torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=factor, patience=patience,
                                                           min_lr=min_lr)


def _run_plateau(lib, dev, trace, lr0, min_lr, factor, patience):
    """Steps siren_plateau_step and torch's scheduler through `trace` side by side, asserting lr,
    num_bad and best after every step; returns the per-step (lr, num_bad) of the device."""
    opt, sch = _torch_plateau(lr0, min_lr, factor, patience)
    state = _opt_state_tensor(lr0, min_lr, factor, patience, dev)
    cap = len(trace)
    lh = torch.full((cap + 2,), NAN, device=dev)
    rh = torch.full((cap + 2,), NAN, dtype=torch.float64, device=dev)
    sse = torch.zeros(2, device=dev)
    seen = []
    for k, v in enumerate(trace):
        sse[0] = float(v)
        ok(lib.siren_plateau_step(ptr(state), ptr(sse), ctypes.c_double(1.0), ptr(lh), ptr(rh), cap, S()), lib)
        sch.step(float(v))
        st = SirenOptState.from_buffer_copy(bytes(state.cpu().numpy().tobytes()))
        assert st.lr == opt.param_groups[0]["lr"], (k, st.lr, opt.param_groups[0]["lr"])
        assert st.num_bad == sch.num_bad_epochs, (k, st.num_bad, sch.num_bad_epochs)
        assert st.best == sch.best, (k, st.best, sch.best)
        assert st.last_epoch == k + 1 and st.step == k + 1
        seen.append((st.lr, st.num_bad))
    assert np.array_equal(lh.cpu().numpy()[:cap], np.asarray(trace, F32), equal_nan=True)
    assert np.array_equal(rh.cpu().numpy()[:cap], np.array([s[0] for s in seen]))
    assert torch.isnan(lh[cap:]).all() and torch.isnan(rh[cap:]).all()
    return seen


def test_plateau_positive_trace_matches_torch(lib, dev):
    rng = np.random.default_rng(3)
    trace = [1.0]
    for _ in range(79):   # improvements, gains inside the relative threshold, plateaus, set-backs
        f = rng.choice([0.9, 1.0, 1.0 - 5e-5, 1.0 - 9.9e-5, 1.2, 0.999])
        trace.append(trace[-1] * f)
    trace = np.asarray(trace, F32)
    seen = _run_plateau(lib, dev, trace, 1e-3, 3e-4, 0.8, 2)
    lrs = [s[0] for s in seen]
    assert len(set(lrs)) >= 4 and lrs[-1] == 3e-4               # reductions happened, down to min_lr


def test_plateau_eps_gate_refuses_the_reduction(lib, dev):
    """lr 1e-3 and min_lr 1e-3 - 5e-9: the reduction would move lr by less than eps = 1e-8, so it is
    refused (lr stays 1e-3) and num_bad resets."""
    lr0 = 1e-3
    seen = _run_plateau(lib, dev, np.full(7, 0.5, F32), lr0, lr0 - 5e-9, 0.8, 1)
    assert [s[0] for s in seen] == [lr0] * 7
    assert [s[1] for s in seen] == [0, 1, 0, 1, 0, 1, 0]


def test_plateau_nan_loss_is_a_bad_epoch(lib, dev):
    trace = np.array([1.0, 0.9, np.nan, np.nan, np.nan, 0.8, np.nan], F32)
    seen = _run_plateau(lib, dev, trace, 1e-3, 1e-6, 0.8, 1)
    assert [s[1] for s in seen] == [0, 0, 1, 0, 1, 0, 1]
    assert seen[2][0] == 1e-3 and seen[3][0] == 1e-3 * 0.8 and seen[-1][0] == 1e-3 * 0.8
