"""The multi-resolution STFT loss kernels (csrc/stft.hip; run.py:127, :160) one entry point at a
time against tests/mrstft_ref.py, the definition written with torch.stft and autograd in fp64.

Inputs (spectral_ref.signals, seed 1): n = 1536 (every frame of the 2048-point resolution touches a
reflected edge), n = 5003 (a multiple of no hop, rows pad to 5120; T = 42 / 21 / 101), n = 8448, and the
clamp case n = 5003 with x[:2048] = 0; and, with seed 2, n = 1025 (the shortest signal the loss takes,
one or two tiles per grid; seed 1 fails the precondition there).  All five pass the clamp-margin
precondition at all three resolutions.  The kernels get the fp32 roundings of x and y, and the fp64 reference is evaluated on
those same fp32 values."""
import numpy as np
import pytest
import torch

import mrstft_ref as mr

pytestmark = pytest.mark.gpu

CASES = {"n1025": (1025, False, 2), "n1536": (1536, False), "n5003": (5003, False), "n8448": (8448, False),
         "clamp": (5003, True)}   # (n, clamp[, seed])
NBP = (528, 1040, 272)            # bins padded to 16, per resolution
CHAIN = (304, 608, 128)           # the longer of the two interleaved fp32 chains: 16 * ceil(ceil(win / 16) / 2)
_REF, _GPU, _BASIS = {}, {}, {}


def rows_of(n):
    return (n + 255) // 256 * 256


def ref(case):
    """Inputs and fp64 / fp32 CPU results of one case: computed once, shared, never modified."""
    if case not in _REF:
        n, clamp, *seed = CASES[case]
        x, y = mr.signals(n, *seed)
        if clamp:
            x[:2048] = 0
        x32, y32 = x.float(), y.float()
        xd, yd = x32.double(), y32.double()
        for res in mr.RES:
            assert mr.clamp_margin_ok(xd, res), f"precondition: no bin of x within [eps/4, 4 eps] of the clamp {res}"
        loss64, g64 = mr.loss_and_grad(mr.mrstft_loss, xd, yd)
        _, g32 = mr.loss_and_grad(mr.mrstft_loss, x32, y32)
        _REF[case] = dict(n=n, x32=x32, y32=y32, X=[mr.stft(xd, res) for res in mr.RES], loss64=float(loss64),
                          terms64=[float(v) for v in mr.terms(xd, yd)], g64=g64, e_torch32=mr.grad_err(g32, g64))
    return _REF[case]


def basis_on(dev):
    if "b" not in _BASIS:
        from inr_for_audio_amd.engine import mrstft_basis
        _BASIS["b"] = mrstft_basis(dev)
    return _BASIS["b"]


def gpu(lib, dev, case):
    """The launches of one case (target side, forward, scalars, backward), once."""
    if case in _GPU:
        return _GPU[case]
    from inr_for_audio_amd._lib import check, ptr
    r = ref(case)
    n, R = r["n"], rows_of(r["n"])
    s = torch.cuda.current_stream(dev).cuda_stream
    basis = basis_on(dev)
    ws = torch.zeros(int(lib.siren_mrstft_workspace_floats(n, R)), dtype=torch.float32, device=dev)
    x, y = r["x32"].to(dev), r["y32"].to(dev)
    loss = torch.zeros(4, device=dev)
    g = torch.full((n,), float("nan"), device=dev)
    check(lib.siren_mrstft_forward(ptr(y), n, R, ptr(basis), ptr(ws), 1, s), "mrstft target")
    check(lib.siren_mrstft_forward(ptr(x), n, R, ptr(basis), ptr(ws), 0, s), "mrstft forward")
    check(lib.siren_mrstft_loss(n, R, ptr(ws), ptr(loss), s), "mrstft loss")
    check(lib.siren_mrstft_loss_bwd(n, R, ptr(basis), ptr(ws), ptr(g), s), "mrstft bwd")
    torch.cuda.synchronize(dev)
    T = [int(lib.siren_mrstft_frames(n, k)) for k in range(3)]
    piece = lambda k, w: ws[lib.siren_mrstft_ws_offset(n, R, k, w):][:T[k] * NBP[k]].view(T[k], NBP[k]).cpu()  # noqa: E731
    _GPU[case] = dict(re=[piece(k, 0) for k in range(3)], im=[piece(k, 1) for k in range(3)], loss=loss.cpu().tolist(),
                      g=g.cpu(), ws=ws, x=x, T=T)
    return _GPU[case]


@pytest.mark.parametrize("case", list(CASES))
def test_forward_re_im_vs_fp64(lib, dev, case):
    """re / im of every frame and bin of every resolution.  Bound, from the arithmetic alone: each
    value is a sum of win products x_k v_k (only the window's support enters) accumulated in fp32 in
    two interleaved chains over the 16-k groups; the longer chain has 304 / 608 / 128 terms, and with
    the table's rounding (1/2 ulp), the product's and the final add's that is at most chain + 4
    roundings on any path: |err| <= (chain + 4) * 2^-24 * sum_k |x_k| |v_k|."""
    r, d = ref(case), gpu(lib, dev, case)
    n = r["n"]
    for k, (n_fft, hop, win) in enumerate(mr.RES):
        T, nb, pad = d["T"][k], n_fft // 2 + 1, (n_fft - win) // 2
        assert T == 1 + n // hop
        xp = torch.nn.functional.pad(r["x32"].double()[None, None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
        frames = xp.unfold(0, n_fft, hop)[:, pad:pad + win]                   # [T][win]: the window's support
        assert frames.shape[0] == T
        w = torch.hann_window(win, periodic=True, dtype=torch.float64)
        kb = torch.arange(pad, pad + win, dtype=torch.float64)[:, None] * torch.arange(nb, dtype=torch.float64)[None, :]
        ang = 2 * np.pi * torch.remainder(kb, n_fft) / n_fft
        ref_err = 2.0 ** -40   # the fp64 FFT's own error, e.g. at the exactly-zero im of the last bin
        bound_c = (CHAIN[k] + 4) * 2.0 ** -24 * (frames.abs() @ (w[:, None] * torch.cos(ang)).abs()) + ref_err
        bound_s = (CHAIN[k] + 4) * 2.0 ** -24 * (frames.abs() @ (w[:, None] * torch.sin(ang)).abs()) + ref_err
        X = r["X"][k].T                                                       # [T][bins]
        e_re = (d["re"][k][:, :nb].double() - X.real).abs()
        e_im = (d["im"][k][:, :nb].double() - X.imag).abs()
        print(f"{case} r{k}: max|re err| {float(e_re.max()):.3e} ({float((e_re / bound_c).max()):.3f} of the bound), "
              f"max|im err| {float(e_im.max()):.3e} ({float((e_im / bound_s).max()):.3f} of the bound)")
        assert bool((e_re <= bound_c).all()) and bool((e_im <= bound_s).all())
        assert not d["re"][k][:, nb:].any() and not d["im"][k][:, nb:].any()   # pad bins: zero table columns


@pytest.mark.parametrize("case", list(CASES))
def test_mrstft_loss_vs_fp64(lib, dev, case):
    r, d = ref(case), gpu(lib, dev, case)
    want, got = [r["loss64"]] + r["terms64"], d["loss"]
    rel = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    print(f"{case}: L_mrstft {got[0]:.7f} vs fp64 {want[0]:.7f}; rel of the mean and the terms "
          + " ".join(f"{v:.2e}" for v in rel))
    assert max(rel) <= 1e-5
    if case == "n5003":
        assert abs(want[0] - 0.8389569) < 1e-6
    if case == "clamp":
        assert abs(want[0] - 4.2340820) < 1e-6


@pytest.mark.parametrize("case", list(CASES))
def test_mrstft_grad_vs_fp64(lib, dev, case):
    """e = max|g - g64| / max|g64| against the same error of torch.stft autograd in fp32 on the CPU:
    e <= 8 e_torch32 (the rule of test_gpu_stft.py: the log term amplifies a small bin's error by
    1 / x_mag, so the achievable error depends on the input)."""
    r, d = ref(case), gpu(lib, dev, case)
    e = mr.grad_err(d["g"], r["g64"])
    print(f"{case}: e {e:.3e}, e_torch32 {r['e_torch32']:.3e}, ratio {e / r['e_torch32']:.2f}")
    assert torch.isfinite(d["g"]).all()
    assert e <= 8 * r["e_torch32"]


def test_clamp_case_gradient_is_exactly_zero_where_fp64_is(lib, dev):
    """x[:2048] = 0: 7695 / 7175 / 10023 bins sit on the clamp; g is 0.0 bit for bit exactly at the 1081
    samples that only silent frames of all three resolutions cover, where the fp64 gradient is exactly
    zero, and non-zero at every other sample."""
    r, d = ref("clamp"), gpu(lib, dev, "clamp")
    clamped = [int(((d["re"][k][:, :nb] ** 2 + d["im"][k][:, :nb] ** 2) <= 1e-8).sum())
               for k, nb in enumerate((513, 1025, 257))]
    assert clamped == [7695, 7175, 10023]
    zero64 = r["g64"] == 0
    assert int(zero64.sum()) == 1081
    assert torch.equal(d["g"].view(torch.int32) == 0, zero64)


def test_two_launches_are_bit_identical(lib, dev):
    from inr_for_audio_amd._lib import check, ptr
    d = gpu(lib, dev, "n5003")
    n, R, s = 5003, 5120, torch.cuda.current_stream(dev).cuda_stream
    basis, loss = basis_on(dev), torch.zeros(4, device=dev)
    g2 = torch.full((n,), float("nan"), device=dev)
    ws = d["ws"]
    off = lambda k, w: lib.siren_mrstft_ws_offset(n, R, k, w)  # noqa: E731
    for k in range(3):
        ws[off(k, 0):off(k, 2)] = float("nan")                                  # re, im
        ws[off(k, 4):(off(k + 1, 0) if k < 2 else off(k, 5))] = float("nan")    # dF and the partials
    check(lib.siren_mrstft_forward(ptr(d["x"]), n, R, ptr(basis), ptr(ws), 0, s), "mrstft forward")
    check(lib.siren_mrstft_loss(n, R, ptr(ws), ptr(loss), s), "mrstft loss")
    check(lib.siren_mrstft_loss_bwd(n, R, ptr(basis), ptr(ws), ptr(g2), s), "mrstft bwd")
    torch.cuda.synchronize(dev)
    assert torch.equal(g2.cpu().view(torch.int32), d["g"].view(torch.int32))
    assert loss.cpu().tolist() == d["loss"]
