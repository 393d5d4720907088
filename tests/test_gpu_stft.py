"""The STFT / SNR loss kernels (csrc/stft.hip; run.py:126-128, :160-169) one entry point at a time
against tests/spectral_ref.py, the definition written with torch.stft and autograd in fp64.

Inputs (spectral_ref.signals, seed 1): n = 513 (the shortest signal the transform takes: T = 3, one
tile in every grid, every frame mostly reflection), n = 1536 (T = 7, every frame touches a reflected edge),
n = 5000 (not a multiple of the hop, rows pad to 5120, T = 20 = one 16-frame tile plus a remainder),
n = 8448 (T = 34), and the clamp case n = 5000 with x[:2048] = 0 (seven silent frames).  The kernels
get the fp32 roundings of x and y, and the fp64 reference is evaluated on those same fp32 values."""
import numpy as np
import pytest
import torch

import spectral_ref as sr

pytestmark = pytest.mark.gpu

CASES = {"n513": (513, False), "n1536": (1536, False), "n5000": (5000, False), "n8448": (8448, False), "clamp": (5000, True)}
_REF, _GPU, _BASIS = {}, {}, {}


def rows_of(n):
    return (n + 255) // 256 * 256


def ref(case):
    """Inputs and fp64 / fp32 CPU results of one case: computed once, shared, never modified."""
    if case not in _REF:
        n, clamp = CASES[case]
        x, y = sr.signals(n)
        if clamp:
            x[:2048] = 0
        x32, y32 = x.float(), y.float()
        xd, yd = x32.double(), y32.double()
        assert sr.clamp_margin_ok(xd), "precondition: no bin of x within [eps/4, 4 eps] of the clamp"
        loss64, g64 = sr.loss_and_grad(sr.stft_loss, xd, yd)
        _, g32 = sr.loss_and_grad(sr.stft_loss, x32, y32)
        _REF[case] = dict(n=n, x32=x32, y32=y32, X=sr.stft(xd), loss64=float(loss64), g64=g64,
                          e_torch32=sr.grad_err(g32, g64))
    return _REF[case]


def basis_on(dev):
    if "b" not in _BASIS:
        from inr_for_audio_amd.engine import stft_basis
        _BASIS["b"] = stft_basis(dev)
    return _BASIS["b"]


def gpu(lib, dev, case):
    """The four launches of one case (target side, forward, scalars, backward), once."""
    if case in _GPU:
        return _GPU[case]
    from inr_for_audio_amd._lib import check, ptr
    r = ref(case)
    n, R = r["n"], rows_of(r["n"])
    s = torch.cuda.current_stream(dev).cuda_stream
    basis = basis_on(dev)
    ws = torch.zeros(int(lib.siren_stft_workspace_floats(n, R)), dtype=torch.float32, device=dev)
    x, y = r["x32"].to(dev), r["y32"].to(dev)
    loss = torch.zeros(1, device=dev)
    g = torch.full((n,), float("nan"), device=dev)
    check(lib.siren_stft_forward(ptr(y), n, R, ptr(basis), ptr(ws), 1, s), "stft target")
    check(lib.siren_stft_forward(ptr(x), n, R, ptr(basis), ptr(ws), 0, s), "stft forward")
    check(lib.siren_stft_loss(n, R, ptr(ws), ptr(loss), s), "stft loss")
    check(lib.siren_stft_loss_bwd(n, R, ptr(basis), ptr(ws), ptr(g), s), "stft bwd")
    torch.cuda.synchronize(dev)
    T = int(lib.siren_stft_frames(n))
    piece = lambda k, w: ws[lib.siren_stft_ws_offset(n, R, k):][:T * w].view(T, w).cpu()  # noqa: E731
    _GPU[case] = dict(re=piece(0, 528), im=piece(1, 528), loss=float(loss.item()), g=g.cpu(), ws=ws, x=x, T=T)
    return _GPU[case]


@pytest.mark.parametrize("case", list(CASES))
def test_forward_re_im_vs_fp64(lib, dev, case):
    """re / im of every frame and bin.  Bound, from the arithmetic alone: each value is a sum of 1024
    products x_k v_k accumulated in fp32 in two 512-term chains; with the table's rounding (1/2 ulp),
    the product's and the final add's that is at most 516 roundings on any path, so
    |err| <= 516 * 2^-24 * sum_k |x_k| |v_k| (the fp64 side's own error is 2^-29 smaller)."""
    r, d = ref(case), gpu(lib, dev, case)
    n, T = r["n"], d["T"]
    assert T == 1 + n // 256
    xp = torch.nn.functional.pad(r["x32"].double()[None, None], (512, 512), mode="reflect")[0, 0]
    frames = xp.unfold(0, 1024, 256)                                     # [T][1024]
    assert frames.shape[0] == T
    w = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    k = torch.arange(1024, dtype=torch.float64)[:, None] * torch.arange(513, dtype=torch.float64)[None, :]
    ang = 2 * np.pi * torch.remainder(k, 1024) / 1024
    ref_err = 2.0 ** -40   # the fp64 FFT's own error (~2^-52 x sum|x_k| <= 2^-43), e.g. at the exactly-zero im of bin 512
    bound_c = 516 * 2.0 ** -24 * (frames.abs() @ (w[:, None] * torch.cos(ang)).abs()) + ref_err
    bound_s = 516 * 2.0 ** -24 * (frames.abs() @ (w[:, None] * torch.sin(ang)).abs()) + ref_err
    X = r["X"].T                                                         # [T][513]
    e_re = (d["re"][:, :513].double() - X.real).abs()
    e_im = (d["im"][:, :513].double() - X.imag).abs()
    print(f"{case}: max|re err| {float(e_re.max()):.3e} ({float((e_re / bound_c).max()):.3f} of the bound), "
          f"max|im err| {float(e_im.max()):.3e} ({float((e_im / bound_s).max()):.3f} of the bound)")
    assert bool((e_re <= bound_c).all()) and bool((e_im <= bound_s).all())
    assert not d["re"][:, 513:].any() and not d["im"][:, 513:].any()   # pad bins: zero table columns


@pytest.mark.parametrize("case", list(CASES))
def test_stft_loss_vs_fp64(lib, dev, case):
    r, d = ref(case), gpu(lib, dev, case)
    rel = abs(d["loss"] - r["loss64"]) / abs(r["loss64"])
    print(f"{case}: L_stft {d['loss']:.7f} vs fp64 {r['loss64']:.7f}, rel {rel:.2e}")
    assert rel <= 1e-5
    if case == "clamp":
        assert abs(r["loss64"] - 4.24) < 0.01


@pytest.mark.parametrize("case", list(CASES))
def test_stft_grad_vs_fp64(lib, dev, case):
    """e = max|g - g64| / max|g64| against the same error of torch.stft autograd in fp32 on the CPU:
    e <= 8 e_torch32 (the log term amplifies a small bin's error by 1 / x_mag, so the achievable
    error depends on the input; the factor covers fp32 fma chains against BLAS's blocked sums)."""
    r, d = ref(case), gpu(lib, dev, case)
    e = sr.grad_err(d["g"], r["g64"])
    print(f"{case}: e {e:.3e}, e_torch32 {r['e_torch32']:.3e}, ratio {e / r['e_torch32']:.2f}")
    assert torch.isfinite(d["g"]).all()
    assert e <= 8 * r["e_torch32"]


def test_clamp_case_silent_frames_have_exactly_zero_gradient(lib, dev):
    """x[:2048] = 0: frames 0..6 are exactly zero, their 3591 bins sit on the clamp, and g_stft[:1024],
    which depends on frames 0..5 only, is 0.0 bit for bit."""
    r, d = ref("clamp"), gpu(lib, dev, "clamp")
    p = d["re"][:, :513] ** 2 + d["im"][:, :513] ** 2
    assert int((p <= 1e-8).sum()) == 3591 and not p[:7].any()
    assert not d["g"][:1024].view(torch.int32).any()
    assert not r["g64"][:1024].any() and bool(d["g"][1024:].any())


def test_two_launches_are_bit_identical(lib, dev):
    from inr_for_audio_amd._lib import check, ptr
    d = gpu(lib, dev, "n5000")
    n, R, s = 5000, 5120, torch.cuda.current_stream(dev).cuda_stream
    basis, loss = basis_on(dev), torch.zeros(1, device=dev)
    g2 = torch.full((n,), float("nan"), device=dev)
    ws = d["ws"]
    ws[lib.siren_stft_ws_offset(n, R, 0):lib.siren_stft_ws_offset(n, R, 2)] = float("nan")   # re, im
    ws[lib.siren_stft_ws_offset(n, R, 4):lib.siren_stft_ws_offset(n, R, 5)] = float("nan")   # dF and the partials
    check(lib.siren_stft_forward(ptr(d["x"]), n, R, ptr(basis), ptr(ws), 0, s), "stft forward")
    check(lib.siren_stft_loss(n, R, ptr(ws), ptr(loss), s), "stft loss")
    check(lib.siren_stft_loss_bwd(n, R, ptr(basis), ptr(ws), ptr(g2), s), "stft bwd")
    torch.cuda.synchronize(dev)
    assert torch.equal(g2.cpu().view(torch.int32), d["g"].view(torch.int32))
    assert float(loss.item()) == d["loss"]


@pytest.mark.parametrize("dc", [0.0, 0.3])
def test_snr_loss_and_grad_vs_fp64(lib, dev, dc):
    """SNRLoss at n = 5000, and with a 0.3 DC offset on x (the mean removal): loss and gradient within
    1e-5 relative of fp64 (the gradient in max|.| relative to max|g64|)."""
    from inr_for_audio_amd._lib import check, ptr
    n, R = 5000, 5120
    x, y = sr.signals(n)
    x32, y32 = (x + dc).float(), y.float()
    l64, g64 = sr.loss_and_grad(sr.snr_loss, x32.double(), y32.double())
    s = torch.cuda.current_stream(dev).cuda_stream
    ws = torch.zeros(int(lib.siren_stft_workspace_floats(n, R)), dtype=torch.float32, device=dev)
    loss, g = torch.zeros(1, device=dev), torch.full((n,), float("nan"), device=dev)
    xd, yd = x32.to(dev), y32.to(dev)
    check(lib.siren_snr_loss(ptr(xd), ptr(yd), n, R, ptr(ws), ptr(loss), ptr(g), s), "snr")
    torch.cuda.synchronize(dev)
    rel, e = abs(float(loss.item()) - float(l64)) / abs(float(l64)), sr.grad_err(g.cpu(), g64)
    print(f"dc {dc}: L_snr {float(loss.item()):.6f} vs {float(l64):.6f} (rel {rel:.2e}), grad err {e:.2e}")
    assert float(l64) < 0
    assert rel <= 1e-5 and e <= 1e-5
