"""The module API outside the fused step, on the unfused fp32 HIP layer kernels (layer_fp32.hip):
a lone SineLayer (models.py:114-120), Snake (models.py:235-241) and
SirenWithSnakeTanh.forward_with_activations (models.py:396-423) -- against the reference's own
forward_with_activations values (tests/golden/fwd_bwd_3x256.npz) and against plain fp32 PyTorch
of the same ops (forward and autograd)."""
import os

import numpy as np
import pytest
import torch

from errlog import log, rel

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_forward_with_activations_matches_reference(dev):
    from inr_for_audio_amd.models import SineLayer, SirenWithSnakeTanh
    fb = np.load(os.path.join(G, "fwd_bwd_3x256.npz"))
    g = np.load(os.path.join(G, "gt_bach_1s.npz"))
    t = torch.from_numpy(g["coords"][fb["subset_idx"]]).reshape(1, -1, 1).to(dev)
    torch.manual_seed(0)
    m = SirenWithSnakeTanh(1, 1, 256, 2, 0, 0, first_omega_0=1000.0, hidden_omega_0=30.0).to(dev)
    acts = m.forward_with_activations(t, retain_grad=True)
    sine = [v for k, v in acts.items() if "SineLayer" in k]
    assert len(sine) == 6 and list(acts)[0] == "input"
    errs = {}
    for j in range(3):
        pre = sine[2 * j].detach().reshape(-1, 256)[:16].cpu().numpy()
        y = sine[2 * j + 1].detach().reshape(-1, 256)[:16].cpu().numpy()
        errs[f"preact{j}"] = rel(pre, fb[f"w1000_preact{j}"])
        errs[f"sin{j}"] = float(np.max(np.abs(y - fb[f"w1000_sin{j}"])))
    log("forward_with_activations", **errs)
    # layer 0 agrees to fp32 rounding; the hidden layers inherit sin(|.| ~ 1e3 rad) of layer 0
    # through 256-term sums (the reference's CPU addmm fuses t*w + b for K = 1, this GEMM rounds twice)
    assert errs["preact0"] < 1e-6 and errs["preact1"] < 1e-4 and errs["preact2"] < 1e-4, errs
    assert all(errs[f"sin{j}"] < 2e-3 for j in range(3)), errs   # sin of |.| <= 2e3 rad in fp32
    out = list(acts.values())[-1]
    assert out.shape == (1, t.shape[1], 1)
    assert rel(out.detach().reshape(-1).cpu().numpy(), fb["w1000_out"]) < 1e-3
    # differentiable like the reference's (retain_grad on every entry)
    out.sum().backward()
    assert sine[1].grad is not None and m.net[0].linear.weight.grad is not None
    assert isinstance(m.net[1], SineLayer)


def test_lone_sine_layer_autograd_vs_torch(dev):
    from inr_for_audio_amd.models import SineLayer
    torch.manual_seed(3)
    layer = SineLayer(64, 128, is_first=False, omega_0=30.0).to(dev)
    x = torch.randn(3000, 64, device=dev, requires_grad=True)
    y, pre = layer.forward_with_intermediate(x)
    gy = torch.randn_like(y)
    (y * gy).sum().backward()
    # plain fp32 PyTorch of the same op
    W = layer.linear.weight.detach().clone().requires_grad_(True)
    b = layer.linear.bias.detach().clone().requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    pr = 30.0 * torch.nn.functional.linear(xr, W, b)
    yr = torch.sin(pr)
    (yr * gy).sum().backward()
    errs = {"y": rel(y.detach().cpu(), yr.detach().cpu().double().numpy()),
            "pre": rel(pre.detach().cpu(), pr.detach().cpu().double().numpy()),
            "gW": rel(layer.linear.weight.grad.cpu(), W.grad.cpu().double().numpy()),
            "gb": rel(layer.linear.bias.grad.cpu(), b.grad.cpu().double().numpy()),
            "gx": rel(x.grad.cpu(), xr.grad.cpu().double().numpy())}
    log("lone_sine_layer", **errs)
    assert all(e < 1e-5 for e in errs.values()), errs
    assert torch.allclose(layer(x), y)
    with pytest.raises(RuntimeError):
        layer.cpu()(torch.zeros(4, 64))


@pytest.mark.parametrize("a0", [0.5, None])
def test_snake_and_tanh_modules_vs_torch(dev, a0):
    from inr_for_audio_amd.models import SirenWithSnakeTanh, Snake
    torch.manual_seed(1)
    sn = Snake(96, a=a0).to(dev)
    x = torch.randn(2000, 96, device=dev, requires_grad=True)
    y = sn(x)
    gy = torch.randn_like(y)
    (y * gy).sum().backward()
    a = sn.a.detach().clone().requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    yr = xr + (1.0 / a) * torch.pow(torch.sin(xr * a), 2)      # models.py:241
    (yr * gy).sum().backward()
    errs = {"y": rel(y.detach().cpu(), yr.detach().cpu().double().numpy()),
            "gx": rel(x.grad.cpu(), xr.grad.cpu().double().numpy()),
            "ga": rel(sn.a.grad.cpu(), a.grad.cpu().double().numpy())}
    log(f"snake_module[{a0}]", **errs)
    assert all(e < 1e-5 for e in errs.values()), errs
    # a Tanh / Snake stack walks through forward_with_activations as the reference does
    torch.manual_seed(2)
    m = SirenWithSnakeTanh(1, 1, 128, 1, 1, 1, first_omega_0=500.0, a_initial=a0 or 2.0).to(dev)
    t = torch.linspace(-1, 1, 1000, device=dev).reshape(1, -1, 1)
    acts = m.forward_with_activations(t)
    h = torch.sin(500.0 * torch.nn.functional.linear(t, m.net[0].linear.weight, m.net[0].linear.bias))
    h = torch.sin(30.0 * torch.nn.functional.linear(h, m.net[1].linear.weight, m.net[1].linear.bias))
    z = torch.nn.functional.linear(h, m.net[2].weight, m.net[2].bias)
    h = z + (1.0 / m.net[3].a) * torch.pow(torch.sin(z * m.net[3].a), 2)
    h = torch.tanh(torch.nn.functional.linear(h, m.net[4].weight, m.net[4].bias))
    o = torch.nn.functional.linear(h, m.net[6].weight, m.net[6].bias)
    vals = list(acts.values())
    assert len(vals) == 1 + 2 * 2 + 5        # input, 2 SineLayers x 2, Linear/Snake/Linear/Tanh/Linear
    assert rel(vals[-1].detach().cpu(), o.detach().cpu().double().numpy()) < 1e-5


@pytest.mark.parametrize("a_shape", [(), (1,)])
def test_snake_scalar_a_broadcasts(dev, a_shape):
    """A scalar Snake `a` (the reference's formula broadcasts it over the columns, models.py:241)
    is applied to every column and gets the column-summed gradient in its own shape; an `a` of
    another length is refused instead of read out of bounds."""
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd.models import fp32_act
    torch.manual_seed(3)
    x = torch.randn(700, 40, device=dev, requires_grad=True)
    a = torch.full(a_shape, 0.7, device=dev, requires_grad=True)
    y = fp32_act(x, _lib.FP32_SNAKE, a)
    gy = torch.randn_like(y)
    (y * gy).sum().backward()
    xr = x.detach().clone().requires_grad_(True)
    ar = a.detach().clone().requires_grad_(True)
    yr = xr + (1.0 / ar) * torch.pow(torch.sin(xr * ar), 2)
    (yr * gy).sum().backward()
    assert a.grad.shape == a.shape
    assert rel(y.detach().cpu(), yr.detach().cpu().double().numpy()) < 1e-5
    assert rel(x.grad.cpu(), xr.grad.cpu().double().numpy()) < 1e-5
    assert rel(a.grad.cpu().reshape(-1), ar.grad.cpu().double().numpy().reshape(-1)) < 1e-5
    with pytest.raises(ValueError):
        fp32_act(x, _lib.FP32_SNAKE, torch.ones(39, device=dev))


# ---- the wrappers against fp64 torch autograd on the CPU, per element ------------------------------
# Gates as in test_gpu_layer_kernels.py: chain * 2^-24 * sum|terms| per element (terms from
# fp32_layer_ref), tanh by the CPU-oracle multiple.
def _wrapped_linear(dev, base, W, b, omega, view=lambda t: t, gy=None, x_grad=True):
    """fp32_linear(view(x), W, b, omega) and its backward on the device against the same graph in
    fp64 on the CPU.  gy None: out.sum().backward(), whose gradient arrives as an expanded
    zero-stride tensor.  Returns the device leaves (x, W, b) with their gradients."""
    import fp32_layer_ref as fr
    from gpu_util import col_reduce_chain
    from inr_for_audio_amd.models import _splits, fp32_linear
    from test_gpu_layer_kernels import _gate
    lin = torch.nn.functional.linear
    xd = base.to(dev).requires_grad_(x_grad)
    Wd = W.to(dev).requires_grad_(True)
    bd = None if b is None else b.to(dev).requires_grad_(True)
    out = fp32_linear(view(xd), Wd, bd, omega)
    (out.sum() if gy is None else (out * gy.to(dev)).sum()).backward()
    xr = base.double().requires_grad_(x_grad)
    Wr = W.double().requires_grad_(True)
    br = None if b is None else b.double().requires_grad_(True)
    ref = omega * lin(view(xr), Wr, br)
    (ref.sum() if gy is None else (ref * gy.double()).sum()).backward()
    assert out.shape == ref.shape
    fin, fout = W.shape[1], W.shape[0]
    x2 = view(base).reshape(-1, fin).numpy()
    rows = x2.shape[0]
    g2 = np.ones((rows, fout), np.float32) if gy is None else gy.reshape(rows, fout).numpy()
    _, t_pre = fr.linear(x2, W.numpy(), None if b is None else b.numpy(), omega)
    t = fr.linear_bwd(x2, W.numpy(), omega, g2)
    kchunk, z = fr.split_k(rows, _splits(rows))
    what = f"[{tuple(view(base).shape)},{fout}]"
    # the chains of test_gpu_layer_kernels.py; gb against fp64 autograd also counts the rounding of gz
    r = {"pre": _gate(out.detach().cpu().numpy().reshape(rows, fout), (ref.detach().numpy().reshape(rows, fout), t_pre),
                      fin + 2, "pre" + what),
         "gW": _gate(Wd.grad.cpu().numpy(), (Wr.grad.numpy(), t["gW"][1]), kchunk + z + 2, "gW" + what)}
    if b is not None:
        r["gb"] = _gate(bd.grad.cpu().numpy(), (br.grad.numpy(), t["gb"][1]), col_reduce_chain(rows) + 1, "gb" + what)
    if x_grad:
        r["gx"] = _gate(view(xd.grad).cpu().numpy().reshape(rows, fin), (view(xr.grad).numpy().reshape(rows, fin),
                                                                        t["gx"][1]), fout + 2, "gx" + what)
        assert torch.equal(xd.grad.cpu() == 0, xr.grad == 0)       # nothing outside the view
    else:
        assert xd.grad is None
    log(f"fp32_linear_wrapper{what}", splits=_splits(rows), **r)
    return xd, Wd, bd


@pytest.mark.parametrize("rows", [4095, 4096])
def test_fp32_linear_wrapper_splits_boundary(dev, rows):
    """_splits(rows) goes 1 -> 2 between 4095 and 4096 rows: the wrapper's own slab sizing."""
    from inr_for_audio_amd.models import _splits
    assert _splits(4095) == 1 and _splits(4096) == 2
    g = torch.Generator().manual_seed(rows)
    _wrapped_linear(dev, torch.randn(rows, 5, generator=g), torch.randn(7, 5, generator=g),
                    torch.randn(7, generator=g), 30.0, gy=torch.randn(rows, 7, generator=g))


@pytest.mark.parametrize("case", ["lead_1_N_in", "no_bias", "strided_view", "sum_backward", "x_without_grad"])
def test_fp32_linear_wrapper_calling_forms(dev, case):
    g = torch.Generator().manual_seed(11)
    W, b = torch.randn(9, 6, generator=g), torch.randn(9, generator=g)
    if case == "lead_1_N_in":
        _wrapped_linear(dev, torch.randn(1, 300, 6, generator=g), W, b, 30.0, gy=torch.randn(1, 300, 9, generator=g))
    elif case == "no_bias":
        _, _, bd = _wrapped_linear(dev, torch.randn(300, 6, generator=g), W, None, 1.0,
                                   gy=torch.randn(300, 9, generator=g))
        assert bd is None
    elif case == "strided_view":     # every other column of a [300][12] tensor: not contiguous
        view = lambda t: t[:, ::2]   # noqa: E731
        assert not view(torch.empty(300, 12)).is_contiguous()
        _wrapped_linear(dev, torch.randn(300, 12, generator=g), W, b, 30.0, view=view,
                        gy=torch.randn(300, 9, generator=g))
    elif case == "sum_backward":
        _wrapped_linear(dev, torch.randn(300, 6, generator=g), W, b, 30.0)
    else:
        _wrapped_linear(dev, torch.randn(300, 6, generator=g), W, b, 30.0, gy=torch.randn(300, 9, generator=g),
                        x_grad=False)


def test_fp32_linear_wrapper_backward_twice(dev):
    """backward(retain_graph=True), then backward again with the same gradient: every .grad doubles
    exactly and the caller's gradient tensor is untouched (the C entry point scales gpre in place;
    the wrapper must hand it a copy)."""
    from inr_for_audio_amd.models import fp32_linear
    torch.manual_seed(12)
    x = torch.randn(300, 6, device=dev, requires_grad=True)
    W = torch.randn(9, 6, device=dev, requires_grad=True)
    b = torch.randn(9, device=dev, requires_grad=True)
    G = torch.randn(300, 9, device=dev)
    G0 = G.clone()
    out = fp32_linear(x, W, b, 30.0)
    out.backward(G, retain_graph=True)
    first = [t.grad.clone() for t in (x, W, b)]
    assert torch.equal(G, G0)
    out.backward(G)
    assert torch.equal(G, G0)
    for t, f in zip((x, W, b), first):
        assert torch.equal(t.grad, 2.0 * f)


def test_fp32_act_tanh_and_identity_autograd(dev):
    from inr_for_audio_amd import _lib
    from inr_for_audio_amd.models import fp32_act
    import fp32_layer_ref as fr
    from test_gpu_layer_kernels import _act_data, _oracle_gate, _torch_cpu
    xn, _, gn = _act_data(fr.TANH, 300, 64)
    got = {}
    for kind in (_lib.FP32_TANH, _lib.FP32_IDENTITY):
        x = torch.from_numpy(xn).to(dev).requires_grad_(True)
        y = fp32_act(x, kind)
        (y * torch.from_numpy(gn).to(dev)).sum().backward()
        got[kind] = (y.detach().cpu().numpy(), x.grad.cpu().numpy())
    y, gx = got[_lib.FP32_IDENTITY]
    assert np.array_equal(y.view(np.uint32), xn.view(np.uint32)) and np.array_equal(gx.view(np.uint32), gn.view(np.uint32))
    # tanh against fp64 autograd of torch.tanh on the CPU, gated like the kernel test
    x64 = torch.from_numpy(xn).double().requires_grad_(True)
    y64 = torch.tanh(x64)
    (y64 * torch.from_numpy(gn).double()).sum().backward()
    cpu_y, cpu_gx, _ = _torch_cpu(fr.TANH, xn, None, gn)
    vals = {}
    _oracle_gate("y", got[_lib.FP32_TANH][0], cpu_y, (y64.detach().numpy(), fr.act(fr.TANH, xn)[1]), vals)
    _oracle_gate("gx", got[_lib.FP32_TANH][1], cpu_gx, (x64.grad.numpy(), fr.act_bwd(fr.TANH, xn, gn)["gx"][1]), vals)
    log("fp32_act_wrapper_tanh", **vals)
