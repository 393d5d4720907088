"""The unfused fp32 layers of csrc/layer_fp32.hip and the strided GEMM they run on (kan_gemm_kernel in
csrc/kan.hip, kan_slab_reduce_kernel in csrc/kan_tiles.h), through their four C entry points -- siren_fp32_linear,
siren_fp32_linear_bwd, siren_fp32_act, siren_fp32_act_bwd -- against tests/fp32_layer_ref.py: fp64,
element by element.  `splits` is the test's choice here, not models._splits(rows).

What each shape reaches ((rows, in, out); forward (sam, sak, sbk, sbn) = (in, 1, 1, in), gW
(1, out, in, 1), gx (out, 1, in, 1), so a_k_fast / b_k_fast follow in == 1 and out == 1):
  (1, 1, 1)          every loader flip at once, M = N = K = 1
  (63, 15, 65), (65, 17, 63)   tile tails (63, 65 of 64) and K tails (15, 17 of 16)
  (64, 16, 64)       exact tiles
  (129, 33, 1)       out = 1: gW's A operand k-fast, gx's K = 1
  (200, 1, 129)      in = 1: gW's and gx's B operand k-fast, the forward's K = 1
  (1100, 1, 5), (1100, 70, 3)   many splits over few columns: kan_slab_reduce_kernel<16> at 70 splits
  (1100, 128, 128)   in * out = 16 384: kan_slab_reduce_kernel<64> at 70 splits (unrolled loop + tail)
  (16 400, 3, 257)   rows * out past lay_grid's 16 384 x 256 = 4 194 304: the second grid pass of
                     bias_omega_kernel and scale_kernel
and (16 400, 257) the second pass of act_kernel / act_bwd_kernel.

Gates (u = 2^-24, the fp32 unit roundoff; the library is built with -ffp-contract=off, so a product
and an add round separately): the linear results within  chain * u * sum|terms| + 1e-30  per element,
`chain` the longest sequence of roundings one term goes through, stated beside each gate; identity
bit for bit; sin / cos within the 5 units of 2^-24 of the device sinf / cosf gate (measured 1.142 /
1.185 on [-40, 40], tests/test_gpu_head.py); tanh, Snake and every derivative in units of
2^-24 * scale (fp32_layer_ref's natural scale) within 4 x the figure that torch's CPU fp32
evaluation of the reference's formula reaches on the same inputs, rounded up to an integer first
(the rule of test_gpu_kan_kernels.py for B').  Every output starts as NaN with 16 NaN floats behind
it, every call runs twice and must repeat bit for bit (fixed summation order, no atomics).
Measured on an MI355X, worst error / gate: pre 0.82, gx 0.60, gW 0.065, gb 0.036, Snake da 0.30;
sinf 1.15 and gy * cosf 1.76 units; at (16 400, 257), CPU oracle / device in units of 2^-24 * scale:
tanh y 1.00 / 2.46, gx 1.49 / 1.88; Snake y 1.86 / 1.86, gx 2.99 / 2.52, gy dy/da 2.50 / 2.46."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import fp32_layer_ref as fr
from errlog import log
from gpu_util import col_reduce_chain, ok, ptr, release, stream as S, to_dev

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
U = fr.U
NAN = float("nan")
PAD = 16
FLOOR = 1e-30          # an all-zero sum has bound 0; nothing here is that small otherwise
EPS_SINCOS = 5.0       # tests/test_gpu_head.py EPS_SIN / EPS_COS: ceil(4 x 1.142), ceil(4 x 1.185)


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _nan(n, dev):
    return torch.full((n + PAD,), NAN, dtype=torch.float32, device=dev)


def _read(t, n, what):
    """The first n floats of a NaN-padded device buffer; nothing may be written behind them."""
    got = t.cpu().numpy()
    assert np.isnan(got[n:]).all(), f"{what}: written past its end"
    return got[:n]


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: two runs on the same inputs differ"


def _gate(got, ref_terms, chain, what):
    """|got - ref| <= chain u sum|terms| + FLOOR for every element (NaN fails); returns the worst
    ratio to the gate."""
    ref, terms = ref_terms
    got = np.asarray(got, F64).reshape(ref.shape)
    lim = chain * U * terms + FLOOR
    err = np.abs(got - ref)
    bad = np.argwhere(~(err <= lim))
    assert bad.size == 0, (what, chain, len(bad), bad[:4].tolist(), got[tuple(bad[:4].T)], ref[tuple(bad[:4].T)])
    return float(np.max(err / lim))


# ------------------------------------------------------------------ linear
SHAPES = [(1, 1, 1), (63, 15, 65), (64, 16, 64), (65, 17, 63), (129, 33, 1), (200, 1, 129), (1100, 1, 5),
          (1100, 70, 3), (1100, 128, 128), (16400, 3, 257)]
GRID_CAP = 16384 * 256     # lay_grid: elements one pass covers


def _bwd_splits(rows):
    """1, 2, 7; one above rows / 16, where kchunk's rounding to 16 leaves z < splits; and at 1100
    rows 70, which gives kchunk 16 and z 69 -- above slab_reduce's 64-slab switch."""
    return list(dict.fromkeys([1, 2, 7, rows // 16 + 3] + ([70] if rows == 1100 else [])))


BWD_CASES = [(r, i, o, s) for r, i, o in SHAPES for s in _bwd_splits(r)]


@functools.lru_cache(maxsize=None)
def _linear_data(rows, fin, fout):
    rng = np.random.default_rng(rows * 1000003 + fin * 1009 + fout)
    x, W = rng.normal(size=(rows, fin)).astype(F32), rng.normal(size=(fout, fin)).astype(F32)
    b, g = rng.normal(size=fout).astype(F32), rng.normal(size=(rows, fout)).astype(F32)
    return x, W, b, g


@functools.lru_cache(maxsize=4)
def _bwd_ref(rows, fin, fout, omega):
    x, W, _, g = _linear_data(rows, fin, fout)
    return fr.linear_bwd(x, W, omega, g)


def test_shapes_reach_what_they_claim():
    assert sum(r * o > GRID_CAP for r, _, o in SHAPES) == 1 and 16400 * 257 > GRID_CAP
    assert fr.split_k(1100, 70) == (16, 69) and fr.split_k(1100, 71) == (16, 69)
    assert 1 * 5 < 16384 and 70 * 3 < 16384 and 128 * 128 >= 16384          # slab_reduce's column switch
    for rows, _, _ in SHAPES:                                                # z < splits: slab room unused
        assert fr.split_k(rows, rows // 16 + 3)[1] < rows // 16 + 3
    assert fr.split_k(16400, 7) == (2352, 7) and fr.split_k(1, 7) == (16, 1)


@pytest.mark.parametrize("rows,fin,fout", SHAPES)
def test_linear_forward_vs_fp64(lib, dev, rows, fin, fout):
    """siren_fp32_linear with omega in {1, 30}, b present and NULL."""
    x, W, b, _ = _linear_data(rows, fin, fout)
    xd, Wd, bd = to_dev(x, dev), to_dev(W, dev), to_dev(b, dev)
    n, worst = rows * fout, 0.0
    for omega in (1.0, 30.0):
        for has_b in (True, False):
            what = f"pre[{rows},{fin},{fout}] omega={omega:g} b={has_b}"
            runs = []
            for _ in range(2):
                pre = _nan(n, dev)
                ok(lib.siren_fp32_linear(ptr(xd), rows, fin, fout, ptr(Wd), ptr(bd if has_b else None),
                                         ctypes.c_float(omega), ptr(pre), S()), lib)
                runs.append(_read(pre, n, what))
            _same(runs[0], runs[1], what)
            # chain in + 2: a term's product, the in - 1 adds behind it (the first add, to 0, is
            # exact), the bias add and the multiplication by omega
            worst = max(worst, _gate(runs[0], fr.linear(x, W, b if has_b else None, omega), fin + 2, what))
    log(f"fp32_linear[{rows},{fin},{fout}]", pre=worst)


def _run_bwd(lib, dev, rows, fin, fout, omega, splits, want_gx, want_gb):
    x, W, _, g = _linear_data(rows, fin, fout)
    gz, gW = to_dev(g, dev).clone(), _nan(fout * fin, dev)
    gx = _nan(rows * fin, dev) if want_gx else None
    gb = _nan(fout, dev) if want_gb else None
    slab = _nan(splits * fout * fin, dev) if splits > 1 else None       # sized for splits, not for z
    tmp = _nan(64 * fout, dev)
    ok(lib.siren_fp32_linear_bwd(ptr(to_dev(x, dev)), rows, fin, fout, ptr(to_dev(W, dev)), ctypes.c_float(omega),
                                 ptr(gz), ptr(gx), ptr(gW), ptr(gb), ptr(slab), splits, ptr(tmp), S()), lib)
    what = f"[{rows},{fin},{fout}] splits={splits} omega={omega:g}"
    out = {"gz": gz.cpu().numpy(), "gW": _read(gW, fout * fin, "gW" + what)}
    if want_gx:
        out["gx"] = _read(gx, rows * fin, "gx" + what)
    if want_gb:
        out["gb"] = _read(gb, fout, "gb" + what)
    _read(tmp, 64 * fout, "tmp" + what)
    if slab is not None:
        _read(slab, splits * fout * fin, "slab" + what)
    return out


def _check_bwd(got, rows, fin, fout, omega, splits):
    x, W, _, g = _linear_data(rows, fin, fout)
    ref = _bwd_ref(rows, fin, fout, omega)
    what = f"[{rows},{fin},{fout}] splits={splits} omega={omega:g}"
    # gpre comes back as fl(omega * gpre): one IEEE multiplication, bit for bit
    gz32 = F32(omega) * g
    assert np.array_equal(_bits(got["gz"]), _bits(gz32)), "gz" + what
    kchunk, z = fr.split_k(rows, splits)
    ratios = {}
    # chain kchunk + z + 2: the rounding of gz, a term's product and the kchunk - 1 adds behind it
    # inside its slab, then at most z adds over the slabs (per-group partial sums, then the groups)
    ratios["gW"] = _gate(got["gW"], ref["gW"], kchunk + z + 2, "gW" + what)
    if "gx" in got:
        # chain out + 2: the rounding of gz, a term's product and the out - 1 adds behind it
        ratios["gx"] = _gate(got["gx"], ref["gx"], fout + 2, "gx" + what)
    if "gb" in got:
        # col_reduce's add chain (one pass up to 256 rows, two above) over the fp32 gz the device
        # holds, which the line above pinned bit for bit: no rounding of gz left to count
        z64 = gz32.astype(F64)
        ratios["gb"] = _gate(got["gb"], (z64.sum(0), np.abs(z64).sum(0)), col_reduce_chain(rows), "gb" + what)
    return ratios


@pytest.mark.parametrize("rows,fin,fout,splits", BWD_CASES)
def test_linear_backward_vs_fp64(lib, dev, rows, fin, fout, splits):
    """siren_fp32_linear_bwd: gW through kan_gemm's split-K (slabs + kan_slab_reduce_kernel when
    z > 1), gb through col_reduce, gx; with omega 30 and everything asked for (twice), omega 1 without
    gx, omega 30 without gb."""
    a = _run_bwd(lib, dev, rows, fin, fout, 30.0, splits, True, True)
    a2 = _run_bwd(lib, dev, rows, fin, fout, 30.0, splits, True, True)
    for k in a:
        _same(a[k], a2[k], f"{k}[{rows},{fin},{fout}] splits={splits}")
    worst = _check_bwd(a, rows, fin, fout, 30.0, splits)
    for omega, want_gx, want_gb in ((1.0, False, True), (30.0, True, False)):
        got = _run_bwd(lib, dev, rows, fin, fout, omega, splits, want_gx, want_gb)
        for k, v in _check_bwd(got, rows, fin, fout, omega, splits).items():
            worst[k] = max(worst[k], v)
    kchunk, z = fr.split_k(rows, splits)
    log(f"fp32_linear_bwd[{rows},{fin},{fout},{splits}]", kchunk=kchunk, z=z, **worst)


# ------------------------------------------------------------------ activations
ACT_SHAPES = [(1, 1), (5, 63), (257, 65), (300, 64), (16400, 257)]
KINDS = [fr.IDENTITY, fr.SIN, fr.TANH, fr.SNAKE]
KIND_NAME = {fr.IDENTITY: "identity", fr.SIN: "sin", fr.TANH: "tanh", fr.SNAKE: "snake"}
EDGE = np.array([0.0, -0.0, 20.0, -20.0, 25.5, -31.0, 39.9, -39.9, 9.5, -9.5], F32)


@functools.lru_cache(maxsize=2)
def _act_data(kind, rows, cols):
    """(x, a, gy): sine arguments in [-40, 40] (where the device sinf / cosf were measured) -- half
    uniform over the range, half N(0, 1.5) for the part where tanh is not saturated -- with +-0 and
    |x| >= 20 in the first row when there is room.  Snake: a per column, signs alternating, |a|
    log-uniform over [0.05, 50] with both ends present, and x = argument / a."""
    rng = np.random.default_rng(7919 * kind + 31 * rows + cols)
    n = rows * cols
    arg = np.where(rng.random(n) < 0.5, rng.uniform(-39.9, 39.9, n), rng.normal(0.0, 1.5, n)).astype(F32)
    if n >= 16:
        arg[:EDGE.size] = EDGE
    arg = arg.reshape(rows, cols)
    gy = rng.normal(size=(rows, cols)).astype(F32)
    if kind != fr.SNAKE:
        return arg, None, gy
    mag = np.exp(rng.uniform(np.log(0.05), np.log(50.0), cols))
    if cols >= 2:
        mag[0], mag[-1] = 0.05, 50.0
    a = (np.where(np.arange(cols) % 2 == 0, 1.0, -1.0) * mag).astype(F32)
    x = (arg.astype(F64) / a.astype(F64)[None]).astype(F32)
    assert np.abs(x.astype(F64) * a.astype(F64)[None]).max() <= 40.0
    return x, a, gy


def _torch_cpu(kind, x, a, gy):
    """torch's CPU fp32 evaluation of the reference's formula (torch.sin, torch.tanh, Snake as
    models.py:241 writes it) and its autograd: (y, gx, per-element gy dy/da or None).  `a` enters as a
    full [rows][cols] leaf, so its gradient is the per-element product da sums over the rows."""
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    at = None
    if kind == fr.SIN:
        y = torch.sin(xt)
    elif kind == fr.TANH:
        y = torch.tanh(xt)
    else:
        at = torch.from_numpy(np.broadcast_to(a[None], x.shape).copy()).requires_grad_(True)
        y = xt + (1.0 / at) * torch.pow(torch.sin(xt * at), 2)
    y.backward(torch.from_numpy(gy.copy()))
    return y.detach().numpy(), xt.grad.numpy(), None if at is None else at.grad.numpy()


def _oracle_gate(what, got, cpu, ref_scale, out):
    """got within 4 x ceil(CPU oracle's figure) units of 2^-24 * scale, exact where the scale is 0.
    The CPU figure is taken on the same inputs against the same fp64 reference; one that comes out
    below one unit (a one-element case can be exact) counts as one unit, a single rounding."""
    ref, scale = ref_scale
    cpu_u, _ = fr.units(cpu, ref, scale)
    dev_u, exact = fr.units(got, ref, scale)
    gate = 4 * max(1, math.ceil(cpu_u))
    out.update({what + "_cpu": cpu_u, what + "_dev": dev_u, what + "_gate": gate})
    print(f"{what}: CPU fp32 {cpu_u:.3f}, device {dev_u:.3f} units of 2^-24 scale (gate {gate})")
    assert exact, what
    assert dev_u <= gate, (what, dev_u, cpu_u, gate)


def _act_fwd(lib, dev, kind, x, a):
    rows, cols = x.shape
    y = _nan(rows * cols, dev)
    ok(lib.siren_fp32_act(kind, ptr(to_dev(x, dev)), rows, cols, ptr(None if a is None else to_dev(a, dev)), ptr(y),
                          S()), lib)
    return _read(y, rows * cols, "y").reshape(rows, cols)


@pytest.mark.parametrize("rows,cols", ACT_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_act_forward_vs_fp64(lib, dev, kind, rows, cols):
    x, a, gy = _act_data(kind, rows, cols)
    y = _act_fwd(lib, dev, kind, x, a)
    _same(y, _act_fwd(lib, dev, kind, x, a), "y")
    ref = fr.act(kind, x, a)
    vals = {}
    if kind == fr.IDENTITY:
        assert np.array_equal(_bits(y), _bits(x))                          # a copy, -0 included
    elif kind == fr.SIN:
        vals["y_dev"], _ = fr.units(y, *ref)
        vals["y_cpu"], _ = fr.units(_torch_cpu(kind, x, a, gy)[0], *ref)
        assert vals["y_dev"] <= EPS_SINCOS, vals                           # sinf: 5 units of 2^-24
    else:
        _oracle_gate("y", y, _torch_cpu(kind, x, a, gy)[0], ref, vals)
    if kind == fr.TANH:
        big = np.abs(x) >= 20.0
        assert big.any() or x.size < 16
        assert np.array_equal(y[big], np.sign(x[big]))                     # saturated: exactly +-1
    if kind == fr.SNAKE:
        assert ((x == 0).any() or x.size < 16) and np.all(y[x == 0] == 0)
    log(f"fp32_act[{KIND_NAME[kind]},{rows},{cols}]", **vals)


def _act_bwd(lib, dev, kind, x, a, gy, want_da):
    rows, cols = x.shape
    n = rows * cols
    snake = kind == fr.SNAKE
    gx = _nan(n, dev)
    da = _nan(cols, dev) if snake and want_da else None
    prod = _nan(n, dev) if snake else None
    tmp = _nan(64 * cols, dev) if snake else None
    ok(lib.siren_fp32_act_bwd(kind, ptr(to_dev(x, dev)), rows, cols, ptr(None if a is None else to_dev(a, dev)),
                              ptr(to_dev(gy, dev)), ptr(gx), ptr(da), ptr(prod), ptr(tmp), S()), lib)
    out = {"gx": _read(gx, n, "gx").reshape(rows, cols)}
    if snake:
        out["da_prod"] = _read(prod, n, "da_prod").reshape(rows, cols)
        _read(tmp, 64 * cols, "tmp")
    if da is not None:
        out["da"] = _read(da, cols, "da")
    return out


@pytest.mark.parametrize("rows,cols", ACT_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_act_backward_vs_fp64(lib, dev, kind, rows, cols):
    """siren_fp32_act_bwd; Snake with da (col_reduce in one pass up to 256 rows, in two above) and
    with da = NULL, where da_prod must stay unwritten."""
    x, a, gy = _act_data(kind, rows, cols)
    got = _act_bwd(lib, dev, kind, x, a, gy, True)
    again = _act_bwd(lib, dev, kind, x, a, gy, True)
    for k in got:
        _same(got[k], again[k], k)
    ref = fr.act_bwd(kind, x, gy, a)
    vals = {}
    if kind == fr.IDENTITY:
        assert np.array_equal(_bits(got["gx"]), _bits(gy))
    elif kind == fr.SIN:
        r, s = ref["gx"]                                                    # s = |gy|
        vals["gx_dev"], _ = fr.units(got["gx"], r, s)
        vals["gx_cpu"], _ = fr.units(_torch_cpu(kind, x, a, gy)[1], r, s)
        # gy * cosf(x): 5 units of 2^-24 for cosf and one rounding of the product (|cos| <= 1)
        assert vals["gx_dev"] <= EPS_SINCOS + 1.0, vals
    else:
        _, cpu_gx, cpu_da = _torch_cpu(kind, x, a, gy)
        _oracle_gate("gx", got["gx"], cpu_gx, ref["gx"], vals)
    if kind == fr.TANH:
        sat = np.abs(_act_fwd(lib, dev, kind, x, None)) == 1.0             # where the device's tanhf is +-1
        assert sat.any() or x.size < 16
        assert np.all(got["gx"][sat] == 0)                                  # 1 - t t is exactly 0 there
    if kind == fr.SNAKE:
        assert np.array_equal(_bits(got["gx"][x == 0]), _bits(gy[x == 0]))  # gy (1 + 2 * 0 * 1)
        _oracle_gate("da_prod", got["da_prod"], cpu_da, ref["da_prod"], vals)
        # da: col_reduce's add chain over the device's own da_prod
        p64 = got["da_prod"].astype(F64)
        vals["da"] = _gate(got["da"], (p64.sum(0), np.abs(p64).sum(0)), col_reduce_chain(rows), "da")
        none = _act_bwd(lib, dev, kind, x, a, gy, False)
        assert np.array_equal(_bits(none["gx"]), _bits(got["gx"]))
        assert np.isnan(none["da_prod"]).all()                              # no da: no products written
    log(f"fp32_act_bwd[{KIND_NAME[kind]},{rows},{cols}]", **vals)


def test_act_rows_zero(lib, dev):
    """What the code does today, pinned as it is: siren_fp32_act accepts rows = 0 and writes nothing,
    siren_fp32_act_bwd refuses it (SIREN_ERR_SHAPE, tests/test_capi.py)."""
    x, y = to_dev(np.ones(4, F32), dev), _nan(4, dev)
    ok(lib.siren_fp32_act(fr.SIN, ptr(x), 0, 4, None, ptr(y), S()), lib)
    assert torch.isnan(y).all()
    assert lib.siren_fp32_act_bwd(fr.SIN, ptr(x), 0, 4, None, ptr(x), ptr(y), None, None, None, S()) == 1001
    assert torch.isnan(y).all()
