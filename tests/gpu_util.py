"""Helpers shared by the GPU test modules that call the C-ABI directly (a plain module like
errlog.py: no fixtures, nothing collected)."""
import contextlib
import math

import numpy as np
import torch

from inr_for_audio_amd import _lib

F32 = np.float32
_KEEP = []


def ptr(t):
    return 0 if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(status, lib):
    assert status == 0, lib.siren_status_string(status)


def to_dev(a, dev, dtype=torch.float32):
    """Host array -> device tensor.  Kept alive (module list) so a pointer taken from a
    temporary inside one call can never be recycled by the caching allocator."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dev).to(dtype)
    _KEEP.append(t)
    return t


def release():
    """Drop to_dev's tensors once the device is idle (the modules' autouse fixtures call this
    after each test)."""
    torch.cuda.synchronize()
    _KEEP.clear()


def within_f16(got, ref, abs_slack=1e-5):
    """|got - ref| <= 2^-11 * |ref| + abs_slack elementwise (one fp16 rounding + slack;
    2^-25 covers the subnormal spacing)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    bound = np.abs(np.asarray(ref, np.float64)) * 2.0 ** -11 + abs_slack + 2.0 ** -25
    return float(np.max(err - bound))


def rel(a, b):
    """Relative L2 error of tensor a against b."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def rel_np(a, b):
    """Relative L2 error of array a against the fp64 array b."""
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def col_reduce_chain(nrows):
    """Longest fp32 add chain of col_reduce's documented order: rows r0 + rg, r0 + rg + 4, ... per
    thread, then the four row groups, then the accumulate; two passes above 256 rows (64 row chunks,
    then the 64 chunk sums)."""
    if nrows <= 256:
        return math.ceil(nrows / 4) + 3
    return math.ceil(math.ceil(nrows / 64) / 4) + 3 + 19


def grads(eng, lib):
    """One siren_train_step per micro-batch (no update); (grads, out, g, per-kind launches)."""
    _lib.check(lib.siren_profile_enable(64 * eng.n_micro), "profile_enable")
    eng._launch_grads()
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.check(lib.siren_profile_enable(0), "profile_disable")
    return eng.grads.clone(), eng.ws.out.clone(), eng.ws.g.clone(), {k: n for k, (_, n) in prof.items()}


@contextlib.contextmanager
def option_setter(lib):
    """Yields set_(Opt.X, v) for tests that change knobs part-way: each value holds until the
    block ends, then every knob goes back to what it was (_lib.options)."""
    with contextlib.ExitStack() as stack:
        yield lambda opt, value: stack.enter_context(_lib.options(lib, {opt: value}))
