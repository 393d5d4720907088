"""Host-side checks of the random-Fourier-feature encoding (run.py:141-144): the C-ABI additions,
their validation before any launch, the GaussianEncoding module's draw and train()'s refusals.
No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "siren_hip.h")
RFF_SYMBOLS = {"siren_rff_kpad", "siren_rff_slab_floats", "siren_rff_encode", "siren_rff_first_fwd",
               "siren_rff_first_bwd"}


def _header():
    return open(HEADER).read()


def test_header_declares_rff_entry_points(lib):
    """Declared in the header with a comment citing run.py:141-144, bound in _lib._SIGS, exported."""
    from inr_for_audio_amd import _lib
    src = _header()
    for name in RFF_SYMBOLS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|int32_t|int64_t)\s+" + name + r"\s*\(", src, flags=re.S)
        assert m, f"{name}: no declaration with a header comment"
        assert name in _lib._SIGS and hasattr(lib, name), name
    block = src[src.index("Gaussian random-Fourier-feature encoding"):src.index("int siren_rff_first_bwd")]
    assert block.count("run.py:141-144") >= 4
    assert re.search(r"#define SIREN_ABI_VERSION 12\b", src)
    # additive: the new fields close their structs
    assert re.search(r"int32_t rff_freq, pad3;\s*const float\* rff_B;\s*} siren_net;", src)
    assert re.search(r"uint16_t\* enc;\s*float\* rff_slab;\s*} siren_batch;", src)


def test_struct_sizes_and_field_order(lib):
    from inr_for_audio_amd import _lib
    assert lib.siren_abi_version() == 12
    for k, st in enumerate(_lib.STRUCTS):
        assert lib.siren_struct_size(k) == ctypes.sizeof(st), st.__name__
    assert [f[0] for f in _lib.SirenNet._fields_][-3:] == ["rff_freq", "pad3", "rff_B"]
    assert [f[0] for f in _lib.SirenBatch._fields_][-2:] == ["enc", "rff_slab"]
    assert [s.__name__ for s in _lib.STRUCTS][:3] == ["SirenNet", "SirenGrads", "SirenBatch"]


def _net(in_dim=1, hidden=256, rff_freq=0, rff_B=1):
    """A siren_net whose pointers are all the dummy address 1: validation returns before any launch."""
    from inr_for_audio_amd._lib import SirenNet
    n = SirenNet()
    n.in_dim, n.hidden, n.n_inner = in_dim, hidden, 2
    n.omega0, n.omega = 30.0, 30.0
    n.W0 = n.b0 = n.w_head = n.b_head = 1
    for i in range(2):
        n.b[i] = n.Wh[i] = n.WTh[i] = 1
    n.rff_freq, n.rff_B = rff_freq, rff_B
    return n


def test_net_validation_without_device(lib):
    from inr_for_audio_amd._lib import SirenBatch, SirenGrads
    fwd = lambda n: lib.siren_forward(ctypes.byref(n), ctypes.byref(SirenBatch()), None)  # noqa: E731
    assert fwd(_net(rff_freq=64)) == 1001                 # the net passes; the empty batch is a shape error
    assert fwd(_net(in_dim=2, rff_freq=64)) == 1003       # the encoding needs in_dim == 1
    assert fwd(_net(rff_freq=257)) == 1003
    assert fwd(_net(rff_freq=-1)) == 1003
    assert fwd(_net(rff_freq=64, rff_B=None)) == 1002
    assert fwd(_net(in_dim=3)) == 1003                    # unchanged
    assert fwd(_net(in_dim=3, rff_freq=8)) == 1003
    n = _net(rff_freq=8)
    for fn in (lib.siren_train_step, lib.siren_backward):
        assert fn(ctypes.byref(_net(in_dim=2, rff_freq=8)), ctypes.byref(SirenGrads()), ctypes.byref(SirenBatch()),
                  None) == 1003
        assert fn(ctypes.byref(n), ctypes.byref(SirenGrads()), ctypes.byref(SirenBatch()), None) == 1001
    assert lib.siren_first_fwd(1, 3, 1, 1, ctypes.c_float(1.0), 128, 256, 1, 1, None) == 1003   # unchanged


def test_train_batch_needs_the_encoded_layers_buffers(lib):
    """siren_train_step with rff_freq > 0 refuses a batch without enc / rff_slab (no launch)."""
    from inr_for_audio_amd._lib import MAX_INNER, SirenBatch, SirenGrads
    b = SirenBatch()
    b.rows, b.n_valid, b.n_total, b.splits = 256, 256, 256.0, 1
    for name, _ in SirenBatch._fields_:
        if name in ("coords", "target", "out", "g", "head_part", "sse_part", "gsum_part", "gmax_part", "gscale",
                    "col_part", "col_part2", "red_tmp", "slab"):
            setattr(b, name, 1)
    for i in range(MAX_INNER + 1):
        b.Y[i] = b.C[i] = 1
    b.dZ[0] = b.dZ[1] = 1
    assert lib.siren_train_step(ctypes.byref(_net(rff_freq=8)), ctypes.byref(SirenGrads()), ctypes.byref(b),
                                None) == 1002
    b.enc = 1
    assert lib.siren_train_step(ctypes.byref(_net(rff_freq=8)), ctypes.byref(SirenGrads()), ctypes.byref(b),
                                None) == 1002   # still no rff_slab (and, after it, no gradient pointers)


def test_entry_point_validation_without_device(lib):
    f = ctypes.c_float
    enc = lambda F, rows=10, x=1, B=1, out=1: lib.siren_rff_encode(x, B, F, rows, out, None)  # noqa: E731
    assert enc(0) == 1003 and enc(257) == 1003
    assert enc(8, x=None) == 1002 and enc(8, B=None) == 1002 and enc(8, out=None) == 1002
    assert enc(8, rows=-1) == 1001
    fwd = lambda F, rows=128, H=256, B=1, a=None, E0=None: lib.siren_rff_first_fwd(  # noqa: E731
        1, B, F, 1, 1, f(30), a, rows, H, 1, 1, E0, None, None)
    assert fwd(0) == 1003 and fwd(300) == 1003
    assert fwd(8, B=None) == 1002
    assert fwd(8, a=1) == 1002                            # a Snake first layer needs its E0
    assert fwd(8, rows=100) == 1001 and fwd(8, H=384) == 1001
    bwd = lambda F, rows=128, H=256, B=1, E0=None, ga0=None, enc_=1: lib.siren_rff_first_bwd(  # noqa: E731
        1, 1, 1, E0, 1, B, F, f(30), rows, H, None, 1, enc_, 1, 1, 1, 1, 1, ga0, None)
    assert bwd(0) == 1003 and bwd(257) == 1003
    assert bwd(8, B=None) == 1002 and bwd(8, enc_=None) == 1002
    assert bwd(8, E0=1) == 1002                           # a Snake first layer needs ga0
    assert bwd(8, rows=130) == 1001 and bwd(8, H=200) == 1001


def test_sizing_helpers(lib):
    """enc is padded to the 128-column tile of the weight-gradient GEMM; the encoded layer has its own
    slab, so the shared workspace keeps its in_dim = 1 sizes."""
    assert [lib.siren_rff_kpad(F) for F in (1, 5, 24, 64, 65, 256)] == [128, 128, 128, 128, 256, 512]
    assert lib.siren_rff_kpad(0) == 0 and lib.siren_rff_kpad(257) == 0
    assert lib.siren_rff_slab_floats(1024, 256, 0) == 0 and lib.siren_rff_slab_floats(1000, 256, 8) == 0
    for rows, H, F in ((1024, 256, 64), (256, 128, 256), (441088, 256, 256)):
        n = lib.siren_rff_slab_floats(rows, H, F)
        KP = lib.siren_rff_kpad(F)
        assert n >= 2 * H * KP + H and (n - H) % (H * KP) == 0
        assert (n - H) // (H * KP) - 1 <= max(1, rows // 512)       # slices of >= 8 K-steps of 64 rows


def test_gaussian_encoding_draw_matches_reference_formula():
    """b = torch.randn(encoded_size, input_size) * sigma under the same seed; not trainable."""
    from inr_for_audio_amd import GaussianEncoding
    torch.manual_seed(123)
    enc = GaussianEncoding(10.0, 1, 24)
    torch.manual_seed(123)
    ref = torch.randn(24, 1) * 10.0
    assert torch.equal(enc.b.detach(), ref) and enc.b.shape == (24, 1)
    assert not enc.b.requires_grad and enc.encoded_size == 24
    assert list(enc.state_dict()) == ["b"]
    again = GaussianEncoding(b=ref)
    assert torch.equal(again.b.detach(), ref)
    with pytest.raises(NotImplementedError):
        GaussianEncoding(10.0, 2, 24)                      # input_size must be 1
    with pytest.raises(NotImplementedError):
        GaussianEncoding(10.0, 1, 257)
    with pytest.raises(ValueError):
        GaussianEncoding(10.0, 1)
    with pytest.raises(RuntimeError):
        enc(torch.zeros(4, 1))                             # CPU tensors: no fallback


def test_hip_spec_with_encoding():
    from inr_for_audio_amd import GaussianEncoding
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    m = SirenWithSnakeTanh(48, 1, 200, 1, 1, 0, first_omega_0=300.0, a_initial=0.5)
    with pytest.raises(NotImplementedError):
        m.hip_spec()                                       # without an encoding: in_features in {1, 2}
    spec = m.hip_spec(GaussianEncoding(10.0, 1, 24))
    assert (spec.in_dim, spec.rff_freq, spec.hidden) == (1, 24, 256)
    with pytest.raises(ValueError):
        m.hip_spec(GaussianEncoding(10.0, 1, 16))          # in_features != 2 * encoded_size
    assert m.hip_padding()[m.param_index()["W0"]] == ((256, 48), 0.0)
    assert SirenWithSnakeTanh(1, 1, 256, 2, 0, 0).hip_spec().rff_freq == 0


@pytest.mark.parametrize("kw", [{"method": "mdct"}, {"arch": "kan"}, {"multichannel": True, "num_channels": 2}])
def test_train_refuses_num_freq_where_the_reference_cannot_run(tmp_path, kw):
    from inr_for_audio_amd.run import train
    with pytest.raises(NotImplementedError):
        train(str(tmp_path), "t", "x", 1, num_freq=8, filename=str(tmp_path / "none.wav"), **kw)
    assert not os.listdir(tmp_path)                        # refused before anything is written
