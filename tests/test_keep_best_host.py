"""keep_best=True's host side (run.py:171-174 as the reference meant it): the C entry point's declaration,
binding and argument table, the ABI number that must not move, the engines' keyword and what train()
still refuses before it writes a file.  No GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "siren_hip.h")
OK, SHAPE, NULL, CONFIG = 0, 1001, 1002, 1003


def test_entry_point_declared_and_bound(lib):
    from inr_for_audio_amd import _lib
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^int siren_best_keep\(", src, flags=re.M)
    assert "siren_best_keep" in _lib._SIGS and hasattr(lib, "siren_best_keep")
    res, args = _lib._SIGS["siren_best_keep"]
    assert res is ctypes.c_int and len(args) == 9 and args[2] is ctypes.c_int64 and args[5] is ctypes.c_double
    # the declaration cites the reference lines it implements
    assert re.search(r"/\* run\.py:171-174(?:(?!\*/).)*\*/\s*int siren_best_keep\(", text, flags=re.S)


def test_abi_and_structs_did_not_move(lib):
    """The state is a plain int32[4]: no struct was added, so the ABI number and the struct table stay."""
    from inr_for_audio_amd import _lib
    assert _lib.ABI_VERSION == 12 and lib.siren_abi_version() == 12
    assert "#define SIREN_ABI_VERSION 12" in open(HEADER).read()
    assert len(_lib.STRUCTS) == 10 and lib.siren_struct_size(10) == -1


def test_validation_without_device(lib):
    """Every refusal comes before any launch (there is no device here): addresses are only compared."""
    def K(params=256, best_params=4096, n=1024, state=64, sse=128, n_total=1.0, guard=None, best=512):
        return lib.siren_best_keep(params, best_params, n, state, sse, n_total, guard, best, None)
    for name in ("params", "best_params", "state", "sse", "best"):
        assert K(**{name: None}) == NULL, name
    for n in (0, 3, -4, 6, 1022, 1025):
        assert K(n=n) == SHAPE, n
    assert K(params=260) == SHAPE and K(best_params=4100) == SHAPE and K(best_params=4104) == SHAPE
    for n_total in (0.0, -1.0, float("nan")):
        assert K(n_total=n_total) == CONFIG, n_total
    assert K(best_params=256) == CONFIG            # the live vector is never the destination
    assert K(params=None, n=3) == NULL             # NULL is reported first
    assert K(n=3, n_total=0.0) == SHAPE            # then the shape


def test_engines_expose_the_keyword():
    from inr_for_audio_amd.engine import FitEngine, KanEngine, SirenEngine
    for eng in (SirenEngine, KanEngine):
        p = inspect.signature(eng.__init__).parameters["keep_best"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("best_info", "best_state_dict", "load_best"):
        assert callable(getattr(FitEngine, name))
        assert name not in SirenEngine.__dict__ and name not in KanEngine.__dict__   # built once, in the base
    assert FitEngine.keep_best is False and FitEngine.best_params is None


def test_train_keyword_and_refusals_before_any_file(tmp_path):
    from inr_for_audio_amd.run import train
    p = inspect.signature(train).parameters["keep_best"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    missing = str(tmp_path / "none.wav")
    with pytest.raises(TypeError, match="keep_best"):
        train(str(tmp_path), "t", "missing", 1, keep_best=1, filename=missing)
    # what train() refused without the keyword it refuses with it, and still before the experiment folder
    with pytest.raises(NotImplementedError, match="kan"):
        train(str(tmp_path), "t", "missing", 1, arch="kan", visualization=True, keep_best=True, filename=missing)
    with pytest.raises(NotImplementedError, match="restated_losses"):
        train(str(tmp_path), "t", "missing", 1, alpha=0.2, keep_best=True, filename=missing)
    with pytest.raises(NotImplementedError, match="split_spectral"):
        train(str(tmp_path), "t", "missing", 1, arch="kan", loss_mode="snr", restated_losses=True, keep_best=True,
              filename=missing)
    with pytest.raises(ValueError, match="wave or mdct"):
        train(str(tmp_path), "t", "missing", 1, method="fft", keep_best=True, filename=missing)
    with pytest.raises(ValueError, match="kan_grid_size"):
        train(str(tmp_path), "t", "missing", 1, kan_grid_size=7, keep_best=True, filename=missing)
    assert os.listdir(tmp_path) == []
