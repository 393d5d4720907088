"""The tuning knobs' Python side (_lib.Opt / OPT_DEFAULTS / set_option / options) and the
measurement variants' patches (tools/variants.py).  Host only: siren_set_option and siren_nt_tile
touch no device."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "siren_hip.h")


def test_opt_mirrors_the_header_enum():
    from inr_for_audio_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"enum siren_option\s*\{(.*?)\}", src, flags=re.S).group(1)
    header = {name: int(value) for name, value in re.findall(r"SIREN_OPT_(\w+)\s*=\s*(-?\d+)", body)}
    assert header and header == {o.name: o.value for o in _lib.Opt}


def test_defaults_cover_every_option():
    from inr_for_audio_amd import _lib
    assert set(_lib.OPT_DEFAULTS) == set(_lib.Opt)


def _tile(lib):
    """256 at the defaults, 128 with Opt.NT_TILE = 128."""
    return lib.siren_nt_tile(1 << 20, 1024)


def test_options_nest_and_restore(lib):
    from inr_for_audio_amd._lib import Opt, options
    assert _tile(lib) == 256
    with options(lib, {Opt.NT_TILE: 128}):
        assert _tile(lib) == 128
        with options(lib, {Opt.NT_TILE: 256}):
            assert _tile(lib) == 256
        assert _tile(lib) == 128
    assert _tile(lib) == 256
    # the shape above reads 256 at the default (0 = automatic) as well as at a forced 256; this
    # one has too few tiles for the automatic choice, so it tells the two apart
    with options(lib, {Opt.NT_TILE: 256}):
        assert lib.siren_nt_tile(1024, 1024) == 256
    assert lib.siren_nt_tile(1024, 1024) == 128


def test_options_restore_after_an_exception(lib):
    from inr_for_audio_amd._lib import Opt, options
    with pytest.raises(KeyError):
        with options(lib, {Opt.NT_TILE: 128}):
            try:
                with options(lib, {Opt.NT_TILE: 256}):
                    assert _tile(lib) == 256
                    raise KeyError("inner")
            finally:
                assert _tile(lib) == 128
            raise AssertionError("not reached")
    assert _tile(lib) == 256
    assert lib.siren_nt_tile(1024, 1024) == 128  # the default again, not a forced 256


def test_options_undo_a_partly_rejected_call(lib):
    from inr_for_audio_amd._lib import Opt, SirenError, options
    with pytest.raises(SirenError):
        with options(lib, {Opt.NT_TILE: 128, Opt.NT_PIPE: 3}):
            raise AssertionError("not reached")
    assert _tile(lib) == 256


def test_bound_handles_have_their_own_shadow(lib):
    """A handle from bind() starts at the defaults whatever another handle's shadow holds."""
    import __graft_entry__ as ge
    from inr_for_audio_amd import _lib
    diag = _lib.bind(ge.DIAG_LIB)
    with _lib.options(lib, {_lib.Opt.NT_GRID: 7}):
        assert _lib._opt_shadow(lib)[_lib.Opt.NT_GRID] == 7
        assert _lib._opt_shadow(diag)[_lib.Opt.NT_GRID] == 0
        assert _tile(diag) == 256
        with _lib.options(diag, {_lib.Opt.NT_TILE: 128}):
            assert _tile(diag) == 128 and _tile(lib) == 256
    assert _lib._opt_shadow(lib) == _lib.OPT_DEFAULTS == _lib._opt_shadow(diag)


def test_variants_apply():
    """Every measurement variant's textual patches still find their targets in csrc, and every
    compile-time knob a variant defines is still an #ifndef there (nothing is compiled)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import variants
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    assert variants.VARIANTS and variants.check() == []
