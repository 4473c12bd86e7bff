"""No-GPU checks of the consistency diagnostics' C ABI (include/viekf_diag.h): the library exports every symbol the header
declares, a NULL handle is refused, and include/viekf.h is left declaring exactly capi.SYMBOLS."""
import os
import re

from vi_ekf_amd import capi, diag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(viekf_[a-z_0-9]+)\s*\(", txt)))


def test_diag_header_and_library_agree():
    syms = _declared("viekf_diag.h")
    assert syms == sorted(diag.DIAG_SYMBOLS) and len(syms) == 2
    assert all(s.startswith("viekf_diag_") for s in syms)
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    m = re.search(r"#define\s+VIEKF_DIAG_ONCHIP_MAX_FEATURES\s+(\d+)", open(os.path.join(ROOT, "include", "viekf_diag.h")).read())
    assert m and int(m.group(1)) == diag.ONCHIP_MAX_FEATURES


def test_diag_null_handle_is_invalid():
    L = diag._bind()
    assert L.viekf_diag_consistency(None, None, None, None, None, None, capi.HOST) == capi.ERR_INVALID
    assert b"null batch handle" in L.viekf_last_error()
    assert L.viekf_diag_innovation(None, 6, 1, None, 2, None, None, 2, 0, None, None, None, capi.HOST) == capi.ERR_INVALID


def test_main_header_is_unchanged_by_the_diagnostics():
    syms = _declared("viekf.h")
    assert syms == sorted(capi.SYMBOLS)
    assert not [s for s in syms if s.startswith("viekf_diag_")]
    assert capi.lib().viekf_abi_version() == 1


def test_package_exports():
    import vi_ekf_amd as v
    assert v.consistency is diag.consistency and v.innovation is diag.innovation
