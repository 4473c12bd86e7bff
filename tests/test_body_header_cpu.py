"""No-GPU checks of the fused body-sensor update's C ABI (include/viekf_body.h): the library exports exactly what the header
declares, the header is plain C11, include/viekf.h and capi.SYMBOLS got nothing new, and BatchVIEKF has the method."""
import os
import re
import subprocess

from vi_ekf_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "viekf_body.h")).read()
    nocom = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = sorted(set(re.findall(r"\b(viekf_[a-z_0-9]+)\s*\(", nocom)))
    assert sorted(capi.BODY_SYMBOLS) == syms and len(syms) == 3
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vi_ekf_amd", "libviekf_hip.so")], capture_output=True, text=True, check=True)
    exported = sorted(ln.split()[-1] for ln in out.stdout.splitlines() if re.search(r"\bviekf_(batch_update_body|body_)", ln))
    assert exported == syms, exported                        # exactly the declared ones
    assert int(re.search(r"#define\s+VIEKF_BODY_MAX_M\s+(\d+)", txt).group(1)) == capi.BODY_MAX_M == 8
    assert L.viekf_abi_version() == 1
    # include/viekf.h itself got no new symbol, and neither did capi.SYMBOLS
    assert "update_body" not in open(os.path.join(ROOT, "include", "viekf.h")).read()
    assert not [s for s in capi.SYMBOLS if "body" in s]
    import vi_ekf_amd
    assert callable(vi_ekf_amd.BatchVIEKF.update_body)


def test_header_is_plain_c11(tmp_path):
    """tests/c/body_header.c: C11, -Wall -Wextra -Werror -pedantic, links and runs without a GPU"""
    from vi_ekf_amd import _build
    _build.build()
    libdir = os.path.join(ROOT, "vi_ekf_amd")
    exe = os.path.join(str(tmp_path), "body_header")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "body_header.c"), "-L" + libdir, "-lviekf_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "body header ok" in out.stdout, out.stderr
