"""No-GPU checks of the C ABI of the PIXEL_VEL measurement (include/viekf_pixvel.h): the library exports exactly what the header
declares, the header is plain C11, viekf_pixvel_lds_bytes agrees with the layout header the kernel and the launch site read
(csrc/viekf_pixvel_lds.hpp), include/viekf.h and capi.SYMBOLS got nothing new, and the Python classes have the methods."""
import os
import re
import subprocess

from vi_ekf_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "vi_ekf_amd", "csrc")

def test_header_and_library_agree():
    txt = open(os.path.join(INC, "viekf_pixvel.h")).read()
    nocom = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = sorted(set(re.findall(r"\b(viekf_[a-z_0-9]+)\s*\(", nocom)))
    assert sorted(capi.PIXVEL_SYMBOLS) == syms and len(syms) == 7
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vi_ekf_amd", "libviekf_hip.so")], capture_output=True, text=True, check=True)
    exported = sorted(ln.split()[-1] for ln in out.stdout.splitlines() if re.search(r"\bviekf_\w*(pixel_vel|pixvel|pixel_flow)", ln))
    assert exported == syms, exported                        # exactly the declared ones
    assert int(re.search(r"#define\s+VIEKF_PIXVELS_MAX_M\s+(\d+)", txt).group(1)) == capi.PIXVELS_MAX_M >= 256
    assert L.viekf_abi_version() == 1
    # include/viekf.h itself got no new symbol, and neither did capi.SYMBOLS
    assert "pixel_vels" not in open(os.path.join(INC, "viekf.h")).read()
    assert not [s for s in capi.SYMBOLS if "pix" in s]
    import vi_ekf_amd
    assert callable(vi_ekf_amd.BatchVIEKF.update_pixel_vels) and callable(vi_ekf_amd.BatchVIEKF.eval_pixel_vel)
    assert callable(vi_ekf_amd.FrameIntake.intake_pixel_vel) and callable(vi_ekf_amd.pixel_flow)


def test_null_handles_are_refused():
    L = capi.lib()
    assert L.viekf_batch_update_pixel_vels(None, 1, None, None, None, None, 0, 0.0, None, 0, None, None, 0) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
    assert L.viekf_batch_eval_pixel_vel(None, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_batch_pixel_vels_route(None, 0) == capi.ERR_INVALID
    assert L.viekf_pixel_flow(None, 1, None, None, 1, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_frame_intake_pixel_vel(None, 1, None, None, None, None, None, 0, 0.0, 1, None, None, 0) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()


def test_header_is_plain_c11(tmp_path):
    """tests/c/pixvel_header.c: C11, -Wall -Wextra -Werror -pedantic, links and runs without a GPU"""
    from vi_ekf_amd import _build
    _build.build()
    libdir = os.path.join(ROOT, "vi_ekf_amd")
    exe = os.path.join(str(tmp_path), "pixvel_header")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", exe,
                           os.path.join(ROOT, "tests", "c", "pixvel_header.c"), "-L" + libdir, "-lviekf_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "pixvel header ok" in out.stdout, out.stderr


def test_the_layout_functions_agree_with_the_layout_header(tmp_path):
    """tests/cpp/pixvel_lds_model.cpp: csrc/viekf_pixvel_lds.hpp is plain C++17 with no HIP header; the model program checks both
    layouts (regions disjoint and inside the total, rows on 16-byte boundaries, the stated formulas) over N = 0 .. 300 and
    M = 1 .. 256, and prints byte counts that viekf_pixvel_lds_bytes and viekf_pixvels_lds_bytes answer too"""
    exe = os.path.join(str(tmp_path), "pixvel_lds_model")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pixvel_lds_model.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 failures, max M %d" % capi.PIXVELS_MAX_M in out.stdout, out.stdout
    L = capi.lib()
    for N, M in ((0, 1), (1, 1), (2, 70), (3, 256), (5, 3), (12, 12), (12, 256), (50, 50), (52, 50), (77, 77), (200, 256)):
        one, many = subprocess.run([exe, str(N), str(M)], capture_output=True, text=True, check=True).stdout.split()
        assert L.viekf_pixvel_lds_bytes(N) == int(one) and L.viekf_pixvels_lds_bytes(N, M) == int(many), (N, M)
    assert L.viekf_pixvel_lds_bytes(50) == 9040 and L.viekf_pixvel_lds_bytes(-1) == 0
    assert L.viekf_pixvels_lds_bytes(50, 50) == 150480 <= 160 * 1024 < L.viekf_pixvels_lds_bytes(12, 256)
    assert L.viekf_pixvels_lds_bytes(50, 0) == 0 and L.viekf_pixvels_lds_bytes(50, capi.PIXVELS_MAX_M + 1) == 0 and L.viekf_pixvels_lds_bytes(-1, 1) == 0
