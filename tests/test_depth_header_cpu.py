"""No-GPU checks of the C ABI of a frame's DEPTH updates in one launch (include/viekf_depth.h): the library exports exactly
what the header declares, the header is plain C11, viekf_depths_lds_bytes agrees with the layout header the kernel and the
launch site read (csrc/viekf_depth_lds.hpp), include/viekf.h and capi.SYMBOLS got nothing new, and the Python classes have
the methods."""
import os
import re
import subprocess

from vi_ekf_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "vi_ekf_amd", "csrc")

LAYOUT_MAIN = r"""
#include <cstdio>
#include "viekf_depth_lds.hpp"
int main() {
  const int sizes[][2] = {{0, 1}, {1, 1}, {5, 3}, {5, 256}, {16, 16}, {17, 70}, {50, 50}, {77, 77}, {78, 78}, {79, 79}, {200, 256}};
  for (const auto& s : sizes) {
    const int N = s[0], M = s[1], nx = 17 + 5 * N, n = 16 + 3 * N;
    const viekf::DepthLds L((nx + 1) & ~1, n, M);
    // every region lies behind the one before it, 16-byte aligned where pairs are read, and inside the total
    const bool ok = L.xs == 0 && L.lam >= L.xs + ((nx + 1) & ~1) && L.D >= L.lam + n && L.bad >= L.D + N && L.Si >= L.bad + 1 &&
                    L.W >= L.Si + M && L.total == L.W + L.nW * M && L.nW >= n && L.nW % 2 == 0 && L.W % 2 == 0 && L.Si % 2 == 0;
    std::printf("%d %d %zu %d\n", N, M, L.bytes(), ok ? 1 : 0);
  }
  std::printf("max %d\n", viekf::kDepthsMaxM);
  return 0;
}
"""


def test_header_and_library_agree():
    txt = open(os.path.join(INC, "viekf_depth.h")).read()
    nocom = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = sorted(set(re.findall(r"\b(viekf_[a-z_0-9]+)\s*\(", nocom)))
    assert sorted(capi.DEPTH_SYMBOLS) == syms and len(syms) == 3
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vi_ekf_amd", "libviekf_hip.so")], capture_output=True, text=True, check=True)
    exported = sorted(ln.split()[-1] for ln in out.stdout.splitlines() if re.search(r"\bviekf_(batch_update_depths|depths_|frame_intake_depth)", ln))
    assert exported == syms, exported                        # exactly the declared ones
    assert int(re.search(r"#define\s+VIEKF_DEPTHS_MAX_M\s+(\d+)", txt).group(1)) == capi.DEPTHS_MAX_M >= 256
    assert L.viekf_abi_version() == 1
    # include/viekf.h itself got no new symbol, and neither did capi.SYMBOLS
    assert "update_depths" not in open(os.path.join(INC, "viekf.h")).read()
    assert not [s for s in capi.SYMBOLS if "depth" in s]
    import vi_ekf_amd
    assert callable(vi_ekf_amd.BatchVIEKF.update_depths) and callable(vi_ekf_amd.FrameIntake.intake_depth)


def test_null_handles_are_refused():
    L = capi.lib()
    assert L.viekf_batch_update_depths(None, 8, 1, None, None, None, 0, None, 0, None, None, 0) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
    assert L.viekf_frame_intake_depth(None, 1, None, None, None, None, 0, 1, None, None, 0) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()


def test_header_is_plain_c11(tmp_path):
    """tests/c/depth_header.c: C11, -Wall -Wextra -Werror -pedantic, links and runs without a GPU"""
    from vi_ekf_amd import _build
    _build.build()
    libdir = os.path.join(ROOT, "vi_ekf_amd")
    exe = os.path.join(str(tmp_path), "depth_header")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", exe,
                           os.path.join(ROOT, "tests", "c", "depth_header.c"), "-L" + libdir, "-lviekf_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "depth header ok" in out.stdout, out.stderr


def test_the_layout_function_agrees_with_the_layout_header(tmp_path):
    """csrc/viekf_depth_lds.hpp is plain C++17 with no HIP header: a host program prints DepthLds' byte counts, and
    viekf_depths_lds_bytes answers the same; the regions do not overlap"""
    src, exe = os.path.join(str(tmp_path), "layout.cpp"), os.path.join(str(tmp_path), "layout")
    with open(src, "w") as fh:
        fh.write(LAYOUT_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    L = capi.lib()
    rows = [ln.split() for ln in out if ln and not ln.startswith("max")]
    assert len(rows) == 11
    for N, M, nbytes, ok in rows:
        assert int(ok) == 1, (N, M)
        assert L.viekf_depths_lds_bytes(int(N), int(M)) == int(nbytes), (N, M)
    assert "max %d" % capi.DEPTHS_MAX_M in out
    assert L.viekf_depths_lds_bytes(50, 0) == 0 and L.viekf_depths_lds_bytes(50, capi.DEPTHS_MAX_M + 1) == 0 and L.viekf_depths_lds_bytes(-1, 1) == 0
    assert L.viekf_depths_lds_bytes(50, 50) == 70688 and 2 * 70688 <= 160 * 1024
    assert L.viekf_depths_lds_bytes(78, 78) <= 160 * 1024 < L.viekf_depths_lds_bytes(79, 79)
