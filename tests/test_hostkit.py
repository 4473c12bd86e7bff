"""The host kit of the five handles (vi_ekf_amd/csrc/viekf_hostkit.hpp: DevOwner, copy_user, check_where) is host code only:
tests/cpp/hostkit_model.cpp drives it against a malloc-backed stub of the HIP header (tests/cpp/hipstub) -- a failing hipMalloc
at every position of a set-up, more buffers than the old fixed tables held, count 0, the order of reserve's calls, the copy
kinds.  Built stand-alone with g++ under AddressSanitizer + UndefinedBehaviorSanitizer; leaks are counted by the stub's own
outstanding-allocation count (nothing is preloaded, no Python is involved, no GPU)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hostkit_model_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "hostkit_model")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "hipstub"), "-I", os.path.join(ROOT, "vi_ekf_amd", "csrc"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "hostkit_model.cpp")]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "hostkit model: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "hipstub:" not in r.stderr
    m = re.search(r"checks (\d+) failed (\d+) outstanding (\d+)", r.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) == 0 and int(m.group(3)) == 0


def test_the_kit_header_is_host_only():
    """no device code in the kit (it is compiled above by a compiler that knows none), and the copies it replaced are gone"""
    csrc = os.path.join(ROOT, "vi_ekf_amd", "csrc")
    kit = open(os.path.join(csrc, "viekf_hostkit.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in kit.splitlines())
    for word in ("__device__", "__global__", "hipLaunchKernelGGL", "<<<"):
        assert word not in code, word
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", kit)
    assert [i for i in includes if "/" in i or i.endswith(".hpp")] == ["hip/hip_runtime.h", "../../include/viekf.h", "viekf_host.hpp"]
    srcs = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hpp", ".hip", ".cpp"))}
    assert sum(s.count("where must be VIEKF_HOST") for s in srcs.values()) == 1
    assert sum(len(re.findall(r"#\s*define\s+HIP_TRY\b", s)) for s in srcs.values()) == 1
    assert "bufs[" not in srcs["viekf_sim.hip"] and "bufs[" not in srcs["viekf_klt.hip"]
