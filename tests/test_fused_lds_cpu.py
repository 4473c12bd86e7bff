"""The fused step's LDS is stated once (vi_ekf_amd/csrc/viekf_fused_lds.hpp): the carve-ups ResLds and TileLds (the kernel takes its
pointers from the struct, the launch its byte count), the word map of the scratchpad S.sm through which the waves of a workgroup
talk to each other, and the launch word.  tests/cpp/fused_lds_model.cpp checks the carve-ups for every N (regions inside the total
and on 16-byte boundaries, regions of one life disjoint, the two lives of the shared region, img_len, every dispatch row within its
max_lds_kb, totals equal to the ones recorded from the structs before they moved: tests/golden/fused_lds_totals.txt), the word maps
per set of roles that run together, and pack / unpack of the launch word.  Built stand-alone under AddressSanitizer +
UndefinedBehaviorSanitizer (the driver includes only that header; nothing is preloaded, no Python is involved)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_lds_layouts_word_maps_and_launch_word_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "fused_lds_model")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp", "fused_lds_model.cpp")]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "fused_lds_totals.txt")], capture_output=True, text=True, env=env,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "fused lds model: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    m = re.search(r"cases (\d+) failures (\d+)", r.stdout)
    # 7 BodyCtx sizes x (77 feature counts x staged or not + 50 tile feature counts), the 14 + 2 dispatch rows, the word maps of one /
    # two service waves and of tile single / pair, the launch word
    assert m and int(m.group(2)) == 0 and int(m.group(1)) == 7 * (77 * 2 + 50) + 14 + 2 + 4 + 1
