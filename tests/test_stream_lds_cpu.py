"""The dynamic-LDS carve-ups of k_propagate_stream, k_update_feat_stream, k_update_generic, k_eval_xdot and k_keep_features are
stated once (vi_ekf_amd/csrc/viekf_stream_lds.hpp: the kernel takes its pointers from the struct, the launch its byte count).
tests/cpp/stream_lds_model.cpp checks every struct for N = 0 .. 512 and several BodyCtx sizes: regions disjoint and inside
bytes(), doubles on 8-byte boundaries, bytes() equal to the expression the launch site used before.  The layouts of the wide-P
path (WideLds, BlkLds, PsvLds) and grouped_choice, the rule that picks between the two grouped updates, are in the same header and
the same program: named int sub-regions, 16-byte boundaries where a kernel reads double2, the choice against the dispatch logic
it replaced and against what the kernels assume of it, a few choices pinned.  Built stand-alone under
AddressSanitizer + UndefinedBehaviorSanitizer (the driver includes only that header; nothing is preloaded, no Python is involved)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_lds_layouts_for_every_n_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "stream_lds_model")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp", "stream_lds_model.cpp")]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "stream lds model: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    m = re.search(r"cases (\d+) failures (\d+)", r.stdout)
    # 513 feature counts x (7 BodyCtx sizes x (propagate, propagate with the matrix-core tail, eval_xdot) + update, generic, keep
    #                       + 7 BodyCtx sizes of WideLds + BlkLds at 16 / 24 / 32 + PsvLds
    #                       + the choice under 4 x 2 x 3 tunings + the pinned default) + the three pinned blocked rows
    assert m and int(m.group(2)) == 0 and int(m.group(1)) == 513 * (7 * 3 + 3 + 7 + 3 + 1 + 24 + 1) + 3
