"""The book that keeps the form of P (Full / Lower / Packed) and the location of the live state (vi_ekf_amd/csrc/viekf_pform.hpp)
is pure host logic: tests/cpp/pform_model.cpp applies every event in every reachable state beside a ground truth per buffer and
checks that no reader can take a packed or stale-upper buffer for a better one.  Built stand-alone under AddressSanitizer +
UndefinedBehaviorSanitizer (the driver includes only that header; nothing is preloaded, no Python is involved)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_book_of_p_forms_exhaustively_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "pform_model")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pform_model.cpp")]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "pform model: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    m = re.search(r"states (\d+) violations (\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 1
    fired = [int(n) for n in re.findall(r"fired (\d+)", r.stdout)]
    assert len(fired) == 23 and min(fired) > 0, "an event was left out"
