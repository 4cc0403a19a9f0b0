"""CPU tier: the host side of chaindp_align_resident and chaindp_map_align_seqs -- the checks of the call's arguments, of what has to be
resident, of regions that go up to the hand-off and come down from it, and the reads' offsets (csrc/chaindp_handoff_plan.h, no HIP in
it) -- in a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer.  tests/handoff_stub/ hands the checks arrays of
exactly the stated lengths, makes every refusal and the valid calls beside them.  A sanitizer report (ASan's leak check at exit
included) or a failed assertion of the program fails the test."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "handoff_stub")


def test_handoff_plan_is_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ or make")
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-o", "probe", "probe.cpp"], cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    if r.returncode != 0:
        pytest.skip("sanitizer build not possible here: " + r.stdout[-400:])
    r = subprocess.run(["make", "-s", "all"], cwd=HERE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(HERE, "handoff_plan_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stdout and "LeakSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    m = re.search(r"handoff plan ok: (\d+) accepted, (\d+) refused", r.stdout)
    assert m and int(m.group(1)) >= 80 and int(m.group(2)) >= 60, r.stdout[-3000:]
