"""The work-list planner with the filled clustered dealing as a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/schedule_filled_check.cpp, `make -C csrc schedule_filled_check`): the shapes of tests/test_schedule_filled_cpu.py, both sharing forms,
with and without XCD shares, phased and not, filled and refused at the slot limit, every list walked as the kernels and the launcher walk
it.  Run as a child process: a mismatch or a sanitizer report is a non-zero exit status.  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")


def test_filled_planner_under_asan_ubsan():
    subprocess.run(["make", "-C", CSRC, "schedule_filled_check"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    exe = os.path.join(ROOT, "open-hummingbird-eval_amd", "lib", "build", "schedule_filled_check")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "schedule_filled_check: ok" in r.stdout
