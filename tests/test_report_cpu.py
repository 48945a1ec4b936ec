"""The report of a search (csrc/hbird_report.h: what a finished search of a caller says about itself, and which of the screen's buffers the
read-outs may still hand out), alone and without a GPU: tests/report_check.cpp takes the type through the transitions in the order the searches
make them -- an fp32 search, screened searches where all queries certify, with a second pass, with a second pass and an fp32 tail, with
escalation off, served excluding searches with leftovers and with the hand-over straight to the rungs, buffers reused by a later search, the
bank's events, a change of the copy's form, a failed search, no search at all, three passes of a search with k > 256 -- and holds every
question and every derived count after every step; the level workspace's layout is held against its literal formulas for nq in
{0, 1, 63, 64, 65, 700}.  Built with AddressSanitizer + UndefinedBehaviorSanitizer (`make -C csrc report_check`) and run as a child process: a
mismatch or a sanitizer report is a non-zero exit status."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")


def test_search_report_transitions_under_asan_ubsan():
    subprocess.run(["make", "-C", CSRC, "report_check"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    exe = os.path.join(ROOT, "open-hummingbird-eval_amd", "lib", "build", "report_check")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "report_check: ok" in r.stdout
