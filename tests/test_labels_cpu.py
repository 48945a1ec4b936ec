"""The label table of an index (csrc/hbird_labels.h: own rows as fp32 values or uint16 counts, their counters and sticky flag, the borrowed
table), alone and without a GPU: tests/labels_check.cpp takes the store through the orders the label entries make -- the row stride for
C in {1, 7, 8, 21, 151, 152, 512}, growth with the rows kept (following the bank's capacity, else x 1.5), a reset followed by a change of
form in both directions and by rows of a wider class count, the refused and the accepted denominator, converted and copied rows and what they
do to the conversion's read-back, the replacement by fp32 rows with and without rows, adopt / restore around a failing allocation, the truth
table of missing / own_rows / covers over own {none, short, covering} x borrowed {none, fp32, counts}, the three branches of view() field by
field, every error status, and a failing allocation at every ensure -- and holds every question after every step.  Built with
AddressSanitizer + UndefinedBehaviorSanitizer (`make -C csrc labels_check`) and run as a child process: a mismatch or a sanitizer report is a
non-zero exit status."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")


def test_label_store_transitions_under_asan_ubsan():
    subprocess.run(["make", "-C", CSRC, "labels_check"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    exe = os.path.join(ROOT, "open-hummingbird-eval_amd", "lib", "build", "labels_check")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "labels_check: ok" in r.stdout
