"""The bookkeeping of the bank's lazy copies (csrc/hbird_mirror.h: the fp16 tiles with their centred side arrays, the re-rank's row copy), alone
and without a GPU: tests/mirror_check.cpp defines the device functions of hbird_devbuf.h over malloc / free, with a switch that makes the n-th
allocation fail, and takes the two members of an index through a bank's life -- fresh, made at capacity 256, 100 rows converted, appended to
130 (the partly filled tile again) and to 256, moved to capacity 512, emptied, declined and asked again, dropped -- checking the three
numbers of each mirror, the pending tiles and the program's own live counters after every step; then the four allocations of the centre
arrays each made to fail (the member as before, nothing leaked) and the copies' own failing allocations (automatic: declined at the capacity).
Built with AddressSanitizer + UndefinedBehaviorSanitizer (`make -C csrc mirror_check`) and run as a child process: a mismatch, a leak or a
sanitizer report is a non-zero exit status."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")


def test_bank_copy_bookkeeping_under_asan_ubsan():
    subprocess.run(["make", "-C", CSRC, "mirror_check"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    exe = os.path.join(ROOT, "open-hummingbird-eval_amd", "lib", "build", "mirror_check")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "mirror_check: ok" in r.stdout
