"""The device-buffer type every allocation of an index is a member of (csrc/hbird_devbuf.h), alone and without a GPU: tests/devbuf_check.cpp
defines the header's three device functions over malloc / free / memcpy, with a switch that makes the n-th allocation fail, and checks the
growth policies, the prefix-keeping growth, the state after a failed allocation, moves, drops and hb_index_reserve's three-allocation
sequence against its own live counters.  Built with AddressSanitizer + UndefinedBehaviorSanitizer (`make -C csrc devbuf_check`) and run as
a child process: a mismatch, a leak or a sanitizer report is a non-zero exit status."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")


def test_device_buffer_contract_under_asan_ubsan():
    subprocess.run(["make", "-C", CSRC, "devbuf_check"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    exe = os.path.join(ROOT, "open-hummingbird-eval_amd", "lib", "build", "devbuf_check")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "devbuf_check: ok" in r.stdout
