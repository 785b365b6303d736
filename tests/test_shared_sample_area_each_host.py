"""The argument checks and the host plan of smoe_shared_sample_area_each with a real handle on a box without a GPU:
tests/host/shared_sample_area_each_args_driver.cpp linked with the host-only objects of `make hostcheck` (-DSMOE_HOST_TEST=1:
handles without a device, launches compiled out) under AddressSanitizer + UndefinedBehaviorSanitizer.  Every refusal returns
its code and names its argument in smoe_last_error; the host layer never reads the two device arrays (one-element arrays
under the sanitizer); the plan (LDS need, workgroup count, the two limits) is checked for every (dim, channels) with N = 0, 1,
SSE_POINTS - 1 .. SSE_POINTS + 1, 2^31 workgroups' worth and the 160 KB edge.  The program stands alone: no Python is loaded
under a sanitizer and nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "steered_mixture_of_experts_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_shared_sample_area_each_argument_checks_and_plan_under_asan_and_ubsan():
    build = subprocess.run(["make", "-C", CSRC, "hostcheck_shared_sample_area_each", "-j8"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert build.returncode == 0, build.stdout[-4000:]
    exe = os.path.join(CSRC, "hostcheck", "smoe_sharedsampleareaeachcheck")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    tail = run.stdout[-4000:]
    assert run.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in run.stdout and "runtime error" not in run.stdout, tail
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("sharedsampleareaeachcheck:") and last.endswith(" 0 failed"), tail
    assert int(last.split()[1]) > 250
