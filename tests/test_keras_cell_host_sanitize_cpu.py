"""CPU sanitizer build of the recurrence entry points' host dispatch with DL4SS_RNN_HARD_GATES: csrc/birnn.hip and
the four kernel files it launches through, compiled host-only (--cuda-host-only: no device code) with
AddressSanitizer + UBSan, linked with the stand-alone driver tests/sanitize/keras_cell_abi_check.cpp and run with
halt_on_error -- every combination the flag is not accepted with must be refused before any device call.  (As
tests/test_voiceprint_host_sanitize_cpu.py: a test of its own, with its own flags.)  Builds into a temporary
directory, never the tree."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dl4ss_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
       "-Xarch_host", "-fno-sanitize-recover=undefined"]
# host-only objects in relocatable-device-code form: the link's (empty) device link supplies the fat binary the
# translation units' registrations reference
FLAGS = ["-O1", "-g", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-fgpu-rdc",
         "-Wno-unused-result", "-Wno-undefined-internal", "-I", CSRC, *SAN]
SOURCES = ["birnn.hip", "birnn_fwd.hip", "birnn_bwd.hip", "birnn_fwd_pk.hip", "birnn_bwd_pk.hip"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_hard_gates_dispatch_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as td:
        procs = []
        for src in SOURCES:  # independent translation units: compiled side by side
            obj = os.path.join(td, src.replace(".hip", ".o"))
            procs.append((obj, subprocess.Popen([HIPCC, *FLAGS, "-c", os.path.join(CSRC, src), "-o", obj],
                                                stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
        objs = []
        for obj, p in procs:
            _, err = p.communicate()
            assert p.returncode == 0, err[-2000:]
            objs.append(obj)
        drv = os.path.join(ROOT, "tests", "sanitize", "keras_cell_abi_check.cpp")
        dro = os.path.join(td, "keras_cell_abi_check.o")
        exe = os.path.join(td, "keras_cell_abi_check")
        r = subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-c", drv, "-o", dro],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run([HIPCC, "-fgpu-rdc", "--offload-arch=gfx950", *SAN, dro, *objs, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
                   UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", HIP_VISIBLE_DEVICES="")
        r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
