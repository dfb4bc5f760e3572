"""CPU sanitizer build of the device-resident corpus entry points' host logic: csrc/corpus/corpus.hip compiled
host-only (--cuda-host-only: no device code) with AddressSanitizer + UBSan, linked with the stand-alone driver
tests/sanitize/corpus_abi_check.cpp and run directly with halt_on_error -- both entry points must refuse bad
arguments before any device call.  Built exactly as tests/test_imgq_host_sanitize_cpu.py builds its driver: nothing
is preloaded and nothing is loaded into Python.  Builds into a temporary directory, never the tree."""
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
# a host-only object in relocatable-device-code form: the link's (empty) device link supplies the fat binary the
# translation unit's registration references
FLAGS = ["-O1", "-g", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-fgpu-rdc",
         "-Wno-unused-result", "-Wno-undefined-internal", "-I", CSRC, *SAN]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_corpus_abi_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as td:
        obj = os.path.join(td, "corpus.o")
        r = subprocess.run([HIPCC, *FLAGS, "-c", os.path.join(CSRC, "corpus", "corpus.hip"), "-o", obj],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        drv = os.path.join(ROOT, "tests", "sanitize", "corpus_abi_check.cpp")
        dro = os.path.join(td, "corpus_abi_check.o")
        exe = os.path.join(td, "corpus_abi_check")
        r = subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-c", drv, "-o", dro],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run([HIPCC, "-fgpu-rdc", "--offload-arch=gfx950", *SAN, dro, obj, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
                   UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", HIP_VISIBLE_DEVICES="")
        r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
