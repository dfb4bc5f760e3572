"""In-tree build of ``libdl4ss_hip.so`` (gfx950 only) with plain hipcc.

Every ``dl4ss_amd/csrc/*.hip`` is compiled to an object with
``hipcc --offload-arch=gfx950 -O3 -fPIC`` (in parallel) and linked into one
shared library next to this file.  The library exports the C ABI declared in
the public headers, the ``*.h`` files of ``include/``: every source includes
the core one, ``dl4ss_hip.h`` (through ``csrc/common.h``), and a source whose
entry points have a header of their own includes that one too, so a definition
that disagrees with its prototype fails to compile.  Objects are rebuilt only
when a source or header -- every public one included -- is newer than the
object.

An extension is a directory: the sources of ``csrc/<name>/*.hip`` are linked
into a library of their own, ``libdl4ss_<name>.so``, whose C ABI is declared
by the headers of ``include/<name>/`` (``_lib`` binds them from there).
``libdl4ss_hip.so`` keeps exporting exactly what the headers directly under
``include/`` declare.
"""
import concurrent.futures as cf
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "csrc", "_obj")
LIB = os.path.join(HERE, "libdl4ss_hip.so")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")  # (the sources include its headers by relative path)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
FLAGS = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-munsafe-fp-atomics",
         "-Wno-unused-result", "-fvisibility=hidden"]
# per-file extras: the STFT's radix-4x4 butterflies run 1.2-1.5x faster as scalar fp32
# than SLP-packed into v_pk_add_f32 (the packing needs a v_mov per pair of operands)
FILE_FLAGS = {"stft.hip": ["-fno-slp-vectorize"]}
# no vendor BLAS: every GEMM is a hand-written kernel (gemm.hip, gemm_gl.hip)
LINK = []


def _newer(src, dst, deps):
    if not os.path.exists(dst):
        return True
    t = os.path.getmtime(dst)
    return os.path.getmtime(src) > t or any(os.path.getmtime(d) > t for d in deps)


def _compile(src, obj):
    cmd = [HIPCC, *FLAGS, *FILE_FLAGS.get(os.path.basename(src), []), "-I", CSRC, "-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    return obj


def extensions():
    """name -> source directory of every extension: the directories under csrc/ that hold .hip files."""
    return {d: os.path.join(CSRC, d) for d in sorted(os.listdir(CSRC))
            if d != "_obj" and os.path.isdir(os.path.join(CSRC, d))
            and any(f.endswith(".hip") for f in os.listdir(os.path.join(CSRC, d)))}


def ext_lib(name):
    return os.path.join(HERE, f"libdl4ss_{name}.so")


def _headers(ext=None):
    dirs = [CSRC, INCLUDE] + ([os.path.join(CSRC, ext), os.path.join(INCLUDE, ext)] if ext else [])
    return [os.path.join(d, f) for d in dirs if os.path.isdir(d) for f in os.listdir(d) if f.endswith(".h")]


def _build_lib(src_dir, obj_dir, lib, headers, verbose, jobs):
    os.makedirs(obj_dir, exist_ok=True)
    srcs = sorted(f for f in os.listdir(src_dir) if f.endswith(".hip"))
    objs, todo = [], []
    for f in srcs:
        src = os.path.join(src_dir, f)
        obj = os.path.join(obj_dir, f[:-4] + ".o")
        objs.append(obj)
        if _newer(src, obj, headers):
            todo.append((src, obj))
    jobs = jobs or min(8, max(1, len(todo)))
    with cf.ThreadPoolExecutor(jobs) as ex:
        for obj in ex.map(lambda a: _compile(*a), todo):
            if verbose:
                print("compiled", os.path.basename(obj), file=sys.stderr)
    if todo or not os.path.exists(lib) or any(os.path.getmtime(o) > os.path.getmtime(lib) for o in objs):
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", *objs, "-o", lib, *LINK]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")
    return lib


def build(verbose=False, jobs=None):
    _build_lib(CSRC, OBJ, LIB, _headers(), verbose, jobs)
    for name, src_dir in extensions().items():
        _build_lib(src_dir, os.path.join(OBJ, name), ext_lib(name), _headers(name), verbose, jobs)
    return LIB


if __name__ == "__main__":
    print(build(verbose=True))
