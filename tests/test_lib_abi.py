"""CPU-side checks of the C ABI: the library builds, loads and exports every
symbol that a header of include/ declares, and no other dl4ss_ symbol; every
header is included by a source (no compute calls without a GPU)."""
import ctypes
import os
import re
import shutil
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "dl4ss_amd", "csrc")


def public_headers():
    return sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))


def declared_symbols():
    found = []
    for header in public_headers():
        txt = open(os.path.join(INCLUDE, header)).read()
        found += re.findall(r"^(?:int|long long|void) (dl4ss_\w+)\(", txt, flags=re.M)
    assert len(found) == len(set(found))  # no header declares a name again
    return sorted(found)


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert "dl4ss_stft_fwd" in syms and len(syms) >= 3
    assert "dl4ss_hip.h" in public_headers()


def test_library_exports_every_declared_symbol():
    from dl4ss_amd import build, _lib

    build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(lib, s), f"missing export {s}"
    # the Python binding knows every declared symbol, and nothing undeclared
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    if shutil.which("nm"):  # (binutils present) beside the mangled kernel stubs, exactly the declared symbols
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
        exported = sorted(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.split()[-1].startswith("dl4ss_"))
        assert exported == declared_symbols()


def test_every_public_header_is_included_by_a_source():
    """A header's prototypes are checked against the definitions only where a source compiles them."""
    sources = [open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))]
    for header in public_headers():
        include = re.compile(r'^\s*#\s*include\s*["<][^">\n]*\b' + re.escape(header) + '[">]', flags=re.M)
        assert any(include.search(text) for text in sources), f"no file under dl4ss_amd/csrc includes {header}"
