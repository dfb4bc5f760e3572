"""ctypes binding of ``libdl4ss_hip.so``, derived from the C ABI's one declaration: the public headers, every
``*.h`` file of ``include/``.  ``CORE_HEADER`` comes first and the library must define every entry point it
declares; an entry point of any other header is bound when the library has it and skipped when not, so a header
added to ``include/`` is bound with no change here.

Each header is parsed once at import into a ``Header``, kept by file name in ``HEADERS``, and ``merge_headers`` folds
them into one namespace, refusing an entry point or a constant that two headers declare: every prototype gives the
entry point's ``argtypes`` (``SIGNATURES``), its ``restype`` (``RESTYPES``) and its parameter names (``PARAMS``);
every enum constant and ``#define DL4SS_* <integer>`` lands in ``CONSTANTS``.  A header is compiled against the
definitions it declares (``csrc/common.h`` includes the core one, a source with a header of its own includes that),
so the binding, the prototypes and the definitions cannot drift apart.  A declaration the parser cannot fully
classify raises at import, with the offending text: it never guesses.

``call`` and ``query`` take positional arguments, then keywords by the header's parameter names (``pass_`` and
``lambda_`` for the two that are Python keywords); ``bind`` refuses a missing, unknown or repeated parameter and
any argument count but the prototype's with ``TypeError``, before the library is touched.

An extension is a directory: the headers of ``include/<name>/`` declare the C ABI of a library of its own,
``libdl4ss_<name>.so`` (``build.py`` links it from ``csrc/<name>/``).  They are parsed the same way into
``EXT_HEADERS`` (by file name), kept out of the merged tables above -- those stay what ``libdl4ss_hip.so`` exports --
and ``call`` / ``query`` / ``bind`` / ``exported_symbols`` find their entry points and constants (``EXT_CONSTANTS``)
there.  An extension may not declare a name that another header has.

The product path has no CPU fallback: if the library is missing or a call returns a non-zero ``hipError_t`` this
raises ``RuntimeError`` with the HIP error string.  Tensors are passed as raw device pointers; every call is
enqueued on torch's current HIP stream.
"""
import collections
import ctypes
import keyword
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DL4SS_LIB", os.path.join(_HERE, "libdl4ss_hip.so"))
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
CORE_HEADER = "dl4ss_hip.h"  # the one header whose every entry point the library must define

P = ctypes.c_void_p
I = ctypes.c_int
LL = ctypes.c_longlong
F = ctypes.c_float
U = ctypes.c_uint
D = ctypes.c_double

_VALUE = {"int": I, "long long": LL, "float": F, "unsigned": U, "double": D}  # by-value parameter types
_POINTEE = set(_VALUE) | {"void", "double"}  # what a pointer or array parameter may point at
_RETURN = {"int": I, "long long": LL, "void": None}
_PROTO = re.compile(r"(int|long long|void)\s+(dl4ss_\w+)\s*\(([^()]*)\)\s*;")
_INT = r"(0[xX][0-9a-fA-F]+|\d+)"


Header = collections.namedtuple("Header", "signatures restypes params constants")


def parse_header(text, name="dl4ss_hip.h"):
    """(signatures, restypes, params, constants) of the header ``text`` (``name``: what an error calls it):
    entry -> argtypes list, entry -> restype, entry -> parameter names, and the integer enum constants and
    object-like ``DL4SS_*`` macros."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    sigs, res, params, consts = {}, {}, {}, {}
    for m in re.finditer(r"^(?!\s*#)[^\n]*\bdl4ss_\w+\s*\(", text, flags=re.M):  # every line that opens a prototype
        line = m.group(0).strip()
        proto = _PROTO.match(text, m.start())
        if not proto:
            raise ValueError(f"{name}: cannot parse the declaration at {line!r}")
        ret, entry, plist = proto.groups()
        argtypes, names = [], []
        for p in plist.split(","):
            words = [w for w in re.findall(r"[A-Za-z_]\w*", re.sub(r"\[\d*\]", "", p)) if w != "const"]
            base, pname = " ".join(words[:-1]), words[-1] if words else ""
            pointer = "*" in p or "[" in p
            if base not in (_POINTEE if pointer else _VALUE) or pname in names:
                raise ValueError(f"{name}: cannot classify parameter {p.strip()!r} of {line!r} "
                                 "(unknown type, no name or a repeated name)")
            argtypes.append(P if pointer else _VALUE[base])
            names.append(pname)
        sigs[entry], res[entry], params[entry] = argtypes, _RETURN[ret], tuple(names)
    for m in re.finditer(r"\benum\b[^;]*;", text):  # anonymous `enum { ... };` only: any other form is refused
        enum = re.fullmatch(r"enum\s*\{([^{}]*)\}\s*;", m.group(0))
        if not enum:
            raise ValueError(f"{name}: cannot parse the enum at {m.group(0)[:60]!r}")
        for item in filter(None, (x.strip() for x in enum.group(1).split(","))):
            m = re.fullmatch(r"(\w+)\s*=\s*" + _INT, item)
            if not m:
                raise ValueError(f"{name}: enum constant {item!r} has no integer value")
            consts[m.group(1)] = int(m.group(2), 0)
    for m in re.finditer(r"^#define[ \t]+(DL4SS_\w+)[ \t]+([^\n]*)$", text, flags=re.M):  # (not function-like)
        if not re.fullmatch(_INT, m.group(2).strip()):
            raise ValueError(f"{name}: macro {m.group(0)!r} is not an integer")
        consts[m.group(1)] = int(m.group(2).strip(), 0)
    return sigs, res, params, consts


def merge_headers(parsed):
    """The one namespace of ``parsed`` (file name -> ``Header``, in order): ``ValueError`` for an entry point or a
    constant that a second header declares, naming it and both headers."""
    merged, first = Header({}, {}, {}, {}), {}
    for name, header in parsed.items():
        for symbol in (*header.signatures, *header.constants):
            if symbol in first:
                raise ValueError(f"{name} declares {symbol} again: {first[symbol]} has it")
            first[symbol] = name
        for table, part in zip(merged, header):
            table.update(part)
    return merged


def _parse(name):
    with open(os.path.join(INCLUDE, name)) as f:
        return Header(*parse_header(f.read(), os.path.basename(name)))


HEADERS = {name: _parse(name) for name in
           [CORE_HEADER] + sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h") and f != CORE_HEADER)}
SIGNATURES, RESTYPES, PARAMS, CONSTANTS = merge_headers(HEADERS)
# keyword -> slot of every entry point (a header name that is a Python keyword takes a trailing underscore)
_SLOTS = {name: {p + "_" if keyword.iskeyword(p) else p: i for i, p in enumerate(ps)}
          for name, ps in PARAMS.items()}


def _parse_extensions():
    """(file name -> Header, file name -> library path) of the headers of include/<name>/, refusing a repeated file
    name or a symbol that a header parsed before declares."""
    headers, libs, first = {}, {}, {s: n for n, h in HEADERS.items() for s in (*h.signatures, *h.constants)}
    for ext in sorted(d for d in os.listdir(INCLUDE) if os.path.isdir(os.path.join(INCLUDE, d))):
        for f in sorted(f for f in os.listdir(os.path.join(INCLUDE, ext)) if f.endswith(".h")):
            if f in HEADERS or f in headers:
                raise ValueError(f"include/{ext}/{f}: a header of that name exists already")
            headers[f] = _parse(os.path.join(ext, f))
            libs[f] = os.path.join(_HERE, f"libdl4ss_{ext}.so")
            for symbol in (*headers[f].signatures, *headers[f].constants):
                if symbol in first:
                    raise ValueError(f"{f} declares {symbol} again: {first[symbol]} has it")
                first[symbol] = f
    return headers, libs


EXT_HEADERS, EXT_LIBS = _parse_extensions()
EXT_CONSTANTS = {k: v for h in EXT_HEADERS.values() for k, v in h.constants.items()}
_EXT_OF = {entry: name for name, h in EXT_HEADERS.items() for entry in h.signatures}  # entry point -> its header
_EXT_SLOTS = {entry: {p + "_" if keyword.iskeyword(p) else p: i for i, p in enumerate(EXT_HEADERS[name].params[entry])}
              for entry, name in _EXT_OF.items()}
# knobs the library itself used to read from the environment, retired with plan.RETIRED_KNOBS
RETIRED_ENV = ("DL4SS_ATTN_TILES", "DL4SS_RNN_MAX_WG", "DL4SS_RNN_MIN_BC")

_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    for name in RETIRED_ENV:
        if name in os.environ:
            raise ValueError(f"{name} is retired, its default is the only path (DESIGN.md section 11): unset it")
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"dl4ss HIP library not found at {LIB_PATH}; run `python -m dl4ss_amd.build` "
            "(there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    # an entry point of the core header must resolve.  One of another header is bound when the library has it: the
    # binding tests stand a stub with the core header's names alone in for the library, and DL4SS_LIB may name a
    # build from before that header's source.  Calling one that is missing fails in ctypes' own lookup, with the
    # symbol's name: there is no other path
    for header_name, header in HEADERS.items():
        for name, argtypes in header.signatures.items():
            fn = getattr(lib, name) if header_name == CORE_HEADER else getattr(lib, name, None)
            if fn is not None:
                fn.argtypes = argtypes
                fn.restype = header.restypes[name]
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipGetErrorString.restype = ctypes.c_char_p
    hip.hipGetErrorString.argtypes = [ctypes.c_int]
    lib._hip = hip
    _lib = lib
    return lib


def lib():
    return _load()


_ext_libs = {}


def _load_ext(header):
    """The extension library that defines ``header``'s entry points, every one of them bound (all must resolve)."""
    if header not in _ext_libs:
        path = EXT_LIBS[header]
        if not os.path.exists(path):
            raise RuntimeError(f"dl4ss extension library not found at {path}; run `python -m dl4ss_amd.build` "
                               "(there is no CPU fallback)")
        ext, h = ctypes.CDLL(path), EXT_HEADERS[header]
        for name, argtypes in h.signatures.items():
            fn = getattr(ext, name)
            fn.argtypes, fn.restype = argtypes, h.restypes[name]
        _ext_libs[header] = ext
    return _ext_libs[header]


def _entry(name):
    """The bound function ``name`` of the library that defines it."""
    return getattr(_load_ext(_EXT_OF[name]) if name in _EXT_OF else _load(), name)


def exported_symbols(header=None):
    """Every entry point of libdl4ss_hip.so, or those of the one header (a file name, an extension's too) given."""
    if header is None:
        return list(SIGNATURES)
    return list((HEADERS[header] if header in HEADERS else EXT_HEADERS[header]).signatures)


def stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def ptr(t, strided=False):
    """Raw device pointer of a CUDA tensor.  Unless the call site passes the
    strides itself (``strided=True``), the tensor must be contiguous: a kernel
    sees only the pointer, so a transposed view would be silently misread."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("dl4ss HIP op received a CPU tensor (no CPU fallback)")
    if not strided and not t.is_contiguous():
        raise RuntimeError("dl4ss HIP op received a non-contiguous tensor")
    return ctypes.c_void_p(t.data_ptr())


def bind(name, args, kw):
    """The positional tuple of one call of ``name``: ``args`` first, then ``kw`` by the header's parameter names.
    ``TypeError`` unless every parameter of the prototype is given exactly once."""
    slots, params = (_EXT_SLOTS[name], EXT_HEADERS[_EXT_OF[name]].params[name]) if name in _EXT_OF else \
        (_SLOTS.get(name), PARAMS.get(name))
    if slots is None:
        raise TypeError(f"{name} is not declared in " + ", ".join("include/" + h for h in HEADERS))
    n, given = len(slots), len(args) + len(kw)
    if len(args) > n:
        raise TypeError(f"{name} takes {n} arguments (the last is {params[-1]!r}), {given} given")
    if not kw and given == n:
        return tuple(args)
    out = list(args) + [None] * (n - len(args))
    for k, v in kw.items():
        i = slots.get(k)
        if i is None:
            raise TypeError(f"{name} has no parameter {k!r}")
        if i < len(args):
            raise TypeError(f"{name}: parameter {k!r} given by position and by keyword")
        out[i] = v
    if given != n:  # the keywords are distinct and behind args, so fewer than n leaves a slot unfilled
        missing = [k for k, i in slots.items() if i >= len(args) and k not in kw]
        raise TypeError(f"{name}: missing parameter {missing[0]!r} ({given} of {n} given)")
    return tuple(out)


def query(name, *args, **kw):
    """Call an entry point that returns a value (sizes), not an error code."""
    args = bind(name, args, kw)
    return _entry(name)(*args)


def call(name, *args, **kw):
    args = bind(name, args, kw)
    rc = _entry(name)(*args)
    if rc != 0:
        msg = _load()._hip.hipGetErrorString(rc).decode()
        raise RuntimeError(f"{name} failed: hipError {rc} ({msg})")
    return rc
