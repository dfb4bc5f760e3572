"""ctypes binding of ``libdl4ss_hip.so``, derived from the C ABI's one declaration, ``include/dl4ss_hip.h``
(and ``include/dl4ss_imgq.h``, the image-query encoder's entry points, ``include/dl4ss_optim.h``, Nadam and
Keras's clipnorm, ``include/dl4ss_eval.h``, the target-speaker evaluation, and ``include/dl4ss_align.h``, ATTENTION 'align' on the
bf16 steps, parsed the same way into ``IMGQ_*``, ``OPTIM_*``, ``EVAL_*`` and ``ALIGN_*`` tables).

The header is parsed once at import: every prototype gives the entry point's ``argtypes`` (``SIGNATURES``), its
``restype`` (``RESTYPES``) and its parameter names (``PARAMS``); every enum constant and ``#define DL4SS_* <integer>``
lands in ``CONSTANTS``.  The same header is compiled against every definition (``csrc/common.h`` includes it), so
the binding, the prototypes and the definitions cannot drift apart.  A declaration the parser cannot fully
classify raises at import, with the offending text: it never guesses.

``call`` and ``query`` take positional arguments, then keywords by the header's parameter names (``pass_`` and
``lambda_`` for the two that are Python keywords); ``bind`` refuses a missing, unknown or repeated parameter and
any argument count but the prototype's with ``TypeError``, before the library is touched.

The product path has no CPU fallback: if the library is missing or a call returns a non-zero ``hipError_t`` this
raises ``RuntimeError`` with the HIP error string.  Tensors are passed as raw device pointers; every call is
enqueued on torch's current HIP stream.
"""
import ctypes
import keyword
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DL4SS_LIB", os.path.join(_HERE, "libdl4ss_hip.so"))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "dl4ss_hip.h")
IMGQ_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dl4ss_imgq.h")  # the image-query encoder's entry points
OPTIM_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dl4ss_optim.h")  # Nadam, Keras's clipnorm
EVAL_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dl4ss_eval.h")  # BSS Eval 2.0 gains, the eval mixture
ALIGN_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dl4ss_align.h")  # 'align' attention, bf16 V / dPre

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


with open(HEADER) as _f:
    SIGNATURES, RESTYPES, PARAMS, CONSTANTS = parse_header(_f.read())
# the second public header, in tables of its own: SIGNATURES / RESTYPES / PARAMS / exported_symbols() stay what
# dl4ss_hip.h declares
with open(IMGQ_HEADER) as _f:
    IMGQ_SIGNATURES, IMGQ_RESTYPES, IMGQ_PARAMS, IMGQ_CONSTANTS = parse_header(_f.read(), "dl4ss_imgq.h")
if set(IMGQ_SIGNATURES) & set(SIGNATURES):
    raise ValueError(f"dl4ss_imgq.h declares again: {sorted(set(IMGQ_SIGNATURES) & set(SIGNATURES))}")
# the third, likewise
with open(OPTIM_HEADER) as _f:
    OPTIM_SIGNATURES, OPTIM_RESTYPES, OPTIM_PARAMS, OPTIM_CONSTANTS = parse_header(_f.read(), "dl4ss_optim.h")
if set(OPTIM_SIGNATURES) & (set(SIGNATURES) | set(IMGQ_SIGNATURES)):
    raise ValueError("dl4ss_optim.h declares again: "
                     f"{sorted(set(OPTIM_SIGNATURES) & (set(SIGNATURES) | set(IMGQ_SIGNATURES)))}")
# the fourth
with open(EVAL_HEADER) as _f:
    EVAL_SIGNATURES, EVAL_RESTYPES, EVAL_PARAMS, EVAL_CONSTANTS = parse_header(_f.read(), "dl4ss_eval.h")
_EARLIER = set(SIGNATURES) | set(IMGQ_SIGNATURES) | set(OPTIM_SIGNATURES)
if set(EVAL_SIGNATURES) & _EARLIER:
    raise ValueError(f"dl4ss_eval.h declares again: {sorted(set(EVAL_SIGNATURES) & _EARLIER)}")
# the fifth
with open(ALIGN_HEADER) as _f:
    ALIGN_SIGNATURES, ALIGN_RESTYPES, ALIGN_PARAMS, ALIGN_CONSTANTS = parse_header(_f.read(), "dl4ss_align.h")
if set(ALIGN_SIGNATURES) & (_EARLIER | set(EVAL_SIGNATURES)):
    raise ValueError(f"dl4ss_align.h declares again: {sorted(set(ALIGN_SIGNATURES) & (_EARLIER | set(EVAL_SIGNATURES)))}")
_ALL_PARAMS = {**PARAMS, **IMGQ_PARAMS, **OPTIM_PARAMS, **EVAL_PARAMS, **ALIGN_PARAMS}
# keyword -> slot of every entry point (a header name that is a Python keyword takes a trailing underscore)
_SLOTS = {name: {p + "_" if keyword.iskeyword(p) else p: i for i, p in enumerate(ps)}
          for name, ps in _ALL_PARAMS.items()}
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
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    # the second to fifth headers' entry points.  A library without them still loads: the binding tests stand a
    # stub with the first header's names alone in for the library, and DL4SS_LIB may name a build from before
    # imgq.hip, optim.hip, targeteval.hip or the bf16 'align' forms.  Calling one that is missing fails in ctypes' own lookup, with the symbol's name:
    # there is no other path
    for sigs, restypes in ((IMGQ_SIGNATURES, IMGQ_RESTYPES), (OPTIM_SIGNATURES, OPTIM_RESTYPES),
                           (EVAL_SIGNATURES, EVAL_RESTYPES), (ALIGN_SIGNATURES, ALIGN_RESTYPES)):
        for name, argtypes in sigs.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.argtypes = argtypes
                fn.restype = restypes[name]
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipGetErrorString.restype = ctypes.c_char_p
    hip.hipGetErrorString.argtypes = [ctypes.c_int]
    lib._hip = hip
    _lib = lib
    return lib


def lib():
    return _load()


def exported_symbols():
    return list(SIGNATURES)


def imgq_exported_symbols():
    return list(IMGQ_SIGNATURES)


def optim_exported_symbols():
    return list(OPTIM_SIGNATURES)


def eval_exported_symbols():
    return list(EVAL_SIGNATURES)


def align_exported_symbols():
    return list(ALIGN_SIGNATURES)


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
    slots = _SLOTS.get(name)
    if slots is None:
        raise TypeError(f"{name} is not declared in include/dl4ss_hip.h, include/dl4ss_imgq.h, "
                        "include/dl4ss_optim.h, include/dl4ss_eval.h or include/dl4ss_align.h")
    n, given = len(slots), len(args) + len(kw)
    if len(args) > n:
        raise TypeError(f"{name} takes {n} arguments (the last is {_ALL_PARAMS[name][-1]!r}), {given} given")
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
    return getattr(_load(), name)(*args)


def call(name, *args, **kw):
    args = bind(name, args, kw)
    lb = _load()
    rc = getattr(lb, name)(*args)
    if rc != 0:
        msg = lb._hip.hipGetErrorString(rc).decode()
        raise RuntimeError(f"{name} failed: hipError {rc} ({msg})")
    return rc
