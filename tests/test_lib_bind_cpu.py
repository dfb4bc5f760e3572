"""The binding is derived from the headers of include/, and each is compiled against the definitions (host only).

  * the core header's derived signatures / restypes equal the hand-written tables they replaced, kept below as the
    specification; the merged tables are the disjoint union of every header's;
  * the parser refuses what it cannot classify, naming the text;
  * a definition that disagrees with its prototype does not compile (and the true one does);
  * _lib.bind puts keywords into the header's order and refuses a wrong set of arguments with TypeError;
  * the constants of ops are the header's; the three environment reads the library retired are refused;
  * the converted call sites put every named tensor into its header slot (the library, _lib.ptr and the stream
    stubbed, in the style of test_birnn_wrappers_cpu.py)."""
import ctypes
import os
import re
import subprocess
import types

import pytest
import torch

from conftest import ROOT
from dl4ss_amd import _lib, build, engine, ops, plan

P, I, LL, F, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_uint

# ---- the specification: the tables dl4ss_amd/_lib.py carried by hand, verbatim ----
# name -> argtypes (all return int hipError_t)
SIGNATURES = {
    "dl4ss_stft_fwd": [P, LL, I, I, I, I, P, P, P],
    "dl4ss_stft_fwd_ex": [P, LL, I, I, I, I, P, P, P, LL, LL, P],
    "dl4ss_istft": [P, LL, I, I, I, I, P, P],
    "dl4ss_mix_sources": [P, P, I, I, I, P, P, P, P],
    "dl4ss_gemm": [I, I, I, I, I, P, LL, P, LL, P, LL, P, I, F, I, I, P],
    "dl4ss_gemm_fixed": [I, I, I, I, I, P, LL, P, LL, P, LL, P, I, F, I, I, P, LL, P],
    "dl4ss_gemm_fixed_ws_bytes": [I, I, I, I],
    "dl4ss_gemm_fixed_kps": [I, I],
    "dl4ss_f32_to_bf16": [P, P, LL, P],
    "dl4ss_f32_to_bf16_2d": [P, LL, I, I, P, LL, P],
    "dl4ss_f32_to_bf16_hilo": [P, LL, I, I, P, LL, I, I, U, P],
    "dl4ss_birnn_bias_reduce": [I, I, I, I, P, P, P, P],
    "dl4ss_birnn_bias_reduce_ex": [I, I, I, I, P, P, P, F, P],
    "dl4ss_colsum_bf16": [P, LL, I, I, P, P],
    "dl4ss_colsum_bf16_part_bytes": [I, I],
    "dl4ss_colsum_bf16_det": [P, LL, I, I, P, P, LL, P],
    "dl4ss_colsum_bf16_det_ex": [P, LL, I, I, P, P, LL, F, P],
    "dl4ss_gemm_bf16_gl_ws_bytes": [I, I, I, I, I],
    "dl4ss_gemm_gl_set_config": [I],
    "dl4ss_gemm_bf16_gl": [I, I, I, I, I, P, LL, P, LL, P, LL, P, I, F, I, I, LL, LL, LL, P, LL, P],
    "dl4ss_gemm_bf16_gl_grouped_ws_bytes": [I, P, P, P, P],
    "dl4ss_gemm_bf16_gl_grouped": [I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, LL, P],
    "dl4ss_gemm_bf16_gl_grouped_ex": [I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, LL, I, I, I, P, P],
    "dl4ss_birnn_fwd_ex": [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, LL, P, P],
    "dl4ss_birnn_fwd_xw": [I, I, I, I, P, I, LL, P, LL, P, P, P, P, P, P, P, P, P, P, LL, P, P, I],
    "dl4ss_birnn_fwd_mean": [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, LL, P, P],
    "dl4ss_birnn_fwd_xw_ex": [I, I, I, I, P, I, LL, P, LL, P, P, P, P, P, P, P, P, P, P, P, LL, P, P, I],
    "dl4ss_birnn_fwd_xw_supported": [I, I, I, I, I],
    "dl4ss_birnn_bwd_ex": [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, LL, P, P],
    "dl4ss_mask_attn_loss_ex": [I, I, I, I, I, I, I, P, P, P, LL, P, LL, LL, P, F, F, P, P, LL, P, P, P, P, P],
    "dl4ss_birnn_workspace_bytes": [I, I, I],
    "dl4ss_birnn_fwd": [I, I, I, I, I, P, P, P, P, P, P, P, P, LL, P, P],
    "dl4ss_birnn_bwd": [I, I, I, I, I, P, P, P, P, P, P, P, P, P, LL, P, P],
    "dl4ss_attn_nblk": [I, I],
    "dl4ss_mask_attn_loss": [I, I, I, I, I, I, I, P, P, P, LL, P, LL, LL, P, F, F, P, P, P, P, P, P],
    "dl4ss_pit_select": [P, I, I, I, P, P],
    "dl4ss_loss_finalize": [P, I, I, I, P, F, F, P, P, I, P, P],
    "dl4ss_query_fwd": [P, I, I, I, P, P, P, I, I, P, P, P],
    "dl4ss_query_bwd": [P, I, I, I, P, P, P, P, I, I, P, P, P, P],
    "dl4ss_query_bwd_ex": [P, I, I, I, P, P, P, P, I, I, P, P, P, I, F, P],
    "dl4ss_colsum": [P, LL, I, I, P, P],
    "dl4ss_adam": [P, P, P, P, LL, F, F, F, F, I, P],
    "dl4ss_istft_apply": [P, P, LL, I, I, I, I, P, P],
    "dl4ss_tanh_bwd": [P, P, P, LL, P],
    "dl4ss_attn_dot_nblk": [I],
    "dl4ss_attn_dot_fwd": [P, P, I, I, I, I, I, P, P],
    "dl4ss_attn_dot_bwd": [P, P, I, P, P, I, I, I, I, P, P, P, P],
    "dl4ss_top_k_mask": [P, I, I, F, I, P, P, P, P],
    "dl4ss_attn_dot_fwd_ex": [P, P, I, I, I, I, I, P, LL, P],
    "dl4ss_classifier_select": [P, I, I, F, I, P, I, P, P, P, P],
    "dl4ss_mask_split": [P, P, LL, P, P, P],
    "dl4ss_time_mean": [P, I, I, I, P, P],
    "dl4ss_bss_corr": [P, I, I, I, I, P, P],
    "dl4ss_mix_sources_ex": [P, P, P, I, I, I, P, P, P, P],
    "dl4ss_mix_sources_rot": [P, P, P, P, I, I, I, P, P, P, P],
    "dl4ss_f32_to_bf16_2d_multi": [I, P, P, P, P, P, P, P],
    "dl4ss_mask_attn_loss_bf16v": [I, I, I, I, I, I, I, P, P, P, LL, P, LL, LL, P, F, F, P, P, LL, P, P, P, P, P],
    "dl4ss_bss_gram": [P, I, I, I, I, P, P, P, P],
    "dl4ss_adam_guarded": [P, P, P, P, LL, F, F, F, F, I, P, P, P],
    "dl4ss_adam_guarded_dp": [P, P, P, P, LL, F, F, F, F, I, P, P, P, P],
    "dl4ss_adam_guarded_dp_scaled": [P, P, P, P, LL, F, F, F, F, I, P, P, F, P, P],
    "dl4ss_adam_guarded_dp_scaled_bf16": [P, P, P, P, LL, F, F, F, F, I, P, P, F, P, I, P, P, P, P, P, P],
    "dl4ss_grad_sumsq_parts": [LL],
    "dl4ss_grad_sumsq": [P, LL, P, P],
    "dl4ss_adam_clipped": [P, P, P, P, LL, F, F, F, F, I, P, P, F, P, I, P, P, P, P, P, P, I, F, P, P, P],
    "dl4ss_status_flag": [P, P, P],
    "dl4ss_birnn_plan_info": [I, I, I, I, I, P],
    "dl4ss_debug_set_spin_limit": [ctypes.c_uint],
    "dl4ss_debug_set_place_force": [ctypes.c_int],
    "dl4ss_debug_set_rnn_max_wg": [ctypes.c_int],
    "dl4ss_attn_align_nblk": [I],
    "dl4ss_attn_align_part_floats": [I, I, I],
    "dl4ss_attn_align_fwd": [P, P, I, P, P, P, I, I, I, P, LL, P],
    "dl4ss_attn_align_bwd": [P, P, I, P, P, P, P, I, I, I, P, P, LL, P, P, P, P, P],
    "dl4ss_mask_attn_align_loss": [I, I, I, I, I, I, P, P, P, P, P, P, LL, P, LL, LL, P, F, F, P, P, P, LL, P, P, P],
    "dl4ss_attn_align_finalize": [P, LL, I, I, I, I, P, P, P, P, P, P, P],
    "dl4ss_cls_head_fwd": [P, P, P, I, I, I, P, P, P],
    "dl4ss_cls_head_loss_bwd": [P, P, P, P, I, I, I, I, P, P, P, P, P, P],
    "dl4ss_disc_dims": [I, I, P],
    "dl4ss_disc_ws_bytes": [I, I, I],
    "dl4ss_disc_conv1_fwd": [I, P, P, P, I, I, I, P, P],
    "dl4ss_disc_conv64_fwd": [I, P, P, P, I, I, I, P, P],
    "dl4ss_disc_head_fwd": [I, P, P, P, I, I, I, P, P, P],
    "dl4ss_disc_head_bwd": [I, P, P, P, P, F, I, I, I, P, P, P, P, P, P],
    "dl4ss_disc_conv64_bwd": [I, P, P, P, P, I, I, I, P, P, P, P, LL, P],
    "dl4ss_disc_conv1_bwd": [I, P, P, P, P, I, I, I, P, P, P, P, LL, P],
    "dl4ss_mask_attn_loss_adv": [I, I, I, I, I, P, P, P, LL, P, LL, LL, P, F, F, P, P, P, LL, P, P, P, P, P],
    "dl4ss_mask_attn_loss_adv_bf16v": [I, I, I, I, I, P, P, P, LL, P, LL, LL, P, F, F, P, P, P, LL, P, P, P, P, P],
    "dl4ss_disc_adv_heads": [P, I, F, P, P, P, P],
    "dl4ss_vp_compact": [P, I, I, I, I, F, P, P, P, P, P],
    "dl4ss_vp_shift": [P, P, I, I, I, I, I, P, I, I, P],
    "dl4ss_vp_mean_fwd": [P, I, I, I, P, P, P],
    "dl4ss_vp_mean_bwd": [P, I, I, I, P, P, P],
    "dl4ss_vp_colsum_parts": [LL],
    "dl4ss_vp_colsum": [P, LL, I, P, P, P],
    "dl4ss_spk_memory_fwd": [P, P, P, I, I, I, P, P, P],
    "dl4ss_spk_memory_bwd": [P, P, P, P, P, I, I, I, P, P],
    "dl4ss_spk_memory_store": [P, P, I, I, I, P, P, P],
}
# entry points that return a value rather than a hipError_t
RESTYPES = {"dl4ss_birnn_workspace_bytes": ctypes.c_longlong, "dl4ss_colsum_bf16_part_bytes": ctypes.c_longlong,
            "dl4ss_gemm_bf16_gl_ws_bytes": ctypes.c_longlong, "dl4ss_grad_sumsq_parts": ctypes.c_longlong,
            "dl4ss_gemm_bf16_gl_grouped_ws_bytes": ctypes.c_longlong, "dl4ss_attn_nblk": ctypes.c_int,
            "dl4ss_attn_dot_nblk": ctypes.c_int, "dl4ss_attn_align_nblk": ctypes.c_int,
            "dl4ss_attn_align_part_floats": ctypes.c_longlong, "dl4ss_disc_ws_bytes": ctypes.c_longlong,
            "dl4ss_vp_colsum_parts": ctypes.c_longlong, "dl4ss_gemm_fixed_ws_bytes": ctypes.c_longlong,
            "dl4ss_gemm_fixed_kps": ctypes.c_int, "dl4ss_debug_set_spin_limit": None,
            "dl4ss_debug_set_place_force": None, "dl4ss_debug_set_rnn_max_wg": None}


CORE = _lib.HEADERS["dl4ss_hip.h"]


def test_derived_tables_equal_the_hand_written_ones():
    assert len(SIGNATURES) == 98 and sorted(CORE.signatures) == sorted(SIGNATURES)
    assert _lib.exported_symbols("dl4ss_hip.h") == list(CORE.signatures)
    for name, argtypes in SIGNATURES.items():
        assert CORE.signatures[name] == argtypes, name
        assert CORE.restypes[name] == RESTYPES.get(name, ctypes.c_int), name  # (int: a hipError_t)
        assert len(CORE.params[name]) == len(argtypes), name


def test_merged_tables_are_the_disjoint_union_of_the_headers():
    assert next(iter(_lib.HEADERS)) == _lib.CORE_HEADER == "dl4ss_hip.h"
    assert list(_lib.HEADERS)[1:] == sorted(f for f in os.listdir(os.path.join(ROOT, "include"))
                                            if f.endswith(".h") and f != "dl4ss_hip.h")
    assert len(_lib.SIGNATURES) == sum(len(h.signatures) for h in _lib.HEADERS.values()) == 110
    assert len(_lib.CONSTANTS) == sum(len(h.constants) for h in _lib.HEADERS.values()) == 35
    assert _lib.exported_symbols() == list(_lib.SIGNATURES) == [n for h in _lib.HEADERS.values() for n in h.signatures]
    for h in _lib.HEADERS.values():
        assert isinstance(h, _lib.Header) and set(h.signatures) == set(h.restypes) == set(h.params)
        for name in h.signatures:
            assert (_lib.SIGNATURES[name], _lib.RESTYPES[name], _lib.PARAMS[name]) == \
                (h.signatures[name], h.restypes[name], h.params[name]), name
        assert h.constants.items() <= _lib.CONSTANTS.items()
    assert set(_lib._SLOTS) == set(_lib.PARAMS) == set(_lib.RESTYPES) == set(_lib.SIGNATURES)


def test_parameter_names_are_the_headers():
    """Each header's params against a second, independent reading of its file (the one test_birnn_wrappers_cpu.py
    uses)."""
    for header, (_, _, table, _) in _lib.HEADERS.items():
        text = open(os.path.join(ROOT, "include", header)).read()
        assert table, header
        for name, params in table.items():
            m = re.search(r"\b(?:int|long long|void)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
            assert m, name
            assert [re.split(r"[\s*]+", p.strip().split("[")[0])[-1] for p in m.group(1).split(",")] == list(params), \
                name
            assert len(set(params)) == len(params), name


# ---- the parser fails closed ----
GOOD = ("int dl4ss_a(const float* x, long long n, unsigned m,\n"
        "            int hw[6], float s, void* const* ys, void* stream);\n")


def test_parser_reads_values_pointers_arrays_and_constants():
    text = ("/* int dl4ss_in_a_comment(int x); */\nenum { DL4SS_X = 3, DL4SS_Y = 0x10 /* sixteen */ };\n"
            "#define DL4SS_FLAG 0x100\n#define DL4SS_FN(S) ((S) << 2)\n#define DL4SS_GUARD_H\n" + GOOD +
            "long long dl4ss_b(int n);\nvoid dl4ss_c(unsigned limit);\n")
    sigs, res, params, consts = _lib.parse_header(text)
    assert sigs == {"dl4ss_a": [P, LL, U, P, F, P, P], "dl4ss_b": [I], "dl4ss_c": [U]}  # int hw[6]: a pointer slot
    assert res == {"dl4ss_a": I, "dl4ss_b": LL, "dl4ss_c": None}
    assert params["dl4ss_a"] == ("x", "n", "m", "hw", "s", "ys", "stream")
    assert consts == {"DL4SS_X": 3, "DL4SS_Y": 16, "DL4SS_FLAG": 256}


@pytest.mark.parametrize("bad,named", [
    ("int dl4ss_a(const half* x, int n);\n", "const half* x"),  # an unknown type
    ("int dl4ss_a(size_t n);\n", "size_t n"),
    ("int dl4ss_a(const float*, int n);\n", "const float*"),  # an unnamed parameter
    ("int dl4ss_a(int, int n);\n", "'int'"),
    ("int dl4ss_a(int n, float n);\n", "float n"),  # a repeated name
    ("int dl4ss_a(const float* x, int n\n", "dl4ss_a("),  # truncated: no closing parenthesis
    ("int dl4ss_a(const float* x, int n)\n" + GOOD, "dl4ss_a("),  # no semicolon
    ("static int dl4ss_a(int n);\n", "static int dl4ss_a("),  # more than the pattern in front
    ("double dl4ss_a(int n);\n", "double dl4ss_a("),  # an unknown return type
    ("enum { DL4SS_X = 1, DL4SS_Y };\n", "DL4SS_Y"),  # a constant without a value
    ("enum dl4ss_mode { DL4SS_X = 1 };\n", "enum dl4ss_mode"),  # a tagged enum: not skipped, refused
    ("typedef enum { DL4SS_X = 1 } dl4ss_mode;\n", "} dl4ss_mode"),
    ("#define DL4SS_FLAG (1 << 8)\n", "DL4SS_FLAG"),  # an object-like macro that is no integer
])
def test_parser_refuses_what_it_cannot_classify(bad, named):
    with pytest.raises(ValueError) as e:
        _lib.parse_header(GOOD.replace("dl4ss_a", "dl4ss_ok") + bad)
    assert named in str(e.value)


# ---- the header is compiled against the definitions ----
def _syntax_only(tmp_path, first_param):
    src = tmp_path / "probe.hip"
    src.write_text('#include "common.h"\n'
                   f"DL4SS_API int dl4ss_attn_nblk({first_param} T, int F) {{\n  return (int)T + F;\n}}\n")
    return subprocess.run([build.HIPCC, *build.FLAGS, "-I", build.CSRC, "--cuda-host-only", "-fsyntax-only", str(src)],
                          capture_output=True, text=True)


def test_definition_that_disagrees_with_its_prototype_does_not_compile(tmp_path):
    r = _syntax_only(tmp_path, "long long")
    assert r.returncode != 0 and "conflicting types for 'dl4ss_attn_nblk'" in r.stderr, r.stderr
    r = _syntax_only(tmp_path, "int")  # the control: the true parameter list compiles
    assert r.returncode == 0, r.stderr


# ---- bind ----
def test_bind_orders_keywords_and_refuses_a_wrong_set():
    name = "dl4ss_pit_select"  # (part_loss, B, K, nblk, perm, stream)
    full = dict(part_loss="pl", B=4, K=2, nblk=3, perm="pm", stream="st")
    want = ("pl", 4, 2, 3, "pm", "st")
    assert _lib.PARAMS[name] == tuple(full)
    assert _lib.bind(name, want, {}) == want
    assert _lib.bind(name, (), dict(reversed(full.items()))) == want
    assert _lib.bind(name, ("pl", 4), dict(stream="st", perm="pm", nblk=3, K=2)) == want
    for args, kw, msg in (
            (want[:-1], {}, "'stream'"),  # one too few
            (("pl", 4), dict(K=2, nblk=3, stream="st"), "'perm'"),
            (want + (0,), {}, "7 given"),  # one too many
            (want, dict(stream="st"), "'stream' given by position and by keyword"),
            (want[:5], dict(strm="st"), "'strm'"),  # unknown
            (want[:5], dict(perm="pm"), "'perm' given by position and by keyword"),
            (want[:5], dict(perm="pm", stream="st"), "'perm' given by position and by keyword")):
        with pytest.raises(TypeError, match=msg) as e:
            _lib.bind(name, args, kw)
        assert name in str(e.value)
    with pytest.raises(TypeError, match="dl4ss_nothing"):
        _lib.bind("dl4ss_nothing", (), {})


def test_bind_renames_the_python_keywords():
    n = len(_lib.PARAMS["dl4ss_mask_attn_loss_ex"])
    kw = {p: i for i, p in enumerate(_lib.PARAMS["dl4ss_mask_attn_loss_ex"])}
    assert kw.pop("pass") == 0
    assert _lib.bind("dl4ss_mask_attn_loss_ex", (), dict(kw, pass_=0)) == tuple(range(n))
    with pytest.raises(TypeError, match="'pass'"):
        _lib.bind("dl4ss_mask_attn_loss_ex", (), {**kw, "pass": 0})
    assert _lib.bind("dl4ss_disc_adv_heads", ("s", 3), dict(lambda_=0.5, loss="l", dscore_dis="d", dscore_adv="a",
                                                             stream="st")) == ("s", 3, 0.5, "l", "d", "a", "st")
    renamed = {(e, p) for e, ps in _lib.PARAMS.items() for p in ps if p + "_" in _lib._SLOTS[e]}
    core = {(e, p) for e, p in renamed if e in CORE.params}
    assert {p for _, p in core} == {"pass", "lambda"} and len(core) == 5
    assert renamed - core == {("dl4ss_mask_attn_align_loss_ex", "pass")}  # (of the other headers)


# ---- a stubbed library: records what call / query hand it, touches nothing ----
def tag(t):
    """What the stubbed _lib.ptr returns: a tensor by its address (net.view makes a new tensor per call)."""
    return None if t is None else ("ptr", t.data_ptr() if isinstance(t, torch.Tensor) else id(t))


class FakeLib:
    def __init__(self, returns=()):
        self.calls, self.returns = [], dict(returns)

    def __getattr__(self, name):
        if not name.startswith("dl4ss_"):
            raise AttributeError(name)
        return lambda *args: (self.calls.append((name, args)), self.returns.get(name, 0))[1]


@pytest.fixture
def fake(monkeypatch):
    """A FakeLib; ``install()`` puts it, and the stubs of _lib.ptr and the stream, in place (after a trainer has
    been built against the real library's size queries)."""
    lib = FakeLib()

    def install():
        monkeypatch.setattr(_lib, "_lib", lib)
        monkeypatch.setattr(_lib, "ptr", lambda t, strided=False: tag(t))
        monkeypatch.setattr(_lib, "stream_ptr", lambda stream=None: "stream")

    lib.install = install
    return lib


def test_call_refuses_before_the_library_is_touched(fake):
    fake.install()
    with pytest.raises(TypeError, match="dl4ss_pit_select"):
        _lib.call("dl4ss_pit_select", None, 1, 1, 1, None)
    with pytest.raises(TypeError, match="dl4ss_attn_nblk"):
        _lib.query("dl4ss_attn_nblk", 1, 2, 3)
    assert fake.calls == []
    assert _lib.query("dl4ss_attn_nblk", T=5, F=7) == 0 and fake.calls == [("dl4ss_attn_nblk", (5, 7))]


# ---- constants ----
def test_ops_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "dl4ss_hip.h")).read()

    def header(name):
        m = re.search(r"\b" + name + r"\s*=?\s*(0x[0-9a-fA-F]+|\d+)", text)
        return int(m.group(1), 0)

    for n in ("COMPLEX", "MAG", "LOGMAG", "CONJ"):
        assert getattr(ops, "STFT_" + n) == header("DL4SS_STFT_" + n)
    assert (ops.STFT_COMPLEX, ops.STFT_MAG, ops.STFT_LOGMAG, ops.STFT_CONJ) == (1, 2, 4, 8)
    for n in ("NONE", "TANH", "TANH_BF16", "SPLIT_SLABS"):
        assert getattr(ops, "EPI_" + n) == header("DL4SS_EPI_" + n)
    assert (ops.EPI_NONE, ops.EPI_TANH, ops.EPI_TANH_BF16, ops.EPI_SPLIT_SLABS) == (0, 1, 2, 3)
    assert ops.WS_ZEROED == header("DL4SS_RNN_WS_ZEROED") == 0x100
    assert ops.DGH_PAD8 == header("DL4SS_RNN_DGH_PAD8") == 0x200
    assert ops.DEFER_BIAS == header("DL4SS_RNN_DEFER_BIAS") == 0x400
    assert ops.CELLS == {"lstm": header("DL4SS_CELL_LSTM"), "gru": header("DL4SS_CELL_GRU")} == {"lstm": 0, "gru": 1}
    assert ops.PREC == {"fp32": 0, "bf16": 1}
    # DL4SS_RNN_DOUT_SLABS(S) ((((S) - 1) & 3) << 12): a function-like macro, not parsed
    assert ops.DOUT_SLABS(3) == 2 << 12 and ops.DOUT_SLABS(3) & ~_lib.CONSTANTS["DL4SS_RNN_DOUT_SLABS_MASK"] == 0


# ---- the three environment reads the library retired ----
RETIRED = ("DL4SS_ATTN_TILES", "DL4SS_RNN_MAX_WG", "DL4SS_RNN_MIN_BC")


@pytest.fixture
def unloaded(monkeypatch):
    """_lib as before its first load, with ctypes.CDLL stubbed: _load() binds a stand-in with the core header's names
    alone, no shared object."""
    for name in RETIRED:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", __file__)  # (_load only asks whether the path exists: no built library)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: types.SimpleNamespace(
        hipGetErrorString=types.SimpleNamespace(), **{n: types.SimpleNamespace() for n in CORE.signatures}))


@pytest.mark.parametrize("name", RETIRED)
def test_retired_library_knobs_are_refused(unloaded, monkeypatch, name):
    net = engine.SepNet(cell="lstm", num_layers=1, hidden=40, device="cpu")
    assert name in plan.RETIRED_KNOBS
    plan.step_plan(net, 2, 2048, "fp32")  # unset: nothing raises
    lib = _lib._load()
    assert lib.dl4ss_attn_nblk.argtypes == [I, I] and _lib._load() is lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setenv(name, "2")
    with pytest.raises(ValueError, match=f"{name} is retired"):
        plan.step_plan(net, 2, 2048, "fp32")
    with pytest.raises(ValueError, match=f"{name} is retired"):
        _lib._load()
    assert _lib._lib is None


# ---- the converted call sites ----
def check(fake, entry, want):
    """The one recorded call of ``entry``: the prototype's length, every parameter as ``want`` names it (all of
    them: a parameter ``want`` lacks is a KeyError), and the slot kinds of the specification's SIGNATURES."""
    (name, args), = fake.calls
    params, sig = _lib.PARAMS[entry], SIGNATURES[entry]
    assert name == entry and len(args) == len(params) == len(sig)
    for p, a, kind in zip(params, args, sig):
        w = want[p]
        assert a == (tag(w) if isinstance(w, (torch.Tensor, Stand)) else w), (entry, p, a)
        if kind is F:
            assert type(a) is float, (entry, p, a)
        elif kind is P:
            assert a is None or not isinstance(a, (int, float)), (entry, p, a)
        else:
            assert type(a) is int, (entry, p, a)
    fake.calls.clear()


def _trainer(precision="fp32", mode="label", adv=False, **net):
    net = engine.SepNet(cell="lstm", num_layers=1, hidden=40, device="cpu", **net)
    kw = dict(adversary=engine.DiscNet(17, 129, device="cpu")) if adv else {}
    return engine.SepTrainer(net, 2, 2, 2048, mode=mode, precision=precision, **kw)  # T = 17 frames, F = 129


def _attn_common(tr, perm=None, pred=None):
    TF = tr.T * tr.F
    return dict(B=2, K=2, T=17, F=129, E=50, q=tr.q, X=tr.mag_mix, x_bstride=TF, Y=tr.mag_src, y_bstride=2 * TF,
                y_kstride=TF, perm=perm, s1=tr.s1, s2=tr.s2, part_loss=tr.part_loss, mask_out=None, pred_out=pred,
                stream="stream")


def test_attn_fp32_branch(fake):
    tr = _trainer("fp32")
    fake.install()
    tr.attn(0, pred_out=tr.mean)  # COST: no dPre, no dq partials
    check(fake, "dl4ss_mask_attn_loss_ex", dict(_attn_common(tr, pred=tr.mean), **{"pass": 0}, crm=0, V=tr.V, dPre=None,
                                                dPre_bf16=None, dpre_bf16_ld=0, part_dq=None))
    tr.attn(1, tr.perm)  # GRAD: dPre in place over V
    check(fake, "dl4ss_mask_attn_loss_ex", dict(_attn_common(tr, tr.perm), **{"pass": 1}, crm=0, V=tr.V, dPre=tr.V,
                                                dPre_bf16=None, dpre_bf16_ld=0, part_dq=tr.part_dq))


def test_attn_bf16_branch(fake):
    tr = _trainer("bf16", mode="pit")
    fake.install()
    assert tr.fast and not tr.split
    ld = tr.dPreb.stride(0)
    tr.attn(0)  # (the COST pass gets dPre_bf16 too)
    check(fake, "dl4ss_mask_attn_loss_bf16v", dict(_attn_common(tr), **{"pass": 0}, crm=0, V_bf16=tr.Vb, dPre=None,
                                                   dPre_bf16=tr.dPreb, dpre_bf16_ld=ld, part_dq=None))
    tr.attn(1, tr.perm)
    check(fake, "dl4ss_mask_attn_loss_bf16v", dict(_attn_common(tr, tr.perm), **{"pass": 1}, crm=0, V_bf16=tr.Vb,
                                                   dPre=None, dPre_bf16=tr.dPreb, dpre_bf16_ld=ld, part_dq=tr.part_dq))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_attn_adversarial_branch(fake, precision):
    tr = _trainer(precision, adv=True)
    fake.install()
    fast = precision == "bf16"
    tr.attn(1, gext=tr.adv.gext)
    want = dict(_attn_common(tr), dpred_extra=tr.adv.gext, dPre=None if fast else tr.V,
                dPre_bf16=tr.dPreb if fast else None, dpre_bf16_ld=tr.dPreb.stride(0) if fast else 0,
                part_dq=tr.part_dq)
    if fast:
        check(fake, "dl4ss_mask_attn_loss_adv_bf16v", dict(want, V_bf16=tr.Vb))
    else:
        check(fake, "dl4ss_mask_attn_loss_adv", dict(want, V=tr.V))


def test_attn_align_branch(fake):
    tr = _trainer("fp32", attention="align")
    fake.install()
    w = {n: tr.net.view(f"att.Linear_{i}.weight") for i, n in ((1, "W1"), (2, "W2"), (3, "w3"))}
    for pass_, grad in ((0, False), (1, True)):
        tr.attn(pass_, tr.perm if grad else None)
        check(fake, "dl4ss_mask_attn_align_loss", dict(
            _attn_common(tr, tr.perm if grad else None), **{"pass": pass_}, V=tr.V, **w,
            dPre=tr.V if grad else None, part=tr.part_att if grad else None, part_floats=tr.part_att.numel()))


class Stand:
    """Stands in for a CUDA tensor on the host: the wrappers read only its type, shape and strides."""
    is_cuda = True

    def __init__(self, shape, dtype=torch.float32, ld=None):
        self.shape, self.dtype = tuple(shape), dtype
        self._stride = (ld if ld is not None else self.shape[-1], 1) if len(self.shape) == 2 else (1,)
        self.device = "cuda"

    def dim(self):
        return len(self.shape)

    def stride(self, d):
        return self._stride[d]

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def is_contiguous(self):
        return True


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("clip", [False, True])
def test_adam_forms(fake, clip, shadow):
    fake.install()
    fake.returns["dl4ss_grad_sumsq_parts"] = 3
    p, g, m, v = (Stand((1000,)) for _ in range(4))
    status, loss, flag = Stand((2,), torch.int32), Stand((3,)), Stand((1,))
    part, gnorm, nonfinite = Stand((3,), torch.float64), Stand((2,)), Stand((1,), torch.int32)
    seg = (2, "off", "rows", "cols", "ys", "ldy")
    ops.adam_(p, g, m, v, 7, lr=1e-3, betas=(0.8, 0.9), eps=1e-6, status=status, loss=loss, dp_flag=flag, gscale=0.5,
              shadow=seg if shadow else None, clip=(part, 2.0, gnorm, nonfinite) if clip else None)
    fake.calls[:] = [c for c in fake.calls if c[0] != "dl4ss_grad_sumsq_parts"]
    want = dict(p=p, g=g, m=m, v=v, n=1000, lr=1e-3, beta1=0.8, beta2=0.9, eps=1e-6, step=7, status=status,
                dp_flag=flag, gscale=0.5, loss=loss, stream="stream")
    segs = dict(zip(("nseg", "seg_off", "seg_rows", "seg_cols", "seg_y", "seg_ldy"),
                    seg if shadow else (0, None, None, None, None, None)))
    if clip:
        check(fake, "dl4ss_adam_clipped", dict(want, **segs, part=part, n_part=3, max_norm=2.0, gnorm=gnorm,
                                               nonfinite=nonfinite))
    elif shadow:
        check(fake, "dl4ss_adam_guarded_dp_scaled_bf16", dict(want, **segs))
    else:
        check(fake, "dl4ss_adam_guarded_dp_scaled", want)


def test_gemm_bf16_gl(fake):
    fake.install()
    fake.returns["dl4ss_gemm_bf16_gl_ws_bytes"] = 4096
    A, B = Stand((24, 7), torch.bfloat16, ld=8), Stand((24, 40), torch.bfloat16)  # A stored (K, M): transA
    out, bias, ws = Stand((7, 40), ld=48), Stand((40,)), Stand((8192,), torch.uint8)
    ops.gemm_bf16_gl(A, B, transA=True, bias=bias, beta=0.5, out=out, splitk=2, ws=ws)
    assert fake.calls.pop(0) == ("dl4ss_gemm_bf16_gl_ws_bytes", (7, 40, 24, 2, 1))
    check(fake, "dl4ss_gemm_bf16_gl", dict(transA=1, transB=0, M=7, N=40, K=24, A=A, lda=8, B=B, ldb=40, C=out, ldc=48,
                                           bias=bias, epilogue=0, beta=0.5, splitk=2, batch=1, strideA=0, strideB=0,
                                           strideC=0, ws=ws, ws_bytes=8192, stream="stream"))
    # batched, explicit M / N / K and raw strides; no split: no workspace
    fake.returns["dl4ss_gemm_bf16_gl_ws_bytes"] = 0
    ops.gemm_bf16_gl(A, B, out=out, epilogue=ops.EPI_TANH, batch=2, strideA=96, strideB=480, strideC=168, M=3, N=40,
                     K=7)
    assert fake.calls.pop(0) == ("dl4ss_gemm_bf16_gl_ws_bytes", (3, 40, 7, 1, 2))
    check(fake, "dl4ss_gemm_bf16_gl", dict(transA=0, transB=0, M=3, N=40, K=7, A=A, lda=8, B=B, ldb=40, C=out, ldc=48,
                                           bias=None, epilogue=1, beta=0.0, splitk=1, batch=2, strideA=96, strideB=480,
                                           strideC=168, ws=None, ws_bytes=0, stream="stream"))


def test_grouped_gemm_and_finalize_sites(fake):
    """GroupedGemm.run's two forms share one keyword set; loss_and_grad's finalize calls name every slot."""
    tr = _trainer("fp32")
    fake.install()
    g = ops.GroupedGemm.__new__(ops.GroupedGemm)
    g.__dict__.update(_k0=[], n=2, ta=1, tb=0, grid=0, cfg=1, one_per_cu=0, rowsum=None, ws=Stand((64,), torch.uint8),
                      **{k: k.lower() + "s"
                         for k in ("M", "N", "K", "A", "lda", "B", "ldb", "C", "ldc", "beta", "splitk")})
    want = dict(n=2, transA=1, transB=0, M="ms", N="ns", K="ks", A="as", lda="ldas", B="bs", ldb="ldbs", C="cs",
                ldc="ldcs", beta="betas", splitk="splitks", ws=g.ws, ws_bytes=64, stream="stream")
    g.run()
    check(fake, "dl4ss_gemm_bf16_gl_grouped", want)
    g.grid, g.cfg, g.rowsum = 30, 2, "rowsums"
    g.run()
    check(fake, "dl4ss_gemm_bf16_gl_grouped_ex", dict(want, grid=30, cfg=2, one_per_cu=0, rowsum="rowsums"))
    tr.attn = lambda *a, **k: None
    tr.loss_and_grad()
    check(fake, "dl4ss_loss_finalize", dict(part_loss=tr.part_loss, B=2, K=2, nblk=tr.nblk, perm=None, s1=tr.s1,
                                            s2=tr.s2, loss_out=tr.loss, part_dq=tr.part_dq, qw=tr.net.W, dq=tr.dq,
                                            stream="stream"))
