"""ops.birnn_fwd / birnn_fwd_xw / birnn_bwd marshal their keywords into the positional slots the header and
_lib.SIGNATURES give the superset entry points (host only: _lib.call, _lib.ptr and the stream are stubbed, so no
library call is made).  A swapped out_bf16 / hprev_bf16 would be a silent wrong answer on the device."""
import ctypes
import os
import re

import pytest

from dl4ss_amd import _lib, ops

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dl4ss_hip.h")
# wrapper keyword -> parameter name in the header, where they differ
RENAMED = {"w_hh": "W_hh", "ws": "workspace", "x": "x_bf16", "w_ih": "W_ih_bf16"}


class Stand:
    """Stands in for a tensor: the stubbed _lib.ptr returns it tagged, the wrappers read only shape / stride."""

    def __init__(self, name):
        self.name, self.shape = name, (7, 24)

    def stride(self, dim):
        return (40, 1)[dim]


def header_params(entry):
    """Parameter names of ``entry``'s prototype in include/dl4ss_hip.h, in order."""
    text = open(HEADER).read()
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)\s*;", text)
    assert m, entry
    return [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: rec.append((name, args)))
    monkeypatch.setattr(_lib, "ptr", lambda t, strided=False: None if t is None else ("ptr", t.name))
    monkeypatch.setattr(_lib, "stream_ptr", lambda stream=None: "stream")
    return rec


def check(calls, entry, tensors, scalars):
    """One recorded call of ``entry``: every tensor keyword in its header slot, every other pointer slot None,
    the scalars where the header has them, and the arity and slot kinds of _lib.SIGNATURES."""
    (name, args), = calls
    params, sig = header_params(entry), _lib.SIGNATURES[entry]
    assert name == entry and len(args) == len(params) == len(sig)
    want = {RENAMED.get(k, k): ("ptr", k) for k in tensors}
    want.update(scalars, stream="stream")
    for p, a, kind in zip(params, args, sig):
        assert a == want.get(p), (entry, p, a)
        assert isinstance(a, int) == (kind in (ctypes.c_int, ctypes.c_longlong)), (entry, p, a, kind)


FWD = ("G", "w_hh", "b_hh", "act", "ws", "status", "out", "hprev", "cs", "out_bf16", "hprev_bf16", "h_mean")
XW = ("x", "w_ih", "b_ih") + FWD[1:]
BWD = ("w_hh", "act", "ws", "status", "dOut", "dOut_bcast", "cs", "hprev", "dG", "dGh", "dG_bf16", "dGh_bf16", "db_ih",
       "db_hh")
REQUIRED = {"G", "x", "w_ih", "b_ih", "w_hh", "b_hh", "act", "ws", "status"}


@pytest.mark.parametrize("cell,cid", [("lstm", 0), ("gru", 1)])
@pytest.mark.parametrize("full", [True, False])
def test_birnn_wrapper_slots(calls, cell, cid, full):
    """``full``: every tensor given; else only the required ones -- the absent ones must arrive as None."""
    dims = dict(cell=cid, B=3, T=5, H=11, ws_bytes=4096)

    def kw(names):
        return {k: Stand(k) for k in names if full or k in REQUIRED}

    t = kw(FWD)
    ops.birnn_fwd(cell, 3, 5, 11, ws_bytes=4096, precision="bf16", flags=ops.WS_ZEROED, **t)
    check(calls, "dl4ss_birnn_fwd_mean", t, dict(dims, precision=1 | 0x100))
    calls.clear()
    t = kw(XW)
    ops.birnn_fwd_xw(cell, 3, 5, 11, ws_bytes=4096, **t)
    check(calls, "dl4ss_birnn_fwd_xw_ex", t, dict(dims, Kin=24, ldx=40, ldw=40, ws_zeroed=1))
    calls.clear()
    t = kw(BWD)
    flags = ops.WS_ZEROED | ops.DEFER_BIAS | ops.DGH_PAD8 | ops.DOUT_SLABS(3)
    ops.birnn_bwd(cell, 3, 5, 11, ws_bytes=4096, precision="bf16", flags=flags, **t)
    check(calls, "dl4ss_birnn_bwd_ex", t, dict(dims, precision=1 | 0x100 | 0x400 | 0x200 | (2 << 12)))
    calls.clear()
    ops.birnn_bwd(cell, 3, 5, 11, ws_bytes=4096, **t)  # the defaults: fp32, no flag
    check(calls, "dl4ss_birnn_bwd_ex", t, dict(dims, precision=0))
