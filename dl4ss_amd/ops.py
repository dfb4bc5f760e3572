"""Torch-tensor wrappers over the C ABI (device memory / streams are torch's).  The ABI's constants (STFT_*, EPI_*,
PREC, CELLS, the recurrence flags) take their values from the header through ``_lib.CONSTANTS``; a call to an entry
point of ten or more parameters names every one of them (``_lib.bind`` puts them in the prototype's order).

Each wrapper validates shapes on the host (so a kernel never sees a shape it
does not assume), allocates outputs with torch and enqueues exactly one C-ABI
call on the current stream.
"""
import torch

from . import _lib

_C = _lib.CONSTANTS  # the enums and flag macros of the public headers
STFT_COMPLEX, STFT_MAG, STFT_LOGMAG, STFT_CONJ = (_C["DL4SS_STFT_" + n] for n in ("COMPLEX", "MAG", "LOGMAG", "CONJ"))
N_FFT, HOP = 256, 128
F_BINS = N_FFT // 2 + 1


def n_frames(n_samples):
    return 1 + n_samples // HOP


def _f32c(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"{name}: expected a contiguous float32 CUDA tensor")
    return t


def stft(x, complex_out=True, mag_out=True, log=False, conj=False, out_c=None, out_mag=None, out_bf16=None,
         n_bf16=0):
    """x (..., N) fp32 -> (X (..., T, F, 2) fp32 [re,im], mag (..., T, F) fp32).

    librosa stft(n_fft=256, hop=128) restated (periodic Hann, centre/reflect).
    ``log`` writes log(|X| + eps) into the magnitude output instead.  ``out_bf16`` (rows sig * T + t,
    row stride >= F): bf16 copies of the magnitudes of the first ``n_bf16`` signals, written by the
    same launch (dl4ss_stft_fwd_ex; columns >= F untouched).
    """
    _f32c(x, "stft")
    N = x.shape[-1]
    lead = x.shape[:-1]
    n_sig = x.numel() // N
    T = n_frames(N)
    flags = (STFT_COMPLEX if complex_out else 0) | ((STFT_LOGMAG if log else STFT_MAG) if mag_out else 0)
    flags |= STFT_CONJ if conj else 0
    if complex_out and out_c is None:
        out_c = torch.empty(*lead, T, F_BINS, 2, device=x.device, dtype=torch.float32)
    if mag_out and out_mag is None:
        out_mag = torch.empty(*lead, T, F_BINS, device=x.device, dtype=torch.float32)
    if out_bf16 is not None:
        if not mag_out or out_bf16.dtype != torch.bfloat16 or out_bf16.stride(-1) != 1 or \
                out_bf16.shape[0] < n_bf16 * T or out_bf16.stride(0) < F_BINS or n_bf16 > n_sig:
            raise RuntimeError("stft: out_bf16 must be bf16 rows (>= n_bf16 * T, row stride >= 129) of a magnitude")
        _lib.call("dl4ss_stft_fwd_ex", x=_lib.ptr(x), n_sig=n_sig, n_samples=N, n_fft=N_FFT, hop=HOP, flags=flags,
                  X_c64=_lib.ptr(out_c) if complex_out else None, mag=_lib.ptr(out_mag), mag_bf16=_lib.ptr(out_bf16),
                  ld_bf16=out_bf16.stride(0), n_sig_bf16=n_bf16, stream=_lib.stream_ptr())
        return out_c, out_mag
    _lib.call("dl4ss_stft_fwd", _lib.ptr(x), n_sig, N, N_FFT, HOP, flags, _lib.ptr(out_c) if complex_out else None,
              _lib.ptr(out_mag) if mag_out else None, _lib.stream_ptr())
    return out_c, out_mag


def istft(S, conj=False, out=None):
    """S (..., T, F, 2) fp32 -> y (..., 128*(T-1)) fp32 (librosa istft restated)."""
    _f32c(S, "istft")
    if S.shape[-1] != 2 or S.shape[-2] != F_BINS:
        raise RuntimeError("istft: expected (..., T, 129, 2)")
    T = S.shape[-3]
    lead = S.shape[:-3]
    n_sig = S.numel() // (T * F_BINS * 2)
    L = HOP * (T - 1)
    if out is None:
        out = torch.empty(*lead, L, device=S.device, dtype=torch.float32)
    _lib.call("dl4ss_istft", _lib.ptr(S), n_sig, T, N_FFT, HOP, STFT_CONJ if conj else 0, _lib.ptr(out),
              _lib.stream_ptr())
    return out


def mix_sources(raw, gains, out_src=None, out_mix=None, stats_ws=None, lengths=None, shifts=None):
    """raw (B, K, N) fp32 sources, gains (B, K) fp32 -> (scaled sources (B, K, N),
    mixture (B, N)) -- normalise, gain, sum.  lengths (B, K) int32: each
    source's own length (normalised over it, zero beyond; list-file wavs).  shifts (B, K)
    int32: the AUGMENT_DATA rotation np.append(x[s:], x[:s]) over the source's own length,
    after the normalisation (TDAA_beta/predata_fromList_cRM_123.py:198-200)."""
    _f32c(raw, "mix_sources")
    _f32c(gains, "mix_sources(gains)")
    B, K, N = raw.shape
    if tuple(gains.shape) != (B, K):
        raise RuntimeError("mix_sources: gains must be (B, K)")
    if out_src is None:
        out_src = torch.empty(B, K, N, device=raw.device, dtype=torch.float32)
    if out_mix is None:
        out_mix = torch.empty(B, N, device=raw.device, dtype=torch.float32)
    if stats_ws is None:
        stats_ws = torch.empty(B * K * 32, device=raw.device, dtype=torch.float32)
    if lengths is not None and (lengths.dtype != torch.int32 or tuple(lengths.shape) != (B, K)):
        raise RuntimeError("mix_sources: lengths must be (B, K) int32")
    if shifts is not None and (shifts.dtype != torch.int32 or tuple(shifts.shape) != (B, K) or not shifts.is_cuda
                               or not shifts.is_contiguous()):
        raise RuntimeError("mix_sources: shifts must be a contiguous (B, K) int32 CUDA tensor")
    _lib.call("dl4ss_mix_sources_rot", raw=_lib.ptr(raw), lengths=_lib.ptr(lengths), shifts=_lib.ptr(shifts),
              gains=_lib.ptr(gains), B=B, K=K, N=N, stats_ws=_lib.ptr(stats_ws), out_src=_lib.ptr(out_src),
              out_mix=_lib.ptr(out_mix), stream=_lib.stream_ptr())
    return out_src, out_mix


# ---------------------------------------------------------------------------
# device-resident corpus (include/corpus/dl4ss_corpus.h, libdl4ss_corpus.so; dl4ss_amd.corpus builds the pool)
# ---------------------------------------------------------------------------
CORPUS_DTYPES = {torch.int16: _lib.EXT_CONSTANTS["DL4SS_CORPUS_I16"],
                 torch.float32: _lib.EXT_CONSTANTS["DL4SS_CORPUS_F32"]}
MAX_MIX_SOURCES = 16  # K <= Ks <= 16, as dl4ss_mix_sources' K


def _corpus_tables(name, pool, offsets, lengths):
    """The pool and its tables as the kernels take them; -> n_clips."""
    if not (pool.is_cuda and pool.dim() == 1 and pool.is_contiguous() and pool.dtype in CORPUS_DTYPES):
        raise RuntimeError(f"{name}: pool must be a flat contiguous int16 or float32 CUDA tensor")
    if pool.data_ptr() % 16:
        raise RuntimeError(f"{name}: pool must be 16-B aligned")
    n = offsets.numel()
    for t, dt, what in ((offsets, torch.int64, "offsets"), (lengths, torch.int32, "lengths")):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == (n,)):
            raise RuntimeError(f"{name}: {what} must be a contiguous (n_clips,) {dt} CUDA tensor")
    return n


def corpus_stats(pool, offsets, lengths, out=None, ws=None):
    """Per-clip {mean, 1 / max|x - mean|} (n_clips, 2) fp32 of a corpus pool, once per corpus: the statistics
    mix_sources computes every step, with its arithmetic (dl4ss_corpus_stats)."""
    n = _corpus_tables("corpus_stats", pool, offsets, lengths)
    if out is None:
        out = torch.empty(n, 2, device=pool.device, dtype=torch.float32)
    if ws is None:
        ws = torch.empty(max(1, 32 * n), device=pool.device, dtype=torch.float32)
    _f32c(out, "corpus_stats(out)")
    _f32c(ws, "corpus_stats(ws)")
    if tuple(out.shape) != (n, 2) or ws.numel() < 32 * n:
        raise RuntimeError("corpus_stats: out must be (n_clips, 2) and ws hold 32 n_clips floats")
    _lib.call("dl4ss_corpus_stats", pool=_lib.ptr(pool), dtype=CORPUS_DTYPES[pool.dtype], offsets=_lib.ptr(offsets),
              lengths=_lib.ptr(lengths), n_clips=n, ws=_lib.ptr(ws), clip_stats=_lib.ptr(out),
              stream=_lib.stream_ptr())
    return out


def mix_corpus(pool, offsets, lengths, clip_stats, clips, gains, K, N, shifts=None, max_len=None, out_src=None,
               out_mix=None, out_len=None, bad=None):
    """One step's batch from a device-resident corpus in one launch (dl4ss_mix_corpus): clips, gains, shifts
    (B, Ks) int32 / fp32 / int32 CUDA tensors name each source's clip, gain and rotation; sources 0..K-1 ->
    out_src (B, K, N), all Ks summed -> out_mix (B, N), the values mix_sources gives for the gathered clips.
    ``max_len``: the corpus's crop length; N below it is refused (the statistics are over the stored crop).
    ``bad`` (1,) int32: goes up by one per source whose clip id is outside the corpus (that source is silent); a
    fresh zeroed one unless given.  -> (out_src, out_mix, bad)."""
    if max_len is not None and N < max_len:
        raise ValueError(f"mix_corpus: N = {N} is below the corpus's max_len = {max_len} (the clip statistics are "
                         "over the stored crop)")
    n = _corpus_tables("mix_corpus", pool, offsets, lengths)
    _f32c(clip_stats, "mix_corpus(clip_stats)")
    _f32c(gains, "mix_corpus(gains)")
    if tuple(clip_stats.shape) != (n, 2) or n < 1:
        raise RuntimeError("mix_corpus: clip_stats must be (n_clips, 2), n_clips >= 1")
    if clips.dim() != 2:
        raise RuntimeError("mix_corpus: clips must be (B, Ks)")
    B, Ks = clips.shape
    if not (1 <= K <= Ks <= MAX_MIX_SOURCES) or N < 1 or B > 65535:
        raise RuntimeError(f"mix_corpus: needs 1 <= K <= Ks <= {MAX_MIX_SOURCES}, N >= 1, B <= 65535 "
                           f"(K {K}, Ks {Ks}, N {N}, B {B})")
    for t, what in ((clips, "clips"), (shifts, "shifts")):
        if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
                                  and tuple(t.shape) == (B, Ks)):
            raise RuntimeError(f"mix_corpus: {what} must be a contiguous (B, Ks) int32 CUDA tensor")
    if tuple(gains.shape) != (B, Ks):
        raise RuntimeError("mix_corpus: gains must be (B, Ks)")
    dev = pool.device
    if out_src is None:
        out_src = torch.empty(B, K, N, device=dev, dtype=torch.float32)
    if out_mix is None:
        out_mix = torch.empty(B, N, device=dev, dtype=torch.float32)
    if bad is None:
        bad = torch.zeros(1, device=dev, dtype=torch.int32)
    _f32c(out_src, "mix_corpus(out_src)")
    _f32c(out_mix, "mix_corpus(out_mix)")
    if tuple(out_src.shape) != (B, K, N) or tuple(out_mix.shape) != (B, N):
        raise RuntimeError("mix_corpus: out_src must be (B, K, N) and out_mix (B, N)")
    if out_len is not None and not (out_len.is_cuda and out_len.dtype == torch.int32 and out_len.is_contiguous()
                                    and tuple(out_len.shape) == (B, Ks)):
        raise RuntimeError("mix_corpus: out_len must be a contiguous (B, Ks) int32 CUDA tensor")
    if not (bad.is_cuda and bad.dtype == torch.int32 and bad.numel() >= 1):
        raise RuntimeError("mix_corpus: bad must be an int32 CUDA tensor")
    _lib.call("dl4ss_mix_corpus", pool=_lib.ptr(pool), dtype=CORPUS_DTYPES[pool.dtype], offsets=_lib.ptr(offsets),
              lengths=_lib.ptr(lengths), clip_stats=_lib.ptr(clip_stats), n_clips=n, clips=_lib.ptr(clips),
              shifts=_lib.ptr(shifts), gains=_lib.ptr(gains), B=B, K=K, Ks=Ks, N=N, out_src=_lib.ptr(out_src),
              out_mix=_lib.ptr(out_mix), out_len=_lib.ptr(out_len), bad=_lib.ptr(bad), stream=_lib.stream_ptr())
    return out_src, out_mix, bad


# ---------------------------------------------------------------------------
# dense contractions
# ---------------------------------------------------------------------------
PREC = {"fp32": _C["DL4SS_PREC_F32"], "bf16": _C["DL4SS_PREC_BF16"]}
# EPI_TANH_BF16: tanh written as bf16 (gemm_bf16_gl only).  EPI_SPLIT_SLABS, gemm_bf16_gl split-K only: leave the
# fp32 slabs in ws for their consumer (no combine, out not written)
EPI_NONE, EPI_TANH, EPI_TANH_BF16, EPI_SPLIT_SLABS = (_C["DL4SS_EPI_" + n]
                                                      for n in ("NONE", "TANH", "TANH_BF16", "SPLIT_SLABS"))


def _mat(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1):
        raise RuntimeError(f"{name}: expected a 2-D row-major float32 CUDA matrix (unit inner stride)")
    return t


def auto_splitk(M, N, K, target_wgs=1024, min_k=512):
    """Split-K factor that gives a short-and-wide GEMM ~target_wgs workgroups (128 x 128
    tiles) while keeping >= min_k of K per split."""
    tiles = -(-M // 128) * -(-N // 128)
    s = max(1, min(-(-target_wgs // tiles), K // min_k))
    return int(s)


_fixed_ws = {}


def _fixed_workspace(dev, nbytes):
    """split-K slab workspace of dl4ss_gemm_fixed, one per device and stream, grown on demand
    (never inside a graph capture: an eager call sizes it first, or the caller passes its own)"""
    key = (dev, torch.cuda.current_stream().cuda_stream)
    ws = _fixed_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("gemm(reduce='fixed'): split-K workspace must be sized before graph capture")
        ws = _fixed_ws[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
    return ws


def gemm_fixed_ws_bytes(M, N, K, splitk):
    """Bytes of split-K workspace gemm(reduce="fixed") needs for this shape and factor (an int or "auto");
    0 when the effective split is 1."""
    if splitk == "auto":
        splitk = auto_splitk(M, N, K)
    nb = int(_lib.query("dl4ss_gemm_fixed_ws_bytes", int(M), int(N), int(K), int(splitk)))
    if nb < 0:
        raise RuntimeError(f"gemm_fixed_ws_bytes: bad shape {(M, N, K)}")
    return nb


def gemm(A, B, transA=False, transB=False, bias=None, epilogue=EPI_NONE, beta=0.0, out=None, precision="fp32",
         splitk=1, reduce="atomic", ws=None):
    """out = op(A) @ op(B) (+ bias) (tanh) (+ beta*out).  op(A) = A.T if transA.

    A is stored (M, K) or (K, M) if transA; B is stored (K, N) or (N, K) if transB.
    splitk="auto": split K over workgroups (fp32 atomics) when the tile grid is small
    (needs epilogue none; a beta = 0 output is zeroed first).
    reduce="fixed" (fp32): the split's partial tiles go to fp32 slabs that a second launch adds in a fixed
    order (dl4ss_gemm_fixed): any beta, out neither zeroed nor read when beta = 0, the same bits on every call.
    ws: the caller's slab workspace (a uint8 or float tensor of gemm_fixed_ws_bytes), else a per-device/stream
    one grown on demand.
    """
    if reduce not in ("atomic", "fixed"):
        raise ValueError(f"gemm: reduce {reduce!r}, expected 'atomic' or 'fixed'")
    if reduce == "atomic" and ws is not None:
        raise ValueError("gemm: ws belongs to reduce='fixed'")
    _mat(A, "gemm(A)")
    _mat(B, "gemm(B)")
    M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    Kb, N = (B.shape[1], B.shape[0]) if transB else (B.shape[0], B.shape[1])
    if K != Kb:
        raise RuntimeError(f"gemm: inner dims differ ({K} vs {Kb})")
    if out is None:
        if beta != 0.0 or (reduce == "atomic" and splitk > 1):
            raise RuntimeError("gemm: accumulation needs an output tensor")
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    _mat(out, "gemm(out)")
    if tuple(out.shape) != (M, N):
        raise RuntimeError(f"gemm: out shape {tuple(out.shape)} != {(M, N)}")
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise RuntimeError("gemm: bias must be contiguous with N elements")
    if reduce == "fixed":
        return _gemm_fixed(A, B, transA, transB, M, N, K, bias, epilogue, beta, out, precision, splitk, ws)
    if splitk == "auto":
        splitk = auto_splitk(M, N, K) if epilogue == EPI_NONE else 1
        if splitk > 1 and beta == 0.0:
            out.zero_()
            beta = 1.0
        elif splitk > 1 and beta != 1.0:
            splitk = 1
    _lib.call("dl4ss_gemm", transA=int(transA), transB=int(transB), M=M, N=N, K=K, A=_lib.ptr(A, True), lda=A.stride(0),
              B=_lib.ptr(B, True), ldb=B.stride(0), C=_lib.ptr(out, True), ldc=out.stride(0), bias=_lib.ptr(bias),
              epilogue=epilogue, beta=float(beta), precision=PREC[precision], splitk=int(splitk),
              stream=_lib.stream_ptr())
    return out


def _gemm_fixed(A, B, transA, transB, M, N, K, bias, epilogue, beta, out, precision, splitk, ws):
    """gemm(reduce="fixed") behind gemm()'s shape checks: every refusal on the host, then dl4ss_gemm_fixed."""
    if splitk == "auto":  # whatever beta is: the combine applies it, out is not pre-zeroed
        splitk = auto_splitk(M, N, K) if epilogue == EPI_NONE else 1
    splitk = int(splitk)
    nb = gemm_fixed_ws_bytes(M, N, K, splitk)
    if nb > 0:  # the effective split is > 1
        if epilogue != EPI_NONE:
            raise RuntimeError("gemm(reduce='fixed'): a split needs epilogue none")
        if precision != "fp32":
            raise RuntimeError(f"gemm(reduce='fixed'): a split is fp32 only, not precision {precision!r}")
        if ws is not None:
            if not (ws.is_cuda and ws.is_contiguous() and ws.dtype in (torch.uint8, torch.float32)):
                raise RuntimeError("gemm(reduce='fixed'): ws must be a contiguous uint8 or float32 CUDA tensor")
            if ws.numel() * ws.element_size() < nb:
                raise RuntimeError(f"gemm(reduce='fixed'): workspace of {ws.numel() * ws.element_size()} bytes < {nb}")
        else:
            ws = _fixed_workspace(A.device, nb)
    else:
        ws = None
    _lib.call("dl4ss_gemm_fixed", transA=int(transA), transB=int(transB), M=M, N=N, K=K, A=_lib.ptr(A, True),
              lda=A.stride(0), B=_lib.ptr(B, True), ldb=B.stride(0), C=_lib.ptr(out, True), ldc=out.stride(0),
              bias=_lib.ptr(bias), epilogue=epilogue, beta=float(beta), precision=PREC[precision], splitk=splitk,
              ws=_lib.ptr(ws), ws_bytes=ws.numel() * ws.element_size() if ws is not None else 0,
              stream=_lib.stream_ptr())
    return out


GEMM_GL_TARGET_WGS = 512  # gemm_gl (2 workgroups per CU): split-K to about two per CU


def _mat_bf16(t, name):
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1):
        raise RuntimeError(f"{name}: expected a 2-D row-major bfloat16 CUDA matrix (unit inner stride)")
    return t


_gl_ws = {}


def _gl_workspace(dev, nbytes):
    """split-K slab workspace of dl4ss_gemm_bf16_gl, one per device and stream, grown on demand
    (never inside a graph capture: the eager warm-up step sizes it)"""
    key = (dev, torch.cuda.current_stream().cuda_stream)
    ws = _gl_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("gemm_bf16_gl: split-K workspace must be sized before graph capture")
        ws = _gl_ws[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
    return ws


def gemm_bf16_gl(A, B, transA=False, transB=False, bias=None, epilogue=EPI_NONE, beta=0.0, out=None, splitk=1,
                 batch=1, strideA=0, strideB=0, strideC=0, M=None, N=None, K=None, ws=None):
    """out (fp32, or bf16 with EPI_TANH_BF16) = op(A) @ op(B) (+ bias) (epilogue) (+ beta*out)
    with bf16 A and B through the LDS-DMA MFMA kernel (dl4ss_gemm_bf16_gl, gemm_gl.hip).
    Layout conventions as gemm(); split-K is deterministic (fp32 slabs + fixed-order
    reduce); batch > 1 takes raw element strides from the first-member views.  ws: the
    caller's split-K workspace (a uint8 tensor), else a per-device/stream one grown on demand."""
    _mat_bf16(A, "gemm_bf16_gl(A)")
    _mat_bf16(B, "gemm_bf16_gl(B)")
    if M is None:
        M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
        Kb, N = (B.shape[1], B.shape[0]) if transB else (B.shape[0], B.shape[1])
        if K != Kb:
            raise RuntimeError(f"gemm_bf16_gl: inner dims differ ({K} vs {Kb})")
    if out is None:
        if beta != 0.0:
            raise RuntimeError("gemm_bf16_gl: accumulation needs an output tensor")
        out = torch.empty(M, N, device=A.device,
                          dtype=torch.bfloat16 if epilogue == EPI_TANH_BF16 else torch.float32)
    if epilogue == EPI_TANH_BF16:
        _mat_bf16(out, "gemm_bf16_gl(out, bf16 epilogue)")
    else:
        _mat(out, "gemm_bf16_gl(out)")
    if batch == 1 and tuple(out.shape) != (M, N):
        raise RuntimeError(f"gemm_bf16_gl: out shape {tuple(out.shape)} != {(M, N)}")
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise RuntimeError("gemm_bf16_gl: bias must be contiguous with N elements")
    if splitk == "auto":
        splitk = auto_splitk(M, N, K, target_wgs=max(1, GEMM_GL_TARGET_WGS // batch)) if epilogue == EPI_NONE else 1
    nb = _lib.query("dl4ss_gemm_bf16_gl_ws_bytes", M, N, K, int(splitk), int(batch))
    if nb > 0 and ws is not None and ws.numel() < nb:
        raise RuntimeError(f"gemm_bf16_gl: workspace of {ws.numel()} bytes < {nb}")
    ws = (ws if ws is not None else _gl_workspace(A.device, nb)) if nb > 0 else None
    _lib.call("dl4ss_gemm_bf16_gl", transA=int(transA), transB=int(transB), M=M, N=N, K=K, A=_lib.ptr(A, True),
              lda=A.stride(0), B=_lib.ptr(B, True), ldb=B.stride(0), C=_lib.ptr(out, True), ldc=out.stride(0),
              bias=_lib.ptr(bias), epilogue=epilogue, beta=float(beta), splitk=int(splitk), batch=int(batch),
              strideA=int(strideA), strideB=int(strideB), strideC=int(strideC), ws=_lib.ptr(ws),
              ws_bytes=ws.numel() if ws is not None else 0, stream=_lib.stream_ptr())
    return out


class GroupedGemm:
    """A fixed list of bf16 GEMM problems C_i = op(A_i) @ op(B_i) + beta_i C_i run as ONE grouped
    launch (dl4ss_gemm_bf16_gl_grouped; + one split-K combine launch).  Each problem is a dict
    with A, B (bf16 views, 16-B aligned rows), out (fp32 view), transA, transB, beta, splitk and
    optionally M, N, K (else from the shapes).  The argument arrays are built once: the tensors
    must stay alive (and at the same addresses) for as long as run() is called."""

    def __init__(self, problems, device, grid=0, cfg=1, one_per_cu=False):
        """grid > 0: the persistent form (dl4ss_gemm_bf16_gl_grouped_ex): ``grid`` workgroups walk the
        tiles, in tile configuration ``cfg`` (1: 128 x 128, 2: 256 x 128 one per CU); one_per_cu pads
        cfg 1 to one workgroup per CU."""
        import ctypes
        self.grid, self.cfg, self.one_per_cu = int(grid), int(cfg), int(bool(one_per_cu))
        if not 1 <= len(problems) <= 16:
            raise RuntimeError("GroupedGemm: 1..16 problems")
        ta, tb = int(problems[0]["transA"]), int(problems[0]["transB"])
        dims, self._keep, kept = [], [], []
        self._k0 = []  # K = 0 problems with beta != 1: C = beta C, applied by run()
        for p in problems:
            A, B, out = p["A"], p["B"], p["out"]
            _mat_bf16(A, "GroupedGemm(A)")
            _mat_bf16(B, "GroupedGemm(B)")
            _mat(out, "GroupedGemm(out)")
            if int(p["transA"]) != ta or int(p["transB"]) != tb:
                raise RuntimeError("GroupedGemm: every problem needs the same transA / transB")
            M, K = (A.shape[1], A.shape[0]) if ta else (A.shape[0], A.shape[1])
            Kb, N = (B.shape[1], B.shape[0]) if tb else (B.shape[0], B.shape[1])
            shapeA, shapeB = (M, K), (Kb, N)
            M, N, K = p.get("M", M), p.get("N", N), p.get("K", K)
            if p.get("K") is None and K != Kb:
                raise RuntimeError(f"GroupedGemm: inner dims differ ({K} vs {Kb})")
            if not any(x in p for x in ("M", "N", "K")):
                if tuple(out.shape) != (M, N):
                    raise RuntimeError(f"GroupedGemm: out shape {tuple(out.shape)} != {(M, N)}")
            # explicit M / N / K: the kernel and its combine must stay inside every view
            # (the argument arrays are frozen here, so a wrong view would be written past silently)
            if not (0 <= M <= shapeA[0] and 0 <= K <= shapeA[1] and K <= shapeB[0] and 0 <= N <= shapeB[1]):
                raise RuntimeError(f"GroupedGemm: M, N, K = {(M, N, K)} exceed the operand views")
            if not (out.shape[0] >= M and out.shape[1] >= N and (N == 0 or out.stride(0) >= N)):
                raise RuntimeError(f"GroupedGemm: out view {tuple(out.shape)} (ldc {out.stride(0)}) < {(M, N)}")
            # empty problems (an empty batch: M or N = 0, or K = 0) launch nothing: no output, or
            # C = beta C with an empty sum
            if M == 0 or N == 0:
                continue
            if K == 0:
                if float(p.get("beta", 0.0)) != 1.0:
                    self._k0.append((out[:M, :N], float(p.get("beta", 0.0))))
                continue
            dims.append((M, N, K))
            kept.append(p)
            self._keep += [A, B, out]
        problems = kept
        n = len(problems)
        self.n = n
        if n == 0:
            return
        Iv = lambda xs: (ctypes.c_int * n)(*xs)
        Lv = lambda xs: (ctypes.c_longlong * n)(*xs)
        Pv = lambda xs: (ctypes.c_void_p * n)(*xs)
        self.n, self.ta, self.tb = n, ta, tb
        self.M, self.N, self.K = Iv([d[0] for d in dims]), Iv([d[1] for d in dims]), Iv([d[2] for d in dims])
        self.A = Pv([p["A"].data_ptr() for p in problems])
        self.lda = Lv([p["A"].stride(0) for p in problems])
        self.B = Pv([p["B"].data_ptr() for p in problems])
        self.ldb = Lv([p["B"].stride(0) for p in problems])
        self.C = Pv([p["out"].data_ptr() for p in problems])
        self.ldc = Lv([p["out"].stride(0) for p in problems])
        self.beta = (ctypes.c_float * n)(*[float(p.get("beta", 0.0)) for p in problems])
        self.splitk = Iv([int(p.get("splitk", 1)) for p in problems])
        # optional per-problem row sums of op(A) ("rowsum": an M-float view; persistent form only)
        rs = [p.get("rowsum") for p in problems]
        for r, (M, _, _), p in zip(rs, dims, problems):
            if r is not None:
                _f32c(r, "GroupedGemm(rowsum)")
                if r.numel() < M or int(p.get("splitk", 1)) != 1 or not (p["transA"] and not p["transB"]):
                    raise RuntimeError("GroupedGemm: rowsum needs M floats, an unsplit problem, transA and not transB")
                self._keep.append(r)
        self.rowsum = Pv([r.data_ptr() if r is not None else None for r in rs]) if any(r is not None for r in rs) \
            else None
        nb = _lib.query("dl4ss_gemm_bf16_gl_grouped_ws_bytes", n, self.M, self.N, self.K, self.splitk)
        if nb < 0:
            raise RuntimeError("GroupedGemm: bad problem list")
        self.ws = torch.empty(max(int(nb), 1), device=device, dtype=torch.uint8)

    def run(self):
        for c, beta in self._k0:
            c.zero_() if beta == 0.0 else c.mul_(beta)  # beta 0: C is not read (stale NaN included)
        if self.n == 0:
            return
        group = dict(n=self.n, transA=self.ta, transB=self.tb, M=self.M, N=self.N, K=self.K, A=self.A, lda=self.lda,
                     B=self.B, ldb=self.ldb, C=self.C, ldc=self.ldc, beta=self.beta, splitk=self.splitk,
                     ws=_lib.ptr(self.ws), ws_bytes=self.ws.numel(), stream=_lib.stream_ptr())
        if self.grid > 0 or self.cfg != 1 or self.rowsum is not None:
            _lib.call("dl4ss_gemm_bf16_gl_grouped_ex", grid=self.grid, cfg=self.cfg, one_per_cu=self.one_per_cu,
                      rowsum=self.rowsum, **group)
            return
        _lib.call("dl4ss_gemm_bf16_gl_grouped", **group)


def to_bf16(x, out=None):
    """bf16 copy (round to nearest even) of a contiguous fp32 CUDA tensor."""
    _f32c(x, "to_bf16")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    if out.dtype != torch.bfloat16 or not out.is_contiguous() or out.numel() != x.numel():
        raise RuntimeError("to_bf16: out must be a contiguous bfloat16 tensor of the same size")
    _lib.call("dl4ss_f32_to_bf16", _lib.ptr(x), _lib.ptr(out), x.numel(), _lib.stream_ptr())
    return out


def colsum(A, out):
    """out += A.sum(0) for a row-major matrix view A (M, N)."""
    _mat(A, "colsum")
    _lib.call("dl4ss_colsum", _lib.ptr(A, True), A.stride(0), A.shape[0], A.shape[1], _lib.ptr(out), _lib.stream_ptr())
    return out


def grad_sumsq_parts(n):
    """The number of fp64 partials grad_sumsq writes for n elements (1 .. 1024, a function of n alone)."""
    return int(_lib.query("dl4ss_grad_sumsq_parts", int(n)))


def grad_sumsq(g, part=None):
    """part[j] = the fp64 sum of squares of the j-th fixed contiguous range of the flat fp32 gradient g
    (grad_sumsq_parts(g.numel()) ranges; a fixed order, bitwise reproducible).  part.sum() is ||g||^2; the
    clipped adam_ sums the partials itself."""
    _f32c(g, "grad_sumsq")
    n_part = grad_sumsq_parts(g.numel())
    if part is None:
        part = torch.empty(n_part, device=g.device, dtype=torch.float64)
    if part.dtype != torch.float64 or part.numel() < n_part:
        raise ValueError(f"grad_sumsq: part must hold {n_part} float64 values")
    _lib.call("dl4ss_grad_sumsq", _lib.ptr(g), g.numel(), _lib.ptr(part), _lib.stream_ptr())
    return part


def check_clip_norm(x, name="clip_norm"):
    """A clipping threshold as a float: positive (+inf allowed: measure and guard only), not NaN."""
    x = float(x)
    if not x > 0.0:  # also NaN
        raise ValueError(f"{name} must be positive (inf allowed), got {x}")
    return x


CLIP_TORCH, CLIP_KERAS = (_C[k] for k in ("DL4SS_CLIP_TORCH", "DL4SS_CLIP_KERAS"))
CLIP_MAX_PARTS = _C["DL4SS_CLIP_MAX_PARTS"]
STATUS_NONFINITE_GRAD = _C["DL4SS_STATUS_NONFINITE_GRAD"]  # the sticky bit of status[0]


def _clip_args(clip, n, name, n_part=None):
    """(part, n_part, max_norm, gnorm, nonfinite) of a ``clip`` tuple, checked.  ``n_part`` None: part holds
    grad_sumsq's partials of the n-element gradient; a number: part's first n_part values, whatever wrote them."""
    part, max_norm, gnorm, nonfinite = clip
    max_norm = check_clip_norm(max_norm, f"{name}: max_norm")
    if n_part is None:
        n_part = grad_sumsq_parts(n)
    elif not 1 <= int(n_part) <= CLIP_MAX_PARTS:
        raise ValueError(f"{name}: 1 <= n_part <= {CLIP_MAX_PARTS}")
    if part.dtype != torch.float64 or part.numel() < n_part:
        raise ValueError(f"{name}: clip needs the {n_part} float64 partials of grad_sumsq")
    if gnorm is not None and (gnorm.dtype != torch.float32 or gnorm.numel() < 2):
        raise ValueError(f"{name}: gnorm must hold 2 float32 values")
    if nonfinite.dtype != torch.int32 or nonfinite.numel() < 1:
        raise ValueError(f"{name}: nonfinite must be an int32 counter")
    return part, int(n_part), max_norm, gnorm, nonfinite


def _clip_kw(clip, n, name, clip_rule, n_part, sticky):
    """The clip's keywords of the dl4ss_optim.h entry points (clip None: part NULL, unclipped)."""
    if clip_rule not in (CLIP_TORCH, CLIP_KERAS):
        raise ValueError(f"{name}: clip_rule {clip_rule!r}, expected {CLIP_TORCH} (torch) or {CLIP_KERAS} (Keras)")
    if clip is None:
        return dict(part=None, n_part=0, clip_rule=int(clip_rule), max_norm=0.0, gnorm=None, nonfinite=None,
                    nonfinite_sticky=0)
    part, n_part, max_norm, gnorm, nonfinite = _clip_args(clip, n, name, n_part)
    return dict(part=_lib.ptr(part), n_part=n_part, clip_rule=int(clip_rule), max_norm=max_norm,
                gnorm=_lib.ptr(gnorm), nonfinite=_lib.ptr(nonfinite), nonfinite_sticky=int(bool(sticky)))


def _update_kw(p, g, m, v, step, lr, betas, eps, status, loss, dp_flag, gscale, shadow, name):
    """The keywords every guarded update shares, shadow segments included (none: nseg 0)."""
    for t in (p, g, m, v):
        _f32c(t, name)
    if status is not None and status.numel() < 2:
        raise ValueError(f"{name}: the status word needs 2 ints (timed out, refused-update count)")
    nseg, seg_off, seg_rows, seg_cols, seg_y, seg_ldy = shadow if shadow is not None else (0,) + (None,) * 5
    return dict(p=_lib.ptr(p), g=_lib.ptr(g), m=_lib.ptr(m), v=_lib.ptr(v), n=p.numel(), lr=float(lr),
                beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), step=int(step),
                status=_lib.ptr(status), dp_flag=_lib.ptr(dp_flag), gscale=float(gscale), loss=_lib.ptr(loss),
                nseg=nseg, seg_off=seg_off, seg_rows=seg_rows, seg_cols=seg_cols, seg_y=seg_y, seg_ldy=seg_ldy,
                stream=_lib.stream_ptr())


def nadam_(p, g, m, v, step, schedule, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, status=None, loss=None, dp_flag=None,
           gscale=1.0, shadow=None, clip=None, clip_rule=CLIP_KERAS, n_part=None, sticky=False):
    """Keras 1's Nadam step on flat buffers (dl4ss_nadam, include/dl4ss_optim.h has the formulas), arguments as
    adam_.  ``schedule``: (mu(step), mu(step + 1), P(step)) as Python floats, adam.nadam_schedule's.  ``clip``:
    adam_'s tuple, by ``clip_rule`` CLIP_KERAS (c = max_norm / nrm where nrm >= max_norm, else 1) or CLIP_TORCH;
    ``n_part``: part holds that many partials, of this gradient or of several side by side (the joint norm);
    ``sticky``: a refusal for a non-finite sum also sets bit STATUS_NONFINITE_GRAD of status[0]."""
    mu, mu_next, mu_prod = (float(x) for x in schedule)
    kw = _update_kw(p, g, m, v, step, lr, betas, eps, status, loss, dp_flag, gscale, shadow, "nadam_")
    _lib.call("dl4ss_nadam", mu=mu, mu_next=mu_next, mu_prod=mu_prod,
              **_clip_kw(clip, p.numel(), "nadam_", clip_rule, n_part, sticky), **kw)


def adam_(p, g, m, v, step, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, status=None, loss=None, dp_flag=None, gscale=1.0,
          shadow=None, clip=None, clip_rule=CLIP_TORCH, n_part=None, sticky=False):
    """torch Adam step on flat buffers; with ``status`` (the recurrence hand-off status word,
    2 ints: {timed out, refused-update count}) the update is refused on device when a hand-off
    of this step timed out, loss[0] is set to NaN and status[1] counts the refusal
    (dl4ss_adam_guarded_dp's 2-int status form); with ``dp_flag`` (the all-reduced status flag
    behind the flat gradient) also when a data-parallel peer's hand-off timed out.  ``gscale``: the
    update uses g * gscale (1 / world_size on a SUM-reduced gradient; 1 is bitwise the unscaled step).
    ``shadow``: (nseg, seg_off, seg_rows, seg_cols, seg_y, seg_ldy) ctypes arrays -- bf16 copies of the
    updated parameters written by the same launch (dl4ss_adam_guarded_dp_scaled_bf16).
    ``clip``: (part, max_norm, gnorm, nonfinite) -- the gradient's global norm clipped to max_norm
    (dl4ss_adam_clipped): part = grad_sumsq(g), gnorm a float32[2] that receives {the norm of g * gscale, the
    coefficient c} (or None), nonfinite an int32[1] that counts the updates refused because g held an Inf
    or NaN (refused like a timed-out step: status[1] counts them too).  None: today's call, unchanged.
    ``clip_rule`` CLIP_KERAS, ``n_part`` or ``sticky`` (nadam_'s): dl4ss_adam_clipped_ex; without them every call
    reaches the entry point it always reached, with the same arguments."""
    if clip is not None and (clip_rule != CLIP_TORCH or n_part is not None or sticky):
        kw = _update_kw(p, g, m, v, step, lr, betas, eps, status, loss, dp_flag, gscale, shadow, "adam_")
        _lib.call("dl4ss_adam_clipped_ex", **_clip_kw(clip, p.numel(), "adam_", clip_rule, n_part, sticky), **kw)
        return
    for t in (p, g, m, v):
        _f32c(t, "adam")
    if status is not None and status.numel() < 2:
        raise ValueError("adam_: the status word needs 2 ints (timed out, refused-update count)")
    if clip is not None:
        part, max_norm, gnorm, nonfinite = clip
        max_norm = check_clip_norm(max_norm, "adam_: max_norm")
        n_part = grad_sumsq_parts(p.numel())
        if part.dtype != torch.float64 or part.numel() < n_part:
            raise ValueError(f"adam_: clip needs the {n_part} float64 partials of grad_sumsq")
        if gnorm is not None and (gnorm.dtype != torch.float32 or gnorm.numel() < 2):
            raise ValueError("adam_: gnorm must hold 2 float32 values")
        if nonfinite.dtype != torch.int32 or nonfinite.numel() < 1:
            raise ValueError("adam_: nonfinite must be an int32 counter")
    # the parameters the three entry points share, then the shadow segments (none: nseg 0), then the clip's
    step_kw = dict(p=_lib.ptr(p), g=_lib.ptr(g), m=_lib.ptr(m), v=_lib.ptr(v), n=p.numel(), lr=float(lr),
                   beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), step=int(step),
                   status=_lib.ptr(status), dp_flag=_lib.ptr(dp_flag), gscale=float(gscale), loss=_lib.ptr(loss),
                   stream=_lib.stream_ptr())
    if clip is not None or shadow is not None:
        nseg, seg_off, seg_rows, seg_cols, seg_y, seg_ldy = shadow if shadow is not None else (0,) + (None,) * 5
        step_kw.update(nseg=nseg, seg_off=seg_off, seg_rows=seg_rows, seg_cols=seg_cols, seg_y=seg_y, seg_ldy=seg_ldy)
    if clip is not None:
        _lib.call("dl4ss_adam_clipped", part=_lib.ptr(part), n_part=n_part, max_norm=max_norm, gnorm=_lib.ptr(gnorm),
                  nonfinite=_lib.ptr(nonfinite), **step_kw)
    elif shadow is not None:
        _lib.call("dl4ss_adam_guarded_dp_scaled_bf16", **step_kw)
    else:
        _lib.call("dl4ss_adam_guarded_dp_scaled", **step_kw)


# the Discriminator's launch sequences, over the caller's buffers (autograd's Functions, the adversarial step)
def disc_forward(prec, maps, params, ys, logit, score):
    """maps (N, T, F) -> score (N): three convs and the head.  ``params``: the eight parameters in state_dict
    order (cnn, cnn1, cnn2, final; weight, bias); ``ys``: the three channels-last activations."""
    w1, b1, w2, b2, w3, b3, wf, bf = (_lib.ptr(p) for p in params)
    (N, T, F), (y1, y2, y3), st = maps.shape, ys, _lib.stream_ptr()
    _lib.call("dl4ss_disc_conv1_fwd", prec, _lib.ptr(maps), w1, b1, N, T, F, _lib.ptr(y1), st)
    for x, y, w, b in ((y1, y2, w2, b2), (y2, y3, w3, b3)):
        _lib.call("dl4ss_disc_conv64_fwd", prec, _lib.ptr(x), w, b, N, x.shape[1], x.shape[2], _lib.ptr(y), st)
    _lib.call("dl4ss_disc_head_fwd", prec=prec, y3=_lib.ptr(y3), wf=wf, bf=bf, N=N, H3=y3.shape[1], W3=y3.shape[2],
              z=_lib.ptr(logit), score=_lib.ptr(score), stream=st)


def disc_backward(prec, maps, weights, ys, dys, score, dscore, target, loss, dz, grads, dx, ws, ws_bytes):
    """The backward of disc_forward from ``dscore`` (N), or (dscore None) from the head's fused loss
    mean_n (score_n - target)^2 -> ``loss``.  ``weights``: cnn, cnn1, cnn2, final; ``grads``: the eight parameter
    gradients in state_dict order; ``dys``: scratch like ``ys``; ``dx`` (N, T, F) or None: the input gradient."""
    w1, w2, w3, wf = (_lib.ptr(w) for w in weights)
    dw1, db1, dw2, db2, dw3, db3, dwf, dbf = (_lib.ptr(g) for g in grads)
    (N, T, F), (y1, y2, y3), (d1, d2, d3), ws, st = maps.shape, ys, dys, _lib.ptr(ws), _lib.stream_ptr()
    _lib.call("dl4ss_disc_head_bwd", prec=prec, y3=_lib.ptr(y3), wf=wf, score=_lib.ptr(score), dscore=_lib.ptr(dscore),
              target=float(target), N=N, H3=y3.shape[1], W3=y3.shape[2], loss=_lib.ptr(loss), dz=_lib.ptr(dz), dwf=dwf,
              dbf=dbf, dy3=_lib.ptr(d3), stream=st)
    for x, y, dy, w, dx_, dw, db in ((y2, y3, d3, w3, d2, dw3, db3), (y1, y2, d2, w2, d1, dw2, db2)):
        _lib.call("dl4ss_disc_conv64_bwd", prec=prec, x=_lib.ptr(x), y=_lib.ptr(y), dy=_lib.ptr(dy), w=w, N=N,
                  Hin=x.shape[1], Win=x.shape[2], dx=_lib.ptr(dx_), dw=dw, db=db, ws=ws, ws_bytes=ws_bytes, stream=st)
    _lib.call("dl4ss_disc_conv1_bwd", prec=prec, x=_lib.ptr(maps), y1=_lib.ptr(y1), dy1=_lib.ptr(d1), w=w1, N=N, T=T,
              F=F, dx=_lib.ptr(dx), dw=dw1, db=db1, ws=ws, ws_bytes=ws_bytes, stream=st)


# ---------------------------------------------------------------------------
# the bidirectional recurrence
# ---------------------------------------------------------------------------
CELLS = {"lstm": _C["DL4SS_CELL_LSTM"], "gru": _C["DL4SS_CELL_GRU"]}
# flags OR-ed into the recurrence entry points' precision argument (include/dl4ss_hip.h)
WS_ZEROED = _C["DL4SS_RNN_WS_ZEROED"]  # the caller keeps the hand-off workspace zeroed
DGH_PAD8 = _C["DL4SS_RNN_DGH_PAD8"]  # each direction's bf16 dGh columns start 16-B aligned
DEFER_BIAS = _C["DL4SS_RNN_DEFER_BIAS"]  # bias partials stay in the workspace (dl4ss_birnn_bias_reduce)
HARD_GATES = _C["DL4SS_RNN_HARD_GATES"]  # Keras 1's LSTM cell: hard_sigmoid i / f / o gates (fp32 LSTM only)
GATES = ("logistic", "hard")


def gate_flags(gates, cell="lstm", precision="fp32"):
    """The recurrence flag of a net's ``gates`` setting: 0 for "logistic", HARD_GATES for "hard", which exists
    for the LSTM on the fp32 recurrence only (ValueError otherwise, before any device call)."""
    if gates not in GATES:
        raise ValueError(f"gates {gates!r}: expected one of {GATES}")
    if gates == "logistic":
        return 0
    if cell != "lstm":
        raise ValueError(f"gates='hard' is Keras 1's LSTM cell: cell {cell!r} has no hard-gates form")
    if PREC[precision] != 0:
        raise ValueError("gates='hard' (Keras 1's LSTM cell) needs the fp32 recurrence: the packed bf16 recurrence "
                         f"has no hard-gates form (the recurrence resolves to {precision!r}; use precision='fp32', "
                         "or precision='bf16' with rnn_precision='fp32')")
    return HARD_GATES


def DOUT_SLABS(n):  # DL4SS_RNN_DOUT_SLABS(S): the BPTT sums dOut's S split-K slabs itself
    return ((n - 1) & 3) << 12


def birnn_fwd(cell, B, T, H, *, G, w_hh, b_hh, act, ws, ws_bytes, status, out=None, hprev=None, cs=None,
              out_bf16=None, hprev_bf16=None, h_mean=None, precision="fp32", flags=0):
    """One bidirectional layer's recurrence over the input projections G (dl4ss_birnn_fwd_mean, the
    superset of dl4ss_birnn_fwd / _fwd_ex: absent tensors are None)."""
    p = _lib.ptr
    _lib.call("dl4ss_birnn_fwd_mean", CELLS[cell], PREC[precision] | flags, B, T, H, p(G), p(w_hh), p(b_hh), p(out),
              p(hprev), p(act), p(cs), p(out_bf16), p(hprev_bf16), p(h_mean), p(ws), ws_bytes, p(status),
              _lib.stream_ptr())


def birnn_fwd_xw(cell, B, T, H, *, x, w_ih, b_ih, w_hh, b_hh, act, ws, ws_bytes, status, out=None, hprev=None,
                 cs=None, out_bf16=None, hprev_bf16=None, h_mean=None, ws_zeroed=True):
    """The recurrence with the input projection x w_ih^T + b_ih fused into it (dl4ss_birnn_fwd_xw_ex; bf16
    rows x (B*T, Kin) and w_ih (2 NG H, Kin), row strides taken from the views)."""
    p = _lib.ptr
    _lib.call("dl4ss_birnn_fwd_xw_ex", CELLS[cell], B, T, H, p(x, True), x.shape[1], x.stride(0), p(w_ih, True),
              w_ih.stride(0), p(b_ih), p(w_hh), p(b_hh), p(out), p(hprev), p(act), p(cs), p(out_bf16), p(hprev_bf16),
              p(h_mean), p(ws), ws_bytes, p(status), _lib.stream_ptr(), int(ws_zeroed))


def birnn_bwd(cell, B, T, H, *, w_hh, act, ws, ws_bytes, status, dOut=None, dOut_bcast=None, cs=None, hprev=None,
              dG=None, dGh=None, dG_bf16=None, dGh_bf16=None, db_ih=None, db_hh=None, precision="fp32", flags=0):
    """One bidirectional layer's BPTT (dl4ss_birnn_bwd_ex, the superset of dl4ss_birnn_bwd: absent
    tensors are None)."""
    p = _lib.ptr
    _lib.call("dl4ss_birnn_bwd_ex", CELLS[cell], PREC[precision] | flags, B, T, H, p(dOut), p(dOut_bcast), p(w_hh),
              p(act), p(cs), p(hprev), p(dG), p(dGh), p(dG_bf16), p(dGh_bf16), p(db_ih), p(db_hh), p(ws), ws_bytes,
              p(status), _lib.stream_ptr())


# split-precision operand images (dl4ss_f32_to_bf16_hilo), hi / lo per segment by pattern bit: three terms
# [x_hi | x_lo | x_hi] . [w_hi | w_hi | w_lo] (K' = 3 K), two terms [x_hi | x_hi] . [w_hi | w_lo] (K' = 2 K)
A_SPLIT, W_SPLIT = 0b010, 0b100
A_SPLIT2, W_SPLIT2 = 0b00, 0b10


def pad8(n):
    """n rounded up to a multiple of 8 (16-B aligned bf16 operand rows)"""
    return (n + 7) // 8 * 8


def hilo(x, y, segw, pattern, nseg=3):
    """y = the split image of the fp32 rows x: nseg segments of segw, hi / lo by pattern bits."""
    _lib.call("dl4ss_f32_to_bf16_hilo", x=_lib.ptr(x, True), ldx=x.stride(0), rows=x.shape[0], cols=x.shape[1],
              y=_lib.ptr(y), ldy=y.stride(0), segw=segw, nseg=nseg, pattern=pattern, stream=_lib.stream_ptr())


def birnn_plan(cell, B, H, precision="bf16", max_wg=0):
    """The persistent recurrence's plan {BC, NG, J, nchunk, grid} under a co-residency budget
    of max_wg workgroups (0: the current device's); None when no plan fits (host-only for
    max_wg > 0)."""
    import ctypes

    info = (ctypes.c_int * 5)()
    rc = _lib.lib().dl4ss_birnn_plan_info(CELLS[cell], int(B), int(H),
                                          1 if precision == "bf16" else 0, int(max_wg), info)
    if rc != 0:
        return None
    return dict(zip(("BC", "NG", "J", "nchunk", "grid"), list(info)))


# ---------------------------------------------------------------------------
# voiceprint encoder / speaker memory (voiceprint.hip)
# ---------------------------------------------------------------------------
VP_RULES = {"nonzero": 0, "gt": 1}


def _i32c(t, name, numel):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == numel):
        raise RuntimeError(f"{name}: expected a contiguous int32 CUDA tensor of {numel} elements")
    return t


def vp_compact(x, rule="nonzero", thr=None, lengths=None, xc=None, len_out=None, idx=None):
    """x (n, T, F) -> (xc (n, T, F) the valid frames as a prefix, len (n) int32, idx (n, T) int32, -1 behind
    len).  rule "nonzero": any bin != 0; "gt": any bin > thr; lengths (n) int32: a plain prefix instead."""
    _f32c(x, "vp_compact")
    if x.dim() != 3:
        raise RuntimeError("vp_compact: expected (n, T, F)")
    if rule not in VP_RULES:
        raise ValueError(f"vp_compact: rule {rule!r}, expected one of {sorted(VP_RULES)}")
    if rule == "gt" and thr is None and lengths is None:
        raise ValueError("vp_compact: rule 'gt' needs thr")
    n, T, F = x.shape
    if lengths is not None:
        _i32c(lengths, "vp_compact(lengths)", n)
    i32 = dict(device=x.device, dtype=torch.int32)
    xc = torch.empty_like(x) if xc is None else _f32c(xc, "vp_compact(xc)")
    len_out = torch.empty(n, **i32) if len_out is None else _i32c(len_out, "vp_compact(len)", n)
    idx = torch.empty(n, T, **i32) if idx is None else _i32c(idx, "vp_compact(idx)", n * T)
    if xc.numel() != x.numel():
        raise RuntimeError("vp_compact: xc must have x's size")
    _lib.call("dl4ss_vp_compact", x=_lib.ptr(x), n=n, T=T, F=F, rule=VP_RULES[rule],
              thr=float(0.0 if thr is None else thr), len_in=_lib.ptr(lengths), xc=_lib.ptr(xc), len=_lib.ptr(len_out),
              idx=_lib.ptr(idx), stream=_lib.stream_ptr())
    return xc, len_out, idx


def vp_shift(src, dst, lengths, c0, c1, direction, other=0):
    """dst (n, T, ld)[:, :, c0:c1] = src's rows moved by +(T - len) (direction +1, zero fill in front) or back
    (-1, zero rows behind len); the other columns: other 0 untouched, 1 src on rows < len and zero behind,
    2 src."""
    _f32c(src, "vp_shift(src)")
    _f32c(dst, "vp_shift(dst)")
    if src.dim() != 3 or src.shape != dst.shape:
        raise RuntimeError("vp_shift: src and dst must be (n, T, ld) of one shape")
    n, T, ld = src.shape
    _i32c(lengths, "vp_shift(lengths)", n)
    _lib.call("dl4ss_vp_shift", src=_lib.ptr(src), dst=_lib.ptr(dst), n=n, T=T, ld=ld, c0=int(c0), c1=int(c1),
              len=_lib.ptr(lengths), dir=int(direction), other=int(other), stream=_lib.stream_ptr())
    return dst


def vp_mean_fwd(out, lengths, vec=None):
    """out (n, T, 2H) in the recurrence's frame -> vec (n, 2H): each utterance's mean over its own frames."""
    _f32c(out, "vp_mean_fwd")
    n, T, D = out.shape
    _i32c(lengths, "vp_mean_fwd(lengths)", n)
    vec = torch.empty(n, D, device=out.device, dtype=torch.float32) if vec is None else _f32c(vec, "vp_mean_fwd(vec)")
    if D % 2 or vec.numel() != n * D:
        raise RuntimeError("vp_mean_fwd: out (n, T, 2H), vec (n, 2H)")
    _lib.call("dl4ss_vp_mean_fwd", _lib.ptr(out), n, T, D // 2, _lib.ptr(lengths), _lib.ptr(vec), _lib.stream_ptr())
    return vec


def vp_mean_bwd(dvec, lengths, dout):
    """dvec (n, 2H) -> dout (n, T, 2H), every element written."""
    _f32c(dvec, "vp_mean_bwd")
    _f32c(dout, "vp_mean_bwd(dout)")
    n, T, D = dout.shape
    _i32c(lengths, "vp_mean_bwd(lengths)", n)
    if D % 2 or dvec.numel() != n * D:
        raise RuntimeError("vp_mean_bwd: dvec (n, 2H), dout (n, T, 2H)")
    _lib.call("dl4ss_vp_mean_bwd", _lib.ptr(dvec), n, T, D // 2, _lib.ptr(lengths), _lib.ptr(dout), _lib.stream_ptr())
    return dout


def vp_colsum_part(M, C, device):
    """The partial-sum buffer vp_colsum needs for an (M, C) matrix."""
    P = _lib.query("dl4ss_vp_colsum_parts", int(M))
    if P < 0:
        raise RuntimeError(f"vp_colsum: M = {M} unsupported")
    return torch.empty(P * C, device=device, dtype=torch.float32)


def vp_colsum(A, out, part):
    """out (C) = column sums of the contiguous A (M, C) in a fixed order for any M (two stages through ``part``,
    no atomics: the same input gives the same bits); every element of out written."""
    _f32c(A, "vp_colsum")
    _f32c(out, "vp_colsum(out)")
    _f32c(part, "vp_colsum(part)")
    if A.dim() != 2 or out.numel() != A.shape[1]:
        raise RuntimeError("vp_colsum: A (M, C), out (C)")
    M, C = A.shape
    if part.numel() < _lib.query("dl4ss_vp_colsum_parts", M) * C:
        raise RuntimeError("vp_colsum: part too small (ops.vp_colsum_part)")
    _lib.call("dl4ss_vp_colsum", _lib.ptr(A), M, C, _lib.ptr(part), _lib.ptr(out), _lib.stream_ptr())
    return out


def _spk_args(v, ids, mem, name):
    _f32c(v, name)
    _f32c(mem, f"{name}(mem)")
    if v.dim() != 2 or mem.dim() != 2 or mem.shape[1] != v.shape[1]:
        raise RuntimeError(f"{name}: v (n, E) and mem (M, E)")
    n, E = v.shape
    if n > 1024 or E > 128:
        raise RuntimeError(f"{name}: n <= 1024 and E <= 128")
    _i32c(ids, f"{name}(ids)", n)
    return n, E, mem.shape[0]


def spk_memory_fwd(v, ids, mem, u=None, q=None):
    """v (n, E), ids (n) int32, mem (M, E) -> (q (n, E) the speakers' normalised memory rows with this batch's
    unit voiceprints accumulated, u (n, E) the unit voiceprints).  mem is only read."""
    n, E, M = _spk_args(v, ids, mem, "spk_memory_fwd")
    u = torch.empty_like(v) if u is None else _f32c(u, "spk_memory_fwd(u)")
    q = torch.empty_like(v) if q is None else _f32c(q, "spk_memory_fwd(q)")
    if u.numel() != n * E or q.numel() != n * E:
        raise RuntimeError("spk_memory_fwd: u and q must be (n, E)")
    _lib.call("dl4ss_spk_memory_fwd", _lib.ptr(v), _lib.ptr(ids), _lib.ptr(mem), n, E, M, _lib.ptr(u), _lib.ptr(q),
              _lib.stream_ptr())
    return q, u


def spk_memory_bwd(dq, v, u, ids, mem, dv=None):
    """dq (n, E) -> dv (n, E) (v, ids, mem as given to spk_memory_fwd, u as it wrote it)."""
    n, E, M = _spk_args(v, ids, mem, "spk_memory_bwd")
    _f32c(dq, "spk_memory_bwd(dq)")
    _f32c(u, "spk_memory_bwd(u)")
    dv = torch.empty_like(v) if dv is None else _f32c(dv, "spk_memory_bwd(dv)")
    if dq.numel() != n * E or u.numel() != n * E or dv.numel() != n * E:
        raise RuntimeError("spk_memory_bwd: dq, u and dv must be (n, E)")
    _lib.call("dl4ss_spk_memory_bwd", dq=_lib.ptr(dq), v=_lib.ptr(v), u=_lib.ptr(u), ids=_lib.ptr(ids),
              mem=_lib.ptr(mem), n=n, E=E, M=M, dv=_lib.ptr(dv), stream=_lib.stream_ptr())
    return dv


def spk_memory_store(q, ids, mem, status=None):
    """mem[ids[i]] = q[i] (ids outside [0, M) skipped); with ``status`` nothing is stored when status[0] != 0."""
    n, E, M = _spk_args(q, ids, mem, "spk_memory_store")
    _lib.call("dl4ss_spk_memory_store", _lib.ptr(q), _lib.ptr(ids), n, E, M, _lib.ptr(mem), _lib.ptr(status),
              _lib.stream_ptr())
    return mem


# ---- image query (csrc/imgq.hip, include/dl4ss_imgq.h) ----
def imgq_param_count(h, w, E):
    """Floats in the image-query encoder's parameter block for (h, w) images and E outputs."""
    P = _lib.query("dl4ss_imgq_param_count", h=int(h), w=int(w), E=int(E))
    if P < 0:
        raise ValueError(f"image query: images of {h} x {w} with E = {E}: {_C['DL4SS_IMGQ_MIN_HW']} <= h, w <= "
                         f"{_C['DL4SS_IMGQ_MAX_HW']} and 1 <= E <= {_C['DL4SS_IMGQ_MAX_E']}")
    return P


def _imgq_args(images, params, E, name):
    _f32c(images, name)
    _f32c(params, f"{name}(params)")
    if images.dim() != 3:
        raise RuntimeError(f"{name}: images (n, h, w)")
    n, h, w = images.shape
    P = imgq_param_count(h, w, E)
    if params.numel() < P:
        raise RuntimeError(f"{name}: params holds {params.numel()} floats, the encoder has {P}")
    if n > _C["DL4SS_IMGQ_MAX_N"]:
        raise RuntimeError(f"{name}: n <= {_C['DL4SS_IMGQ_MAX_N']}")
    return n, h, w, P


def imgq_fwd(images, params, E, vec=None):
    """images (n, h, w), params (the flat parameter block) -> vec (n, E), every element written."""
    n, h, w, _ = _imgq_args(images, params, E, "imgq_fwd")
    vec = torch.empty(n, E, device=images.device, dtype=torch.float32) if vec is None else _f32c(vec, "imgq_fwd(vec)")
    if vec.numel() != n * E:
        raise RuntimeError("imgq_fwd: vec must be (n, E)")
    _lib.call("dl4ss_imgq_fwd", images=_lib.ptr(images), params=_lib.ptr(params), n=n, h=h, w=w, E=int(E),
              vec=_lib.ptr(vec), stream=_lib.stream_ptr())
    return vec


def imgq_bwd(images, dvec, params, dpart):
    """dvec (n, E) -> dpart (n, ld): each image's own parameter gradient, columns behind the parameter count zero,
    every element written (the forward is recomputed from the images)."""
    _f32c(dvec, "imgq_bwd(dvec)")
    _f32c(dpart, "imgq_bwd(dpart)")
    if dvec.dim() != 2 or dpart.dim() != 2:
        raise RuntimeError("imgq_bwd: dvec (n, E), dpart (n, ld)")
    E = dvec.shape[1]
    n, h, w, P = _imgq_args(images, params, E, "imgq_bwd")
    if dvec.shape[0] != n or dpart.shape[0] != n or dpart.shape[1] < P:
        raise RuntimeError(f"imgq_bwd: dvec ({n}, E) and dpart ({n}, ld >= {P})")
    _lib.call("dl4ss_imgq_bwd", images=_lib.ptr(images), dvec=_lib.ptr(dvec), params=_lib.ptr(params), n=n, h=h, w=w,
              E=E, dpart=_lib.ptr(dpart), ld=dpart.shape[1], dpart_floats=dpart.numel(), stream=_lib.stream_ptr())
    return dpart


def imgq_reduce(dpart, out):
    """out (ld) = column sums of dpart (n, ld), rows added pairwise in a fixed order (include/dl4ss_imgq.h): the same
    bits for the same n; every element of out written."""
    _f32c(dpart, "imgq_reduce")
    _f32c(out, "imgq_reduce(out)")
    if dpart.dim() != 2 or out.numel() != dpart.shape[1]:
        raise RuntimeError("imgq_reduce: dpart (n, ld), out (ld)")
    _lib.call("dl4ss_imgq_reduce", dpart=_lib.ptr(dpart), n=dpart.shape[0], ld=dpart.shape[1], out=_lib.ptr(out),
              stream=_lib.stream_ptr())
    return out


def imgq_guard(loss, status):
    """status[0] |= 2 on device when loss[0] is not finite (the image-query step's refusal of such a step)."""
    _f32c(loss, "imgq_guard(loss)")
    _lib.call("dl4ss_imgq_guard", loss=_lib.ptr(loss), status=_lib.ptr(status), stream=_lib.stream_ptr())
