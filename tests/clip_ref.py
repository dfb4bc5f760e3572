"""fp64 restatement of the global-norm gradient clip (dl4ss_grad_sumsq + dl4ss_adam_clipped), in the style of
small_ref.py: from the SAME fp32 inputs the kernels get, with bars counted from the fp32 roundings.

    S = sum g_i^2;  nrm = gscale sqrt(S);  c = min(1, max_norm / (nrm + 1e-6));  f = gscale c

(torch.nn.utils.clip_grad_norm_'s coefficient on the mean gradient g gscale).  The device evaluates all of it
in fp64 from an fp64 sum of exact squares; its S differs from the one here only by the order of at most ~1e7
fp64 additions of non-negative terms (relative 1e7 2^-53 ~ 1e-9 at the very worst, 1e-13 typically, far below
u = 2^-24).  What is rounded to fp32 is

    gnorm = {fl(nrm), fl(c)}: one rounding each, u relative; the tests allow 2 u;
    f32   = fl(f), the factor the update multiplies g by: the device's fp64 f and this one round to the same
            fp32 number or to neighbours, so f_dev = f32 (1 + d), |d| <= 2 u (one fp32 ulp is at most 2 u).

adam_clipped is small_ref.adam at gscale = f32 with those 2 more units on gs = g f32 carried through its bars:
    m': (1 - b1) gs moves by at most 2 u |gs|:                          dm += 2 u |gs|
    v': (1 - b2) gs^2 moves by (1 + 2 u)^2 - 1 = 4 u + 4 u^2 relative:  dv += (4 u + 4 u^2)(1 - b2) gs^2
    p': the larger dm through step dm / denom; the extra <= 4 u relative on v' is 2 u on the root and the
        update x, and the counted 8.5 u + 2 u still fits the 12 u |x| small_ref.adam allows.
No bar here comes from what a GPU returned.
"""
import numpy as np
import torch

import small_ref as sr

U = sr.U
GNORM_U = 2  # units allowed on each of gnorm's two fp32 numbers


def f32(x):
    return float(np.float32(x))


def sumsq(g):
    """the exact squares of the fp32 gradient summed in fp64"""
    g = g.double().reshape(-1)
    return float((g * g).sum())


def clip(g, max_norm, gscale=1.0):
    """(nrm, c, f) in fp64 from the fp32 gradient g, the fp32 threshold and the fp32 gscale"""
    gscale, max_norm = f32(gscale), f32(max_norm)
    nrm = gscale * float(np.sqrt(sumsq(g)))
    c = min(1.0, max_norm / (nrm + 1e-6))
    return nrm, c, gscale * c


def adam_clipped(p, g, m, v, lr, b1, b2, eps, step, max_norm, gscale=1.0):
    """((p', dp), (m', dm), (v', dv), (nrm, c, f32)): the clipped update and its bars (see above)."""
    nrm, c, f = clip(g, max_norm, gscale)
    f_32 = f32(f)
    (p2, _), (m2, dm), (v2, dv) = sr.adam(p, g, m, v, lr, b1, b2, eps, step, f_32)
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    gs = g.double() * f_32
    dm = dm + 2 * U * gs.abs()
    dv = dv + (4 * U + 4 * U * U) * (1.0 - b2) * gs * gs
    step_sz = lr / f32(1.0 - b1 ** step)
    denom = v2.sqrt() / f32(np.sqrt(1.0 - b2 ** step)) + eps
    x = step_sz * m2 / denom
    dp = U * p2.abs() + step_sz * dm / denom + 12 * U * x.abs()
    return (p2, dp), (m2, dm), (v2, dv), (nrm, c, f_32)


def gnorm_close(got, nrm, c):
    """gnorm (2 fp32 numbers) within GNORM_U units of the fp64 norm and coefficient"""
    a, b = float(got[0]), float(got[1])
    return abs(a - nrm) <= GNORM_U * U * nrm and abs(b - c) <= GNORM_U * U * c
