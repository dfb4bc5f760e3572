"""fp64 restatement of Keras 1's Nadam and of Keras's clipnorm (dl4ss_nadam, dl4ss_adam_clipped_ex; the formulas are
in include/dl4ss_optim.h), in the style of small_ref.adam / clip_ref.adam_clipped: from the SAME fp32 inputs the
kernel gets, with the scalars formed as the launcher forms them and bars counted from the fp32 roundings.

    mu(i) = b1 (1 - 0.5 0.96^(i d)),  P(t) = mu(1) ... mu(t)      (Python floats, multiplied from i = 1 on)
    a1 = fl(lr (1 - mu(t)) / (1 - P(t))),  a2 = fl(lr mu(t+1) / (1 - P(t) mu(t+1))),  bc2s = fl(sqrt(1 - b2^t))
    gs = g f;  m' = b1 m + (1 - b1) gs;  v' = b2 v + (1 - b2) gs^2;
    p' = p - (a1 gs + a2 m') / (sqrt(v') / bc2s + eps)

The kernel evaluates m' = fma(b1, m, (1 - b1) gs), v' = fma(b2, v, ((1 - b2) gs) gs), num = fma(a1, gs, a2 m'),
den = sqrtf(v') / bc2s + eps, p' = p - num / den, every fused multiply-add explicit.  Counted roundings, u = 2^-24
(1 - b1 and 1 - b2 are exact for b1, b2 in [0.5, 1]: Sterbenz; a1, a2, bc2s are shared with the kernel exactly):
  gs: one product (exact at f = 1 or a power of two).
  m': the product (1 - b1) gs carries gs (1) and its own rounding (1), the fma rounds once (u |m'|); half a unit
      for second order:                       |dm| <= u |m'| + 2.5 u (1 - b1) |gs|
  v': ((1 - b2) gs) gs carries gs twice (2) and two products (2), the fma rounds once (u v'); half a unit for
      second order:                           |dv| <= u v' + 4.5 u (1 - b2) gs^2     (<= 5.5 u v')
  p': the final subtraction u |p'|; dm through a2 / den; and on X = (|a1 gs| + |a2 m'|) / den -- NOT on the
      update |x| <= X: the numerator is a sum of two products that may cancel -- the product a1 gs (gs 1, product
      absorbed by the fma: 1 u |a1 gs|) and a2 m' (1 u |a2 m'|), together <= 1 u X; the fma (1); den: dv <= 5.5 u v'
      through the root (2.75), sqrtf (1), / bc2s (1), + eps (1) = 5.75; the quotient (1): 8.75 u, within the 10 u
      taken:                                  |dp| <= u |p'| + a2 |dm| / den + 10 u X.
With an active clip the device's fp64 factor f and the one here round to the same fp32 number or to neighbours,
f_dev = f32 (1 + d), |d| <= 2 u (clip_ref.py), i.e. 2 more units on gs: dm += 2 u (1 - b1) |gs|,
dv += (4 u + 4 u^2)(1 - b2) gs^2, and on p' 2 u on a1 gs and 2 u on den: 14 u X.
No bar here comes from what a GPU returned.

Keras's clipnorm (Optimizer.get_gradients, clip_norm): S = sum g^2 over every gradient of the step,
nrm = gscale sqrt(S), c = clipnorm / nrm if nrm >= clipnorm, else 1: no + 1e-6, and >= in place of a min.
"""
import numpy as np
import torch

import clip_ref as cr
import small_ref as sr

U = sr.U
DEFAULTS = dict(lr=0.002, b1=0.9, b2=0.999, eps=1e-8, schedule_decay=0.004)


def f32(x):
    return float(np.float32(x))


def mu(i, b1=0.9, d=0.004):
    return b1 * (1.0 - 0.5 * 0.96 ** (i * d))


def schedule(t, b1=0.9, d=0.004):
    """(mu(t), mu(t + 1), P(t)) from scratch: the product multiplied sequentially from i = 1."""
    P = mu(1, b1, d)
    for i in range(2, t + 1):
        P *= mu(i, b1, d)
    return mu(t, b1, d), mu(t + 1, b1, d), P


def scalars(lr, b1, b2, t, d=0.004, mu_next_of=None, sched=None):
    """(a1, a2, bc2s) as the launcher forms them: in double from the fp32 lr, beta2 and the double schedule (of
    the fp32 beta1), each rounded once to fp32.  mu_next_of: the step whose mu stands in for mu(t + 1) (a wrong
    restatement, for test_nadam_ref_cpu.py).  sched: (mu(t), mu(t + 1), P(t)) given, e.g. P = 0 (the product's
    underflow: a1 = lr (1 - mu), a2 = lr mu_next)."""
    lr, b1, b2 = f32(lr), f32(b1), f32(b2)
    m_t, m_n, P = schedule(t, b1, d) if sched is None else sched
    if mu_next_of is not None:
        m_n = mu(mu_next_of, b1, d)
    return f32(lr * (1.0 - m_t) / (1.0 - P)), f32(lr * m_n / (1.0 - P * m_n)), f32(np.sqrt(1.0 - b2 ** t))


def keras_clip(g, clipnorm, gscale=1.0):
    """(nrm, c, f) in fp64 from the fp32 gradient(s) g (a tensor or a list: the joint norm), the fp32 threshold
    and the fp32 gscale, by Keras's rule."""
    gscale, clipnorm = f32(gscale), f32(clipnorm)
    gs = g if isinstance(g, (list, tuple)) else [g]
    nrm = gscale * float(np.sqrt(sum(cr.sumsq(x) for x in gs)))
    c = clipnorm / nrm if nrm >= clipnorm else 1.0
    return nrm, c, gscale * c


def nadam(p, g, m, v, lr, b1, b2, eps, step, f=1.0, d=0.004, clipped=False, drop_a2=None, mu_next_of=None,
          sched=None):
    """((p', dp), (m', dm), (v', dv)): one update at the fp32 factor f (gscale, or clip's f32) and its bars.
    clipped: f came from an active clip (2 more units on gs, see above).  drop_a2 (an element index) and
    mu_next_of: wrong restatements for test_nadam_ref_cpu.py."""
    a1, a2, bc2s = scalars(lr, b1, b2, step, d, mu_next_of, sched)
    b1, b2, eps, f = f32(b1), f32(b2), f32(eps), f32(f)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gs = g * f
    m2 = b1 * m + (1.0 - b1) * gs
    v2 = b2 * v + (1.0 - b2) * gs * gs
    den = v2.sqrt() / bc2s + eps
    t1, t2 = a1 * gs, a2 * m2
    if drop_a2 is not None:
        t2 = t2.clone()
        t2[drop_a2] = 0.0
    p2 = p - (t1 + t2) / den
    extra = 2.0 if clipped else 0.0
    dm = U * m2.abs() + (2.5 + extra) * U * (1.0 - b1) * gs.abs()
    dv = U * v2 + (4.5 + 2 * extra + (4 * U if clipped else 0.0)) * U * (1.0 - b2) * gs * gs
    X = (t1.abs() + (a2 * m2).abs()) / den
    dp = U * p2.abs() + a2 * dm / den + (10.0 + 2 * extra) * U * X
    return (p2, dp), (m2, dm), (v2, dv)


def nadam_clipped(p, g, m, v, lr, b1, b2, eps, step, clipnorm, gscale=1.0, d=0.004, joint=None):
    """((p', dp), (m', dm), (v', dv), (nrm, c, f32)): Nadam under Keras's clipnorm.  joint: every gradient of the
    norm (a list; default g alone)."""
    nrm, c, f = keras_clip(g if joint is None else joint, clipnorm, gscale)
    f_32 = f32(f)
    return nadam(p, g, m, v, lr, b1, b2, eps, step, f_32, d, clipped=c != 1.0) + ((nrm, c, f_32),)


def emulate_f32(p, g, m, v, lr, b1, b2, eps, step, f=1.0, d=0.004):
    """The kernel's own sequence in numpy fp32 (each fma emulated in fp64 and rounded once: the products of two
    fp32 numbers are exact in fp64, the sums of two such lose at most 2^-53 relative): p', m', v'."""
    a1, a2, bc2s = (np.float32(x) for x in scalars(lr, b1, b2, step, d))
    r = lambda x: np.asarray(x, np.float64).astype(np.float32)
    b1, b2, eps, f = np.float32(b1), np.float32(b2), np.float32(eps), np.float32(f)
    p, g, m, v = (t.numpy().astype(np.float32) for t in (p, g, m, v))
    gs = r(g.astype(np.float64) * f)
    omb1, omb2 = np.float32(1) - b1, np.float32(1) - b2
    m2 = r(np.float64(b1) * m + np.float64(r(np.float64(omb1) * gs)))
    v2 = r(np.float64(b2) * v + np.float64(r(np.float64(r(np.float64(omb2) * gs)) * gs)))
    den = r(np.float64(r(np.float64(np.sqrt(v2)) / np.float64(bc2s))) + np.float64(eps))
    num = r(np.float64(a1) * gs + np.float64(r(np.float64(a2) * m2)))
    p2 = r(np.float64(p) - np.float64(r(np.float64(num) / np.float64(den))))
    return tuple(torch.from_numpy(x.astype(np.float64)) for x in (p2, m2, v2))
