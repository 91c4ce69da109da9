"""Restatements of the lazy-Adam contract of include/twotower_hip.h (tt_adam_step_f32), shared by tests/test_adam_cpu.py and
tests/test_gpu_adam.py.

* the f32 one mirrors the device arithmetic operation by operation - NumPy's f32 + - * / sqrt are correctly rounded, like the
  device's __fadd_rn / __fsub_rn / __fmul_rn / __fdiv_rn / sqrtf, and nothing is contracted - so the GPU results are compared
  with it BIT FOR BIT;
* the f64 one is the same formulas in double precision (what torch.optim.SparseAdam / Adam compute), with exact scalars.

    m' = m + (g - m) * omb1        v' = v + (g*g - v) * omb2        w' = w - (alpha_t * m') / (sqrt(v') + eps)
    omb1 = 1 - beta1,  omb2 = 1 - beta2,  alpha_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)

Sparse g: oracle.two_tower.dedup_sum (the order of the device's duplicate sums) over the pairs whose id lies in [0, rows).
Dense g: slab 0 + slab 1 + ... (ascending, starting at slab 0), then + (2*l2)*w.
"""
import math

import numpy as np

from oracle import two_tower as tt

BETA1, BETA2, EPS = 0.9, 0.999, 1e-7          # Keras 2.15 Adam defaults


def coefficients32(lr, beta1, beta2, step):
    """(omb1, omb2, alpha_t) as np.float32, computed as the library does: lr and the betas are the f32 values of tt_adam_hyper
    widened to f64, every result is rounded once to f32."""
    lr, b1, b2 = (float(np.float32(x)) for x in (lr, beta1, beta2))
    alpha = lr * math.sqrt(1.0 - b2 ** int(step)) / (1.0 - b1 ** int(step))
    return np.float32(1.0 - b1), np.float32(1.0 - b2), np.float32(alpha)


def coefficients64(lr, beta1, beta2, step):
    return 1.0 - beta1, 1.0 - beta2, lr * math.sqrt(1.0 - beta2 ** int(step)) / (1.0 - beta1 ** int(step))


def _update(w, m, v, g, omb1, omb2, alpha, eps):
    """The three formulas on arrays of one dtype with scalars of that dtype, in exactly the order of the parentheses."""
    m2 = m + (g - m) * omb1
    v2 = v + (g * g - v) * omb2
    w2 = w - (alpha * m2) / (np.sqrt(v2) + eps)
    return w2, m2, v2


def _scalars(dtype, lr, beta1, beta2, eps, step):
    if dtype == np.float32:
        return coefficients32(lr, beta1, beta2, step) + (np.float32(eps),)
    assert dtype == np.float64
    return tuple(np.float64(x) for x in coefficients64(lr, beta1, beta2, step)) + (np.float64(eps),)


def sparse_adam(table, m, v, ids, grads, lr, step, beta1=BETA1, beta2=BETA2, eps=EPS):
    """In place on ``table``, ``m``, ``v`` (one dtype, f32 or f64): the rows of the valid ids only.  Returns the distinct valid ids."""
    ids = np.asarray(ids)
    ok = (ids >= 0) & (ids < table.shape[0])
    uniq, g = tt.dedup_sum(ids[ok], np.ascontiguousarray(grads[ok], dtype=table.dtype))
    if len(uniq):
        omb1, omb2, alpha, e = _scalars(table.dtype, lr, beta1, beta2, eps, step)
        table[uniq], m[uniq], v[uniq] = _update(table[uniq], m[uniq], v[uniq], g, omb1, omb2, alpha, e)
    return uniq


def dense_adam(w, m, v, slabs, l2, lr, step, beta1=BETA1, beta2=BETA2, eps=EPS):
    """In place on flat ``w``, ``m``, ``v``; ``slabs`` [n_slabs, count] of the same dtype."""
    dt = w.dtype.type
    g = slabs[0].copy()
    for k in range(1, slabs.shape[0]):
        g = g + slabs[k]
    g = g + (dt(2.0) * dt(l2)) * w
    omb1, omb2, alpha, e = _scalars(w.dtype, lr, beta1, beta2, eps, step)
    w[...], m[...], v[...] = _update(w, m, v, g, omb1, omb2, alpha, e)


def bits(a):
    """The bit patterns of an f32 array (so that -0.0 != +0.0 and NaNs compare)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
