"""Restatements of the row-wise Adagrad contract of include/twotower_hip.h (tt_rowwise_adagrad_step_f32), shared by
tests/test_rowwise_cpu.py and tests/test_gpu_rowwise.py.

    q_j = g_j * g_j      S = sum_j q_j      a' = a + S * inv_dim      w' = w - (lr * g) / sqrt(a' + eps)

* the f32 one mirrors the device operation by operation - NumPy's f32 + * / sqrt are correctly rounded, like the device's
  __fadd_rn / __fmul_rn / __fdiv_rn / sqrtf, and nothing is contracted - INCLUDING the order of S and
  inv_dim = np.float32(1) / np.float32(dim), so the GPU results are compared with it BIT FOR BIT;
* the f64 one is the same formulas in double precision with exact scalars (S a plain f64 sum, inv_dim = 1 / dim).

Order of S (a function of dim alone): lpr = min(32, dim/4 rounded up to a power of two) lanes own the row; lane l holds the
float4 chunks c = l, l + lpr, ... < dim/4 and adds its q values one after the other - chunks ascending, elements ascending inside
a chunk, the sum starting AT its first value; a lane without a chunk holds +0; then the butterfly p_l = p_l + p_{l xor off} for
off = 1, 2, 4, ... < lpr, after which every lane holds the same bits.

Sparse g: oracle.two_tower.dedup_sum (the order of the device's duplicate sums) over the pairs whose id lies in [0, rows).
"""
import numpy as np

from oracle import two_tower as tt


def lanes_per_row(dim):
    """min(32, dim/4 rounded up to a power of two)."""
    dim4, lpr = dim // 4, 1
    while lpr < dim4 and lpr < 32:
        lpr *= 2
    return lpr


def roundings_on_the_longest_path(dim):
    """R: the additions on the longest path of S - a lane's in-lane adds (4 * chunks - 1 for the lane with the most chunks)
    plus log2(lpr) butterfly adds."""
    dim4, lpr = dim // 4, lanes_per_row(dim)
    chunks = -(-dim4 // lpr)
    return 4 * chunks - 1 + int(np.log2(lpr))


def row_sum_of_squares32(g):
    """S of every row of the f32 array g [n, dim] in the device's order; returns f32 [n]."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    n, dim = g.shape
    assert dim % 4 == 0
    dim4, lpr = dim // 4, lanes_per_row(dim)
    q = (g * g).reshape(n, dim4, 4)                      # f32 products, one rounding each
    p = np.zeros((n, lpr), dtype=np.float32)             # a lane without a chunk: +0
    for l in range(min(lpr, dim4)):
        acc = None
        for c in range(l, dim4, lpr):
            for e in range(4):
                acc = q[:, c, e].copy() if acc is None else acc + q[:, c, e]      # starts AT the first value
        p[:, l] = acc
    off = 1
    while off < lpr:
        p = p + p[:, np.arange(lpr) ^ off]               # every lane: p_l + p_{l xor off}
        off *= 2
    assert (p.view(np.uint32) == p[:, :1].view(np.uint32)).all()     # every lane ends with the same bits
    return p[:, 0].copy()


def rowwise_update32(w, a, g, lr, eps):
    """(w', a') for f32 rows w, g [n, dim] and accumulators a [n], operation by operation as the device."""
    dim = g.shape[1]
    f = np.float32
    inv_dim = f(1) / f(dim)
    a2 = a + row_sum_of_squares32(g) * inv_dim
    den = np.sqrt(a2 + f(eps))
    return w - (f(lr) * g) / den[:, None], a2


def rowwise_update64(w, a, g, lr, eps):
    """The same formulas in f64 with exact scalars."""
    a2 = a + (g * g).sum(axis=1) * (1.0 / g.shape[1])
    return w - (lr * g) / np.sqrt(a2 + eps)[:, None], a2


def sparse_rowwise_adagrad(table, row_accum, ids, grads, lr, eps=1e-7):
    """In place on ``table`` [rows, dim] and ``row_accum`` [rows] (one dtype, f32 or f64): the rows of the valid ids only.
    Returns the distinct valid ids."""
    ids = np.asarray(ids)
    ok = (ids >= 0) & (ids < table.shape[0])
    uniq, g = tt.dedup_sum(ids[ok], np.ascontiguousarray(grads[ok], dtype=table.dtype))
    if len(uniq):
        upd = rowwise_update32 if table.dtype == np.float32 else rowwise_update64
        assert table.dtype in (np.float32, np.float64) and row_accum.dtype == table.dtype
        table[uniq], row_accum[uniq] = upd(table[uniq], row_accum[uniq], g, lr, eps)
    return uniq


def dense_adagrad(w, acc, slabs, l2, lr, eps=1e-7):
    """In place on flat f32 ``w``, ``acc``: the element-wise Adagrad of tt_dense_update_f32; ``slabs`` [n_slabs, count]."""
    f = w.dtype.type
    g = slabs[0].copy()
    for k in range(1, slabs.shape[0]):
        g = g + slabs[k]
    g = g + (f(2.0) * f(l2)) * w
    acc[...] = acc + g * g
    w[...] = w - (f(lr) * g) / np.sqrt(acc + f(eps))


def bits(a):
    """The bit patterns of an f32 array (so that -0.0 != +0.0 and NaNs compare)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
