"""NumPy restatement of the int8 top-k path (tt_quantize_rows_i8, tt_retrieval_topk_i8_f32), shared by test_topk_i8_cpu.py
and test_gpu_topk_i8.py.  Every step is the f32 / integer arithmetic the contract names, so the GPU result must equal it
bit for bit:

- ``np_quantize``: amax = max|x|, scale = amax / 127 (f32 division), code = clip(rint(x / scale), -127, 127) (rint rounds
  half to even); a zero row has scale 0 and zero codes.
- ``np_stage1``: iscore = qc . codes (integers below 2^24: the f32 matrix product is exact whatever its summation order),
  key = f32(iscore) * scales[j]; the k1 best by (key descending, index ascending) without the excluded ids; scores
  key * qscale; tail (-inf, -1).
- ``np_order``: the stage-2 order of given scores: (score descending, index ascending), best k, tail (-inf, -1).
- ``recall_corpus`` / ``exact_topk_ids`` / ``recall_at_k``: the recall condition's corpora and yardstick (f64 exact top-k).
"""
import numpy as np

RECALL_MIN = 0.99
RECALL_SHAPE = dict(nq=64, n=20_000, d=128)
RECALL_CASES = [(10, 40), (100, 256)]                 # (k, k1)


def np_quantize(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    amax = np.abs(x).max(axis=1)
    scale = (amax / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.rint(x / scale[:, None])
    r = np.where(scale[:, None] == 0, np.float32(0), r)
    return np.clip(r, -127, 127).astype(np.int8), scale


def np_keys(qc, codes, scales):
    """f32 keys [nq, nc]: f32(iscore) * scales[j]."""
    iscore = qc.astype(np.float32) @ codes.astype(np.float32).T           # exact: integer partial sums below 2^24
    return (iscore * scales.astype(np.float32)[None, :]).astype(np.float32)


def np_stage1(qc, qscale, codes, scales, k1, excluded=None):
    """(scores f32 [nq, k1], ids int64 [nq, k1]) of the scan: per query the k1 best by (key desc, index asc)."""
    nq, nc = qc.shape[0], codes.shape[0]
    keys = np_keys(qc, codes, scales)
    S = np.full((nq, k1), -np.inf, dtype=np.float32)
    I = np.full((nq, k1), -1, dtype=np.int64)
    idx = np.arange(nc)
    for r in range(nq):
        keep = np.ones(nc, dtype=bool)
        if excluded is not None and len(excluded[r]):
            e = np.asarray(excluded[r], dtype=np.int64)
            keep[e[(e >= 0) & (e < nc)]] = False
        cand = idx[keep]
        kr = keys[r, cand]
        if len(cand) > k1:                                                    # only keys at or above the k1-th largest can enter
            sel = kr >= np.partition(kr, len(cand) - k1)[len(cand) - k1]
            cand, kr = cand[sel], kr[sel]
        best = cand[np.lexsort((cand, -kr))[:k1]]
        I[r, :len(best)] = best
        S[r, :len(best)] = keys[r, best] * np.float32(qscale[r])
    return S, I


def np_order(scores, ids, k):
    """Stage-2 order of one query's candidates (ids >= 0): best k by (score desc, index asc), tail (-inf, -1)."""
    scores, ids = np.asarray(scores, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    ok = ids >= 0
    scores, ids = scores[ok], ids[ok]
    o = np.lexsort((ids, -scores))[:k]
    S = np.full(k, -np.inf, dtype=np.float32)
    I = np.full(k, -1, dtype=np.int64)
    S[:len(o)] = scores[o]
    I[:len(o)] = ids[o]
    return S, I


def np_topk_i8(q, x, k, k1, excluded=None):
    """Ids [nq, k] of the whole path with a re-rank in f64 (for recall calibration only: the GPU re-rank is the f32 MFMA)."""
    codes, scales = np_quantize(x)
    qc, qs = np_quantize(q)
    _, cand = np_stage1(qc, qs, codes, scales, k1, excluded)
    out = np.full((q.shape[0], k), -1, dtype=np.int64)
    for r in range(q.shape[0]):
        c = cand[r][cand[r] >= 0]
        s = x[c].astype(np.float64) @ q[r].astype(np.float64)
        best = c[np.lexsort((c, -s))[:k]]
        out[r, :len(best)] = best
    return out


def recall_corpus(kind, nq, n, d):
    rng = np.random.default_rng(0)
    if kind == "uniform":
        return (rng.random((nq, d), dtype=np.float32) * 2 - 1), (rng.random((n, d), dtype=np.float32) * 2 - 1)
    return rng.standard_normal((nq, d), dtype=np.float32), rng.standard_normal((n, d), dtype=np.float32)


def exact_topk_ids(q, x, k):
    s = q.astype(np.float64) @ x.astype(np.float64).T
    return np.stack([np.lexsort((np.arange(x.shape[0]), -s[r]))[:k] for r in range(q.shape[0])])


def recall_at_k(got, exact):
    """Mean over queries of |got_r & exact_r| / k (padding -1 never counts)."""
    k = exact.shape[1]
    return float(np.mean([len(set(g[g >= 0].tolist()) & set(e.tolist())) / k for g, e in zip(got, exact)]))
