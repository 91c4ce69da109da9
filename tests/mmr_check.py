"""NumPy restatement of tt_mmr_rerank_f32 (include/twotower_hip.h): every step one IEEE f32 operation, so the GPU result
must equal it bit for bit.  Checker only - nothing here is used by the product."""
import functools

import numpy as np

F = np.float32


def np_dot_all(rows):
    """G[j, p] = dot(rows[j], rows[p]) for every pair: four partial sums by d mod 4 from +0, d ascending, the product rounded
    and then the sum, joined as (s0 + s1) + (s2 + s3)."""
    n, d = rows.shape
    assert rows.dtype == F and d % 4 == 0
    acc = np.zeros((n, n, 4), dtype=F)
    for d0 in range(0, d, 4):
        acc = acc + rows[:, None, d0:d0 + 4] * rows[None, :, d0:d0 + 4]
    assert acc.dtype == F
    return (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])


def np_mmr_one(scores, idx, c, k, lam, groups=None, cap=0):
    """One query: (out_scores f32 [k], out_idx int64 [k])."""
    scores = np.asarray(scores, dtype=F)
    idx = np.asarray(idx, dtype=np.int64)
    k1, nc = len(scores), c.shape[0]
    valid = (idx >= 0) & (idx < nc) & np.isfinite(scores)
    out_s = np.full(k, -np.inf, dtype=F)
    out_i = np.full(k, -1, dtype=np.int64)
    if not valid.any():
        return out_s, out_i
    rows = np.zeros((k1, c.shape[1]), dtype=F)
    rows[valid] = c[idx[valid]]                                   # invalid candidates are never read from c
    g = np_dot_all(rows)
    n2 = np.diagonal(g).astype(F)
    with np.errstate(divide="ignore"):
        inv = np.where(n2 > 0, F(1.0) / np.sqrt(n2, dtype=F), F(0.0)).astype(F)
    sim = ((g * inv[:, None]).astype(F) * inv[None, :]).astype(F)   # sim[j, p] = (dot * inv_j) * inv_p
    lo, hi = scores[valid].min(), scores[valid].max()
    rel = np.zeros(k1, dtype=F)
    if hi > lo:
        rel[valid] = (scores[valid] - lo) / (hi - lo)
    lam = F(lam)
    om = F(1.0) - lam
    grp = np.full(k1, -1, dtype=np.int64)
    if cap > 0:
        grp[valid] = np.asarray(groups)[idx[valid]]
    pen = np.zeros(k1, dtype=F)
    cnt = np.zeros(k1, dtype=np.int64)
    picked = np.zeros(k1, dtype=bool)
    for t in range(k):
        eligible = valid & ~picked & ~((grp >= 0) & (cnt >= cap))
        if not eligible.any():
            break
        val = (lam * rel).astype(F) - (om * pen).astype(F)
        assert val.dtype == F
        val = np.where(eligible, val, -np.inf)
        p = int(np.argmax(val))                                   # the first of equal maxima: the lower position
        picked[p] = True
        out_s[t], out_i[t] = scores[p], idx[p]
        pen = np.where(valid & (sim[:, p] > pen), sim[:, p], pen).astype(F)
        cnt += valid & (grp >= 0) & (grp == grp[p])
    return out_s, out_i


def np_mmr(scores, idx, c, k, lam, groups=None, cap=0):
    """Batch: scores f32 [nq, k1], idx int64 [nq, k1] -> (f32 [nq, k], int64 [nq, k])."""
    scores, idx = np.atleast_2d(np.asarray(scores, dtype=F)), np.atleast_2d(np.asarray(idx, dtype=np.int64))
    c = np.ascontiguousarray(c, dtype=F)
    outs = [np_mmr_one(s, i, c, k, lam, groups, cap) for s, i in zip(scores, idx)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def exact_pool(q, c, k1):
    """The f64-exact top k1 of every query, (score descending, index ascending): (scores f32 [nq, k1], idx int64 [nq, k1])."""
    s = q.astype(np.float64) @ c.astype(np.float64).T
    order = np.lexsort((np.broadcast_to(np.arange(c.shape[0]), s.shape), -s), axis=1)[:, :k1]
    return np.take_along_axis(s, order, 1).astype(F), order.astype(np.int64)


CLUSTER_N, CLUSTER_D, CLUSTER_GROUPS, CLUSTER_QUERIES, CLUSTER_POOL = 2000, 32, 100, 16, 64


@functools.lru_cache(maxsize=None)
def cluster_corpus():
    """The property test's corpus: 2000 rows around 100 centroids (row r belongs to cluster and group r % 100), rows =
    centroid + 0.3 N(0, 1); 16 queries, each the sum of 4 distinct centroids + 0.1 N(0, 1); the pool of a query is its
    f64-exact top 64.  (c f32 [n, D], groups int32 [n], q f32 [nq, D], pool scores f32 [nq, 64], pool idx int64 [nq, 64]).
    With this generator (default_rng(0): centroids, then row noise, then per query its 4 centroids and its noise) the pools
    span 4 - 8 groups and the mean intra-list cosine of the k = 10 list is 0.771 / 0.535 / 0.276 at lambda = 1 / 0.5 / 0."""
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((CLUSTER_GROUPS, CLUSTER_D))
    groups = (np.arange(CLUSTER_N) % CLUSTER_GROUPS).astype(np.int32)
    c = (cent[groups] + 0.3 * rng.standard_normal((CLUSTER_N, CLUSTER_D))).astype(F)
    q = np.stack([cent[rng.choice(CLUSTER_GROUPS, 4, replace=False)].sum(0) + 0.1 * rng.standard_normal(CLUSTER_D)
                  for _ in range(CLUSTER_QUERIES)]).astype(F)
    s, i = exact_pool(q, c, CLUSTER_POOL)
    for a in (c, groups, q, s, i):
        a.setflags(write=False)
    return c, groups, q, s, i


def intra_list_cosine(c, lists):
    """Mean pairwise cosine (f64) inside every list of corpus rows, averaged over the lists."""
    out = []
    for row in lists:
        x = c[row[row >= 0]].astype(np.float64)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        g = x @ x.T
        n = len(x)
        out.append((g.sum() - n) / (n * (n - 1)))
    return float(np.mean(out))
