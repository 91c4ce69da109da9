"""IVF helpers shared by test_ivf_cpu.py and test_gpu_ivf.py.

- ``clustered``: the seeded clustered synthetic corpus (NumPy).  ``nclusters`` unit directions; item j = direction
  lab_j + noise * N(0, I) / sqrt(d); queries = random items + (noise / 2) * N(0, I) / sqrt(d).  Uniform random vectors
  would give IVF no structure to use.
- ``np_ivf_build`` / ``np_ivf_search``: a NumPy restatement of serving.IVF (spherical k-means on a sample of at most
  256 * nlist items, empty clusters re-seeded from the largest, placement by argmax centroid with ties to the lower list,
  stable order within a list) and of the search (exact top-k over the nprobe best lists, ties to the lower id).  It is the
  yardstick the recall threshold of the GPU test was calibrated with (``recall_at_k``).
- ``union_reference``: the rows of the probed lists of one query, gathered in ascending original id.
"""
import numpy as np

# recall@10 of the NumPy restatement on clustered(**RECALL_CORPUS) with nlist 128, nprobe 16 (= nlist / 8):
# 0.872 at k-means seed 0 (0.60 at nprobe 4, 0.98 at nprobe 64; test_numpy_restatement_recall in test_ivf_cpu.py checks it
# stays above RECALL_MIN for seeds 0..2).  The GPU test requires RECALL_MIN of serving.IVF on the same corpus.
RECALL_CORPUS = dict(n=20_000, d=64, nclusters=200, nq=256, seed=7)
RECALL_NLIST, RECALL_NPROBE, RECALL_K = 128, 16, 10
RECALL_MIN = 0.80


def clustered(n, d, nclusters, nq, seed, noise=1.5):
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((nclusters, d))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    lab = rng.integers(0, nclusters, n)
    x = dirs[lab] + noise * rng.standard_normal((n, d)) / np.sqrt(d)
    q = x[rng.integers(0, n, nq)] + 0.5 * noise * rng.standard_normal((nq, d)) / np.sqrt(d)
    return x.astype(np.float32), q.astype(np.float32)


def _argmax_lower(s):
    return np.argmax(s, axis=1)                       # first maximum: ties to the lower list


def np_ivf_build(x, nlist, seed=0, iters=10):
    rng = np.random.default_rng(seed)
    n = x.shape[0]
    m = min(n, 256 * nlist)
    sample = x[np.sort(rng.permutation(n)[:m])].astype(np.float64)
    cent = sample[rng.permutation(m)[:nlist]]
    cent /= np.maximum(np.linalg.norm(cent, axis=1, keepdims=True), 1e-300)
    for _ in range(iters):
        a = _argmax_lower(sample @ cent.T)
        sums = np.zeros_like(cent)
        np.add.at(sums, a, sample)
        counts = np.bincount(a, minlength=nlist)
        norms = np.linalg.norm(sums, axis=1)
        new = sums / np.maximum(norms, 1e-300)[:, None]
        empty = np.nonzero((counts == 0) | (norms == 0))[0]
        if len(empty):
            new[empty] = new[np.argmax(counts)] + 0.05 * rng.standard_normal((len(empty), x.shape[1]))
        cent = new / np.linalg.norm(new, axis=1, keepdims=True)
    a = _argmax_lower(x.astype(np.float64) @ cent.T)
    order = np.argsort(a, kind="stable")
    offsets = np.zeros(nlist + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(a, minlength=nlist))
    return cent, offsets, order


def np_ivf_search(q, x, cent, offsets, order, k, nprobe):
    """(ids [nq, k] int64, -1 padded) of the exact top-k over the nprobe best lists (f64 scores)."""
    out = np.full((q.shape[0], k), -1, dtype=np.int64)
    cs = q.astype(np.float64) @ cent.T
    for r in range(q.shape[0]):
        probes = np.lexsort((np.arange(cent.shape[0]), -cs[r]))[:nprobe]
        ids = np.sort(np.concatenate([order[offsets[l]:offsets[l + 1]] for l in probes]))
        s = x[ids].astype(np.float64) @ q[r].astype(np.float64)
        best = ids[np.lexsort((ids, -s))[:k]]
        out[r, :len(best)] = best
    return out


def exact_topk_ids(q, x, k):
    s = q.astype(np.float64) @ x.astype(np.float64).T
    return np.stack([np.lexsort((np.arange(x.shape[0]), -s[r]))[:k] for r in range(q.shape[0])])


def recall_at_k(got, exact):
    """Mean over queries of |got_r & exact_r| / k (padding -1 never counts)."""
    k = exact.shape[1]
    return float(np.mean([len(set(g[g >= 0].tolist()) & set(e.tolist())) / k for g, e in zip(got, exact)]))


def union_reference(list_ids, offsets, probes):
    """Original ids of the probed lists' rows, ascending (the corpus order tt_retrieval_topk_f32 sees in the reference)."""
    return np.sort(np.concatenate([list_ids[offsets[l]:offsets[l + 1]] for l in probes]))
