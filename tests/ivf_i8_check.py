"""Int8 IVF helpers shared by test_ivf_i8_cpu.py and test_gpu_ivf_i8.py: the NumPy restatement of the search, composed of the
restatements of its two parents (ivf_check.py: lists and probes; int8_check.py: quantiser, keys and stage-1 order).

``np_ivf_i8_search``: per query, the probed lists' rows gathered in ascending original id, the k1 best by (int8 key
descending, id ascending), re-ranked in f64 (calibration only: the GPU re-rank is the f32 MFMA chain), best k."""
import numpy as np

from int8_check import np_keys, np_quantize

RECALL_CASES = [(10, 32), (10, 40), (100, 256)]      # (k, k1): rerank 4 at k = 10 gives 40; 32 is default_k1's floor


def np_ivf_i8_search(q, x, cent, offsets, order, k, k1, nprobe):
    """(ids [nq, k] int64, -1 padded)."""
    codes, scales = np_quantize(x)
    qc, _ = np_quantize(q)
    out = np.full((q.shape[0], k), -1, dtype=np.int64)
    cs = q.astype(np.float64) @ cent.T
    for r in range(q.shape[0]):
        probes = np.lexsort((np.arange(cent.shape[0]), -cs[r]))[:nprobe]
        ids = np.sort(np.concatenate([order[offsets[l]:offsets[l + 1]] for l in probes]))
        keys = np_keys(qc[r:r + 1], codes[ids], scales[ids])[0]
        cand = ids[np.lexsort((ids, -keys))[:k1]]
        s = x[cand].astype(np.float64) @ q[r].astype(np.float64)
        best = cand[np.lexsort((cand, -s))[:k]]
        out[r, :len(best)] = best
    return out
