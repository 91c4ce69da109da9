"""Restatements of the mixed-negative-sampling contract of include/twotower_hip.h (tt_sample_candidates_i64), shared by
tests/test_sample_cpu.py and tests/test_gpu_sample.py.

* ``draw`` is the sampler: element start + i of the stream (seed, tensor_id) of oracle.synth, the uniform bucket
  ((x >> 32) * n_items) >> 32, and with an alias table u = (x & 0xFFFFFF) * 2^-24, id = bucket if u < thr[bucket] else idx[bucket].
  Integer arithmetic and one exact f32 product: the device's ids are compared with it exactly.
* ``mixture_prob`` is the probability the kernel writes for a candidate, in f32 operation by operation (NumPy's f32 * + / are
  correctly rounded, like __fmul_rn / __fadd_rn / __fdiv_rn): fl(fl(fl(B * f) + fl(N * u)) / fl(B + N)), 1.0 for an id out of range.
* ``alias_distribution`` is the distribution an alias table implies when u lives on the 2^-24 grid, computed exactly.
* ``mixed_step`` is one train step's forward and backward pass with the item side over the candidate list, from the functions of
  oracle.two_tower (which take more candidates than queries, candidate ids and candidate probabilities) in f64.
"""
import numpy as np

from oracle import synth, two_tower as tt

TID_SAMPLED_NEGATIVES = 10          # the trainer's tensor id of the sampled-negative stream
U24 = 2.0 ** -24


def raw(seed, tensor_id, start, n):
    """Elements start .. start + n - 1 of the stream, the counter taken mod 2^64."""
    key = synth.stream_key(seed, tensor_id)
    with np.errstate(over="ignore"):
        idx = np.uint64(start % (1 << 64)) + np.arange(n, dtype=np.uint64)
        return synth.mix(key + idx)


def draw(seed, tensor_id, start, n, n_items, alias=None):
    """int64 [n]: the sampled ids.  ``alias`` = (thr f32 [n_items], idx int32 [n_items]) or None (uniform)."""
    x = raw(seed, tensor_id, start, n)
    b = (((x >> np.uint64(32)) * np.uint64(n_items)) >> np.uint64(32)).astype(np.int64)
    if alias is None:
        return b
    thr, idx = alias
    u = (x & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(U24)
    return np.where(u < np.asarray(thr, dtype=np.float32)[b], b, np.asarray(idx)[b].astype(np.int64))


def mixture_prob(ids, n_pos, n_neg, n_items, freq_at, sampler_prob_at=None):
    """f32 [len(ids)]: ``freq_at`` / ``sampler_prob_at`` hold item_freq[id] / sampler_prob[id] of every candidate (anything where
    the id is out of range); sampler_prob_at None = the uniform sampler's fl(1 / fl(n_items))."""
    ids = np.asarray(ids)
    f = np.asarray(freq_at, dtype=np.float32)
    u = np.float32(1.0) / np.float32(n_items) if sampler_prob_at is None else np.asarray(sampler_prob_at, dtype=np.float32)
    p = (np.float32(n_pos) * f + np.float32(n_neg) * u) / np.float32(n_pos + n_neg)
    ok = (ids >= 0) & (ids < n_items)
    return np.where(ok, p, np.float32(1.0)).astype(np.float32)


def candidates(pos_ids, n_items, n_neg, seed, tensor_id, start, alias=None, item_freq=None, sampler_prob=None):
    """(cand_ids int64 [B + N], cand_prob f32 [B + N] or None, flag 0/1) from whole [n_items] vectors."""
    pos_ids = np.asarray(pos_ids, dtype=np.int64)
    ids = np.concatenate([pos_ids, draw(seed, tensor_id, start, n_neg, n_items, alias)])
    ok = (ids >= 0) & (ids < n_items)
    prob = None
    if item_freq is not None:
        safe = np.where(ok, ids, 0)
        prob = mixture_prob(ids, len(pos_ids), n_neg, n_items, np.asarray(item_freq)[safe],
                            None if sampler_prob is None else np.asarray(sampler_prob)[safe])
    return ids, prob, int((~ok).any())


def alias_distribution(thr, idx):
    """(p f64 [n], indegree int [n]): bucket b is drawn with probability 1/n and keeps its own item for the m_b = #{u on the
    2^-24 grid : u < thr[b]} = ceil(thr[b] * 2^24) of the 2^24 values of u; the rest goes to idx[b]."""
    thr = np.asarray(thr, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    n = len(thr)
    m = np.clip(np.ceil(thr * 2.0 ** 24), 0, 2.0 ** 24)
    own = m * U24
    p = own.copy()
    np.add.at(p, idx, 1.0 - own)
    indegree = np.bincount(idx[own < 1.0], minlength=n)
    return p / n, indegree


def l2n(x, eps=1e-12):
    s = (x * x).sum(axis=1, keepdims=True)
    return x / np.sqrt(np.maximum(s, eps))


def l2n_grad(x, dy, eps=1e-12):
    s = (x * x).sum(axis=1, keepdims=True)
    t = (x * dy).sum(axis=1, keepdims=True)
    inv = 1.0 / np.sqrt(np.maximum(s, eps))
    return np.where(s >= eps, inv * (dy - x * (t * inv * inv)), dy * inv)


def mixed_step(state, user_ids, cand_ids, temperature, cand_prob=None, relu_masks=None, normalize=False, sample_weight=None):
    """Forward + backward of one mixed step on an oracle.two_tower.ModelState (f64): B queries against the B + N candidates
    ``cand_ids`` (the positive of query i is candidate i), accidental hits removed, the logQ correction with ``cand_prob``.
    Returns loss, q, c, dq, dc, due, die and the towers' kernel / bias gradients (no l2 term)."""
    ua = tt.tower_fwd(tt.embedding_gather(state.user_table, user_ids), state.user_tower.weights, state.user_tower.biases)
    ia = tt.tower_fwd(tt.embedding_gather(state.item_table, cand_ids), state.item_tower.weights, state.item_tower.biases)
    q, c = (l2n(ua[-1]), l2n(ia[-1])) if normalize else (ua[-1], ia[-1])
    kw = dict(temperature=temperature, sample_weight=sample_weight, candidate_sampling_probability=cand_prob,
              candidate_ids=cand_ids, remove_accidental_hits=True, dtype=q.dtype)
    loss = tt.retrieval_loss(q, c, **kw)[0]
    dq, dc = tt.retrieval_grad(q, c, **kw)
    gq, gc = (l2n_grad(ua[-1], dq), l2n_grad(ia[-1], dc)) if normalize else (dq, dc)
    um, im = (None, None) if relu_masks is None else relu_masks
    due, udw, udb = tt.tower_bwd(ua, state.user_tower.weights, gq, um)
    die, idw, idb = tt.tower_bwd(ia, state.item_tower.weights, gc, im)
    return dict(loss=loss, q=q, c=c, dq=dq, dc=dc, due=due, die=die, udw=udw, udb=udb, idw=idw, idb=idb)
