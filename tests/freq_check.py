"""Restatement of the streaming frequency estimator's contract of include/twotower_hip.h (tt_frequency_estimate_i64), shared by
tests/test_freq_cpu.py and tests/test_gpu_freq.py.  Vectorised NumPy, f32 operation by operation (NumPy's f32 * + / are
correctly rounded, like __fmul_rn / __fadd_rn / __fdiv_rn), so the device's sketch words and probabilities are compared with it
bit for bit.

The sketch is the pair (``last`` int32 [H, M], ``delta`` f32 [H, M]); ``pack`` / ``unpack`` turn it into / out of the device's
int64 words (low half ``last``, high half the bits of ``delta``).

* ``slots_of``  the slot of every id under every hash: ((x >> 32) * M) >> 32, x = element (uint64)id of the stream
                (seed, tensor_id + h) of oracle.synth.
* ``update``    step 1 of the contract: every slot hit by an in-range id whose last != t is updated exactly once.
* ``estimate``  step 2: D = max over the hashes of (last == 0 ? (float)t : delta).
* ``call``      one whole call: update with ids[:n_update], estimate all, the output formula; returns (prob f32 [n], flag 0/1).
"""
import numpy as np

from oracle import synth

TID_FREQ_HASH_BASE = 56             # the trainer's tensor id of hash row 0


def new_sketch(hashes, slots):
    return np.zeros((hashes, slots), dtype=np.int32), np.zeros((hashes, slots), dtype=np.float32)


def pack(last, delta):
    lo = np.ascontiguousarray(last, dtype=np.int32).view(np.uint32).astype(np.uint64)
    hi = np.ascontiguousarray(delta, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((hi << np.uint64(32)) | lo).view(np.int64)


def unpack(words):
    w = np.ascontiguousarray(words, dtype=np.int64).view(np.uint64)
    last = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    delta = (w >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return last, delta


def in_range(ids, n_items):
    ids = np.asarray(ids, dtype=np.int64)
    return (ids >= 0) & (ids < n_items)


def slots_of(ids, hashes, slots, seed, tensor_id):
    """int64 [hashes, len(ids)]; ids are taken as uint64 (an id out of range hashes somewhere too - nobody reads that slot)."""
    x = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    out = np.empty((hashes, len(x)), dtype=np.int64)
    with np.errstate(over="ignore"):
        for h in range(hashes):
            m = synth.mix(synth.stream_key(seed, tensor_id + h) + x)
            out[h] = (((m >> np.uint64(32)) * np.uint64(slots)) >> np.uint64(32)).astype(np.int64)
    return out


def update(last, delta, ids, t, alpha, n_items, seed, tensor_id):
    """In place.  1 - alpha is formed once, in f32."""
    ids = np.asarray(ids, dtype=np.int64)
    ids = ids[in_range(ids, n_items)]
    hashes, slots = last.shape
    a = np.float32(alpha)
    oma = np.float32(1.0) - a
    s = slots_of(ids, hashes, slots, seed, tensor_id)
    for h in range(hashes):
        hit = np.unique(s[h])
        hit = hit[last[h, hit] != t]
        old = last[h, hit]
        gap = (np.int64(t) - old.astype(np.int64)).astype(np.float32)
        moved = (oma * delta[h, hit]).astype(np.float32) + (a * gap).astype(np.float32)
        delta[h, hit] = np.where(old == 0, gap, moved).astype(np.float32)
        last[h, hit] = t


def estimate(last, delta, ids, t, n_items, seed, tensor_id):
    """D f32 [len(ids)] (anything where the id is out of range)."""
    hashes, slots = last.shape
    s = slots_of(ids, hashes, slots, seed, tensor_id)
    rows = np.arange(hashes)[:, None]
    d = np.where(last[rows, s] == 0, np.float32(t), delta[rows, s]).astype(np.float32)
    return d.max(axis=0)


def call(last, delta, ids, n_update, t, alpha, n_items, seed, tensor_id, sampler_prob=None, mix=False):
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    assert 0 <= n_update <= n and t >= 1 and 0.0 < alpha <= 1.0 and (not mix or 1 <= n_update < n)
    ok = in_range(ids, n_items)
    update(last, delta, ids[:n_update], t, alpha, n_items, seed, tensor_id)
    big = estimate(last, delta, ids, t, n_items, seed, tensor_id)
    p = (np.float32(1.0) / big).astype(np.float32)
    if mix:
        safe = np.where(ok, ids, 0)
        u = np.float32(1.0) / np.float32(n_items) if sampler_prob is None else np.asarray(sampler_prob, dtype=np.float32)[safe]
        p = ((p + (np.float32(n - n_update) * u).astype(np.float32)).astype(np.float32) / np.float32(n)).astype(np.float32)
    return np.where(ok, p, np.float32(1.0)).astype(np.float32), int((~ok).any())
