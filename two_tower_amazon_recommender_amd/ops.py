"""Tensor-level wrappers over the C ABI (``include/twotower_hip.h``).

PyTorch is plumbing here: it owns device memory and the HIP stream; every op below
hands raw device pointers and the current stream to ``libtwotower_hip.so``.  There is
no eager/PyTorch fallback — a missing library or a CPU tensor raises.

Reference anchors: the ops are what ``src/models`` / ``src/training`` of the reference
(docstring stubs, ``src/models/__init__.py:1``) would have run through TensorFlow /
TFRS for the config in ``configs/data_config.yaml:54-71``.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import DenseSeg, TT_OPT_ADAGRAD, TT_OPT_SGD

_OPT = {"sgd": TT_OPT_SGD, "adagrad": TT_OPT_ADAGRAD}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, dtype, name: str, ndim: int | None = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA/HIP tensor (there is no CPU fallback), got device {t.device}")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")
    return t


def _p(t):
    return None if t is None else t.data_ptr()


# ----------------------------------------------------------------------------- synthetic
def fill_uniform_(dst: torch.Tensor, seed: int, tensor_id: int, lo: float, scale: float, start: int = 0):
    """dst.flat[i] = fl32(fl32(u(start+i)*scale)+lo); bit-identical to oracle.synth.uniform_f32."""
    _chk(dst, torch.float32, "dst")
    lib = _lib.load()
    _lib.check(lib.tt_fill_uniform_f32(_p(dst), dst.numel(), seed, tensor_id, start, lo, scale, _stream()),
               "tt_fill_uniform_f32")
    return dst


def fill_uniform_rows_(dst: torch.Tensor, seed: int, tensor_id: int, lo: float, scale: float, row_start: int, row_stride: int):
    """dst[lr, :] = row (row_start + lr*row_stride) of the synthetic [*, dim] tensor (a row-sharded table's shard)."""
    _chk(dst, torch.float32, "dst", 2)
    lib = _lib.load()
    _lib.check(lib.tt_fill_uniform_rows_f32(_p(dst), dst.shape[0], dst.shape[1], row_start, row_stride, seed, tensor_id,
                                            lo, scale, _stream()), "tt_fill_uniform_rows_f32")
    return dst


def fill_ids_(dst: torch.Tensor, seed: int, tensor_id: int, num_rows: int, variant: str = "U", start: int = 0):
    _chk(dst, torch.int64, "dst")
    v = {"U": _lib.TT_IDS_UNIFORM, "Z": _lib.TT_IDS_POWERLAW}[variant]
    lib = _lib.load()
    _lib.check(lib.tt_fill_ids_i64(_p(dst), dst.numel(), seed, tensor_id, start, num_rows, v, _stream()),
               "tt_fill_ids_i64")
    return dst


# ----------------------------------------------------------------------------- a6/a7 id encoding
def strings_to_padded_bytes(values) -> "torch.Tensor":
    """Host helper: list of str -> zero-padded [n, width] uint8 matrix of UTF-8 bytes (width a multiple of 8)."""
    import numpy as np
    enc = [v.encode("utf-8") for v in values]
    width = max(8, (max((len(b) for b in enc), default=1) + 7) // 8 * 8)
    mat = np.zeros((len(enc), width), dtype=np.uint8)
    for i, b in enumerate(enc):
        if b"\0" in b:
            raise ValueError("id strings must not contain NUL bytes")
        mat[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return torch.from_numpy(mat)


def encode_ids(rows_u8: torch.Tensor):
    """codes[i] = rank of row i among the sorted distinct rows (the reference's sorted-enumerate / LabelEncoder ids).
    Returns (int64 codes [n], int32 n_unique [1]) on the device."""
    _chk(rows_u8, torch.uint8, "rows_u8", 2)
    n, width = rows_u8.shape
    lib = _lib.load()
    ws = torch.empty(int(lib.tt_encode_ids_workspace_bytes(n)), dtype=torch.uint8, device=rows_u8.device)
    codes = torch.empty(n, dtype=torch.int64, device=rows_u8.device)
    nuniq = torch.zeros(1, dtype=torch.int32, device=rows_u8.device)
    _lib.check(lib.tt_encode_ids_u8(_p(rows_u8), n, width, _p(ws), ws.numel(), _p(codes), _p(nuniq), _stream()),
               "tt_encode_ids_u8")
    return codes, nuniq


# ----------------------------------------------------------------------------- a1 gather
def embedding_gather(table: torch.Tensor, ids: torch.Tensor, out: torch.Tensor | None = None,
                     oob_flag: torch.Tensor | None = None) -> torch.Tensor:
    """out[b,:] = table[ids[b],:].  ``oob_flag`` (int32[1]) is set to 1 on any out-of-range id."""
    _chk(table, torch.float32, "table", 2)
    _chk(ids, torch.int64, "ids", 1)
    n, d = ids.numel(), table.shape[1]
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=table.device)
    _chk(out, torch.float32, "out", 2)
    if tuple(out.shape) != (n, d):
        raise RuntimeError(f"embedding_gather: out must be [{n}, {d}] (n_ids, dim), got {tuple(out.shape)}")
    if oob_flag is not None:
        _chk(oob_flag, torch.int32, "oob_flag")
    lib = _lib.load()
    _lib.check(lib.tt_embedding_gather_f32(_p(table), table.shape[0], d, _p(ids), n, _p(out), _p(oob_flag), _stream()),
               "tt_embedding_gather_f32")
    return out


def embedding_gather2(table_a, ids_a, out_a, table_b, ids_b, out_b, oob_flag=None):
    """Both towers' lookups in one launch."""
    for t, nme in ((table_a, "table_a"), (table_b, "table_b"), (out_a, "out_a"), (out_b, "out_b")):
        _chk(t, torch.float32, nme, 2)
    _chk(ids_a, torch.int64, "ids_a", 1)
    _chk(ids_b, torch.int64, "ids_b", 1)
    if ids_a.numel() != ids_b.numel() or table_a.shape[1] != table_b.shape[1]:
        raise RuntimeError("embedding_gather2: both lookups must share n_ids and dim")
    want = (ids_a.numel(), table_a.shape[1])
    if tuple(out_a.shape) != want or tuple(out_b.shape) != want:
        raise RuntimeError(f"embedding_gather2: outputs must be [{want[0]}, {want[1]}] (n_ids, dim), got "
                           f"{tuple(out_a.shape)} and {tuple(out_b.shape)}")
    lib = _lib.load()
    _lib.check(lib.tt_embedding_gather2_f32(_p(table_a), table_a.shape[0], _p(ids_a), _p(out_a),
                                            _p(table_b), table_b.shape[0], _p(ids_b), _p(out_b),
                                            table_a.shape[1], ids_a.numel(), _p(oob_flag), _stream()),
               "tt_embedding_gather2_f32")
    return out_a, out_b


def embedding_gather_add_(out, table, ids, oob_flag=None):
    """out[p, :] += table[ids[p], :] — a further feature summed into a tower input (hashed category, cfg5)."""
    _chk(table, torch.float32, "table", 2)
    _chk(ids, torch.int64, "ids", 1)
    _chk(out, torch.float32, "out", 2)
    if out.shape[0] != ids.numel() or out.shape[1] != table.shape[1]:
        raise RuntimeError("embedding_gather_add_: out must be [n_ids, dim]")
    lib = _lib.load()
    _lib.check(lib.tt_embedding_gather_add_f32(_p(table), table.shape[0], table.shape[1], _p(ids), ids.numel(), _p(out),
                                               _p(oob_flag), _stream()), "tt_embedding_gather_add_f32")
    return out


def hash_buckets(rows_u8: torch.Tensor, n_buckets: int) -> torch.Tensor:
    """int64 bucket of every zero-padded byte row: FNV-1a-64 mod n_buckets (oracle/hashing.py)."""
    _chk(rows_u8, torch.uint8, "rows_u8", 2)
    n, width = rows_u8.shape
    out = torch.empty(n, dtype=torch.int64, device=rows_u8.device)
    lib = _lib.load()
    _lib.check(lib.tt_hash_bucket_u8(_p(rows_u8), n, width, n_buckets, _p(out), _stream()), "tt_hash_bucket_u8")
    return out


# ----------------------------------------------------------------------------- embedding bag (pooled item titles)
POOLINGS = {"sum": _lib.TT_POOL_SUM, "mean": _lib.TT_POOL_MEAN, "sqrtn": _lib.TT_POOL_SQRTN}


def _bag_args(what, table, tokens, bag_rows, pooling, out, accumulate, batch_ids, inv, oob_flag):
    """The argument checks the two bag forward ops share; returns (n_token_rows, L, dim, n_bags, out)."""
    _chk(table, torch.float32, "table", 2)
    _chk(tokens, torch.int32, "tokens", 2)
    if pooling not in POOLINGS:
        raise ValueError(f"{what}: pooling must be one of {tuple(POOLINGS)}, got {pooling!r}")
    n_rows, L = tokens.shape
    d = table.shape[1]
    if bag_rows is not None:
        _chk(bag_rows, torch.int64, "bag_rows", 1)
    n_bags = n_rows if bag_rows is None else bag_rows.numel()
    if out is None:
        if accumulate:
            raise ValueError(f"{what}: accumulate=True adds into `out`, which must be given")
        out = torch.empty((n_bags, d), dtype=torch.float32, device=table.device)
    _chk(out, torch.float32, "out", 2)
    if tuple(out.shape) != (n_bags, d):
        raise RuntimeError(f"{what}: out must be [{n_bags}, {d}] (n_bags, dim), got {tuple(out.shape)}")
    if batch_ids is not None:
        _chk(batch_ids, torch.int64, "batch_ids")
        if batch_ids.numel() != n_bags * L:
            raise RuntimeError(f"{what}: batch_ids must hold n_bags * L = {n_bags * L} entries, got {batch_ids.numel()}")
    if inv is not None:
        _chk(inv, torch.float32, "inv", 1)
        if inv.numel() != n_bags:
            raise RuntimeError(f"{what}: inv must hold n_bags = {n_bags} entries, got {inv.numel()}")
    if oob_flag is not None:
        _chk(oob_flag, torch.int32, "oob_flag")
    return n_rows, L, d, n_bags, out


def embedding_bag(table: torch.Tensor, tokens: torch.Tensor, bag_rows: torch.Tensor | None = None, pooling: str = "mean",
                  out: torch.Tensor | None = None, accumulate: bool = False, batch_ids: torch.Tensor | None = None,
                  inv: torch.Tensor | None = None, oob_flag: torch.Tensor | None = None) -> torch.Tensor:
    """out[b, :] (+)= pool(table[t, :] for the valid tokens t of row bag_rows[b] of ``tokens``) - ``tt_embedding_bag_fwd_f32``.
    ``tokens`` [n_token_rows, L] int32, -1 = padding (anywhere in a row); ``bag_rows`` [n_bags] int64 (None: bag b is row b;
    -1: an empty bag); ``pooling`` "sum" | "mean" | "sqrtn"; ``accumulate`` adds into ``out`` (which must then be given).
    Optional outputs: ``batch_ids`` [n_bags * L] int64 (every slot's token, -1 where skipped: what the sort plan sorts) and
    ``inv`` [n_bags] f32 (the pooling scale; 0 for an empty bag).  ``oob_flag`` (int32[1]) is set on any token or bag row out
    of range."""
    n_rows, L, d, n_bags, out = _bag_args("embedding_bag", table, tokens, bag_rows, pooling, out, accumulate, batch_ids, inv, oob_flag)
    _lib.check(_lib.load().tt_embedding_bag_fwd_f32(_p(table), table.shape[0], d, _p(tokens), n_rows, L, _p(bag_rows), n_bags,
                                                    POOLINGS[pooling], int(bool(accumulate)), _p(out), _p(batch_ids), _p(inv),
                                                    _p(oob_flag), _stream()), "tt_embedding_bag_fwd_f32")
    return out


def history_bag(table: torch.Tensor, tokens: torch.Tensor, bag_rows: torch.Tensor | None = None,
                exclude: torch.Tensor | None = None, base=None, pooling: str = "mean", out: torch.Tensor | None = None,
                accumulate: bool = False, batch_ids: torch.Tensor | None = None, inv: torch.Tensor | None = None,
                oob_flag: torch.Tensor | None = None) -> torch.Tensor:
    """``embedding_bag`` with leave-one-out and a base row, in one launch (``tt_history_bag_fwd_f32``): the pooled user-history
    feature.  ``exclude`` [n_bags] int64: bag b skips every slot whose token equals exclude[b] (written to ``batch_ids`` as -1,
    not counted).  ``base`` = (base_table [rows, dim] f32, base_ids [n_bags] int64): out[b] = base_table[base_ids[b]] + pooled
    (an out-of-range base id: a zero row and the flag); it takes the place of ``accumulate``, which must then be False.
    Every other argument is ``embedding_bag``'s."""
    if base is not None and accumulate:
        raise ValueError("history_bag: the base row takes the place of out's row: accumulate must be False with a base")
    n_rows, L, d, n_bags, out = _bag_args("history_bag", table, tokens, bag_rows, pooling, out, accumulate, batch_ids, inv, oob_flag)
    if exclude is not None:
        _chk(exclude, torch.int64, "exclude", 1)
        if exclude.numel() != n_bags:
            raise RuntimeError(f"history_bag: exclude must hold n_bags = {n_bags} entries, got {exclude.numel()}")
    base_table = base_ids = None
    if base is not None:
        base_table, base_ids = base
        _chk(base_table, torch.float32, "base_table", 2)
        _chk(base_ids, torch.int64, "base_ids", 1)
        if base_table.shape[1] != d or base_ids.numel() != n_bags:
            raise RuntimeError(f"history_bag: base must be ([rows, {d}] f32, [{n_bags}] int64), got {tuple(base_table.shape)} "
                               f"and {tuple(base_ids.shape)}")
    _lib.check(_lib.load().tt_history_bag_fwd_f32(_p(table), table.shape[0], d, _p(tokens), n_rows, L, _p(bag_rows), n_bags,
                                                  POOLINGS[pooling], int(bool(accumulate)), _p(out), _p(batch_ids), _p(inv),
                                                  _p(oob_flag), _p(exclude), _p(base_table),
                                                  0 if base_table is None else base_table.shape[0], _p(base_ids), _stream()),
               "tt_history_bag_fwd_f32")
    return out


def history_attention(table: torch.Tensor, tokens: torch.Tensor, attn: torch.Tensor, bag_rows: torch.Tensor | None = None,
                      exclude: torch.Tensor | None = None, base=None, out: torch.Tensor | None = None,
                      batch_ids: torch.Tensor | None = None, weights: torch.Tensor | None = None,
                      pooled: torch.Tensor | None = None, oob_flag: torch.Tensor | None = None):
    """The history bag pooled by a learned query with a recency bias, in one launch (``tt_history_attention_fwd_f32``):
    ``attn`` [dim + L] f32 = [a | p]; for the valid slots j of a bag (``history_bag``'s rules: padding, out-of-range tokens and
    ``exclude`` skipped) r_j = valid slots behind j, e_j = <table[t_j], a> / sqrt(dim) + p[r_j], w = softmax(e),
    out[b] = base row + sum_j w_j table[t_j].  ``tokens``, ``bag_rows``, ``exclude``, ``base``, ``batch_ids`` and ``oob_flag``
    are ``history_bag``'s; ``weights`` [n_bags, L] (0 in a skipped slot) and ``pooled`` [n_bags, dim] (the pooled term without
    the base row) are allocated when None.  dim a multiple of 4 in 4..1024, L in 1..64.  Returns (out, weights, pooled)."""
    n_rows, L, d, n_bags, out = _bag_args("history_attention", table, tokens, bag_rows, "sum", out, False, batch_ids, None, oob_flag)
    _chk(attn, torch.float32, "attn", 1)
    if attn.numel() != d + L:
        raise RuntimeError(f"history_attention: attn must hold dim + L = {d + L} entries ([a | p]), got {attn.numel()}")
    if exclude is not None:
        _chk(exclude, torch.int64, "exclude", 1)
        if exclude.numel() != n_bags:
            raise RuntimeError(f"history_attention: exclude must hold n_bags = {n_bags} entries, got {exclude.numel()}")
    base_table = base_ids = None
    if base is not None:
        base_table, base_ids = base
        _chk(base_table, torch.float32, "base_table", 2)
        _chk(base_ids, torch.int64, "base_ids", 1)
        if base_table.shape[1] != d or base_ids.numel() != n_bags:
            raise RuntimeError(f"history_attention: base must be ([rows, {d}] f32, [{n_bags}] int64), got "
                               f"{tuple(base_table.shape)} and {tuple(base_ids.shape)}")
    if weights is None:
        weights = torch.empty((n_bags, L), dtype=torch.float32, device=table.device)
    _chk(weights, torch.float32, "weights", 2)
    if tuple(weights.shape) != (n_bags, L):
        raise RuntimeError(f"history_attention: weights must be [{n_bags}, {L}] (n_bags, L), got {tuple(weights.shape)}")
    if pooled is None:
        pooled = torch.empty((n_bags, d), dtype=torch.float32, device=table.device)
    _chk(pooled, torch.float32, "pooled", 2)
    if tuple(pooled.shape) != (n_bags, d):
        raise RuntimeError(f"history_attention: pooled must be [{n_bags}, {d}] (n_bags, dim), got {tuple(pooled.shape)}")
    _lib.check(_lib.load().tt_history_attention_fwd_f32(_p(table), table.shape[0], d, _p(tokens), n_rows, L, _p(bag_rows), n_bags,
                                                        _p(attn), _p(out), _p(batch_ids), _p(weights), _p(pooled), _p(oob_flag),
                                                        _p(exclude), _p(base_table),
                                                        0 if base_table is None else base_table.shape[0], _p(base_ids), _stream()),
               "tt_history_attention_fwd_f32")
    return out, weights, pooled


def history_attention_num_slabs(n: int) -> int:
    """Slab count of ``history_attention_bwd`` for ``n`` bags (``tt_history_attention_num_slabs``, a host query)."""
    return int(_lib.load().tt_history_attention_num_slabs(n))


def history_attention_bwd(table: torch.Tensor, batch_ids: torch.Tensor, weights: torch.Tensor, pooled: torch.Tensor,
                          dy: torch.Tensor, attn: torch.Tensor, L: int, slot_grads: torch.Tensor | None = None,
                          dattn_slabs: torch.Tensor | None = None):
    """The backward launch of ``history_attention`` (``tt_history_attention_bwd_f32``) from the forward's ``batch_ids``,
    ``weights`` and ``pooled`` and ``dy`` [n_bags, dim]: ``slot_grads`` [n_bags * L, dim] gets ONE gradient row per kept slot
    (w_j dy[b] + de_j a / sqrt(dim), de_j = w_j (<dy[b], h_j> - <dy[b], pooled[b]>); a skipped slot's row is left untouched) -
    what ``sparse_sgd_`` / ``sparse_adagrad_`` / ``adam_step_`` take with a plain ``SparsePlan(n_bags * L)`` run over
    ``batch_ids`` - and ``dattn_slabs`` [n_slabs, dim + L] the gradient of ``attn`` as slabs over contiguous bags, every slab
    written in full: the form ``make_dense_seg`` / ``make_adam_seg`` sum.  Both are allocated when None (the slot rows
    uninitialised, ``history_attention_num_slabs(n_bags)`` slabs).  Returns (slot_grads, dattn_slabs)."""
    _chk(table, torch.float32, "table", 2)
    _chk(batch_ids, torch.int64, "batch_ids")
    _chk(weights, torch.float32, "weights", 2)
    _chk(pooled, torch.float32, "pooled", 2)
    _chk(dy, torch.float32, "dy", 2)
    _chk(attn, torch.float32, "attn", 1)
    n_bags, d = dy.shape
    L = int(L)
    if table.shape[1] != d or tuple(pooled.shape) != (n_bags, d):
        raise RuntimeError(f"history_attention_bwd: dy and pooled must be [n_bags, dim] with the table's dim {table.shape[1]}, got "
                           f"{tuple(dy.shape)} and {tuple(pooled.shape)}")
    if tuple(weights.shape) != (n_bags, L) or batch_ids.numel() != n_bags * L:
        raise RuntimeError(f"history_attention_bwd: weights must be [{n_bags}, {L}] and batch_ids hold {n_bags * L} entries, got "
                           f"{tuple(weights.shape)} and {batch_ids.numel()}")
    if attn.numel() != d + L:
        raise RuntimeError(f"history_attention_bwd: attn must hold dim + L = {d + L} entries, got {attn.numel()}")
    if slot_grads is None:
        slot_grads = torch.empty((n_bags * L, d), dtype=torch.float32, device=table.device)
    _chk(slot_grads, torch.float32, "slot_grads", 2)
    if tuple(slot_grads.shape) != (n_bags * L, d):
        raise RuntimeError(f"history_attention_bwd: slot_grads must be [{n_bags * L}, {d}] (n_bags * L, dim), got {tuple(slot_grads.shape)}")
    if dattn_slabs is None:
        dattn_slabs = torch.empty((history_attention_num_slabs(n_bags), d + L), dtype=torch.float32, device=table.device)
    _chk(dattn_slabs, torch.float32, "dattn_slabs", 2)
    if dattn_slabs.shape[0] < 1 or dattn_slabs.shape[1] != d + L:
        raise RuntimeError(f"history_attention_bwd: dattn_slabs must be [n_slabs, {d + L}] (dim + L), got {tuple(dattn_slabs.shape)}")
    _lib.check(_lib.load().tt_history_attention_bwd_f32(_p(table), table.shape[0], d, L, _p(batch_ids), _p(weights), _p(pooled),
                                                        _p(dy), n_bags, _p(attn), _p(slot_grads), _p(dattn_slabs),
                                                        dattn_slabs.shape[0], _stream()), "tt_history_attention_bwd_f32")
    return slot_grads, dattn_slabs


class GruBuffers:
    """What ``history_gru(keep=...)`` leaves for ``history_gru_bwd``, for ``n_bags`` bags of ``L`` slots at width ``dim``:
    ``batch_ids`` [n_bags * L] int64 (the slots' tokens, -1 where skipped), ``x`` [n_bags * L, dim] (the slot rows, zeros where
    skipped), ``gates`` [n_bags * L, 3 dim] (the input projection, overwritten in place by z | r | n of every kept slot),
    ``gn`` [n_bags * L, dim] (g_n of every kept slot), ``hprev`` [n_bags * L, dim] (h_{t-1} of every slot) and the backward's
    ``da`` / ``dg`` [n_bags * L, 3 dim].  4 * n_bags * L * dim * 12 bytes (+ the ids)."""

    def __init__(self, n_bags: int, L: int, dim: int, device, backward: bool = True):
        m = int(n_bags) * int(L)
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        self.n_bags, self.L, self.dim = int(n_bags), int(L), int(dim)
        self.batch_ids = torch.empty(m, dtype=torch.int64, device=device)
        self.x, self.gates, self.gn, self.hprev = f(m, dim), f(m, 3 * dim), f(m, dim), f(m, dim)
        self.da, self.dg = (f(m, 3 * dim), f(m, 3 * dim)) if backward else (None, None)

    @classmethod
    def wrap(cls, L: int, batch_ids, x, gates, gn, hprev):
        """The buffers of a forward whose kept tensors were handed out one by one (``torch.ops.twotower.history_gru``)."""
        for t, name in ((x, "x"), (gates, "gates"), (gn, "gn"), (hprev, "hprev")):
            _chk(t, torch.float32, name, 2)
        _chk(batch_ids, torch.int64, "batch_ids", 1)
        m, d = x.shape
        if m % L or batch_ids.numel() != m or tuple(gates.shape) != (m, 3 * d) or tuple(gn.shape) != (m, d) or tuple(hprev.shape) != (m, d):
            raise RuntimeError(f"GruBuffers.wrap: need batch_ids [{m}], x / gn / hprev [{m}, {d}] and gates [{m}, {3 * d}] with "
                               f"n_bags * L = {m} a multiple of L = {L}")
        self = cls(0, L, d, x.device)
        self.n_bags, self.batch_ids, self.x, self.gates, self.gn, self.hprev = m // L, batch_ids, x, gates, gn, hprev
        self.da, self.dg = torch.empty_like(gates), torch.empty_like(gates)
        return self


def _chk_gru(what: str, d: int, L: int, W, U, b):
    _chk(W, torch.float32, "W", 2)
    _chk(U, torch.float32, "U", 2)
    if b is not None:
        _chk(b, torch.float32, "b", 2)
    if d % 32 or not 32 <= d <= 256:
        raise RuntimeError(f"{what}: dim must be a multiple of 32 in 32..256, got {d}")
    if not 1 <= L <= 64:
        raise RuntimeError(f"{what}: L must be in 1..64, got {L}")
    if tuple(W.shape) != (d, 3 * d) or tuple(U.shape) != (d, 3 * d) or (b is not None and tuple(b.shape) != (2, 3 * d)):
        raise RuntimeError(f"{what}: W and U must be [{d}, {3 * d}] (dim, 3 dim: z | r | n) and b [2, {3 * d}] (b_i, b_r), got "
                           f"{tuple(W.shape)}, {tuple(U.shape)} and {None if b is None else tuple(b.shape)}")


def history_gru(table: torch.Tensor, tokens: torch.Tensor, W: torch.Tensor, U: torch.Tensor, b: torch.Tensor,
                bag_rows: torch.Tensor | None = None, exclude: torch.Tensor | None = None, base=None,
                out: torch.Tensor | None = None, batch_ids: torch.Tensor | None = None, oob_flag: torch.Tensor | None = None,
                keep=False, scratch: "GruBuffers | None" = None):
    """The history bag encoded by a GRU (Keras ``GRU(dim, reset_after=True)``, zero initial state, mask-aware): over the kept
    slots of a bag in slot order - ``history_bag``'s rules: padding, out-of-range tokens and ``exclude`` skipped; the newest
    kept item is the last step - a = x W + b[0], g = h U + b[1], z = sigmoid(a_z + g_z), r = sigmoid(a_r + g_r),
    n = tanh(a_n + r g_n), h <- z h + (1 - z) n; out[b] = base row + h_final (no kept slot: the base row itself).  ``W``, ``U``
    [dim, 3 dim] with the gate column blocks z | r | n, ``b`` [2, 3 dim].  Three launches: the slot resolve
    (``tt_history_gru_resolve_f32``), the input projection over all slots (``tt_dense_fwd_batched_f32``) and the recurrence
    (``tt_history_gru_fwd_f32``).  ``tokens``, ``bag_rows``, ``exclude``, ``base``, ``batch_ids`` and ``oob_flag`` are
    ``history_attention``'s.  dim a multiple of 32 in 32..256, L in 1..64.  ``keep``: False - returns ``out``, nothing else is
    kept; True or a ``GruBuffers`` of this shape - returns (out, buffers) for ``history_gru_bwd`` (``batch_ids`` is then the
    buffers' own unless given).  ``scratch`` (inference only, ``keep`` False): a ``GruBuffers`` for AT LEAST n_bags bags of this
    (L, dim) whose ``x`` / ``gates`` / ``batch_ids`` serve as the call's workspace instead of fresh allocations."""
    n_rows, L, d, n_bags, out = _bag_args("history_gru", table, tokens, bag_rows, "sum", out, False, batch_ids, None, oob_flag)
    _chk_gru("history_gru", d, L, W, U, b)
    if exclude is not None:
        _chk(exclude, torch.int64, "exclude", 1)
        if exclude.numel() != n_bags:
            raise RuntimeError(f"history_gru: exclude must hold n_bags = {n_bags} entries, got {exclude.numel()}")
    base_table = base_ids = None
    if base is not None:
        base_table, base_ids = base
        _chk(base_table, torch.float32, "base_table", 2)
        _chk(base_ids, torch.int64, "base_ids", 1)
        if base_table.shape[1] != d or base_ids.numel() != n_bags:
            raise RuntimeError(f"history_gru: base must be ([rows, {d}] f32, [{n_bags}] int64), got "
                               f"{tuple(base_table.shape)} and {tuple(base_ids.shape)}")
    bufs = None
    if keep is not False and keep is not None:
        bufs = GruBuffers(n_bags, L, d, table.device) if keep is True else keep
        if not isinstance(bufs, GruBuffers) or (bufs.n_bags, bufs.L, bufs.dim) != (n_bags, L, d):
            raise RuntimeError(f"history_gru: keep must be a bool or a GruBuffers for ({n_bags}, {L}, {d}) (n_bags, L, dim)")
        if batch_ids is None:
            batch_ids = bufs.batch_ids
        x, a = bufs.x, bufs.gates
    elif scratch is not None:
        if not isinstance(scratch, GruBuffers) or (scratch.L, scratch.dim) != (L, d) or scratch.n_bags < n_bags:
            raise RuntimeError(f"history_gru: scratch must be a GruBuffers for at least {n_bags} bags of ({L}, {d}) (L, dim)")
        x, a = scratch.x[:n_bags * L], scratch.gates[:n_bags * L]
        if batch_ids is None:
            batch_ids = scratch.batch_ids[:n_bags * L]
    else:
        x = torch.empty((n_bags * L, d), dtype=torch.float32, device=table.device)
        a = torch.empty((n_bags * L, 3 * d), dtype=torch.float32, device=table.device)
        if batch_ids is None:
            batch_ids = torch.empty(n_bags * L, dtype=torch.int64, device=table.device)
    if n_bags == 0:
        return out if bufs is None else (out, bufs)
    lib = _lib.load()
    _lib.check(lib.tt_history_gru_resolve_f32(_p(table), table.shape[0], d, _p(tokens), n_rows, L, _p(bag_rows), n_bags, _p(exclude),
                                              _p(x), _p(batch_ids), _p(oob_flag), _stream()), "tt_history_gru_resolve_f32")
    dense_fwd(x, W, b[0], False, out=a)
    if bufs is not None and batch_ids is not bufs.batch_ids:
        bufs.batch_ids = batch_ids.view(-1)
    _lib.check(lib.tt_history_gru_fwd_f32(_p(a), _p(batch_ids), n_bags, L, d, _p(U), _p(b[1]), _p(out), _p(base_table),
                                          0 if base_table is None else base_table.shape[0], _p(base_ids), _p(oob_flag),
                                          _p(None if bufs is None else bufs.gates), _p(None if bufs is None else bufs.gn),
                                          _p(None if bufs is None else bufs.hprev), _stream()), "tt_history_gru_fwd_f32")
    return out if bufs is None else (out, bufs)


def history_gru_bwd(bufs: GruBuffers, dy: torch.Tensor, W: torch.Tensor, U: torch.Tensor, slot_grads: torch.Tensor | None = None,
                    dw_slabs: torch.Tensor | None = None, du_slabs: torch.Tensor | None = None,
                    db_slabs: torch.Tensor | None = None):
    """The backward of ``history_gru`` from its kept ``GruBuffers`` and ``dy`` [n_bags, dim]: the recurrent launch
    (``tt_history_gru_bwd_f32``: the slots in reverse from dh = dy, writing the pre-activation gradients ``da`` / ``dg``) and
    two ``tt_dense_bwd_batched_f32`` launches over all n_bags * L slots.  ``slot_grads`` [n_bags * L, dim] = da W^T gets ONE
    gradient row per slot (zeros for a skipped one) - what the sparse optimizers take with a plain ``SparsePlan(n_bags * L)``
    run over ``bufs.batch_ids``; ``dw_slabs`` / ``du_slabs`` [n_slabs, dim, 3 dim] and ``db_slabs`` [2, n_slabs, 3 dim] (b_i,
    b_r) are the parameters' gradients as ``dense_bwd_num_slabs(n_bags * L)`` slabs, every slab written in full: the form
    ``make_dense_seg`` / ``make_adam_seg`` sum.  All are allocated when None.  Returns (slot_grads, dw_slabs, du_slabs, db_slabs)."""
    if not isinstance(bufs, GruBuffers) or bufs.da is None:
        raise RuntimeError("history_gru_bwd: bufs must be the GruBuffers history_gru(keep=...) returned (with backward buffers)")
    n_bags, L, d = bufs.n_bags, bufs.L, bufs.dim
    _chk_gru("history_gru_bwd", d, L, W, U, None)
    _chk(dy, torch.float32, "dy", 2)
    if tuple(dy.shape) != (n_bags, d):
        raise RuntimeError(f"history_gru_bwd: dy must be [{n_bags}, {d}] (n_bags, dim), got {tuple(dy.shape)}")
    m = n_bags * L
    ns = dense_bwd_num_slabs(max(m, 1))
    dev = dy.device
    if slot_grads is None:
        slot_grads = torch.empty((m, d), dtype=torch.float32, device=dev)
    _chk(slot_grads, torch.float32, "slot_grads", 2)
    if tuple(slot_grads.shape) != (m, d):
        raise RuntimeError(f"history_gru_bwd: slot_grads must be [{m}, {d}] (n_bags * L, dim), got {tuple(slot_grads.shape)}")
    if dw_slabs is None:
        dw_slabs = torch.empty((ns, d, 3 * d), dtype=torch.float32, device=dev)
    if du_slabs is None:
        du_slabs = torch.empty((ns, d, 3 * d), dtype=torch.float32, device=dev)
    if db_slabs is None:
        db_slabs = torch.empty((2, ns, 3 * d), dtype=torch.float32, device=dev)
    for t, name, shape in ((dw_slabs, "dw_slabs", (ns, d, 3 * d)), (du_slabs, "du_slabs", (ns, d, 3 * d)), (db_slabs, "db_slabs", (2, ns, 3 * d))):
        _chk(t, torch.float32, name)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"history_gru_bwd: {name} must be {list(shape)} (n_slabs = dense_bwd_num_slabs(n_bags * L) = {ns}), got "
                               f"{tuple(t.shape)}")
    if n_bags == 0:
        dw_slabs.zero_(), du_slabs.zero_(), db_slabs.zero_()
        return slot_grads, dw_slabs, du_slabs, db_slabs
    _lib.check(_lib.load().tt_history_gru_bwd_f32(_p(bufs.batch_ids), _p(bufs.gates), _p(bufs.gn), _p(bufs.hprev), _p(dy), n_bags, L, d,
                                                  _p(U), _p(bufs.da), _p(bufs.dg), _stream()), "tt_history_gru_bwd_f32")
    dense_bwd(bufs.x, W, bufs.da, slot_grads, None, dw_slabs, db_slabs[0])
    dense_bwd(bufs.hprev, U, bufs.dg, None, None, du_slabs, db_slabs[1])
    return slot_grads, dw_slabs, du_slabs, db_slabs


SELF_ATTENTION_HEADS = (1, 2, 4, 8)


class SelfAttnBuffers:
    """What ``history_self_attention(keep=...)`` leaves for ``history_self_attention_bwd``, for ``n_bags`` bags of ``L`` slots at
    width ``dim`` with ``heads`` heads: ``batch_ids`` [n_bags * L] int64 (the slots' tokens, -1 where skipped), ``newest``
    [n_bags] int32 (the slot of the newest kept item, -1 for an emptied bag), ``xn`` [n_bags, dim] (its row), ``T`` and ``P``
    [n_bags, heads * dim] (the queries and the pooled rows), ``weights`` [n_bags, heads, L] and the backward's ``dP`` / ``dT``
    [n_bags, heads * dim] and ``dxn`` [n_bags, dim].  Nothing is n_bags * L * dim: 4 * n_bags * (4 heads + 2) * dim bytes (+ the
    ids and weights)."""

    def __init__(self, n_bags: int, L: int, dim: int, heads: int, device, backward: bool = True):
        n, hd = int(n_bags), int(heads) * int(dim)
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        self.n_bags, self.L, self.dim, self.heads = n, int(L), int(dim), int(heads)
        self.batch_ids = torch.empty(n * int(L), dtype=torch.int64, device=device)
        self.newest = torch.empty(n, dtype=torch.int32, device=device)
        self.xn, self.T, self.P, self.weights = f(n, dim), f(n, hd), f(n, hd), f(n, int(heads), int(L))
        self.dP, self.dT, self.dxn = (f(n, hd), f(n, hd), f(n, dim)) if backward else (None, None, None)
        self.table = self.db = None              # the table of the last forward; the backward GEMMs' throwaway bias slabs

    @classmethod
    def wrap(cls, table, batch_ids, newest, xn, T, P, weights):
        """The buffers of a forward whose kept tensors were handed out one by one (``torch.ops.twotower.history_self_attention``)."""
        for t, name in ((table, "table"), (xn, "xn"), (T, "T"), (P, "P")):
            _chk(t, torch.float32, name, 2)
        _chk(weights, torch.float32, "weights", 3)
        _chk(batch_ids, torch.int64, "batch_ids", 1)
        _chk(newest, torch.int32, "newest", 1)
        n, d = xn.shape
        _, h, L = weights.shape
        if (table.shape[1] != d or weights.shape[0] != n or newest.numel() != n or batch_ids.numel() != n * L or tuple(T.shape) != (n, h * d)
                or tuple(P.shape) != (n, h * d)):
            raise RuntimeError(f"SelfAttnBuffers.wrap: need table [rows, {d}], batch_ids [{n * L}], newest [{n}], xn [{n}, {d}], T / P [{n}, {h * d}] and "
                               f"weights [{n}, {h}, {L}], got {tuple(batch_ids.shape)}, {tuple(newest.shape)}, {tuple(xn.shape)}, "
                               f"{tuple(T.shape)}, {tuple(P.shape)} and {tuple(weights.shape)}")
        self = cls(0, L, d, h, xn.device)
        self.n_bags, self.batch_ids, self.newest, self.xn, self.T, self.P, self.weights = n, batch_ids, newest, xn, T, P, weights
        self.dP, self.dT, self.dxn, self.table = torch.empty_like(P), torch.empty_like(T), torch.empty_like(xn), table
        return self


def _chk_self_attention(what: str, d: int, L: int, Wqk, Wvo, p) -> int:
    """The shape checks of the self-attention ops; returns the head count (read from ``Wqk``)."""
    _chk(Wqk, torch.float32, "Wqk", 2)
    _chk(Wvo, torch.float32, "Wvo", 2)
    if p is not None:
        _chk(p, torch.float32, "p", 2)
    if d % 32 or not 32 <= d <= 256:
        raise RuntimeError(f"{what}: dim must be a multiple of 32 in 32..256, got {d}")
    if not 1 <= L <= 64:
        raise RuntimeError(f"{what}: L must be in 1..64, got {L}")
    h = Wqk.shape[1] // d
    if h not in SELF_ATTENTION_HEADS or tuple(Wqk.shape) != (d, h * d) or tuple(Wvo.shape) != (h * d, d) or (
            p is not None and tuple(p.shape) != (h, L)):
        raise RuntimeError(f"{what}: Wqk must be [{d}, H * {d}], Wvo [H * {d}, {d}] and p [H, {L}] with H heads in "
                           f"{SELF_ATTENTION_HEADS}, got {tuple(Wqk.shape)}, {tuple(Wvo.shape)} and "
                           f"{None if p is None else tuple(p.shape)}")
    return h


def history_self_attention_num_slabs(n: int) -> int:
    """Slab count of ``history_self_attention_bwd``'s ``dp_slabs`` for ``n`` bags (``tt_history_self_attention_num_slabs``)."""
    return int(_lib.load().tt_history_self_attention_num_slabs(n))


def history_self_attention(table: torch.Tensor, tokens: torch.Tensor, Wqk: torch.Tensor, Wvo: torch.Tensor, p: torch.Tensor,
                           bag_rows: torch.Tensor | None = None, exclude: torch.Tensor | None = None, base=None,
                           out: torch.Tensor | None = None, oob_flag: torch.Tensor | None = None, keep=False,
                           scratch: "SelfAttnBuffers | None" = None):
    """The history bag encoded by one multi-head self-attention block read at the last position: the newest kept item n of a
    bag is the query.  Over the kept slots j (``history_bag``'s rules: padding, out-of-range tokens and ``exclude`` skipped), with
    r_j the kept slots behind j: T = x_n Wqk, e_hj = <x_j, T_h> / sqrt(dim) + p[h, r_j], w_h = softmax_j(e_h), P_h = sum_j w_hj x_j,
    out[b] = base row + concat_h(P_h) Wvo (no kept slot: the base row itself).  ``Wqk`` [dim, H dim], ``Wvo`` [H dim, dim], ``p``
    [H, L]; H in {1, 2, 4, 8}, dim a multiple of 32 in 32..256, L in 1..64.  Five launches (four without a base): the resolve
    (``tt_history_self_attention_resolve_f32``), T (``tt_dense_fwd_batched_f32``), the pool
    (``tt_history_self_attention_pool_fwd_f32``), O (the GEMM again, into ``out``) and the base-row add
    (``tt_history_self_attention_combine_f32``).  ``tokens``, ``bag_rows``, ``exclude``, ``base`` and ``oob_flag`` are
    ``history_attention``'s.  ``keep``: False - returns ``out``, nothing else is kept; True or a ``SelfAttnBuffers`` of this shape -
    returns (out, buffers) for ``history_self_attention_bwd`` (the slots' ids are the buffers' ``batch_ids``).  ``scratch``
    (inference only, ``keep`` False): a ``SelfAttnBuffers`` for AT LEAST n_bags bags of this (L, dim, heads) whose tensors serve as
    the call's workspace instead of fresh allocations."""
    what = "history_self_attention"
    n_rows, L, d, n_bags, out = _bag_args(what, table, tokens, bag_rows, "sum", out, False, None, None, oob_flag)
    h = _chk_self_attention(what, d, L, Wqk, Wvo, p)
    if exclude is not None:
        _chk(exclude, torch.int64, "exclude", 1)
        if exclude.numel() != n_bags:
            raise RuntimeError(f"{what}: exclude must hold n_bags = {n_bags} entries, got {exclude.numel()}")
    base_table = base_ids = None
    if base is not None:
        base_table, base_ids = base
        _chk(base_table, torch.float32, "base_table", 2)
        _chk(base_ids, torch.int64, "base_ids", 1)
        if base_table.shape[1] != d or base_ids.numel() != n_bags:
            raise RuntimeError(f"{what}: base must be ([rows, {d}] f32, [{n_bags}] int64), got "
                               f"{tuple(base_table.shape)} and {tuple(base_ids.shape)}")
    bufs = None
    if keep is not False and keep is not None:
        bufs = SelfAttnBuffers(n_bags, L, d, h, table.device) if keep is True else keep
        if not isinstance(bufs, SelfAttnBuffers) or (bufs.n_bags, bufs.L, bufs.dim, bufs.heads) != (n_bags, L, d, h):
            raise RuntimeError(f"{what}: keep must be a bool or a SelfAttnBuffers for ({n_bags}, {L}, {d}, {h}) (n_bags, L, dim, heads)")
        w = bufs
    elif scratch is not None:
        if not isinstance(scratch, SelfAttnBuffers) or (scratch.L, scratch.dim, scratch.heads) != (L, d, h) or scratch.n_bags < n_bags:
            raise RuntimeError(f"{what}: scratch must be a SelfAttnBuffers for at least {n_bags} bags of ({L}, {d}, {h}) (L, dim, heads)")
        w = scratch
    else:
        w = SelfAttnBuffers(n_bags, L, d, h, table.device, backward=False)
    if bufs is not None:
        bufs.table = table
    if n_bags == 0:
        return out if bufs is None else (out, bufs)
    batch_ids, newest, xn, T, P, weights = (w.batch_ids.view(-1)[:n_bags * L], w.newest[:n_bags], w.xn[:n_bags], w.T[:n_bags],
                                            w.P[:n_bags], w.weights[:n_bags])
    lib = _lib.load()
    base_rows = 0 if base_table is None else base_table.shape[0]
    _lib.check(lib.tt_history_self_attention_resolve_f32(_p(table), table.shape[0], d, _p(tokens), n_rows, L, _p(bag_rows), n_bags,
                                                         _p(exclude), _p(base_ids), base_rows, _p(batch_ids), _p(newest), _p(xn),
                                                         _p(oob_flag), _stream()), "tt_history_self_attention_resolve_f32")
    dense_fwd(xn, Wqk, None, False, out=T)
    _lib.check(lib.tt_history_self_attention_pool_fwd_f32(_p(table), table.shape[0], d, L, h, _p(batch_ids), n_bags, _p(T), _p(p),
                                                          _p(P), _p(weights), _stream()), "tt_history_self_attention_pool_fwd_f32")
    dense_fwd(P, Wvo, None, False, out=out)
    if base_table is not None:
        _lib.check(lib.tt_history_self_attention_combine_f32(_p(out), _p(newest), n_bags, d, _p(base_table), base_rows, _p(base_ids),
                                                             _stream()), "tt_history_self_attention_combine_f32")
    return out if bufs is None else (out, bufs)


def history_self_attention_bwd(bufs: SelfAttnBuffers, dy: torch.Tensor, Wqk: torch.Tensor, Wvo: torch.Tensor,
                               slot_grads: torch.Tensor | None = None, dwqk_slabs: torch.Tensor | None = None,
                               dwvo_slabs: torch.Tensor | None = None, dp_slabs: torch.Tensor | None = None):
    """The backward of ``history_self_attention`` from its kept ``SelfAttnBuffers`` (which remember the table the forward read)
    and ``dy`` [n_bags, dim]: (dP, dWvo) = ``tt_dense_bwd_batched_f32`` of dy, the pool backward
    (``tt_history_self_attention_pool_bwd_f32``), (dxn, dWqk) = the GEMM again from dT, and the query gradient
    (``tt_history_self_attention_query_grad_f32``) - four launches.  ``slot_grads`` [n_bags * L, dim] gets ONE gradient row per
    kept slot (a skipped slot's row is left untouched) - what the sparse optimizers take with a plain ``SparsePlan(n_bags * L)``
    run over ``bufs.batch_ids``; ``dwqk_slabs`` [n_slabs, dim, H dim] and ``dwvo_slabs`` [n_slabs, H dim, dim]
    (n_slabs = ``dense_bwd_num_slabs(n_bags)``) and ``dp_slabs`` [``history_self_attention_num_slabs(n_bags)``, H * L] are the
    parameters' gradients as slabs, every slab written in full: the form ``make_dense_seg`` / ``make_adam_seg`` sum.  All are
    allocated when None.  Returns (slot_grads, dwqk_slabs, dwvo_slabs, dp_slabs)."""
    what = "history_self_attention_bwd"
    if not isinstance(bufs, SelfAttnBuffers) or bufs.dP is None:
        raise RuntimeError(f"{what}: bufs must be the SelfAttnBuffers history_self_attention(keep=...) returned (with backward buffers)")
    n_bags, L, d, h = bufs.n_bags, bufs.L, bufs.dim, bufs.heads
    if _chk_self_attention(what, d, L, Wqk, Wvo, None) != h:
        raise RuntimeError(f"{what}: Wqk / Wvo are not the {h}-head kernels of the forward")
    _chk(dy, torch.float32, "dy", 2)
    table = bufs.table
    if table is None:
        raise RuntimeError(f"{what}: bufs have been through no forward yet")
    if tuple(dy.shape) != (n_bags, d):
        raise RuntimeError(f"{what}: dy must be [{n_bags}, {d}] (n_bags, dim), got {tuple(dy.shape)}")
    m = n_bags * L
    ns, nsp = dense_bwd_num_slabs(max(n_bags, 1)), history_self_attention_num_slabs(n_bags)
    dev = dy.device
    if slot_grads is None:
        slot_grads = torch.empty((m, d), dtype=torch.float32, device=dev)
    _chk(slot_grads, torch.float32, "slot_grads", 2)
    if tuple(slot_grads.shape) != (m, d):
        raise RuntimeError(f"{what}: slot_grads must be [{m}, {d}] (n_bags * L, dim), got {tuple(slot_grads.shape)}")
    if dwqk_slabs is None:
        dwqk_slabs = torch.empty((ns, d, h * d), dtype=torch.float32, device=dev)
    if dwvo_slabs is None:
        dwvo_slabs = torch.empty((ns, h * d, d), dtype=torch.float32, device=dev)
    if dp_slabs is None:
        dp_slabs = torch.empty((nsp, h * L), dtype=torch.float32, device=dev)
    for t, name, shape in ((dwqk_slabs, "dwqk_slabs", (ns, d, h * d)), (dwvo_slabs, "dwvo_slabs", (ns, h * d, d))):
        _chk(t, torch.float32, name)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{what}: {name} must be {list(shape)} (n_slabs = dense_bwd_num_slabs(n_bags) = {ns}), got {tuple(t.shape)}")
    _chk(dp_slabs, torch.float32, "dp_slabs", 2)
    if dp_slabs.shape[0] < 1 or dp_slabs.shape[1] != h * L:
        raise RuntimeError(f"{what}: dp_slabs must be [n_slabs, {h * L}] (heads * L), got {tuple(dp_slabs.shape)}")
    if n_bags == 0:
        dwqk_slabs.zero_(), dwvo_slabs.zero_(), dp_slabs.zero_()
        return slot_grads, dwqk_slabs, dwvo_slabs, dp_slabs
    if bufs.db is None:                          # the GEMMs' bias slabs: there is no bias, they are written and thrown away
        bufs.db = torch.empty((ns, h * d), dtype=torch.float32, device=dev)
    db = bufs.db
    dense_bwd(bufs.P, Wvo, dy, bufs.dP, None, dwvo_slabs, db)
    lib = _lib.load()
    _lib.check(lib.tt_history_self_attention_pool_bwd_f32(_p(table), table.shape[0], d, L, h, _p(bufs.batch_ids), _p(bufs.weights),
                                                          _p(bufs.P), _p(bufs.dP), _p(bufs.T), n_bags, _p(slot_grads), _p(bufs.dT),
                                                          _p(dp_slabs), dp_slabs.shape[0], _stream()),
               "tt_history_self_attention_pool_bwd_f32")
    dense_bwd(bufs.xn, Wqk, bufs.dT, bufs.dxn, None, dwqk_slabs, db)
    _lib.check(lib.tt_history_self_attention_query_grad_f32(_p(bufs.newest), _p(bufs.dxn), n_bags, L, d, _p(slot_grads), _stream()),
               "tt_history_self_attention_query_grad_f32")
    return slot_grads, dwqk_slabs, dwvo_slabs, dp_slabs


def embedding_bag_bwd(dy: torch.Tensor, inv: torch.Tensor | None, order: torch.Tensor, L: int, order_bags: torch.Tensor,
                      gs: torch.Tensor | None = None):
    """The backward launch of ``embedding_bag`` (``tt_embedding_bag_bwd_f32``): ``gs[b, :] = dy[b, :] * inv[b]`` (``gs`` None -
    sum pooling - skips it: the bags' gradient rows are ``dy`` itself) and ``order_bags[j] = order[j] // L``, the bag of every
    sorted slot of a sort plan over ``batch_ids``.  Returns (the gradient rows to hand to the sparse update, order_bags)."""
    _chk(dy, torch.float32, "dy", 2)
    _chk(order, torch.int32, "order", 1)
    _chk(order_bags, torch.int32, "order_bags", 1)
    n_bags, d = dy.shape
    if order.numel() != n_bags * L or order_bags.numel() != n_bags * L:
        raise RuntimeError(f"embedding_bag_bwd: order and order_bags must hold n_bags * L = {n_bags * L} entries")
    if gs is not None:
        _chk(gs, torch.float32, "gs", 2)
        _chk(inv, torch.float32, "inv", 1)
        if gs.shape != dy.shape or inv.numel() != n_bags:
            raise RuntimeError("embedding_bag_bwd: gs must have dy's shape and inv n_bags entries")
    _lib.check(_lib.load().tt_embedding_bag_bwd_f32(_p(dy), _p(inv), n_bags, d, L, _p(order), n_bags * L, _p(gs), _p(order_bags),
                                                    _stream()), "tt_embedding_bag_bwd_f32")
    return (dy if gs is None else gs), order_bags


# ----------------------------------------------------------------------------- mixed negative sampling
SAMPLERS = {"uniform": _lib.TT_SAMPLER_UNIFORM, "alias": _lib.TT_SAMPLER_ALIAS}


def build_alias_table(prob):
    """Walker's alias table of the distribution ``prob`` (any non-negative weights, normalised here) by Vose's method, in NumPy
    f64 on the host - once per run, deterministic: ``(thr f32 [n], idx int32 [n])``.  A draw takes a uniform bucket b and
    u on the 2^-24 grid and returns ``b if u < thr[b] else idx[b]`` (``sample_candidates``, sampler "alias"); the thresholds are
    rounded to that grid, so the table's implied distribution is exact to 2^-25 / n per bucket."""
    import numpy as np
    p = np.asarray(prob, dtype=np.float64).reshape(-1)
    n = p.size
    if n == 0 or not np.isfinite(p).all() or (p < 0).any():
        raise ValueError("build_alias_table: the weights must be finite and non-negative (and there must be some)")
    total = p.sum()
    if not total > 0:
        raise ValueError("build_alias_table: the weights are all zero")
    if n >= 1 << 31:
        raise ValueError("build_alias_table: at most 2^31 - 1 items (the alias indices are int32)")
    scaled = (p / total * n).tolist()
    thr = [1.0] * n
    idx = list(range(n))
    small = [i for i in range(n - 1, -1, -1) if scaled[i] < 1.0]      # (popped from the end: ascending item order)
    large = [i for i in range(n - 1, -1, -1) if scaled[i] >= 1.0]
    while small and large:
        s, g = small.pop(), large[-1]
        thr[s], idx[s] = scaled[s], g
        scaled[g] = (scaled[g] + scaled[s]) - 1.0
        if scaled[g] < 1.0:
            small.append(large.pop())
    # what is left on either list is 1 up to rounding: the bucket keeps itself
    grid = np.rint(np.clip(np.asarray(thr, dtype=np.float64), 0.0, 1.0) * 16777216.0) / 16777216.0
    return grid.astype(np.float32), np.asarray(idx, dtype=np.int32)


def sample_candidates(pos_ids: torch.Tensor, n_items: int, n_neg: int, out_ids: torch.Tensor, out_prob: torch.Tensor | None = None,
                      *, sampler: str = "uniform", alias=None, item_freq: torch.Tensor | None = None,
                      sampler_prob: torch.Tensor | None = None, seed: int, tensor_id: int, start: int,
                      oob_flag: torch.Tensor | None = None):
    """A step's candidate list in one launch (``tt_sample_candidates_i64``): ``out_ids[:B] = pos_ids`` and ``out_ids[B + i]`` =
    draw ``start + i`` of the stream (seed, tensor_id) from ``n_items`` items - ``sampler`` "uniform", or "alias" with ``alias`` =
    (thr f32 [n_items], idx int32 [n_items]) device tensors (``build_alias_table``).  With ``item_freq`` (f32 [n_items], every
    item's in-batch frequency) ``out_prob[j]`` = (B * item_freq[id] + N * u_id) / (B + N) for every candidate, u_id =
    ``sampler_prob[id]`` (None: 1 / n_items) - the ``cand_prob`` of the scorer.  ``out_ids`` / ``out_prob`` may be longer than
    B + N; the rest is not touched.  Returns (out_ids[:B + N], out_prob[:B + N] or None)."""
    _chk(pos_ids, torch.int64, "pos_ids", 1)
    _chk(out_ids, torch.int64, "out_ids", 1)
    if sampler not in SAMPLERS:
        raise ValueError(f"sample_candidates: sampler must be one of {tuple(SAMPLERS)}, got {sampler!r}")
    b, n_neg, n_items = pos_ids.numel(), int(n_neg), int(n_items)
    n = b + max(n_neg, 0)
    if out_ids.numel() < n:
        raise RuntimeError(f"sample_candidates: out_ids must hold B + N = {n} entries, got {out_ids.numel()}")
    thr = idx = None
    if sampler == "alias":
        if alias is None:
            raise ValueError("sample_candidates: sampler 'alias' needs alias=(thr, idx)")
        thr, idx = alias
        _chk(thr, torch.float32, "alias thr", 1)
        _chk(idx, torch.int32, "alias idx", 1)
        if thr.numel() != n_items or idx.numel() != n_items:
            raise RuntimeError(f"sample_candidates: the alias table must have n_items = {n_items} entries")
    elif alias is not None:
        raise ValueError("sample_candidates: alias is given but the sampler is 'uniform'")
    for t, name in ((item_freq, "item_freq"), (sampler_prob, "sampler_prob")):
        if t is not None:
            _chk(t, torch.float32, name, 1)
            if t.numel() != n_items:
                raise RuntimeError(f"sample_candidates: {name} must have n_items = {n_items} entries, got {t.numel()}")
    if item_freq is not None:
        if out_prob is None:
            raise ValueError("sample_candidates: item_freq is given, so out_prob must be too")
        _chk(out_prob, torch.float32, "out_prob", 1)
        if out_prob.numel() < n:
            raise RuntimeError(f"sample_candidates: out_prob must hold B + N = {n} entries, got {out_prob.numel()}")
    if oob_flag is not None:
        _chk(oob_flag, torch.int32, "oob_flag")
    if not (0 <= int(seed) < 1 << 64 and 0 <= int(tensor_id) < 1 << 64 and 0 <= int(start) < 1 << 64):
        raise ValueError("sample_candidates: seed, tensor_id and start are unsigned 64-bit counters")
    _lib.check(_lib.load().tt_sample_candidates_i64(_p(pos_ids), b, n_items, n_neg, SAMPLERS[sampler], _p(thr), _p(idx),
                                                    _p(item_freq), _p(sampler_prob), int(seed), int(tensor_id), int(start),
                                                    _p(out_ids), _p(out_prob) if item_freq is not None else None, _p(oob_flag),
                                                    _stream()), "tt_sample_candidates_i64")
    return out_ids[:n], (out_prob[:n] if item_freq is not None else None)


# ----------------------------------------------------------------------------- streaming item-frequency estimation
MAX_FREQ_HASHES = 4


def new_frequency_sketch(hashes: int, slots: int, device) -> torch.Tensor:
    """A fresh sketch of the streaming frequency estimator: int64 [hashes, slots] of zeros (every slot: never hit)."""
    hashes, slots = int(hashes), int(slots)
    if not 1 <= hashes <= MAX_FREQ_HASHES:
        raise ValueError(f"new_frequency_sketch: hashes must be in 1..{MAX_FREQ_HASHES}, got {hashes}")
    if not 1 <= slots <= 1 << 32:
        raise ValueError(f"new_frequency_sketch: slots must be in 1..2^32, got {slots}")
    return torch.zeros(hashes, slots, dtype=torch.int64, device=device)


def unpack_frequency_sketch(sketch: torch.Tensor):
    """(last int32 [hashes, slots], delta f32 [hashes, slots]) of a sketch's packed slots: ``last`` = the 1-based step of the
    slot's last hit (0 = never), ``delta`` = its estimated gap in steps.  Copies; any device."""
    if not isinstance(sketch, torch.Tensor) or sketch.dtype != torch.int64 or sketch.dim() != 2:
        raise RuntimeError("unpack_frequency_sketch: expected an int64 [hashes, slots] tensor")
    halves = sketch.contiguous().view(torch.int32).reshape(sketch.shape[0], sketch.shape[1], 2)     # little-endian: low half first
    return halves[..., 0].clone(), halves[..., 1].contiguous().view(torch.float32).clone()


def frequency_estimate_(sketch: torch.Tensor, ids: torch.Tensor, n_update: int, step: int, alpha: float, n_items: int,
                        out: torch.Tensor, *, seed: int, tensor_id: int, sampler_prob: torch.Tensor | None = None,
                        mix: bool = False, oob_flag: torch.Tensor | None = None) -> torch.Tensor:
    """The streaming frequency estimator (``tt_frequency_estimate_i64``, Yi et al. 2019): the first ``n_update`` of ``ids`` - the
    step's positives - update ``sketch`` (``new_frequency_sketch``) IN PLACE at the 1-based ``step`` with the moving-average
    coefficient ``alpha``, then ``out[j]`` = the estimated probability 1 / D_j of EVERY id, D_j = the largest estimated gap over
    the sketch's hash rows.  ``mix``: ``out[j]`` = (1 / D_j + N u_j) / (B + N) with B = n_update, N = len(ids) - n_update and u_j =
    ``sampler_prob[id]`` (None: 1 / n_items) - the candidate probability of mixed negative sampling.  ``n_update = 0`` only reads.
    ``out`` may be longer than ``ids``; the rest is not touched.  Returns out[:len(ids)]."""
    _chk(sketch, torch.int64, "sketch", 2)
    _chk(ids, torch.int64, "ids", 1)
    _chk(out, torch.float32, "out", 1)
    n, n_update, n_items, step = ids.numel(), int(n_update), int(n_items), int(step)
    hashes, slots = sketch.shape
    if not 1 <= hashes <= MAX_FREQ_HASHES or slots < 1:
        raise RuntimeError(f"frequency_estimate_: sketch must be [hashes in 1..{MAX_FREQ_HASHES}, slots >= 1], got {list(sketch.shape)}")
    if out.numel() < n:
        raise RuntimeError(f"frequency_estimate_: out must hold len(ids) = {n} entries, got {out.numel()}")
    if ids.device != sketch.device or out.device != sketch.device:
        raise RuntimeError("frequency_estimate_: sketch, ids and out must be on one device")
    if sampler_prob is not None:
        _chk(sampler_prob, torch.float32, "sampler_prob", 1)
        if sampler_prob.numel() != n_items:
            raise RuntimeError(f"frequency_estimate_: sampler_prob must have n_items = {n_items} entries, got {sampler_prob.numel()}")
        if not mix:
            raise ValueError("frequency_estimate_: sampler_prob is given but mix is off")
    if oob_flag is not None:
        _chk(oob_flag, torch.int32, "oob_flag")
    if not (0 <= int(seed) < 1 << 64 and 0 <= int(tensor_id) < (1 << 64) - MAX_FREQ_HASHES):
        raise ValueError("frequency_estimate_: seed and tensor_id are unsigned 64-bit counters")
    _lib.check(_lib.load().tt_frequency_estimate_i64(_p(ids), n, n_update, n_items, _p(sketch), hashes, slots, step, float(alpha),
                                                     int(seed), int(tensor_id), _p(sampler_prob), 1 if mix else 0, _p(out),
                                                     _p(oob_flag), _stream()), "tt_frequency_estimate_i64")
    return out[:n]


# ----------------------------------------------------------------------------- sharded routing
def route_by_owner(ids, world: int, num_rows: int, cap: int, send_ids, pos_flat, flags=None):
    _chk(ids, torch.int64, "ids", 1)
    _chk(send_ids, torch.int64, "send_ids")
    _chk(pos_flat, torch.int64, "pos_flat")
    if send_ids.numel() < world * cap or pos_flat.numel() < ids.numel():
        raise RuntimeError("route_by_owner: output buffers too small")
    lib = _lib.load()
    _lib.check(lib.tt_route_by_owner_i64(_p(ids), ids.numel(), world, num_rows, cap, _p(send_ids), _p(pos_flat), _p(flags),
                                         _stream()), "tt_route_by_owner_i64")


def route_tables_by_owner(ids_list, world: int, num_rows_list, local_offsets, cap: int, send_ids, pos_flats, flags=None):
    """Several tables, one launch: send_ids is [world][n_tables][cap] (see tt_route_tables_by_owner_i64)."""
    t = len(ids_list)
    n = ids_list[0].numel()
    for ids, pos in zip(ids_list, pos_flats):
        _chk(ids, torch.int64, "ids", 1)
        _chk(pos, torch.int64, "pos_flat")
        if ids.numel() != n or pos.numel() < n:
            raise RuntimeError("route_tables_by_owner: every table needs n_ids ids and a pos_flat of n_ids")
    _chk(send_ids, torch.int64, "send_ids")
    if send_ids.numel() < world * t * cap:
        raise RuntimeError("route_tables_by_owner: send_ids too small")
    arr = (_lib.RouteTable * t)(*[_lib.RouteTable(_p(ids_list[i]), int(num_rows_list[i]), int(local_offsets[i]), _p(pos_flats[i]))
                                  for i in range(t)])
    lib = _lib.load()
    _lib.check(lib.tt_route_tables_by_owner_i64(arr, t, n, world, cap, _p(send_ids), _p(flags), _stream()),
               "tt_route_tables_by_owner_i64")


def scatter_rows(src, idx, dst):
    _chk(src, torch.float32, "src", 2)
    _chk(idx, torch.int64, "idx", 1)
    _chk(dst, torch.float32, "dst", 2)
    if src.shape[1] != dst.shape[1] or idx.numel() != src.shape[0]:
        raise RuntimeError("scatter_rows: shape mismatch")
    lib = _lib.load()
    _lib.check(lib.tt_scatter_rows_f32(_p(src), _p(idx), src.shape[0], src.shape[1], _p(dst), dst.shape[0], _stream()),
               "tt_scatter_rows_f32")


# ----------------------------------------------------------------------------- a5 sparse optimizer
class SparsePlan:
    """Sorted (id, position) list of one id batch; reusable buffers."""

    def __init__(self, n_ids: int, device):
        lib = _lib.load()
        self.n_ids = n_ids
        self.ws_bytes = int(lib.tt_sparse_plan_workspace_bytes(n_ids))
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.sorted_ids = torch.empty(n_ids, dtype=torch.int64, device=device)
        self.order = torch.empty(n_ids, dtype=torch.int32, device=device)
        self._apply_ws = None
        self._adam_ws = None
        self._rowwise_ws = None

    @property
    def grad_order(self) -> torch.Tensor:
        """What the update kernels index the gradient rows with: row grad_order[j] is the gradient of sorted slot j."""
        return self.order

    @property
    def grad_rows(self) -> int:
        """Rows of the gradient tensor the update kernels read through ``grad_order``."""
        return self.n_ids

    def adam_ws(self, dim: int) -> torch.Tensor:
        """Piece-sum workspace of ``adam_step_`` for rows of ``dim`` floats (allocated once; never initialised)."""
        need = max(adam_workspace_bytes(self.n_ids, dim), 256)
        if self._adam_ws is None or self._adam_ws.numel() < need:
            self._adam_ws = torch.empty(need, dtype=torch.uint8, device=self.sorted_ids.device)
        return self._adam_ws

    def rowwise_ws(self, dim: int) -> torch.Tensor:
        """Piece-sum workspace of ``rowwise_adagrad_step_`` for rows of ``dim`` floats (allocated once; never initialised)."""
        need = max(rowwise_adagrad_workspace_bytes(self.n_ids, dim), 256)
        if self._rowwise_ws is None or self._rowwise_ws.numel() < need:
            self._rowwise_ws = torch.empty(need, dtype=torch.uint8, device=self.sorted_ids.device)
        return self._rowwise_ws

    def apply_ws(self, dim: int) -> torch.Tensor:
        """Piece-sum workspace of the apply kernels for rows of ``dim`` floats (allocated once)."""
        need = int(_lib.load().tt_sparse_apply_workspace_bytes(self.n_ids, dim))
        if self._apply_ws is None or self._apply_ws.numel() < need:
            self._apply_ws = torch.zeros(need, dtype=torch.uint8, device=self.sorted_ids.device)   # contract: zeroed once
        return self._apply_ws

    def run(self, ids: torch.Tensor, num_rows: int) -> "SparsePlan":
        _chk(ids, torch.int64, "ids", 1)
        if ids.numel() != self.n_ids:
            raise RuntimeError(f"SparsePlan: built for {self.n_ids} ids, got {ids.numel()}")
        lib = _lib.load()
        _lib.check(lib.tt_sparse_plan(_p(ids), self.n_ids, num_rows, _p(self.workspace), self.ws_bytes,
                                      _p(self.sorted_ids), _p(self.order), _stream()), "tt_sparse_plan")
        return self


class BagPlan(SparsePlan):
    """The sort plan of an ``embedding_bag`` batch: ``run`` sorts the n_bags * L slot tokens (``batch_ids``), ``backward`` turns
    the sorted slots' positions into bag indices (``order_bags``) - and scales the bags' gradient rows - so that
    ``sparse_sgd_`` / ``sparse_adagrad_`` / ``adam_step_`` update the bag table from the [n_bags, dim] gradient rows: no
    per-token gradient row is ever written."""

    def __init__(self, n_bags: int, L: int, device):
        super().__init__(n_bags * L, device)
        self.n_bags, self.L = n_bags, L
        self.order_bags = torch.zeros(n_bags * L, dtype=torch.int32, device=device)

    @property
    def grad_order(self) -> torch.Tensor:
        return self.order_bags

    @property
    def grad_rows(self) -> int:
        return self.n_bags

    def backward(self, dy: torch.Tensor, inv: torch.Tensor | None = None, gs: torch.Tensor | None = None) -> torch.Tensor:
        """One launch after ``run``: returns the gradient rows for the update (``gs`` = dy * inv, or ``dy`` when gs is None)."""
        return embedding_bag_bwd(dy, inv, self.order, self.L, self.order_bags, gs)[0]


def sparse_plan_batched(plans, ids_list, num_rows_list):
    """Sort up to 4 id lists (user, item, hashed category, ...) in ONE launch (key-range partitions: csrc/sort.hip)."""
    n = len(plans)
    args = []
    for plan, ids, rows in zip(plans, ids_list, num_rows_list):
        _chk(ids, torch.int64, "ids", 1)
        if ids.numel() != plan.n_ids:
            raise RuntimeError(f"SparsePlan: built for {plan.n_ids} ids, got {ids.numel()}")
        args.append(_lib.SparsePlanArgs(_p(ids), plan.n_ids, int(rows), _p(plan.workspace), plan.ws_bytes,
                                        _p(plan.sorted_ids), _p(plan.order)))
    arr = (_lib.SparsePlanArgs * n)(*args)
    _lib.check(_lib.load().tt_sparse_plan_batched(arr, n, _stream()), "tt_sparse_plan_batched")


def _chk_plan_grads(grads, plan: SparsePlan, table, what: str):
    """A BagPlan's positions are bag indices: the gradient tensor must hold exactly one row per bag."""
    if isinstance(plan, BagPlan) and tuple(grads.shape) != (plan.n_bags, table.shape[1]):
        raise RuntimeError(f"{what}: grads must be [{plan.n_bags}, {table.shape[1]}] (one row per bag, dim), got {tuple(grads.shape)}")


def sparse_sgd_(table, grads, plan: SparsePlan, lr: float):
    """``plan`` may be a ``BagPlan`` (after its ``backward``): ``grads`` then holds one row per bag."""
    _chk(table, torch.float32, "table", 2)
    _chk(grads, torch.float32, "grads", 2)
    _chk_plan_grads(grads, plan, table, "sparse_sgd_")
    lib = _lib.load()
    _lib.check(lib.tt_sparse_sgd_f32(_p(table), table.shape[0], table.shape[1], _p(grads), _p(plan.sorted_ids),
                                     _p(plan.grad_order), plan.n_ids, lr, _p(plan.apply_ws(table.shape[1])), _stream()),
               "tt_sparse_sgd_f32")
    return table


def sparse_adagrad_(table, accum, grads, plan: SparsePlan, lr: float, eps: float = 1e-7):
    _chk(table, torch.float32, "table", 2)
    _chk(accum, torch.float32, "accum", 2)
    _chk(grads, torch.float32, "grads", 2)
    _chk_plan_grads(grads, plan, table, "sparse_adagrad_")
    lib = _lib.load()
    _lib.check(lib.tt_sparse_adagrad_f32(_p(table), _p(accum), table.shape[0], table.shape[1], _p(grads),
                                         _p(plan.sorted_ids), _p(plan.grad_order), plan.n_ids, lr, eps,
                                         _p(plan.apply_ws(table.shape[1])), _stream()), "tt_sparse_adagrad_f32")
    return table


def sparse_update2_(opt: str, table_a, accum_a, grads_a, plan_a: SparsePlan,
                    table_b, accum_b, grads_b, plan_b: SparsePlan, lr: float, eps: float = 1e-7):
    """User and item table updates in one launch."""
    lib = _lib.load()
    _lib.check(lib.tt_sparse_update2_f32(_OPT[opt], _p(table_a), _p(accum_a), table_a.shape[0], _p(grads_a),
                                         _p(plan_a.sorted_ids), _p(plan_a.order),
                                         _p(table_b), _p(accum_b), table_b.shape[0], _p(grads_b),
                                         _p(plan_b.sorted_ids), _p(plan_b.order),
                                         table_a.shape[1], plan_a.n_ids, lr, eps, _p(plan_a.apply_ws(table_a.shape[1])),
                                         _p(plan_b.apply_ws(table_b.shape[1])), _stream()), "tt_sparse_update2_f32")


# ----------------------------------------------------------------------------- a2 dense layers
MAX_FUSED_LOOKUP_ROWS = 32768       # tt_dense_lookup: the ids of one dW split are staged in LDS


class IdBuckets:
    """Row-range id lists (``tt_id_buckets``, ABI v9) for one train step's tables: the forward lookup (``make_lookup(...,
    buckets=b.desc(t, gen))``) appends every id to the list of the row range the optimizer launch's sorting workgroup owns, and
    ``optimizer_step_ids_(..., buckets=[...])`` of the same step reads ~64 entries per workgroup instead of all the ids.
    ``cap == 0``: the shape takes no lists (dim > 128 or more than 16384 ids)."""

    def __init__(self, table_rows, dim: int, n_ids: int, segs, device):
        lib = _lib.load()
        n = len(table_rows)
        rows = (_lib.C.c_int64 * n)(*table_rows)
        groups, width, cap = (_lib.C.c_int32 * n)(), (_lib.C.c_uint32 * n)(), _lib.C.c_int32(0)
        arr_s = (DenseSeg * len(segs))(*segs)
        _lib.check(lib.tt_optimizer_ids_geometry(rows, n, dim, n_ids, arr_s, len(segs), groups, width, _lib.C.byref(cap)),
                   "tt_optimizer_ids_geometry")
        self.groups, self.width, self.cap = list(groups), list(width), int(cap.value)
        self.per = int(lib.tt_id_buckets_workspace_bytes())
        self.ws = torch.zeros(n * self.per, dtype=torch.uint8, device=device)

    def desc(self, t: int, gen: int) -> "_lib.IdBuckets":
        base = self.ws.data_ptr() + t * self.per
        return _lib.IdBuckets(base, base + self.COUNT_BYTES, self.groups[t], self.width[t], self.cap, gen & 0xFFFFFFFF)

    COUNT_BYTES = 256 * 256          # one counter per 256-byte line (csrc/common.h: kBucketGroupsMax * kBucketCountStride * 4)

    def counts(self, t: int) -> torch.Tensor:
        return self.ws[t * self.per: t * self.per + self.COUNT_BYTES].view(torch.int32)[:: 64][: self.groups[t]]


def make_lookup(table, ids, table2=None, ids2=None, oob_flag=None, buckets=None) -> "_lib.DenseLookup":
    """The embedding lookup fused into a tower's FIRST Dense layer (``tt_dense_lookup``): the layer's input row r is
    ``table[ids[r]]`` (+ ``table2[ids2[r]]``), read straight into the GEMM tiles — never written to HBM."""
    _chk(table, torch.float32, "lookup table", 2)
    _chk(ids, torch.int64, "lookup ids", 1)
    if (table2 is None) != (ids2 is None):
        raise RuntimeError("make_lookup: table2 and ids2 go together")
    if table2 is not None:
        _chk(table2, torch.float32, "lookup table2", 2)
        _chk(ids2, torch.int64, "lookup ids2", 1)
        if table2.shape[1] != table.shape[1] or ids2.numel() != ids.numel():
            raise RuntimeError("make_lookup: table2 / ids2 must match table's width and the number of ids")
    if oob_flag is not None:
        _chk(oob_flag, torch.int32, "oob_flag")
    if ids.numel() > MAX_FUSED_LOOKUP_ROWS:
        raise RuntimeError(f"make_lookup: at most {MAX_FUSED_LOOKUP_ROWS} rows per fused lookup")
    lk = _lib.DenseLookup(_p(table), _p(ids), table.shape[0], _p(table2), _p(ids2), 0 if table2 is None else table2.shape[0],
                          _p(oob_flag))
    if buckets is not None:
        lk.buckets = buckets
    lk._keep = (table, ids, table2, ids2, oob_flag)      # the struct holds raw pointers: keep the tensors alive with it
    lk._mk = (ids.numel(), table.shape[1])
    return lk


def _no_lookup():
    return _lib.DenseLookup()


def _fwd_args(x, w, b, y, tid, lookup, bits):
    """One layer's ``tt_dense_fwd_args``; with a lookup the input rows come from the embedding table and x is not passed."""
    return _lib.DenseFwdArgs(None if lookup is not None else _p(x), _p(w), _p(b), _p(y), tid,
                             lookup if lookup is not None else _no_lookup(), _p(bits))


def _in_shape(x, lookup):
    if lookup is not None:
        return lookup._mk
    _chk(x, torch.float32, "x", 2)
    return x.shape[0], x.shape[1]


def relu_bits_like(m: int, n: int, device) -> torch.Tensor:
    """[m, n/32] int32 buffer for the sign bits a forward layer writes beside its output (n % 32 == 0)."""
    if n % 32:
        raise RuntimeError(f"relu bits need a layer width that is a multiple of 32, got {n}")
    return torch.empty((m, n // 32), dtype=torch.int32, device=device)


def _chk_bits(bits, m, n, what):
    if bits is None:
        return
    if bits.dtype != torch.int32 or not bits.is_cuda or not bits.is_contiguous() or tuple(bits.shape) != (m, n // 32) or n % 32:
        raise RuntimeError(f"{what}: expected a contiguous CUDA int32 tensor [{m}, {n}/32] (width a multiple of 32), got "
                           f"{bits.dtype} {tuple(bits.shape)}")


def dense_fwd(x, w, b, relu: bool, out=None, dropout=None, lookup=None, relu_bits=None):
    """y = act(x@w+b); ``dropout`` = (rate, seed, tensor_id, counter_offset) applies inverted dropout to y.
    With ``lookup`` (make_lookup) x is ignored: the input rows come from the embedding table.
    ``relu_bits`` (relu_bits_like): also written, bit = (y > 0) — the next layer's backward takes it as its dx mask."""
    _chk(w, torch.float32, "w", 2)
    if b is not None:
        _chk(b, torch.float32, "b", 1)
    m, k = _in_shape(x, lookup)
    n = w.shape[1]
    if w.shape[0] != k:
        raise RuntimeError(f"dense_fwd: input is [{m},{k}] but w is {tuple(w.shape)}")
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=w.device)
    _chk(out, torch.float32, "out", 2)
    if tuple(out.shape) != (m, n):
        raise RuntimeError(f"dense_fwd: out must be [{m},{n}], got {tuple(out.shape)}")
    rate, seed, tid, off = dropout if dropout is not None else (0.0, 0, 0, 0)
    _chk_bits(relu_bits, m, n, "dense_fwd: relu_bits")
    arr = (_lib.DenseFwdArgs * 1)(_fwd_args(x, w, b, out, tid, lookup, relu_bits))
    _lib.check(_lib.load().tt_dense_fwd_batched_f32(arr, 1, m, k, n, int(relu), rate, seed, off, _stream()),
               "tt_dense_fwd_batched_f32")
    return out


def dense_bwd_num_slabs(m: int) -> int:
    return int(_lib.load().tt_dense_bwd_num_slabs(m))


def dense_bwd(x, w, dz, dx, dx_relu_src, dw_slabs, db_slabs, dx_scale: float = 1.0, lookup=None, dx_relu_bits=None):
    """dx = dz@w^T (* (dx_relu_src>0)); dw_slabs/db_slabs get the split-K partials.  With ``lookup`` the layer's input
    (needed by dw = x^T dz) is read from the embedding table.  ``dx_relu_bits`` (the sign bits the previous layer's
    forward wrote) replaces ``dx_relu_src`` as the mask."""
    _chk(w, torch.float32, "w", 2)
    _chk(dz, torch.float32, "dz", 2)
    m, k = _in_shape(x, lookup)
    n = w.shape[1]
    if dx is not None:
        _chk(dx, torch.float32, "dx", 2)
    if dx_relu_src is not None:
        _chk(dx_relu_src, torch.float32, "dx_relu_src", 2)
    ns = dense_bwd_num_slabs(m)
    if dw_slabs is not None or db_slabs is not None:      # both None: dx only
        _chk(dw_slabs, torch.float32, "dw_slabs")
        _chk(db_slabs, torch.float32, "db_slabs")
        if dw_slabs.numel() < ns * k * n or db_slabs.numel() < ns * n:
            raise RuntimeError("dense_bwd: slab buffers too small")
    _chk_bits(dx_relu_bits, m, k, "dense_bwd: dx_relu_bits")
    arr = _bwd_args([x], [w], [dz], [dx], [dx_relu_src], [dw_slabs], [db_slabs], None if lookup is None else [lookup], [dx_relu_bits])
    _lib.check(_lib.load().tt_dense_bwd_batched_f32(arr, 1, dx_scale, m, k, n, _stream()), "tt_dense_bwd_batched_f32")
    return ns


def dense_fwd2(xs, ws, bs, ys, relu: bool, dropout=None, lookups=None, relu_bits=(None, None)):
    """Layer l of both towers in one launch: ys[i] = act(xs[i] @ ws[i] + bs[i]).  dropout = (rate, seed, (tid_a, tid_b), offset).
    lookups = (lookup_a, lookup_b): the towers' first layer reads its input rows from the embedding tables."""
    m, k = _in_shape(xs[0], None if lookups is None else lookups[0])
    n = ws[0].shape[1]
    rate, seed, tids, off = dropout if dropout is not None else (0.0, 0, (0, 0), 0)
    for i in range(2):
        _chk_bits(relu_bits[i], m, n, "dense_fwd2: relu_bits")
    arr = (_lib.DenseFwdArgs * 2)(*[_fwd_args(xs[i], ws[i], bs[i], ys[i], tids[i], None if lookups is None else lookups[i], relu_bits[i])
                                    for i in range(2)])
    _lib.check(_lib.load().tt_dense_fwd_batched_f32(arr, 2, m, k, n, int(relu), rate, seed, off, _stream()),
               "tt_dense_fwd_batched_f32")


def tower_fwd2_supported(m: int, k0: int, h: int, n1: int) -> bool:
    """Shapes the fused two-layer tower forward takes (csrc/tower.hip)."""
    return bool(_lib.load().tt_tower_fwd2_supported(m, k0, h, n1))


def tower_fwd2(xs, w0s, b0s, hs, h_bits, w1s, b1s, ys, dropout=None, lookups=None):
    """h = relu(x @ w0 + b0) [dropout], y = h @ w1 + b1 for both towers in ONE launch (the hidden tile stays in LDS; h and
    its sign bits are still written for the backward pass).  Bit-identical to dense_fwd2 called for each layer.
    dropout = (rate, seed, (tid_a, tid_b), offset) for the hidden layer; lookups as in dense_fwd2."""
    m, k0 = _in_shape(xs[0], None if lookups is None else lookups[0])
    h, n1 = w0s[0].shape[1], w1s[0].shape[1]
    rate, seed, tids, off = dropout if dropout is not None else (0.0, 0, (0, 0), 0)
    for i in range(2):
        _chk(w0s[i], torch.float32, "w0", 2); _chk(w1s[i], torch.float32, "w1", 2)
        _chk(hs[i], torch.float32, "h", 2); _chk(ys[i], torch.float32, "y", 2)
        if tuple(w0s[i].shape) != (k0, h) or tuple(w1s[i].shape) != (h, n1) or tuple(hs[i].shape) != (m, h) or tuple(ys[i].shape) != (m, n1):
            raise RuntimeError("tower_fwd2: shape mismatch between the layers' weights and buffers")
        _chk_bits(h_bits[i], m, h, "tower_fwd2: h_bits")
    l0 = (_lib.DenseFwdArgs * 2)(*[_fwd_args(xs[i], w0s[i], b0s[i], hs[i], tids[i], None if lookups is None else lookups[i], h_bits[i])
                                   for i in range(2)])
    l1 = (_lib.DenseFwdArgs * 2)(*[_fwd_args(hs[i], w1s[i], b1s[i], ys[i], 0, None, None) for i in range(2)])
    _lib.check(_lib.load().tt_tower_fwd2_batched_f32(l0, l1, 2, m, k0, h, n1, rate, seed, off, _stream()), "tt_tower_fwd2_batched_f32")


def dense_bwd2(xs, ws, dzs, dxs, dx_relu_srcs, dw_slabs, db_slabs, dx_scale: float = 1.0, lookups=None, dx_relu_bits=(None, None),
               riders=None):
    """Backward of layer l of both towers: one launch (dx and dw+db tiles side by side; dx only / dw only: one each).
    ``riders = (segs, opt, lr, eps)``: the dense update of ANOTHER layer's segments in the same launch
    (``tt_dense_bwd_batched_update_f32``; bit-identical to ``dense_update_`` behind the launch)."""
    m, k = _in_shape(xs[0], None if lookups is None else lookups[0])
    n = ws[0].shape[1]
    for i in range(2):
        _chk_bits(dx_relu_bits[i], m, k, "dense_bwd2: dx_relu_bits")
    arr = _bwd_args(xs, ws, dzs, dxs, dx_relu_srcs, dw_slabs, db_slabs, lookups, dx_relu_bits)
    if riders is not None:
        segs, opt, lr, eps = riders
        arr_s = (DenseSeg * len(segs))(*segs)
        _lib.check(_lib.load().tt_dense_bwd_batched_update_f32(arr, 2, dx_scale, m, k, n, arr_s, len(segs), _OPT[opt], lr, eps, _stream()),
                   "tt_dense_bwd_batched_update_f32")
        return
    _lib.check(_lib.load().tt_dense_bwd_batched_f32(arr, 2, dx_scale, m, k, n, _stream()), "tt_dense_bwd_batched_f32")


def _bwd_args(xs, ws, dzs, dxs, dx_relu_srcs, dw_slabs, db_slabs, lookups, dx_relu_bits):
    """The ``tt_dense_bwd_args`` array of one layer: an element per tower (two), or the single layer's one."""
    n = len(ws)
    return (_lib.DenseBwdArgs * n)(*[_lib.DenseBwdArgs(None if lookups is not None else _p(xs[i]), _p(ws[i]), _p(dzs[i]), _p(dxs[i]),
                                                      _p(dx_relu_srcs[i]), _p(dw_slabs[i]), _p(db_slabs[i]),
                                                      lookups[i] if lookups is not None else _no_lookup(),
                                                      _p(dx_relu_bits[i])) for i in range(n)])


def tower_bwd2_supported(m: int, k0: int, k1: int, n: int) -> bool:
    return bool(_lib.load().tt_tower_bwd2_supported(m, k0, k1, n))


def tower_bwd2_workspace(m: int, device) -> torch.Tensor:
    """The dependency counters of ``tower_bwd2`` (zeroed once; every launch leaves them zeroed; int32 word 4*(m//64) = error)."""
    return torch.zeros(int(_lib.load().tt_tower_bwd2_workspace_bytes(m)), dtype=torch.uint8, device=device)


def tower_bwd2(upper: dict, lower: dict, workspace: torch.Tensor, dx_scale_upper: float = 1.0, dx_scale_lower: float = 1.0):
    """Backward of layers l (``upper``) and l-1 (``lower``) of both towers in ONE launch (``tt_tower_bwd2_batched_f32``); each
    dict holds ``dense_bwd2``'s arguments: xs, ws, dzs, dxs, dx_relu_srcs, dw_slabs, db_slabs and optionally lookups, dx_relu_bits.
    ``upper['dxs'][i]`` must BE ``lower['dzs'][i]``.  Bit-identical to the two ``dense_bwd2`` calls."""
    none2 = (None, None)
    lk = lower.get("lookups")
    m, k0 = _in_shape(lower["xs"][0], None if lk is None else lk[0])
    k1, n = upper["ws"][0].shape[0], upper["ws"][0].shape[1]
    bu, bl = upper.get("dx_relu_bits", none2), lower.get("dx_relu_bits", none2)
    for i in range(2):
        _chk_bits(bu[i], m, k1, "tower_bwd2: upper dx_relu_bits")
        _chk_bits(bl[i], m, k0, "tower_bwd2: lower dx_relu_bits")
    au = _bwd_args(upper["xs"], upper["ws"], upper["dzs"], upper["dxs"], upper["dx_relu_srcs"], upper["dw_slabs"], upper["db_slabs"], None, bu)
    al = _bwd_args(lower["xs"], lower["ws"], lower["dzs"], lower["dxs"], lower["dx_relu_srcs"], lower["dw_slabs"], lower["db_slabs"], lk, bl)
    _lib.check(_lib.load().tt_tower_bwd2_batched_f32(au, al, 2, dx_scale_upper, dx_scale_lower, m, k0, k1, n, _p(workspace), _stream()),
               "tt_tower_bwd2_batched_f32")


def dense_update_(segs: list[DenseSeg], opt: str, lr: float, eps: float = 1e-7, apply: bool = True):
    arr = (DenseSeg * len(segs))(*segs)
    lib = _lib.load()
    _lib.check(lib.tt_dense_update_f32(arr, len(segs), _OPT[opt], int(apply), lr, eps, _stream()), "tt_dense_update_f32")


def optimizer_step_(opt: str, tables, segs: list[DenseSeg], lr: float, eps: float = 1e-7):
    """The train step's whole optimizer in ONE launch: ``tables`` = [(table, accum or None, grads, plan), ...] (up to 3
    embedding tables of one width whose plans hold the same number of ids) + the dense tower segments."""
    dim, n_ids = tables[0][0].shape[1], tables[0][3].n_ids
    arr_t = (_lib.SparseTable * len(tables))()
    for i, (table, accum, grads, plan) in enumerate(tables):
        _chk(table, torch.float32, "table", 2)
        _chk(grads, torch.float32, "grads", 2)
        if accum is not None:
            _chk(accum, torch.float32, "accum", 2)
        if table.shape[1] != dim or plan.n_ids != n_ids or tuple(grads.shape) != (n_ids, dim):
            raise RuntimeError("optimizer_step_: every table needs the same dim, the same number of ids and [n_ids, dim] gradients")
        arr_t[i] = _lib.SparseTable(_p(table), _p(accum), table.shape[0], _p(grads), _p(plan.sorted_ids), _p(plan.order),
                                    _p(plan.apply_ws(dim)))
    arr_s = (DenseSeg * len(segs))(*segs)
    _lib.check(_lib.load().tt_optimizer_step_f32(_OPT[opt], arr_t, len(tables), dim, n_ids, arr_s, len(segs), lr, eps, _stream()),
               "tt_optimizer_step_f32")


def sparse_plan_max_lds_ids() -> int:
    """Longest id list the one-launch LDS sort takes: 16384."""
    return int(_lib.load().tt_sparse_plan_max_lds_ids())


def optimizer_ids_max_ids() -> int:
    """Longest id list per table the optimizer step from raw ids takes: 65536 (beyond 16384: the long-list kernel)."""
    return int(_lib.load().tt_optimizer_ids_max_ids())


def id_range_load_(out_max: torch.Tensor, ids_list, table_rows, dim: int, segs: list[DenseSeg]):
    """Skew probe (``tt_id_range_load``): out_max[t] (int32, device) = the most ids of ``ids_list[t]`` in one of table t's row
    ranges - what ONE workgroup of the one-launch optimizer would have to sort and apply.  One small launch; the caller copies
    ``out_max`` to pinned host memory without waiting (TwoTowerTrainer.poll_ids)."""
    n = len(ids_list)
    _chk(out_max, torch.int32, "out_max", 1)
    if out_max.numel() < n:
        raise RuntimeError("id_range_load_: out_max needs one int32 per table")
    for ids in ids_list:
        _chk(ids, torch.int64, "ids", 1)
        if ids.numel() != ids_list[0].numel():
            raise RuntimeError("id_range_load_: every table needs the same number of ids")
    ptrs = (_lib.C.c_void_p * n)(*[ids.data_ptr() for ids in ids_list])
    rows = (_lib.C.c_int64 * n)(*[int(r) for r in table_rows])
    arr_s = (DenseSeg * len(segs))(*segs)
    _lib.check(_lib.load().tt_id_range_load(ptrs, rows, n, dim, ids_list[0].numel(), arr_s, len(segs), _p(out_max), _stream()),
               "tt_id_range_load")
    return out_max


def optimizer_step_ids_(opt: str, tables, segs: list[DenseSeg], lr: float, eps: float = 1e-7, buckets=None):
    """The same step from the RAW ids, no sort-plan launch: ``tables`` = [(table, accum or None, grads, ids, plan), ...]
    (``plan`` only lends its apply workspace); n_ids <= optimizer_ids_max_ids().  Bit-identical to
    ``sparse_plan_batched`` + ``optimizer_step_``."""
    dim, n_ids = tables[0][0].shape[1], tables[0][3].numel()
    arr_t = (_lib.SparseTableIds * len(tables))()
    for i, (table, accum, grads, ids, plan) in enumerate(tables):
        _chk(table, torch.float32, "table", 2)
        _chk(grads, torch.float32, "grads", 2)
        _chk(ids, torch.int64, "ids", 1)
        if accum is not None:
            _chk(accum, torch.float32, "accum", 2)
            if accum.shape != table.shape:
                raise RuntimeError("optimizer_step_ids_: accum must have the table's shape")
        if table.shape[1] != dim or ids.numel() != n_ids or plan.n_ids != n_ids or tuple(grads.shape) != (n_ids, dim):
            raise RuntimeError("optimizer_step_ids_: every table needs the same dim, the same number of ids and [n_ids, dim] gradients")
        arr_t[i] = _lib.SparseTableIds(_p(table), _p(accum), table.shape[0], _p(grads), _p(ids), _p(plan.apply_ws(dim)))
        if buckets is not None and buckets[i] is not None:       # the row-range lists this step's forward lookup filled
            arr_t[i].buckets = buckets[i]
    arr_s = (DenseSeg * len(segs))(*segs)
    _lib.check(_lib.load().tt_optimizer_step_ids_f32(_OPT[opt], arr_t, len(tables), dim, n_ids, arr_s, len(segs), lr, eps, _stream()),
               "tt_optimizer_step_ids_f32")


def make_dense_seg(param, accum, grad_slabs, n_slabs: int, l2: float, grad_out=None, slab_stride: int | None = None) -> DenseSeg:
    """``slab_stride`` (default: the parameter's size): floats between two slabs of ``grad_slabs``."""
    count = param.numel()
    return DenseSeg(_p(param), _p(accum), _p(grad_slabs), _p(grad_out), count, count if slab_stride is None else int(slab_stride),
                    n_slabs, l2)


# ----------------------------------------------------------------------------- global-norm gradient clipping
CLIP_MODES = {"rows": _lib.TT_CLIP_ROWS, "sum": _lib.TT_CLIP_BAG_SUM, "mean": _lib.TT_CLIP_BAG_MEAN, "sqrtn": _lib.TT_CLIP_BAG_SQRTN,
              "mask": _lib.TT_CLIP_SLOT_MASK}


def make_clip_rows(grads, weight: float = 1.0, slot_ids=None, mode: str = "rows") -> "_lib.ClipBuffer":
    """One gradient-row buffer of ``clip_global_norm_``: ``grads`` [rows, dim] f32, row r counts ``weight`` + w(mode) times -
    "rows": nothing more; "sum" / "mean" / "sqrtn": ``slot_ids`` [rows, L] int64, n_r = its entries >= 0, + n_r / 1 / n_r / 1 (an
    empty bag: 0); "mask": ``slot_ids`` [rows] int64, + 1 where the id is >= 0.  The caller keeps the tensors alive."""
    _chk(grads, torch.float32, "grads", 2)
    if mode not in CLIP_MODES:
        raise ValueError(f"make_clip_rows: mode must be one of {tuple(CLIP_MODES)}, got {mode!r}")
    rows, dim = grads.shape
    L = 0
    if mode == "rows":
        slot_ids = None
    else:
        _chk(slot_ids, torch.int64, "slot_ids")
        if slot_ids.numel() == 0 and rows:
            raise RuntimeError("make_clip_rows: slot_ids is empty")
        L = 1 if mode == "mask" else slot_ids.numel() // max(rows, 1)
        if slot_ids.numel() != rows * L:
            raise RuntimeError(f"make_clip_rows: slot_ids must hold rows * L ids (mask: one per row), got {slot_ids.numel()} for {rows} rows")
    return _lib.ClipBuffer(_p(grads), _p(slot_ids), rows, 0, 0, dim, L, 0, CLIP_MODES[mode], float(weight), 0)


def make_clip_dense(grad_slabs, count: int, n_slabs: int = 1, slab_stride: int | None = None) -> "_lib.ClipBuffer":
    """One dense gradient of ``clip_global_norm_``: ``n_slabs`` slabs of ``count`` floats, ``slab_stride`` (default count) apart,
    which are summed (slab order) before they are squared - what ``make_dense_seg`` / ``make_adam_seg`` hand the optimizer."""
    _chk(grad_slabs, torch.float32, "grad_slabs")
    stride = int(count) if slab_stride is None else int(slab_stride)
    if n_slabs >= 1 and count >= 0 and grad_slabs.numel() < (n_slabs - 1) * stride + count:
        raise RuntimeError("make_clip_dense: grad_slabs must hold n_slabs slabs of slab_stride >= count floats")
    return _lib.ClipBuffer(_p(grad_slabs), None, 0, int(count), stride, 0, 0, int(n_slabs), _lib.TT_CLIP_DENSE, 0.0, 0)


class ClipList:
    """The buffer list of ``clip_global_norm_``, built once for buffers that stay where they are: ``row_buffers`` =
    ``make_clip_rows`` descriptors, ``dense_segs`` = ``make_clip_dense`` descriptors or the optimizer's own segments
    (``make_dense_seg`` / ``make_adam_seg``: their gradient slabs are taken).  ``workspace_bytes``: what the call needs."""

    def __init__(self, row_buffers, dense_segs=()):
        bufs = list(row_buffers)
        for s in dense_segs:
            bufs.append(s if isinstance(s, _lib.ClipBuffer) else
                        _lib.ClipBuffer(s.grad_slabs, None, 0, s.count, s.slab_stride, 0, 0, s.n_slabs, _lib.TT_CLIP_DENSE, 0.0, 0))
        if len(bufs) > _lib.TT_CLIP_MAX_BUFFERS:
            raise ValueError(f"clip_global_norm_: at most {_lib.TT_CLIP_MAX_BUFFERS} buffers per call (got {len(bufs)})")
        self.n = len(bufs)
        self.arr = (_lib.ClipBuffer * max(self.n, 1))(*bufs)
        self.workspace_bytes = int(_lib.load().tt_clip_workspace_bytes(self.arr, self.n))
        if self.workspace_bytes < 0:
            raise ValueError("clip_global_norm_: " + _lib.load().tt_last_error().decode("utf-8", "replace"))


def clip_global_norm_(row_buffers, dense_segs=(), clipnorm: float = 1.0, workspace=None, stats=None):
    """tf.clip_by_global_norm over all the buffers IN PLACE, two launches (``tt_clip_global_norm_f32``): every buffer is
    multiplied by clipnorm / max(norm, clipnorm).  ``row_buffers`` may be a prebuilt ``ClipList`` (then ``dense_segs`` is not
    read).  Returns ``stats`` (2 f32 on the device, unsynchronised): [the norm before clipping, the scale applied]."""
    lst = row_buffers if isinstance(row_buffers, ClipList) else ClipList(row_buffers, dense_segs)
    given = [t.device for t in (stats, workspace) if t is not None]
    dev = given[0] if given else torch.device("cuda", torch.cuda.current_device())
    if stats is None:
        stats = torch.empty(2, device=dev)
    _chk(stats, torch.float32, "stats", 1)
    if stats.numel() < 2:
        raise RuntimeError("clip_global_norm_: stats needs 2 floats")
    if workspace is None:
        workspace = torch.empty(lst.workspace_bytes, dtype=torch.uint8, device=dev)
    _chk(workspace, torch.uint8, "workspace")
    _lib.check(_lib.load().tt_clip_global_norm_f32(lst.arr, lst.n, float(clipnorm), _p(workspace), workspace.numel(), _p(stats), _stream()),
               "tt_clip_global_norm_f32")
    return stats


# ----------------------------------------------------------------------------- lazy Adam
def adam_workspace_bytes(n_ids: int, dim: int) -> int:
    """Piece-sum workspace of ``adam_step_`` per table: 256-byte aligned, needs no initialisation; 0 for no ids."""
    return int(_lib.load().tt_adam_workspace_bytes(n_ids, dim))


class AdamHyper:
    """Hyper-parameters of one lazy-Adam step (``tt_adam_hyper``): Keras Adam's defaults and the 1-based global ``step`` the bias
    correction is taken from.  The library computes 1 - beta1, 1 - beta2 and lr * sqrt(1 - beta2^step) / (1 - beta1^step) on the
    host in f64 and rounds each once to f32."""

    def __init__(self, lr: float = 0.001, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-7, step: int = 1):
        self.lr, self.beta1, self.beta2, self.eps, self.step = float(lr), float(beta1), float(beta2), float(eps), int(step)

    def struct(self) -> "_lib.AdamHyper":
        return _lib.AdamHyper(self.lr, self.beta1, self.beta2, self.eps, self.step)


def make_adam_seg(param, m, v, grad_slabs, n_slabs: int, l2: float, slab_stride: int | None = None) -> "_lib.AdamSeg":
    """One dense segment of ``adam_step_``: ``param``, ``m``, ``v`` [count] and ``grad_slabs`` [n_slabs][slab_stride]."""
    for t, name in ((param, "param"), (m, "m"), (v, "v"), (grad_slabs, "grad_slabs")):
        _chk(t, torch.float32, name)
    count = param.numel()
    stride = count if slab_stride is None else int(slab_stride)
    if m.numel() != count or v.numel() != count:
        raise RuntimeError("make_adam_seg: m and v must have the parameter's size")
    if n_slabs < 1 or stride < count or grad_slabs.numel() < (n_slabs - 1) * stride + count:
        raise RuntimeError("make_adam_seg: grad_slabs must hold n_slabs slabs of slab_stride >= count floats")
    return _lib.AdamSeg(_p(param), _p(m), _p(v), _p(grad_slabs), count, stride, n_slabs, l2)


def adam_step_(tables, segs, hyper: AdamHyper):
    """One lazy-Adam step (``tt_adam_step_f32``: two launches): ``tables`` = [(table, m, v, grads, plan), ...] - up to 3 embedding
    tables of one width whose plans (``sparse_plan_batched`` / ``SparsePlan.run``) hold the same number of ids - and ``segs`` =
    ``make_adam_seg`` descriptions of the dense parameters.  Either list may be empty.  Only the rows of the plans' ids change."""
    for table, m, v, grads, _ in tables:
        _chk(table, torch.float32, "table", 2)
        _chk(m, torch.float32, "m", 2)
        _chk(v, torch.float32, "v", 2)
        _chk(grads, torch.float32, "grads", 2)
    dim, n_ids = (tables[0][0].shape[1], tables[0][4].n_ids) if tables else (4, 0)
    arr_t = (_lib.AdamTable * max(len(tables), 1))()
    for i, (table, m, v, grads, plan) in enumerate(tables):
        if m.shape != table.shape or v.shape != table.shape:
            raise RuntimeError("adam_step_: m and v must have the table's shape")
        if table.shape[1] != dim or plan.n_ids != n_ids or tuple(grads.shape) != (plan.grad_rows, dim):
            raise RuntimeError("adam_step_: every table needs the same dim, the same number of ids and [n_ids, dim] gradients "
                               "([n_bags, dim] with a BagPlan)")
        arr_t[i] = _lib.AdamTable(_p(table), _p(m), _p(v), table.shape[0], _p(grads), _p(plan.sorted_ids), _p(plan.grad_order),
                                  _p(plan.adam_ws(dim)))
    arr_s = (_lib.AdamSeg * max(len(segs), 1))(*segs)
    h = hyper.struct()
    _lib.check(_lib.load().tt_adam_step_f32(arr_t, len(tables), dim, n_ids, arr_s, len(segs), C.byref(h), _stream()),
               "tt_adam_step_f32")


# ----------------------------------------------------------------------------- row-wise Adagrad
def rowwise_adagrad_workspace_bytes(n_ids: int, dim: int) -> int:
    """Piece-sum workspace of ``rowwise_adagrad_step_`` per table: 256-byte aligned, needs no initialisation; 0 for no ids."""
    return int(_lib.load().tt_rowwise_adagrad_workspace_bytes(n_ids, dim))


def rowwise_adagrad_step_(tables, segs, lr: float, eps: float = 1e-7):
    """One row-wise Adagrad step (``tt_rowwise_adagrad_step_f32``: two launches): ``tables`` = [(table, row_accum, grads, plan),
    ...] - up to 3 embedding tables of one width whose plans (``sparse_plan_batched`` / ``SparsePlan.run``) hold the same number
    of ids, each with ONE accumulator float per row (``row_accum`` [rows]) - and ``segs`` = the ``make_dense_seg`` descriptions of
    the dense parameters (with their element-wise Adagrad accumulators), which take the plain Adagrad update.  Either list may
    be empty.  Only the rows of the plans' ids change, their accumulators included."""
    for table, row_accum, grads, _ in tables:
        _chk(table, torch.float32, "table", 2)
        _chk(row_accum, torch.float32, "row_accum", 1)
        _chk(grads, torch.float32, "grads", 2)
    dim, n_ids = (tables[0][0].shape[1], tables[0][3].n_ids) if tables else (4, 0)
    arr_t = (_lib.RowwiseTable * max(len(tables), 1))()
    for i, (table, row_accum, grads, plan) in enumerate(tables):
        if row_accum.numel() != table.shape[0]:
            raise RuntimeError(f"rowwise_adagrad_step_: row_accum must be [rows] = [{table.shape[0]}] (one float per table row), "
                               f"got {tuple(row_accum.shape)}")
        if table.shape[1] != dim or plan.n_ids != n_ids or tuple(grads.shape) != (plan.grad_rows, dim):
            raise RuntimeError("rowwise_adagrad_step_: every table needs the same dim, the same number of ids and [n_ids, dim] "
                               "gradients ([n_bags, dim] with a BagPlan)")
        arr_t[i] = _lib.RowwiseTable(_p(table), _p(row_accum), table.shape[0], _p(grads), _p(plan.sorted_ids), _p(plan.grad_order),
                                     _p(plan.rowwise_ws(dim)))
    arr_s = (_lib.DenseSeg * max(len(segs), 1))(*segs)
    _lib.check(_lib.load().tt_rowwise_adagrad_step_f32(arr_t, len(tables), dim, n_ids, arr_s, len(segs), float(lr), float(eps),
                                                       _stream()), "tt_rowwise_adagrad_step_f32")


# ----------------------------------------------------------------------------- L2-normalised tower outputs
L2_NORMALIZE_EPS = 1e-12            # tf.math.l2_normalize's default (a floor of the SUM OF SQUARES)


def _l2_shape(groups, what: str):
    """(rows, dim) shared by every tensor of every problem (1 or 2 problems: the towers of one launch)."""
    n = len(groups[0])
    if n not in (1, 2) or any(len(g) != n for g in groups):
        raise ValueError(f"{what}: one or two problems, every argument a tuple of that length")
    for g in groups:
        for t in g:
            _chk(t, torch.float32, what, 2)
            if t.shape != groups[0][0].shape:
                raise RuntimeError(f"{what}: every tensor must be [{groups[0][0].shape[0]}, {groups[0][0].shape[1]}], "
                                   f"got {tuple(t.shape)}")
    return n, groups[0][0].shape[0], groups[0][0].shape[1]


def l2_normalize2(xs, ys, eps: float = L2_NORMALIZE_EPS):
    """ys[i] = xs[i] / sqrt(max(sum(xs[i]^2, axis=1), eps)) (tf.math.l2_normalize) for one or two [rows, dim] problems
    - both towers' outputs - in ONE launch (``tt_l2_normalize_fwd_f32``).  ys[i] must not be xs[i]."""
    n, rows, dim = _l2_shape((xs, ys), "l2_normalize2")
    arr = (_lib.L2NormFwdArgs * n)(*[_lib.L2NormFwdArgs(_p(xs[i]), _p(ys[i])) for i in range(n)])
    _lib.check(_lib.load().tt_l2_normalize_fwd_f32(arr, n, rows, dim, eps, _stream()), "tt_l2_normalize_fwd_f32")
    return ys


def l2_normalize_bwd2(xs, dys, dxs, eps: float = L2_NORMALIZE_EPS):
    """dxs[i] = gradient of l2_normalize2 at xs[i] given dys[i], for one or two problems in ONE launch
    (``tt_l2_normalize_bwd_f32``: the row sums are recomputed from xs, nothing is saved by the forward).  dxs[i] may be dys[i]."""
    n, rows, dim = _l2_shape((xs, dys, dxs), "l2_normalize_bwd2")
    arr = (_lib.L2NormBwdArgs * n)(*[_lib.L2NormBwdArgs(_p(xs[i]), _p(dys[i]), _p(dxs[i])) for i in range(n)])
    _lib.check(_lib.load().tt_l2_normalize_bwd_f32(arr, n, rows, dim, eps, _stream()), "tt_l2_normalize_bwd_f32")
    return dxs


def l2_normalize(x, out=None, eps: float = L2_NORMALIZE_EPS):
    """One-tower form of ``l2_normalize2``."""
    out = torch.empty_like(x) if out is None else out
    return l2_normalize2((x,), (out,), eps)[0]


def l2_normalize_bwd(x, dy, out=None, eps: float = L2_NORMALIZE_EPS):
    """One-tower form of ``l2_normalize_bwd2``."""
    out = torch.empty_like(x) if out is None else out
    return l2_normalize_bwd2((x,), (dy,), (out,), eps)[0]


# ----------------------------------------------------------------------------- dense numeric side features
MAX_DENSE_FEATURES = 32


def dense_features(*problems, clip: float = 0.0, oob_flag: torch.Tensor | None = None):
    """The numeric side-feature branch of a tower input (Keras Normalization -> Dense without bias) for one or two problems -
    both towers - in ONE launch (``tt_dense_features_fwd_f32``).  Every problem is the tuple
    ``(feat, ids, mean, inv_std, proj, out, accumulate, z_out)``: ``feat`` [rows, F] f32 (1 <= F <= 32), ``ids`` [n] int64,
    ``mean`` / ``inv_std`` [F] f32 (both None: no normalisation), ``proj`` [F, dim] f32, ``out`` [n, dim] f32 (None: allocated;
    must be given with ``accumulate``), ``z_out`` [n, F] f32 or None.
    out[b] (+)= z(feat[ids[b]]) @ proj with z_f = clamp((x_f - mean_f) * inv_std_f, -clip, clip) (``clip`` 0: no clamp), every
    f32 operation rounded on its own, the sum over f ascending from 0.  An id of -1 contributes z = 0; any other id out of
    range does too and sets ``oob_flag`` (int32[1]).  Returns the tuple of the problems' ``out``."""
    if len(problems) not in (1, 2):
        raise ValueError("dense_features: one or two problems")
    if oob_flag is not None:
        _chk(oob_flag, torch.int32, "oob_flag")
    arr = (_lib.DenseFeaturesFwdArgs * len(problems))()
    outs, dim = [], None
    for i, prob in enumerate(problems):
        if len(prob) != 8:
            raise ValueError("dense_features: a problem is (feat, ids, mean, inv_std, proj, out, accumulate, z_out)")
        feat, ids, mean, inv_std, proj, out, accumulate, z_out = prob
        _chk(feat, torch.float32, "feat", 2)
        _chk(ids, torch.int64, "ids", 1)
        _chk(proj, torch.float32, "proj", 2)
        n, F = ids.numel(), feat.shape[1]
        if proj.shape[0] != F:
            raise RuntimeError(f"dense_features: proj must be [{F}, dim] (F = feat.shape[1]), got {tuple(proj.shape)}")
        if dim is None:
            dim = proj.shape[1]
        if proj.shape[1] != dim:
            raise RuntimeError("dense_features: every problem's proj needs the same dim")
        if (mean is None) != (inv_std is None):
            raise ValueError("dense_features: mean and inv_std are given both or neither")
        for t, name in ((mean, "mean"), (inv_std, "inv_std")):
            if t is not None:
                _chk(t, torch.float32, name, 1)
                if t.numel() != F:
                    raise RuntimeError(f"dense_features: {name} must hold F = {F} entries, got {t.numel()}")
        if out is None:
            if accumulate:
                raise ValueError("dense_features: accumulate=True adds into `out`, which must be given")
            out = torch.empty((n, dim), dtype=torch.float32, device=feat.device)
        _chk(out, torch.float32, "out", 2)
        if tuple(out.shape) != (n, dim):
            raise RuntimeError(f"dense_features: out must be [{n}, {dim}] (n, dim), got {tuple(out.shape)}")
        if z_out is not None:
            _chk(z_out, torch.float32, "z_out", 2)
            if tuple(z_out.shape) != (n, F):
                raise RuntimeError(f"dense_features: z_out must be [{n}, {F}] (n, F), got {tuple(z_out.shape)}")
        arr[i] = _lib.DenseFeaturesFwdArgs(_p(feat), feat.shape[0], F, int(bool(accumulate)), _p(ids), n, _p(mean), _p(inv_std),
                                           _p(proj), _p(out), _p(z_out))
        outs.append(out)
    _lib.check(_lib.load().tt_dense_features_fwd_f32(arr, len(problems), dim, float(clip), _p(oob_flag), _stream()),
               "tt_dense_features_fwd_f32")
    return tuple(outs)


def dense_features_num_slabs(n: int) -> int:
    """Slab count of ``dense_features_bwd`` for ``n`` rows (``tt_dense_features_num_slabs``, a host query)."""
    return int(_lib.load().tt_dense_features_num_slabs(n))


def dense_features_bwd(*problems):
    """The projection kernels' gradients for one or two problems in ONE launch (``tt_dense_features_bwd_f32``).  Every problem is
    ``(z, dy, dp_slabs)``: ``z`` [n, F] (the forward's ``z_out``), ``dy`` [n, dim] (the gradient w.r.t. the tower input rows),
    ``dp_slabs`` [n_slabs, F, dim] (None: allocated with ``dense_features_num_slabs(n)`` slabs).  Slab s is written with the
    sum of z[b, f] * dy[b, d] over its ceil(n / n_slabs) contiguous rows - every slab in full, an empty one as zeros: the form
    ``make_dense_seg`` / ``make_adam_seg`` sum.  Returns the tuple of the problems' ``dp_slabs``."""
    if len(problems) not in (1, 2):
        raise ValueError("dense_features_bwd: one or two problems")
    arr = (_lib.DenseFeaturesBwdArgs * len(problems))()
    outs, dim = [], None
    for i, prob in enumerate(problems):
        if len(prob) != 3:
            raise ValueError("dense_features_bwd: a problem is (z, dy, dp_slabs)")
        z, dy, dp = prob
        _chk(z, torch.float32, "z", 2)
        _chk(dy, torch.float32, "dy", 2)
        n, F = z.shape
        if dim is None:
            dim = dy.shape[1]
        if tuple(dy.shape) != (n, dim):
            raise RuntimeError(f"dense_features_bwd: dy must be [{n}, {dim}] (n, dim), got {tuple(dy.shape)}")
        if dp is None:
            dp = torch.empty((dense_features_num_slabs(n), F, dim), dtype=torch.float32, device=z.device)
        _chk(dp, torch.float32, "dp_slabs", 3)
        if tuple(dp.shape[1:]) != (F, dim) or dp.shape[0] < 1:
            raise RuntimeError(f"dense_features_bwd: dp_slabs must be [n_slabs, {F}, {dim}], got {tuple(dp.shape)}")
        arr[i] = _lib.DenseFeaturesBwdArgs(_p(z), _p(dy), n, F, dp.shape[0], _p(dp))
        outs.append(dp)
    _lib.check(_lib.load().tt_dense_features_bwd_f32(arr, len(problems), dim, _stream()), "tt_dense_features_bwd_f32")
    return tuple(outs)


# ----------------------------------------------------------------------------- time-of-interaction context features
TIME_FIELDS = ("hour", "day_of_week", "month", "period")       # the fixed field order (bit f of the C ABI's field_mask)
TIME_FIELD_ROWS = {"hour": 24, "day_of_week": 7, "month": 12}  # "period": the caller's bucket count
TIME_MISSING = -2 ** 63                                         # a pair without a timestamp
MAX_TIME_BUCKETS = 4096


def _time_fields(fields, buckets: int):
    """The validated (fields in the fixed order, field_mask) of a field selection."""
    fields = tuple(fields)
    bad = [f for f in fields if f not in TIME_FIELDS]
    if bad or not fields or len(set(fields)) != len(fields):
        raise ValueError(f"time fields must be a non-empty subset of {TIME_FIELDS} without repeats, got {fields!r}")
    if isinstance(buckets, bool) or not isinstance(buckets, int):
        raise ValueError("time buckets must be an int")
    if "period" in fields and not 1 <= buckets <= MAX_TIME_BUCKETS:
        raise ValueError(f"the 'period' field needs buckets in 1..{MAX_TIME_BUCKETS}, got {buckets}")
    if "period" not in fields and buckets != 0:
        raise ValueError("buckets must be 0 without the 'period' field")
    ordered = tuple(f for f in TIME_FIELDS if f in fields)
    return ordered, sum(1 << TIME_FIELDS.index(f) for f in ordered)


def time_field_layout(fields, buckets: int = 0):
    """(offsets, R) of the time table: ``offsets[f]`` = first row of enabled field f's block, in the fixed field order (hour 24
    rows, day_of_week 7, month 12, period ``buckets``); R = the rows of the table.  A host function (no device, no library)."""
    ordered, _ = _time_fields(fields, buckets)
    offsets, r = {}, 0
    for f in ordered:
        offsets[f] = r
        r += buckets if f == "period" else TIME_FIELD_ROWS[f]
    return offsets, r


def _chk_time_range(time_min: int, time_max: int):
    for v, name in ((time_min, "time_min"), (time_max, "time_max")):
        if isinstance(v, bool) or not isinstance(v, int) or not -2 ** 63 <= v < 2 ** 63:
            raise ValueError(f"{name} must be an int64")
    if time_min > time_max or time_max - time_min >= 2 ** 40:
        raise ValueError("need time_min <= time_max and time_max - time_min < 2^40")


def time_context(timestamps: torch.Tensor, table: torch.Tensor, fields, buckets: int, time_min: int, time_max: int,
                 out: torch.Tensor | None = None, accumulate: bool = False, base=None, idx_out: torch.Tensor | None = None,
                 oob_flag: torch.Tensor | None = None) -> torch.Tensor:
    """out[p] (+)= the sum, in field order, of the time table's rows a pair's timestamp picks (``tt_time_context_fwd_f32``).
    ``timestamps`` [n] int64 (whole seconds since the epoch, UTC; ``TIME_MISSING``: adds nothing, indices -1); ``table``
    [R, dim] f32 (``time_field_layout``); ``base`` = (base_table [rows, dim], base_ids [n] int64): out[p] = base_table[base_ids[p]]
    + the sum, in ONE launch (in the place of ``accumulate``; an out-of-range base id: a zero row and ``oob_flag``);
    ``idx_out`` [n, F] int32: the F row indices of every pair, for ``time_context_bwd``."""
    ordered, mask = _time_fields(fields, buckets)
    _chk_time_range(time_min, time_max)
    _chk(timestamps, torch.int64, "timestamps", 1)
    _chk(table, torch.float32, "table", 2)
    n, (rows, d) = timestamps.numel(), table.shape
    if rows != time_field_layout(ordered, buckets)[1]:
        raise RuntimeError(f"time_context: the table must have {time_field_layout(ordered, buckets)[1]} rows for {ordered}, got {rows}")
    if base is not None and accumulate:
        raise ValueError("time_context: the base row takes the place of out's row: accumulate must be False with a base")
    if out is None:
        if accumulate:
            raise ValueError("time_context: accumulate=True adds into `out`, which must be given")
        out = torch.empty((n, d), dtype=torch.float32, device=table.device)
    _chk(out, torch.float32, "out", 2)
    if tuple(out.shape) != (n, d):
        raise RuntimeError(f"time_context: out must be [{n}, {d}] (n, dim), got {tuple(out.shape)}")
    base_table = base_ids = None
    if base is not None:
        base_table, base_ids = base
        _chk(base_table, torch.float32, "base_table", 2)
        _chk(base_ids, torch.int64, "base_ids", 1)
        if base_table.shape[1] != d or base_ids.numel() != n:
            raise RuntimeError(f"time_context: base must be ([rows, {d}] f32, [{n}] int64), got {tuple(base_table.shape)} and "
                               f"{tuple(base_ids.shape)}")
    if idx_out is not None:
        _chk(idx_out, torch.int32, "idx_out", 2)
        if tuple(idx_out.shape) != (n, len(ordered)):
            raise RuntimeError(f"time_context: idx_out must be [{n}, {len(ordered)}] (n, fields), got {tuple(idx_out.shape)}")
    if oob_flag is not None:
        _chk(oob_flag, torch.int32, "oob_flag")
    _lib.check(_lib.load().tt_time_context_fwd_f32(_p(timestamps), n, _p(table), rows, d, mask, buckets, time_min, time_max, _p(out),
                                                   int(bool(accumulate)), _p(base_table),
                                                   0 if base_table is None else base_table.shape[0], _p(base_ids), _p(idx_out),
                                                   _p(oob_flag), _stream()), "tt_time_context_fwd_f32")
    return out


def time_context_bwd(idx: torch.Tensor, dy: torch.Tensor, fields, buckets: int, grad: torch.Tensor | None = None) -> torch.Tensor:
    """The time table's fully reduced gradient [R, dim] from the forward's ``idx`` [n, F] int32 and ``dy`` [n, dim]
    (``tt_time_context_bwd_f32``): one launch, no atomics, every row written (a row nobody hit: zeros - ``grad`` need not be
    cleared), the summation order a fixed function of (n, idx)."""
    ordered, mask = _time_fields(fields, buckets)
    rows = time_field_layout(ordered, buckets)[1]
    _chk(idx, torch.int32, "idx", 2)
    _chk(dy, torch.float32, "dy", 2)
    n, d = dy.shape
    if tuple(idx.shape) != (n, len(ordered)):
        raise RuntimeError(f"time_context_bwd: idx must be [{n}, {len(ordered)}] (n, fields), got {tuple(idx.shape)}")
    if grad is None:
        grad = torch.empty((rows, d), dtype=torch.float32, device=dy.device)
    _chk(grad, torch.float32, "grad", 2)
    if tuple(grad.shape) != (rows, d):
        raise RuntimeError(f"time_context_bwd: grad must be [{rows}, {d}] (R, dim), got {tuple(grad.shape)}")
    _lib.check(_lib.load().tt_time_context_bwd_f32(_p(idx), _p(dy), n, d, mask, buckets, rows, _p(grad), _stream()),
               "tt_time_context_bwd_f32")
    return grad


# ----------------------------------------------------------------------------- rating-prediction head
RATING_DIMS = (32, 64, 128, 256)


def _chk_rating_head(what: str, q, c, w1, w2):
    _chk(q, torch.float32, "q", 2)
    _chk(c, torch.float32, "c", 2)
    _chk(w1, torch.float32, "W1", 2)
    _chk(w2, torch.float32, "w2", 1)
    n, d = q.shape
    h = w2.numel()
    if tuple(c.shape) != (n, d):
        raise RuntimeError(f"{what}: q and c must have one shape [n, D], got {tuple(q.shape)} and {tuple(c.shape)}")
    if tuple(w1.shape) != (2 * d, h):
        raise RuntimeError(f"{what}: W1 must be [2 D, H] = [{2 * d}, {h}], got {tuple(w1.shape)}")
    return n, d, h


def rating_head(q, c, w1, b1, w2, b2, pred=None, h=None):
    """The rating head's forward pass in ONE launch (``tt_rating_head_fwd_f32``): ``q``, ``c`` [n, D] (D in 32 / 64 / 128 / 256),
    ``w1`` [2 D, H] (rows 0..D-1 multiply q, rows D..2D-1 multiply c; H a multiple of 32 in 32..256), ``b1`` [H], ``w2`` [H],
    ``b2`` [1]:  h = relu(b1 + q @ w1[:D] + c @ w1[D:]),  pred = b2 + h @ w2.  Returns (pred [n], h [n, H]); both may be
    given (views of longer buffers are fine: nothing past row n is touched)."""
    n, d, hd = _chk_rating_head("rating_head", q, c, w1, w2)
    _chk(b1, torch.float32, "b1", 1)
    _chk(b2, torch.float32, "b2", 1)
    if b1.numel() != hd or b2.numel() != 1:
        raise RuntimeError(f"rating_head: b1 must hold H = {hd} entries and b2 one, got {b1.numel()} and {b2.numel()}")
    pred = torch.empty(n, dtype=torch.float32, device=q.device) if pred is None else pred
    h = torch.empty((n, hd), dtype=torch.float32, device=q.device) if h is None else h
    _chk(pred, torch.float32, "pred", 1)
    _chk(h, torch.float32, "h", 2)
    if pred.numel() != n or tuple(h.shape) != (n, hd):
        raise RuntimeError(f"rating_head: pred must be [{n}] and h [{n}, {hd}], got {tuple(pred.shape)} and {tuple(h.shape)}")
    _lib.check(_lib.load().tt_rating_head_fwd_f32(_p(q), _p(c), n, d, hd, _p(w1), _p(b1), _p(w2), _p(b2), _p(pred), _p(h), _stream()),
               "tt_rating_head_fwd_f32")
    return pred, h


def rating_head_num_slabs(n: int) -> int:
    """Slab count of ``rating_head_bwd`` for ``n`` pairs (``tt_rating_head_num_slabs``, a host query)."""
    return int(_lib.load().tt_rating_head_num_slabs(n))


def rating_head_bwd(q, c, h, pred, rating, w1, w2, grad_scale: float, dq, dc, kslabs=None, bslabs=None, se_slabs=None,
                    sample_weight=None, accumulate: bool = False, n_slabs: int | None = None):
    """The rating head's backward pass for the MSE loss in ONE launch (``tt_rating_head_bwd_f32``).  With e = pred - rating
    (a non-finite rating: a missing label, no gradient), w = sample_weight (None: 1) and g = grad_scale * w * e:
    dq / dc [n, D] receive (``accumulate``: are added) the gradient w.r.t. q / c; ``kslabs`` [n_slabs, 2 D H + H] the slabs of
    dW1 (row-major) followed by dw2, ``bslabs`` [n_slabs, H + 1] those of db1 followed by db2, ``se_slabs`` [n_slabs] the
    slabs' sums of w e^2.  Slab s covers ceil(n / n_slabs) contiguous rows; every slab is written in full (an empty one as
    zeros).  Buffers not given are allocated with ``n_slabs`` (default ``rating_head_num_slabs(n)``) slabs.
    Returns (dq, dc, kslabs, bslabs, se_slabs)."""
    n, d, hd = _chk_rating_head("rating_head_bwd", q, c, w1, w2)
    _chk(h, torch.float32, "h", 2)
    _chk(pred, torch.float32, "pred", 1)
    _chk(rating, torch.float32, "rating", 1)
    _chk(dq, torch.float32, "dq", 2)
    _chk(dc, torch.float32, "dc", 2)
    if tuple(h.shape) != (n, hd) or pred.numel() != n or rating.numel() != n:
        raise RuntimeError(f"rating_head_bwd: h must be [{n}, {hd}], pred and rating [{n}]")
    if tuple(dq.shape) != (n, d) or tuple(dc.shape) != (n, d):
        raise RuntimeError(f"rating_head_bwd: dq and dc must be [{n}, {d}], got {tuple(dq.shape)} and {tuple(dc.shape)}")
    if sample_weight is not None:
        _chk(sample_weight, torch.float32, "sample_weight", 1)
        if sample_weight.numel() != n:
            raise RuntimeError(f"rating_head_bwd: sample_weight must hold n = {n} entries")
    if n_slabs is None:
        n_slabs = kslabs.shape[0] if kslabs is not None else rating_head_num_slabs(n)
    ks = 2 * d * hd + hd
    kslabs = torch.empty((n_slabs, ks), dtype=torch.float32, device=q.device) if kslabs is None else kslabs
    bslabs = torch.empty((n_slabs, hd + 1), dtype=torch.float32, device=q.device) if bslabs is None else bslabs
    se_slabs = torch.empty(n_slabs, dtype=torch.float32, device=q.device) if se_slabs is None else se_slabs
    for t, name, shape in ((kslabs, "kslabs", (n_slabs, ks)), (bslabs, "bslabs", (n_slabs, hd + 1)), (se_slabs, "se_slabs", (n_slabs,))):
        _chk(t, torch.float32, name)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"rating_head_bwd: {name} must be {list(shape)}, got {list(t.shape)}")
    _lib.check(_lib.load().tt_rating_head_bwd_f32(_p(q), _p(c), _p(h), _p(pred), _p(rating), _p(sample_weight), float(grad_scale),
                                                  n, d, hd, _p(w1), _p(w2), _p(dq), _p(dc), int(bool(accumulate)),
                                                  _p(kslabs), _p(bslabs), _p(se_slabs), int(n_slabs), _stream()),
               "tt_rating_head_bwd_f32")
    return dq, dc, kslabs, bslabs, se_slabs


# ----------------------------------------------------------------------------- DCN-v2 cross layer
def _chk_cross(what: str, x0, x, w):
    _chk(x0, torch.float32, "x0", 2)
    _chk(x, torch.float32, "x", 2)
    _chk(w, torch.float32, "w", 2)
    n, d = x0.shape
    if tuple(x.shape) != (n, d) or tuple(w.shape) != (d, d):
        raise RuntimeError(f"{what}: x0 and x must be [n, D] and w [D, D], got {tuple(x0.shape)}, {tuple(x.shape)} and {tuple(w.shape)}")
    return n, d


def cross_layer(*problems, u=None):
    """One DCN-v2 cross layer (tfrs.layers.dcn.Cross) for one or two problems - both towers - in ONE launch
    (``tt_cross_fwd_f32``).  Every problem is ``(x0, x, w, b, y)``: ``x0`` [n, D] the summed input rows, ``x`` [n, D] the layer's
    input (``x0`` itself at layer 0), ``w`` [D, D] ([in, out]), ``b`` [D], ``y`` [n, D] or None (allocated); D a multiple of 32
    in 32..256, every problem with its own n.  y = x0 * (x @ w + b) + x, the product and the sum rounded separately.
    ``u``: None (inference) or one [n, D] buffer per problem that receives u = x @ w + b for ``cross_layer_bwd``.  ``y`` and
    ``u`` must not alias ``x`` / ``x0``.  Returns the tuple of the problems' ``y``."""
    if len(problems) not in (1, 2):
        raise ValueError("cross_layer: one or two problems")
    us = (None,) * len(problems) if u is None else ((u,) if isinstance(u, torch.Tensor) else tuple(u))
    if len(us) != len(problems):
        raise ValueError("cross_layer: u holds one buffer per problem")
    arr = (_lib.CrossFwdArgs * len(problems))()
    outs, dim = [], None
    for i, prob in enumerate(problems):
        if len(prob) != 5:
            raise ValueError("cross_layer: a problem is (x0, x, w, b, y)")
        x0, x, w, b, y = prob
        n, d = _chk_cross("cross_layer", x0, x, w)
        _chk(b, torch.float32, "b", 1)
        if dim is None:
            dim = d
        if d != dim or b.numel() != d:
            raise RuntimeError("cross_layer: every problem needs the same D, and b must hold D entries")
        y = torch.empty((n, d), dtype=torch.float32, device=x.device) if y is None else y
        _chk(y, torch.float32, "y", 2)
        if tuple(y.shape) != (n, d):
            raise RuntimeError(f"cross_layer: y must be [{n}, {d}], got {tuple(y.shape)}")
        if us[i] is not None:
            _chk(us[i], torch.float32, "u", 2)
            if tuple(us[i].shape) != (n, d):
                raise RuntimeError(f"cross_layer: u must be [{n}, {d}], got {tuple(us[i].shape)}")
        arr[i] = _lib.CrossFwdArgs(_p(x0), _p(x), _p(w), _p(b), _p(us[i]), _p(y), n)
        outs.append(y)
    _lib.check(_lib.load().tt_cross_fwd_f32(arr, len(problems), dim, _stream()), "tt_cross_fwd_f32")
    return tuple(outs)


def cross_num_slabs(n: int) -> int:
    """Slab count of ``cross_layer_bwd`` for ``n`` rows (``tt_cross_num_slabs``, a host query)."""
    return int(_lib.load().tt_cross_num_slabs(n))


def cross_layer_bwd(*problems, x_is_x0: bool = False, accumulate_dx0: bool = False, n_slabs: int | None = None,
                    slab_stride: int | None = None):
    """The backward pass of one cross layer for one or two problems in ONE launch (``tt_cross_bwd_f32``).  Every problem is
    ``(x0, x, u, w, g, dx, dx0, dw_slabs, db_slabs)``: ``u`` the forward launch's ``u``, ``g`` [n, D] the gradient w.r.t. y.
    With t = g * x0:  upper layers (``x_is_x0`` False): dx = g + t @ w.T and dx0 = g * u (``accumulate_dx0``: dx0 += g * u);
    layer 0 (``x_is_x0``: x is x0): dx = ((g + t @ w.T) + g * u) [+ dx0, read only, may be None].  ``dx`` (None: allocated)
    must not alias g, x0, x or u.  ``dw_slabs`` / ``db_slabs``: flat f32 tensors that START at slab 0 of dW = x.T @ t and of
    db = t.sum(0); slab s sits ``slab_stride`` floats further on, so several layers and both towers can share one
    [n_slabs, slab_stride] array (both None: an [n_slabs, D D + D] array of the problem's own, ``n_slabs`` default
    ``cross_num_slabs(n)``).  Slab s covers ceil(n / n_slabs) contiguous rows; every slab is written in full (an empty one as
    zeros).  Returns one ``(dx, dx0, dw_slabs [n_slabs, D, D], db_slabs [n_slabs, D])`` per problem (views)."""
    if len(problems) not in (1, 2):
        raise ValueError("cross_layer_bwd: one or two problems")
    arr = (_lib.CrossBwdArgs * len(problems))()
    outs, dim = [], None
    for i, prob in enumerate(problems):
        if len(prob) != 9:
            raise ValueError("cross_layer_bwd: a problem is (x0, x, u, w, g, dx, dx0, dw_slabs, db_slabs)")
        x0, x, u, w, g, dx, dx0, dws, dbs = prob
        n, d = _chk_cross("cross_layer_bwd", x0, x, w)
        if dim is None:
            dim = d
        if d != dim:
            raise RuntimeError("cross_layer_bwd: every problem needs the same D")
        if x_is_x0 and x.data_ptr() != x0.data_ptr():
            raise ValueError("cross_layer_bwd: x_is_x0 needs x to be x0")
        dx = torch.empty((n, d), dtype=torch.float32, device=x.device) if dx is None else dx
        if dx0 is None and not x_is_x0:
            if accumulate_dx0:
                raise ValueError("cross_layer_bwd: accumulate_dx0=True adds into `dx0`, which must be given")
            dx0 = torch.empty((n, d), dtype=torch.float32, device=x.device)
        for t, name in ((u, "u"), (g, "g"), (dx, "dx"), (dx0, "dx0")):
            if t is not None:
                _chk(t, torch.float32, name, 2)
                if tuple(t.shape) != (n, d):
                    raise RuntimeError(f"cross_layer_bwd: {name} must be [{n}, {d}], got {tuple(t.shape)}")
        if (dws is None) != (dbs is None):
            raise ValueError("cross_layer_bwd: dw_slabs and db_slabs are given both or neither")
        if dws is None:
            ns = cross_num_slabs(n) if n_slabs is None else int(n_slabs)
            stride = d * d + d
            slabs = torch.empty(max(ns, 1) * stride, dtype=torch.float32, device=x.device)
            dws, dbs = slabs, slabs[d * d:]
        else:
            if n_slabs is None or slab_stride is None:
                raise ValueError("cross_layer_bwd: dw_slabs / db_slabs need n_slabs and slab_stride")
            ns, stride = int(n_slabs), int(slab_stride)
            _chk(dws, torch.float32, "dw_slabs", 1)
            _chk(dbs, torch.float32, "db_slabs", 1)
            if ns >= 1 and (dws.numel() < (ns - 1) * stride + d * d or dbs.numel() < (ns - 1) * stride + d):
                raise RuntimeError("cross_layer_bwd: dw_slabs / db_slabs must reach n_slabs slabs of slab_stride floats")
        arr[i] = _lib.CrossBwdArgs(_p(x0), _p(x), _p(u), _p(w), _p(g), _p(dx), _p(dx0), _p(dws), _p(dbs), n, stride, ns,
                                   int(bool(x_is_x0)), int(bool(accumulate_dx0)))
        outs.append((dx, dx0, dws, dbs, ns, stride, d))
    _lib.check(_lib.load().tt_cross_bwd_f32(arr, len(problems), dim, _stream()), "tt_cross_bwd_f32")
    return tuple((dx, dx0, torch.as_strided(dws, (ns, d, d), (stride, d, 1)), torch.as_strided(dbs, (ns, d), (stride, 1)))
                 for dx, dx0, dws, dbs, ns, stride, d in outs)


# ----------------------------------------------------------------------------- layer normalisation of the hidden layers
LAYER_NORM_EPS = 1e-3          # Keras LayerNormalization's default epsilon


def _chk_layer_norm(what: str, z, gamma):
    _chk(z, torch.float32, "z", 2)
    _chk(gamma, torch.float32, "gamma", 1)
    n, d = z.shape
    if d % 32 or not 32 <= d <= 1024:
        raise RuntimeError(f"{what}: the row width must be a multiple of 32 in 32..1024, got {d}")
    if gamma.numel() != d:
        raise RuntimeError(f"{what}: gamma must hold {d} entries, got {gamma.numel()}")
    return n, d


def layer_norm2(*problems, eps: float = LAYER_NORM_EPS, relu: bool = False, dropout=None):
    """Layer normalisation (Keras LayerNormalization, biased two-pass variance) with an optional ReLU and dropout for one or
    two problems - both towers - in ONE launch (``tt_layer_norm_fwd_f32``).  Every problem is ``(z, gamma, beta, y, relu_bits)``:
    ``z`` [rows, dim] the Dense layer's pre-activation, ``gamma`` / ``beta`` [dim], ``y`` [rows, dim] or None (allocated; must
    not be ``z``), ``relu_bits`` None or a ``relu_bits_like(rows, dim)`` buffer that receives the sign bits of y.  dim is a
    multiple of 32 in 32..1024 and the same in every problem; every problem has its own rows.
    ``dropout`` = (rate, seed, tensor_ids, counter_offset) - ``tensor_ids`` one id or one per problem - applies the inverted
    dropout of ``dense_fwd`` (same stream, same mask) behind the ReLU.  Returns the tuple of the problems' ``y``."""
    if len(problems) not in (1, 2):
        raise ValueError("layer_norm2: one or two problems")
    if not eps > 0:
        raise ValueError(f"layer_norm2: eps must be > 0, got {eps}")
    rate, seed, tids, off = dropout if dropout is not None else (0.0, 0, 0, 0)
    tids = (int(tids),) * len(problems) if not isinstance(tids, (tuple, list)) else tuple(int(t) for t in tids)
    if len(tids) != len(problems):
        raise ValueError("layer_norm2: dropout holds one tensor id per problem")
    arr = (_lib.LayerNormFwdArgs * len(problems))()
    outs, dim = [], None
    for i, prob in enumerate(problems):
        if len(prob) != 5:
            raise ValueError("layer_norm2: a problem is (z, gamma, beta, y, relu_bits)")
        z, gamma, beta, y, bits = prob
        n, d = _chk_layer_norm("layer_norm2", z, gamma)
        _chk(beta, torch.float32, "beta", 1)
        if dim is None:
            dim = d
        if d != dim or beta.numel() != d:
            raise RuntimeError("layer_norm2: every problem needs the same dim, and beta must hold dim entries")
        y = torch.empty((n, d), dtype=torch.float32, device=z.device) if y is None else y
        _chk(y, torch.float32, "y", 2)
        if tuple(y.shape) != (n, d):
            raise RuntimeError(f"layer_norm2: y must be [{n}, {d}], got {tuple(y.shape)}")
        if y.data_ptr() == z.data_ptr() and n:
            raise ValueError("layer_norm2: y must not alias z (the backward pass reads z)")
        _chk_bits(bits, n, d, "layer_norm2: relu_bits")
        arr[i] = _lib.LayerNormFwdArgs(_p(z), _p(gamma), _p(beta), _p(y), _p(bits), tids[i], n)
        outs.append(y)
    _lib.check(_lib.load().tt_layer_norm_fwd_f32(arr, len(problems), dim, float(eps), int(bool(relu)), float(rate), int(seed), int(off),
                                                 _stream()), "tt_layer_norm_fwd_f32")
    return tuple(outs)


def layer_norm_num_slabs(rows: int) -> int:
    """Slab count of ``layer_norm_bwd2`` for ``rows`` rows (``tt_layer_norm_num_slabs``, a host query)."""
    return int(_lib.load().tt_layer_norm_num_slabs(rows))


def layer_norm_bwd2(*problems, eps: float = LAYER_NORM_EPS, n_slabs: int | None = None, slab_stride: int | None = None):
    """The backward pass of ``layer_norm2`` for one or two problems in ONE launch (``tt_layer_norm_bwd_f32``).  Every problem is
    ``(z, gamma, dn, dz, dgamma_slabs, dbeta_slabs)``: ``dn`` [rows, dim] the gradient w.r.t. xhat * gamma + beta (the ReLU /
    dropout mask already applied), ``dz`` [rows, dim], None (allocated) or ``dn`` itself (in place); mean and variance are
    recomputed from ``z``.  ``dgamma_slabs`` / ``dbeta_slabs``: flat f32 tensors that START at slab 0 of
    dgamma = (dn * xhat).sum(0) and dbeta = dn.sum(0); slab s sits ``slab_stride`` floats further on, so all layers and both
    towers can share one [n_slabs, slab_stride] array (both None: an [n_slabs, 2 dim] array of the problem's own).  All
    problems share ``n_slabs`` (default ``layer_norm_num_slabs`` of the longest problem) and ``slab_stride``; slab s covers
    ceil(rows / n_slabs) contiguous rows of its problem and every slab is written in full (an empty one as zeros).  Returns one
    ``(dz, dgamma_slabs [n_slabs, dim], dbeta_slabs [n_slabs, dim])`` per problem (views)."""
    if len(problems) not in (1, 2):
        raise ValueError("layer_norm_bwd2: one or two problems")
    if not eps > 0:
        raise ValueError(f"layer_norm_bwd2: eps must be > 0, got {eps}")
    for prob in problems:
        if len(prob) != 6:
            raise ValueError("layer_norm_bwd2: a problem is (z, gamma, dn, dz, dgamma_slabs, dbeta_slabs)")
    own = [prob[4] is None for prob in problems]
    if any((prob[4] is None) != (prob[5] is None) for prob in problems) or len(set(own)) != 1:
        raise ValueError("layer_norm_bwd2: dgamma_slabs and dbeta_slabs are given both or neither, for every problem alike")
    if own[0]:
        if slab_stride is not None:
            raise ValueError("layer_norm_bwd2: slab_stride belongs to caller-provided slabs")
        ns = max(layer_norm_num_slabs(max(prob[0].shape[0] for prob in problems)), 1) if n_slabs is None else int(n_slabs)
        stride = 2 * problems[0][0].shape[1]
    else:
        if n_slabs is None or slab_stride is None:
            raise ValueError("layer_norm_bwd2: dgamma_slabs / dbeta_slabs need n_slabs and slab_stride")
        ns, stride = int(n_slabs), int(slab_stride)
    if ns < 1:
        raise ValueError(f"layer_norm_bwd2: n_slabs must be >= 1, got {ns}")
    arr = (_lib.LayerNormBwdArgs * len(problems))()
    outs, dim = [], None
    for i, (z, gamma, dn, dz, dgs, dbs) in enumerate(problems):
        n, d = _chk_layer_norm("layer_norm_bwd2", z, gamma)
        if dim is None:
            dim = d
        if d != dim:
            raise RuntimeError("layer_norm_bwd2: every problem needs the same dim")
        dz = torch.empty((n, d), dtype=torch.float32, device=z.device) if dz is None else dz
        for t, name in ((dn, "dn"), (dz, "dz")):
            _chk(t, torch.float32, name, 2)
            if tuple(t.shape) != (n, d):
                raise RuntimeError(f"layer_norm_bwd2: {name} must be [{n}, {d}], got {tuple(t.shape)}")
        if n and (dz.data_ptr() == z.data_ptr() or dn.data_ptr() == z.data_ptr()):
            raise ValueError("layer_norm_bwd2: dz and dn must not alias z (dz may be dn)")
        if dgs is None:
            slabs = torch.empty(ns * stride, dtype=torch.float32, device=z.device)
            dgs, dbs = slabs, slabs[d:]
        else:
            _chk(dgs, torch.float32, "dgamma_slabs", 1)
            _chk(dbs, torch.float32, "dbeta_slabs", 1)
            if stride < 2 * d and ns > 1:
                raise RuntimeError(f"layer_norm_bwd2: slab_stride must be >= 2 * dim = {2 * d}, got {stride}")
            if dgs.numel() < (ns - 1) * stride + d or dbs.numel() < (ns - 1) * stride + d:
                raise RuntimeError("layer_norm_bwd2: dgamma_slabs / dbeta_slabs must reach n_slabs slabs of slab_stride floats")
        arr[i] = _lib.LayerNormBwdArgs(_p(z), _p(gamma), _p(dn), _p(dz), _p(dgs), _p(dbs), n)
        outs.append((dz, dgs, dbs, d))
    _lib.check(_lib.load().tt_layer_norm_bwd_f32(arr, len(problems), dim, float(eps), ns, stride, _stream()), "tt_layer_norm_bwd_f32")
    return tuple((dz, torch.as_strided(dgs, (ns, d), (stride, 1)), torch.as_strided(dbs, (ns, d), (stride, 1)))
                 for dz, dgs, dbs, d in outs)


def adapt_normalization(x):
    """Keras ``Normalization.adapt`` over the rows of ``x`` [rows, F]: mean and variance of every column in f64, ``inv_std`` =
    1 / max(sqrt(var), 1e-7); returns (mean [F], inv_std [F]) as f32 NumPy arrays.  Non-finite input raises."""
    import numpy as np
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.ndim != 2 or a.shape[0] < 1:
        raise ValueError(f"adapt_normalization: x must be [rows >= 1, F], got shape {tuple(a.shape)}")
    a = a.astype(np.float64)
    if not np.isfinite(a).all():
        raise ValueError("adapt_normalization: x holds non-finite values")
    mean = a.mean(axis=0)
    var = ((a - mean) ** 2).mean(axis=0)
    inv_std = 1.0 / np.maximum(np.sqrt(var), 1e-7)
    return mean.astype(np.float32), inv_std.astype(np.float32)


# ----------------------------------------------------------------------------- a3+a4 retrieval
SCORER_PRECISIONS = ("f32", "bf16x3")


def _precision_entry(stem: str, precision: str):
    """(function, its name) of the scorer entry ``stem`` in the given precision."""
    if precision not in SCORER_PRECISIONS:
        raise ValueError(f"precision must be one of {SCORER_PRECISIONS}, got {precision!r}")
    name = f"tt_retrieval_{stem}_f32" if precision == "f32" else f"tt_retrieval_{stem}_bf16x3_f32"
    return getattr(_lib.load(), name), name


def retrieval_workspace_bytes(nq: int, nc: int, dim: int) -> int:
    """Workspace of the fused training entries (retrieval_fwd_bwd): includes the [nq, nc] f32 logit buffer pass 2 reads back."""
    return int(_lib.load().tt_retrieval_workspace_bytes(nq, nc, dim))


def retrieval_fwd_workspace_bytes(nq: int, nc: int, dim: int) -> int:
    """Workspace of the forward-only / separate-backward entries (no logit buffer)."""
    return int(_lib.load().tt_retrieval_fwd_workspace_bytes(nq, nc, dim))


def _chk_retrieval(q, c, sample_weight=None, cand_prob=None, cand_ids=None, hard_thr=None, lse=None, per_row=None,
                   dq=None, dc=None):
    """dtype / device / shape checks shared by the retrieval entry points: the kernels index the optional vectors by
    query (nq) or candidate (nc) without looking at their length."""
    _chk(q, torch.float32, "query_embeddings", 2)
    _chk(c, torch.float32, "candidate_embeddings", 2)
    if q.shape[1] != c.shape[1]:
        raise RuntimeError(f"retrieval: embedding dims differ: {q.shape[1]} vs {c.shape[1]}")
    nq, nc = q.shape[0], c.shape[0]
    for t, dt, name, n in ((sample_weight, torch.float32, "sample_weight", nq), (hard_thr, torch.float32, "hard_thr", nq),
                           (lse, torch.float32, "lse", nq), (per_row, torch.float32, "per_row", nq),
                           (cand_prob, torch.float32, "candidate_sampling_probability", nc),
                           (cand_ids, torch.int64, "candidate_ids", nc)):
        if t is not None:
            _chk(t, dt, name, 1)
            if t.numel() != n:
                raise RuntimeError(f"retrieval: {name} must have {n} entries, got {t.numel()}")
    for t, name, ref in ((dq, "dq", q), (dc, "dc", c)):
        if t is not None:
            _chk(t, torch.float32, name, 2)
            if tuple(t.shape) != tuple(ref.shape):
                raise RuntimeError(f"retrieval: {name} must be {tuple(ref.shape)}, got {tuple(t.shape)}")


def retrieval_rank_workspace_bytes(nq: int, nc: int, dim: int) -> int:
    """Workspace of the metric (rank) pass alone: no gradient slabs (those make the full workspace as large as the
    candidate corpus when nc >= 65536)."""
    return int(_lib.load().tt_retrieval_rank_workspace_bytes(nq, nc, dim))


def retrieval_fwd(q, c, inv_temperature: float, workspace, lse, per_row, loss, sample_weight=None,
                  cand_prob=None, cand_ids=None, diag_offset: int = 0, hard_thr=None, precision: str = "f32"):
    """Forward only (validation loss).  precision "bf16x3": the logits' products on the bf16 MFMA (dim 128 / 256)."""
    _chk_retrieval(q, c, sample_weight, cand_prob, cand_ids, hard_thr, lse, per_row)
    fn, name = _precision_entry("fwd", precision)
    _lib.check(fn(_p(q), _p(c), q.shape[0], c.shape[0], q.shape[1], diag_offset, inv_temperature,
                  _p(sample_weight), _p(cand_prob), _p(cand_ids), _p(hard_thr), _p(workspace),
                  workspace.numel(), _p(lse), _p(per_row), _p(loss), _stream()),
               name)
    return loss


def retrieval_bwd(q, c, inv_temperature: float, workspace, lse, dq, dc, sample_weight=None, cand_prob=None,
                  cand_ids=None, diag_offset: int = 0, grad_scale: float = 1.0, hard_thr=None):
    _chk_retrieval(q, c, sample_weight, cand_prob, cand_ids, hard_thr, lse, None, dq, dc)
    lib = _lib.load()
    _lib.check(lib.tt_retrieval_bwd_f32(_p(q), _p(c), q.shape[0], c.shape[0], q.shape[1], diag_offset, inv_temperature,
                                        _p(sample_weight), _p(cand_prob), _p(cand_ids), _p(hard_thr), _p(lse), grad_scale,
                                        _p(workspace), workspace.numel(), _p(dq), _p(dc), _stream()),
               "tt_retrieval_bwd_f32")
    return dq, dc


def retrieval_fwd_bwd(q, c, inv_temperature: float, workspace, lse, per_row, loss, dq, dc, sample_weight=None,
                      cand_prob=None, cand_ids=None, diag_offset: int = 0, grad_scale: float = 1.0, hard_thr=None,
                      precision: str = "f32"):
    """Loss and both gradients in two fused passes (training form).  precision "f32": exact f32 products on the
    f32-input MFMA; "bf16x3": the f32-emulated split-bf16 form on the bf16 MFMA (dim 128 / 256)."""
    _chk_retrieval(q, c, sample_weight, cand_prob, cand_ids, hard_thr, lse, per_row, dq, dc)
    fn, name = _precision_entry("fwd_bwd", precision)
    _lib.check(fn(_p(q), _p(c), q.shape[0], c.shape[0], q.shape[1], diag_offset, inv_temperature,
                  _p(sample_weight), _p(cand_prob), _p(cand_ids), _p(hard_thr), grad_scale, _p(workspace),
                  workspace.numel(), _p(lse), _p(per_row), _p(loss), _p(dq), _p(dc), _stream()),
               name)
    return loss


PAIRWISE_KINDS = {"logistic": 0, "hinge": 1}          # TT_PAIRWISE_LOGISTIC / TT_PAIRWISE_HINGE
PAIRWISE_REDUCTIONS = {"mean": 0, "sum": 1}           # TT_PAIRWISE_MEAN / TT_PAIRWISE_SUM


def retrieval_pairwise_workspace_bytes(nq: int, nc: int, dim: int) -> int:
    """Workspace of the pairwise-loss entries: row terms, per-split row partials and gradient slabs - no [nq, nc] buffer."""
    return int(_lib.load().tt_retrieval_pairwise_workspace_bytes(nq, nc, dim))


def _pairwise_codes(kind: str, margin: float, reduction: str):
    if kind not in PAIRWISE_KINDS:
        raise ValueError(f"pairwise loss kind must be one of {tuple(PAIRWISE_KINDS)}, got {kind!r}")
    if reduction not in PAIRWISE_REDUCTIONS:
        raise ValueError(f"pairwise loss reduction must be one of {tuple(PAIRWISE_REDUCTIONS)}, got {reduction!r}")
    return PAIRWISE_KINDS[kind], float(margin), PAIRWISE_REDUCTIONS[reduction]


def retrieval_pairwise_fwd(q, c, inv_temperature: float, workspace, per_row, loss, kind: str = "logistic", margin: float = 1.0,
                           reduction: str = "mean", sample_weight=None, cand_prob=None, cand_ids=None, diag_offset: int = 0,
                           hard_thr=None):
    """Forward only (validation) of the pairwise loss ``kind`` ("logistic" = BPR, "hinge") over the in-batch negatives: writes
    per_row [nq] and loss [1].  ``reduction`` "mean": every row's sum is divided by its number of negatives; "sum": it is not."""
    _chk_retrieval(q, c, sample_weight, cand_prob, cand_ids, hard_thr, None, per_row)
    k, m, r = _pairwise_codes(kind, margin, reduction)
    _lib.check(_lib.load().tt_retrieval_pairwise_fwd_f32(
        _p(q), _p(c), q.shape[0], c.shape[0], q.shape[1], diag_offset, inv_temperature, _p(sample_weight), _p(cand_prob),
        _p(cand_ids), _p(hard_thr), _p(workspace), workspace.numel(), _p(per_row), _p(loss), k, m, r, _stream()),
        "tt_retrieval_pairwise_fwd_f32")
    return loss


def retrieval_pairwise_fwd_bwd(q, c, inv_temperature: float, workspace, per_row, loss, dq, dc, kind: str = "logistic",
                               margin: float = 1.0, reduction: str = "mean", sample_weight=None, cand_prob=None, cand_ids=None,
                               diag_offset: int = 0, grad_scale: float = 1.0, hard_thr=None):
    """The pairwise loss and both gradients (training form): two passes over the logits, exact f32 products, no atomics."""
    _chk_retrieval(q, c, sample_weight, cand_prob, cand_ids, hard_thr, None, per_row, dq, dc)
    k, m, r = _pairwise_codes(kind, margin, reduction)
    _lib.check(_lib.load().tt_retrieval_pairwise_fwd_bwd_f32(
        _p(q), _p(c), q.shape[0], c.shape[0], q.shape[1], diag_offset, inv_temperature, _p(sample_weight), _p(cand_prob),
        _p(cand_ids), _p(hard_thr), grad_scale, _p(workspace), workspace.numel(), _p(per_row), _p(loss), _p(dq), _p(dc), k, m, r,
        _stream()), "tt_retrieval_pairwise_fwd_bwd_f32")
    return loss


def retrieval_rank(q, c, inv_temperature: float, pos_index, workspace=None, cand_prob=None, out=None, precision: str = "f32"):
    """rank[i] = #candidates scoring strictly above query i's true candidate ``pos_index[i]`` (int32 [nq]).
    precision "bf16x3": the logits' products on the bf16 MFMA (dim 128 / 256)."""
    fn, name = _precision_entry("rank", precision)
    _chk(q, torch.float32, "query_embeddings", 2)
    _chk(c, torch.float32, "candidate_embeddings", 2)
    _chk(pos_index, torch.int64, "pos_index", 1)
    if cand_prob is not None:
        _chk(cand_prob, torch.float32, "candidate_sampling_probability", 1)
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    if q.shape[1] != c.shape[1]:
        raise RuntimeError(f"retrieval: embedding dims differ: {q.shape[1]} vs {c.shape[1]}")
    if pos_index.numel() != nq or (cand_prob is not None and cand_prob.numel() != nc):
        raise RuntimeError("retrieval_rank: pos_index needs nq entries and candidate_sampling_probability nc")
    if workspace is None:       # the rank pass needs only the bias / threshold / count regions, not the gradient slabs
        workspace = torch.empty(retrieval_rank_workspace_bytes(nq, nc, d), dtype=torch.uint8, device=q.device)
    if out is None:
        out = torch.empty(nq, dtype=torch.int32, device=q.device)
    _lib.check(fn(_p(q), _p(c), nq, nc, d, inv_temperature, _p(cand_prob), _p(pos_index),
                  _p(workspace), workspace.numel(), _p(out), _stream()),
               name)
    return out


TOPK_MAX_K = _lib.TT_TOPK_MAX_K


def _topk_buffers(what: str, need: int, nq: int, k: int, device, workspace, out):
    """(workspace, scores, indices) of a top-k call: allocated where the caller passed none, checked where it did."""
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    else:
        _chk(workspace, torch.uint8, "workspace", 1)
    if out is None:
        out = (torch.empty(nq, k, dtype=torch.float32, device=device), torch.empty(nq, k, dtype=torch.int64, device=device))
    scores, indices = out
    _chk(scores, torch.float32, "out scores", 2)
    _chk(indices, torch.int64, "out indices", 2)
    if tuple(scores.shape) != (nq, k) or tuple(indices.shape) != (nq, k):
        raise ValueError(f"{what}: out tensors must be [{nq}, {k}]")
    return workspace, scores, indices


def retrieval_topk_workspace_bytes(nq: int, nc: int, dim: int, k: int) -> int:
    """Workspace of ``retrieval_topk`` (0 for a shape the call refuses)."""
    return int(_lib.load().tt_retrieval_topk_workspace_bytes(nq, nc, dim, k))


def exclusions_csr(exclusions, nq: int):
    """(offsets int64 [nq + 1], indices int64) with every query's segment sorted ascending, from either a CSR pair
    (offsets[0] == 0, non-decreasing, offsets[nq] <= len(indices)) or a padded [nq, E] int64 tensor (-1 = padding; any
    value outside the corpus matches nothing).  Sorted on the device; (None, None) when there is nothing to exclude."""
    if exclusions is None:
        return None, None
    if isinstance(exclusions, torch.Tensor):
        _chk(exclusions, torch.int64, "exclusions", 2)
        if exclusions.shape[0] != nq:
            raise ValueError(f"exclusions: padded form needs {nq} rows, got shape {tuple(exclusions.shape)}")
        e = exclusions.shape[1]
        if e == 0:
            return None, None
        idx = torch.sort(exclusions, dim=1).values.reshape(-1)
        offsets = torch.arange(0, (nq + 1) * e, e, dtype=torch.int64, device=exclusions.device)
        return offsets, idx
    if not isinstance(exclusions, (tuple, list)) or len(exclusions) != 2:
        raise TypeError("exclusions: expected a padded [nq, E] int64 tensor or a CSR pair (offsets, indices)")
    offsets, idx = exclusions
    _chk(offsets, torch.int64, "exclusion offsets", 1)
    _chk(idx, torch.int64, "exclusion indices", 1)
    if offsets.numel() != nq + 1:
        raise ValueError(f"exclusion offsets: need nq + 1 = {nq + 1} entries, got {offsets.numel()}")
    bad = (offsets[0] != 0) | (offsets[-1] > idx.numel()) | (offsets.diff() < 0).any()
    if bool(bad):
        raise ValueError("exclusion offsets must start at 0, be non-decreasing and end within the index array")
    if idx.numel() == 0:
        return None, None
    # sort within segments: by value, then (stable) by segment
    seg = torch.searchsorted(offsets[1:], torch.arange(idx.numel(), device=idx.device), right=True)
    o1 = torch.argsort(idx, stable=True)
    o2 = torch.argsort(seg[o1], stable=True)
    return offsets.contiguous(), idx[o1][o2].contiguous()


def retrieval_topk(q, c, k: int, exclusions=None, workspace=None, out=None):
    """Exact top-k retrieval (tfrs BruteForce): (scores f32 [nq, k], indices int64 [nq, k]) of the plain dot products
    q @ c.T, score descending, ties by ascending candidate index.  ``exclusions``: a CSR pair (offsets [nq + 1], indices)
    or a padded [nq, E] int64 tensor with -1 padding - excluded candidates never appear; when fewer than k remain the
    tail is (-inf, -1).  ``out``: optional (scores, indices) to write into."""
    _chk(q, torch.float32, "query_embeddings", 2)
    _chk(c, torch.float32, "candidate_embeddings", 2)
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    if q.shape[1] != c.shape[1]:
        raise RuntimeError(f"retrieval_topk: embedding dims differ: {q.shape[1]} vs {c.shape[1]}")
    k = int(k)
    if not 1 <= k <= min(TOPK_MAX_K, nc):
        raise ValueError(f"retrieval_topk: k = {k} must be in [1, min({TOPK_MAX_K}, nc = {nc})]")
    off, idx = exclusions_csr(exclusions, nq)
    workspace, scores, indices = _topk_buffers("retrieval_topk", retrieval_topk_workspace_bytes(nq, nc, d, k), nq, k, q.device,
                                               workspace, out)
    _lib.check(_lib.load().tt_retrieval_topk_f32(_p(q), _p(c), nq, nc, d, k, _p(off), _p(idx), _p(workspace),
                                                 workspace.numel(), _p(scores), _p(indices), _stream()),
               "tt_retrieval_topk_f32")
    return scores, indices


def quantize_rows_i8(x, out=None):
    """Per-row symmetric int8 quantisation (``tt_quantize_rows_i8``): (codes int8 [n, D], scales f32 [n]) with
    scale = max|row| / 127 and code = clamp(rint(x / scale), -127, 127), half to even; a zero row has scale 0 and zero
    codes.  ``out``: optional (codes, scales) to write into."""
    _chk(x, torch.float32, "x", 2)
    n, d = x.shape
    if d not in (32, 64, 128, 256):
        raise ValueError(f"quantize_rows_i8: dim = {d} must be one of 32, 64, 128, 256")
    if n < 1:
        raise ValueError("quantize_rows_i8: x must have at least one row")
    if out is None:
        out = (torch.empty(n, d, dtype=torch.int8, device=x.device), torch.empty(n, dtype=torch.float32, device=x.device))
    codes, scales = out
    _chk(codes, torch.int8, "out codes", 2)
    _chk(scales, torch.float32, "out scales", 1)
    if tuple(codes.shape) != (n, d) or scales.numel() != n:
        raise ValueError(f"quantize_rows_i8: out tensors must be [{n}, {d}] and [{n}]")
    _lib.check(_lib.load().tt_quantize_rows_i8(_p(x), n, d, _p(codes), _p(scales), _stream()), "tt_quantize_rows_i8")
    return codes, scales


def default_k1(k: int, nc: int, rerank: bool = True, factor: int = 4) -> int:
    """Stage-1 candidates of ``retrieval_topk_i8``: min(TOPK_MAX_K, nc, max(factor * k, 32)) with a re-rank, k without."""
    return min(TOPK_MAX_K, nc, max(factor * k, 32)) if rerank else k


def retrieval_topk_i8_workspace_bytes(nq: int, nc: int, dim: int, k: int, k1: int) -> int:
    """Workspace of ``retrieval_topk_i8`` (0 for a shape the call refuses)."""
    return int(_lib.load().tt_retrieval_topk_i8_workspace_bytes(nq, nc, dim, k, k1))


def retrieval_topk_i8(q, codes, scales, k: int, c=None, k1: int | None = None, exclusions=None, workspace=None, out=None):
    """Int8-quantised top-k: the queries are quantised like the corpus (``quantize_rows_i8``), the int8 scan keeps each
    query's ``k1`` best candidates by (int32 dot product * row scale, index ascending), and, with the f32 corpus ``c``,
    those are re-scored exactly (``retrieval_topk``'s score of the pair, bit for bit) and the best k returned.  Without
    ``c`` the stage-1 order is returned (k1 = k) with scores key * query scale.  ``k1`` defaults to
    min(TOPK_MAX_K, nc, max(4 k, 32)) with ``c`` and to k without.  Exclusions, padding and outputs as ``retrieval_topk``."""
    _chk(q, torch.float32, "query_embeddings", 2)
    _chk(codes, torch.int8, "codes", 2)
    _chk(scales, torch.float32, "scales", 1)
    nq, d = q.shape
    nc = codes.shape[0]
    if codes.shape[1] != d:
        raise RuntimeError(f"retrieval_topk_i8: embedding dims differ: q {d}, codes {codes.shape[1]}")
    if scales.numel() != nc:
        raise ValueError(f"retrieval_topk_i8: scales needs {nc} entries (one per code row), got {scales.numel()}")
    if c is not None:
        _chk(c, torch.float32, "candidate_embeddings", 2)
        if tuple(c.shape) != (nc, d):
            raise RuntimeError(f"retrieval_topk_i8: c must be [{nc}, {d}] like codes, got {tuple(c.shape)}")
    k = int(k)
    if not 1 <= k <= min(TOPK_MAX_K, nc):
        raise ValueError(f"retrieval_topk_i8: k = {k} must be in [1, min({TOPK_MAX_K}, nc = {nc})]")
    k1 = default_k1(k, nc, c is not None) if k1 is None else int(k1)
    if not k <= k1 <= min(TOPK_MAX_K, nc):
        raise ValueError(f"retrieval_topk_i8: k1 = {k1} must be in [k = {k}, min({TOPK_MAX_K}, nc = {nc})]")
    if c is None and k1 != k:
        raise ValueError(f"retrieval_topk_i8: without c there is no re-rank: k1 = {k1} must equal k = {k}")
    off, idx = exclusions_csr(exclusions, nq)
    workspace, scores, indices = _topk_buffers("retrieval_topk_i8", retrieval_topk_i8_workspace_bytes(nq, nc, d, k, k1), nq, k,
                                               q.device, workspace, out)
    _lib.check(_lib.load().tt_retrieval_topk_i8_f32(_p(q), _p(codes), _p(scales), _p(c), nq, nc, d, k, k1, _p(off), _p(idx),
                                                    _p(workspace), workspace.numel(), _p(scores), _p(indices), _stream()),
               "tt_retrieval_topk_i8_f32")
    return scores, indices


def mmr_rerank(scores, idx, c, k: int, lam: float, groups=None, max_per_group: int = 0, out=None):
    """MMR diversified re-ranking (``tt_mmr_rerank_f32``) of the pool a top-k call returned: ``scores`` f32 [nq, k1] best
    first and ``idx`` int64 [nq, k1] rows of the f32 corpus ``c`` [nc, D] in original order (-1 = padding).  Greedily picks
    ``k`` <= k1 candidates per query by lam * (min-max normalised score) - (1 - lam) * (largest cosine to an item already
    picked, floored at 0), ties to the earlier candidate; with ``groups`` int32 [nc] and ``max_per_group`` = m > 0 at most m
    picks share a group id (-1: never capped).  Returns (scores f32 [nq, k] - the original scores, in pick order -, indices
    int64 [nq, k]); when the pool runs out the tail is (-inf, -1).  ``lam`` = 1 without a cap keeps the first k valid
    candidates.  One launch, no workspace.  ``out``: optional (scores, indices) to write into."""
    _chk(scores, torch.float32, "scores", 2)
    _chk(idx, torch.int64, "idx", 2)
    _chk(c, torch.float32, "candidate_embeddings", 2)
    nq, k1 = scores.shape
    if tuple(idx.shape) != (nq, k1):
        raise ValueError(f"mmr_rerank: idx must be [{nq}, {k1}] like scores, got {tuple(idx.shape)}")
    nc, d = c.shape
    k, max_per_group, lam = int(k), int(max_per_group), float(lam)
    if not 1 <= k1 <= TOPK_MAX_K:
        raise ValueError(f"mmr_rerank: the pool k1 = {k1} must be in [1, {TOPK_MAX_K}]")
    if not 1 <= k <= k1:
        raise ValueError(f"mmr_rerank: k = {k} must be in [1, k1 = {k1}]")
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"mmr_rerank: lam = {lam} must be in [0, 1]")
    if max_per_group < 0:
        raise ValueError(f"mmr_rerank: max_per_group = {max_per_group} must be >= 0")
    if groups is not None:
        _chk(groups, torch.int32, "groups", 1)
        if groups.numel() != nc:
            raise ValueError(f"mmr_rerank: groups needs {nc} entries (one per corpus row), got {groups.numel()}")
    elif max_per_group > 0:
        raise ValueError(f"mmr_rerank: max_per_group = {max_per_group} needs groups")
    _, out_s, out_i = _topk_buffers("mmr_rerank", 0, nq, k, scores.device, None, out)
    if nq == 0:                                              # (empty tensors have no address to hand over)
        return out_s, out_i
    _lib.check(_lib.load().tt_mmr_rerank_f32(_p(scores), _p(idx), nq, k1, _p(c), nc, d, _p(groups), max_per_group, lam, k,
                                             _p(out_s), _p(out_i), _stream()), "tt_mmr_rerank_f32")
    return out_s, out_i


def check_list_offsets(list_offsets, n: int, what: str) -> None:
    """Raise unless list_offsets starts at 0, is non-decreasing and ends at n (checked on the device)."""
    bad = (list_offsets[0] != 0) | (list_offsets[-1] != n) | (list_offsets.diff() < 0).any()
    if bool(bad):
        raise ValueError(f"{what}: list_offsets must start at 0, be non-decreasing and end at n = {n}")


def ivf_search_workspace_bytes(nq: int, nlist: int, n: int, dim: int, k: int, nprobe: int) -> int:
    """Workspace of ``ivf_search`` (0 for a shape the call refuses)."""
    return int(_lib.load().tt_ivf_search_workspace_bytes(nq, nlist, n, dim, k, nprobe))


def ivf_search(q, centroids, list_offsets, list_vectors, list_ids, k: int, nprobe: int, exclusions=None, workspace=None,
               out=None, check_offsets: bool = True):
    """IVF approximate top-k: ``retrieval_topk`` restricted to the items of the ``nprobe`` inverted lists whose centroids
    score highest for each query.  Index: centroids f32 [nlist, D], list_offsets int64 [nlist + 1], list_vectors f32 [n, D]
    (list l = rows list_offsets[l] .. list_offsets[l + 1]), list_ids int32 [n] (original item id of every row).  Returns
    (scores f32 [nq, k], ORIGINAL item ids int64 [nq, k]), ties by ascending id, tail (-inf, -1) when fewer than k
    candidates remain.  ``exclusions`` hold original ids, in either form ``retrieval_topk`` takes.  ``check_offsets``:
    validate list_offsets on the device (a host synchronisation; an index that validated them once may skip it)."""
    _chk(q, torch.float32, "query_embeddings", 2)
    _chk(centroids, torch.float32, "centroids", 2)
    _chk(list_offsets, torch.int64, "list_offsets", 1)
    _chk(list_vectors, torch.float32, "list_vectors", 2)
    _chk(list_ids, torch.int32, "list_ids", 1)
    nq, d = q.shape
    nlist, n = centroids.shape[0], list_vectors.shape[0]
    if centroids.shape[1] != d or list_vectors.shape[1] != d:
        raise RuntimeError(f"ivf_search: embedding dims differ: q {d}, centroids {centroids.shape[1]}, "
                           f"list_vectors {list_vectors.shape[1]}")
    if list_offsets.numel() != nlist + 1:
        raise ValueError(f"ivf_search: list_offsets needs nlist + 1 = {nlist + 1} entries, got {list_offsets.numel()}")
    if list_ids.numel() != n:
        raise ValueError(f"ivf_search: list_ids needs {n} entries (one per list_vectors row), got {list_ids.numel()}")
    k, nprobe = int(k), int(nprobe)
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"ivf_search: k = {k} must be in [1, {TOPK_MAX_K}]")
    if not 1 <= nprobe <= min(TOPK_MAX_K, nlist):
        raise ValueError(f"ivf_search: nprobe = {nprobe} must be in [1, min({TOPK_MAX_K}, nlist = {nlist})]")
    if check_offsets:
        check_list_offsets(list_offsets, n, "ivf_search")
    off, idx = exclusions_csr(exclusions, nq)
    workspace, scores, indices = _topk_buffers("ivf_search", ivf_search_workspace_bytes(nq, nlist, n, d, k, nprobe), nq, k, q.device,
                                               workspace, out)
    _lib.check(_lib.load().tt_ivf_search_f32(_p(q), nq, _p(centroids), nlist, _p(list_offsets), _p(list_vectors), _p(list_ids),
                                             n, d, k, nprobe, _p(off), _p(idx), _p(workspace), workspace.numel(), _p(scores),
                                             _p(indices), _stream()),
               "tt_ivf_search_f32")
    return scores, indices


def ivf_search_i8_workspace_bytes(nq: int, nlist: int, n: int, dim: int, k: int, k1: int, nprobe: int) -> int:
    """Workspace of ``ivf_search_i8`` (0 for a shape the call refuses)."""
    return int(_lib.load().tt_ivf_search_i8_workspace_bytes(nq, nlist, n, dim, k, k1, nprobe))


def ivf_search_i8(q, centroids, list_offsets, list_codes, list_scales, list_ids, k: int, nprobe: int, c=None,
                  k1: int | None = None, exclusions=None, workspace=None, out=None, check_offsets: bool = True):
    """Int8 IVF top-k: ``retrieval_topk_i8`` restricted to the rows of the ``nprobe`` inverted lists ``ivf_search`` probes.
    Index: centroids f32 [nlist, D], list_offsets int64 [nlist + 1] and list_ids int32 [n] as ``ivf_search``; list_codes int8
    [n, D] and list_scales f32 [n], the ``quantize_rows_i8`` output of the items in list order.  ``c``: the f32 corpus [n, D]
    in ORIGINAL id order - the ``k1`` stage-1 candidates (by int32 dot product * row scale, original id ascending) are then
    re-scored exactly (``retrieval_topk``'s score of the pair, bit for bit) and the best k returned; without ``c`` the
    stage-1 order is returned (k1 = k) with scores key * query scale.  ``k1`` defaults to ``default_k1(k, n, c is not
    None)``.  Returns (scores f32 [nq, k], ORIGINAL item ids int64 [nq, k]), tail (-inf, -1) when fewer than k candidates
    remain.  Exclusions (original ids), outputs and ``check_offsets`` as ``ivf_search``."""
    _chk(q, torch.float32, "query_embeddings", 2)
    _chk(centroids, torch.float32, "centroids", 2)
    _chk(list_offsets, torch.int64, "list_offsets", 1)
    _chk(list_codes, torch.int8, "list_codes", 2)
    _chk(list_scales, torch.float32, "list_scales", 1)
    _chk(list_ids, torch.int32, "list_ids", 1)
    nq, d = q.shape
    nlist, n = centroids.shape[0], list_codes.shape[0]
    if centroids.shape[1] != d or list_codes.shape[1] != d:
        raise RuntimeError(f"ivf_search_i8: embedding dims differ: q {d}, centroids {centroids.shape[1]}, "
                           f"list_codes {list_codes.shape[1]}")
    if list_offsets.numel() != nlist + 1:
        raise ValueError(f"ivf_search_i8: list_offsets needs nlist + 1 = {nlist + 1} entries, got {list_offsets.numel()}")
    if list_ids.numel() != n or list_scales.numel() != n:
        raise ValueError(f"ivf_search_i8: list_ids and list_scales need {n} entries (one per list_codes row), got "
                         f"{list_ids.numel()} and {list_scales.numel()}")
    if c is not None:
        _chk(c, torch.float32, "candidate_embeddings", 2)
        if tuple(c.shape) != (n, d):
            raise RuntimeError(f"ivf_search_i8: c must be [{n}, {d}] like list_codes, got {tuple(c.shape)}")
    k, nprobe = int(k), int(nprobe)
    if not 1 <= k <= min(TOPK_MAX_K, n):
        raise ValueError(f"ivf_search_i8: k = {k} must be in [1, min({TOPK_MAX_K}, n = {n})]")
    k1 = default_k1(k, n, c is not None) if k1 is None else int(k1)
    if not k <= k1 <= min(TOPK_MAX_K, n):
        raise ValueError(f"ivf_search_i8: k1 = {k1} must be in [k = {k}, min({TOPK_MAX_K}, n = {n})]")
    if c is None and k1 != k:
        raise ValueError(f"ivf_search_i8: without c there is no re-rank: k1 = {k1} must equal k = {k}")
    if not 1 <= nprobe <= min(TOPK_MAX_K, nlist):
        raise ValueError(f"ivf_search_i8: nprobe = {nprobe} must be in [1, min({TOPK_MAX_K}, nlist = {nlist})]")
    if check_offsets:
        check_list_offsets(list_offsets, n, "ivf_search_i8")
    off, idx = exclusions_csr(exclusions, nq)
    workspace, scores, indices = _topk_buffers("ivf_search_i8", ivf_search_i8_workspace_bytes(nq, nlist, n, d, k, k1, nprobe), nq,
                                               k, q.device, workspace, out)
    _lib.check(_lib.load().tt_ivf_search_i8_f32(_p(q), nq, _p(centroids), nlist, _p(list_offsets), _p(list_codes),
                                                _p(list_scales), _p(list_ids), _p(c), n, d, k, k1, nprobe, _p(off), _p(idx),
                                                _p(workspace), workspace.numel(), _p(scores), _p(indices), _stream()),
               "tt_ivf_search_i8_f32")
    return scores, indices


def retrieval_batch_rank(q, c, inv_temperature: float, cand_prob=None, cand_ids=None, diag_offset: int = 0, workspace=None, out=None):
    """In-batch rank of every query's positive (candidate i + diag_offset) under the scores the loss sees - temperature,
    sampling-probability correction, accidental hits removed (int32 [nq]); top-k accuracy = mean(rank < k)."""
    _chk_retrieval(q, c, None, cand_prob, cand_ids)
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    if workspace is None:
        workspace = torch.empty(retrieval_rank_workspace_bytes(nq, nc, d), dtype=torch.uint8, device=q.device)
    if out is None:
        out = torch.empty(nq, dtype=torch.int32, device=q.device)
    lib = _lib.load()
    _lib.check(lib.tt_retrieval_batch_rank_f32(_p(q), _p(c), nq, nc, d, diag_offset, inv_temperature, _p(cand_prob), _p(cand_ids),
                                               _p(workspace), workspace.numel(), _p(out), _stream()), "tt_retrieval_batch_rank_f32")
    return out


def retrieval_hard_negative_thresholds(q, c, inv_temperature: float, k: int, workspace, cand_prob=None, cand_ids=None,
                                       diag_offset: int = 0, scratch=None, out=None):
    """Per-query thresholds for ``num_hard_negatives = k`` (pass as ``hard_thr`` to the loss entry points)."""
    _chk(q, torch.float32, "query_embeddings", 2)
    _chk(c, torch.float32, "candidate_embeddings", 2)
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    if scratch is None:
        scratch = torch.empty(nq * nc, dtype=torch.float32, device=q.device)
    if out is None:
        out = torch.empty(nq, dtype=torch.float32, device=q.device)
    lib = _lib.load()
    _lib.check(lib.tt_retrieval_hard_negative_thresholds_f32(_p(q), _p(c), nq, nc, d, diag_offset, inv_temperature,
                                                             _p(cand_prob), _p(cand_ids), k, _p(workspace), workspace.numel(),
                                                             _p(scratch), scratch.numel() * 4, _p(out), _stream()),
               "tt_retrieval_hard_negative_thresholds_f32")
    return out
