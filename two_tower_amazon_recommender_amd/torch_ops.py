"""``torch.ops.twotower.*`` — the hot-path kernels registered as PyTorch custom ops (``torch.library``), as
``north_star`` asks ("exposed to Python through PyTorch-ROCm custom ops that keep the repo's
tfrs.tasks.Retrieval-style call signature") and SURVEY.md §8(b) row 3 specifies.  Each op is a thin, typed front
over the same C ABI (``include/twotower_hip.h``, reached through ``ops``): schema + fake (meta) implementation +
autograd formula, so the ops compose with ``torch.autograd``, ``torch.compile`` tracing and ``opcheck``.  There
is no CPU implementation: the ops are registered for ``device_types="cuda"`` only and a CPU tensor raises.

    loss, per_example, dq, dc = torch.ops.twotower.retrieval_loss(q, c, w, p, ids, inv_t, diag_offset, k)
    rows = torch.ops.twotower.embedding_gather(table, ids)
    pooled = torch.ops.twotower.embedding_bag(table, tokens, bag_rows, "mean")
    x = torch.ops.twotower.history_bag(hist_table, histories, user_ids, item_ids, user_table, user_ids, "mean")
    x, w, pooled, slot_ids = torch.ops.twotower.history_attention(hist_table, histories, user_ids, item_ids, user_table, user_ids,
                                                                  attn)        # autograd w.r.t. attn = [query | recency bias]
    x = x + torch.ops.twotower.dense_features(feat, ids, mean, inv_std, proj, clip)   # autograd w.r.t. proj
    x = x + torch.ops.twotower.time_context(timestamps, time_table, "hour,day_of_week", 0, t_min, t_max)   # autograd w.r.t. time_table
    y    = torch.ops.twotower.dense_fwd(x, w, b, relu)                  # autograd through twotower::dense_bwd
    torch.ops.twotower.sparse_update_(table, accum, grads, ids, "adagrad", lr, eps)
    torch.ops.twotower.sparse_adam_(table, exp_avg, exp_avg_sq, grads, ids, step, lr, 0.9, 0.999, 1e-7)
    torch.ops.twotower.sparse_rowwise_adagrad_(table, row_accum, grads, ids, lr, eps)   # row_accum: [rows], one float per row

What the reference would have run through TensorFlow / TFRS for these (``/root/reference/pyproject.toml:22,24``;
settings ``configs/data_config.yaml:54-71``; the task object's call signature: SURVEY.md Appendix A).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import ops

NS = "twotower"


_WS_CACHE: dict = {}
_PLAN_CACHE: dict = {}


def _ws(nq: int, nc: int, d: int, device, forward_only: bool = False) -> Tensor:
    """Scorer workspace; the training entry's includes the [nq, nc] f32 dot-product buffer its second pass reads back
    (4*nq*nc bytes: 268 MB at 8192 x 8192, 4.3 GB at 32768 x 32768).  Kept per (kind, device, stream) instead of being
    allocated on every call: the kernels of one stream run in order, so successive calls can share it.  The LARGEST buffer seen
    is kept (a loop alternating two batch shapes re-allocated 268 MB per call when only the last shape was held: VERDICT r03);
    ``release_workspaces()`` drops them.  Nothing is cached while the stream is being captured into a HIP graph: a buffer
    allocated there lives in the graph's private pool and must not be handed to eager calls afterwards."""
    n = ops.retrieval_fwd_workspace_bytes(nq, nc, d) if forward_only else ops.retrieval_workspace_bytes(nq, nc, d)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n, dtype=torch.uint8, device=device)
    key = (bool(forward_only), str(device), torch.cuda.current_stream(device).cuda_stream)
    hit = _WS_CACHE.get(key)
    if hit is not None and hit.numel() >= n:
        return hit
    _WS_CACHE.pop(key, None)                 # (freed before the larger one is allocated)
    buf = torch.empty(n, dtype=torch.uint8, device=device)
    _WS_CACHE[key] = buf
    return buf


def _plan(n: int, device) -> "ops.SparsePlan":
    """One SparsePlan (sorted ids, positions, piece workspace) per (length, device, stream) for ``sparse_update_``."""
    if torch.cuda.is_current_stream_capturing():
        return ops.SparsePlan(n, device)
    key = (int(n), str(device), torch.cuda.current_stream(device).cuda_stream)
    hit = _PLAN_CACHE.get(key)
    if hit is None:
        hit = _PLAN_CACHE[key] = ops.SparsePlan(n, device)
    return hit


def release_workspaces() -> None:
    """Drop every cached scorer workspace and sort plan of the custom ops (they are re-allocated on the next call)."""
    _WS_CACHE.clear()
    _PLAN_CACHE.clear()
    _TOPK_WS.clear()
    _PW_WS.clear()


# --------------------------------------------------------------------------------------------- a1 lookup
@torch.library.custom_op(f"{NS}::embedding_gather", mutates_args=(), device_types="cuda")
def embedding_gather(table: Tensor, ids: Tensor) -> Tensor:
    """rows[b, :] = table[ids[b], :] (ids outside the table give a zero row, like the C entry point; use the trainer's
    flag for TF's raise).  Not differentiable: the table is trained by ``sparse_update_`` on the row gradients."""
    return ops.embedding_gather(table.contiguous(), ids.contiguous())


@embedding_gather.register_fake
def _(table, ids):
    return table.new_empty((ids.shape[0], table.shape[1]))


@torch.library.custom_op(f"{NS}::embedding_bag", mutates_args=(), device_types="cuda")
def embedding_bag(table: Tensor, tokens: Tensor, bag_rows: Optional[Tensor], pooling: str = "mean") -> Tensor:
    """pooled[b, :] = pool of the rows table[t, :] over the valid tokens t of row bag_rows[b] (None: row b) of ``tokens``
    [rows, L] int32 (-1 = padding; ``ops.embedding_bag``); ``pooling`` "sum", "mean" or "sqrtn"; an empty bag gives a zero
    row.  Not differentiable: the table is trained through ``ops.BagPlan`` and the sparse updates on the bags' gradient rows."""
    return ops.embedding_bag(table.contiguous(), tokens.contiguous(), None if bag_rows is None else bag_rows.contiguous(), pooling)


@embedding_bag.register_fake
def _(table, tokens, bag_rows, pooling="mean"):
    return table.new_empty(((tokens.shape[0] if bag_rows is None else bag_rows.shape[0]), table.shape[1]))


@torch.library.custom_op(f"{NS}::history_bag", mutates_args=(), device_types="cuda")
def history_bag(table: Tensor, tokens: Tensor, bag_rows: Optional[Tensor], exclude: Optional[Tensor], base_table: Optional[Tensor],
                base_ids: Optional[Tensor], pooling: str = "mean") -> Tensor:
    """``embedding_bag`` with leave-one-out and a base row in one launch (``ops.history_bag``, the pooled user-history feature):
    bag b skips every slot whose token equals ``exclude[b]``, and out[b] = base_table[base_ids[b]] + pooled when the base pair
    is given (both or neither).  Not differentiable: the table is trained through ``ops.BagPlan`` and the sparse updates."""
    if (base_table is None) != (base_ids is None):
        raise ValueError("history_bag: base_table and base_ids go together")
    c = lambda t: None if t is None else t.contiguous()
    return ops.history_bag(table.contiguous(), tokens.contiguous(), c(bag_rows), c(exclude),
                           None if base_table is None else (c(base_table), c(base_ids)), pooling)


@history_bag.register_fake
def _(table, tokens, bag_rows, exclude, base_table, base_ids, pooling="mean"):
    return table.new_empty(((tokens.shape[0] if bag_rows is None else bag_rows.shape[0]), table.shape[1]))


@torch.library.custom_op(f"{NS}::history_attention", mutates_args=(), device_types="cuda")
def history_attention(table: Tensor, tokens: Tensor, bag_rows: Optional[Tensor], exclude: Optional[Tensor],
                      base_table: Optional[Tensor], base_ids: Optional[Tensor], attn: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The history bag pooled by a learned query with a recency bias (``ops.history_attention``; ``attn`` [dim + L] = [a | p]):
    (out [n_bags, dim] = base row + sum_j w_j table[t_j], weights [n_bags, L], pooled [n_bags, dim], batch_ids [n_bags * L]
    int64 - the slots' tokens, -1 where skipped).  Autograd with respect to ``attn`` only (from the gradients of ``out`` and
    ``pooled``), through ``twotower::history_attention_bwd``.  The table's gradient is sparse - one row per kept slot, the first
    result of ``history_attention_bwd`` - and goes through ``sparse_update_`` / ``sparse_adam_`` with ``batch_ids`` as the ids;
    the base table's gradient rows are the gradient of ``out`` itself."""
    if (base_table is None) != (base_ids is None):
        raise ValueError("history_attention: base_table and base_ids go together")
    c = lambda t: None if t is None else t.contiguous()
    n_bags = tokens.shape[0] if bag_rows is None else bag_rows.shape[0]
    ids = torch.empty(n_bags * tokens.shape[1], dtype=torch.int64, device=table.device)
    out, weights, pooled = ops.history_attention(table.contiguous(), tokens.contiguous(), attn.contiguous(), c(bag_rows), c(exclude),
                                                 None if base_table is None else (c(base_table), c(base_ids)), batch_ids=ids)
    return out, weights, pooled, ids


@history_attention.register_fake
def _(table, tokens, bag_rows, exclude, base_table, base_ids, attn):
    n_bags, L = (tokens.shape[0] if bag_rows is None else bag_rows.shape[0]), tokens.shape[1]
    return (table.new_empty((n_bags, table.shape[1])), table.new_empty((n_bags, L)), table.new_empty((n_bags, table.shape[1])),
            tokens.new_empty((n_bags * L,), dtype=torch.int64))


@torch.library.custom_op(f"{NS}::history_attention_bwd", mutates_args=(), device_types="cuda")
def history_attention_bwd(table: Tensor, batch_ids: Tensor, weights: Tensor, pooled: Tensor, dy: Tensor,
                          attn: Tensor) -> Tuple[Tensor, Tensor]:
    """(slot_grads [n_bags * L, dim], dattn [dim + L]) of ``history_attention`` given dL/dout and what the forward returned: one
    gradient row per kept slot (a skipped slot's row is zero here) for ``sparse_update_`` / ``sparse_adam_`` with ``batch_ids``
    as the ids, and the gradient of ``attn``, the backward launch's slabs summed."""
    n_bags, L = weights.shape
    slot_grads = torch.zeros((n_bags * L, table.shape[1]), dtype=torch.float32, device=table.device)
    _, slabs = ops.history_attention_bwd(table.contiguous(), batch_ids.contiguous(), weights.contiguous(), pooled.contiguous(),
                                         dy.contiguous(), attn.contiguous(), L, slot_grads=slot_grads)
    return slot_grads, slabs.sum(dim=0)


@history_attention_bwd.register_fake
def _(table, batch_ids, weights, pooled, dy, attn):
    return table.new_empty((weights.shape[0] * weights.shape[1], table.shape[1])), torch.empty_like(attn, memory_format=torch.contiguous_format)


def _attention_setup(ctx, inputs, output):
    table, attn = inputs[0], inputs[6]
    _, weights, pooled, batch_ids = output
    ctx.save_for_backward(table, batch_ids, weights, pooled, attn)


def _attention_backward(ctx, d_out, d_weights, d_pooled, d_ids):
    table, batch_ids, weights, pooled, attn = ctx.saved_tensors
    dy = d_out if d_pooled is None else (d_pooled if d_out is None else d_out + d_pooled)
    dattn = None
    if ctx.needs_input_grad[6] and dy is not None:
        dattn = torch.ops.twotower.history_attention_bwd(table, batch_ids, weights, pooled, dy, attn)[1]
    return None, None, None, None, None, None, dattn


history_attention.register_autograd(_attention_backward, setup_context=_attention_setup)


@torch.library.custom_op(f"{NS}::history_gru", mutates_args=(), device_types="cuda")
def history_gru(table: Tensor, tokens: Tensor, bag_rows: Optional[Tensor], exclude: Optional[Tensor], base_table: Optional[Tensor],
                base_ids: Optional[Tensor], W: Tensor, U: Tensor, b: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The history bag encoded by a GRU (``ops.history_gru``; ``W``, ``U`` [dim, 3 dim] with the gate blocks z | r | n, ``b``
    [2, 3 dim] = b_i, b_r): (out [n_bags, dim] = base row + h_final, batch_ids [n_bags * L] int64 - the slots' tokens, -1 where
    skipped -, and the kept buffers x [n_bags * L, dim], gates [n_bags * L, 3 dim], gn and hprev [n_bags * L, dim]).  Autograd
    with respect to ``W``, ``U`` and ``b`` (from the gradient of ``out``), through ``twotower::history_gru_bwd``.  The table's
    gradient is sparse - one row per slot, the first result of ``history_gru_bwd`` - and goes through ``sparse_update_`` /
    ``sparse_adam_`` with ``batch_ids`` as the ids; the base table's gradient rows are the gradient of ``out`` itself."""
    if (base_table is None) != (base_ids is None):
        raise ValueError("history_gru: base_table and base_ids go together")
    c = lambda t: None if t is None else t.contiguous()
    out, bufs = ops.history_gru(table.contiguous(), tokens.contiguous(), W.contiguous(), U.contiguous(), b.contiguous(), c(bag_rows),
                                c(exclude), None if base_table is None else (c(base_table), c(base_ids)), keep=True)
    return out, bufs.batch_ids, bufs.x, bufs.gates, bufs.gn, bufs.hprev


@history_gru.register_fake
def _(table, tokens, bag_rows, exclude, base_table, base_ids, W, U, b):
    n_bags, L, d = (tokens.shape[0] if bag_rows is None else bag_rows.shape[0]), tokens.shape[1], table.shape[1]
    return (table.new_empty((n_bags, d)), tokens.new_empty((n_bags * L,), dtype=torch.int64), table.new_empty((n_bags * L, d)),
            table.new_empty((n_bags * L, 3 * d)), table.new_empty((n_bags * L, d)), table.new_empty((n_bags * L, d)))


@torch.library.custom_op(f"{NS}::history_gru_bwd", mutates_args=(), device_types="cuda")
def history_gru_bwd(batch_ids: Tensor, x: Tensor, gates: Tensor, gn: Tensor, hprev: Tensor, dy: Tensor, W: Tensor,
                    U: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(slot_grads [n_bags * L, dim], dW [dim, 3 dim], dU [dim, 3 dim], db [2, 3 dim]) of ``history_gru`` given dL/dout and what
    the forward returned: one gradient row per slot (zeros for a skipped one) for ``sparse_update_`` / ``sparse_adam_`` with
    ``batch_ids`` as the ids, and the parameters' gradients, the backward launches' slabs summed."""
    L = x.shape[0] // dy.shape[0] if dy.shape[0] else 1
    bufs = ops.GruBuffers.wrap(L, batch_ids.contiguous(), x.contiguous(), gates.contiguous(), gn.contiguous(), hprev.contiguous())
    slot_grads, dw, du, db = ops.history_gru_bwd(bufs, dy.contiguous(), W.contiguous(), U.contiguous())
    return slot_grads, dw.sum(dim=0), du.sum(dim=0), db.sum(dim=1)


@history_gru_bwd.register_fake
def _(batch_ids, x, gates, gn, hprev, dy, W, U):
    return (x.new_empty(x.shape), torch.empty_like(W, memory_format=torch.contiguous_format),
            torch.empty_like(U, memory_format=torch.contiguous_format), W.new_empty((2, W.shape[1])))


def _gru_setup(ctx, inputs, output):
    W, U = inputs[6], inputs[7]
    _, batch_ids, x, gates, gn, hprev = output
    ctx.save_for_backward(batch_ids, x, gates, gn, hprev, W, U)


def _gru_backward(ctx, d_out, d_ids, d_x, d_gates, d_gn, d_hprev):
    batch_ids, x, gates, gn, hprev, W, U = ctx.saved_tensors
    dW = dU = db = None
    if d_out is not None and any(ctx.needs_input_grad[6:9]):
        _, dW, dU, db = torch.ops.twotower.history_gru_bwd(batch_ids, x, gates, gn, hprev, d_out, W, U)
    pick = lambda g, i: g if ctx.needs_input_grad[i] else None
    return None, None, None, None, None, None, pick(dW, 6), pick(dU, 7), pick(db, 8)


history_gru.register_autograd(_gru_backward, setup_context=_gru_setup)


@torch.library.custom_op(f"{NS}::history_self_attention", mutates_args=(), device_types="cuda")
def history_self_attention(table: Tensor, tokens: Tensor, bag_rows: Optional[Tensor], exclude: Optional[Tensor],
                           base_table: Optional[Tensor], base_ids: Optional[Tensor], Wqk: Tensor, Wvo: Tensor,
                           p: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The history bag encoded by multi-head self-attention read at the newest kept item (``ops.history_self_attention``;
    ``Wqk`` [dim, H dim], ``Wvo`` [H dim, dim], ``p`` [H, L]): (out [n_bags, dim] = base row + concat_h(P_h) Wvo, batch_ids
    [n_bags * L] int64 - the slots' tokens, -1 where skipped -, and the kept buffers newest [n_bags] int32, xn [n_bags, dim], T and P
    [n_bags, H dim], weights [n_bags, H, L]).  Autograd with respect to ``Wqk``, ``Wvo`` and ``p`` (from the gradient of ``out``),
    through ``twotower::history_self_attention_bwd``.  The table's gradient is sparse - one row per kept slot, the first result of
    ``history_self_attention_bwd`` - and goes through ``sparse_update_`` / ``sparse_adam_`` with ``batch_ids`` as the ids; the
    base table's gradient rows are the gradient of ``out`` itself."""
    if (base_table is None) != (base_ids is None):
        raise ValueError("history_self_attention: base_table and base_ids go together")
    c = lambda t: None if t is None else t.contiguous()
    out, bufs = ops.history_self_attention(table.contiguous(), tokens.contiguous(), Wqk.contiguous(), Wvo.contiguous(), p.contiguous(),
                                           c(bag_rows), c(exclude), None if base_table is None else (c(base_table), c(base_ids)),
                                           keep=True)
    return out, bufs.batch_ids, bufs.newest, bufs.xn, bufs.T, bufs.P, bufs.weights


@history_self_attention.register_fake
def _(table, tokens, bag_rows, exclude, base_table, base_ids, Wqk, Wvo, p):
    n_bags, L, d = (tokens.shape[0] if bag_rows is None else bag_rows.shape[0]), tokens.shape[1], table.shape[1]
    hd = Wqk.shape[1]
    return (table.new_empty((n_bags, d)), tokens.new_empty((n_bags * L,), dtype=torch.int64),
            tokens.new_empty((n_bags,), dtype=torch.int32), table.new_empty((n_bags, d)), table.new_empty((n_bags, hd)),
            table.new_empty((n_bags, hd)), table.new_empty((n_bags, p.shape[0], L)))


@torch.library.custom_op(f"{NS}::history_self_attention_bwd", mutates_args=(), device_types="cuda")
def history_self_attention_bwd(table: Tensor, batch_ids: Tensor, newest: Tensor, xn: Tensor, T: Tensor, P: Tensor, weights: Tensor,
                               dy: Tensor, Wqk: Tensor, Wvo: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(slot_grads [n_bags * L, dim], dWqk [dim, H dim], dWvo [H dim, dim], dp [H, L]) of ``history_self_attention`` given dL/dout
    and what the forward returned: one gradient row per kept slot (zeros for a skipped one) for ``sparse_update_`` /
    ``sparse_adam_`` with ``batch_ids`` as the ids, and the parameters' gradients, the backward launches' slabs summed."""
    c = lambda t: t.contiguous()
    bufs = ops.SelfAttnBuffers.wrap(c(table), c(batch_ids), c(newest), c(xn), c(T), c(P), c(weights))
    slot_grads = torch.zeros((bufs.n_bags * bufs.L, bufs.dim), dtype=torch.float32, device=dy.device)
    _, dwqk, dwvo, dp = ops.history_self_attention_bwd(bufs, c(dy), c(Wqk), c(Wvo), slot_grads=slot_grads)
    return slot_grads, dwqk.sum(dim=0), dwvo.sum(dim=0), dp.sum(dim=0).view(bufs.heads, bufs.L)


@history_self_attention_bwd.register_fake
def _(table, batch_ids, newest, xn, T, P, weights, dy, Wqk, Wvo):
    return (xn.new_empty((batch_ids.shape[0], xn.shape[1])), torch.empty_like(Wqk, memory_format=torch.contiguous_format),
            torch.empty_like(Wvo, memory_format=torch.contiguous_format), xn.new_empty((weights.shape[1], weights.shape[2])))


def _self_attention_setup(ctx, inputs, output):
    table, Wqk, Wvo = inputs[0], inputs[6], inputs[7]
    _, batch_ids, newest, xn, T, P, weights = output
    ctx.save_for_backward(table, batch_ids, newest, xn, T, P, weights, Wqk, Wvo)


def _self_attention_backward(ctx, d_out, d_ids, d_newest, d_xn, d_T, d_P, d_weights):
    table, batch_ids, newest, xn, T, P, weights, Wqk, Wvo = ctx.saved_tensors
    dWqk = dWvo = dp = None
    if d_out is not None and any(ctx.needs_input_grad[6:9]):
        _, dWqk, dWvo, dp = torch.ops.twotower.history_self_attention_bwd(table, batch_ids, newest, xn, T, P, weights, d_out, Wqk, Wvo)
    pick = lambda g, i: g if ctx.needs_input_grad[i] else None
    return None, None, None, None, None, None, pick(dWqk, 6), pick(dWvo, 7), pick(dp, 8)


history_self_attention.register_autograd(_self_attention_backward, setup_context=_self_attention_setup)


@torch.library.custom_op(f"{NS}::sample_candidates", mutates_args=(), device_types="cuda")
def sample_candidates(pos_ids: Tensor, n_items: int, n_neg: int, seed: int, tensor_id: int, start: int,
                      alias_thr: Optional[Tensor], alias_idx: Optional[Tensor], item_freq: Optional[Tensor],
                      sampler_prob: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """Mixed negative sampling (``ops.sample_candidates``): (candidate_ids [B + n_neg] = ``pos_ids`` followed by draws
    start .. start + n_neg - 1 of the stream (seed, tensor_id), candidate_sampling_probability).  The alias sampler is used
    when ``alias_thr`` / ``alias_idx`` are given, the uniform one otherwise; without ``item_freq`` the second result is empty.
    Both results go to ``retrieval_loss`` as ``candidate_ids`` / ``candidate_sampling_probability``."""
    if (alias_thr is None) != (alias_idx is None):
        raise ValueError("sample_candidates: alias_thr and alias_idx go together")
    n = pos_ids.numel() + n_neg
    ids = torch.empty(n, dtype=torch.int64, device=pos_ids.device)
    prob = torch.empty(n if item_freq is not None else 0, dtype=torch.float32, device=pos_ids.device)
    alias = None if alias_thr is None else (alias_thr.contiguous(), alias_idx.contiguous())
    ops.sample_candidates(pos_ids.contiguous(), n_items, n_neg, ids, prob if item_freq is not None else None,
                          sampler="uniform" if alias is None else "alias", alias=alias,
                          item_freq=None if item_freq is None else item_freq.contiguous(),
                          sampler_prob=None if sampler_prob is None else sampler_prob.contiguous(),
                          seed=seed, tensor_id=tensor_id, start=start)
    return ids, prob


@sample_candidates.register_fake
def _(pos_ids, n_items, n_neg, seed, tensor_id, start, alias_thr, alias_idx, item_freq, sampler_prob):
    n = pos_ids.shape[0] + n_neg
    return pos_ids.new_empty((n,)), pos_ids.new_empty((n if item_freq is not None else 0,), dtype=torch.float32)


# --------------------------------------------------------------------------------------------- a3 + a4
@torch.library.custom_op(f"{NS}::retrieval_loss", mutates_args=(), device_types="cuda")
def retrieval_loss(query_embeddings: Tensor, candidate_embeddings: Tensor, sample_weight: Optional[Tensor],
                   candidate_sampling_probability: Optional[Tensor], candidate_ids: Optional[Tensor],
                   inv_temperature: float, diag_offset: int, num_hard_negatives: int,
                   precision: str = "f32") -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """In-batch sampled-softmax loss (SUM) of tfrs.tasks.Retrieval AND its gradients, in the fused two-pass form
    (exact f32: 6*Bq*Bc*D executed FLOPs - pass 2 reads the raw dot products of pass 1 back from the workspace;
    bf16x3: both passes compute them).  Returns (loss [], per-example loss [Bq], dLoss/dq, dLoss/dc);
    the autograd formula multiplies the saved gradients by the incoming scalar gradient.  ``candidate_ids`` given =
    accidental-hit removal; ``num_hard_negatives`` > 0 keeps the positive and the k hardest negatives per query;
    ``precision`` "f32" (exact f32 products) or "bf16x3" (f32-emulated split-bf16 products, dim 128 / 256)."""
    q, c = query_embeddings.contiguous(), candidate_embeddings.contiguous()
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    ws = _ws(nq, nc, d, q.device)
    lse, per_row = q.new_empty(nq), q.new_empty(nq)
    loss = q.new_empty(1)
    dq, dc = torch.empty_like(q), torch.empty_like(c)
    thr = None
    if num_hard_negatives > 0:
        thr = ops.retrieval_hard_negative_thresholds(q, c, inv_temperature, num_hard_negatives, ws,
                                                     cand_prob=candidate_sampling_probability, cand_ids=candidate_ids,
                                                     diag_offset=diag_offset)
    ops.retrieval_fwd_bwd(q, c, inv_temperature, ws, lse, per_row, loss, dq, dc, sample_weight=sample_weight,
                          cand_prob=candidate_sampling_probability, cand_ids=candidate_ids, diag_offset=diag_offset,
                          hard_thr=thr, precision=precision)
    return loss.reshape(()), per_row, dq, dc


@retrieval_loss.register_fake
def _(q, c, sample_weight, candidate_sampling_probability, candidate_ids, inv_temperature, diag_offset, num_hard_negatives,
      precision="f32"):
    return q.new_empty(()), q.new_empty((q.shape[0],)), torch.empty_like(q), torch.empty_like(c)


def _retrieval_setup(ctx, inputs, output):
    _, per_example, dq, dc = output
    # only the scalar loss carries a gradient: the per-example losses and the two gradient tensors are results, not
    # differentiable functions here (a loss built from per_example would otherwise train on silent zeros)
    ctx.mark_non_differentiable(per_example, dq, dc)
    ctx.save_for_backward(dq, dc)


def _retrieval_backward(ctx, g_loss, g_per_example, g_dq, g_dc):
    dq, dc = ctx.saved_tensors
    # the upstream gradient of the scalar loss stays on the device (no host sync)
    sdq, sdc = torch._foreach_mul((dq, dc), g_loss)            # (one launch for both)
    return sdq, sdc, None, None, None, None, None, None, None


retrieval_loss.register_autograd(_retrieval_backward, setup_context=_retrieval_setup)


@torch.library.custom_op(f"{NS}::retrieval_loss_value", mutates_args=(), device_types="cuda")
def retrieval_loss_value(query_embeddings: Tensor, candidate_embeddings: Tensor, sample_weight: Optional[Tensor],
                         candidate_sampling_probability: Optional[Tensor], candidate_ids: Optional[Tensor],
                         inv_temperature: float, diag_offset: int, num_hard_negatives: int,
                         precision: str = "f32") -> Tuple[Tensor, Tensor]:
    """Forward only (validation): (loss [], per-example loss [Bq]) in one statistics pass; ``precision`` as in
    ``retrieval_loss`` (a task that trains in bf16x3 validates in bf16x3)."""
    q, c = query_embeddings.contiguous(), candidate_embeddings.contiguous()
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    ws = _ws(nq, nc, d, q.device, forward_only=True)
    lse, per_row = q.new_empty(nq), q.new_empty(nq)
    loss = q.new_empty(1)
    thr = None
    if num_hard_negatives > 0:
        thr = ops.retrieval_hard_negative_thresholds(q, c, inv_temperature, num_hard_negatives, ws,
                                                     cand_prob=candidate_sampling_probability, cand_ids=candidate_ids,
                                                     diag_offset=diag_offset)
    ops.retrieval_fwd(q, c, inv_temperature, ws, lse, per_row, loss, sample_weight=sample_weight,
                      cand_prob=candidate_sampling_probability, cand_ids=candidate_ids, diag_offset=diag_offset, hard_thr=thr,
                      precision=precision)
    return loss.reshape(()), per_row


@retrieval_loss_value.register_fake
def _(q, c, sample_weight, candidate_sampling_probability, candidate_ids, inv_temperature, diag_offset, num_hard_negatives,
      precision="f32"):
    return q.new_empty(()), q.new_empty((q.shape[0],))


_PW_WS: dict = {}


def _pairwise_ws(nq: int, nc: int, d: int, device) -> Tensor:
    """Workspace of the pairwise-loss ops, kept per (device, stream) like the scorer's (the largest one seen)."""
    n = max(ops.retrieval_pairwise_workspace_bytes(nq, nc, d), 1)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n, dtype=torch.uint8, device=device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    hit = _PW_WS.get(key)
    if hit is not None and hit.numel() >= n:
        return hit
    _PW_WS.pop(key, None)
    buf = _PW_WS[key] = torch.empty(n, dtype=torch.uint8, device=device)
    return buf


def _pairwise_thresholds(q, c, sample_prob, candidate_ids, inv_temperature, diag_offset, num_hard_negatives):
    """hard_thr of the pairwise ops: the scorer's hard-negative thresholds (its own forward workspace), None without mining."""
    if num_hard_negatives <= 0:
        return None
    ws = _ws(q.shape[0], c.shape[0], q.shape[1], q.device, forward_only=True)
    return ops.retrieval_hard_negative_thresholds(q, c, inv_temperature, num_hard_negatives, ws, cand_prob=sample_prob,
                                                  cand_ids=candidate_ids, diag_offset=diag_offset)


@torch.library.custom_op(f"{NS}::retrieval_pairwise_loss", mutates_args=(), device_types="cuda")
def retrieval_pairwise_loss(query_embeddings: Tensor, candidate_embeddings: Tensor, sample_weight: Optional[Tensor],
                            candidate_sampling_probability: Optional[Tensor], candidate_ids: Optional[Tensor],
                            inv_temperature: float, diag_offset: int, num_hard_negatives: int, kind: str, margin: float,
                            reduction: str) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Pairwise loss over the in-batch negatives AND its gradients (``ops.retrieval_pairwise_fwd_bwd``): ``kind`` "logistic"
    (BPR: softplus(s_neg - s_pos)) or "hinge" (max(0, margin - (s_pos - s_neg))) on the logits ``retrieval_loss`` sees;
    ``reduction`` "mean" (per row, over its negatives) or "sum".  Returns (loss [], per-example loss [Bq], dLoss/dq, dLoss/dc);
    the autograd formula multiplies the saved gradients by the incoming scalar gradient.  ``candidate_ids`` given = accidental-hit
    removal; ``num_hard_negatives`` > 0 keeps the k hardest negatives per query (the triplet setting)."""
    q, c = query_embeddings.contiguous(), candidate_embeddings.contiguous()
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    thr = _pairwise_thresholds(q, c, candidate_sampling_probability, candidate_ids, inv_temperature, diag_offset, num_hard_negatives)
    per_row, loss = q.new_empty(nq), q.new_empty(1)
    dq, dc = torch.empty_like(q), torch.empty_like(c)
    ops.retrieval_pairwise_fwd_bwd(q, c, inv_temperature, _pairwise_ws(nq, nc, d, q.device), per_row, loss, dq, dc, kind=kind,
                                   margin=margin, reduction=reduction, sample_weight=sample_weight,
                                   cand_prob=candidate_sampling_probability, cand_ids=candidate_ids, diag_offset=diag_offset,
                                   hard_thr=thr)
    return loss.reshape(()), per_row, dq, dc


@retrieval_pairwise_loss.register_fake
def _(q, c, sample_weight, candidate_sampling_probability, candidate_ids, inv_temperature, diag_offset, num_hard_negatives, kind,
      margin, reduction):
    return q.new_empty(()), q.new_empty((q.shape[0],)), torch.empty_like(q), torch.empty_like(c)


def _pairwise_backward(ctx, g_loss, g_per_example, g_dq, g_dc):
    dq, dc = ctx.saved_tensors
    sdq, sdc = torch._foreach_mul((dq, dc), g_loss)
    return sdq, sdc, None, None, None, None, None, None, None, None, None


retrieval_pairwise_loss.register_autograd(_pairwise_backward, setup_context=_retrieval_setup)


@torch.library.custom_op(f"{NS}::retrieval_pairwise_loss_value", mutates_args=(), device_types="cuda")
def retrieval_pairwise_loss_value(query_embeddings: Tensor, candidate_embeddings: Tensor, sample_weight: Optional[Tensor],
                                  candidate_sampling_probability: Optional[Tensor], candidate_ids: Optional[Tensor],
                                  inv_temperature: float, diag_offset: int, num_hard_negatives: int, kind: str, margin: float,
                                  reduction: str) -> Tuple[Tensor, Tensor]:
    """Forward only (validation) of ``retrieval_pairwise_loss``: (loss [], per-example loss [Bq]) in one pass."""
    q, c = query_embeddings.contiguous(), candidate_embeddings.contiguous()
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    thr = _pairwise_thresholds(q, c, candidate_sampling_probability, candidate_ids, inv_temperature, diag_offset, num_hard_negatives)
    per_row, loss = q.new_empty(nq), q.new_empty(1)
    ops.retrieval_pairwise_fwd(q, c, inv_temperature, _pairwise_ws(nq, nc, d, q.device), per_row, loss, kind=kind, margin=margin,
                               reduction=reduction, sample_weight=sample_weight, cand_prob=candidate_sampling_probability,
                               cand_ids=candidate_ids, diag_offset=diag_offset, hard_thr=thr)
    return loss.reshape(()), per_row


@retrieval_pairwise_loss_value.register_fake
def _(q, c, sample_weight, candidate_sampling_probability, candidate_ids, inv_temperature, diag_offset, num_hard_negatives, kind,
      margin, reduction):
    return q.new_empty(()), q.new_empty((q.shape[0],))


@torch.library.custom_op(f"{NS}::retrieval_rank", mutates_args=(), device_types="cuda")
def retrieval_rank(query_embeddings: Tensor, candidate_embeddings: Tensor, true_candidate_index: Tensor,
                   candidate_sampling_probability: Optional[Tensor], inv_temperature: float) -> Tensor:
    """rank[i] = number of candidates scoring strictly above query i's true candidate (int32): Recall@K / NDCG@K."""
    return ops.retrieval_rank(query_embeddings.contiguous(), candidate_embeddings.contiguous(), inv_temperature,
                              true_candidate_index.contiguous(), cand_prob=candidate_sampling_probability)


@retrieval_rank.register_fake
def _(q, c, true_candidate_index, candidate_sampling_probability, inv_temperature):
    return q.new_empty((q.shape[0],), dtype=torch.int32)


@torch.library.custom_op(f"{NS}::retrieval_batch_rank", mutates_args=(), device_types="cuda")
def retrieval_batch_rank(query_embeddings: Tensor, candidate_embeddings: Tensor, candidate_sampling_probability: Optional[Tensor],
                         candidate_ids: Optional[Tensor], inv_temperature: float, diag_offset: int) -> Tensor:
    """In-batch rank of every query's positive under the scores the loss sees (int32): batch top-k accuracy = mean(rank < k)."""
    return ops.retrieval_batch_rank(query_embeddings.contiguous(), candidate_embeddings.contiguous(), inv_temperature,
                                    cand_prob=candidate_sampling_probability, cand_ids=candidate_ids, diag_offset=diag_offset)


@retrieval_batch_rank.register_fake
def _(q, c, candidate_sampling_probability, candidate_ids, inv_temperature, diag_offset):
    return q.new_empty((q.shape[0],), dtype=torch.int32)


_TOPK_WS: dict = {}


def _topk_ws(nq: int, nc: int, d: int, k: int, device) -> Tensor:
    """Workspace of the top-k op, kept per (device, stream) like the scorer's (the largest one seen)."""
    n = max(ops.retrieval_topk_workspace_bytes(nq, nc, d, k), 1)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n, dtype=torch.uint8, device=device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    hit = _TOPK_WS.get(key)
    if hit is not None and hit.numel() >= n:
        return hit
    _TOPK_WS.pop(key, None)
    buf = _TOPK_WS[key] = torch.empty(n, dtype=torch.uint8, device=device)
    return buf


@torch.library.custom_op(f"{NS}::retrieval_topk", mutates_args=(), device_types="cuda")
def retrieval_topk(query_embeddings: Tensor, candidate_embeddings: Tensor, k: int, exclusion_offsets: Optional[Tensor],
                   exclusion_indices: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """Exact top-k of q @ c.T (tfrs BruteForce): (scores f32 [nq, k], indices int64 [nq, k]), ties by ascending index;
    optional CSR exclusions.  Not differentiable (serving)."""
    q, c = query_embeddings.contiguous(), candidate_embeddings.contiguous()
    ex = None if exclusion_offsets is None else (exclusion_offsets.contiguous(), exclusion_indices.contiguous())
    return ops.retrieval_topk(q, c, k, exclusions=ex, workspace=_topk_ws(q.shape[0], c.shape[0], q.shape[1], k, q.device))


@retrieval_topk.register_fake
def _(q, c, k, exclusion_offsets, exclusion_indices):
    return q.new_empty((q.shape[0], k)), q.new_empty((q.shape[0], k), dtype=torch.int64)


_IVF_WS: dict = {}


def _ivf_ws(nq: int, nlist: int, n: int, d: int, k: int, nprobe: int, device) -> Tensor:
    """Workspace of the IVF op, kept per (device, stream) like the top-k op's (the largest one seen)."""
    need = max(ops.ivf_search_workspace_bytes(nq, nlist, n, d, k, nprobe), 1)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(need, dtype=torch.uint8, device=device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    hit = _IVF_WS.get(key)
    if hit is not None and hit.numel() >= need:
        return hit
    _IVF_WS.pop(key, None)
    buf = _IVF_WS[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return buf


@torch.library.custom_op(f"{NS}::ivf_search", mutates_args=(), device_types="cuda")
def ivf_search(query_embeddings: Tensor, centroids: Tensor, list_offsets: Tensor, list_vectors: Tensor, list_ids: Tensor,
               k: int, nprobe: int, exclusion_offsets: Optional[Tensor], exclusion_indices: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """IVF approximate top-k (ops.ivf_search): (scores f32 [nq, k], original item ids int64 [nq, k]) over the items of the
    nprobe best lists, ties by ascending id; optional CSR exclusions of original ids.  Not differentiable (serving)."""
    q = query_embeddings.contiguous()
    ex = None if exclusion_offsets is None else (exclusion_offsets.contiguous(), exclusion_indices.contiguous())
    ws = _ivf_ws(q.shape[0], centroids.shape[0], list_vectors.shape[0], q.shape[1], k, nprobe, q.device)
    return ops.ivf_search(q, centroids.contiguous(), list_offsets.contiguous(), list_vectors.contiguous(), list_ids.contiguous(),
                          k, nprobe, exclusions=ex, workspace=ws)


@ivf_search.register_fake
def _(q, centroids, list_offsets, list_vectors, list_ids, k, nprobe, exclusion_offsets, exclusion_indices):
    return q.new_empty((q.shape[0], k)), q.new_empty((q.shape[0], k), dtype=torch.int64)


_I8_WS: dict = {}


def _i8_ws(nq: int, nc: int, d: int, k: int, k1: int, device) -> Tensor:
    """Workspace of the int8 top-k op, kept per (device, stream) like the top-k op's (the largest one seen)."""
    need = max(ops.retrieval_topk_i8_workspace_bytes(nq, nc, d, k, k1), 1)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(need, dtype=torch.uint8, device=device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    hit = _I8_WS.get(key)
    if hit is not None and hit.numel() >= need:
        return hit
    _I8_WS.pop(key, None)
    buf = _I8_WS[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return buf


@torch.library.custom_op(f"{NS}::quantize_rows_i8", mutates_args=(), device_types="cuda")
def quantize_rows_i8(x: Tensor) -> Tuple[Tensor, Tensor]:
    """Per-row symmetric int8 quantisation (ops.quantize_rows_i8): (codes int8 [n, D], scales f32 [n])."""
    return ops.quantize_rows_i8(x.contiguous())


@quantize_rows_i8.register_fake
def _(x):
    return x.new_empty(x.shape, dtype=torch.int8), x.new_empty((x.shape[0],))


@torch.library.custom_op(f"{NS}::retrieval_topk_i8", mutates_args=(), device_types="cuda")
def retrieval_topk_i8(query_embeddings: Tensor, codes: Tensor, scales: Tensor, candidate_embeddings: Optional[Tensor], k: int,
                      k1: int, exclusion_offsets: Optional[Tensor], exclusion_indices: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """Int8-quantised top-k (ops.retrieval_topk_i8): k1 stage-1 candidates per query from the int8 scan, re-scored exactly
    against candidate_embeddings when given (else k1 must equal k); optional CSR exclusions.  Not differentiable (serving)."""
    q = query_embeddings.contiguous()
    c = None if candidate_embeddings is None else candidate_embeddings.contiguous()
    ex = None if exclusion_offsets is None else (exclusion_offsets.contiguous(), exclusion_indices.contiguous())
    ws = _i8_ws(q.shape[0], codes.shape[0], q.shape[1], k, k1, q.device)
    return ops.retrieval_topk_i8(q, codes.contiguous(), scales.contiguous(), k, c=c, k1=k1, exclusions=ex, workspace=ws)


@retrieval_topk_i8.register_fake
def _(q, codes, scales, c, k, k1, exclusion_offsets, exclusion_indices):
    return q.new_empty((q.shape[0], k)), q.new_empty((q.shape[0], k), dtype=torch.int64)


@torch.library.custom_op(f"{NS}::mmr_rerank", mutates_args=(), device_types="cuda")
def mmr_rerank(scores: Tensor, idx: Tensor, candidate_embeddings: Tensor, k: int, lam: float, groups: Optional[Tensor],
               max_per_group: int) -> Tuple[Tensor, Tensor]:
    """MMR diversified re-ranking of a top-k pool (ops.mmr_rerank): k of the k1 candidates per query, relevance traded
    against the cosine to the items already picked, optionally at most max_per_group per group id.  Not differentiable
    (serving)."""
    g = None if groups is None else groups.contiguous()
    return ops.mmr_rerank(scores.contiguous(), idx.contiguous(), candidate_embeddings.contiguous(), k, lam, groups=g,
                          max_per_group=max_per_group)


@mmr_rerank.register_fake
def _(scores, idx, c, k, lam, groups, max_per_group):
    return scores.new_empty((scores.shape[0], k)), scores.new_empty((scores.shape[0], k), dtype=torch.int64)


_IVF_I8_WS: dict = {}


def _ivf_i8_ws(nq: int, nlist: int, n: int, d: int, k: int, k1: int, nprobe: int, device) -> Tensor:
    """Workspace of the int8 IVF op, kept per (device, stream) like the top-k op's (the largest one seen)."""
    need = max(ops.ivf_search_i8_workspace_bytes(nq, nlist, n, d, k, k1, nprobe), 1)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(need, dtype=torch.uint8, device=device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    hit = _IVF_I8_WS.get(key)
    if hit is not None and hit.numel() >= need:
        return hit
    _IVF_I8_WS.pop(key, None)
    buf = _IVF_I8_WS[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return buf


@torch.library.custom_op(f"{NS}::ivf_search_i8", mutates_args=(), device_types="cuda")
def ivf_search_i8(query_embeddings: Tensor, centroids: Tensor, list_offsets: Tensor, list_codes: Tensor, list_scales: Tensor,
                  list_ids: Tensor, candidate_embeddings: Optional[Tensor], k: int, k1: int, nprobe: int,
                  exclusion_offsets: Optional[Tensor], exclusion_indices: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """Int8 IVF top-k (ops.ivf_search_i8): the int8 scan of the nprobe best lists keeps k1 candidates per query, re-scored
    exactly against candidate_embeddings (the f32 corpus in original id order) when given (else k1 must equal k); optional
    CSR exclusions of original ids.  Not differentiable (serving)."""
    q = query_embeddings.contiguous()
    c = None if candidate_embeddings is None else candidate_embeddings.contiguous()
    ex = None if exclusion_offsets is None else (exclusion_offsets.contiguous(), exclusion_indices.contiguous())
    ws = _ivf_i8_ws(q.shape[0], centroids.shape[0], list_codes.shape[0], q.shape[1], k, k1, nprobe, q.device)
    return ops.ivf_search_i8(q, centroids.contiguous(), list_offsets.contiguous(), list_codes.contiguous(),
                             list_scales.contiguous(), list_ids.contiguous(), k, nprobe, c=c, k1=k1, exclusions=ex, workspace=ws)


@ivf_search_i8.register_fake
def _(q, centroids, list_offsets, list_codes, list_scales, list_ids, c, k, k1, nprobe, exclusion_offsets, exclusion_indices):
    return q.new_empty((q.shape[0], k)), q.new_empty((q.shape[0], k), dtype=torch.int64)


# --------------------------------------------------------------------------------------------- a2 dense layers
@torch.library.custom_op(f"{NS}::dense_fwd", mutates_args=(), device_types="cuda")
def dense_fwd(x: Tensor, w: Tensor, b: Optional[Tensor], relu: bool) -> Tensor:
    """y = act(x @ w + b)  (Keras Dense, [in, out] kernel; f32-input MFMA)."""
    return ops.dense_fwd(x.contiguous(), w.contiguous(), None if b is None else b.contiguous(), relu)


@dense_fwd.register_fake
def _(x, w, b, relu):
    return x.new_empty((x.shape[0], w.shape[1]))


@torch.library.custom_op(f"{NS}::dense_bwd", mutates_args=(), device_types="cuda")
def dense_bwd(x: Tensor, w: Tensor, dy: Tensor, y: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """(dx, dw, db) of y = act(x @ w + b) given dL/dy; ``y`` (the layer's ReLU output) masks dy, None = linear layer.
    dw / db: split-K slabs over the batch summed in slab order (bitwise reproducible)."""
    x, w, dy = x.contiguous(), w.contiguous(), dy.contiguous()
    m, k, n = x.shape[0], x.shape[1], w.shape[1]
    dz = dy if y is None else torch.ops.aten.threshold_backward(dy, y, 0.0)    # dy where y > 0 else 0: ONE kernel (gt + where: two)
    ns = ops.dense_bwd_num_slabs(m)
    dx = torch.empty_like(x)
    dw_slabs, db_slabs = x.new_empty(ns, k, n), x.new_empty(ns, n)
    ops.dense_bwd(x, w, dz, dx, None, dw_slabs, db_slabs)
    dw, db = x.new_empty(k, n), x.new_empty(n)
    segs = [ops.make_dense_seg(dw, None, dw_slabs, ns, 0.0, dw), ops.make_dense_seg(db, None, db_slabs, ns, 0.0, db)]
    ops.dense_update_(segs, "sgd", 0.0, apply=False)          # slab sums only (grad_out), nothing is updated
    return dx, dw, db


@dense_bwd.register_fake
def _(x, w, dy, y):
    return torch.empty_like(x), torch.empty_like(w), x.new_empty((w.shape[1],))


def _dense_setup(ctx, inputs, output):
    x, w, b, relu = inputs
    ctx.save_for_backward(x, w, output if relu else None)
    ctx.has_bias = b is not None


def _dense_backward(ctx, dy):
    x, w, y = ctx.saved_tensors
    dx, dw, db = torch.ops.twotower.dense_bwd(x, w, dy, y)
    return dx, dw, (db if ctx.has_bias else None), None


dense_fwd.register_autograd(_dense_backward, setup_context=_dense_setup)


# --------------------------------------------------------------------------------------------- L2-normalised tower outputs
@torch.library.custom_op(f"{NS}::l2_normalize", mutates_args=(), device_types="cuda")
def l2_normalize(x: Tensor, eps: float = 1e-12) -> Tensor:
    """y = x / sqrt(max(sum(x^2, axis=1), eps)) per row of x [rows, dim] (tf.math.l2_normalize): what a model that scores
    unit-norm embeddings puts between ``dense_fwd`` and ``retrieval_loss``.  Autograd through ``twotower::l2_normalize_bwd``."""
    return ops.l2_normalize(x.contiguous(), eps=eps)


@l2_normalize.register_fake
def _(x, eps=1e-12):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op(f"{NS}::l2_normalize_bwd", mutates_args=(), device_types="cuda")
def l2_normalize_bwd(x: Tensor, dy: Tensor, eps: float = 1e-12) -> Tensor:
    """dx of ``l2_normalize`` at x given dL/dy (the row sums are recomputed from x: the forward saves nothing but x)."""
    return ops.l2_normalize_bwd(x.contiguous(), dy.contiguous(), eps=eps)


@l2_normalize_bwd.register_fake
def _(x, dy, eps=1e-12):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


def _l2_setup(ctx, inputs, output):
    x, eps = inputs
    ctx.save_for_backward(x)
    ctx.eps = eps


def _l2_backward(ctx, dy):
    (x,) = ctx.saved_tensors
    return torch.ops.twotower.l2_normalize_bwd(x, dy, ctx.eps), None


l2_normalize.register_autograd(_l2_backward, setup_context=_l2_setup)


# --------------------------------------------------------------------------------------------- dense numeric side features
@torch.library.custom_op(f"{NS}::dense_features", mutates_args=(), device_types="cuda")
def dense_features(feat: Tensor, ids: Tensor, mean: Optional[Tensor], inv_std: Optional[Tensor], proj: Tensor,
                   clip: float = 0.0) -> Tensor:
    """out[b] = z(feat[ids[b]]) @ proj, z = clamp((x - mean) * inv_std, -clip, clip) (``ops.dense_features``: the numeric side
    features of a tower input; ``mean`` / ``inv_std`` both None: no normalisation).  Autograd with respect to ``proj`` only,
    through ``twotower::dense_features_bwd``: the features are data, not parameters."""
    c = lambda t: None if t is None else t.contiguous()
    return ops.dense_features((feat.contiguous(), ids.contiguous(), c(mean), c(inv_std), proj.contiguous(), None, False, None),
                              clip=clip)[0]


@dense_features.register_fake
def _(feat, ids, mean, inv_std, proj, clip=0.0):
    return proj.new_empty((ids.shape[0], proj.shape[1]))


@torch.library.custom_op(f"{NS}::dense_features_bwd", mutates_args=(), device_types="cuda")
def dense_features_bwd(feat: Tensor, ids: Tensor, mean: Optional[Tensor], inv_std: Optional[Tensor], proj: Tensor, dy: Tensor,
                       clip: float = 0.0) -> Tensor:
    """dL/dproj [F, dim] of ``dense_features`` given dL/dout: the normalised features are recomputed by the forward launch (the
    forward op keeps nothing but its inputs), the backward launch writes the slabs and the slabs are summed here."""
    c = lambda t: None if t is None else t.contiguous()
    z = torch.empty((ids.shape[0], feat.shape[1]), dtype=torch.float32, device=feat.device)
    ops.dense_features((feat.contiguous(), ids.contiguous(), c(mean), c(inv_std), proj.contiguous(), None, False, z), clip=clip)
    (slabs,) = ops.dense_features_bwd((z, dy.contiguous(), None))
    return slabs.sum(dim=0)


@dense_features_bwd.register_fake
def _(feat, ids, mean, inv_std, proj, dy, clip=0.0):
    return torch.empty_like(proj, memory_format=torch.contiguous_format)


def _features_setup(ctx, inputs, output):
    feat, ids, mean, inv_std, proj, clip = inputs
    ctx.save_for_backward(feat, ids, mean, inv_std, proj)
    ctx.clip = clip


def _features_backward(ctx, dy):
    feat, ids, mean, inv_std, proj = ctx.saved_tensors
    dproj = torch.ops.twotower.dense_features_bwd(feat, ids, mean, inv_std, proj, dy, ctx.clip) if ctx.needs_input_grad[4] else None
    return None, None, None, None, dproj, None


dense_features.register_autograd(_features_backward, setup_context=_features_setup)


# --------------------------------------------------------------------------------------------- time-of-interaction context
@torch.library.custom_op(f"{NS}::time_context", mutates_args=(), device_types="cuda")
def time_context(timestamps: Tensor, table: Tensor, fields: str, buckets: int, time_min: int, time_max: int) -> Tensor:
    """out[p] = the sum, in field order, of the rows of ``table`` [R, dim] that ``timestamps[p]`` (int64 seconds since the epoch)
    picks (``ops.time_context``).  ``fields``: the enabled fields, comma separated ("hour,day_of_week,month,period").  Autograd
    with respect to ``table``, through ``twotower::time_context_bwd``."""
    return ops.time_context(timestamps.contiguous(), table.contiguous(), tuple(fields.split(",")), buckets, time_min, time_max)


@time_context.register_fake
def _(timestamps, table, fields, buckets, time_min, time_max):
    return table.new_empty((timestamps.shape[0], table.shape[1]))


@torch.library.custom_op(f"{NS}::time_context_bwd", mutates_args=(), device_types="cuda")
def time_context_bwd(timestamps: Tensor, table: Tensor, dy: Tensor, fields: str, buckets: int, time_min: int, time_max: int) -> Tensor:
    """dL/dtable [R, dim] of ``time_context`` given dL/dout: the row indices are recomputed by the forward launch (the forward op
    keeps nothing but its inputs), the backward launch writes the fully reduced gradient."""
    f = tuple(fields.split(","))
    idx = torch.empty((timestamps.shape[0], len(f)), dtype=torch.int32, device=table.device)
    ops.time_context(timestamps.contiguous(), table.contiguous(), f, buckets, time_min, time_max, idx_out=idx)
    return ops.time_context_bwd(idx, dy.contiguous(), f, buckets)


@time_context_bwd.register_fake
def _(timestamps, table, dy, fields, buckets, time_min, time_max):
    return torch.empty_like(table, memory_format=torch.contiguous_format)


def _time_setup(ctx, inputs, output):
    timestamps, table, ctx.fields, ctx.buckets, ctx.time_min, ctx.time_max = inputs
    ctx.save_for_backward(timestamps, table)


def _time_backward(ctx, dy):
    timestamps, table = ctx.saved_tensors
    dtable = None
    if ctx.needs_input_grad[1]:
        dtable = torch.ops.twotower.time_context_bwd(timestamps, table, dy, ctx.fields, ctx.buckets, ctx.time_min, ctx.time_max)
    return None, dtable, None, None, None, None


time_context.register_autograd(_time_backward, setup_context=_time_setup)


# --------------------------------------------------------------------------------------------- rating-prediction head
@torch.library.custom_op(f"{NS}::rating_head", mutates_args=(), device_types="cuda")
def rating_head(q: Tensor, c: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor) -> Tensor:
    """pred [n] = b2 + relu(b1 + q @ w1[:D] + c @ w1[D:]) @ w2 (``ops.rating_head``: one launch).  Autograd with respect to all
    six inputs through ``twotower::rating_head_bwd``."""
    return ops.rating_head(q.contiguous(), c.contiguous(), w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous())[0]


@rating_head.register_fake
def _(q, c, w1, b1, w2, b2):
    return q.new_empty((q.shape[0],))


@torch.library.custom_op(f"{NS}::rating_head_bwd", mutates_args=(), device_types="cuda")
def rating_head_bwd(q: Tensor, c: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor,
                    grad_pred: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The six input gradients of ``rating_head`` given dL/dpred: h is recomputed by the forward launch (the forward op keeps
    nothing but its inputs); the ONE backward launch takes the upstream gradient in the place of the error (pred = grad_pred,
    rating = 0, grad_scale = 1: g = grad_pred exactly), and its slabs are summed here."""
    q, c, w1, w2 = q.contiguous(), c.contiguous(), w1.contiguous(), w2.contiguous()
    n, d = q.shape
    hd = w2.numel()
    _, h = ops.rating_head(q, c, w1, b1.contiguous(), w2, b2.contiguous())
    dq, dc = torch.empty_like(q), torch.empty_like(c)
    if n == 0:
        z = lambda t: torch.zeros_like(t, memory_format=torch.contiguous_format)
        return dq, dc, z(w1), z(b1), z(w2), z(b2)
    _, _, ks, bs, _ = ops.rating_head_bwd(q, c, h, grad_pred.to(torch.float32).contiguous(), torch.zeros(n, device=q.device), w1, w2,
                                          1.0, dq, dc)
    ks, bs = ks.sum(dim=0), bs.sum(dim=0)
    return dq, dc, ks[:2 * d * hd].view(2 * d, hd).clone(), bs[:hd].clone(), ks[2 * d * hd:].clone(), bs[hd:].clone()


@rating_head_bwd.register_fake
def _(q, c, w1, b1, w2, b2, grad_pred):
    e = lambda t: torch.empty_like(t, memory_format=torch.contiguous_format)
    return e(q), e(c), e(w1), e(b1), e(w2), e(b2)


def _rating_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _rating_backward(ctx, grad_pred):
    return torch.ops.twotower.rating_head_bwd(*ctx.saved_tensors, grad_pred)


rating_head.register_autograd(_rating_backward, setup_context=_rating_setup)


# --------------------------------------------------------------------------------------------- DCN-v2 cross layer
@torch.library.custom_op(f"{NS}::cross_layer", mutates_args=(), device_types="cuda")
def cross_layer(x0: Tensor, x: Tensor, w: Tensor, b: Tensor) -> Tensor:
    """y [n, D] = x0 * (x @ w + b) + x (``ops.cross_layer``: one launch; tfrs.layers.dcn.Cross with x0 the stack's input).
    Autograd with respect to all four inputs through ``twotower::cross_layer_bwd``."""
    return ops.cross_layer((x0.contiguous(), x.contiguous(), w.contiguous(), b.contiguous(), None))[0]


@cross_layer.register_fake
def _(x0, x, w, b):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op(f"{NS}::cross_layer_bwd", mutates_args=(), device_types="cuda")
def cross_layer_bwd(x0: Tensor, x: Tensor, w: Tensor, b: Tensor, grad_y: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The four input gradients of ``cross_layer`` given dL/dy: u is recomputed by the forward launch (the forward op keeps
    nothing but its inputs), the ONE backward launch runs in its upper-layer form (x0 and x are separate inputs) and its slabs
    are summed here."""
    x0, x, w, b = x0.contiguous(), x.contiguous(), w.contiguous(), b.contiguous()
    n = x.shape[0]
    if n == 0:
        z = lambda t: torch.zeros_like(t, memory_format=torch.contiguous_format)
        return z(x0), z(x), z(w), z(b)
    u = torch.empty_like(x)
    ops.cross_layer((x0, x, w, b, None), u=(u,))
    ((dx, dx0, dws, dbs),) = ops.cross_layer_bwd((x0, x, u, w, grad_y.to(torch.float32).contiguous(), None, None, None, None))
    return dx0, dx, dws.sum(dim=0), dbs.sum(dim=0)


@cross_layer_bwd.register_fake
def _(x0, x, w, b, grad_y):
    e = lambda t: torch.empty_like(t, memory_format=torch.contiguous_format)
    return e(x0), e(x), e(w), e(b)


def _cross_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _cross_backward(ctx, grad_y):
    return torch.ops.twotower.cross_layer_bwd(*ctx.saved_tensors, grad_y)


cross_layer.register_autograd(_cross_backward, setup_context=_cross_setup)


# --------------------------------------------------------------------------------------------- layer normalisation
@torch.library.custom_op(f"{NS}::layer_norm", mutates_args=(), device_types="cuda")
def layer_norm(z: Tensor, gamma: Tensor, beta: Tensor, eps: float, relu: bool) -> Tensor:
    """y [rows, dim] = act(LayerNorm(z) * gamma + beta) over the last dim (``ops.layer_norm2``: one launch; Keras
    LayerNormalization, biased two-pass variance, ``relu``: a ReLU behind it; no dropout).  dim a multiple of 32 in 32..1024.
    Autograd with respect to z, gamma and beta through ``twotower::layer_norm_bwd``."""
    return ops.layer_norm2((z.contiguous(), gamma.contiguous(), beta.contiguous(), None, None), eps=eps, relu=relu)[0]


@layer_norm.register_fake
def _(z, gamma, beta, eps, relu):
    return torch.empty_like(z, memory_format=torch.contiguous_format)


@torch.library.custom_op(f"{NS}::layer_norm_bwd", mutates_args=(), device_types="cuda")
def layer_norm_bwd(z: Tensor, gamma: Tensor, y: Tensor, grad_y: Tensor, eps: float, relu: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """(dz, dgamma, dbeta) of ``layer_norm`` given dL/dy: with ``relu`` the gradient is masked by y > 0 first; mean and variance
    are recomputed from z by the ONE backward launch, whose slabs are summed here."""
    z, gamma = z.contiguous(), gamma.contiguous()
    if z.shape[0] == 0:
        return torch.zeros_like(z), torch.zeros_like(gamma), torch.zeros_like(gamma)
    dn = grad_y.to(torch.float32).contiguous()
    dn = torch.where(y > 0, dn, torch.zeros_like(dn)) if relu else dn.clone()
    ((dz, dgs, dbs),) = ops.layer_norm_bwd2((z, gamma, dn, dn, None, None), eps=eps)
    return dz, dgs.sum(dim=0), dbs.sum(dim=0)


@layer_norm_bwd.register_fake
def _(z, gamma, y, grad_y, eps, relu):
    e = lambda t: torch.empty_like(t, memory_format=torch.contiguous_format)
    return e(z), e(gamma), e(gamma)


def _layer_norm_setup(ctx, inputs, output):
    z, gamma, _, ctx.eps, ctx.relu = inputs
    ctx.save_for_backward(z, gamma, output)


def _layer_norm_backward(ctx, grad_y):
    z, gamma, y = ctx.saved_tensors
    dz, dg, db = torch.ops.twotower.layer_norm_bwd(z, gamma, y, grad_y, ctx.eps, ctx.relu)
    return dz, dg, db, None, None


layer_norm.register_autograd(_layer_norm_backward, setup_context=_layer_norm_setup)


# --------------------------------------------------------------------------------------------- a5 sparse optimizer
@torch.library.custom_op(f"{NS}::sparse_update_", mutates_args=("table", "accum"), device_types="cuda")
def sparse_update_(table: Tensor, accum: Optional[Tensor], grads: Tensor, ids: Tensor, optimizer: str, lr: float,
                   eps: float) -> None:
    """Fused sparse SGD / Keras-2.15 Adagrad on the rows ``ids`` of ``table`` (in place; duplicates summed first, in
    ascending position order): one sort launch + one apply launch."""
    if optimizer not in ("sgd", "adagrad"):
        raise ValueError(f"optimizer must be 'sgd' or 'adagrad', got {optimizer!r}")
    plan = _plan(ids.numel(), ids.device).run(ids.contiguous(), table.shape[0])
    if optimizer == "sgd":
        ops.sparse_sgd_(table, grads.contiguous(), plan, lr)
    else:
        if accum is None:
            raise ValueError("sparse_update_: Adagrad needs the accumulator tensor")
        ops.sparse_adagrad_(table, accum, grads.contiguous(), plan, lr, eps)


@torch.library.custom_op(f"{NS}::sparse_adam_", mutates_args=("table", "exp_avg", "exp_avg_sq"), device_types="cuda")
def sparse_adam_(table: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, grads: Tensor, ids: Tensor, step: int, lr: float,
                 beta1: float, beta2: float, eps: float) -> None:
    """Lazy Adam (TF-Addons LazyAdam / torch.optim.SparseAdam, Keras's epsilon placement) on the rows ``ids`` of ``table`` (in
    place; duplicates summed first; ``step`` is the 1-based global step of the bias correction): one sort launch + two launches."""
    plan = _plan(ids.numel(), ids.device).run(ids.contiguous(), table.shape[0])
    ops.adam_step_([(table, exp_avg, exp_avg_sq, grads.contiguous(), plan)], [], ops.AdamHyper(lr, beta1, beta2, eps, step))


@torch.library.custom_op(f"{NS}::sparse_rowwise_adagrad_", mutates_args=("table", "row_accum"), device_types="cuda")
def sparse_rowwise_adagrad_(table: Tensor, row_accum: Tensor, grads: Tensor, ids: Tensor, lr: float, eps: float) -> None:
    """Row-wise Adagrad (FBGEMM / TorchRec's "exact row-wise" Adagrad, Keras's epsilon placement) on the rows ``ids`` of ``table``
    (in place; duplicates summed first): ``row_accum`` [rows] holds ONE accumulator per row and grows by the mean of the row's
    squared gradient.  One sort launch + two launches."""
    plan = _plan(ids.numel(), ids.device).run(ids.contiguous(), table.shape[0])
    ops.rowwise_adagrad_step_([(table, row_accum, grads.contiguous(), plan)], [], lr, eps)


# --------------------------------------------------------------------------------------------- global-norm gradient clipping
@torch.library.custom_op(f"{NS}::clip_by_global_norm_", mutates_args=("tensors",), device_types="cuda")
def clip_by_global_norm_(tensors: List[Tensor], clip_norm: float) -> Tensor:
    """tf.clip_by_global_norm / ``torch.nn.utils.clip_grad_norm_`` over contiguous f32 gradient tensors IN PLACE, two launches
    for all of them (``ops.clip_global_norm_``: up to 24 tensors per call): every tensor *= clip_norm / max(norm, clip_norm).
    Returns [the norm before clipping, the scale] (2 f32 on the device, unsynchronised)."""
    for t in tensors:
        ops._chk(t, torch.float32, "tensors")
    if not tensors:
        raise ValueError("clip_by_global_norm_: no tensors")
    stats = torch.empty(2, device=tensors[0].device)
    return ops.clip_global_norm_([], [ops.make_clip_dense(t.view(-1), t.numel()) for t in tensors], clip_norm, stats=stats)


@clip_by_global_norm_.register_fake
def _(tensors, clip_norm):
    return torch.empty(2, dtype=torch.float32, device=tensors[0].device)


# --------------------------------------------------------------------------------------------- streaming frequency estimation
@torch.library.custom_op(f"{NS}::frequency_estimate_", mutates_args=("sketch",), device_types="cuda")
def frequency_estimate_(sketch: Tensor, ids: Tensor, n_update: int, step: int, alpha: float, n_items: int, seed: int,
                        tensor_id: int, sampler_prob: Optional[Tensor], mix: bool) -> Tensor:
    """The streaming frequency estimator of the logQ correction (``ops.frequency_estimate_``, Yi et al. 2019): the first
    ``n_update`` of ``ids`` update ``sketch`` (int64 [hashes, slots], ``ops.new_frequency_sketch``) IN PLACE at the 1-based
    ``step``; returns every id's estimated probability [len(ids)] - the ``candidate_sampling_probability`` of
    ``retrieval_loss`` (``mix``: under the mixture with ``len(ids) - n_update`` sampled negatives)."""
    prob = torch.empty(ids.numel(), dtype=torch.float32, device=ids.device)
    ops.frequency_estimate_(sketch, ids.contiguous(), n_update, step, alpha, n_items, prob, seed=seed, tensor_id=tensor_id,
                            sampler_prob=None if sampler_prob is None else sampler_prob.contiguous(), mix=mix)
    return prob


@frequency_estimate_.register_fake
def _(sketch, ids, n_update, step, alpha, n_items, seed, tensor_id, sampler_prob, mix):
    return ids.new_empty((ids.shape[0],), dtype=torch.float32)


OPS = ("frequency_estimate_", "clip_by_global_norm_", "embedding_gather","embedding_bag", "history_bag", "history_attention", "history_attention_bwd", "history_gru", "history_gru_bwd", "history_self_attention", "history_self_attention_bwd", "retrieval_loss", "retrieval_loss_value", "retrieval_rank", "retrieval_batch_rank", "retrieval_topk", "ivf_search", "quantize_rows_i8", "retrieval_topk_i8", "ivf_search_i8", "mmr_rerank", "dense_fwd",
       "dense_bwd", "l2_normalize", "l2_normalize_bwd", "dense_features", "dense_features_bwd", "time_context", "time_context_bwd", "rating_head", "rating_head_bwd", "cross_layer", "cross_layer_bwd", "layer_norm", "layer_norm_bwd", "sparse_update_", "sparse_adam_", "sparse_rowwise_adagrad_")
