"""``Retrieval`` — the task object of the hot path, with the call signature of
``tfrs.tasks.Retrieval`` (tensorflow-recommenders 0.7.x; the reference declares the dependency at
``/root/reference/pyproject.toml:24`` and the settings at ``configs/data_config.yaml:68-71`` but never
calls it).  The scorer, the in-batch sampled-softmax loss and its gradient run in ONE family of fused
HIP kernels (csrc/score.hip); softmax probabilities are never stored (the exact-f32 training entry keeps the raw
[num_queries, num_candidates] dot products in its workspace between its two passes; the forward-only form keeps nothing).

The task dispatches through the registered custom ops ``torch.ops.twotower.retrieval_loss`` (training: loss and
both gradients in the fused two-pass form, 6*Bq*Bc*D executed FLOPs, gradients saved for autograd) and
``torch.ops.twotower.retrieval_loss_value`` (no gradient needed: one statistics pass) — ``torch_ops.py``.

Pairwise losses over the in-batch negatives run in a kernel family of their own (csrc/pairwise.hip, the ops
``torch.ops.twotower.retrieval_pairwise_loss`` / ``retrieval_pairwise_loss_value``): ``loss=tasks.PairwiseLogisticLoss()``
(alias ``tasks.BPRLoss``: sum over the negatives j of softplus(s_ij - s_i,pos), Rendle 2009) and
``loss=tasks.PairwiseHingeLoss(margin=1.0)`` (sum of max(0, margin - (s_i,pos - s_ij)): the triplet loss, with
``num_hard_negatives=k`` over the k hardest negatives).  The logits are the ones the softmax sees (temperature,
sampling-probability correction), accidental hits and mined-out negatives are not pairs, ``sample_weight`` weights a query's
row.  A stated choice: ``reduction="mean"`` (the default) divides every query's sum by ITS number of negatives, so that a
margin and a learning rate keep their meaning when the batch size changes, and ``reduction="sum"`` is the plain sum over all
pairs; the loss is then summed over the queries, like the softmax loss.  This is NOT TF-Ranking's normalisation (which
averages over all pairs of the batch).  A query without negatives contributes nothing.  f32 only.

Differences from TFRS, all loud:
  * ``loss`` must be None, ``tasks.CategoricalCrossentropy(from_logits=True, reduction="sum")`` - the TFRS default - or one of
    the two pairwise losses above; anything else (pointwise / MSE losses of tfrs.losses, another reduction of the
    cross-entropy) needs the [queries x candidates] score matrix and raises NotImplementedError;
  * ``metrics`` takes a ``metrics.FactorizedTopK`` built WITH its candidate corpus (``FactorizedTopK(candidates=...)``);
    it is updated when ``compute_metrics`` is true, and ``candidate_ids`` must then be the int64 index of every
    candidate in that corpus (the reference's ``item_idx``); ``loss_metrics`` takes objects with
    ``update_state(loss)``; ``batch_metrics`` takes ``metrics.TopKCategoricalAccuracy(k)`` objects (the Keras metric TFRS
    users pass there): in-batch top-k accuracy is ``rank < k`` from one fused rank pass over the batch's candidates, under
    the scores the loss sees (temperature, sampling-probability correction, accidental hits removed) - no score matrix;
    any other Keras metric would need the [queries x candidates] matrix and raises TypeError.  As in TFRS
    (``metric.update_state(labels, scores)``) they are NOT weighted by ``sample_weight``.  TFRS computes them on the scores
    AFTER hard-negative mining; the rank pass sees every in-batch candidate, so ``batch_metrics`` together with
    ``num_hard_negatives`` raises NotImplementedError instead of reporting a different number;
  * ``num_hard_negatives=k`` keeps the positive and the k highest-scoring negatives per query
    (tfrs.layers.loss.HardNegativeMining); negatives tied with the k-th are all kept;
  * ``candidate_ids`` must be an int64 tensor (the reference's ids are int64:
    ``prepare_training_data.py:209-210``).
"""
from __future__ import annotations

import torch

from . import torch_ops  # noqa: F401  (registers torch.ops.twotower.*)


class CategoricalCrossentropy:
    """Marker for the TFRS default loss (``tf.keras.losses.CategoricalCrossentropy(from_logits=True, reduction=SUM)``)."""

    def __init__(self, from_logits: bool = True, reduction: str = "sum"):
        self.from_logits, self.reduction = bool(from_logits), str(reduction).lower()


class _PairwiseLoss:
    kind = None

    def __init__(self, reduction: str = "mean"):
        self.reduction = str(reduction).lower()
        if self.reduction not in ("mean", "sum"):
            raise ValueError(f"{type(self).__name__}(reduction=...): 'mean' (per query, over its negatives) or 'sum', "
                             f"got {reduction!r}")
        self.margin = 1.0                    # (read by the hinge only)


class PairwiseLogisticLoss(_PairwiseLoss):
    """BPR / pairwise logistic loss over the in-batch negatives: softplus(s_neg - s_pos) per (positive, negative) pair."""
    kind = "logistic"


BPRLoss = PairwiseLogisticLoss


class PairwiseHingeLoss(_PairwiseLoss):
    """Pairwise hinge (triplet) loss over the in-batch negatives: max(0, margin - (s_pos - s_neg)) per pair."""
    kind = "hinge"

    def __init__(self, margin: float = 1.0, reduction: str = "mean"):
        super().__init__(reduction)
        self.margin = float(margin)
        if self.margin != self.margin or self.margin in (float("inf"), float("-inf")):
            raise ValueError(f"PairwiseHingeLoss(margin=...): must be finite, got {margin!r}")


class Retrieval:
    """A factorized retrieval task: in-batch softmax (or a pairwise loss) over query x candidate dot products."""

    def __init__(self, loss=None, metrics=None, batch_metrics=None, loss_metrics=None, temperature=None,
                 num_hard_negatives=None, remove_accidental_hits=False, name="retrieval_task", precision="f32"):
        self._pairwise = loss if isinstance(loss, _PairwiseLoss) else None
        if loss is not None and self._pairwise is None and not (
                isinstance(loss, CategoricalCrossentropy) and loss.from_logits and loss.reduction == "sum"):
            raise NotImplementedError("Retrieval(loss=...): the HIP path implements the TFRS default loss - tasks."
                                      "CategoricalCrossentropy(from_logits=True, reduction='sum') - and the pairwise losses "
                                      "tasks.PairwiseLogisticLoss / BPRLoss and tasks.PairwiseHingeLoss; pointwise losses (and "
                                      "other reductions of the cross-entropy) need the [queries x candidates] score matrix, "
                                      "which the fused kernels never materialise")
        from .metrics import TopKCategoricalAccuracy
        self._batch_metrics = list(batch_metrics) if batch_metrics is not None else []
        for m in self._batch_metrics:
            if not isinstance(m, TopKCategoricalAccuracy):
                raise TypeError("Retrieval(batch_metrics=...) takes metrics.TopKCategoricalAccuracy(k) objects (in-batch top-k "
                                "accuracy from the fused rank pass); other metrics would need the in-batch score matrix")
        if metrics is not None:
            from .metrics import FactorizedTopK
            if not isinstance(metrics, FactorizedTopK) or metrics.candidates is None:
                raise TypeError("Retrieval(metrics=...) takes a metrics.FactorizedTopK built with its candidate corpus "
                                "(FactorizedTopK(candidates=item_corpus_embeddings))")
        if self._batch_metrics and num_hard_negatives is not None:
            raise NotImplementedError("Retrieval(batch_metrics=..., num_hard_negatives=k): TFRS evaluates batch metrics on the scores "
                                      "after hard-negative mining; the fused rank pass ranks against every in-batch candidate")
        self._factorized_metrics = metrics
        self._loss_metrics = list(loss_metrics) if loss_metrics is not None else []
        for m in self._loss_metrics:
            if not hasattr(m, "update_state"):
                raise TypeError("Retrieval(loss_metrics=...): every entry needs update_state(loss)")
        if num_hard_negatives is not None and num_hard_negatives < 1:
            raise ValueError("num_hard_negatives must be a positive integer")
        if temperature is not None and temperature <= 0:
            raise ValueError("temperature must be positive")
        self._temperature = temperature
        self._num_hard_negatives = num_hard_negatives
        self._remove_accidental_hits = remove_accidental_hits
        if precision not in ("f32", "bf16x3"):
            raise ValueError("precision must be 'f32' or 'bf16x3'")
        if self._pairwise is not None and precision != "f32":
            raise NotImplementedError("Retrieval(loss=<pairwise loss>, precision='bf16x3'): the pairwise kernels are exact f32 only")
        self._precision = precision          # (extension) matrix-product precision of the training passes: torch_ops.py
        self.name = name
        self.last_per_example_loss = None

    @property
    def factorized_metrics(self):
        return self._factorized_metrics

    def __call__(self, query_embeddings, candidate_embeddings, sample_weight=None, candidate_sampling_probability=None,
                 candidate_ids=None, compute_metrics=True, compute_batch_metrics=True, diag_offset: int = 0):
        """Returns the scalar loss (a 0-d CUDA tensor with autograd).  ``diag_offset`` (extension): the
        positive of query i is candidate i + diag_offset — used by the sharded multi-GPU slab."""
        if self._remove_accidental_hits and candidate_ids is None:
            raise ValueError("When accidental hit removal is enabled, candidate ids must be supplied.")
        q, c = query_embeddings, candidate_embeddings
        if q.dim() != 2 or c.dim() != 2 or q.shape[1] != c.shape[1]:
            raise RuntimeError(f"Retrieval: expected [Bq,D] and [Bc,D] embeddings, got {tuple(q.shape)} and {tuple(c.shape)}")
        inv_t = 1.0 if self._temperature is None else 1.0 / self._temperature
        ids = candidate_ids if self._remove_accidental_hits else None
        sw = None if sample_weight is None else sample_weight.to(torch.float32).contiguous()
        cp = None if candidate_sampling_probability is None else candidate_sampling_probability.to(torch.float32).contiguous()
        k = 0 if self._num_hard_negatives is None else int(self._num_hard_negatives)
        pw = self._pairwise
        if pw is not None and torch.is_grad_enabled() and (q.requires_grad or c.requires_grad):
            loss, per_example, _, _ = torch.ops.twotower.retrieval_pairwise_loss(q, c, sw, cp, ids, inv_t, diag_offset, k, pw.kind,
                                                                                 pw.margin, pw.reduction)
        elif pw is not None:
            loss, per_example = torch.ops.twotower.retrieval_pairwise_loss_value(q, c, sw, cp, ids, inv_t, diag_offset, k, pw.kind,
                                                                                 pw.margin, pw.reduction)
        elif torch.is_grad_enabled() and (q.requires_grad or c.requires_grad):
            loss, per_example, _, _ = torch.ops.twotower.retrieval_loss(q, c, sw, cp, ids, inv_t, diag_offset, k, self._precision)
        else:
            loss, per_example = torch.ops.twotower.retrieval_loss_value(q, c, sw, cp, ids, inv_t, diag_offset, k, self._precision)
        self.last_per_example_loss = per_example
        if compute_metrics and self._factorized_metrics is not None:
            if candidate_ids is None:
                raise ValueError("Retrieval(metrics=FactorizedTopK): pass candidate_ids = the index of every candidate "
                                 "in the metric's corpus")
            with torch.no_grad():
                true_index = candidate_ids[diag_offset:diag_offset + q.shape[0]]
                self._factorized_metrics.update_state(q.detach(), None, true_index)
        if compute_batch_metrics and self._batch_metrics:
            with torch.no_grad():
                rank = torch.ops.twotower.retrieval_batch_rank(q.detach(), c.detach(), cp, ids, inv_t, diag_offset)
                for m in self._batch_metrics:
                    m.update_state_from_ranks(rank)              # unweighted, as TFRS: only the loss and loss_metrics see sample_weight
        for m in self._loss_metrics:
            m.update_state(loss.detach())
        return loss

    @property
    def batch_metrics(self):
        return self._batch_metrics

    call = __call__


class MeanSquaredError:
    """Marker for ``tf.keras.losses.MeanSquaredError()`` (reduction SUM_OVER_BATCH_SIZE), the one loss ``Ranking`` implements."""


class Ranking:
    """A ranking task with the call signature of ``tfrs.tasks.Ranking``: ``task(labels, predictions, sample_weight=None)``
    returns the scalar loss, here the mean squared error - mean over ALL n pairs (Keras SUM_OVER_BATCH_SIZE: the divisor is n)
    of w (prediction - label)^2.  (Extension) a NaN label is a missing one: the pair contributes nothing, the divisor stays n.
    The predictions come from ``torch.ops.twotower.rating_head`` (the HIP rating head, with autograd); the loss itself is
    n elementwise operations in torch.  ``metrics`` takes objects with ``update_state(labels, predictions)``."""

    def __init__(self, loss=None, metrics=None, name="ranking_task"):
        if loss is not None and not isinstance(loss, MeanSquaredError):
            raise NotImplementedError("Ranking(loss=...): only tasks.MeanSquaredError() is implemented")
        self._metrics = list(metrics) if metrics is not None else []
        for m in self._metrics:
            if not hasattr(m, "update_state"):
                raise TypeError("Ranking(metrics=...): every entry needs update_state(labels, predictions)")
        self.name = name

    def __call__(self, labels, predictions, sample_weight=None, compute_metrics=True):
        labels = labels.to(predictions.dtype).reshape(-1)
        predictions = predictions.reshape(-1)
        if labels.numel() != predictions.numel():
            raise RuntimeError(f"Ranking: {labels.numel()} labels for {predictions.numel()} predictions")
        valid = torch.isfinite(labels)
        e = torch.where(valid, predictions - torch.nan_to_num(labels), torch.zeros_like(predictions))
        e2 = e * e
        if sample_weight is not None:
            e2 = e2 * sample_weight.to(predictions.dtype).reshape(-1)
        loss = e2.sum() / max(predictions.numel(), 1)
        if compute_metrics:
            with torch.no_grad():
                for m in self._metrics:
                    m.update_state(labels, predictions.detach())
        return loss

    call = __call__
