"""Serving: exact nearest-neighbour retrieval over the item corpus, shaped like ``tfrs.layers.factorized_top_k.BruteForce``
(the serving side the reference's README promises and its ``src/serving/`` leaves empty).

    bf = BruteForce(k=10).index_from_trainer(trainer)          # item-tower corpus; the user tower as the query model
    scores, item_ids = bf(torch.tensor([3, 17, 42]))           # [3, 10] each
    scores, item_ids = bf.query_with_exclusions(users, seen)   # never returns an excluded item

Every call is one ``tt_retrieval_topk_f32`` (score-and-select fused on the f32 MFMA, then a merge across corpus splits):
no [queries x corpus] score matrix is formed.  Ties are broken by the lower candidate index, so the answer is unique.
"""
from __future__ import annotations

import torch

from . import ops


class BruteForce:
    """Exact top-k retrieval index.  ``query_model``: a callable mapping the queries passed to ``__call__`` to
    [nq, D] f32 embeddings (None: the queries ARE the embeddings).  ``k``: default number of results."""

    def __init__(self, query_model=None, k: int = 10):
        self.query_model = query_model
        self.k = int(k)
        self._candidates = None
        self._identifiers = None
        self._ws = None                      # workspace kept across calls (the largest needed so far)

    def index(self, candidates: torch.Tensor, identifiers=None) -> "BruteForce":
        """candidates: [n, D] f32 device tensor.  identifiers: optional [n] integer tensor; results then carry
        identifiers[index] instead of the row index (padding stays -1)."""
        if candidates.dim() != 2:
            raise ValueError(f"BruteForce.index: candidates must be [n, D], got shape {tuple(candidates.shape)}")
        self._candidates = candidates.detach().to(torch.float32).contiguous()
        if identifiers is not None:
            ids = torch.as_tensor(identifiers, device=self._candidates.device)
            if ids.dim() != 1 or ids.numel() != candidates.shape[0]:
                raise ValueError(f"BruteForce.index: identifiers must be [{candidates.shape[0]}], got {tuple(ids.shape)}")
            if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
                raise TypeError(f"BruteForce.index: identifiers must be integers, got {ids.dtype}")
            identifiers = ids.to(torch.int64).contiguous()
        self._identifiers = identifiers
        return self

    def index_from_trainer(self, trainer, item_category_ids: torch.Tensor | None = None) -> "BruteForce":
        """Index the trainer's whole item corpus (``item_corpus_embeddings``); unless a query model was given, queries
        are user ids run through the user tower (``user_embeddings``)."""
        self.index(trainer.item_corpus_embeddings(item_category_ids))
        if self.query_model is None:
            self.query_model = trainer.user_embeddings
        return self

    def _workspace(self, nq: int, k: int) -> torch.Tensor:
        c = self._candidates
        n = max(ops.retrieval_topk_workspace_bytes(nq, c.shape[0], c.shape[1], k), 1)
        if self._ws is None or self._ws.numel() < n:
            self._ws = None
            self._ws = torch.empty(n, dtype=torch.uint8, device=c.device)
        return self._ws

    def _query(self, queries, exclusions, k):
        if self._candidates is None:
            raise RuntimeError("BruteForce: call index() or index_from_trainer() first")
        q = self.query_model(queries) if self.query_model is not None else queries
        q = q.to(torch.float32).contiguous()
        if q.dim() == 1:
            q = q[None]
        k = self.k if k is None else int(k)
        scores, idx = ops.retrieval_topk(q, self._candidates, k, exclusions=exclusions, workspace=self._workspace(q.shape[0], k))
        if self._identifiers is None:
            return scores, idx
        ids = self._identifiers[idx.clamp(min=0)]
        return scores, torch.where(idx >= 0, ids, torch.full_like(ids, -1))

    def __call__(self, queries, k: int | None = None):
        """(scores f32 [nq, k], identifiers or indices int64 [nq, k]), best first."""
        return self._query(queries, None, k)

    def query_with_exclusions(self, queries, exclusions, k: int | None = None):
        """As ``__call__``, never returning an excluded candidate.  ``exclusions`` holds candidate ROW indices: a padded
        [nq, E] int64 tensor (-1 = padding) or a CSR pair (offsets [nq + 1], indices).  When fewer than k candidates
        remain, the tail is (-inf, -1)."""
        return self._query(queries, exclusions, k)
