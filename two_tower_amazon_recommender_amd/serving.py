"""Serving: exact nearest-neighbour retrieval over the item corpus, shaped like ``tfrs.layers.factorized_top_k.BruteForce``
(the serving side the reference's README promises and its ``src/serving/`` leaves empty).

    bf = BruteForce(k=10).index_from_trainer(trainer)          # item-tower corpus; the user tower as the query model
    scores, item_ids = bf(torch.tensor([3, 17, 42]))           # [3, 10] each
    scores, item_ids = bf.query_with_exclusions(users, seen)   # never returns an excluded item

Every call is one ``tt_retrieval_topk_f32`` (score-and-select fused on the f32 MFMA, then a merge across corpus splits):
no [queries x corpus] score matrix is formed.  Ties are broken by the lower candidate index, so the answer is unique.

``IVF`` is the approximate index next to it (an inverted file: spherical k-means lists, ``nprobe`` lists scanned per query,
one ``tt_ivf_search_f32`` per call).  It has the same methods and answers exactly what ``BruteForce`` answers over the
items of the probed lists; with ``nprobe = nlist`` the two agree bit for bit.

    ivf = IVF(k=10, nlist=1024, nprobe=32).index_from_trainer(trainer)

``Int8BruteForce`` scans the whole corpus as int8 codes (a quarter of the bytes; one ``tt_retrieval_topk_i8_f32`` per
call) and re-scores the ``rerank * k`` survivors of every query exactly, so the scores it returns are ``BruteForce``'s;
with ``keep_f32=False`` it serves the quantised order alone, from a quarter of the memory.

    i8 = Int8BruteForce(k=10, rerank=4).index_from_trainer(trainer)

``Int8IVF`` combines the two: ``IVF``'s lists held as int8 codes (one ``tt_ivf_search_i8_f32`` per call), the same exact
re-rank; it answers what ``Int8BruteForce`` answers over the items of the probed lists.

    i8ivf = Int8IVF(k=10, nlist=1024, nprobe=32, rerank=4).index_from_trainer(trainer)

``MMR`` wraps any of the four and diversifies what it returns: the index is asked for a pool of ``pool * k`` candidates,
and one ``tt_mmr_rerank_f32`` launch per call picks k of them greedily, trading the (min-max normalised) score against the
largest cosine to an item already picked (Maximal Marginal Relevance), optionally with at most ``max_per_group`` items of
one group.  ``lambda_ = 1`` without a cap is the index's own top-k.

    mmr = MMR(BruteForce(k=10), lambda_=0.7, pool=4, max_per_group=2).index_from_trainer(trainer, groups=item_groups)
"""
from __future__ import annotations

import torch

from . import ops


def _trainer_query_model(trainer, at_time):
    """The default query model of ``index_from_trainer``: the user tower, with the time context where the model has one."""
    if not getattr(trainer.cfg, "time_fields", ()):
        if at_time is not None:
            raise ValueError("index_from_trainer: at_time was given but the model has no time features (cfg.time_fields == ())")
        return trainer.user_embeddings
    if at_time is not None:
        at = int(at_time)

        def as_of(user_ids):
            return trainer.user_embeddings(user_ids, timestamps=torch.full((user_ids.numel(),), at, dtype=torch.int64, device=trainer.dev))
        return as_of

    def with_timestamps(queries):
        if not isinstance(queries, (tuple, list)) or len(queries) != 2:
            raise ValueError("the model has time features: a query is (user_ids, timestamps [n] int64) - or index with at_time=")
        return trainer.user_embeddings(queries[0], timestamps=queries[1])
    return with_timestamps


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

    def index_from_trainer(self, trainer, item_category_ids: torch.Tensor | None = None, at_time: int | None = None) -> "BruteForce":
        """Index the trainer's whole item corpus (``item_corpus_embeddings``); unless a query model was given, queries
        are user ids run through the user tower (``user_embeddings``).  A model with time features (cfg.time_fields): with
        ``at_time`` (whole seconds since the epoch) the queries stay plain user ids, scored "as of" that second; without it
        a query is the pair (user_ids, timestamps [n] int64)."""
        self.index(trainer.item_corpus_embeddings(item_category_ids))
        if self.query_model is None:
            self.query_model = _trainer_query_model(trainer, at_time)
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


class IVF(BruteForce):
    """Inverted-file approximate top-k index (``tfrs.layers.factorized_top_k.ScaNN``'s role, without quantisation).

    ``index`` runs ``iters`` rounds of spherical k-means on a seeded sample of at most 256 * nlist items (assignment with
    ``tt_retrieval_topk_f32(sample, centroids, 1)``, each centroid the normalised mean of its members, an empty cluster
    re-seeded from the largest one with a seeded perturbation), then places every item in the list of its best centroid
    (ties to the lower list) and reorders the corpus list by list, items in ascending row order within a list.  The build
    is deterministic: the same corpus, nlist and seed give bit-identical arrays (stable sorts and f64 prefix sums, no
    atomics).  A query scans the ``nprobe`` lists whose centroids score highest for it."""

    def __init__(self, query_model=None, k: int = 10, nlist: int = 1024, nprobe: int = 32, seed: int = 0, iters: int = 10):
        super().__init__(query_model, k)
        self.nlist, self.nprobe, self.seed, self.iters = int(nlist), int(nprobe), int(seed), int(iters)
        if self.nlist < 1:
            raise ValueError(f"IVF: nlist must be positive, got {self.nlist}")
        if not 1 <= self.nprobe <= min(ops.TOPK_MAX_K, self.nlist):
            raise ValueError(f"IVF: nprobe = {self.nprobe} must be in [1, min({ops.TOPK_MAX_K}, nlist = {self.nlist})]")
        if self.iters < 0:
            raise ValueError(f"IVF: iters must be >= 0, got {self.iters}")
        self.centroids = self.list_offsets = self.list_vectors = self.list_ids = None

    # ------------------------------------------------------------------ build
    @staticmethod
    def _assign(x: torch.Tensor, centroids: torch.Tensor, batch: int = 1 << 20) -> torch.Tensor:
        """Best centroid of every row (int64 [n]; ties to the lower list), in batches of rows."""
        out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
        ws = None
        for s in range(0, x.shape[0], batch):
            xb = x[s:s + batch]
            n = max(ops.retrieval_topk_workspace_bytes(xb.shape[0], centroids.shape[0], x.shape[1], 1), 1)
            if ws is None or ws.numel() < n:
                ws = torch.empty(n, dtype=torch.uint8, device=x.device)
            out[s:s + xb.shape[0]] = ops.retrieval_topk(xb, centroids, 1, workspace=ws)[1][:, 0]
        return out

    @staticmethod
    def _segment_sums(x: torch.Tensor, assign: torch.Tensor, nlist: int):
        """(f64 member sums [nlist, D], counts int64 [nlist]) by a stable sort and f64 prefix sums (deterministic)."""
        order = torch.argsort(assign, stable=True)
        counts = torch.bincount(assign, minlength=nlist)
        ends = torch.cumsum(counts, 0)
        # prefix sums along the rows of the transposed members (an inner-dimension scan: fast, and no atomics)
        xt = x[order].to(torch.float64).T.contiguous()
        csum = torch.cat([xt.new_zeros(x.shape[1], 1), torch.cumsum(xt, 1)], 1)
        return (csum[:, ends] - csum[:, ends - counts]).T, counts

    def _build_lists(self, candidates: torch.Tensor, identifiers):
        """The list build both IVF classes share: (x f32 [n, D] contiguous, order int64 [n] - the original row of every
        reordered row -, identifiers int64 or None); sets ``centroids``, ``list_offsets`` and ``list_ids``."""
        what = type(self).__name__
        if candidates.dim() != 2:
            raise ValueError(f"{what}.index: candidates must be [n, D], got shape {tuple(candidates.shape)}")
        x = candidates.detach().to(torch.float32).contiguous()
        n, d = x.shape
        if n < self.nlist:
            raise ValueError(f"{what}.index: nlist = {self.nlist} exceeds the {n} candidates")
        dev = x.device
        g = torch.Generator(device=dev).manual_seed(self.seed)
        m = min(n, 256 * self.nlist)
        sample = x[torch.sort(torch.randperm(n, device=dev, generator=g)[:m]).values].contiguous()
        cent = torch.nn.functional.normalize(sample[torch.randperm(m, device=dev, generator=g)[:self.nlist]], dim=1)
        for _ in range(self.iters):
            sums, counts = self._segment_sums(sample, self._assign(sample, cent.contiguous()), self.nlist)
            norms = sums.norm(dim=1)
            new = (sums / norms.clamp(min=1e-300)[:, None]).to(torch.float32)
            empty = torch.nonzero((counts == 0) | (norms == 0)).flatten().tolist()
            if empty:                                       # re-seed from the largest cluster, perturbed (seeded)
                big = int(torch.argmax(counts))
                noise = torch.randn(len(empty), d, device=dev, generator=g, dtype=torch.float32)
                new[empty] = new[big][None] + 0.05 * noise
            cent = torch.nn.functional.normalize(new, dim=1)
        cent = cent.contiguous()
        assign = self._assign(x, cent)
        order = torch.argsort(assign, stable=True)
        counts = torch.bincount(assign, minlength=self.nlist)
        self.centroids = cent
        self.list_offsets = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).contiguous()
        self.list_ids = order.to(torch.int32).contiguous()
        if identifiers is not None:
            ids = torch.as_tensor(identifiers, device=dev)
            if ids.dim() != 1 or ids.numel() != n:
                raise ValueError(f"{what}.index: identifiers must be [{n}], got {tuple(ids.shape)}")
            if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
                raise TypeError(f"{what}.index: identifiers must be integers, got {ids.dtype}")
            identifiers = ids.to(torch.int64).contiguous()
        return x, order, identifiers

    def index(self, candidates: torch.Tensor, identifiers=None) -> "IVF":
        """candidates: [n, D] f32 device tensor (n >= nlist).  identifiers: as ``BruteForce.index``."""
        x, order, identifiers = self._build_lists(candidates, identifiers)
        self.list_vectors = x[order].contiguous()
        self._candidates = self.list_vectors                # shape / device of the corpus for the base class
        self._identifiers = identifiers
        return self

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        if self.centroids is None:
            raise RuntimeError("IVF: call index() or index_from_trainer() first")
        return {"nlist": self.nlist, "centroids": self.centroids, "list_offsets": self.list_offsets,
                "list_vectors": self.list_vectors, "list_ids": self.list_ids}

    def load_state_dict(self, state: dict) -> "IVF":
        cent = state["centroids"]
        nlist = int(state["nlist"])
        if cent.dim() != 2 or cent.shape[0] != nlist or state["list_offsets"].numel() != nlist + 1:
            raise ValueError(f"IVF.load_state_dict: arrays do not match nlist = {nlist}")
        if self.nprobe > nlist:
            raise ValueError(f"IVF.load_state_dict: nprobe = {self.nprobe} exceeds the index's nlist = {nlist}")
        self.nlist = nlist
        self.centroids = cent.to(torch.float32).contiguous()
        self.list_offsets = state["list_offsets"].to(torch.int64).contiguous()
        self.list_vectors = state["list_vectors"].to(torch.float32).contiguous()
        self.list_ids = state["list_ids"].to(torch.int32).contiguous()
        if self.list_ids.numel() != self.list_vectors.shape[0] or self.centroids.shape[1] != self.list_vectors.shape[1]:
            raise ValueError("IVF.load_state_dict: list_ids / list_vectors / centroids shapes disagree")
        ops.check_list_offsets(self.list_offsets, self.list_vectors.shape[0], "IVF.load_state_dict")
        self._candidates = self.list_vectors
        self._identifiers = None
        self._ws = None
        return self

    # ------------------------------------------------------------------ query
    def _workspace(self, nq: int, k: int) -> torch.Tensor:
        v = self.list_vectors
        n = max(ops.ivf_search_workspace_bytes(nq, self.nlist, v.shape[0], v.shape[1], k, self.nprobe), 1)
        if self._ws is None or self._ws.numel() < n:
            self._ws = None
            self._ws = torch.empty(n, dtype=torch.uint8, device=v.device)
        return self._ws

    def _query(self, queries, exclusions, k):
        if self.centroids is None:
            raise RuntimeError("IVF: call index() or index_from_trainer() first")
        q = self.query_model(queries) if self.query_model is not None else queries
        q = q.to(torch.float32).contiguous()
        if q.dim() == 1:
            q = q[None]
        k = self.k if k is None else int(k)
        scores, idx = ops.ivf_search(q, self.centroids, self.list_offsets, self.list_vectors, self.list_ids, k, self.nprobe,
                                     exclusions=exclusions, workspace=self._workspace(q.shape[0], k), check_offsets=False)
        if self._identifiers is None:
            return scores, idx
        ids = self._identifiers[idx.clamp(min=0)]
        return scores, torch.where(idx >= 0, ids, torch.full_like(ids, -1))


class Int8BruteForce(BruteForce):
    """Quantised exhaustive top-k index: the corpus is held as per-row symmetric int8 codes and f32 scales
    (``ops.quantize_rows_i8``), every query is quantised the same way inside the scan, and the k1 = min(TOPK_MAX_K, n,
    max(rerank * k, 32)) best candidates by quantised score are re-scored against the f32 rows (``keep_f32=True``): the
    returned scores are then exactly ``BruteForce``'s for the returned items, and the answer differs only where a true
    top-k item fell outside the k1 candidates.  ``keep_f32=False`` drops the f32 rows: no re-rank, k1 = k, scores are the
    dequantised products.  Exclusions and identifiers as ``BruteForce``."""

    def __init__(self, query_model=None, k: int = 10, rerank: int = 4, keep_f32: bool = True):
        super().__init__(query_model, k)
        self.rerank, self.keep_f32 = int(rerank), bool(keep_f32)
        if self.rerank < 1:
            raise ValueError(f"Int8BruteForce: rerank must be >= 1, got {self.rerank}")
        self.codes = self.scales = None

    def index(self, candidates: torch.Tensor, identifiers=None) -> "Int8BruteForce":
        """candidates: [n, D] f32 device tensor, D in {32, 64, 128, 256}.  identifiers: as ``BruteForce.index``."""
        super().index(candidates, identifiers)
        self.codes, self.scales = ops.quantize_rows_i8(self._candidates)
        if not self.keep_f32:
            self._candidates = None
        self._ws = None
        return self

    def k1(self, k: int) -> int:
        """Stage-1 candidates per query for a top-k request."""
        return ops.default_k1(k, self.codes.shape[0], self.keep_f32, self.rerank)

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        if self.codes is None:
            raise RuntimeError("Int8BruteForce: call index() or index_from_trainer() first")
        state = {"codes": self.codes, "scales": self.scales}
        if self.keep_f32:
            state["candidates"] = self._candidates
        return state

    def load_state_dict(self, state: dict) -> "Int8BruteForce":
        codes, scales = state["codes"], state["scales"]
        if codes.dim() != 2 or codes.dtype != torch.int8 or scales.dim() != 1 or scales.numel() != codes.shape[0]:
            raise ValueError("Int8BruteForce.load_state_dict: codes must be int8 [n, D] and scales [n]")
        cand = state.get("candidates")
        if self.keep_f32:
            if cand is None:
                raise ValueError("Int8BruteForce.load_state_dict: keep_f32=True needs the state's f32 'candidates'")
            if tuple(cand.shape) != tuple(codes.shape):
                raise ValueError(f"Int8BruteForce.load_state_dict: candidates {tuple(cand.shape)} do not match codes "
                                 f"{tuple(codes.shape)}")
            self._candidates = cand.to(torch.float32).contiguous()
        else:
            self._candidates = None
        self.codes = codes.contiguous()
        self.scales = scales.to(torch.float32).contiguous()
        self._identifiers = None
        self._ws = None
        return self

    # ------------------------------------------------------------------ query
    def _workspace(self, nq: int, k: int) -> torch.Tensor:
        n, d = self.codes.shape
        need = max(ops.retrieval_topk_i8_workspace_bytes(nq, n, d, k, self.k1(k)), 1)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.codes.device)
        return self._ws

    def _query(self, queries, exclusions, k):
        if self.codes is None:
            raise RuntimeError("Int8BruteForce: call index() or index_from_trainer() first")
        q = self.query_model(queries) if self.query_model is not None else queries
        q = q.to(torch.float32).contiguous()
        if q.dim() == 1:
            q = q[None]
        k = self.k if k is None else int(k)
        scores, idx = ops.retrieval_topk_i8(q, self.codes, self.scales, k, c=self._candidates, k1=self.k1(k),
                                            exclusions=exclusions, workspace=self._workspace(q.shape[0], k))
        if self._identifiers is None:
            return scores, idx
        ids = self._identifiers[idx.clamp(min=0)]
        return scores, torch.where(idx >= 0, ids, torch.full_like(ids, -1))


class Int8IVF(IVF):
    """Quantised inverted-file index: ``IVF``'s lists (with equal arguments, bit-identical ``centroids``, ``list_offsets`` and
    ``list_ids``) held as ``Int8BruteForce``'s per-row int8 codes and f32 scales in list order (``list_codes``,
    ``list_scales``; ``list_vectors`` is None).  A query scans the int8 rows of its ``nprobe`` lists (one
    ``tt_ivf_search_i8_f32`` per call), keeps the k1 = min(TOPK_MAX_K, n, max(rerank * k, 32)) best by quantised score and,
    with ``keep_f32=True``, re-scores them against the f32 corpus, which is kept in ORIGINAL order (the re-rank gathers by
    item id): the returned scores are then exactly ``BruteForce``'s for the returned items.  ``keep_f32=False`` drops the
    f32 rows: no re-rank, k1 = k, scores are the dequantised products.  The answer is ``Int8BruteForce``'s over the items
    of the probed lists; with ``nprobe = nlist`` the two agree bit for bit.

    Index size: n (D + 8) bytes (codes, scales, ids) plus the centroids, plus 4 n D bytes with the re-rank.
    Identifiers and exclusions as ``BruteForce`` (exclusions hold original row indices)."""

    QUANT_BATCH = 1 << 20                    # reordered f32 rows alive at a time during the build

    def __init__(self, query_model=None, k: int = 10, nlist: int = 1024, nprobe: int = 32, seed: int = 0, iters: int = 10,
                 rerank: int = 4, keep_f32: bool = True):
        super().__init__(query_model, k, nlist, nprobe, seed, iters)
        self.rerank, self.keep_f32 = int(rerank), bool(keep_f32)
        if self.rerank < 1:
            raise ValueError(f"Int8IVF: rerank must be >= 1, got {self.rerank}")
        self.list_codes = self.list_scales = None

    def index(self, candidates: torch.Tensor, identifiers=None) -> "Int8IVF":
        """candidates: [n, D] f32 device tensor (n >= nlist, D in {32, 64, 128, 256}).  identifiers: as
        ``BruteForce.index``."""
        if candidates.dim() == 2 and candidates.shape[1] not in (32, 64, 128, 256):
            raise ValueError(f"Int8IVF.index: dim = {candidates.shape[1]} must be one of 32, 64, 128, 256")
        x, order, identifiers = self._build_lists(candidates, identifiers)
        n, d = x.shape
        codes = torch.empty(n, d, dtype=torch.int8, device=x.device)
        scales = torch.empty(n, dtype=torch.float32, device=x.device)
        for s in range(0, n, self.QUANT_BATCH):                 # the quantiser is per row: batches change nothing
            e = min(n, s + self.QUANT_BATCH)
            ops.quantize_rows_i8(x[order[s:e]], out=(codes[s:e], scales[s:e]))
        self.list_codes, self.list_scales, self.list_vectors = codes, scales, None
        self._candidates = x if self.keep_f32 else None         # ORIGINAL order: the re-rank gathers by item id
        self._identifiers = identifiers
        self._ws = None
        return self

    def k1(self, k: int) -> int:
        """Stage-1 candidates per query for a top-k request."""
        return ops.default_k1(k, self.list_codes.shape[0], self.keep_f32, self.rerank)

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        if self.centroids is None:
            raise RuntimeError("Int8IVF: call index() or index_from_trainer() first")
        state = {"nlist": self.nlist, "centroids": self.centroids, "list_offsets": self.list_offsets,
                 "list_codes": self.list_codes, "list_scales": self.list_scales, "list_ids": self.list_ids}
        if self.keep_f32:
            state["candidates"] = self._candidates
        return state

    def load_state_dict(self, state: dict) -> "Int8IVF":
        cent, codes, scales = state["centroids"], state["list_codes"], state["list_scales"]
        nlist = int(state["nlist"])
        if cent.dim() != 2 or cent.shape[0] != nlist or state["list_offsets"].numel() != nlist + 1:
            raise ValueError(f"Int8IVF.load_state_dict: arrays do not match nlist = {nlist}")
        if self.nprobe > nlist:
            raise ValueError(f"Int8IVF.load_state_dict: nprobe = {self.nprobe} exceeds the index's nlist = {nlist}")
        if codes.dim() != 2 or codes.dtype != torch.int8 or scales.dim() != 1 or scales.numel() != codes.shape[0]:
            raise ValueError("Int8IVF.load_state_dict: list_codes must be int8 [n, D] and list_scales [n]")
        if state["list_ids"].numel() != codes.shape[0] or cent.shape[1] != codes.shape[1]:
            raise ValueError("Int8IVF.load_state_dict: list_ids / list_codes / centroids shapes disagree")
        cand = state.get("candidates")
        if self.keep_f32:
            if cand is None:
                raise ValueError("Int8IVF.load_state_dict: keep_f32=True needs the state's f32 'candidates'")
            if tuple(cand.shape) != tuple(codes.shape):
                raise ValueError(f"Int8IVF.load_state_dict: candidates {tuple(cand.shape)} do not match list_codes "
                                 f"{tuple(codes.shape)}")
        list_offsets = state["list_offsets"].to(torch.int64).contiguous()
        ops.check_list_offsets(list_offsets, codes.shape[0], "Int8IVF.load_state_dict")
        self.nlist = nlist
        self.centroids = cent.to(torch.float32).contiguous()
        self.list_offsets = list_offsets
        self.list_codes = codes.contiguous()
        self.list_scales = scales.to(torch.float32).contiguous()
        self.list_ids = state["list_ids"].to(torch.int32).contiguous()
        self.list_vectors = None
        self._candidates = cand.to(torch.float32).contiguous() if self.keep_f32 else None
        self._identifiers = None
        self._ws = None
        return self

    # ------------------------------------------------------------------ query
    def _workspace(self, nq: int, k: int) -> torch.Tensor:
        n, d = self.list_codes.shape
        need = max(ops.ivf_search_i8_workspace_bytes(nq, self.nlist, n, d, k, self.k1(k), self.nprobe), 1)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.list_codes.device)
        return self._ws

    def _query(self, queries, exclusions, k):
        if self.centroids is None:
            raise RuntimeError("Int8IVF: call index() or index_from_trainer() first")
        q = self.query_model(queries) if self.query_model is not None else queries
        q = q.to(torch.float32).contiguous()
        if q.dim() == 1:
            q = q[None]
        k = self.k if k is None else int(k)
        scores, idx = ops.ivf_search_i8(q, self.centroids, self.list_offsets, self.list_codes, self.list_scales, self.list_ids,
                                        k, self.nprobe, c=self._candidates, k1=self.k1(k), exclusions=exclusions,
                                        workspace=self._workspace(q.shape[0], k), check_offsets=False)
        if self._identifiers is None:
            return scores, idx
        ids = self._identifiers[idx.clamp(min=0)]
        return scores, torch.where(idx >= 0, ids, torch.full_like(ids, -1))


class MMR:
    """Diversified re-ranking (Maximal Marginal Relevance, ``ops.mmr_rerank``) over any of the indices above.

    ``index``: a ``BruteForce`` / ``IVF`` / ``Int8BruteForce`` / ``Int8IVF`` (its ``k`` is the default number of results and its
    query model is used).  ``lambda_`` in [0, 1]: 1 = relevance only, 0 = diversity only.  ``pool``: the candidates asked of
    the index, as a multiple of k (``ops.default_k1``: at least 32, at most ``TOPK_MAX_K`` and the corpus).
    ``max_per_group``: at most that many results share a group id (0: no cap; needs ``groups`` when indexing).

    The wrapper keeps the f32 corpus in ORIGINAL row order (the index's own copy where it has one in that order) and the
    identifiers; the inner index is built without identifiers, so what it returns are corpus rows."""

    def __init__(self, index, lambda_: float = 0.7, pool: int = 4, max_per_group: int = 0):
        self.inner = index
        self.lambda_, self.pool, self.max_per_group = float(lambda_), int(pool), int(max_per_group)
        if not 0.0 <= self.lambda_ <= 1.0:
            raise ValueError(f"MMR: lambda_ = {lambda_} must be in [0, 1]")
        if self.pool < 1:
            raise ValueError(f"MMR: pool must be >= 1, got {self.pool}")
        if self.max_per_group < 0:
            raise ValueError(f"MMR: max_per_group must be >= 0, got {self.max_per_group}")
        self._corpus = self._identifiers = self._groups = None

    @property
    def k(self) -> int:
        return self.inner.k

    def _set_groups(self, groups, n: int, device):
        if groups is not None:
            g = torch.as_tensor(groups, device=device)
            if g.dim() != 1 or g.numel() != n:
                raise ValueError(f"MMR.index: groups must be [{n}], got {tuple(g.shape)}")
            if g.is_floating_point() or g.is_complex() or g.dtype == torch.bool:
                raise TypeError(f"MMR.index: groups must be integers, got {g.dtype}")
            groups = g.to(torch.int32).contiguous()
        elif self.max_per_group > 0:
            raise ValueError(f"MMR.index: max_per_group = {self.max_per_group} needs groups")
        self._groups = groups

    def index(self, candidates: torch.Tensor, identifiers=None, groups=None) -> "MMR":
        """candidates, identifiers: as ``BruteForce.index``.  groups: optional [n] integer tensor, the group id of every
        candidate (-1: never capped)."""
        if candidates.dim() != 2:
            raise ValueError(f"MMR.index: candidates must be [n, D], got shape {tuple(candidates.shape)}")
        x = candidates.detach().to(torch.float32).contiguous()
        n = x.shape[0]
        if identifiers is not None:
            ids = torch.as_tensor(identifiers, device=x.device)
            if ids.dim() != 1 or ids.numel() != n:
                raise ValueError(f"MMR.index: identifiers must be [{n}], got {tuple(ids.shape)}")
            if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
                raise TypeError(f"MMR.index: identifiers must be integers, got {ids.dtype}")
            identifiers = ids.to(torch.int64).contiguous()
        self._set_groups(groups, n, x.device)
        self.inner.index(x)                                  # no identifiers: the index answers corpus rows
        self._corpus, self._identifiers = x, identifiers
        return self

    def index_from_trainer(self, trainer, item_category_ids: torch.Tensor | None = None, at_time: int | None = None,
                           groups=None) -> "MMR":
        """As ``BruteForce.index_from_trainer``; ``groups`` as in ``index``."""
        self.index(trainer.item_corpus_embeddings(item_category_ids), groups=groups)
        if self.inner.query_model is None:
            self.inner.query_model = _trainer_query_model(trainer, at_time)
        return self

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        """The inner index's state (plus ``groups`` where there are any)."""
        if not hasattr(self.inner, "state_dict"):
            raise RuntimeError(f"MMR: {type(self.inner).__name__} has no state to save; index() it again instead")
        state = dict(self.inner.state_dict())
        if self._groups is not None:
            state["groups"] = self._groups
        return state

    def load_state_dict(self, state: dict) -> "MMR":
        if not hasattr(self.inner, "load_state_dict"):
            raise RuntimeError(f"MMR: {type(self.inner).__name__} has no state to load; index() it instead")
        inner = self.inner.load_state_dict(state)
        if getattr(inner, "list_vectors", None) is not None:     # IVF keeps its rows list by list: back to original order
            corpus = torch.empty_like(inner.list_vectors)
            corpus[inner.list_ids.to(torch.int64)] = inner.list_vectors
        elif inner._candidates is not None:
            corpus = inner._candidates
        else:
            raise ValueError("MMR.load_state_dict: the state holds no f32 corpus (an int8 index saved with keep_f32=False)")
        self._set_groups(state.get("groups"), corpus.shape[0], corpus.device)
        self._corpus, self._identifiers = corpus, None
        return self

    # ------------------------------------------------------------------ query
    def _query(self, queries, exclusions, k):
        if self._corpus is None:
            raise RuntimeError("MMR: call index() or index_from_trainer() first")
        k = self.inner.k if k is None else int(k)
        n = self._corpus.shape[0]
        if not 1 <= k <= min(ops.TOPK_MAX_K, n):
            raise ValueError(f"MMR: k = {k} must be in [1, min({ops.TOPK_MAX_K}, n = {n})]")
        k1 = ops.default_k1(k, n, True, self.pool)
        scores, idx = self.inner._query(queries, exclusions, k1)
        scores, idx = ops.mmr_rerank(scores, idx, self._corpus, k, self.lambda_, groups=self._groups,
                                     max_per_group=self.max_per_group)
        if self._identifiers is None:
            return scores, idx
        ids = self._identifiers[idx.clamp(min=0)]
        return scores, torch.where(idx >= 0, ids, torch.full_like(ids, -1))

    def __call__(self, queries, k: int | None = None):
        """(scores f32 [nq, k], identifiers or indices int64 [nq, k]) in the diversified order; the scores are the index's
        own, so they need not descend.  When the pool runs out (exclusions, caps) the tail is (-inf, -1)."""
        return self._query(queries, None, k)

    def query_with_exclusions(self, queries, exclusions, k: int | None = None):
        """As ``__call__``, never returning an excluded candidate (``exclusions`` as ``BruteForce.query_with_exclusions``)."""
        return self._query(queries, exclusions, k)
