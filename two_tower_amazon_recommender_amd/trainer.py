"""Single-GPU train step of the two-tower retrieval model: the whole hot path on HIP kernels.

This is the explicit (no autograd) engine that ``train.py`` and ``bench.py`` drive:

    ids ──► tower fwd, the embedding lookup fused into its input tile (both layers of both towers: 1 launch)
        ──► fused scorer + softmax loss (pass 1: loss + dq, combine, pass 2: dc, slab reduction: 4 launches)
        ──► tower bwd (dx + dw + db per layer: 2 launches)
        ──► optimizer (sort of the ids, duplicate sums, sparse SGD/Adagrad of all tables, dense update: 1 launch;
                       lazy Adam: sort plan + two launches, ``ops.adam_step_``; row-wise Adagrad: sort plan + two
                       launches, ``ops.rowwise_adagrad_step_``)

All buffers are allocated once for a fixed batch size; ``step`` enqueues those 8 launches (cfg3; one more per extra tower
layer) through ONE C call (``tt_train_step_f32``) on the current stream and never synchronises (it can be captured in a
HIP graph).

Reference anchors: hyper-parameters are the ``model:`` block of
``/root/reference/configs/data_config.yaml:54-71`` (embedding_dim, *_tower_dims, l2_regularization,
training.learning_rate, retrieval.temperature, candidate_sampling "in_batch"); inputs are the int64
``user_idx`` / ``item_idx`` columns of ``prepare_training_data.py:209-210``.  The reference never
implemented the step itself (``src/training/__init__.py:1``).
"""
from __future__ import annotations

import functools
import math
import os
from dataclasses import dataclass, field

import torch

from . import _lib, ops

# tensor-id convention of the synthetic initialiser (must match oracle/synth.py, which restates it
# for the tests; the product does not import the oracle)
TID_USER_TABLE, TID_ITEM_TABLE, TID_USER_IDS, TID_ITEM_IDS = 1, 2, 3, 4
TID_CATEGORY_TABLE, TID_CATEGORY_IDS = 5, 6
TID_TITLE_TABLE, TID_TITLE_IDS, TID_TITLE_LENGTHS = 7, 8, 9
TID_HISTORY_TABLE = 11
TID_USER_FEATURE_PROJ, TID_ITEM_FEATURE_PROJ = 12, 13       # the projection kernels of the numeric side features
TID_USER_FEATURES, TID_ITEM_FEATURES = 14, 15               # synthetic_user_features / synthetic_item_features
TID_SAMPLED_NEGATIVES = 10               # candidate_sampling="mixed": draw i of step s is element s * n_sampled_negatives + i
TID_DENSE_BASE = 16
TID_RATING_W1, TID_RATING_W2 = 40, 41        # the rating head's two kernels (between the Dense kernels' 16..31 and the dropout streams)
TID_GRU_BASE = 42                            # the history GRU: the input kernel W is 42, the recurrent kernel U 43
TID_SELF_ATTENTION_BASE = 44                 # the history self-attention: Wqk is 44, Wvo 45
TID_CROSS_BASE = 48                          # the cross kernels: layer l of tower t is 48 + 2 l + t (48..53)
TID_FREQ_HASH_BASE = 56                      # the streaming frequency estimator's hash rows: row h is 56 + h (56..59)
TID_TIME_BASE = 60                           # the time-of-interaction context: the table is 60, synthetic_timestamps 61
TIME_MISSING = ops.TIME_MISSING              # a pair without a timestamp
MAX_CROSS_LAYERS = 3
# poolings of the user-history feature: the bag launch's three, the attention pool (csrc/history_attn.hip) and the GRU encoder
# (csrc/history_gru.hip), history only
HISTORY_POOLINGS = tuple(ops.POOLINGS) + ("attention", "gru")
# every encoder history_pooling takes: the poolings and the multi-head self-attention block (csrc/history_selfattn.hip)
HISTORY_ENCODERS = HISTORY_POOLINGS + ("self_attention",)
LR_DECAYS = ("none", "cosine", "linear", "inverse_sqrt")
SAMPLING_BIAS_ESTIMATORS = ("none", "streaming")
RETRIEVAL_LOSSES = ("softmax", "bpr", "hinge")
PAIRWISE_KIND_OF_LOSS = {"bpr": "logistic", "hinge": "hinge"}     # retrieval_loss -> the kernel family's kind
TID_DROPOUT_BASE = 64


@dataclass
class TwoTowerConfig:
    n_users: int
    n_items: int
    embedding_dim: int = 128                       # configs/data_config.yaml:55
    tower_dims: list = field(default_factory=lambda: [512, 256, 128])   # :56 user_tower_dims (and the item tower's if below is None)
    item_tower_dims: list | None = None            # :57 item_tower_dims; None = same as tower_dims
    temperature: float = 0.1                       # :70
    l2_regularization: float = 1e-6                # :59
    learning_rate: float = 0.001                   # :63
    optimizer: str = "sgd"                         # unspecified by the reference; north_star: SGD / Adagrad; "adam" = lazy Adam
    adagrad_initial_accumulator: float = 0.1       # Keras 2.15 default
    adagrad_epsilon: float = 1e-7                  # Keras 2.15 default
    # optimizer="rowwise_adagrad": FBGEMM / TorchRec's exact row-wise Adagrad on the embedding tables - ONE accumulator float per
    # row, fed with the mean of the row's squared gradient (rows floats of state instead of rows x dim) - and the element-wise
    # Adagrad above on the dense parameters; both adagrad_* settings apply (epsilon inside the root, as "adagrad")
    # optimizer="adam": lazy Adam (TF-Addons LazyAdam / torch.optim.SparseAdam) - only the rows of the batch's ids are touched,
    # the bias correction comes from the global step; Keras 2.15 Adam's defaults (its learning_rate default is :63's 0.001)
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-7
    # global-norm gradient clipping (Keras optimizers' global_clipnorm=, tf.clip_by_global_norm): every gradient of the step -
    # dense parameters and the embedding tables' per-occurrence rows (IndexedSlices.values: duplicates not merged) - is scaled by
    # c / max(norm, c) between the backward pass and the optimizer, in two launches (csrc/clip.hip).  The l2 term, which the
    # optimizer kernels add, is neither counted nor scaled.  0 = off.  Single-GPU trainer, Python sequence of launches, no graph
    # capture.
    global_clipnorm: float = 0.0
    # learning-rate schedule (Keras LearningRateSchedule; a host function, ``learning_rate_at``): learning_rate is the PEAK, reached
    # after lr_warmup_steps linear warm-up steps; then lr_decay "none" | "cosine" | "linear" (over lr_decay_steps steps, down to
    # lr_min_ratio * peak, constant from there) | "inverse_sqrt" (peak * sqrt(max(warmup, 1) / (step + 1)), not below the floor).
    lr_warmup_steps: int = 0
    lr_decay: str = "none"
    lr_decay_steps: int = 0
    lr_min_ratio: float = 0.0
    batch_size: int = 1024                         # :62
    dropout_rate: float = 0.0                      # :58 is 0.1; parity/bench runs use 0
    # BASELINE configs[4] "30 categories as hash features": a [n_category_buckets, embedding_dim] table whose row
    # (bucket of the pair's hashed category) is ADDED to the item embedding before the item tower.  0 = no such feature.
    n_category_buckets: int = 0
    # matrix products of the scorer + softmax loss: "f32" (exact f32 products on the f32-input MFMA: the parity-safe default
    # and the headline) or "bf16x3" (f32-emulated through a three-way bf16 split on the bf16 MFMA; scorer dim 128 / 256)
    scorer_precision: str = "f32"
    # the retrieval loss over the step's candidates: "softmax" (the in-batch sampled softmax of tfrs.tasks.Retrieval, the default),
    # "bpr" (pairwise logistic: softplus(s_neg - s_pos) over a query's negatives, Rendle 2009) or "hinge" (pairwise hinge:
    # max(0, pairwise_margin - (s_pos - s_neg))), on the same logits - temperature, logQ correction, accidental hits removed
    # (csrc/pairwise.hip).  pairwise_reduction "mean": every query's sum is divided by ITS number of negatives, so a margin and a
    # learning rate keep their meaning when the batch size changes; "sum": the plain sum over the pairs.  Exact f32 only;
    # single-GPU trainer, Python sequence of launches, no graph capture.
    retrieval_loss: str = "softmax"
    pairwise_margin: float = 1.0
    pairwise_reduction: str = "mean"
    # cosine scoring: both towers' outputs are L2-normalised (tf.math.l2_normalize: x / sqrt(max(sum x^2, normalize_eps))) before
    # the scorer, every metric and every embedding the trainer hands out - what the reference's temperature 0.1 is meant for
    # (Yi et al. 2019; SURVEY.md lists the choice as left open).  Off = the towers' raw outputs, as before.
    normalize_embeddings: bool = False
    normalize_eps: float = 1e-12                   # tf.math.l2_normalize's default (a floor of the SUM OF SQUARES)
    # retrieval.candidate_sampling of the reference's schema: "in_batch" (every other pair's item is a negative) or "mixed" - mixed
    # negative sampling (Yang et al. 2020): every step appends n_sampled_negatives items drawn from the whole corpus to the
    # batch's candidates, by the "uniform" sampler or the "unigram" one (word2vec's f^unigram_power of the item frequencies,
    # ``set_item_frequencies``).  Single-GPU trainer, Python sequence of launches, no graph capture.
    candidate_sampling: str = "in_batch"
    n_sampled_negatives: int = 0
    negative_sampler: str = "uniform"
    unigram_power: float = 0.75
    # where the logQ correction's probabilities come from.  "none": from the caller (candidate_sampling_probability / mixed:
    # ``set_item_frequencies``), as before.  "streaming": from the streaming frequency estimator of Yi et al. 2019 (csrc/freq.hip) -
    # a sketch of freq_hashes hash rows x freq_slots slots (0: min(2 * n_items, 2^25)) of "steps since this item was last a
    # positive", updated by every train batch with the moving-average coefficient freq_alpha; the trainer then applies the
    # correction by itself, in-batch and mixed.  Single-GPU trainer, no graph capture.
    sampling_bias_estimator: str = "none"
    freq_alpha: float = 0.01
    freq_hashes: int = 2
    freq_slots: int = 0
    # time-of-interaction context features (the reference's create_temporal_features; TFRS's context-feature recipe: timestamp ->
    # Discretization -> Embedding and the calendar fields in the query model): every pair carries its int64 timestamp (whole seconds
    # since the Unix epoch, UTC; TIME_MISSING: none) and the rows it picks in ONE trained table - 24 hours, 7 days of the week
    # (Monday 0), 12 months, time_buckets equal periods of [time_min, time_max] (the training split's range; later pairs land in
    # the last bucket, as Keras Discretization does) - are ADDED to the user tower's input.  time_fields: a subset of ("hour",
    # "day_of_week", "month", "period"), kept in that order; () = no such feature.  The table is a DENSE parameter (a full batch
    # hits every row; csrc/time_context.hip): no l2; under optimizer="adam" it takes the dense Adam of the other dense parameters -
    # Keras's non-lazy Adam on an Embedding, not LazyAdam -, and global_clipnorm counts its gradient merged over the batch (Keras
    # would count IndexedSlices.values per occurrence).  Single-GPU trainer, materialised tower inputs, no graph capture.
    time_fields: tuple = ()
    time_buckets: int = 0
    time_min: int = 0
    time_max: int = 0
    # heads of history_pooling "self_attention" (1, 2, 4 or 8; described with the history feature below)
    history_heads: int = 1
    # rating-prediction head (tfrs.tasks.Ranking beside tfrs.tasks.Retrieval): rating_weight > 0 adds one hidden ReLU layer of
    # rating_hidden units (a multiple of 32 in 32..256) over the pair's two tower outputs - the vectors the scorer reads - and a
    # scalar output trained with MSE on the interaction's rating: total = retrieval + rating_weight * L_r, L_r = mean over the
    # batch of w (pred - rating)^2 (a NaN rating: no label).  0 = no head.  Single-GPU trainer, Python sequence of launches, no
    # graph capture.
    rating_weight: float = 0.0
    rating_hidden: int = 128
    # layer normalisation of the hidden layers (Keras LayerNormalization between a hidden Dense layer and its ReLU) in BOTH towers:
    # hidden layer l becomes Dense (linear) -> LayerNorm (gamma_l, beta_l [n_l]; biased variance, layer_norm_epsilon inside the
    # square root: Keras's default 1e-3) -> ReLU -> dropout; the output layer is not normalised.  gamma starts at 1, beta at 0,
    # neither carries the l2 penalty.  Every hidden width must be a multiple of 32 in 32..1024.  Single-GPU trainer, Python
    # sequence of launches, no graph capture.
    layer_norm: bool = False
    layer_norm_epsilon: float = 1e-3
    # DCN-v2 cross layers (tfrs.layers.dcn.Cross, Wang et al. 2021) in BOTH towers, between the summed input rows x_0 and the
    # Dense stack: x_{l+1} = x_0 * (x_l W_l + b_l) + x_l, W_l [embedding_dim, embedding_dim] - explicit bilinear interactions of
    # the features summed into x_0.  0..3 layers; 0 = none.  embedding_dim must be a multiple of 32 in 32..256.  Single-GPU
    # trainer, materialised tower inputs, no graph capture.
    cross_layers: int = 0
    # dense numeric side features (the reference's create_user_features / create_item_features: per-id rating count / mean / std /
    # min / max; TFRS Normalization -> concat -> Dense): a fixed [n_users, n_user_features] / [n_items, n_item_features] f32 matrix
    # (``set_user_features`` / ``set_item_features``; 1..32 columns) whose row is normalised (Keras Normalization; clamped to
    # [-feature_clip, feature_clip] when feature_clip > 0), projected by a trained [F, embedding_dim] kernel - no bias: the first
    # Dense layer's plays that part - and ADDED to the tower's input.  0 = no such feature.  Single-GPU trainer, materialised
    # tower inputs, no graph capture.
    n_user_features: int = 0
    n_item_features: int = 0
    feature_clip: float = 0.0
    # pooled user-history feature (TFRS's context / sequential retrieval shape: Embedding over item ids ->
    # GlobalAveragePooling1D in the query model): every user carries its last user_history_len training items
    # (``set_user_histories``), their rows of a [n_items, embedding_dim] table of its own are pooled ("sum" | "mean" | "sqrtn") and
    # ADDED to the user tower's input - in the train step without the pair's own item (leave-one-out: pooled into the query it is
    # scored against, the label would leak).  0 = no such feature.  Single-GPU trainer, materialised tower inputs, no graph capture.
    # history_pooling "attention": a softmax over the kept slots of e_j = <row_j, a> / sqrt(embedding_dim) + p[recency rank of j]
    # with one trained vector [a | p] (embedding_dim + user_history_len floats, zero-initialised: a fresh model pools by the
    # mean; no l2 penalty) - the histories are stored oldest first, and the rank counts the kept slots behind j.
    # history_pooling "gru": TFRS's sequential-retrieval recipe, Embedding -> GRU(embedding_dim) - Keras GRU(reset_after=True) with
    # zero initial state stepping over the kept slots oldest first (a skipped slot carries the state, as Keras masking does); its
    # final state is added to the user tower's input.  W, U [D, 3D] (gate blocks z | r | n) are BOTH Glorot-uniform (Keras
    # initialises U orthogonally), b [2, 3D] = b_i, b_r starts at zero; none carries the l2 penalty.  embedding_dim must be a
    # multiple of 32 in 32..256.
    # history_pooling "self_attention": one SASRec-style causal self-attention block with history_heads heads (1, 2, 4 or 8), read
    # at the last position - the NEWEST kept item n is the one query: T = x_n Wqk, e_hj = <x_j, T_h> / sqrt(D) + p[h, recency rank
    # of j], w_h = softmax_j, out = user row + concat_h(sum_j w_hj x_j) Wvo.  Wqk [D, H D] holds Wq_h Wk_h^T per head as one D x D
    # form and Wvo [H D, D] holds Wv_h Wo_h (exact generalisations: every GEMM runs over batch rows, never batch * L); both are
    # Glorot-uniform, p [H, L] starts at zero; none carries the l2 penalty.  Deviations from SASRec: the block's feed-forward half
    # is the user tower's Dense stack that follows, there is no LayerNorm and no residual of x_n, and positions enter as the
    # per-head recency bias p instead of position embeddings.  embedding_dim must be a multiple of 32 in 32..256.
    user_history_len: int = 0
    history_pooling: str = "mean"
    # pooled item-title feature (the reference's preprocessing.text_fields: title; TFRS TextVectorization -> Embedding ->
    # GlobalAveragePooling1D): every item carries up to title_max_tokens hashed title tokens (``set_item_titles``), their rows
    # of a [n_title_buckets, embedding_dim] table are pooled ("sum" | "mean" | "sqrtn") and ADDED to the item tower's input.
    # 0 = no such feature.  Single-GPU trainer, materialised tower inputs, no graph capture.
    n_title_buckets: int = 0
    title_max_tokens: int = 16
    title_pooling: str = "mean"
    def __post_init__(self):
        if isinstance(self.time_fields, (list, tuple)) and all(f in ops.TIME_FIELDS for f in self.time_fields) \
                and len(set(self.time_fields)) == len(self.time_fields):
            self.time_fields = tuple(f for f in ops.TIME_FIELDS if f in self.time_fields)       # the fixed order

    @property
    def time_rows(self) -> int:
        """Rows of the time table (0: the feature is off)."""
        return ops.time_field_layout(self.time_fields, self.time_buckets)[1] if self.time_fields else 0

    @property
    def lr_schedule_on(self) -> bool:
        return self.lr_warmup_steps > 0 or self.lr_decay != "none"

    def learning_rate_at(self, step: int) -> float:
        """The rate of the step with 0-based index ``step`` (f64 arithmetic; the kernels take it rounded to f32, like a constant
        rate).  Without a schedule: learning_rate itself."""
        if self.lr_decay == "none" and self.lr_warmup_steps <= 0:        # (first: the default step reads this every time)
            return self.learning_rate
        peak, s, warm = float(self.learning_rate), int(step), int(self.lr_warmup_steps)
        if s < warm:
            return peak * (s + 1) / warm
        t, total, m = s - warm, int(self.lr_decay_steps), float(self.lr_min_ratio)
        if self.lr_decay == "cosine":
            return peak * (m + (1.0 - m) * 0.5 * (1.0 + math.cos(math.pi * min(t, total) / total)))
        if self.lr_decay == "linear":
            return peak * (m + (1.0 - m) * (1.0 - min(t, total) / total))
        if self.lr_decay == "inverse_sqrt":
            return peak * max(m, math.sqrt(max(warm, 1) / (s + 1)))
        return peak

    @property
    def freq_slot_count(self) -> int:
        """Slots per hash row of the frequency sketch: freq_slots, or min(2 * n_items, 2^25) when that is 0."""
        return int(self.freq_slots) if self.freq_slots else min(2 * int(self.n_items), 1 << 25)

    @property
    def user_dims(self) -> list:
        return list(self.tower_dims)

    @property
    def item_dims(self) -> list:
        return list(self.tower_dims if self.item_tower_dims is None else self.item_tower_dims)

    @property
    def symmetric(self) -> bool:
        return self.user_dims == self.item_dims

    @property
    def history_attention(self) -> bool:
        """The history feature is on and pooled by attention."""
        return self.user_history_len > 0 and self.history_pooling == "attention"

    @property
    def history_gru(self) -> bool:
        """The history feature is on and encoded by the GRU."""
        return self.user_history_len > 0 and self.history_pooling == "gru"

    @property
    def history_self_attention(self) -> bool:
        """The history feature is on and encoded by the multi-head self-attention block."""
        return self.user_history_len > 0 and self.history_pooling == "self_attention"

    def dense_segment_count(self, cross: bool = True, attention: bool = True, gru: bool = True, self_attention: bool = True) -> int:
        """Segments of the dense optimizer launches (``dense_layout``): a kernel and a bias per Dense layer, a projection kernel
        per side with numeric features, two for the rating head, two for the cross layers (``cross=False``: without those), one
        for the history attention's vector (``attention=False``: without it), one for the layer normalisation's gammas and betas,
        one for the time table, four for the history GRU - W, U, b_i, b_r - (``gru=False``: without those), three for the history
        self-attention - Wqk, Wvo, p - (``self_attention=False``: without those)."""
        skip = {g for g, on in (("cross", cross), ("attention", attention), ("gru", gru), ("self_attention", self_attention)) if not on}
        return sum(s.group not in skip for s in dense_layout(self).segments)

    def validate(self):
        if self.optimizer not in ("sgd", "adagrad", "adam", "rowwise_adagrad"):
            raise ValueError(f"optimizer must be 'sgd', 'adagrad', 'adam' or 'rowwise_adagrad', got {self.optimizer!r}")
        if not 0.0 <= self.adam_beta1 < 1.0:
            raise ValueError("adam_beta1 must be in [0, 1)")
        if not 0.0 <= self.adam_beta2 < 1.0:
            raise ValueError("adam_beta2 must be in [0, 1)")
        if not self.adam_epsilon > 0:
            raise ValueError("adam_epsilon must be > 0")
        if self.embedding_dim % 4 or any(d % 4 for d in self.user_dims + self.item_dims):
            raise ValueError("embedding_dim and tower dims must be multiples of 4")
        if self.user_dims[-1] != self.item_dims[-1]:
            raise ValueError("both towers must end in the same (scorer) dimension")
        if self.tower_dims[-1] not in (32, 64, 128, 256):
            raise ValueError("the last tower dim (scorer dim) must be one of 32, 64, 128, 256")
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        if self.temperature <= 0:
            raise ValueError("temperature must be positive")
        if self.n_category_buckets < 0:
            raise ValueError("n_category_buckets must be >= 0")
        if self.scorer_precision not in ops.SCORER_PRECISIONS:
            raise ValueError(f"scorer_precision must be one of {ops.SCORER_PRECISIONS}")
        if self.scorer_precision == "bf16x3" and self.tower_dims[-1] not in (128, 256):
            raise ValueError("scorer_precision='bf16x3' needs a scorer dim (last tower dim) of 128 or 256")
        if self.retrieval_loss not in RETRIEVAL_LOSSES:
            raise ValueError(f"retrieval_loss must be one of {RETRIEVAL_LOSSES}, got {self.retrieval_loss!r}")
        if isinstance(self.pairwise_margin, bool) or not isinstance(self.pairwise_margin, (int, float)) \
                or not math.isfinite(self.pairwise_margin):
            raise ValueError("pairwise_margin must be a finite number")
        if self.pairwise_reduction not in ops.PAIRWISE_REDUCTIONS:
            raise ValueError(f"pairwise_reduction must be one of {tuple(ops.PAIRWISE_REDUCTIONS)}, got {self.pairwise_reduction!r}")
        if self.retrieval_loss != "softmax" and self.scorer_precision != "f32":
            raise ValueError(f"retrieval_loss={self.retrieval_loss!r} needs scorer_precision='f32': the pairwise kernels are exact "
                             "f32 only")
        if not isinstance(self.normalize_embeddings, bool):
            raise ValueError("normalize_embeddings must be a bool")
        if not self.normalize_eps > 0:
            raise ValueError("normalize_eps must be > 0")
        if self.n_title_buckets < 0:
            raise ValueError("n_title_buckets must be >= 0")
        if not 1 <= self.title_max_tokens <= 64:
            raise ValueError("title_max_tokens must be in 1..64")
        if self.title_pooling not in ops.POOLINGS:
            raise ValueError(f"title_pooling must be one of {tuple(ops.POOLINGS)}")
        if not 0 <= self.user_history_len <= 64:
            raise ValueError("user_history_len must be 0 (no history feature) or in 1..64")
        if self.history_pooling not in HISTORY_ENCODERS:
            raise ValueError(f"history_pooling must be one of {HISTORY_ENCODERS}")
        if self.history_self_attention and not (32 <= self.embedding_dim <= 256 and self.embedding_dim % 32 == 0):
            raise ValueError("history_pooling='self_attention' needs an embedding_dim that is a multiple of 32 in 32..256 "
                             f"(got {self.embedding_dim})")
        if isinstance(self.history_heads, bool) or self.history_heads not in ops.SELF_ATTENTION_HEADS:
            raise ValueError(f"history_heads must be one of {ops.SELF_ATTENTION_HEADS}, got {self.history_heads!r}")
        if self.history_gru and not (32 <= self.embedding_dim <= 256 and self.embedding_dim % 32 == 0):
            raise ValueError(f"history_pooling='gru' needs an embedding_dim that is a multiple of 32 in 32..256 (got {self.embedding_dim})")
        if self.user_history_len and self.n_items >= 2 ** 31:
            raise ValueError("user_history_len > 0 needs n_items < 2^31: the history tokens are int32")
        if self.user_history_len and self.candidate_sampling == "mixed":
            raise ValueError("user_history_len > 0 with candidate_sampling='mixed' is not implemented: a sampled negative that "
                             "sits in the query's history is not left out")
        for name in ("n_user_features", "n_item_features"):
            f = getattr(self, name)
            if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f <= ops.MAX_DENSE_FEATURES:
                raise ValueError(f"{name} must be 0 (no numeric features) or an int in 1..{ops.MAX_DENSE_FEATURES}")
        if not isinstance(self.time_fields, tuple) or any(f not in ops.TIME_FIELDS for f in self.time_fields) \
                or len(set(self.time_fields)) != len(self.time_fields):
            raise ValueError(f"time_fields must be a tuple of distinct fields out of {ops.TIME_FIELDS}, got {self.time_fields!r}")
        tb = self.time_buckets
        if isinstance(tb, bool) or not isinstance(tb, int) or not 0 <= tb <= ops.MAX_TIME_BUCKETS:
            raise ValueError(f"time_buckets must be an int in 0..{ops.MAX_TIME_BUCKETS}")
        if ("period" in self.time_fields) != (tb > 0):
            raise ValueError("time_buckets must be >= 1 exactly when time_fields holds 'period' "
                             f"(got time_fields {self.time_fields!r}, time_buckets {tb})")
        for name in ("time_min", "time_max"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not -2 ** 63 <= v < 2 ** 63:
                raise ValueError(f"{name} must be an int64 (whole seconds since the epoch)")
        if self.time_min > self.time_max or self.time_max - self.time_min >= 2 ** 40:
            raise ValueError(f"need time_min <= time_max and time_max - time_min < 2^40 (got {self.time_min}, {self.time_max})")
        if not (self.feature_clip >= 0.0 and math.isfinite(self.feature_clip)):
            raise ValueError("feature_clip must be a finite number >= 0 (0: no clipping)")
        if self.candidate_sampling not in ("in_batch", "mixed"):
            raise ValueError(f"candidate_sampling must be 'in_batch' or 'mixed', got {self.candidate_sampling!r}")
        if self.negative_sampler not in ("uniform", "unigram"):
            raise ValueError(f"negative_sampler must be 'uniform' or 'unigram', got {self.negative_sampler!r}")
        if self.candidate_sampling == "mixed":
            if self.n_sampled_negatives < 1:
                raise ValueError("candidate_sampling='mixed' needs n_sampled_negatives >= 1")
            if self.batch_size + self.n_sampled_negatives > 65536:
                raise ValueError("batch_size + n_sampled_negatives must be <= 65536")
            if self.n_category_buckets > 0:
                raise ValueError("candidate_sampling='mixed' with n_category_buckets > 0: a sampled item has no interaction row "
                                 "to take a category from")
        elif self.n_sampled_negatives != 0:
            raise ValueError("n_sampled_negatives must be 0 with candidate_sampling='in_batch'")
        if not (self.unigram_power >= 0.0 and math.isfinite(self.unigram_power)):
            raise ValueError("unigram_power must be a finite number >= 0")
        if self.sampling_bias_estimator not in SAMPLING_BIAS_ESTIMATORS:
            raise ValueError(f"sampling_bias_estimator must be one of {SAMPLING_BIAS_ESTIMATORS}, got {self.sampling_bias_estimator!r}")
        a = self.freq_alpha
        if isinstance(a, bool) or not isinstance(a, (int, float)) or not 0.0 < a <= 1.0:
            raise ValueError("freq_alpha must be in (0, 1]")
        fh = self.freq_hashes
        if isinstance(fh, bool) or not isinstance(fh, int) or not 1 <= fh <= ops.MAX_FREQ_HASHES:
            raise ValueError(f"freq_hashes must be an int in 1..{ops.MAX_FREQ_HASHES}")
        fs = self.freq_slots
        if isinstance(fs, bool) or not isinstance(fs, int) or not 0 <= fs <= 1 << 32:
            raise ValueError("freq_slots must be an int in 1..2^32, or 0 for min(2 * n_items, 2^25)")
        if isinstance(self.rating_weight, bool) or not isinstance(self.rating_weight, (int, float)) \
                or not (self.rating_weight >= 0.0 and math.isfinite(self.rating_weight)):
            raise ValueError("rating_weight must be a finite number >= 0 (0: no rating head)")
        h = self.rating_hidden
        if isinstance(h, bool) or not isinstance(h, int) or not (32 <= h <= 256 and h % 32 == 0):
            raise ValueError("rating_hidden must be a multiple of 32 in 32..256")
        cl = self.cross_layers
        if isinstance(cl, bool) or not isinstance(cl, int) or not 0 <= cl <= MAX_CROSS_LAYERS:
            raise ValueError(f"cross_layers must be an int in 0..{MAX_CROSS_LAYERS} (0: no cross layers)")
        if cl and not (32 <= self.embedding_dim <= 256 and self.embedding_dim % 32 == 0):
            raise ValueError(f"cross_layers > 0 needs an embedding_dim that is a multiple of 32 in 32..256 (got {self.embedding_dim})")
        if not isinstance(self.layer_norm, bool):
            raise ValueError("layer_norm must be a bool")
        eps = self.layer_norm_epsilon
        if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (eps > 0 and math.isfinite(eps)):
            raise ValueError("layer_norm_epsilon must be a finite number > 0")
        if self.layer_norm:
            hidden = self.user_dims[:-1] + self.item_dims[:-1]
            if len(self.user_dims) < 2 or len(self.item_dims) < 2:
                raise ValueError("layer_norm=True needs towers with a hidden layer (the output layer is not normalised)")
            if any(n % 32 or not 32 <= n <= 1024 for n in hidden):
                raise ValueError(f"layer_norm=True needs hidden widths that are multiples of 32 in 32..1024 (got {hidden})")
        c = self.global_clipnorm
        if isinstance(c, bool) or not isinstance(c, (int, float)) or not (c >= 0.0 and math.isfinite(c)):
            raise ValueError("global_clipnorm must be a finite number >= 0 (0: no clipping)")
        for name in ("lr_warmup_steps", "lr_decay_steps"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} must be an int >= 0")
        if self.lr_decay not in LR_DECAYS:
            raise ValueError(f"lr_decay must be one of {LR_DECAYS}, got {self.lr_decay!r}")
        if self.lr_decay in ("cosine", "linear") and self.lr_decay_steps < 1:
            raise ValueError(f"lr_decay={self.lr_decay!r} needs lr_decay_steps >= 1")
        m = self.lr_min_ratio
        if isinstance(m, bool) or not isinstance(m, (int, float)) or not 0.0 <= m <= 1.0:
            raise ValueError("lr_min_ratio must be in [0, 1]")
        # the optimizer launches take TT_MAX_DENSE_SEGS segments.  Refused: a model whose optional blocks do not fit - blamed on
        # the block that holds the first segment past the limit (towers that are over it on their own: on the first optional block)
        segs = dense_layout(self).segments
        if len(segs) > _lib.TT_MAX_DENSE_SEGS and segs[-1].group != "towers":
            first = max(_lib.TT_MAX_DENSE_SEGS, sum(s.group == "towers" for s in segs))
            group = segs[first].group
            raise NotImplementedError(f"{_SEGMENT_GROUPS[group]} to the model's {[s.group for s in segs].index(group)}: the optimizer "
                                      f"launches take at most {_lib.TT_MAX_DENSE_SEGS} (use towers of at most 3 layers, or drop a feature)")


# what each optional block of ``dense_layout`` adds to the dense optimizer launches (validate's refusal)
_SEGMENT_GROUPS = {"features": "the numeric side features add one dense segment per side",
                   "head": "the rating head adds two dense segments",
                   "cross": "the cross layers add two dense segments",
                   "attention": "the history attention adds one dense segment",
                   "norm": "the layer normalisation adds one dense segment",
                   "time": "the time context table adds one dense segment",
                   "gru": "the history GRU adds four dense segments",
                   "self_attention": "the history self-attention adds three dense segments"}


@dataclass(frozen=True)
class DenseBlock:
    """One parameter of ``dense_flat``: the floats [offset, end) viewed as ``shape``.  ``glorot`` = (tensor id of the synthetic
    initialiser, fan_in + fan_out) of a kernel; None: the parameter starts at ``fill`` (0; the layer normalisation's gammas: 1) -
    or, with ``embedding`` (a tensor id), at Keras Embedding's U(-0.05, 0.05) like the embedding tables (the time table)."""
    name: str
    offset: int
    shape: tuple
    glorot: tuple | None = None
    fill: float = 0.0
    embedding: int | None = None

    @property
    def end(self) -> int:
        return self.offset + math.prod(self.shape)

    def view(self, flat):
        return flat[self.offset:self.end].view(self.shape)


@dataclass(frozen=True)
class DenseSegment:
    """One segment of the dense optimizer launches: the floats [lo, hi) of ``dense_flat`` (and of its accumulator / moments),
    whether the l2 term applies, the floats between two of its gradient slabs, and the block group it belongs to."""
    name: str
    lo: int
    hi: int
    l2: bool
    stride: int
    group: str                                   # "towers" | "features" | "head" | "cross" | "attention" | "norm" | "time" | "gru" | "self_attention"

    @property
    def size(self) -> int:
        return self.hi - self.lo


@dataclass(frozen=True)
class DenseLayout:
    blocks: dict                                 # name -> DenseBlock, in the order of dense_flat
    segments: tuple                              # DenseSegment, in the order of the optimizer launches
    total: int                                   # floats of dense_flat

    def segment(self, name: str) -> DenseSegment:
        return next(s for s in self.segments if s.name == name)


def dense_layout(cfg: TwoTowerConfig) -> DenseLayout:
    """Where every dense parameter sits in ``dense_flat`` and which optimizer segment covers it - a function of the config alone
    (plain integers: no device, no library), and the ONE place that knows.  In floats and in this order:

        user tower, item tower     per layer W [k, n] | b [n]; a segment per W (l2) and per b
        P_user [Fu, D], P_item     the numeric side features' projection kernels, a segment each (l2)
        rating head                W1 [2S, H] | w2 [H] | b1 [H] | b2 [1]; the segments W1 | w2 (l2) and b1 | b2
        cross layers               from a 16-byte boundary (the head's parameter count is odd, the cross launches load float4s -
                                   up to 3 idle floats): user W_0 .. W_{L-1} | item W_0 .. | user b_0 .. | item b_0 ..; every
                                   kernel is one segment (l2), every bias another - their gradient slabs are laid out like the
                                   parameters, so both segments' slab stride is the whole cross block
        history attention          from a 16-byte boundary (the launches load a as float4s): [a (D) | p (user_history_len)],
                                   one segment, no l2
        layer normalisation        from a 16-byte boundary (the launches load gamma and beta as float4s): user gamma_0 .. | item
                                   gamma_0 .. | user beta_0 .. | item beta_0 .., one entry per hidden layer; ONE segment, no l2 -
                                   the gradient slabs are laid out like the parameters, so its slab stride is the whole block
        time table                 from a 16-byte boundary (the launches load its rows as float4s): [time_rows, D], the enabled
                                   fields' row blocks in their fixed order; ONE segment, no l2, one gradient "slab" - the backward
                                   launch writes the fully reduced gradient
        history GRU                from a 16-byte boundary (the launches load its rows as float4s): W [D, 3D] | U [D, 3D] |
                                   b [2, 3D] = b_i, b_r; four segments - W, U, b_i, b_r -, none with l2: the gradient GEMMs write
                                   one slab array per kernel and one per bias row
        history self-attention     from a 16-byte boundary: Wqk [D, H D] | Wvo [H D, D] | p [H, L]; three segments, none with l2:
                                   the gradient GEMMs write one slab array per kernel, the pool backward launch p's

    Every optional block sits BEHIND what was there before it: switching one on moves no existing offset, and without the
    blocks behind it dense_flat ends behind the cross block with no trailing pad."""
    blocks, segs, off = {}, [], 0
    d = cfg.embedding_dim

    def block(name, shape, glorot=None, fill=0.0, embedding=None):
        nonlocal off
        blocks[name] = blk = DenseBlock(name, off, tuple(shape), glorot, fill, embedding)
        off = blk.end
        return blk

    def segment(group, name, first, last, l2, stride=None):
        segs.append(DenseSegment(name, first.offset, last.end, l2, last.end - first.offset if stride is None else stride, group))

    sides = (("user", cfg.user_dims, cfg.n_user_features, TID_USER_FEATURE_PROJ),
             ("item", cfg.item_dims, cfg.n_item_features, TID_ITEM_FEATURE_PROJ))
    for t, (side, dims, _, _) in enumerate(sides):
        for l, (k, n) in enumerate(zip([d] + dims, dims)):
            w = block(f"{side}.W{l}", (k, n), (TID_DENSE_BASE + 2 * l + t, k + n))
            b = block(f"{side}.b{l}", (n,))
            segment("towers", w.name, w, w, True)
            segment("towers", b.name, b, b, False)
    for side, _, f, tid in sides:
        if f:
            p = block(f"P_{side}", (f, d), (tid, f + d))
            segment("features", p.name, p, p, True)
    if cfg.rating_weight > 0:                    # (w2 is the [H, 1] kernel of the output unit)
        s, h = cfg.tower_dims[-1], cfg.rating_hidden
        w1, w2 = block("head.W1", (2 * s, h), (TID_RATING_W1, 2 * s + h)), block("head.w2", (h,), (TID_RATING_W2, h + 1))
        b1, b2 = block("head.b1", (h,)), block("head.b2", (1,))
        segment("head", "head.kernels", w1, w2, True)
        segment("head", "head.biases", b1, b2, False)
    if cfg.cross_layers:
        off = start = (off + 3) // 4 * 4
        ws = [block(f"cross.{side}.W{l}", (d, d), (TID_CROSS_BASE + 2 * l + t, 2 * d))
              for t, (side, _, _, _) in enumerate(sides) for l in range(cfg.cross_layers)]
        bs = [block(f"cross.{side}.b{l}", (d,)) for side, _, _, _ in sides for l in range(cfg.cross_layers)]
        segment("cross", "cross.kernels", ws[0], ws[-1], True, off - start)
        segment("cross", "cross.biases", bs[0], bs[-1], False, off - start)
    if cfg.history_attention:
        off = (off + 3) // 4 * 4
        a = block("history_attn", (d + cfg.user_history_len,))
        segment("attention", a.name, a, a, False)
    if cfg.layer_norm:
        off = (off + 3) // 4 * 4
        gs = [block(f"norm.{side}.g{l}", (n,), fill=1.0) for side, dims, _, _ in sides for l, n in enumerate(dims[:-1])]
        bs = [block(f"norm.{side}.b{l}", (n,)) for side, dims, _, _ in sides for l, n in enumerate(dims[:-1])]
        if gs:
            segment("norm", "norm", gs[0], bs[-1], False)
    if cfg.time_fields:
        off = (off + 3) // 4 * 4
        t = block("time_table", (cfg.time_rows, d), embedding=TID_TIME_BASE)
        segment("time", t.name, t, t, False)
    if cfg.history_gru:
        off = (off + 3) // 4 * 4
        w = block("history_gru.W", (d, 3 * d), (TID_GRU_BASE, 4 * d))
        u = block("history_gru.U", (d, 3 * d), (TID_GRU_BASE + 1, 4 * d))
        b = block("history_gru.b", (2, 3 * d))
        segment("gru", w.name, w, w, False)
        segment("gru", u.name, u, u, False)
        segs.append(DenseSegment("history_gru.b_i", b.offset, b.offset + 3 * d, False, 3 * d, "gru"))
        segs.append(DenseSegment("history_gru.b_r", b.offset + 3 * d, b.end, False, 3 * d, "gru"))
    if cfg.history_self_attention:
        off = (off + 3) // 4 * 4
        hd = cfg.history_heads * d
        wqk = block("history_sa.Wqk", (d, hd), (TID_SELF_ATTENTION_BASE, d + d))
        wvo = block("history_sa.Wvo", (hd, d), (TID_SELF_ATTENTION_BASE + 1, hd + d))
        pb = block("history_sa.p", (cfg.history_heads, cfg.user_history_len))
        for blk in (wqk, wvo, pb):
            segment("self_attention", blk.name, blk, blk, False)
    return DenseLayout(blocks, tuple(segs), off)


class Tower:
    """Dense stack: ReLU on all but the last layer (Keras Dense)."""

    def __init__(self, cfg: TwoTowerConfig, tower_dims: list, flat: torch.Tensor, flat_acc, offset: int, dev, rows: int | None = None):
        """``rows``: rows of every activation / gradient buffer (default cfg.batch_size; the item tower of mixed negative
        sampling holds batch_size + n_sampled_negatives)."""
        self.dims = [cfg.embedding_dim] + list(tower_dims)
        self.n_layers = len(tower_dims)
        self.rows = b = cfg.batch_size if rows is None else int(rows)
        self.w, self.b, self.w_acc, self.b_acc = [], [], [], []
        for l in range(self.n_layers):
            k, n = self.dims[l], self.dims[l + 1]
            self.w.append(flat[offset:offset + k * n].view(k, n))
            self.w_acc.append(None if flat_acc is None else flat_acc[offset:offset + k * n].view(k, n))
            offset += k * n
            self.b.append(flat[offset:offset + n])
            self.b_acc.append(None if flat_acc is None else flat_acc[offset:offset + n])
            offset += n
        self.end_offset = offset
        ns = ops.dense_bwd_num_slabs(b)
        self.n_slabs = ns
        self.acts = [torch.empty(b, self.dims[0], device=dev)] + \
                    [torch.empty(b, self.dims[l + 1], device=dev) for l in range(self.n_layers)]
        # dz[l]: gradient w.r.t. the pre-activation of layer l; dz[n_layers-1] is the scorer's dq/dc
        self.dz = [torch.empty(b, self.dims[l + 1], device=dev) for l in range(self.n_layers)]
        self.demb = torch.empty(b, self.dims[0], device=dev)
        # cfg.normalize_embeddings: the L2-normalised output (what the scorer reads as q / c) and the scorer's gradient w.r.t. it
        self.unit = self.dunit = None
        if cfg.normalize_embeddings:
            self.alloc_unit()
        # sign bits of the hidden (ReLU) activations, written by the forward GEMM's epilogue and read by the next layer's dx
        # epilogue as its mask: [b, n/32] words instead of re-reading acts[l] (indexed like acts; None where n % 32 != 0)
        self.bits = [None] + [ops.relu_bits_like(b, self.dims[l + 1], dev) if (l < self.n_layers - 1 and self.dims[l + 1] % 32 == 0)
                              else None for l in range(self.n_layers)]
        self.dw_slabs = [torch.empty(ns, self.dims[l], self.dims[l + 1], device=dev) for l in range(self.n_layers)]
        self.db_slabs = [torch.empty(ns, self.dims[l + 1], device=dev) for l in range(self.n_layers)]
        # cfg.cross_layers: the cross stack between acts[0] (x_0) and layer 0.  xc[l] = x_{l+1} (layer 0 reads xc[-1]) and
        # cu[l] = u_l stay for the backward chain; layer 0 writes its input gradient G_L into cg[0], the chain alternates
        # between cg[0] and cg[1] (a launch never writes the buffer it reads) and ends in demb; ca collects the gradient that
        # reaches x_0 through the Hadamard factors of layers 1 .. L-1.  The parameters (views of dense_flat) and the gradient
        # slabs belong to the trainer: ``set_cross``.
        self.n_cross = nc = cfg.cross_layers
        self.cross_w, self.cross_b, self.cross_dw_slabs, self.cross_db_slabs = [], [], [], []
        self.cross_n_slabs = self.cross_slab_stride = 0
        d0 = self.dims[0]
        self.xc = [torch.empty(b, d0, device=dev) for _ in range(nc)]
        self.cu = [torch.empty(b, d0, device=dev) for _ in range(nc)]
        self.cg = [torch.empty(b, d0, device=dev) for _ in range(min(nc, 2))]
        self.ca = torch.empty(b, d0, device=dev) if nc > 1 else None
        # cfg.layer_norm: hidden layer l writes its pre-activation z_l into pre[l]; the normalisation launch reads it and writes
        # acts[l + 1] and bits[l + 1]; the backward launch reads it again (mean and variance are recomputed) and turns what layer
        # l + 1's dx epilogue wrote into dz[l] - the gradient w.r.t. the normalised value - into the gradient w.r.t. z_l, in
        # place.  gamma / beta (views of dense_flat) and the gradient slabs belong to the trainer: ``set_layer_norm``.
        self.ln = bool(cfg.layer_norm)
        self.ln_eps = float(cfg.layer_norm_epsilon)
        self.pre = [torch.empty(b, self.dims[l + 1], device=dev) for l in range(self.n_layers - 1)] if self.ln else []
        self.ln_gamma, self.ln_beta, self.ln_dg_slabs, self.ln_db_slabs = [], [], [], []
        self.ln_n_slabs = self.ln_slab_stride = 0
        # what each kind of pass launches, built on first use (towers_forward / towers_backward).  The plans hold views of the
        # buffers and parameters above: whoever rebinds one of those after a pass has run clears them.
        self.plans = {}

    def set_layer_norm(self, gammas, betas, dg_slabs, db_slabs, n_slabs: int, slab_stride: int):
        """The normalisation's gamma / beta [n_l] per hidden layer and, per layer, the flat views that start at slab 0 of its
        dgamma / dbeta in the trainer's shared [n_slabs, slab_stride] gradient-slab array."""
        self.ln_gamma, self.ln_beta, self.ln_dg_slabs, self.ln_db_slabs = list(gammas), list(betas), list(dg_slabs), list(db_slabs)
        self.ln_n_slabs, self.ln_slab_stride = int(n_slabs), int(slab_stride)
        self.plans.clear()

    def set_cross(self, ws, bs, dw_slabs, db_slabs, n_slabs: int, slab_stride: int):
        """The cross stack's parameters [D, D] / [D] per layer and, per layer, the flat views that start at slab 0 of its dW /
        db in the trainer's shared [n_slabs, slab_stride] gradient-slab array."""
        self.cross_w, self.cross_b, self.cross_dw_slabs, self.cross_db_slabs = list(ws), list(bs), list(dw_slabs), list(db_slabs)
        self.cross_n_slabs, self.cross_slab_stride = int(n_slabs), int(slab_stride)
        self.plans.clear()

    def layer_input(self, l: int, rows: int | None = None):
        """What Dense layer ``l`` reads: acts[l] - for layer 0 under cross layers the crossed rows x_L."""
        x = self.xc[-1] if (l == 0 and self.n_cross) else self.acts[l]
        return x if rows is None else x[:rows]

    def input_grad(self):
        """Where Dense layer 0 writes its input gradient: demb - under cross layers G_L, which the cross chain turns into demb."""
        return self.cg[0] if self.n_cross else self.demb

    def cross_fwd_problem(self, l: int, keep_u: bool, rows: int | None = None):
        n = self.rows if rows is None else rows
        x0 = self.acts[0][:n]
        return (x0, x0 if l == 0 else self.xc[l - 1][:n], self.cross_w[l], self.cross_b[l], self.xc[l][:n]), \
            (self.cu[l][:n] if keep_u else None)

    def cross_bwd_problem(self, l: int):
        L = self.n_cross
        return (self.acts[0], self.acts[0] if l == 0 else self.xc[l - 1], self.cu[l], self.cross_w[l], self.cg[(L - 1 - l) % 2],
                self.demb if l == 0 else self.cg[(L - l) % 2], self.ca, self.cross_dw_slabs[l], self.cross_db_slabs[l])

    def alloc_unit(self):
        if self.unit is None:
            self.unit, self.dunit = torch.empty_like(self.acts[-1]), torch.empty_like(self.acts[-1])

    @staticmethod
    def param_count(cfg: TwoTowerConfig, tower_dims: list) -> int:
        dims = [cfg.embedding_dim] + list(tower_dims)
        return sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(len(tower_dims)))

    def forward(self, dropout=None, lookup=None, rows: int | None = None):
        """This tower alone through ``towers_forward``: dropout = (rate, seed, tower_index, first_global_row) in training, None =
        inference; lookup (ops.make_lookup): layer 0 reads its input rows from the embedding table (acts[0] is not used); rows:
        only the first ``rows`` rows of the buffers (an in-batch evaluation on the longer item tower of mixed sampling)."""
        return towers_forward((self,), None if dropout is None else (dropout,), None if lookup is None else (lookup,),
                              None if rows is None else (rows,))[0]

    def backward(self, dropout_rate: float = 0.0, dx: bool = True, dw: bool = True, lookup=None):
        """This tower alone through the backward driver: consumes dz[-1]; leaves demb (dx) and the dw/db slabs (dw).
        backward(dx=True, dw=False) followed by backward(dx=False, dw=True) is the same computation with every dx first."""
        _backward_pass((self,), dropout_rate, None if lookup is None else (lookup,), dx, dw)

    def segments(self, l2: float, grad_flat=None, grad_offset: int = 0):
        segs = []
        off = grad_offset
        for l in range(self.n_layers):
            for p, acc, slabs, reg in ((self.w[l], self.w_acc[l], self.dw_slabs[l], l2),
                                       (self.b[l], self.b_acc[l], self.db_slabs[l], 0.0)):
                gout = None if grad_flat is None else grad_flat[off:off + p.numel()]
                segs.append(ops.make_dense_seg(p, acc, slabs, self.n_slabs, reg, gout))
                off += p.numel()
        return segs


# ---------------------------------------------------------------------------------------------------------------------------
# The two drivers of the tower stacks.  ``towers`` is a tuple of one or two Towers; what a pass launches depends only on the
# towers, its row counts, which towers read through a lookup and whether it trains, so it is decided ONCE per such key
# (``Tower.plans``): a plan is the list of (launcher, args, kwargs) with every buffer view already cut, plus the slots of those
# kwargs that a step fills in - the dropout tuples, the lookup structs, the dx scale.  A step fills the slots and walks the list.
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dropout_scale(dropout_rate: float) -> float:
    """1 / (1 - rate) in the f32 arithmetic of the forward kernels' launchers."""
    if not dropout_rate > 0.0:
        return 1.0
    one = torch.ones((), dtype=torch.float32)
    return (one / (one - torch.tensor(dropout_rate, dtype=torch.float32))).item()


def _layer_dropout(drops, l: int, width: int):
    """The dropout tuple of ONE launch behind hidden layer ``l`` (``width`` columns) from its towers' (rate, seed, tower_index,
    first_global_row): the stream of tower t is tensor id TID_DROPOUT_BASE + 2 l + t - a shared launch takes the pair of ids -
    and starts at element first_global_row * width.  None: nothing is dropped (training at rate 0)."""
    rate, seed, _, row0 = drops[0]
    if not rate > 0.0:
        return None
    tids = tuple(TID_DROPOUT_BASE + 2 * l + d[2] for d in drops)
    return (rate, seed, tids if len(tids) == 2 else tids[0], row0 * width)


def _share(towers, l: int, looks, relu: bool = False) -> bool:
    """Whether Dense layer ``l`` of ``towers`` is ONE launch: two towers that agree on the layer's (k, n), on their rows (hence
    on n_slabs) and on whether layer 0 reads through a lookup.  ``relu``: the launch applies the layer's activation, so the
    layer must be hidden in both towers or the output of both."""
    if len(towers) < 2 or l >= min(t.n_layers for t in towers):
        return False
    a, b = towers
    return (a.dims[l:l + 2] == b.dims[l:l + 2] and a.rows == b.rows and a.n_slabs == b.n_slabs and (l > 0 or looks[0] == looks[1])
            and not (relu and (l < a.n_layers - 1) != (l < b.n_layers - 1)))


class _Plan:
    """Launches in order and the kwargs slots a step fills: ``drops`` (kwargs, tower indices, layer, width), ``looks`` (dict,
    key, tower index or None for both), ``scales`` (kwargs, key).  ``shared``: some launch serves both towers - two towers that
    share none run one after the other instead, each through its own plan (a tower's activations are still in cache when its
    next layer reads them)."""

    def __init__(self):
        self.launches, self.drops, self.looks, self.scales, self.outputs, self.shared = [], [], [], [], None, False

    def add(self, fn, args, problems: int = 1, **kw):
        self.launches.append((fn, args, kw))
        self.shared |= problems > 1
        return kw


def _forward_plan(towers, rows, looks, train: bool, together: bool) -> _Plan:
    plan, n, ln = _Plan(), len(towers), towers[0].ln
    cut = lambda x, i: None if x is None else x[:rows[i]]
    if towers[0].n_cross:                        # the cross stack in front of layer 0, one launch per layer for all towers
        if any(looks):
            raise ValueError("towers_forward: the cross layers read materialised input rows (acts[0]), not a fused lookup")
        for l in range(towers[0].n_cross):
            probs, us = zip(*[t.cross_fwd_problem(l, train, rows[i]) for i, t in enumerate(towers)])
            plan.add(ops.cross_layer, probs, n, u=us if train else None)       # u_l stays for the backward chain
    depth = max(t.n_layers for t in towers)
    # the last two layers (ReLU hidden + linear output) of both towers in ONE launch when their shapes allow it: the hidden tile
    # never leaves the CU between them (csrc/tower.hip); two-layer towers are that launch alone (with the lookup inside), deeper
    # ones - the reference's [512, 256, 128] - run the layers below one by one first.  Never with layer normalisation, which
    # sits between the two layers.
    a = towers[0]
    tail = (n == 2 and depth >= 2 and a.n_layers == towers[1].n_layers and not ln and together
            and _share(towers, depth - 2, looks, True) and _share(towers, depth - 1, looks, True)
            and ops.tower_fwd2_supported(rows[0], a.dims[depth - 2], a.dims[depth - 1], a.dims[depth]))
    for l in range(depth):
        act = [i for i, t in enumerate(towers) if l < t.n_layers]
        hid = [i for i in act if l < towers[i].n_layers - 1]
        x = {i: towers[i].layer_input(l, rows[i]) for i in act}
        # with layer normalisation a hidden layer is the linear launch into pre[l] and the normalisation launch, which applies
        # ReLU and dropout and writes acts[l + 1] and bits[l + 1]
        y = {i: cut(towers[i].pre[l] if (ln and i in hid) else towers[i].acts[l + 1], i) for i in act}
        bits = {i: None if ln else cut(towers[i].bits[l + 1], i) for i in act}
        drop = lambda idx: (idx, l, towers[idx[0]].dims[l + 1])
        pair = lambda v: tuple(v(towers[i]) if callable(v) else v[i] for i in act)
        if tail and l == depth - 2:
            kw = plan.add(ops.tower_fwd2, (pair(x), pair(lambda t: t.w[l]), pair(lambda t: t.b[l]), pair(y), pair(bits),
                                           pair(lambda t: t.w[l + 1]), pair(lambda t: t.b[l + 1]), pair(lambda t: t.acts[l + 2])),
                          2, dropout=None, lookups=None)
            plan.drops.append((kw,) + drop((0, 1)))
            if l == 0 and looks[0]:
                plan.looks.append((kw, "lookups", None))
            break
        if _share(towers, l, looks, relu=not ln) and together:
            kw = plan.add(ops.dense_fwd2, (pair(x), pair(lambda t: t.w[l]), pair(lambda t: t.b[l]), pair(y)), 2, relu=bool(hid) and not ln,
                          dropout=None, lookups=None, relu_bits=pair(bits))
            if hid and not ln:
                plan.drops.append((kw,) + drop((0, 1)))
            if l == 0 and looks[0]:
                plan.looks.append((kw, "lookups", None))
        else:
            for i in act:
                t = towers[i]
                kw = plan.add(ops.dense_fwd, (x[i], t.w[l], t.b[l]), relu=i in hid and not ln, out=y[i], dropout=None, lookup=None,
                              relu_bits=bits[i])
                if i in hid and not ln:
                    plan.drops.append((kw,) + drop((i,)))
                if l == 0 and looks[i]:
                    plan.looks.append((kw, "lookup", i))
        if ln and hid:
            probs = {i: (y[i], towers[i].ln_gamma[l], towers[i].ln_beta[l], cut(towers[i].acts[l + 1], i), cut(towers[i].bits[l + 1], i))
                     for i in hid}
            # one launch for both towers where the widths agree, whatever the rows (mixed sampling's longer item tower)
            shared = len(hid) == 2 and towers[0].dims[l + 1] == towers[1].dims[l + 1] and together
            for idx in ([tuple(hid)] if shared else [(i,) for i in hid]):
                kw = plan.add(ops.layer_norm2, tuple(probs[i] for i in idx), len(idx), eps=towers[idx[0]].ln_eps, relu=True, dropout=None)
                plan.drops.append((kw,) + drop(idx))
    if not train:
        plan.drops = []
    plan.outputs = tuple(cut(t.acts[-1], i) for i, t in enumerate(towers))
    return plan


def towers_forward(towers, dropouts=None, lookups=None, rows=None):
    """The forward pass of ``towers`` (one Tower, or both), layer by layer; returns their outputs.  Per tower: ``dropouts`` =
    (rate, seed, tower_index, first_global_row) in training (also at rate 0), None = inference - inverted dropout follows every
    hidden (ReLU) layer, fused into the launch that applies the ReLU; ``lookups`` (ops.make_lookup): layer 0 gathers its input
    rows from the embedding table itself (acts[0] is not used); ``rows``: fewer than the tower holds = an inference pass over the
    first rows of every buffer, which shares no launch with the other tower.  Towers that share no launch run one after the other."""
    n = len(towers)
    train = dropouts is not None and dropouts[0] is not None
    nrows = tuple(t.rows if rows is None or rows[i] is None else int(rows[i]) for i, t in enumerate(towers))
    alone = lambda: tuple(towers_forward((t,), None if dropouts is None else (dropouts[i],), None if lookups is None else (lookups[i],),
                                         (nrows[i],))[0] for i, t in enumerate(towers))
    if any(r != t.rows for t, r in zip(towers, nrows)):
        if train:
            raise ValueError("towers_forward: a partial forward pass is an inference pass (no dropout)")
        if n > 1:
            return alone()
    looks = (False,) * n if lookups is None else tuple(lk is not None for lk in lookups)
    # a shared launch that drops out needs one (rate, seed, offset) for both towers: equal rows give exactly that; mixed
    # sampling's towers count their rows separately (and share only the normalisation launch of step 0)
    together = not train or len({(d[0], d[1], d[3]) if d[0] > 0.0 else None for d in dropouts}) == 1
    key = ("forward", towers[1:], nrows, looks, train, together)
    plan = towers[0].plans.get(key)
    if plan is None:
        plan = towers[0].plans[key] = _forward_plan(towers, nrows, looks, train, together)
    if n > 1 and not plan.shared:
        return alone()
    for kw, idx, l, width in plan.drops:
        kw["dropout"] = _layer_dropout([dropouts[i] for i in idx], l, width)
    for kw, name, i in plan.looks:
        kw[name] = lookups if i is None else lookups[i]
    for fn, args, kw in plan.launches:
        fn(*args, **kw)
    return plan.outputs


def _backward_plan(towers, looks, dx: bool, dw: bool, bwd2_ws) -> _Plan:
    plan, n, ln = _Plan(), len(towers), towers[0].ln
    if not (dx and dw) and (ln or towers[0].n_cross):
        raise NotImplementedError("towers_backward: the backward launches of layer normalisation and of the cross layers compute dx and "
                                  "dW in one pass (no dx-first split, no on_embedding_grads)")
    depth = max(t.n_layers for t in towers)

    def layer(l, idx):
        """dense_bwd2's arguments of layer ``l`` for the towers ``idx``: the mask of dx comes from bits[l], from acts[l] - the
        (dropped-out) ReLU output of layer l - 1 - where the width is not a multiple of 32."""
        ts = [towers[i] for i in idx]
        bits = tuple(t.bits[l] if (l > 0 and dx) else None for t in ts)
        return dict(xs=tuple(t.layer_input(l) for t in ts), ws=tuple(t.w[l] for t in ts), dzs=tuple(t.dz[l] for t in ts),
                    dxs=tuple((t.dz[l - 1] if l > 0 else t.input_grad()) if dx else None for t in ts),
                    dx_relu_srcs=tuple(t.acts[l] if (l > 0 and dx and b is None) else None for t, b in zip(ts, bits)),
                    dw_slabs=tuple(t.dw_slabs[l] if dw else None for t in ts), db_slabs=tuple(t.db_slabs[l] if dw else None for t in ts),
                    lookups=None, dx_relu_bits=bits)

    # layers 1 and 0 of both towers in ONE launch (tt_tower_bwd2_batched_f32) where a workspace is given and the shapes allow it
    a = towers[0]
    head = (bwd2_ws is not None and dx and dw and n == 2 and depth >= 2 and a.n_layers == towers[1].n_layers and not ln
            and _share(towers, 1, looks) and _share(towers, 0, looks) and ops.tower_bwd2_supported(a.rows, a.dims[0], a.dims[1], a.dims[2]))
    for l in range(depth - 1, -1, -1):
        act = tuple(i for i, t in enumerate(towers) if l < t.n_layers)
        if head and l == 1:
            upper, lower = layer(1, act), layer(0, act)
            plan.scales.append((plan.add(ops.tower_bwd2, (upper, lower, bwd2_ws), 2, dx_scale_upper=1.0, dx_scale_lower=1.0), "dx_scale_upper"))
            if looks[0]:
                plan.looks.append((lower, "lookups", None))
            break
        for idx in ([act] if _share(towers, l, looks) else [(i,) for i in act]):
            g = layer(l, idx)
            if len(idx) == 2:
                kw = plan.add(ops.dense_bwd2, (g["xs"], g["ws"], g["dzs"], g["dxs"], g["dx_relu_srcs"], g["dw_slabs"], g["db_slabs"]),
                              2, dx_scale=1.0, lookups=None, dx_relu_bits=g["dx_relu_bits"])
            else:
                kw = plan.add(ops.dense_bwd, tuple(g[k][0] for k in ("xs", "ws", "dzs", "dxs", "dx_relu_srcs", "dw_slabs", "db_slabs")),
                              dx_scale=1.0, lookup=None, dx_relu_bits=g["dx_relu_bits"][0])
            if l > 0:
                plan.scales.append((kw, "dx_scale"))
            elif looks[idx[0]]:
                plan.looks.append((kw, "lookups", None) if len(idx) == 2 else (kw, "lookup", idx[0]))
        if ln and l > 0:
            # layer l's dx epilogue left the gradient w.r.t. the normalised value in dz[l - 1]; the normalisation's backward launch
            # turns it into the gradient w.r.t. the pre-activation IN PLACE (and writes the dgamma / dbeta slabs) before Dense
            # layer l - 1 reads it.  One launch for both towers where the widths agree.
            probs = {i: (towers[i].pre[l - 1], towers[i].ln_gamma[l - 1], towers[i].dz[l - 1], towers[i].dz[l - 1],
                         towers[i].ln_dg_slabs[l - 1], towers[i].ln_db_slabs[l - 1]) for i in act}
            shared = len(act) == 2 and towers[0].dims[l] == towers[1].dims[l]
            for idx in ([act] if shared else [(i,) for i in act]):
                plan.add(ops.layer_norm_bwd2, tuple(probs[i] for i in idx), len(idx), eps=a.ln_eps, n_slabs=a.ln_n_slabs, slab_stride=a.ln_slab_stride)
    L = a.n_cross                                # the cross chain behind layer 0: from G_L (cg[0]) down to demb
    for l in range(L - 1, -1, -1):
        plan.add(ops.cross_layer_bwd, tuple(t.cross_bwd_problem(l) for t in towers), n, x_is_x0=l == 0, accumulate_dx0=0 < l < L - 1,
                 n_slabs=a.cross_n_slabs, slab_stride=a.cross_slab_stride)
    return plan


def _backward_pass(towers, dropout_rate: float, lookups, dx: bool = True, dw: bool = True, bwd2_ws=None):
    """One walk down the Dense stacks (and the cross chains): dx and dW + db of every layer, or only the one or the other."""
    if not dw:
        lookups = None                           # dx = dz W^T reads no layer input: the dx-only pass of layer 0 needs no lookup
    looks = (False,) * len(towers) if lookups is None else tuple(lk is not None for lk in lookups)
    key = ("backward", towers[1:], looks, dx, dw, id(bwd2_ws))
    plan = towers[0].plans.get(key)
    if plan is None:
        plan = towers[0].plans[key] = _backward_plan(towers, looks, dx, dw, bwd2_ws)
    if len(towers) > 1 and not plan.shared:
        for i, t in enumerate(towers):
            _backward_pass((t,), dropout_rate, None if lookups is None else (lookups[i],), dx, dw)
        return
    scale = _dropout_scale(dropout_rate)
    for kw, name in plan.scales:
        kw[name] = scale
    for kw, name, i in plan.looks:
        kw[name] = lookups if i is None else lookups[i]
    for fn, args, kw in plan.launches:
        fn(*args, **kw)


def towers_backward(towers, dropout_rate: float = 0.0, lookups=None, on_embedding_grads=None, bwd2_ws=None):
    """The backward pass of ``towers`` (one Tower, or both): consumes dz[-1]; leaves demb and the dw / db slabs.  ``lookups`` as in
    ``towers_forward`` (dW = x^T dz of layer 0 reads the rows through them).  With ``on_embedding_grads`` every dx launch of every
    layer comes first, the callback runs as soon as demb is complete (the sharded trainer starts the gradient exchange there) and
    the dW + db launches follow, beside the transfer.  ``bwd2_ws`` (ops.tower_bwd2_workspace): layers 1 and 0 in ONE launch
    where the shapes allow it - never in the split pass."""
    if on_embedding_grads is None:
        return _backward_pass(towers, dropout_rate, lookups, bwd2_ws=bwd2_ws)
    _backward_pass(towers, dropout_rate, lookups, dx=True, dw=False)
    on_embedding_grads()
    _backward_pass(towers, dropout_rate, lookups, dx=False, dw=True)


@dataclass
class EmbeddingTable:
    """One embedding table of the trainer with everything that belongs to it: the checkpoint prefix (``user`` -> the keys
    ``user_table``, ``user_accum``, ``user_m``, ``user_v``, ``user_row_accum``), the tensor id of the synthetic initialiser, the
    optimizer state of the configured optimizer (Adagrad: ``accum``; lazy Adam: ``m``, ``v``; row-wise Adagrad: ``row_accum``
    [rows], and ``accum`` stays None so that no kernel that expects [rows, dim] can be handed it; else None), the sort plan of its
    updates, and ``extra`` - the tensors checkpointed beside it under their own keys (the title / history token rows)."""
    prefix: str
    tensor_id: int
    table: torch.Tensor
    accum: torch.Tensor | None = None
    m: torch.Tensor | None = None
    v: torch.Tensor | None = None
    plan: object = None
    extra: dict = field(default_factory=dict)
    row_accum: torch.Tensor | None = None

    @classmethod
    def new(cls, cfg: TwoTowerConfig, dev, prefix: str, tensor_id: int, rows: int, plan, extra=None) -> "EmbeddingTable":
        table = torch.empty(rows, cfg.embedding_dim, device=dev)
        accum = torch.full_like(table, cfg.adagrad_initial_accumulator) if cfg.optimizer == "adagrad" else None
        m, v = (torch.zeros_like(table), torch.zeros_like(table)) if cfg.optimizer == "adam" else (None, None)
        row_accum = None
        if cfg.optimizer == "rowwise_adagrad":
            row_accum = torch.full((rows,), cfg.adagrad_initial_accumulator, device=dev)
        return cls(prefix, tensor_id, table, accum, m, v, plan, dict(extra or {}), row_accum)

    def state(self) -> dict:
        """Checkpoint key -> tensor."""
        named = {"table": self.table, "accum": self.accum, "m": self.m, "v": self.v, "row_accum": self.row_accum}
        return {**{f"{self.prefix}_{k}": t for k, t in named.items() if t is not None}, **self.extra}

    def init_synthetic(self, cfg: TwoTowerConfig, seed: int):
        """Keras Embedding's U(-0.05, 0.05) from the counter-based generator; the optimizer state as freshly allocated."""
        ops.fill_uniform_(self.table, seed, self.tensor_id, -0.05, 0.1)
        if self.accum is not None:
            self.accum.fill_(cfg.adagrad_initial_accumulator)
        if self.m is not None:
            self.m.zero_(), self.v.zero_()
        if self.row_accum is not None:
            self.row_accum.fill_(cfg.adagrad_initial_accumulator)

    def opt_args(self, grads) -> tuple:
        """What this table contributes to the configured optimizer's ``ops`` call with ``grads`` as its gradient rows: the table,
        the state that optimizer allocated, the gradients and the sort plan - (table, m, v, grads, plan) for lazy Adam, (table,
        row_accum, grads, plan) for row-wise Adagrad, (table, accum, grads, plan) for SGD (accum None) and Adagrad."""
        state = (self.m, self.v) if self.m is not None else (self.row_accum,) if self.row_accum is not None else (self.accum,)
        return (self.table, *state, grads, self.plan)

    @staticmethod
    def update(cfg: TwoTowerConfig, tables, segs, lr: float, adam_step: int):
        """THE place that maps cfg.optimizer to a call: the update of ``tables`` (``opt_args`` tuples) from their sort plans,
        which have run.  Lazy Adam and row-wise Adagrad take all of them, and the dense segments ``segs`` that ride along, in
        one call; SGD and Adagrad take one launch per table (their dense segments have a launch of their own)."""
        if cfg.optimizer == "adam":
            ops.adam_step_(tables, segs, ops.AdamHyper(lr, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_epsilon, adam_step))
        elif cfg.optimizer == "rowwise_adagrad":
            ops.rowwise_adagrad_step_(tables, segs, lr, cfg.adagrad_epsilon)
        else:
            for table, accum, grads, plan in tables:
                if cfg.optimizer == "sgd":
                    ops.sparse_sgd_(table, grads, plan, lr)
                else:
                    ops.sparse_adagrad_(table, accum, grads, plan, lr, cfg.adagrad_epsilon)

    def apply(self, cfg: TwoTowerConfig, grads, adam_step: int, adam_segs=(), lr: float | None = None):
        """The configured optimizer's update of this table alone (``update``) from its sort plan (which has run; a ``BagPlan``
        after its ``backward``: ``grads`` then holds one row per bag).  ``adam_segs``: dense segments that ride in the same
        lazy-Adam / row-wise Adagrad call.  ``lr``: the step's rate (default: the configured one)."""
        self.update(cfg, [self.opt_args(grads)], list(adam_segs), cfg.learning_rate if lr is None else lr, adam_step)


@dataclass
class FeatureSide:
    """The numeric side features of one tower: the fixed [rows, F] matrix with its normalisation, the projection kernel (a view
    of dense_flat), the step's normalised rows (kept for the backward launch), the projection's gradient slabs and the tower
    whose input rows the projected features are added to."""
    side: str                                    # "user" | "item": the checkpoint keys' prefix
    features: torch.Tensor
    mean: torch.Tensor
    inv_std: torch.Tensor
    P: torch.Tensor
    z: torch.Tensor
    slabs: torch.Tensor
    n_slabs: int
    tower: object = None

    def state(self) -> dict:
        """Checkpoint key -> tensor (the kernel itself is part of ``dense``)."""
        return {f"{self.side}_features": self.features, f"{self.side}_feature_mean": self.mean, f"{self.side}_feature_inv_std": self.inv_std}


def _side_fields(fs: FeatureSide | None):
    return (None,) * 6 if fs is None else (fs.features, fs.mean, fs.inv_std, fs.P, fs.z, fs.slabs)


def _table_fields(t: EmbeddingTable | None):
    return (None,) * 5 if t is None else (t.table, t.accum, t.m, t.v, t.plan)


def _glorot_uniform_(w, seed: int, tensor_id: int, fan: int):
    """Keras Glorot-uniform, limit sqrt(6 / (fan_in + fan_out)) - formed in f64 and rounded once to f32, the scale as the f32 sum
    lim + lim: bit for bit what oracle.two_tower.synthetic_state draws."""
    lim = torch.tensor(math.sqrt(6.0 / fan), dtype=torch.float64).to(torch.float32)
    ops.fill_uniform_(w, seed, tensor_id, -lim.item(), (lim + lim).item())


# what of the checkpoint's config must equal the trainer's: (key, its value in a checkpoint from before the key existed - such
# a checkpoint loads into a trainer without the feature -, what to add to the refusal, the config field that must be on for
# the check to apply or None).  rating_weight: whether there is a head must agree, not the weight.
_CHECKPOINT_CHECKS = (
    ("n_users", None, "", None), ("n_items", None, "", None), ("embedding_dim", None, "", None), ("tower_dims", None, "", None),
    ("item_tower_dims", None, "", None), ("optimizer", None, "", None), ("n_category_buckets", 0, "", None),
    ("n_user_features", 0, ": the numeric side features (and their projection kernels in 'dense') belong to the trained model", None),
    ("n_item_features", 0, ": the numeric side features (and their projection kernels in 'dense') belong to the trained model", None),
    ("rating_weight", 0.0, " (with / without a rating head): the head's parameters in 'dense' belong to the trained model", None),
    ("rating_hidden", TwoTowerConfig.rating_hidden, "", "rating_weight"),
    ("cross_layers", 0, ": the cross kernels in 'dense' belong to the trained model", None),
    ("layer_norm", False, ": the gammas and betas in 'dense' belong to the trained model", None),
    ("layer_norm_epsilon", TwoTowerConfig.layer_norm_epsilon, "", "layer_norm"),
    ("n_title_buckets", 0, "", None), ("user_history_len", 0, "", None), ("history_pooling", "mean", "", "user_history_len"),
    ("history_heads", 1, ": the self-attention kernels in 'dense' belong to the trained model", "history_self_attention"),
    ("title_max_tokens", None, "", "n_title_buckets"), ("title_pooling", None, "", "n_title_buckets"),
    ("time_fields", (), ": the time table in 'dense' belongs to the trained model", None),
    ("time_buckets", 0, "", "time_fields"), ("time_min", 0, "", "time_fields"), ("time_max", 0, "", "time_fields"))


# what graph replay is not implemented for: (config -> bool, the refusal)
_GRAPH_REFUSALS = (
    (lambda c: c.dropout_rate > 0.0, "dropout: the per-step counter is a kernel argument"),
    (lambda c: c.optimizer == "adam", "optimizer='adam': the global step, and so the bias-corrected step size, is a kernel argument"),
    (lambda c: c.optimizer == "rowwise_adagrad", "optimizer='rowwise_adagrad' is not implemented: the warm-up step's update of the "
     "row accumulators is not undone"),
    (lambda c: c.candidate_sampling == "mixed", "candidate_sampling='mixed' is not implemented: the sampler's counter is a kernel "
     "argument and the step is the Python sequence of per-tower launches"),
    (lambda c: c.sampling_bias_estimator == "streaming", "the streaming frequency estimator (sampling_bias_estimator='streaming') "
     "is not implemented: the step number is a launch argument"),
    (lambda c: c.n_title_buckets, "the title feature (n_title_buckets > 0) is not implemented: the warm-up step's update of the "
     "title table is not undone"),
    (lambda c: c.user_history_len, "the user-history feature (user_history_len > 0) is not implemented: the warm-up step's update "
     "of the history table is not undone"),
    (lambda c: c.n_user_features or c.n_item_features, "the numeric side features (n_user_features / n_item_features > 0) is not "
     "implemented: the step is the Python sequence of launches over materialised tower inputs"),
    (lambda c: c.rating_weight > 0, "the rating head (rating_weight > 0) is not implemented: the step is the Python sequence of launches"),
    (lambda c: c.cross_layers, "cross layers (cross_layers > 0) is not implemented: the step is the Python sequence of launches over "
     "materialised tower inputs"),
    (lambda c: c.layer_norm, "layer normalisation (layer_norm=True) is not implemented: the step is the Python sequence of launches"),
    (lambda c: c.time_fields, "the time context features (time_fields) is not implemented: the step is the Python sequence of "
     "launches over materialised tower inputs"),
    (lambda c: c.global_clipnorm > 0, "gradient clipping (global_clipnorm > 0) is not implemented: the step is the Python sequence of "
     "launches"),
    (lambda c: c.retrieval_loss != "softmax", "a pairwise retrieval loss (retrieval_loss='bpr' / 'hinge') is not implemented: the "
     "step is the Python sequence of launches"),
    (lambda c: c.lr_schedule_on, "a learning-rate schedule (lr_warmup_steps / lr_decay): the step's rate is a kernel argument"))


class TwoTowerTrainer:
    def __init__(self, cfg: TwoTowerConfig, device="cuda:0", seed: int | None = None):
        cfg.validate()
        self.cfg = cfg
        self.dev = dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("TwoTowerTrainer needs a CUDA/HIP device: there is no CPU fallback")
        b, d = cfg.batch_size, cfg.embedding_dim
        # mixed negative sampling: the item side of the step - tower buffers, sort plan, title slots, candidate list - holds the
        # batch's items followed by the sampled ones (bi rows); the user side keeps b
        self.mixed = cfg.candidate_sampling == "mixed"
        bi = b + (cfg.n_sampled_negatives if self.mixed else 0)
        # (row-wise Adagrad: the dense parameters keep the element-wise Adagrad accumulator, exactly as under "adagrad")
        adagrad, adam = cfg.optimizer in ("adagrad", "rowwise_adagrad"), cfg.optimizer == "adam"
        # where every dense parameter sits and which optimizer segment covers it: dense_layout, the one place that knows
        self.layout = lay = dense_layout(cfg)
        self.rating_on = cfg.rating_weight > 0
        self._attn_on = cfg.history_attention
        self._gru_on = cfg.history_gru
        self._sa_on = cfg.history_self_attention
        self._slot_rows = self._attn_on or self._gru_on or self._sa_on     # the history update takes one gradient row per slot
        sd, rh, ncl = cfg.tower_dims[-1], cfg.rating_hidden, cfg.cross_layers
        self.dense_flat = torch.zeros(lay.total, device=dev)
        self._fill_constant_blocks()             # (the layer normalisation's gammas start at 1 with or without a seed)
        self.dense_accum = torch.full_like(self.dense_flat, cfg.adagrad_initial_accumulator) if adagrad else None
        self.dense_grad = torch.empty_like(self.dense_flat)        # summed gradients (multi-GPU all-reduce bucket)
        # lazy Adam: first / second moment beside every table and beside dense_flat (allocated for Adam only), and the 1-based
        # global step the bias correction is taken from - part of the optimizer state (checkpointed)
        self.dense_m, self.dense_v = (torch.zeros_like(self.dense_flat), torch.zeros_like(self.dense_flat)) if adam else (None, None)
        self.adam_step = 1
        self.user_tower = ut = Tower(cfg, cfg.user_dims, self.dense_flat, self.dense_accum, lay.blocks["user.W0"].offset, dev)
        self.item_tower = it = Tower(cfg, cfg.item_dims, self.dense_flat, self.dense_accum, lay.blocks["item.W0"].offset, dev, rows=bi)
        grad_slabs = {}                          # segment name -> (its gradient slabs, their count): the segment loop below
        for side, tower in (("user", ut), ("item", it)):
            for l in range(tower.n_layers):
                grad_slabs[f"{side}.W{l}"] = (tower.dw_slabs[l], tower.n_slabs)
                grad_slabs[f"{side}.b{l}"] = (tower.db_slabs[l], tower.n_slabs)
        self.ws = torch.empty(ops.retrieval_workspace_bytes(b, bi, sd), dtype=torch.uint8, device=dev)
        # a pairwise retrieval loss: its kernel family's kind and its own workspace (allocated only with the option on)
        self.pairwise_kind = PAIRWISE_KIND_OF_LOSS.get(cfg.retrieval_loss)
        self.pairwise_ws = None
        if self.pairwise_kind is not None:
            self.pairwise_ws = torch.empty(ops.retrieval_pairwise_workspace_bytes(b, bi, sd), dtype=torch.uint8, device=dev)
        self.lse = torch.empty(b, device=dev)
        self.per_row = torch.empty(b, device=dev)
        self.loss = torch.empty(1, device=dev)
        self.oob = torch.zeros(1, dtype=torch.int32, device=dev)
        # mixed: the step's candidate ids and (once set_item_frequencies ran) their probabilities under the mixture of the two
        # candidate streams, both written by the sampler launch; the frequency vectors and the alias table of the unigram sampler
        self.cand_ids = torch.empty(bi, dtype=torch.int64, device=dev) if self.mixed else None
        self.cand_prob = torch.empty(bi, device=dev) if self.mixed else None
        self.item_freq = self.sampler_prob = self.alias = None
        # streaming frequency estimator: the sketch (optimizer-like state: checkpointed) and the in-batch candidates'
        # estimated probabilities, which go to the scorer as cand_prob (mixed: the estimator overwrites ``cand_prob``)
        self.freq_on = cfg.sampling_bias_estimator == "streaming"
        self.freq_sketch = ops.new_frequency_sketch(cfg.freq_hashes, cfg.freq_slot_count, dev) if self.freq_on else None
        self.freq_prob = torch.empty(b, device=dev) if self.freq_on else None
        self._freq_step = -1                     # the step (0-based) whose estimator launch has run
        # the embedding tables, one record each (EmbeddingTable: table, optimizer state, sort plan); a table that is off is None
        user = EmbeddingTable.new(cfg, dev, "user", TID_USER_TABLE, cfg.n_users, ops.SparsePlan(b, dev))
        item = EmbeddingTable.new(cfg, dev, "item", TID_ITEM_TABLE, cfg.n_items, ops.SparsePlan(bi, dev))
        cat = title = history = None
        if cfg.n_category_buckets:
            cat = EmbeddingTable.new(cfg, dev, "cat", TID_CATEGORY_TABLE, cfg.n_category_buckets, ops.SparsePlan(b, dev))
        # pooled item-title feature: the bag table with its optimizer state, every item's token row (all padding until
        # set_item_titles), and the per-step buffers the bag launches fill - the slot tokens the sort plan sorts, the pooling
        # scales, and (mean / sqrtn) the scaled gradient rows
        self.item_titles = self.title_ids = self.title_inv = self.title_gs = None
        if cfg.n_title_buckets:
            lt = cfg.title_max_tokens
            self.item_titles = torch.full((cfg.n_items, lt), -1, dtype=torch.int32, device=dev)
            title = EmbeddingTable.new(cfg, dev, "title", TID_TITLE_TABLE, cfg.n_title_buckets, ops.BagPlan(bi, lt, dev),
                                       {"item_titles": self.item_titles})
            self.title_ids = torch.empty(bi * lt, dtype=torch.int64, device=dev)
            self.title_inv = torch.empty(bi, device=dev)
            self.title_gs = torch.empty(bi, d, device=dev) if cfg.title_pooling != "sum" else None
        # pooled user-history feature: the mirror on the user side - a [n_items, dim] table of its own with its optimizer state,
        # every user's history row (all padding until set_user_histories) and the per-step buffers of the bag launches
        self.user_history = self.history_ids = self.history_inv = self.history_gs = None
        self.history_attn = self.history_weights = self.history_pooled = self.history_slot_grads = self._ha_slabs = None
        self.gru_W = self.gru_U = self.gru_b = self._gru_bufs = self._gru_slabs = self._gru_scratch = None
        self.sa_Wqk = self.sa_Wvo = self.sa_p = self._sa_bufs = self._sa_slabs = self._sa_scratch = None
        if cfg.user_history_len:
            lh = cfg.user_history_len
            self.user_history = torch.full((cfg.n_users, lh), -1, dtype=torch.int32, device=dev)
            self.history_ids = torch.empty(b * lh, dtype=torch.int64, device=dev)
            if self._attn_on:
                # attention pooling: the slots' gradient rows differ, so the update takes one row per slot through a plain sort
                # plan; the step keeps the weights and the pooled rows for the backward launch, which also writes the slabs of
                # the attention vector's dense segment
                plan = ops.SparsePlan(b * lh, dev)
                self.history_attn = lay.blocks["history_attn"].view(self.dense_flat)
                self.history_weights = torch.empty(b, lh, device=dev)
                self.history_pooled = torch.empty(b, d, device=dev)
                self.history_slot_grads = torch.zeros(b * lh, d, device=dev)
                ns = ops.history_attention_num_slabs(b)
                self._ha_slabs = torch.empty(ns, self.history_attn.numel(), device=dev)
                grad_slabs["history_attn"] = (self._ha_slabs, ns)
            elif self._gru_on:
                # GRU encoder: one gradient row per slot through a plain sort plan, as under attention; the step keeps the slot
                # rows, the gate activations and the states (ops.GruBuffers: 48 * b * lh * d bytes with the backward's da / dg)
                # and the gradient GEMMs write the slabs of the four dense segments
                plan = ops.SparsePlan(b * lh, dev)
                self.gru_W, self.gru_U, self.gru_b = (lay.blocks[f"history_gru.{k}"].view(self.dense_flat) for k in ("W", "U", "b"))
                self._gru_bufs = ops.GruBuffers(b, lh, d, dev)
                self._gru_bufs.batch_ids = self.history_ids
                self.history_slot_grads = torch.zeros(b * lh, d, device=dev)
                ns = ops.dense_bwd_num_slabs(b * lh)
                self._gru_slabs = (torch.empty(ns, d, 3 * d, device=dev), torch.empty(ns, d, 3 * d, device=dev),
                                   torch.empty(2, ns, 3 * d, device=dev))
                grad_slabs["history_gru.W"], grad_slabs["history_gru.U"] = (self._gru_slabs[0], ns), (self._gru_slabs[1], ns)
                grad_slabs["history_gru.b_i"], grad_slabs["history_gru.b_r"] = (self._gru_slabs[2][0], ns), (self._gru_slabs[2][1], ns)
            elif self._sa_on:
                # self-attention encoder: one gradient row per kept slot through a plain sort plan, as under attention; the step
                # keeps the newest rows, the queries, the pooled rows and the weights (ops.SelfAttnBuffers: nothing of b * lh * d);
                # the gradient GEMMs write the slabs of the two kernels' segments, the pool backward launch those of p
                plan = ops.SparsePlan(b * lh, dev)
                hh = cfg.history_heads
                self.sa_Wqk, self.sa_Wvo, self.sa_p = (lay.blocks[f"history_sa.{k}"].view(self.dense_flat) for k in ("Wqk", "Wvo", "p"))
                self._sa_bufs = ops.SelfAttnBuffers(b, lh, d, hh, dev)
                self._sa_bufs.batch_ids = self.history_ids
                self.history_slot_grads = torch.zeros(b * lh, d, device=dev)
                ns, nsp = ops.dense_bwd_num_slabs(b), ops.history_self_attention_num_slabs(b)
                self._sa_slabs = (torch.empty(ns, d, hh * d, device=dev), torch.empty(ns, hh * d, d, device=dev),
                                  torch.empty(nsp, hh * lh, device=dev))
                grad_slabs["history_sa.Wqk"], grad_slabs["history_sa.Wvo"] = (self._sa_slabs[0], ns), (self._sa_slabs[1], ns)
                grad_slabs["history_sa.p"] = (self._sa_slabs[2], nsp)
            else:
                plan = ops.BagPlan(b, lh, dev)
                self.history_inv = torch.empty(b, device=dev)
                self.history_gs = torch.empty(b, d, device=dev) if cfg.history_pooling != "sum" else None
            history = EmbeddingTable.new(cfg, dev, "history", TID_HISTORY_TABLE, cfg.n_items, plan, {"user_history": self.user_history})
        self.tables = {t.prefix: t for t in (user, item, cat, title, history) if t is not None}
        # the records' fields under the names the rest of the project reads (here and for the feature sides below)
        self.user_table, self.user_accum, self.user_m, self.user_v, self.user_plan = _table_fields(user)
        self.item_table, self.item_accum, self.item_m, self.item_v, self.item_plan = _table_fields(item)
        self.cat_table, self.cat_accum, self.cat_m, self.cat_v, self.cat_plan = _table_fields(cat)
        self.title_table, self.title_accum, self.title_m, self.title_v, self.title_plan = _table_fields(title)
        self.history_table, self.history_accum, self.history_m, self.history_v, self.history_plan = _table_fields(history)
        # what the configured optimizer's calls take for the tables of the pairs' ids (EmbeddingTable.opt_args) - every pointer is
        # fixed from here on, so the list is built once (the category row's gradient is the item-tower input gradient itself)
        trio = [(user, ut.demb), (item, it.demb)] + ([(cat, it.demb)] if cat is not None else [])
        self._opt_tables = tabs = [t.opt_args(g) for t, g in trio]
        for t in (user, item, cat, title, history):
            if t is not None:
                setattr(self, f"{t.prefix}_row_accum", t.row_accum)
        # numeric side features, per side: the fixed feature matrix with its normalisation (zeros / mean 0 / inv_std 1 until the
        # setter ran: z = 0, nothing is added), the projection kernel (a view of dense_flat), the step's normalised rows (kept for
        # the backward launch) and the gradient slabs the dense optimizer segment sums
        self.sides = {}
        for side, f, rows, nb, tower in (("user", cfg.n_user_features, cfg.n_users, b, ut), ("item", cfg.n_item_features, cfg.n_items, bi, it)):
            if f:
                ns = ops.dense_features_num_slabs(nb)
                self.sides[side] = fs = FeatureSide(side, torch.zeros(rows, f, device=dev), torch.zeros(f, device=dev), torch.ones(f, device=dev),
                                                    lay.blocks[f"P_{side}"].view(self.dense_flat), torch.empty(nb, f, device=dev),
                                                    torch.empty(ns, f, d, device=dev), ns, tower)
                grad_slabs[f"P_{side}"] = (fs.slabs, ns)
        self.user_features, self.user_feature_mean, self.user_feature_inv_std, self.P_user, self._fz_user, self._fslabs_user = \
            _side_fields(self.sides.get("user"))
        self.item_features, self.item_feature_mean, self.item_feature_inv_std, self.P_item, self._fz_item, self._fslabs_item = \
            _side_fields(self.sides.get("item"))
        self._feature_sides = [(fs.side, fs.P, fs.slabs, fs.n_slabs) for fs in self.sides.values()]
        # rating head: the four parameters (views of dense_flat), the step's predictions and hidden activations (kept for the
        # backward launch) and the gradient slabs of the two dense segments (W1 | w2 with l2, b1 | b2 without)
        self.W1_rating = self.w2_rating = self.b1_rating = self.b2_rating = None
        self.rating_pred = self._r_h = self._r_kslabs = self._r_bslabs = self._r_se = None
        self.eval_rating_se = self.eval_rating_count = None
        if self.rating_on:
            self.W1_rating, self.w2_rating, self.b1_rating, self.b2_rating = \
                (lay.blocks[f"head.{k}"].view(self.dense_flat) for k in ("W1", "w2", "b1", "b2"))
            ns = ops.rating_head_num_slabs(b)
            self.rating_pred = torch.zeros(b, device=dev)
            self._r_h = torch.empty(b, rh, device=dev)
            self._r_kslabs = torch.empty(ns, lay.segment("head.kernels").size, device=dev)
            self._r_bslabs = torch.empty(ns, lay.segment("head.biases").size, device=dev)
            self._r_se = torch.zeros(ns, device=dev)
            grad_slabs["head.kernels"], grad_slabs["head.biases"] = (self._r_kslabs, ns), (self._r_bslabs, ns)
        # cross layers: the parameters (views of dense_flat) and ONE gradient-slab array for all layers of both towers, laid out
        # like the parameters, so that two dense segments - every kernel (l2 like any kernel), every bias - sum it
        self._c_slabs = None
        self._c_nslabs = 0
        if ncl:
            kernels, biases = lay.segment("cross.kernels"), lay.segment("cross.biases")
            self._c_nslabs = ns = ops.cross_num_slabs(bi)
            self._c_slabs = torch.empty(ns * kernels.stride, device=dev)
            for side, tower in (("user", ut), ("item", it)):
                ws = [lay.blocks[f"cross.{side}.W{l}"] for l in range(ncl)]
                bs = [lay.blocks[f"cross.{side}.b{l}"] for l in range(ncl)]
                tower.set_cross([w.view(self.dense_flat) for w in ws], [x.view(self.dense_flat) for x in bs],
                                [self._c_slabs[w.offset - kernels.lo:] for w in ws], [self._c_slabs[x.offset - kernels.lo:] for x in bs],
                                ns, kernels.stride)
            grad_slabs["cross.kernels"], grad_slabs["cross.biases"] = (self._c_slabs, ns), (self._c_slabs[biases.lo - kernels.lo:], ns)
        # layer normalisation: gamma / beta per hidden layer (views of dense_flat) and ONE gradient-slab array for all layers of
        # both towers, laid out like the parameters, which the block's one dense segment sums
        self._ln_slabs = None
        self._ln_nslabs = 0
        if cfg.layer_norm:
            norm = lay.segment("norm")
            self._ln_nslabs = ns = ops.layer_norm_num_slabs(bi)
            self._ln_slabs = torch.empty(ns * norm.stride, device=dev)
            for side, tower in (("user", ut), ("item", it)):
                gs = [lay.blocks[f"norm.{side}.g{l}"] for l in range(tower.n_layers - 1)]
                bs = [lay.blocks[f"norm.{side}.b{l}"] for l in range(tower.n_layers - 1)]
                tower.set_layer_norm([g.view(self.dense_flat) for g in gs], [x.view(self.dense_flat) for x in bs],
                                     [self._ln_slabs[g.offset - norm.lo:] for g in gs], [self._ln_slabs[x.offset - norm.lo:] for x in bs],
                                     ns, norm.stride)
            grad_slabs["norm"] = (self._ln_slabs, ns)
        # time context: the table (a view of dense_flat), the step's kept row indices and the fully reduced gradient the
        # backward launch writes - the ONE "slab" of the table's dense segment
        self.time_on = bool(cfg.time_fields)
        self.time_table = self._time_idx = self._time_grad = None
        if self.time_on:
            self.time_table = lay.blocks["time_table"].view(self.dense_flat)
            self._time_idx = torch.empty(b, len(cfg.time_fields), dtype=torch.int32, device=dev)
            self._time_grad = torch.empty_like(self.time_table)
            grad_slabs["time_table"] = (self._time_grad, 1)
        # high priority = a hardware queue of its own (ROCm pools queues per priority): the sort plans always run BESIDE
        # the main stream's kernels, whatever other streams the process has created
        self._side = torch.cuda.Stream(device=dev, priority=-1)
        # where the sort plan runs: in front of the forward pass on the main stream (default since the partitioned sort:
        # ~6 us of kernel), or beside it on the side stream (TT_PLAN_STREAM=side: two cross-stream waits per step, which
        # cost more than the kernel: cfg3 step 0.687-0.689 ms against 0.677-0.681 ms; DESIGN.md section 4, K2 plan)
        self.plan_on_side_stream = os.environ.get("TT_PLAN_STREAM", "main") == "side"
        self.step_index = 0                      # counter of the dropout stream (global batch row = step*batch + r)
        # the step the learning-rate schedule is read at: the one in progress - forward_backward (or the composite call) sets it
        # before it counts step_index on, so apply_gradients still sees the step whose gradients it applies
        self._lr_step = 0
        # cfg.global_clipnorm: the buffer list of the two clip launches, their workspace and [norm, scale] - built on first use
        self._clip = self._clip_ws = self._clip_stats = None
        # K1 inside the first tower layer's GEMMs (0: gather2 launch + acts[0]).  Every 64-column tile of the first layer reads
        # the embedding rows through the ids again: up to 256 columns that costs less than materialising them (cfg3: 13.6 us
        # of gather against +3.6 us in the GEMMs; cfg4 1.875 vs 1.881 ms), at 512 columns it costs more (cfg5: the layer-0
        # launches 99 us longer, the gather 55 us; step 15.28 vs 15.24 ms) - r03 A/B
        # (r04: at small batches the gather launch's fixed cost decides - the reference's own config, [512, 256, 128] at batch 1024:
        # 0.1631-0.1638 ms fused against 0.1644-0.1654 with the gather launch)
        self.fuse_lookup = os.environ.get("TT_FUSE_LOOKUP", "1" if (cfg.tower_dims[0] < 512 or cfg.batch_size <= 2048) else "0") != "0"
        if cfg.n_title_buckets:                  # the pooled titles are added to the materialised item-tower input (_tower_inputs)
            self.fuse_lookup = False
        if cfg.user_history_len:                 # the user tower's input is one bag launch: user row + pooled history (_tower_inputs)
            self.fuse_lookup = False
        if self._feature_sides:                  # the projected features are added to the materialised tower inputs (_tower_inputs)
            self.fuse_lookup = False
        if cfg.cross_layers:                     # the cross layers read the materialised tower inputs (Tower.forward)
            self.fuse_lookup = False
        if self.time_on:                         # the time rows are added to the materialised user-tower input (_tower_inputs)
            self.fuse_lookup = False
        self.fuse_sort = os.environ.get("TT_FUSE_SORT", "1") != "0"   # the optimizer launch sorts the ids itself (no plan launch)
        self.fuse_optimizer = True               # sparse + dense optimizer in one launch (False: dense_update, sparse_update2 [, cat])
        # the whole step behind ONE C call (tt_train_step_f32: the same launches - eight at cfg3 -, enqueued in C - one FFI crossing per step
        # instead of nine; cfg1 is host-bound).  TT_COMPOSITE_STEP=0: the Python sequence of the separate entry points.
        self.use_composite = os.environ.get("TT_COMPOSITE_STEP", "1") != "0"
        if cfg.layer_norm:                       # tt_train_step_f32 cannot describe the normalisation launches between the layers
            self.use_composite = False
        self._cstep = None
        self._id_bucket_ws = None
        # layers 1 and 0 of the backward pass in ONE launch (tt_tower_bwd2_batched_f32: the lower layer's tiles wait inside the
        # launch for the rows of dz they read); TT_BWD2=0: one launch per layer
        self.bwd2_ws = None
        if (os.environ.get("TT_BWD2", "0") != "0" and cfg.symmetric and len(cfg.tower_dims) >= 2 and not cfg.layer_norm
                and ops.tower_bwd2_supported(b, d, cfg.tower_dims[0], cfg.tower_dims[1])):
            self.bwd2_ws = ops.tower_bwd2_workspace(b, dev)
        self.flag_poll_every = 50                # steps between asynchronous polls of the out-of-range flag (0 = never)
        self._oob_host = self._oob_event = None
        self._oob_step = -1
        # r04: the one-launch optimizer gives every row range of a table to ONE workgroup.  Ids uniform over the rows put
        # batch / groups ~ 64-270 ids into each; a vocabulary in order of frequency (what StringLookup.adapt builds) puts a third
        # of a power-law batch into the first range, and that workgroup is the launch (cfg3, ids ~ rows * u^4: 12 -> 169 us, step
        # 0.560 -> 0.746 ms).  Every flag_poll_every steps a one-workgroup-per-table probe (tt_id_range_load) counts the batch's
        # ids per range; its result is read from pinned memory when it has landed, never waited for, and while some range holds
        # more than skew_limit ids the steps take the plan launch + tt_optimizer_step_f32 instead (the sorted list is spread
        # over all CUs whatever the ids: 38 us at cfg3), and return to the one launch when the load falls below 3/4 of the limit.
        # 384: the overloaded workgroup costs ~0.066 us per id at dim 128, the plan path ~25 us more than the balanced launch
        # (the reference's own config, batch 1024, power-law ids, largest range 498-541: 0.2053 ms without the probe, 0.1834 at
        # limit 512 - flapping -, 0.1694 at 384 and 256; cfg1's 177 ids must NOT switch: its Python sequence of launches is
        # host-bound, 0.060 -> 0.090 ms).  TT_SKEW_LIMIT=0: never switch.
        self.skew_limit = int(os.environ.get("TT_SKEW_LIMIT", "384"))
        self.range_load = 0                      # largest row-range load the last finished probe saw
        self._skew_state = False
        self._skew_dev = self._skew_host = self._skew_event = None
        self.dropout_seed = 0 if seed is None else seed
        # the dense optimizer's segments, in the layout's order: parameter range, gradient slabs, l2 and slab stride are stated
        # once, and the accumulator's / the moments' views are cut with the same range
        self._segs = []
        self._adam_segs = [] if adam else None
        for seg in lay.segments:
            lo, hi = seg.lo, seg.hi
            (slabs, ns), reg = grad_slabs[seg.name], cfg.l2_regularization if seg.l2 else 0.0
            self._segs.append(ops.make_dense_seg(self.dense_flat[lo:hi], None if self.dense_accum is None else self.dense_accum[lo:hi],
                                                 slabs, ns, reg, slab_stride=seg.stride))
            if adam:
                self._adam_segs.append(ops.make_adam_seg(self.dense_flat[lo:hi], self.dense_m[lo:hi], self.dense_v[lo:hi], slabs, ns,
                                                         reg, slab_stride=seg.stride))
        # the segments that ride in the table calls of lazy Adam (its own form of them) and of row-wise Adagrad; None: SGD and
        # Adagrad, which update the dense parameters in a launch of their own or inside their one fused launch
        rowwise = cfg.optimizer == "rowwise_adagrad"
        self._riding = self._adam_segs if adam else self._segs if rowwise else None
        # how a step groups the id tables into plan-fed calls (EmbeddingTable.update), as (tables, riding segments) - the segments
        # ride with the first call.  Lazy Adam: every table in ONE call; row-wise Adagrad: user + item in one, then the category
        # table alone; mixed sampling, whose two plans hold different id counts (B and B + N): one call per table; SGD / Adagrad
        # otherwise: the category table, behind the unfused sparse_update2_ (their other forms are single fused launches)
        groups = [tabs[:1], tabs[1:]] if self.mixed else [tabs] if adam else [tabs[:2], tabs[2:]] if rowwise else [tabs[2:]]
        self._table_calls = [(g, (self._riding or []) if k == 0 else []) for k, g in enumerate(groups) if g]
        if seed is not None:
            self.init_synthetic(seed)

    # ------------------------------------------------------------------ init
    def init_synthetic(self, seed: int):
        """Keras defaults (Embedding U(-0.05,0.05), Dense Glorot-uniform, zero bias) from the counter-based
        generator: identical, bit for bit, to oracle.two_tower.synthetic_state(seed, ...)."""
        for t in self.tables.values():
            t.init_synthetic(self.cfg, seed)
        self.dense_flat.zero_()
        self._fill_constant_blocks()
        for blk in self.layout.blocks.values():                # Glorot-uniform kernels, zero biases, the time table like an Embedding
            if blk.glorot is not None:
                _glorot_uniform_(blk.view(self.dense_flat), seed, *blk.glorot)
            elif blk.embedding is not None:
                ops.fill_uniform_(blk.view(self.dense_flat), seed, blk.embedding, -0.05, 0.1)
        if self.dense_accum is not None:
            self.dense_accum.fill_(self.cfg.adagrad_initial_accumulator)
        if self.dense_m is not None:
            self.dense_m.zero_(), self.dense_v.zero_()
        self.adam_step = 1

    def _fill_constant_blocks(self):
        """The parameters that start at a constant other than zero (``DenseBlock.fill``: the layer normalisation's gammas)."""
        for blk in self.layout.blocks.values():
            if blk.glorot is None and blk.fill != 0.0:
                blk.view(self.dense_flat).fill_(blk.fill)

    def init_rating_bias(self, x: float):
        """Sets the head's output bias b2 (train.py: the mean finite training rating, so that the head starts from the constant
        predictor instead of 0)."""
        if not self.rating_on:
            raise ValueError("init_rating_bias: the model has no rating head (cfg.rating_weight == 0)")
        if not math.isfinite(float(x)):
            raise ValueError("init_rating_bias: x must be finite")
        self.b2_rating.fill_(float(x))

    def synthetic_batch(self, seed: int, step: int, variant: str = "U", out=None):
        b = self.cfg.batch_size
        if out is None:
            out = (torch.empty(b, dtype=torch.int64, device=self.dev), torch.empty(b, dtype=torch.int64, device=self.dev))
        ops.fill_ids_(out[0], seed, TID_USER_IDS, self.cfg.n_users, variant, start=step * b)
        ops.fill_ids_(out[1], seed, TID_ITEM_IDS, self.cfg.n_items, variant, start=step * b)
        return out

    def synthetic_categories(self, seed: int, step: int, variant: str = "Z", out=None):
        """Category bucket of every pair of synthetic step ``step`` (power-law by default: a few big categories)."""
        b = self.cfg.batch_size
        if out is None:
            out = torch.empty(b, dtype=torch.int64, device=self.dev)
        ops.fill_ids_(out, seed, TID_CATEGORY_IDS, self.cfg.n_category_buckets, variant, start=step * b)
        return out

    def synthetic_timestamps(self, seed: int, step: int, out=None) -> torch.Tensor:
        """The int64 timestamps of synthetic step ``step``, uniform over [time_min, time_max] from the counter-based generator
        (tensor id 61, elements step * batch ..)."""
        b, cfg = self.cfg.batch_size, self.cfg
        if out is None:
            out = torch.empty(b, dtype=torch.int64, device=self.dev)
        ops.fill_ids_(out, seed, TID_TIME_BASE + 1, cfg.time_max - cfg.time_min + 1, "U", start=step * b)
        return out.add_(cfg.time_min)

    def synthetic_item_titles(self, seed: int, variant: str = "Z") -> torch.Tensor:
        """A synthetic [n_items, title_max_tokens] int32 token matrix from the id generator: power-law tokens (a few frequent
        words), 1..title_max_tokens of them per item, the rest padding."""
        n, lt = self.cfg.n_items, self.cfg.title_max_tokens
        tok = torch.empty(n * lt, dtype=torch.int64, device=self.dev)
        length = torch.empty(n, dtype=torch.int64, device=self.dev)
        ops.fill_ids_(tok, seed, TID_TITLE_IDS, self.cfg.n_title_buckets, variant)
        ops.fill_ids_(length, seed, TID_TITLE_LENGTHS, lt, "U")
        slot = torch.arange(lt, device=self.dev)
        return torch.where(slot[None, :] <= length[:, None], tok.view(n, lt), -1).to(torch.int32)

    def set_item_titles(self, tokens: torch.Tensor):
        """tokens [n_items, title_max_tokens] int32: the hashed title tokens of every item (``data.title_tokens``), -1 = no
        token in that slot.  Tokens outside [0, n_title_buckets) are skipped by the kernels and raise through ``check_ids``."""
        if self.item_titles is None:
            raise ValueError("set_item_titles: the model has no title feature (cfg.n_title_buckets == 0)")
        if tuple(tokens.shape) != tuple(self.item_titles.shape) or tokens.dtype != torch.int32:
            raise ValueError(f"set_item_titles: tokens must be int32 {list(self.item_titles.shape)} (n_items, title_max_tokens), "
                             f"got {tokens.dtype} {list(tokens.shape)}")
        self.item_titles.copy_(tokens)

    def set_user_histories(self, tokens: torch.Tensor):
        """tokens [n_users, user_history_len] int32: every user's last training items (``data.user_histories``), -1 = no item in
        that slot.  Items outside [0, n_items) are skipped by the kernel and raise through ``check_ids``."""
        if self.user_history is None:
            raise ValueError("set_user_histories: the model has no history feature (cfg.user_history_len == 0)")
        if tuple(tokens.shape) != tuple(self.user_history.shape) or tokens.dtype != torch.int32:
            raise ValueError(f"set_user_histories: tokens must be int32 {list(self.user_history.shape)} (n_users, user_history_len), "
                             f"got {tokens.dtype} {list(tokens.shape)}")
        self.user_history.copy_(tokens)

    def _synthetic_features(self, seed: int, tid: int, rows: int, f: int) -> torch.Tensor:
        out = torch.empty(rows, f, device=self.dev)
        if f:
            ops.fill_uniform_(out, seed, tid, 0.0, 5.0)
        return out

    def synthetic_user_features(self, seed: int) -> torch.Tensor:
        """A synthetic [n_users, n_user_features] f32 matrix, U(0, 5) from the counter-based generator (tensor id 14)."""
        return self._synthetic_features(seed, TID_USER_FEATURES, self.cfg.n_users, self.cfg.n_user_features)

    def synthetic_item_features(self, seed: int) -> torch.Tensor:
        """A synthetic [n_items, n_item_features] f32 matrix, U(0, 5) from the counter-based generator (tensor id 15)."""
        return self._synthetic_features(seed, TID_ITEM_FEATURES, self.cfg.n_items, self.cfg.n_item_features)

    def _set_features(self, side: str, x, mean, inv_std):
        import numpy as np
        what = f"set_{side}_features"
        fs = self.sides.get(side)
        if fs is None:
            raise ValueError(f"{what}: the model has no numeric {side} features (cfg.n_{side}_features == 0)")
        dst = fs.features
        a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        if tuple(a.shape) != tuple(dst.shape):
            raise ValueError(f"{what}: x must be {list(dst.shape)} (rows, n_{side}_features), got {list(a.shape)}")
        a = np.ascontiguousarray(a, dtype=np.float32)
        if not np.isfinite(a).all():
            raise ValueError(f"{what}: x holds non-finite values")
        if (mean is None) != (inv_std is None):
            raise ValueError(f"{what}: mean and inv_std are given both or neither")
        if mean is None:
            mean, inv_std = ops.adapt_normalization(a)
        stats = []
        for t, name in ((mean, "mean"), (inv_std, "inv_std")):
            t = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t), dtype=np.float32).reshape(-1)
            if t.size != a.shape[1] or not np.isfinite(t).all():
                raise ValueError(f"{what}: {name} must hold {a.shape[1]} finite entries")
            stats.append(t)
        dst.copy_(torch.from_numpy(a))
        fs.mean.copy_(torch.from_numpy(stats[0]))
        fs.inv_std.copy_(torch.from_numpy(stats[1]))

    def set_user_features(self, x, mean=None, inv_std=None):
        """x [n_users, n_user_features]: every user's numeric features (finite; ``data.rating_features``).  ``mean`` / ``inv_std``
        [F]: the normalisation's statistics; both None: adapted from x (``ops.adapt_normalization``, Keras Normalization.adapt)."""
        self._set_features("user", x, mean, inv_std)

    def set_item_features(self, x, mean=None, inv_std=None):
        """x [n_items, n_item_features]: every item's numeric features; see ``set_user_features``."""
        self._set_features("item", x, mean, inv_std)

    def set_item_frequencies(self, freq):
        """freq [n_items]: every item's probability of being an in-batch candidate (its share of the training pairs; train.py's
        ``--correct-sampling-bias`` vector).  Mixed negative sampling only: from the next step on the sampler launch writes every
        candidate's probability under the mixture of the in-batch and the sampled stream and the scorer applies the logQ
        correction with it.  With negative_sampler="unigram" this also builds the sampler: the distribution freq^unigram_power /
        sum (NumPy f64), its f32 vector (the kernel's ``sampler_prob``) and Walker's alias table (``ops.build_alias_table``)."""
        import numpy as np
        if not self.mixed:
            raise ValueError("set_item_frequencies: the trainer does not sample negatives (cfg.candidate_sampling == 'in_batch'); "
                             "pass candidate_sampling_probability to step() instead")
        f = freq.detach().cpu().numpy() if torch.is_tensor(freq) else np.asarray(freq)
        f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
        if f.size != self.cfg.n_items or not np.isfinite(f).all() or (f < 0).any():
            raise ValueError(f"set_item_frequencies: freq must hold n_items = {self.cfg.n_items} finite, non-negative entries")
        self.item_freq = torch.from_numpy(f.astype(np.float32)).to(self.dev)
        if self.cfg.negative_sampler == "unigram":
            w = f ** self.cfg.unigram_power if self.cfg.unigram_power != 0.0 else np.ones_like(f)
            if not w.sum() > 0:
                raise ValueError("set_item_frequencies: the unigram sampler needs some positive frequency")
            thr, idx = ops.build_alias_table(w)
            self.sampler_prob = torch.from_numpy((w / w.sum()).astype(np.float32)).to(self.dev)
            self.alias = (torch.from_numpy(thr).to(self.dev), torch.from_numpy(idx).to(self.dev))

    def _check_categories(self, category_ids):
        if (category_ids is None) != (self.cat_table is None):
            raise ValueError("category_ids must be given exactly when cfg.n_category_buckets > 0")
        if category_ids is not None and category_ids.numel() != self.cfg.batch_size:
            raise ValueError(f"category_ids must have {self.cfg.batch_size} entries")

    def _check_batch(self, *id_tensors):
        """The tower buffers hold exactly cfg.batch_size rows: more ids would write past them, fewer would leave stale
        rows that the scorer still reads."""
        b = self.cfg.batch_size
        for t in id_tensors:
            if t is not None and t.numel() != b:
                raise ValueError(f"batch must have exactly {b} entries (got {t.numel()}): the kernels' buffers are sized "
                                 "for cfg.batch_size; pad or drop a ragged last batch")

    def _lookups(self, user_ids, item_ids, category_ids):
        """K1 fused into the towers' first layer (fwd GEMM and dW GEMM read the table rows themselves): the
        [batch, dim] tower inputs are never written to HBM.  None when the batch is too long for the fused form.  Mixed
        sampling's train step passes ``cand_ids`` - the trainer's own list, one id per row of the item tower - as ``item_ids``."""
        self._check_batch(user_ids, None if item_ids is self.cand_ids else item_ids, category_ids)
        if not self.fuse_lookup or self.item_tower.rows > ops.MAX_FUSED_LOOKUP_ROWS:
            return None
        return (ops.make_lookup(self.user_table, user_ids, oob_flag=self.oob),
                ops.make_lookup(self.item_table, item_ids, self.cat_table, category_ids, self.oob))

    def _tower_inputs(self, user=None, item=None, *, category_ids=None, exclude=None, keep: bool = False, features_only: bool = False,
                      timestamps=None):
        """Materialised tower-input rows (no fused lookup), and the ONE place that knows what is summed into them: the id's table
        row + the hashed category's row (item) + the pooled title rows (item) + the pooled, attended or GRU-encoded history (user) + the
        time rows of the pairs' ``timestamps`` (user; without a history ONE launch with the user row as its base, else added
        behind the history launch) + the projected numeric features.
        ``user`` / ``item`` = (ids, rows to write) or None: any number of ids, either side alone.
        ``exclude``: the items the history launch leaves out (the train step's positives); ``keep``: the train step - the slot
        tokens, pooling scales and normalised feature rows stay for the backward launches and the update; an inference pass
        writes none of those buffers, so it may run between a step's backward pass and its ``apply_gradients``.
        ``features_only``: the rows already hold everything but the numeric features (``item_corpus_embeddings``)."""
        cfg = self.cfg
        if features_only:
            pass
        elif self.history_table is not None:     # the item gather, then ONE launch for the user side: user row + pooled history
            if item is not None:
                ops.embedding_gather(self.item_table, item[0], out=item[1], oob_flag=self.oob)
            if user is not None and self._attn_on:   # (the weights and pooled rows of an inference pass are never read)
                ids, n = user[0], user[0].numel()
                ops.history_attention(self.history_table, self.user_history, self.history_attn, bag_rows=ids, exclude=exclude,
                                      base=(self.user_table, ids), out=user[1], batch_ids=self.history_ids if keep else None,
                                      weights=self.history_weights[:n], pooled=self.history_pooled[:n], oob_flag=self.oob)
            elif user is not None and self._gru_on:
                self._history_gru(user, exclude, keep)
            elif user is not None and self._sa_on:
                self._history_self_attention(user, exclude, keep)
            elif user is not None:
                ops.history_bag(self.history_table, self.user_history, bag_rows=user[0], exclude=exclude, base=(self.user_table, user[0]),
                                pooling=cfg.history_pooling, out=user[1], batch_ids=self.history_ids if keep else None,
                                inv=self.history_inv if keep else None, oob_flag=self.oob)
            if user is not None and self.time_on:
                self._time_context(timestamps, user, keep, base=False)
        elif self.time_on:                       # the item gather, then ONE launch for the user side: user row + time rows
            if item is not None:
                ops.embedding_gather(self.item_table, item[0], out=item[1], oob_flag=self.oob)
            if user is not None:
                self._time_context(timestamps, user, keep, base=True)
        elif user is not None and item is not None and user[0].numel() == item[0].numel():
            ops.embedding_gather2(self.user_table, user[0], user[1], self.item_table, item[0], item[1], self.oob)
        else:
            for table, side in ((self.user_table, user), (self.item_table, item)):
                if side is not None:
                    ops.embedding_gather(table, side[0], out=side[1], oob_flag=self.oob)
        if item is not None and not features_only:
            if category_ids is not None:
                ops.embedding_gather_add_(item[1], self.cat_table, category_ids, self.oob)
            if self.title_table is not None:
                ops.embedding_bag(self.title_table, self.item_titles, bag_rows=item[0], pooling=cfg.title_pooling, out=item[1],
                                  accumulate=True, batch_ids=self.title_ids if keep else None, inv=self.title_inv if keep else None,
                                  oob_flag=self.oob)
        probs = []                               # one launch for the sides that are present and have the feature
        for name, side in (("user", user), ("item", item)):
            fs = self.sides.get(name)
            if fs is not None and side is not None:
                probs.append((fs.features, side[0], fs.mean, fs.inv_std, fs.P, side[1], True, fs.z if keep else None))
        if probs:
            ops.dense_features(*probs, clip=cfg.feature_clip, oob_flag=self.oob)

    def _history_gru(self, user, exclude, keep: bool, chunk: int = 4096):
        """The GRU launches of ``_tower_inputs``: user row + the final state over the kept slots.  The train step (``keep``)
        runs on the step's kept buffers; an inference pass takes any number of ids, ``chunk`` bags at a time on ONE scratch of
        its own (allocated on first use, grown when a longer chunk comes), so it writes nothing a pending step still needs."""
        ids, out = user
        args = (self.history_table, self.user_history, self.gru_W, self.gru_U, self.gru_b)
        if keep:
            ops.history_gru(*args, bag_rows=ids, exclude=exclude, base=(self.user_table, ids), out=out, batch_ids=self.history_ids,
                            oob_flag=self.oob, keep=self._gru_bufs)
            return
        need = min(ids.numel(), chunk)
        if self._gru_scratch is None or self._gru_scratch.n_bags < need:
            self._gru_scratch = None
            self._gru_scratch = ops.GruBuffers(need, self.cfg.user_history_len, self.cfg.embedding_dim, self.dev, backward=False)
        for lo in range(0, ids.numel(), chunk):
            part = ids[lo:lo + chunk]
            ops.history_gru(*args, bag_rows=part, exclude=None if exclude is None else exclude[lo:lo + chunk],
                            base=(self.user_table, part), out=out[lo:lo + chunk], oob_flag=self.oob, scratch=self._gru_scratch)

    def _history_self_attention(self, user, exclude, keep: bool, chunk: int = 4096):
        """The self-attention launches of ``_tower_inputs``: user row + the attended history read at the newest kept item.  The
        train step (``keep``) runs on the step's kept buffers; an inference pass takes any number of ids, ``chunk`` bags at a
        time on ONE scratch of its own (allocated on first use, grown when a longer chunk comes): never more than chunk * H * D
        floats per buffer, and nothing a pending step still needs is written."""
        ids, out = user
        cfg = self.cfg
        args = (self.history_table, self.user_history, self.sa_Wqk, self.sa_Wvo, self.sa_p)
        if keep:
            ops.history_self_attention(*args, bag_rows=ids, exclude=exclude, base=(self.user_table, ids), out=out, oob_flag=self.oob,
                                       keep=self._sa_bufs)
            return
        need = min(ids.numel(), chunk)
        if self._sa_scratch is None or self._sa_scratch.n_bags < need:
            self._sa_scratch = None
            self._sa_scratch = ops.SelfAttnBuffers(need, cfg.user_history_len, cfg.embedding_dim, cfg.history_heads, self.dev,
                                                   backward=False)
        for lo in range(0, ids.numel(), chunk):
            part = ids[lo:lo + chunk]
            ops.history_self_attention(*args, bag_rows=part, exclude=None if exclude is None else exclude[lo:lo + chunk],
                                       base=(self.user_table, part), out=out[lo:lo + chunk], oob_flag=self.oob,
                                       scratch=self._sa_scratch)

    def _time_context(self, timestamps, user, keep: bool, base: bool):
        """The time launch of ``_tower_inputs``: the rows ``timestamps`` pick, summed, on top of the user row (``base``) or of
        what the history launch wrote; ``keep``: the row indices stay for ``_time_backward``."""
        cfg, (ids, out) = self.cfg, user
        ops.time_context(timestamps, self.time_table, cfg.time_fields, cfg.time_buckets, cfg.time_min, cfg.time_max, out=out,
                         accumulate=not base, base=(self.user_table, ids) if base else None,
                         idx_out=self._time_idx[:ids.numel()] if keep else None, oob_flag=self.oob)

    def _time_backward(self):
        """The time table's gradient, fully reduced, from the user tower's input gradient (demb) and the kept row indices: one
        launch after the towers' backward - the ONE slab of the table's dense segment."""
        ops.time_context_bwd(self._time_idx, self.user_tower.demb, self.cfg.time_fields, self.cfg.time_buckets, grad=self._time_grad)

    def _check_timestamps(self, timestamps, n: int | None = None, where: str = "step"):
        """``timestamps`` are required exactly when the model has the time features; int64 [n] on the device."""
        if self.time_on and timestamps is None:
            raise ValueError(f"{where}: the model has time features (cfg.time_fields = {self.cfg.time_fields}): pass "
                             "timestamps=<int64 [batch], seconds since the epoch, TIME_MISSING = none>")
        if not self.time_on and timestamps is not None:
            raise ValueError(f"{where}: timestamps were passed but the model has no time features (cfg.time_fields == ())")
        if timestamps is not None:
            ops._chk(timestamps, torch.int64, "timestamps", 1)
            n = self.cfg.batch_size if n is None else n
            if timestamps.numel() != n:
                raise ValueError(f"{where}: timestamps must have {n} entries (one per pair), got {timestamps.numel()}")

    def _features_backward(self):
        """The projection kernels' gradient slabs from the towers' input gradients (demb) and the kept normalised rows: one
        launch for both sides, after the towers' backward."""
        if self.sides:
            ops.dense_features_bwd(*[(fs.z, fs.tower.demb, fs.slabs) for fs in self.sides.values()])

    def _history_backward(self):
        """Attention pooling: the slots' gradient rows and the attention vector's gradient slabs from the user tower's input
        gradient (demb), one launch after the towers' backward - in front of the optimizer launches, which update the vector.
        GRU: the same from three launches - the reverse recurrence, then the slot rows with dW / db_i and dU / db_r as GEMMs.
        Self-attention: the same from four - two gradient GEMMs round the pool backward, then the newest rows' query share."""
        if self._attn_on:
            ops.history_attention_bwd(self.history_table, self.history_ids, self.history_weights, self.history_pooled,
                                      self.user_tower.demb, self.history_attn, self.cfg.user_history_len,
                                      slot_grads=self.history_slot_grads, dattn_slabs=self._ha_slabs)
        elif self._gru_on:                       # the recurrent backward launch and the two gradient GEMM launches
            dw, du, db = self._gru_slabs
            ops.history_gru_bwd(self._gru_bufs, self.user_tower.demb, self.gru_W, self.gru_U, slot_grads=self.history_slot_grads,
                                dw_slabs=dw, du_slabs=du, db_slabs=db)
        elif self._sa_on:                        # (dP, dWvo), the pool backward, (dxn, dWqk), the newest rows' += dxn: four launches
            dwqk, dwvo, dp = self._sa_slabs
            ops.history_self_attention_bwd(self._sa_bufs, self.user_tower.demb, self.sa_Wqk, self.sa_Wvo,
                                           slot_grads=self.history_slot_grads, dwqk_slabs=dwqk, dwvo_slabs=dwvo, dp_slabs=dp)

    def _outputs(self, towers, rows=None):
        """The embeddings of ``towers`` (whose forward pass has just run) as everything downstream sees them - scorer, metrics,
        serving: the last layer's output, L2-normalised into ``tower.unit`` when cfg.normalize_embeddings - one launch where the
        towers' row counts agree, else (mixed sampling's longer item tower) one per tower.  ``rows``: only the first rows[i]
        rows of towers[i] (a partial pass).  The ONE place that decides."""
        part = lambda bufs: tuple(bufs) if rows is None else tuple(x[:n] for x, n in zip(bufs, rows))
        xs = part(t.acts[-1] for t in towers)
        if not self.cfg.normalize_embeddings:
            return xs
        ys = part(t.unit for t in towers)
        if len(set(rows or [t.rows for t in towers])) == 1:
            ops.l2_normalize2(xs, ys, self.cfg.normalize_eps)
        else:
            for x, y in zip(xs, ys):
                ops.l2_normalize2((x,), (y,), self.cfg.normalize_eps)
        return ys

    def _outputs_backward(self, towers, grads):
        """The mirror of ``_outputs`` in the train step: cfg.normalize_embeddings - the scorer's gradients ``grads`` are w.r.t. the
        unit vectors, and one launch (one per tower where the row counts differ) turns them into the last layers' dz."""
        if not self.cfg.normalize_embeddings:
            return
        xs, dzs = tuple(t.acts[-1] for t in towers), tuple(t.dz[-1] for t in towers)
        if len({t.rows for t in towers}) == 1:
            ops.l2_normalize_bwd2(xs, grads, dzs, self.cfg.normalize_eps)
        else:
            for x, g, dz in zip(xs, grads, dzs):
                ops.l2_normalize_bwd2((x,), (g,), (dz,), self.cfg.normalize_eps)

    # ------------------------------------------------------------------ the hot path
    def _check_ratings(self, ratings):
        if self.rating_on and ratings is None:
            raise ValueError("the model has a rating head (cfg.rating_weight > 0): pass ratings=<f32 [batch], NaN = no label>")
        if not self.rating_on and ratings is not None:
            raise ValueError("ratings were passed but the model has no rating head (cfg.rating_weight == 0)")
        if ratings is not None:
            ops._chk(ratings, torch.float32, "ratings", 1)
            self._check_batch(ratings)

    def _rating_forward(self, q, c, rows: int | None = None, pred=None):
        """The head's forward launch over the first ``rows`` pairs of q / c (default: the batch); fills ``rating_pred`` / the kept h."""
        n = self.cfg.batch_size if rows is None else rows
        ops.rating_head(q[:n], c[:n], self.W1_rating, self.b1_rating, self.w2_rating, self.b2_rating,
                        pred=self.rating_pred[:n] if pred is None else pred, h=self._r_h[:n])

    def _rating_forward_backward(self, q, c, dq, dc, ratings, sample_weight):
        """The head's two launches of the train step, right behind the scorer's: the forward over the vectors the scorer has
        just read, the backward ADDING the head's gradient into the scorer's dq / dc (the first batch_size candidate rows) and
        writing the slabs of the two dense segments and of the squared error."""
        b = self.cfg.batch_size
        self._rating_forward(q, c)
        ops.rating_head_bwd(q[:b], c[:b], self._r_h, self.rating_pred, ratings, self.W1_rating, self.w2_rating,
                            2.0 * self.cfg.rating_weight / b, dq[:b], dc[:b], self._r_kslabs, self._r_bslabs, self._r_se,
                            sample_weight=sample_weight, accumulate=True)

    @property
    def rating_loss(self) -> torch.Tensor:
        """L_r of the last train step: the mean over the batch (the divisor is batch_size, not the number of labels) of
        w (pred - rating)^2 over the pairs with a finite rating; device scalar, unsynchronised, formed from the slabs on demand."""
        if not self.rating_on:
            raise ValueError("rating_loss: the model has no rating head (cfg.rating_weight == 0)")
        return self._r_se.sum() / self.cfg.batch_size

    def forward_backward(self, user_ids: torch.Tensor, item_ids: torch.Tensor, sample_weight=None,
                         candidate_sampling_probability=None, candidate_ids=None, category_ids=None, ratings=None,
                         timestamps=None, *, _sampled: bool = False):
        """Loss and every gradient of one step, for both samplings.  In-batch: the item side is the pairs' items.  Mixed negative
        sampling: the item side is ``cand_ids`` (B + N rows: the sampler launch runs here unless ``step`` has run it,
        ``_sampled``), the scorer works at [B] x [B + N] with the positive of query i at candidate i, and ``cand_ids`` always
        goes to it - a sampled id equal to a row's own positive is a false negative, which the scorer masks.
        ``timestamps`` [batch] int64: the pairs' interaction times (required iff cfg.time_fields; the context is on the user
        side only, so mixed sampling takes it too)."""
        cfg, ut, it = self.cfg, self.user_tower, self.item_tower
        self._check_ratings(ratings)
        if self.time_on or timestamps is not None:
            self._check_timestamps(timestamps, where="forward_backward")
        if self.mixed:
            if candidate_sampling_probability is not None or candidate_ids is not None or category_ids is not None:
                raise ValueError("candidate_sampling='mixed': the trainer draws the candidates itself - candidate_ids, "
                                 "candidate_sampling_probability (set_item_frequencies) and category_ids cannot be passed")
            self._check_batch(user_ids, item_ids, sample_weight)
            if not _sampled:
                self.sample_candidates(item_ids)
            ids = candidate_ids = self.cand_ids
            if self.item_freq is not None or self.freq_on:
                candidate_sampling_probability = self.cand_prob
        else:
            self._check_categories(category_ids)
            if self.freq_on and not (candidate_sampling_probability is self.freq_prob and self._freq_step == self.step_index):
                candidate_sampling_probability = self._update_frequencies(item_ids, candidate_sampling_probability)   # (step() has not)
            ids = item_ids
        lks = self._lookups(user_ids, ids, category_ids)
        if lks is None:                          # (the history launch leaves out the pair's own item)
            self._tower_inputs((user_ids, ut.acts[0]), (ids, it.acts[0]), category_ids=category_ids, exclude=item_ids, keep=True,
                               timestamps=timestamps)
        # the dropout streams count rows per tower: consecutive steps never share a position
        step, rate, seed = self.step_index, cfg.dropout_rate, self.dropout_seed
        towers_forward((ut, it), ((rate, seed, 0, step * ut.rows), (rate, seed, 1, step * it.rows)), lookups=lks)
        q, c = self._outputs((ut, it))
        # normalised: the scorer's gradients are w.r.t. the unit vectors; _outputs_backward turns them into the last layer's dz
        dq, dc = (ut.dunit, it.dunit) if cfg.normalize_embeddings else (ut.dz[-1], it.dz[-1])
        # loss + dq + dc in two fused passes over the logits (probabilities never stored; f32: raw dot products kept in self.ws)
        if self.pairwise_kind is not None:       # (the same outputs; self.lse is not touched)
            ops.retrieval_pairwise_fwd_bwd(q, c, 1.0 / cfg.temperature, self.pairwise_ws, self.per_row, self.loss, dq, dc,
                                           kind=self.pairwise_kind, margin=cfg.pairwise_margin, reduction=cfg.pairwise_reduction,
                                           sample_weight=sample_weight, cand_prob=candidate_sampling_probability,
                                           cand_ids=candidate_ids)
        else:
            ops.retrieval_fwd_bwd(q, c, 1.0 / cfg.temperature, self.ws, self.lse, self.per_row, self.loss, dq, dc,
                                  sample_weight=sample_weight, cand_prob=candidate_sampling_probability, cand_ids=candidate_ids,
                                  precision=cfg.scorer_precision)
        if self.rating_on:                       # the pairs are the first batch_size candidate rows; sampled rows get no head gradient
            self._rating_forward_backward(q, c, dq, dc, ratings, sample_weight)
        self._outputs_backward((ut, it), (dq, dc))
        towers_backward((ut, it), cfg.dropout_rate, lookups=lks, bwd2_ws=self.bwd2_ws)
        self._features_backward()
        if self.time_on:
            self._time_backward()
        self._history_backward()
        self._lr_step = self.step_index
        self.step_index += 1
        return self.loss

    # ------------------------------------------------------------------ learning-rate schedule and gradient clipping
    def learning_rate_at(self, step: int) -> float:
        """The schedule's rate at the 0-based step ``step`` (``TwoTowerConfig.learning_rate_at``)."""
        return self.cfg.learning_rate_at(step)

    @property
    def learning_rate(self) -> float:
        """The rate of the step in progress (after ``forward_backward``: of the step whose gradients wait for
        ``apply_gradients``) - what every optimizer launch takes.  Without a schedule: cfg.learning_rate."""
        return self.cfg.learning_rate_at(self._lr_step)

    def _clip_list(self):
        """Every gradient buffer as it stands between the backward pass and ``apply_gradients``, with the factor of its rows:
        the towers' input gradients count once per id table that consumes them (user; item, category) plus w(n) per bag that is
        pooled into them (title; history by sum / mean / sqrtn - the bags' scaled rows are formed from them later, inside
        ``apply_gradients``), the attention pool's slot rows count where the slot was kept (a skipped slot's row is stale), and
        every dense segment's slabs are summed before they are squared."""
        cfg = self.cfg
        user = dict(weight=1.0)
        if self.history_table is not None and not self._slot_rows:
            user.update(slot_ids=self.history_ids, mode=cfg.history_pooling)
        item = dict(weight=2.0 if self.cat_table is not None else 1.0)
        if self.title_table is not None:
            item.update(slot_ids=self.title_ids, mode=cfg.title_pooling)
        rows = [ops.make_clip_rows(self.user_tower.demb, **user), ops.make_clip_rows(self.item_tower.demb, **item)]
        if self._slot_rows:                      # attention, GRU and self-attention alike: a kept slot's row counts once
            rows.append(ops.make_clip_rows(self.history_slot_grads, 0.0, self.history_ids, "mask"))
        return ops.ClipList(rows, self._segs if self._adam_segs is None else self._adam_segs)

    def clip_gradients(self):
        """cfg.global_clipnorm > 0: scales every gradient of the step IN PLACE by c / max(global norm, c) - two launches, between
        ``forward_backward`` and ``apply_gradients`` (``step`` calls it there).  Leaves ``grad_norm`` and ``clip_scale``.  The l2
        term is added by the optimizer launches: it is neither counted nor scaled.  Off: nothing happens."""
        if not self.cfg.global_clipnorm > 0:
            return None
        if self._clip is None:
            self._clip = self._clip_list()
            self._clip_ws = torch.empty(self._clip.workspace_bytes, dtype=torch.uint8, device=self.dev)
            self._clip_stats = torch.zeros(2, device=self.dev)
        return ops.clip_global_norm_(self._clip, clipnorm=self.cfg.global_clipnorm, workspace=self._clip_ws, stats=self._clip_stats)

    def _clip_stat(self, i: int, what: str) -> torch.Tensor:
        if self._clip_stats is None:
            raise ValueError(f"{what}: no step has been clipped (cfg.global_clipnorm == 0, or clip_gradients has not run)")
        return self._clip_stats[i]

    @property
    def grad_norm(self) -> torch.Tensor:
        """The global gradient norm of the last clipped step BEFORE clipping; device scalar, unsynchronised."""
        return self._clip_stat(0, "grad_norm")

    @property
    def clip_scale(self) -> torch.Tensor:
        """c / max(grad_norm, c) of the last clipped step; device scalar, unsynchronised."""
        return self._clip_stat(1, "clip_scale")

    # ------------------------------------------------------------------ mixed negative sampling
    def sample_candidates(self, item_ids: torch.Tensor) -> torch.Tensor:
        """The sampler launch of the step about to run: ``cand_ids`` = the batch's items followed by draws step_index * N ..
        step_index * N + N - 1 of the stream (seed, TID_SAMPLED_NEGATIVES) - so a resumed run draws what an uninterrupted one
        does - and, once the frequencies are set, ``cand_prob``."""
        cfg = self.cfg
        unigram = cfg.negative_sampler == "unigram"
        if unigram and self.alias is None:
            raise ValueError("negative_sampler='unigram' needs the item frequencies: call set_item_frequencies first")
        counted = not self.freq_on           # the correction from set_item_frequencies' vector (streaming: from the sketch, below)
        ops.sample_candidates(item_ids, cfg.n_items, cfg.n_sampled_negatives, self.cand_ids, self.cand_prob,
                              sampler="alias" if unigram else "uniform", alias=self.alias if unigram else None,
                              item_freq=self.item_freq if counted else None,
                              sampler_prob=self.sampler_prob if unigram and counted else None,
                              seed=self.dropout_seed, tensor_id=TID_SAMPLED_NEGATIVES,
                              start=self.step_index * cfg.n_sampled_negatives, oob_flag=self.oob)
        if self.freq_on:
            # right behind the sampler: the batch's items update the sketch, every candidate - sampled ones included - gets the
            # mixture's probability with the sketch's expected in-batch count in the place of B * item_freq
            self._estimate(self.cand_ids, cfg.batch_size, self.step_index + 1, self.cand_prob, mix=True,
                           sampler_prob=self.sampler_prob if unigram else None)
        return self.cand_ids

    # ------------------------------------------------------------------ streaming frequency estimation
    def _estimate(self, ids, n_update: int, step: int, out, mix: bool = False, sampler_prob=None):
        """One call of the estimator on the trainer's sketch: hash rows TID_FREQ_HASH_BASE + h of the trainer's seed."""
        return ops.frequency_estimate_(self.freq_sketch, ids, n_update, step, self.cfg.freq_alpha, self.cfg.n_items, out,
                                       seed=self.dropout_seed, tensor_id=TID_FREQ_HASH_BASE, sampler_prob=sampler_prob, mix=mix,
                                       oob_flag=self.oob)

    def _refuse_given_probability(self, given, where: str):
        if given is not None:
            raise ValueError(f"{where}: sampling_bias_estimator='streaming' - the trainer estimates every candidate's sampling "
                             "probability itself, candidate_sampling_probability cannot be passed")

    def _update_frequencies(self, item_ids, given=None):
        """The in-batch train step's estimator launch, in front of everything else: the batch's items update the sketch at the
        1-based step step_index + 1 and ``freq_prob`` - the scorer's cand_prob - gets their estimated probabilities."""
        self._refuse_given_probability(given, "step")
        ops._chk(item_ids, torch.int64, "item_ids", 1)
        if item_ids.numel() != self.cfg.batch_size:
            raise ValueError(f"item_ids must hold batch_size = {self.cfg.batch_size} ids, got {item_ids.numel()}")
        self._estimate(item_ids, self.cfg.batch_size, self.step_index + 1, self.freq_prob)
        self._freq_step = self.step_index
        return self.freq_prob

    def _read_frequencies(self, item_ids, given=None):
        """``evaluate``'s estimator launch: the in-batch candidates' probabilities as the sketch stands, nothing is updated."""
        self._refuse_given_probability(given, "evaluate")
        return self._estimate(item_ids, 0, max(self.step_index, 1), self.freq_prob)

    def estimated_item_probability(self, ids: torch.Tensor) -> torch.Tensor:
        """The estimator's present probability 1 / D of ANY number of item ids ([n] f32; 1.0 for an id out of range, which also
        sets the out-of-range flag): an estimate-only call, the sketch is not changed.  The probability of the item being among a
        step's positives - it saturates at 1 for items that occur several times per batch."""
        if not self.freq_on:
            raise ValueError("estimated_item_probability: the trainer has no estimator (cfg.sampling_bias_estimator == 'none')")
        ids = ids.to(device=self.dev, dtype=torch.int64).reshape(-1).contiguous()
        return self._estimate(ids, 0, max(self.step_index, 1), torch.empty(ids.numel(), device=self.dev))

    # ------------------------------------------------------------------ the optimizer and the step
    def apply_gradients(self, step_ids=None):
        """``step_ids`` = [user ids, item ids (, category ids)]: the optimizer launch sorts them itself (no plan launch ran).
        Mixed negative sampling: with ``step_ids`` the sort plans run here (over the user ids and ``cand_ids``).  The step's rate
        and lazy Adam's 1-based global step are read ONCE, for every call of the step; the latter counts on at the end."""
        cfg, lr, t = self.cfg, self.learning_rate, self.adam_step
        if self.mixed and step_ids is not None:
            ops.sparse_plan_batched([self.user_plan, self.item_plan], [step_ids[0], self.cand_ids], [cfg.n_users, cfg.n_items])
        self._apply_table_gradients(step_ids, lr, t)
        if self.title_table is not None:
            self._apply_title_gradients(lr, t)
        if self.history_table is not None:
            self._apply_history_gradients(lr, t)
        if self._adam_segs is not None:          # lazy Adam
            self.adam_step = t + 1

    def _apply_history_gradients(self, lr: float, adam_step: int):
        """The history table's update, the mirror of ``_apply_title_gradients`` on the user side: the sort plan over the step's
        slot items (an excluded slot is -1 there: no gradient), the bags' scaled user-tower input gradient rows, the optimizer.
        Attention pooling: the slots' own gradient rows (``_history_backward`` wrote them) through the plain sort plan."""
        cfg, plan = self.cfg, self.history_plan
        plan.run(self.history_ids, cfg.n_items)
        if self._slot_rows:                      # one gradient row per kept slot, written by the step's backward launch
            gs = self.history_slot_grads
        else:
            gs = plan.backward(self.user_tower.demb, self.history_inv, self.history_gs)
        EmbeddingTable.update(cfg, [self.tables["history"].opt_args(gs)], [], lr, adam_step)

    def _apply_title_gradients(self, lr: float, adam_step: int):
        """The title table's update: sort plan over the step's slot tokens, one launch that scales the item-tower input gradient
        rows by the bags' pooling scales and turns the plan's slot positions into bag indices, then the configured optimizer on
        [batch, dim] gradient rows (a slot's gradient is its bag's row: no per-token rows)."""
        cfg, plan = self.cfg, self.title_plan
        plan.run(self.title_ids, cfg.n_title_buckets)
        gs = plan.backward(self.item_tower.demb, self.title_inv, self.title_gs)
        EmbeddingTable.update(cfg, [self.tables["title"].opt_args(gs)], [], lr, adam_step)

    def _apply_table_gradients(self, step_ids, lr: float, adam_step: int):
        """The update of the pairs' id tables and of the dense parameters.  In-batch SGD / Adagrad keep their fused forms, whose
        grouping was measured: sort + every table + the dense segments in ONE launch straight from the raw ids (``step_ids``),
        the same from the sort plans, or (fuse_optimizer = False) the dense launch and the user + item launch.  Everything else
        - lazy Adam, row-wise Adagrad, mixed sampling, the category table behind the unfused pair - is the plan-fed calls of
        ``_table_calls``, in front of which SGD / Adagrad update the dense segments in a launch of their own."""
        cfg, tabs = self.cfg, self._opt_tables
        fused = self._riding is None and not self.mixed
        if fused and step_ids is not None:
            tables = [(table, accum, grads, ids, plan) for (table, accum, grads, plan), ids in zip(tabs, step_ids)]
            ops.optimizer_step_ids_(cfg.optimizer, tables, self._segs, lr, cfg.adagrad_epsilon)
            return
        if fused and self.fuse_optimizer:
            ops.optimizer_step_(cfg.optimizer, tabs, self._segs, lr, cfg.adagrad_epsilon)
            return
        if self._riding is None:
            ops.dense_update_(self._segs, cfg.optimizer, lr, cfg.adagrad_epsilon)
        if fused:
            ops.sparse_update2_(cfg.optimizer, *tabs[0], *tabs[1], lr, cfg.adagrad_epsilon)
        for tables, segs in self._table_calls:
            EmbeddingTable.update(cfg, tables, segs, lr, adam_step)

    def step(self, user_ids: torch.Tensor, item_ids: torch.Tensor, **loss_kw) -> torch.Tensor:
        """One train step; returns the (device, unsynchronised) retrieval loss (SUM over the batch).
        With cfg.normalize_embeddings the step never takes the composite C call (``tt_train_step_f32`` cannot describe the two
        normalisation launches): it runs the Python sequence ``forward_backward`` + ``apply_gradients(step_ids=...)`` - the path
        asymmetric towers take - with one launch after the towers' forward and one in front of their backward.
        Mixed negative sampling: the sampler launch comes in front of everything else (the plans and both lookups read
        ``cand_ids``), the sort plans always run, on the main stream, and the step is the Python sequence."""
        cfg = self.cfg
        self._check_ratings(loss_kw.get("ratings"))
        if not self.rating_on:
            loss_kw.pop("ratings", None)
        if self.time_on:
            self._check_timestamps(loss_kw.get("timestamps"))
        elif "timestamps" in loss_kw:            # (None is dropped: the composite call does not know the argument)
            self._check_timestamps(loss_kw.pop("timestamps"))
        if self.mixed:
            bad = [k for k, v in loss_kw.items() if v is not None and k not in ("sample_weight", "ratings", "timestamps")]
            if bad:
                raise ValueError(f"candidate_sampling='mixed': the trainer draws the candidates itself - {', '.join(sorted(bad))} cannot "
                                 "be passed to step() (the correction comes from set_item_frequencies)")
        self._check_batch(user_ids, item_ids, loss_kw.get("category_ids"), loss_kw.get("sample_weight"),
                          loss_kw.get("candidate_sampling_probability"), loss_kw.get("candidate_ids"))
        if self.freq_on and not self.mixed:      # in front of everything else; its output is the step's cand_prob (the composite call's too)
            loss_kw["candidate_sampling_probability"] = self._update_frequencies(item_ids, loss_kw.get("candidate_sampling_probability"))
        # (never inside a graph capture: the poll queries an event recorded outside it and would bake a D2H copy into every replay)
        if self.flag_poll_every and self.step_index % self.flag_poll_every == 0 and not torch.cuda.is_current_stream_capturing():
            self.poll_ids()
        item_side = item_ids
        if self.mixed:                           # (with the streaming estimator the sampler call updates the sketch)
            item_side = self.sample_candidates(item_ids)
            loss_kw["_sampled"] = True
        # the sort plans depend on the ids only: one launch for all tables, in front of the forward pass (or beside it)
        plans, ids, rows = [self.user_plan, self.item_plan], [user_ids, item_side], [cfg.n_users, cfg.n_items]
        if loss_kw.get("category_ids") is not None and self.cat_plan is not None:
            plans.append(self.cat_plan); ids.append(loss_kw["category_ids"]); rows.append(cfg.n_category_buckets)
        # fuse_sort: no plan launch at all - the optimizer launch's workgroups sort the ids of their own row range in LDS
        # and update exactly those rows (tt_optimizer_step_ids_f32; lists up to 65536 ids) - unless the batches are skewed
        # (lazy Adam, row-wise Adagrad and mixed sampling always take the sort plan: no composite call, no one-launch form and so
        # no skew probe)
        shape_ok = (self._riding is None and not self.mixed and self.fuse_sort and self.fuse_optimizer
                    and user_ids.numel() <= ops.optimizer_ids_max_ids() and (self.cat_table is None) == (len(ids) == 2))
        if shape_ok:
            self._poll_skew(ids, rows)
        fused_sort = shape_ok and not self._skewed()
        # (the clip launches sit between the backward pass and the optimizer: never composite)
        if (fused_sort and not cfg.global_clipnorm > 0 and self.use_composite and self.fuse_lookup and cfg.symmetric
                and not cfg.normalize_embeddings and not cfg.layer_norm and not self.rating_on and self.pairwise_kind is None
                and cfg.batch_size <= ops.MAX_FUSED_LOOKUP_ROWS):
            return self._step_composite(ids, **loss_kw)
        side = self._side if (self.plan_on_side_stream and not fused_sort and not self.mixed) else None
        if side is not None:
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):        # one launch for all tables (csrc/sort.hip)
                ops.sparse_plan_batched(plans, ids, rows)
        elif not fused_sort:
            ops.sparse_plan_batched(plans, ids, rows)
        loss = self.forward_backward(user_ids, item_ids, **loss_kw)
        if side is not None:
            main.wait_stream(side)
        self.clip_gradients()
        self.apply_gradients(step_ids=ids if fused_sort else None)
        return loss

    def _build_composite(self):
        """The step's description for tt_train_step_f32 (include/twotower_hip.h): every buffer of the step is allocated once,
        so the struct is filled once; step() rewrites the id pointers, the dropout row counter and the optional inputs."""
        cfg, ut, it = self.cfg, self.user_tower, self.item_tower
        st = _lib.TrainStep()
        st.batch, st.n_layers = cfg.batch_size, ut.n_layers
        if ut.n_layers > _lib.TT_MAX_TOWER_LAYERS or len(self._segs) > _lib.TT_MAX_DENSE_SEGS:
            return None
        for l, d in enumerate(ut.dims):
            st.dims[l] = d
        p = ops._p
        for l in range(ut.n_layers):
            for i, tw in enumerate((ut, it)):
                f, b = st.fwd[l][i], st.bwd[l][i]
                f.x = None if l == 0 else p(tw.acts[l])
                f.w, f.b, f.y = p(tw.w[l]), p(tw.b[l]), p(tw.acts[l + 1])
                f.dropout_tensor_id = TID_DROPOUT_BASE + 2 * l + i
                f.relu_bits = p(tw.bits[l + 1])
                b.x = None if l == 0 else p(tw.acts[l])
                b.w, b.dz = p(tw.w[l]), p(tw.dz[l])
                b.dx = p(tw.dz[l - 1] if l > 0 else tw.demb)
                b.dx_relu_bits = p(tw.bits[l]) if l > 0 else None
                b.dx_relu_src = p(tw.acts[l]) if (l > 0 and tw.bits[l] is None) else None
                b.dw_slabs, b.db_slabs = p(tw.dw_slabs[l]), p(tw.db_slabs[l])
        for i, (table, rows2) in enumerate(((self.user_table, None), (self.item_table, self.cat_table))):
            for lk in (st.fwd[0][i].lookup, st.bwd[0][i].lookup):
                lk.table, lk.table_rows, lk.oob_flag = p(table), table.shape[0], p(self.oob)
                if rows2 is not None:
                    lk.table2, lk.table2_rows = p(rows2), rows2.shape[0]
        st.dropout_rate, st.dropout_seed = cfg.dropout_rate, self.dropout_seed
        st.scorer_precision = ops.SCORER_PRECISIONS.index(cfg.scorer_precision)
        st.inv_temperature = 1.0 / cfg.temperature
        st.retrieval_ws, st.retrieval_ws_bytes = p(self.ws), self.ws.numel()
        st.lse, st.per_row, st.loss = p(self.lse), p(self.per_row), p(self.loss)
        st.opt = ops._OPT[cfg.optimizer]
        tabs = self._opt_tables
        st.n_tables = len(tabs)
        for i, (table, accum, grads, plan) in enumerate(tabs):
            t = st.tables[i]
            t.table, t.accum, t.rows, t.grads = p(table), p(accum), table.shape[0], p(grads)
            t.apply_ws = p(plan.apply_ws(cfg.embedding_dim))
        st.n_segs = len(self._segs)
        for i, seg in enumerate(self._segs):
            st.segs[i] = seg
        st.lr, st.eps = cfg.learning_rate, cfg.adagrad_epsilon
        # r04: the forward lookup hands the optimizer launch its row-range id lists (tt_id_buckets, ABI v9): a zeroed workspace
        # is all the caller supplies, tt_train_step_f32 cuts the ranges and stamps a generation per step
        if self._id_bucket_ws is None:
            per = int(_lib.load().tt_id_buckets_workspace_bytes())
            self._id_bucket_ws = torch.zeros(2 * per, dtype=torch.uint8, device=self.dev)
        st.id_bucket_ws, st.id_bucket_ws_bytes = p(self._id_bucket_ws), self._id_bucket_ws.numel()
        return st

    def _step_composite(self, ids, sample_weight=None, candidate_sampling_probability=None, candidate_ids=None,
                        category_ids=None) -> torch.Tensor:
        """forward_backward + apply_gradients as ONE call into the library (same launches, same order, same results)."""
        self._check_categories(category_ids)
        if self._cstep is None:
            self._cstep = self._build_composite()
            if self._cstep is None:                  # more layers / segments than the struct holds: the Python sequence
                self.use_composite = False
                loss = self.forward_backward(ids[0], ids[1], sample_weight=sample_weight, category_ids=category_ids,
                                             candidate_sampling_probability=candidate_sampling_probability, candidate_ids=candidate_ids)
                self.apply_gradients(step_ids=ids)
                return loss
        st = self._cstep
        for t in ids:
            ops._chk(t, torch.int64, "ids", 1)
        for t, name in ((sample_weight, "sample_weight"), (candidate_sampling_probability, "candidate_sampling_probability")):
            if t is not None:
                ops._chk(t, torch.float32, name, 1)
        if candidate_ids is not None:
            ops._chk(candidate_ids, torch.int64, "candidate_ids", 1)
        p = ops._p
        for i in range(2):
            for lk in (st.fwd[0][i].lookup, st.bwd[0][i].lookup):
                lk.ids = p(ids[i])
                if i == 1:
                    lk.ids2 = p(category_ids)
            st.tables[i].ids = p(ids[i])
        if st.n_tables == 3:
            st.tables[2].ids = p(ids[2])
        st.dropout_seed = self.dropout_seed
        st.dropout_row0 = self.step_index * self.cfg.batch_size
        st.scorer_precision = ops.SCORER_PRECISIONS.index(self.cfg.scorer_precision)   # (may be switched between steps: bench's second line)
        self._lr_step = self.step_index
        st.lr, st.eps = self.learning_rate, self.cfg.adagrad_epsilon                     # (re-read every step, like the Python sequence)
        st.inv_temperature, st.dropout_rate = 1.0 / self.cfg.temperature, self.cfg.dropout_rate
        st.sample_weight, st.cand_prob, st.cand_ids = p(sample_weight), p(candidate_sampling_probability), p(candidate_ids)
        _lib.check(_lib.load().tt_train_step_f32(st, ops._stream()), "tt_train_step_f32")
        self.step_index += 1
        return self.loss

    def evaluate(self, user_ids: torch.Tensor, item_ids: torch.Tensor, **loss_kw) -> torch.Tensor:
        """Forward only (validation loss, SUM over the batch); device tensor, unsynchronised."""
        cfg, ut, it = self.cfg, self.user_tower, self.item_tower
        ratings = loss_kw.get("ratings")
        self._check_ratings(ratings)
        self._check_timestamps(loss_kw.get("timestamps"), where="evaluate")
        self._check_categories(loss_kw.get("category_ids"))
        self._check_batch(loss_kw.get("sample_weight"), loss_kw.get("candidate_sampling_probability"),
                          loss_kw.get("candidate_ids"))
        if self.freq_on:             # estimated, not updated: a validation batch is no part of the training stream
            self._check_batch(item_ids)
            loss_kw["candidate_sampling_probability"] = self._read_frequencies(item_ids, loss_kw.get("candidate_sampling_probability"))
        # mixed sampling: the in-batch loss, as without sampling - a partial pass over the first batch_size rows of the item
        # tower's buffers, never through a fused lookup
        b = cfg.batch_size
        rows = (b, b) if self.mixed else None
        self._check_batch(user_ids, item_ids)
        lks = None if self.mixed else self._lookups(user_ids, item_ids, loss_kw.get("category_ids"))
        if lks is None:
            self._tower_inputs((user_ids, ut.acts[0]), (item_ids, it.acts[0][:b]), category_ids=loss_kw.get("category_ids"),
                               timestamps=loss_kw.get("timestamps"))
        towers_forward((ut, it), lookups=lks, rows=rows)
        q, c = self._outputs((ut, it), rows)
        if self.rating_on:
            self._rating_evaluate(q, c, ratings, loss_kw.get("sample_weight"))
        if self.pairwise_kind is not None:
            return ops.retrieval_pairwise_fwd(q, c, 1.0 / cfg.temperature, self.pairwise_ws, self.per_row, self.loss,
                                              kind=self.pairwise_kind, margin=cfg.pairwise_margin, reduction=cfg.pairwise_reduction,
                                              sample_weight=loss_kw.get("sample_weight"),
                                              cand_prob=loss_kw.get("candidate_sampling_probability"),
                                              cand_ids=loss_kw.get("candidate_ids"))
        return ops.retrieval_fwd(q, c, 1.0 / cfg.temperature, self.ws, self.lse, self.per_row, self.loss,
                                 sample_weight=loss_kw.get("sample_weight"), cand_prob=loss_kw.get("candidate_sampling_probability"),
                                 cand_ids=loss_kw.get("candidate_ids"), precision=cfg.scorer_precision)

    def _rating_evaluate(self, q, c, ratings, sample_weight=None):
        """The head's forward launch on a validation batch; leaves ``rating_pred`` and two device scalars for the caller's
        metric - ``eval_rating_se`` (sum of w (pred - rating)^2 over the finite ratings) and ``eval_rating_count`` (their
        number) - formed with torch ops (reporting, not the train step)."""
        self._rating_forward(q, c)
        ok = torch.isfinite(ratings)
        e2 = torch.where(ok, (self.rating_pred - torch.nan_to_num(ratings)) ** 2, torch.zeros_like(ratings))
        self.eval_rating_se = (e2 if sample_weight is None else e2 * sample_weight).sum()
        self.eval_rating_count = ok.sum()

    @torch.no_grad()
    def predict_ratings(self, user_ids: torch.Tensor, item_ids: torch.Tensor, category_ids: torch.Tensor | None = None,
                        timestamps: torch.Tensor | None = None) -> torch.Tensor:
        """The head's prediction for ANY number of (user, item) pairs ([n] f32), computed cfg.batch_size pairs at a time on the
        towers' buffers (inference: no dropout, the stored histories in full).  ``category_ids`` [n]: the pairs' category
        buckets (required iff the model has the feature); ``timestamps`` [n] int64: the pairs' times (required iff the model
        has the time features)."""
        if not self.rating_on:
            raise ValueError("predict_ratings: the model has no rating head (cfg.rating_weight == 0)")
        if (category_ids is None) != (self.cat_table is None):
            raise ValueError("category_ids must be given exactly when cfg.n_category_buckets > 0")
        ut, it, b = self.user_tower, self.item_tower, self.cfg.batch_size
        uid = user_ids.to(device=self.dev, dtype=torch.int64).reshape(-1).contiguous()
        iid = item_ids.to(device=self.dev, dtype=torch.int64).reshape(-1).contiguous()
        n = uid.numel()
        if iid.numel() != n or (category_ids is not None and category_ids.numel() != n):
            raise ValueError(f"predict_ratings: user_ids, item_ids (and category_ids) must have one length, got {n} and {iid.numel()}")
        ts = self._inference_timestamps(timestamps, n, "predict_ratings")
        out = torch.empty(n, device=self.dev)
        for s in range(0, n, b):
            e = min(s + b, n)
            m = e - s
            self._tower_inputs((uid[s:e], ut.acts[0][:m]), (iid[s:e], it.acts[0][:m]),
                               category_ids=None if category_ids is None else category_ids[s:e].to(self.dev).contiguous(),
                               timestamps=None if ts is None else ts[s:e])
            ut.forward()
            it.forward()
            q, c = self._outputs((ut, it))
            self._rating_forward(q, c, rows=m, pred=out[s:e])
        return out

    # ------------------------------------------------------------------ retrieval metrics
    @torch.no_grad()
    def item_corpus_embeddings(self, item_category_ids: torch.Tensor | None = None) -> torch.Tensor:
        """Item-tower output for EVERY item row ([n_items, scorer_dim]; unit-norm rows with cfg.normalize_embeddings), computed
        batch by batch on the tower's buffers.
        item_category_ids [n_items]: the category bucket of every item (required iff the model has the feature)."""
        it, b = self.item_tower, self.item_tower.rows
        n = self.cfg.n_items
        if (item_category_ids is None) != (self.cat_table is None):
            raise ValueError("item_category_ids must be given exactly when cfg.n_category_buckets > 0")
        out = torch.empty(n, it.dims[-1], device=self.dev)
        for s in range(0, n, b):
            e = min(s + b, n)
            # the one pass that does not build its rows through _tower_inputs: a chunk is a CONTIGUOUS row range, so the table
            # rows are a copy and the bags pool a slice of the token matrix - no id tensor, no gather; what is summed is restated
            # here (table row + category row + pooled titles), the numeric features come from the builder
            it.acts[0][:e - s].copy_(self.item_table[s:e])
            if item_category_ids is not None:
                ops.embedding_gather_add_(it.acts[0][:e - s], self.cat_table, item_category_ids[s:e], self.oob)
            if self.title_table is not None:       # bag r of the chunk pools token row s + r
                ops.embedding_bag(self.title_table, self.item_titles[s:e], pooling=self.cfg.title_pooling, out=it.acts[0][:e - s],
                                  accumulate=True, oob_flag=self.oob)
            if self.item_features is not None:
                self._tower_inputs(item=(torch.arange(s, e, dtype=torch.int64, device=self.dev), it.acts[0][:e - s]), features_only=True)
            it.forward()
            out[s:e].copy_(self._outputs((it,))[0][:e - s])
        return out

    def _inference_timestamps(self, timestamps, n: int, where: str):
        """``timestamps`` of an inference pass over ``n`` queries, on the device (None: the model has no time features)."""
        if timestamps is not None and torch.is_tensor(timestamps) and timestamps.dtype == torch.int64:
            timestamps = timestamps.to(self.dev).reshape(-1).contiguous()
        self._check_timestamps(timestamps, n, where)
        return timestamps

    @torch.no_grad()
    def user_embeddings(self, user_ids: torch.Tensor, timestamps: torch.Tensor | None = None) -> torch.Tensor:
        """User-tower output (inference: no dropout; unit-norm rows with cfg.normalize_embeddings) for ANY number of user ids
        ([n, scorer_dim]), computed cfg.batch_size
        ids at a time on the tower's buffers.  Out-of-range ids give the tower output of a zero row and set the trainer's
        out-of-range flag (``check_ids``).  ``timestamps`` [n] int64: the time every query is asked at (required iff the model
        has the time features)."""
        ut, b = self.user_tower, self.cfg.batch_size
        ids = user_ids.to(device=self.dev, dtype=torch.int64).reshape(-1).contiguous()
        n = ids.numel()
        ts = self._inference_timestamps(timestamps, n, "user_embeddings")
        out = torch.empty(n, ut.dims[-1], device=self.dev)
        for s in range(0, n, b):
            e = min(s + b, n)
            # (the full stored history: nothing is left out at inference)
            self._tower_inputs(user=(ids[s:e], ut.acts[0][:e - s]), timestamps=None if ts is None else ts[s:e])
            ut.forward()
            out[s:e].copy_(self._outputs((ut,))[0][:e - s])
        return out

    @torch.no_grad()
    def evaluate_topk(self, user_ids: torch.Tensor, item_ids: torch.Tensor, metric, corpus: torch.Tensor | None = None,
                      timestamps: torch.Tensor | None = None):
        """Updates ``metric`` (metrics.FactorizedTopK) with one batch of (user, true item) pairs scored against the
        whole item corpus; returns the ranks.  ``timestamps`` [batch] int64: required iff the model has the time features."""
        self._check_batch(user_ids, item_ids)
        self._check_timestamps(timestamps, where="evaluate_topk")
        if corpus is None:
            corpus = self.item_corpus_embeddings()
        if self.history_table is not None or self.user_features is not None or self.cfg.cross_layers or self.time_on:
            self._tower_inputs(user=(user_ids, self.user_tower.acts[0]), timestamps=timestamps)
            self.user_tower.forward()
        else:
            self.user_tower.forward(lookup=ops.make_lookup(self.user_table, user_ids, oob_flag=self.oob))
        (q,) = self._outputs((self.user_tower,))
        return metric.update_state(q, corpus, item_ids)

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self) -> dict:
        sd = {"config": dict(self.cfg.__dict__), "dense": self.dense_flat, "step_index": self.step_index, "dropout_seed": self.dropout_seed}
        for rec in (*self.tables.values(), *getattr(self, "sides", {}).values()):    # (the projection kernels are part of "dense")
            sd.update(rec.state())
        if getattr(self, "item_freq", None) is not None:     # mixed negative sampling: the correction (and the unigram sampler) is rebuilt from it
            sd["item_freq"] = self.item_freq
        if getattr(self, "freq_on", False):                  # the streaming frequency estimator's state
            sd["freq_sketch"] = self.freq_sketch
        if self.cfg.optimizer in ("adagrad", "rowwise_adagrad"):
            sd["dense_accum"] = self.dense_accum
        if self.cfg.optimizer == "adam":
            sd.update(dense_m=self.dense_m, dense_v=self.dense_v, adam_step=self.adam_step)
        return sd

    def load_state_dict(self, sd: dict):
        for k, default, note, needs in _CHECKPOINT_CHECKS:
            ck, mine = sd["config"].get(k, default), getattr(self.cfg, k)
            same = (ck > 0) == (mine > 0) if k == "rating_weight" else ck == mine
            if not same and (needs is None or getattr(self.cfg, needs)):
                raise ValueError(f"checkpoint {k}={ck!r} does not match the trainer's {mine!r}{note}")
        for rec in (*self.tables.values(), *self.sides.values()):
            for k, dst in rec.state().items():
                dst.copy_(sd[k])
        self.dense_flat.copy_(sd["dense"])
        if self.sides:                  # the clip belongs to the trained model, like the normalisation switch below
            self.cfg.feature_clip = float(sd["config"].get("feature_clip", 0.0))
        # whether the embeddings are normalised belongs to the trained model, not to the run that loads it: the checkpoint's
        # value replaces the trainer's (a checkpoint from before the switch existed: off)
        self.cfg.normalize_embeddings = bool(sd["config"].get("normalize_embeddings", False))
        self.cfg.normalize_eps = float(sd["config"].get("normalize_eps", TwoTowerConfig.normalize_eps))
        if self.cfg.normalize_embeddings:
            self.user_tower.alloc_unit(); self.item_tower.alloc_unit()
        # the counter-based dropout stream continues where the checkpoint stopped (no replayed masks)
        self.step_index = self._lr_step = int(sd.get("step_index", 0))      # (the learning-rate schedule continues there too)
        self.dropout_seed = int(sd.get("dropout_seed", self.dropout_seed))
        # how the candidates are drawn belongs to the run, not to the model: the trainer keeps its own sampling settings (a
        # checkpoint from before they existed, or from an in-batch run, loads as before); a mixed trainer takes the frequencies
        if self.mixed and sd.get("item_freq") is not None:
            self.set_item_frequencies(sd["item_freq"])
        # the estimator, like the sampling settings, belongs to the run: a trainer without one ignores a checkpoint's sketch; a
        # trainer with one continues on it - a sketch of another shape, or none while the step count is carried on (every slot
        # would look unseen for step_index steps), is refused
        if self.freq_on:
            sk = sd.get("freq_sketch")
            if sk is None and self.step_index > 0:
                raise ValueError(f"the checkpoint carries no freq_sketch but continues at step {self.step_index}: the streaming "
                                 "frequency estimator cannot start there (every item would look unseen for that many steps)")
            if sk is not None:
                if tuple(sk.shape) != tuple(self.freq_sketch.shape) or sk.dtype != torch.int64:
                    raise ValueError(f"checkpoint freq_sketch {sk.dtype} {list(sk.shape)} does not match the trainer's int64 "
                                     f"{list(self.freq_sketch.shape)} (freq_hashes / freq_slots)")
                self.freq_sketch.copy_(sk)
        if self.cfg.optimizer in ("adagrad", "rowwise_adagrad"):
            self.dense_accum.copy_(sd["dense_accum"])
        if self.cfg.optimizer == "adam":
            self.dense_m.copy_(sd["dense_m"]); self.dense_v.copy_(sd["dense_v"])
            self.adam_step = int(sd["adam_step"])

    # ------------------------------------------------------------------ HIP graph replay of the whole step
    def capture_graph(self):
        """Capture one train step (its 8-9 launches, one stream) into a HIP graph.  ``step_graph(u, i)`` then
        copies the ids into the captured buffers and replays: one host call per step, no launch gaps."""
        for refused, what in _GRAPH_REFUSALS:
            if refused(self.cfg):
                raise NotImplementedError(f"graph replay with {what}")
        b = self.cfg.batch_size
        self._g_uid = torch.zeros(b, dtype=torch.int64, device=self.dev)
        self._g_iid = torch.zeros(b, dtype=torch.int64, device=self.dev)
        self._g_kw = {}
        if self.cat_table is not None:
            self._g_kw["category_ids"] = torch.zeros(b, dtype=torch.int64, device=self.dev)
        # what the warm-up steps touch and the undo below restores: row 0 of every table (ids 0), the dense parameters, and
        # their Adagrad accumulators
        touched = [x[:1] for t in self.tables.values() for x in (t.table, t.accum) if x is not None] + \
                  [x for x in (self.dense_flat, self.dense_accum) if x is not None]
        state = [x.clone() for x in touched]
        # one graph per optimizer path (r04): the skew probe runs OUTSIDE the graphs (step_graph) and picks which one to replay
        poll, load, state_was = self.flag_poll_every, self.range_load, self._skew_state
        self.flag_poll_every = 0                       # (no probe / flag poll inside the warm-up or the capture)
        self._graphs = {}
        try:
            for skewed in ((False, True) if self.skew_limit else (False,)):
                self.range_load = self.skew_limit + 1 if skewed else 0
                self._skew_state = skewed
                s = torch.cuda.Stream(device=self.dev)
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    self.step(self._g_uid, self._g_iid, **self._g_kw)   # warm-up on the capture stream (ids 0: touches row 0 only)
                torch.cuda.current_stream().wait_stream(s)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self.step(self._g_uid, self._g_iid, **self._g_kw)
                torch.cuda.synchronize()
                self._graphs[skewed] = g
                for x, saved in zip(touched, state):      # undo the warm-up step's update
                    x.copy_(saved)
        finally:
            self.flag_poll_every, self.range_load, self._skew_state = poll, load, state_was
        self._graph = self._graphs[False]
        return self

    def step_graph(self, user_ids: torch.Tensor, item_ids: torch.Tensor, category_ids: torch.Tensor | None = None) -> torch.Tensor:
        self._check_categories(category_ids)
        self._g_uid.copy_(user_ids, non_blocking=True)
        self._g_iid.copy_(item_ids, non_blocking=True)
        ids, rows = [self._g_uid, self._g_iid], [self.cfg.n_users, self.cfg.n_items]
        if category_ids is not None:
            self._g_kw["category_ids"].copy_(category_ids, non_blocking=True)
            ids.append(self._g_kw["category_ids"]); rows.append(self.cfg.n_category_buckets)
        self._replays = getattr(self, "_replays", 0)
        if len(self._graphs) > 1:                      # the skew probe, outside the graphs: which optimizer path this batch replays
            step_was, self.step_index = self.step_index, self._replays
            self._poll_skew(ids, rows)
            self.step_index = step_was
        self._graphs[self._skewed() if len(self._graphs) > 1 else False].replay()
        self._replays += 1
        if self.flag_poll_every and self._replays % self.flag_poll_every == 0:     # host side, outside the graph
            self.poll_ids()
        return self.loss

    def one_launch_optimizer(self, n_ids: int) -> bool:
        """Whether a step of ``n_ids`` pairs would take tt_optimizer_step_ids_f32 (sort + duplicate sums + update in the optimizer
        launch) right now: the shape allows it and the last skew probe saw no overloaded row range."""
        return bool(self.fuse_sort and self.fuse_optimizer and n_ids <= ops.optimizer_ids_max_ids() and not self._skewed())

    def _skewed(self) -> bool:
        if not self.skew_limit:
            return False
        if self.range_load > self.skew_limit:
            self._skew_state = True
        elif 4 * self.range_load < 3 * self.skew_limit:
            self._skew_state = False
        return self._skew_state

    def _poll_skew(self, ids, rows):
        """The skew probe, never waiting for the GPU: takes the result of the probe in flight if it has landed (checked every
        step while one is in flight - a query of an event), and every ``flag_poll_every`` steps starts a new one on this batch's
        ids: one small launch + a 12-byte copy to pinned memory."""
        if not self.skew_limit or not self.fuse_sort or not self.fuse_optimizer or torch.cuda.is_current_stream_capturing():
            return
        if self._skew_event is not None and self._skew_event.query():
            self.range_load, self._skew_event = int(self._skew_host.max().item()), None
        if self._skew_event is None and self.flag_poll_every and self.step_index % self.flag_poll_every == 0:
            if self._skew_dev is None:
                self._skew_dev = torch.zeros(4, dtype=torch.int32, device=self.dev)
                self._skew_host = torch.zeros(4, dtype=torch.int32).pin_memory()
            ops.id_range_load_(self._skew_dev, ids, rows, self.cfg.embedding_dim, self._segs)
            self._skew_host.copy_(self._skew_dev, non_blocking=True)
            self._skew_event = torch.cuda.Event()
            self._skew_event.record()

    def poll_ids(self):
        """Asynchronous check of the out-of-range flag: looks at the copy the PREVIOUS poll started (if it has landed —
        never waits for the GPU) and starts a new 4-byte device-to-pinned-host copy.  step() calls it every
        ``flag_poll_every`` steps; the copy a poll starts is looked at by the NEXT poll, so a bad id is reported within two
        intervals, with the step range it was seen in.  A bad id in the last interval of a run is only seen by check_ids()
        (train.py calls it at the end of every epoch)."""
        if self._oob_event is not None and self._oob_event.query():
            bad, self._oob_event = int(self._oob_host.item()), None
            if bad:
                self.oob.zero_()
                raise IndexError(f"embedding id out of range at or before step {self._oob_step}")
        if self._oob_event is None:
            if self._oob_host is None:
                self._oob_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._oob_host.copy_(self.oob, non_blocking=True)
            self._oob_event = torch.cuda.Event()
            self._oob_event.record()
            self._oob_step = self.step_index

    def check_ids(self):
        """Host check of the out-of-range flag (TF's CPU gather raises InvalidArgumentError); synchronises."""
        self._oob_event = None
        if int(self.oob.item()) != 0:
            self.oob.zero_()
            raise IndexError("embedding id out of range in a previous step")

    def l2_penalty(self) -> torch.Tensor:
        """l2 * sum(W^2) over the Dense kernels — reporting only (the gradient term is fused in the update)."""
        tot = torch.zeros((), device=self.dev, dtype=torch.float64)
        for seg in self.layout.segments:
            if seg.l2:                           # (kernel by kernel: one f64 sum per parameter, as it was always reported)
                for blk in self.layout.blocks.values():
                    if seg.lo <= blk.offset < seg.hi:
                        tot += (blk.view(self.dense_flat).double() ** 2).sum()
        return self.cfg.l2_regularization * tot
