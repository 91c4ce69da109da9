"""Reads the reference's hyper-parameter schema: the ``model:`` block of
``/root/reference/configs/data_config.yaml:54-71`` (no code in the reference reads it)."""
from __future__ import annotations

import math

import yaml

from .trainer import LR_DECAYS, RETRIEVAL_LOSSES, SAMPLING_BIAS_ESTIMATORS, TwoTowerConfig


def load_yaml(path) -> dict:
    with open(path, "r") as f:           # yaml.safe_load, as download_data.py:32-39 does
        return yaml.safe_load(f)


NUMERIC_FEATURE_SOURCES = ("none", "rating_stats")


def numeric_features_from_dict(doc: dict) -> dict:
    """{source, clip} of the optional ``model.features.numeric`` block (not in the reference's schema): ``source`` rating_stats -
    the per-user / per-item rating count, mean, std, min, max of ``data.rating_features`` - or none; ``clip`` >= 0 clamps the
    normalised values (0: no clipping)."""
    block = (((doc.get("model") or {}).get("features") or {}).get("numeric")) or {}
    source = str(block.get("source", "none") or "none").lower()
    if source not in NUMERIC_FEATURE_SOURCES:
        raise ValueError(f"model.features.numeric.source must be one of {NUMERIC_FEATURE_SOURCES}, got {source!r}")
    clip = float(block.get("clip", 0.0))
    if not clip >= 0.0:
        raise ValueError("model.features.numeric.clip must be >= 0")
    return {"source": source, "clip": clip}


def ranking_from_dict(doc: dict) -> dict:
    """{weight, hidden_dim} of the optional ``model.ranking`` block (not in the reference's schema): the rating-prediction head -
    ``weight`` > 0 trains it beside the retrieval task (total = retrieval + weight * MSE on the rating), ``hidden_dim`` is its
    hidden width (a multiple of 32 in 32..256).  Without the block: no head."""
    import math
    block = (doc.get("model") or {}).get("ranking") or {}
    if not isinstance(block, dict):
        raise ValueError("model.ranking must be a mapping {weight, hidden_dim}")
    weight, hidden = block.get("weight", 0.0), block.get("hidden_dim", 128)
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not (weight >= 0.0 and math.isfinite(weight)):
        raise ValueError(f"model.ranking.weight must be a finite number >= 0, got {weight!r}")
    if isinstance(hidden, bool) or not isinstance(hidden, int) or not (32 <= hidden <= 256 and hidden % 32 == 0):
        raise ValueError(f"model.ranking.hidden_dim must be a multiple of 32 in 32..256, got {hidden!r}")
    return {"weight": float(weight), "hidden_dim": hidden}


def cross_from_dict(doc: dict) -> dict:
    """{layers} of the optional ``model.cross`` block (not in the reference's schema): ``layers`` DCN-v2 cross layers (0..3) in
    both towers, between the summed input features and the Dense stack.  Without the block: none."""
    block = (doc.get("model") or {}).get("cross")
    if block is None:
        return {"layers": 0}
    if not isinstance(block, dict):
        raise ValueError("model.cross must be a mapping {layers}")
    unknown = sorted(set(block) - {"layers"})
    if unknown:
        raise ValueError(f"model.cross: unknown keys {unknown} (low-rank, diag_scale and preactivation forms are not implemented)")
    layers = block.get("layers", 0)
    if isinstance(layers, bool) or not isinstance(layers, int) or not 0 <= layers <= 3:
        raise ValueError(f"model.cross.layers must be an int in 0..3, got {layers!r}")
    return {"layers": layers}


def layer_norm_from_dict(doc: dict) -> dict:
    """{enabled, epsilon} of the optional ``model.layer_norm`` block (not in the reference's schema): Keras LayerNormalization
    between every hidden Dense layer of both towers and its ReLU.  Without the block: off, epsilon 1e-3 (Keras's default)."""
    block = (doc.get("model") or {}).get("layer_norm")
    default = TwoTowerConfig.layer_norm_epsilon
    if block is None:
        return {"enabled": False, "epsilon": default}
    if not isinstance(block, dict):
        raise ValueError("model.layer_norm must be a mapping {enabled, epsilon}")
    unknown = sorted(set(block) - {"enabled", "epsilon"})
    if unknown:
        raise ValueError(f"model.layer_norm: unknown keys {unknown} (center / scale switches, other axes and RMS scaling are not implemented)")
    enabled, eps = block.get("enabled", False), block.get("epsilon", default)
    if not isinstance(enabled, bool):
        raise ValueError(f"model.layer_norm.enabled must be a bool, got {enabled!r}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"model.layer_norm.epsilon must be a finite number > 0, got {eps!r}")
    return {"enabled": enabled, "epsilon": float(eps)}


def time_features_from_dict(doc: dict) -> dict:
    """{fields, buckets} of the optional ``model.features.time`` block (not in the reference's schema; its
    ``create_temporal_features`` is the model's input here): ``fields`` a list out of hour, day_of_week, month, period - kept in
    that order - and ``buckets``, the rows of the period field (1..4096, given exactly when ``period`` is on).  Without the
    block: no fields.  The range the periods cut (time_min, time_max) comes from the training data: train.py sets it."""
    block = ((doc.get("model") or {}).get("features") or {}).get("time")
    if block is None:
        return {"fields": (), "buckets": 0}
    if not isinstance(block, dict):
        raise ValueError("model.features.time must be a mapping {fields, buckets}")
    unknown = sorted(set(block) - {"fields", "buckets"})
    if unknown:
        raise ValueError(f"model.features.time: unknown keys {unknown} (known: ['fields', 'buckets'])")
    return check_time_features(block.get("fields") or (), block.get("buckets", 0), "model.features.time")


def check_time_features(fields, buckets, where: str) -> dict:
    """The validated {fields (in the fixed order), buckets} of a time-feature selection (the YAML block's or the CLI's)."""
    from .ops import MAX_TIME_BUCKETS, TIME_FIELDS
    if isinstance(fields, str) or not isinstance(fields, (list, tuple)):
        raise ValueError(f"{where}: fields must be a list out of {list(TIME_FIELDS)}, got {fields!r}")
    bad = [f for f in fields if f not in TIME_FIELDS]
    if bad or len(set(fields)) != len(fields):
        raise ValueError(f"{where}: unknown or repeated fields {bad or list(fields)} (known: {list(TIME_FIELDS)})")
    if isinstance(buckets, bool) or not isinstance(buckets, int) or not 0 <= buckets <= MAX_TIME_BUCKETS:
        raise ValueError(f"{where}: buckets must be an int in 1..{MAX_TIME_BUCKETS}, got {buckets!r}")
    if "period" in fields and buckets < 1:
        raise ValueError(f"{where}: the 'period' field needs buckets (1..{MAX_TIME_BUCKETS})")
    if "period" not in fields and buckets:
        raise ValueError(f"{where}: buckets is given without the 'period' field")
    return {"fields": tuple(f for f in TIME_FIELDS if f in fields), "buckets": buckets}


LR_SCHEDULE_KEYS = ("warmup_steps", "decay", "decay_steps", "min_ratio")


def optimization_from_dict(doc: dict) -> dict:
    """{global_clipnorm, warmup_steps, decay, decay_steps, min_ratio} of the optional keys ``model.training.global_clipnorm: C``
    and ``model.training.lr_schedule: {warmup_steps, decay, decay_steps, min_ratio}`` (not in the reference's schema): global-norm
    gradient clipping (0: off) and the learning-rate schedule around ``model.training.learning_rate``, its peak.
    ``decay_steps`` is an int or "auto" (train.py: epochs x steps per epoch - warmup_steps).  Without the keys: both off."""
    tr = (doc.get("model") or {}).get("training") or {}
    clip = tr.get("global_clipnorm", 0.0)
    if isinstance(clip, bool) or not isinstance(clip, (int, float)) or not (clip >= 0.0 and math.isfinite(clip)):
        raise ValueError(f"model.training.global_clipnorm must be a finite number >= 0, got {clip!r}")
    block = tr.get("lr_schedule")
    if block is None:
        block = {}
    if not isinstance(block, dict):
        raise ValueError("model.training.lr_schedule must be a mapping {warmup_steps, decay, decay_steps, min_ratio}")
    unknown = sorted(set(block) - set(LR_SCHEDULE_KEYS))
    if unknown:
        raise ValueError(f"model.training.lr_schedule: unknown keys {unknown} (known: {list(LR_SCHEDULE_KEYS)})")
    warm, decay = block.get("warmup_steps", 0), block.get("decay", "none")
    steps, ratio = block.get("decay_steps", 0), block.get("min_ratio", 0.0)
    if isinstance(warm, bool) or not isinstance(warm, int) or warm < 0:
        raise ValueError(f"model.training.lr_schedule.warmup_steps must be an int >= 0, got {warm!r}")
    decay = "none" if decay is None else str(decay).lower()
    if decay not in LR_DECAYS:
        raise ValueError(f"model.training.lr_schedule.decay must be one of {LR_DECAYS}, got {decay!r}")
    if steps != "auto" and (isinstance(steps, bool) or not isinstance(steps, int) or steps < 0):
        raise ValueError(f"model.training.lr_schedule.decay_steps must be an int >= 0 or 'auto', got {steps!r}")
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 <= ratio <= 1.0:
        raise ValueError(f"model.training.lr_schedule.min_ratio must be in [0, 1], got {ratio!r}")
    return {"global_clipnorm": float(clip), "warmup_steps": warm, "decay": decay, "decay_steps": steps, "min_ratio": float(ratio)}


SAMPLING_BIAS_KEYS = ("estimator", "alpha", "hashes", "slots")


def sampling_bias_from_dict(doc: dict) -> dict:
    """{estimator, alpha, hashes, slots} of the optional ``model.retrieval.sampling_bias`` block (not in the reference's schema):
    ``estimator`` streaming - the logQ correction from the streaming frequency estimator (Yi et al. 2019), with the moving-average
    coefficient ``alpha`` and a sketch of ``hashes`` x ``slots`` (0: min(2 * n_items, 2^25)) - or none.  Without the block: none."""
    block = ((doc.get("model") or {}).get("retrieval") or {}).get("sampling_bias")
    d = TwoTowerConfig
    if block is None:
        block = {}
    if not isinstance(block, dict):
        raise ValueError("model.retrieval.sampling_bias must be a mapping {estimator, alpha, hashes, slots}")
    unknown = sorted(set(block) - set(SAMPLING_BIAS_KEYS))
    if unknown:
        raise ValueError(f"model.retrieval.sampling_bias: unknown keys {unknown} (known: {list(SAMPLING_BIAS_KEYS)})")
    est = block.get("estimator", "none")
    est = "none" if est is None else str(est).lower()
    if est not in SAMPLING_BIAS_ESTIMATORS:
        raise ValueError(f"model.retrieval.sampling_bias.estimator must be one of {SAMPLING_BIAS_ESTIMATORS}, got {est!r}")
    alpha, hashes, slots = block.get("alpha", d.freq_alpha), block.get("hashes", d.freq_hashes), block.get("slots", d.freq_slots)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 < alpha <= 1.0:
        raise ValueError(f"model.retrieval.sampling_bias.alpha must be in (0, 1], got {alpha!r}")
    if isinstance(hashes, bool) or not isinstance(hashes, int) or not 1 <= hashes <= 4:
        raise ValueError(f"model.retrieval.sampling_bias.hashes must be an int in 1..4, got {hashes!r}")
    if isinstance(slots, bool) or not isinstance(slots, int) or not 0 <= slots <= 1 << 32:
        raise ValueError(f"model.retrieval.sampling_bias.slots must be an int in 1..2^32 (0: min(2 * n_items, 2^25)), got {slots!r}")
    return {"estimator": est, "alpha": float(alpha), "hashes": hashes, "slots": slots}


RETRIEVAL_LOSS_KEYS = ("kind", "margin", "reduction")
PAIRWISE_REDUCTIONS = ("mean", "sum")


def retrieval_loss_from_dict(doc: dict) -> dict:
    """{kind, margin, reduction} of the optional ``model.retrieval.loss`` block (not in the reference's schema): ``kind``
    softmax (the in-batch sampled softmax, the default) | bpr (pairwise logistic) | hinge (pairwise hinge with ``margin``);
    ``reduction`` mean (every query's sum over its negatives divided by their number) | sum.  Without the block: softmax."""
    block = ((doc.get("model") or {}).get("retrieval") or {}).get("loss")
    d = TwoTowerConfig
    if block is None:
        block = {}
    if not isinstance(block, dict):
        raise ValueError("model.retrieval.loss must be a mapping {kind, margin, reduction}")
    unknown = sorted(set(block) - set(RETRIEVAL_LOSS_KEYS))
    if unknown:
        raise ValueError(f"model.retrieval.loss: unknown keys {unknown} (known: {list(RETRIEVAL_LOSS_KEYS)})")
    kind = str(block.get("kind", d.retrieval_loss)).lower()
    if kind not in RETRIEVAL_LOSSES:
        raise ValueError(f"model.retrieval.loss.kind must be one of {RETRIEVAL_LOSSES}, got {kind!r}")
    margin, reduction = block.get("margin", d.pairwise_margin), str(block.get("reduction", d.pairwise_reduction)).lower()
    if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not math.isfinite(margin):
        raise ValueError(f"model.retrieval.loss.margin must be a finite number, got {margin!r}")
    if reduction not in PAIRWISE_REDUCTIONS:
        raise ValueError(f"model.retrieval.loss.reduction must be one of {PAIRWISE_REDUCTIONS}, got {reduction!r}")
    return {"kind": kind, "margin": float(margin), "reduction": reduction}


def model_config_from_dict(doc: dict, n_users: int, n_items: int, optimizer: str = "adagrad",
                           dropout_override: float | None = None) -> tuple[TwoTowerConfig, dict]:
    """Returns (TwoTowerConfig, training-loop settings {epochs, patience, validation_freq, top_k_eval})."""
    m = doc.get("model")
    if not isinstance(m, dict):
        raise KeyError("config has no 'model:' block (configs/data_config.yaml:54)")
    user_dims, item_dims = list(m["user_tower_dims"]), list(m["item_tower_dims"])
    tr, rt = m.get("training", {}), m.get("retrieval", {})
    sampling = rt.get("candidate_sampling", "in_batch")
    if sampling not in ("in_batch", "mixed"):
        raise NotImplementedError(f"candidate_sampling {sampling!r}: only 'in_batch' and 'mixed' (in-batch plus sampled "
                                  "negatives) are implemented")
    batch_size = int(tr.get("batch_size", 1024))
    # mixed negative sampling: num_sampled_negatives (default: as many as the batch), negative_sampler uniform | unigram,
    # unigram_power - optional keys beside candidate_sampling, not in the reference's schema
    n_neg = int(rt.get("num_sampled_negatives", batch_size)) if sampling == "mixed" else 0
    dropout = float(m.get("dropout_rate", 0.0)) if dropout_override is None else dropout_override
    # not in the reference's schema: model.features.title {buckets, max_tokens, pooling} - the pooled item-title feature
    title = (m.get("features") or {}).get("title") or {}
    # likewise model.features.history {max_items, pooling, heads} - the pooled user-history feature (heads: pooling self_attention)
    hist = (m.get("features") or {}).get("history") or {}
    # likewise model.features.numeric {source: rating_stats | none, clip} - the dense numeric side features (the column counts
    # come from the data: train.py sets n_user_features / n_item_features once it has the matrices)
    numeric = numeric_features_from_dict(doc)
    # likewise model.ranking {weight, hidden_dim} - the rating-prediction head beside the retrieval task
    ranking = ranking_from_dict(doc)
    # likewise model.cross {layers} - DCN-v2 cross layers in both towers
    cross = cross_from_dict(doc)
    # likewise model.layer_norm {enabled, epsilon} - layer normalisation of the towers' hidden layers
    norm = layer_norm_from_dict(doc)
    # likewise model.training.global_clipnorm and model.training.lr_schedule {warmup_steps, decay, decay_steps, min_ratio}
    # (decay_steps "auto": left 0 here - train.py, which knows the number of steps, reads the block itself and resolves it)
    opt = optimization_from_dict(doc)
    # likewise model.retrieval.sampling_bias {estimator, alpha, hashes, slots} - the streaming frequency estimator
    bias = sampling_bias_from_dict(doc)
    # likewise model.features.time {fields, buckets} - the time-of-interaction context features
    when = time_features_from_dict(doc)
    # likewise model.retrieval.loss {kind, margin, reduction} - the pairwise retrieval losses
    rloss = retrieval_loss_from_dict(doc)
    cfg = TwoTowerConfig(
        retrieval_loss=rloss["kind"], pairwise_margin=rloss["margin"], pairwise_reduction=rloss["reduction"],
        time_fields=when["fields"], time_buckets=when["buckets"],
        sampling_bias_estimator=bias["estimator"], freq_alpha=bias["alpha"], freq_hashes=bias["hashes"], freq_slots=bias["slots"],
        global_clipnorm=opt["global_clipnorm"], lr_warmup_steps=opt["warmup_steps"], lr_decay=opt["decay"],
        lr_decay_steps=0 if opt["decay_steps"] == "auto" else opt["decay_steps"], lr_min_ratio=opt["min_ratio"],
        n_users=n_users, n_items=n_items, embedding_dim=int(m["embedding_dim"]), tower_dims=user_dims,
        item_tower_dims=None if item_dims == user_dims else item_dims,
        temperature=float(rt.get("temperature", 1.0)), l2_regularization=float(m.get("l2_regularization", 0.0)),
        learning_rate=float(tr.get("learning_rate", 0.001)), optimizer=optimizer,
        batch_size=batch_size, dropout_rate=dropout,
        candidate_sampling=sampling, n_sampled_negatives=n_neg, negative_sampler=str(rt.get("negative_sampler", "uniform")),
        unigram_power=float(rt.get("unigram_power", 0.75)),
        # not in the reference's schema (left open): an optional key beside retrieval.temperature
        normalize_embeddings=bool(rt.get("normalize_embeddings", False)),
        user_history_len=int(hist.get("max_items", 0)), history_pooling=str(hist.get("pooling", "mean")),
        history_heads=int(hist.get("heads", 1)),
        feature_clip=numeric["clip"], rating_weight=ranking["weight"], rating_hidden=ranking["hidden_dim"],
        n_title_buckets=int(title.get("buckets", 0)), title_max_tokens=int(title.get("max_tokens", 16)),
        title_pooling=str(title.get("pooling", "mean")), cross_layers=cross["layers"],
        layer_norm=norm["enabled"], layer_norm_epsilon=norm["epsilon"])
    loop = dict(epochs=int(tr.get("epochs", 1)), patience=int(tr.get("patience", 5)),
                validation_freq=int(tr.get("validation_freq", 1)), top_k_eval=list(rt.get("top_k_eval", [])))
    return cfg, loop
