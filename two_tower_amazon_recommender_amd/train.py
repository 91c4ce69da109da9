"""``train-model`` / ``python -m two_tower_amazon_recommender_amd.train --config <yaml>`` — the training
entry point the reference declares (``/root/reference/pyproject.toml:67`` ``train-model =
"src.training.train:main"``; ``README.md:39`` ``python src/training/train.py --config ...``) but does not
ship.  Reads the ``model:`` block of the reference's YAML schema (``configs/data_config.yaml:54-71``) and the
parquet written by ``prepare_training_data.py:216-218``; runs every step on the HIP kernels (one GPU here;
under ``python -m torch.distributed.run --nproc-per-node N`` — or with ``--distributed`` — one process per GPU on the
row-sharded trainer of ``sharded.py``: every rank trains on its slice of the interactions, tables are sharded by
``id % N``, collectives go over RCCL).
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import time

import numpy as np
import torch

from . import config as cfgmod
from . import data as datamod
from .trainer import TwoTowerTrainer

log = logging.getLogger("train")


class EarlyStopping:
    """`model.training.patience` of the reference's schema (configs/data_config.yaml:65): stop after `patience`
    consecutive evaluations without an improvement of the validation loss by more than `min_delta`."""

    def __init__(self, patience: int, min_delta: float = 1e-6):
        self.patience, self.min_delta = int(patience), float(min_delta)
        self.best, self.bad = float("inf"), 0

    def update(self, value: float) -> bool:
        """Record one evaluation; returns True when training should stop."""
        if value < self.best - self.min_delta:
            self.best, self.bad = value, 0
        else:
            self.bad += 1
        return self.bad >= self.patience

    def state_dict(self) -> dict:
        return {"best": self.best, "bad": self.bad}

    def load_state_dict(self, sd: dict):
        self.best, self.bad = float(sd["best"]), int(sd["bad"])


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Train the two-tower retrieval model on MI355X (HIP kernels).")
    ap.add_argument("--config", required=True, help="YAML with a `model:` block (configs/data_config.yaml schema)")
    ap.add_argument("--data", default="data/processed/combined_interactions.parquet")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="train on N synthetic interactions instead of --data")
    ap.add_argument("--synthetic-users", type=int, default=10_000)
    ap.add_argument("--synthetic-items", type=int, default=10_000)
    ap.add_argument("--optimizer", default="adagrad", choices=["sgd", "adagrad", "adam", "rowwise_adagrad"],
                    help="adam = lazy Adam (only the rows of a batch's ids are touched): what model.training.learning_rate 0.001 "
                         "is the Keras default of; rowwise_adagrad = one Adagrad accumulator per embedding row (the mean of the "
                         "row's squared gradient; rows instead of rows x dim floats of state), element-wise Adagrad on the dense "
                         "parameters; both: single-GPU trainer only")
    ap.add_argument("--adam-beta1", type=float, default=0.9)
    ap.add_argument("--adam-beta2", type=float, default=0.999)
    ap.add_argument("--adam-epsilon", type=float, default=1e-7)
    ap.add_argument("--category-buckets", type=int, default=0, metavar="N",
                    help="add the hashed category feature: the pair's category (column category / main_category / "
                         "category_encoded) hashed into N buckets, its embedding summed into the item tower input")
    ap.add_argument("--sampling-bias-estimator", default=None, choices=["none", "streaming"],
                    help="streaming = the logQ correction from the streaming frequency estimator (Yi et al. 2019): a hashed sketch of "
                         "every item's gap between sightings, updated by each train batch - no count over the training split; "
                         "replaces --correct-sampling-bias (pick one; overrides model.retrieval.sampling_bias.estimator); "
                         "single-GPU trainer only")
    ap.add_argument("--freq-alpha", type=float, default=None, metavar="A",
                    help="moving-average coefficient of the estimator, in (0, 1] (default model.retrieval.sampling_bias.alpha, else 0.01)")
    ap.add_argument("--freq-hashes", type=int, default=None, metavar="H", help="hash rows of the estimator's sketch (1..4; default 2)")
    ap.add_argument("--freq-slots", type=int, default=None, metavar="M",
                    help="slots per hash row (default 0: min(2 x items, 2^25))")
    ap.add_argument("--title-buckets", type=int, default=None, metavar="N",
                    help="add the pooled item-title feature: every item's title (column title) is tokenised, its first "
                         "--title-max-tokens tokens are hashed into N buckets and their embeddings pooled into the item tower "
                         "input (overrides model.features.title.buckets); single-GPU trainer only")
    ap.add_argument("--title-max-tokens", type=int, default=None, metavar="L", help="title tokens kept per item (1..64; default 16)")
    ap.add_argument("--title-pooling", default=None, choices=["sum", "mean", "sqrtn"], help="how the token rows are pooled (default mean)")
    ap.add_argument("--history-len", type=int, default=None, metavar="L",
                    help="add the pooled user-history feature: every user's last L training interactions (1..64, by the "
                         "timestamp column where there is one) are pooled into the user tower input, the pair's own item left "
                         "out (overrides model.features.history.max_items); single-GPU trainer only")
    ap.add_argument("--history-pooling", default=None, choices=["sum", "mean", "sqrtn", "attention", "gru", "self_attention"],
                    help="how the history rows are pooled (default mean; attention: a learned query with a recency bias; gru: a GRU "
                         "over the items, oldest first; self_attention: multi-head self-attention with the newest item as the query)")
    ap.add_argument("--history-heads", type=int, default=None, choices=[1, 2, 4, 8], metavar="H",
                    help="heads of --history-pooling self_attention (1, 2, 4 or 8; default 1; overrides "
                         "model.features.history.heads)")
    ap.add_argument("--side-features", default=None, choices=["none", "rating_stats"],
                    help="add the dense numeric side features: rating_stats = every user's and every item's rating count / mean / "
                         "std / min / max over the training pairs (column rating), normalised, projected by a trained kernel and "
                         "added to the tower inputs (overrides model.features.numeric.source); single-GPU trainer only")
    ap.add_argument("--feature-clip", type=float, default=None, metavar="C",
                    help="clamp the normalised features to [-C, C] (0: no clipping; overrides model.features.numeric.clip)")
    ap.add_argument("--user-features", default=None, metavar="FILE.npy",
                    help="an external [n_users, F] f32 matrix (F in 1..32) of numeric user features; takes precedence over "
                         "rating_stats on the user side")
    ap.add_argument("--item-features", default=None, metavar="FILE.npy", help="likewise [n_items, F] for the item side")
    ap.add_argument("--time-features", default=None, metavar="FIELDS",
                    help="add the time-of-interaction context features: a comma-separated subset of hour,day_of_week,month,period "
                         "(or none) - the rows the pair's timestamp (column timestamp) picks in one small trained table are added to "
                         "the user tower input (overrides model.features.time.fields); single-GPU trainer only")
    ap.add_argument("--time-buckets", type=int, default=None, metavar="N",
                    help="rows of the period field: N equal periods of the training split's time range (1..4096; later pairs land in "
                         "the last one; overrides model.features.time.buckets)")
    ap.add_argument("--rating-weight", type=float, default=None, metavar="W",
                    help="add the rating-prediction head (joint retrieval + ranking): one hidden ReLU layer over the pair's two "
                         "tower outputs trained with MSE on the rating column, total loss = retrieval + W * MSE (overrides "
                         "model.ranking.weight; 0: no head); single-GPU trainer only")
    ap.add_argument("--rating-hidden", type=int, default=None, metavar="H",
                    help="hidden width of the rating head (a multiple of 32 in 32..256; default model.ranking.hidden_dim, else 128)")
    ap.add_argument("--cross-layers", type=int, default=None, metavar="L",
                    help="DCN-v2 cross layers (0..3) in both towers, between the summed input features and the Dense stack: "
                         "x_{l+1} = x_0 * (x_l W_l + b_l) + x_l (overrides model.cross.layers; 0: none; embedding_dim must be a "
                         "multiple of 32 in 32..256); single-GPU trainer only")
    ap.add_argument("--layer-norm", action="store_true",
                    help="layer normalisation (Keras LayerNormalization) between every hidden Dense layer of both towers and its "
                         "ReLU (overrides model.layer_norm.enabled to true; hidden widths must be multiples of 32 in 32..1024); "
                         "single-GPU trainer only")
    ap.add_argument("--layer-norm-epsilon", type=float, default=None, metavar="E",
                    help="epsilon inside the normalisation's square root (default model.layer_norm.epsilon, else Keras's 1e-3)")
    ap.add_argument("--global-clipnorm", type=float, default=None, metavar="C",
                    help="clip every step's gradient to the global norm C (Keras global_clipnorm / tf.clip_by_global_norm over the "
                         "dense gradients and the embedding rows, two launches; overrides model.training.global_clipnorm; 0: off); "
                         "single-GPU trainer only")
    ap.add_argument("--lr-warmup-steps", type=int, default=None, metavar="W",
                    help="linear warm-up of the learning rate over the first W steps (overrides model.training.lr_schedule.warmup_steps)")
    ap.add_argument("--lr-decay", default=None, choices=["none", "cosine", "linear", "inverse_sqrt"],
                    help="how the rate falls from its peak (model.training.learning_rate) after the warm-up")
    ap.add_argument("--lr-decay-steps", default=None, metavar="N|auto",
                    help="steps of the cosine / linear decay; auto = epochs x steps per epoch - warm-up steps")
    ap.add_argument("--lr-min-ratio", type=float, default=None, metavar="M", help="floor of the decayed rate as a fraction of the peak (0..1)")
    ap.add_argument("--correct-sampling-bias", action="store_true",
                    help="pass every candidate's empirical frequency as candidate_sampling_probability (the logQ correction "
                         "of tfrs.tasks.Retrieval): in-batch negatives otherwise push popular items down")
    ap.add_argument("--candidate-sampling", default=None, choices=["in_batch", "mixed"],
                    help="mixed = mixed negative sampling: every step appends --sampled-negatives items drawn from the whole "
                         "catalogue to the in-batch candidates (overrides model.retrieval.candidate_sampling); with "
                         "--correct-sampling-bias the correction uses the probability of the mixture; single-GPU trainer only")
    ap.add_argument("--sampled-negatives", type=int, default=None, metavar="N",
                    help="sampled negatives per step with mixed sampling (default: model.retrieval.num_sampled_negatives, else the batch size)")
    ap.add_argument("--negative-sampler", default=None, choices=["uniform", "unigram"],
                    help="how the sampled negatives are drawn: uniformly, or from the items' training frequency to the power "
                         "--unigram-power (word2vec's unigram^0.75)")
    ap.add_argument("--unigram-power", type=float, default=None)
    ap.add_argument("--scorer-precision", default="f32", choices=["f32", "bf16x3"],
                    help="matrix products of the scorer + softmax loss: exact f32 (default) or f32-emulated split-bf16 on the "
                         "bf16 matrix cores (scorer dim 128 / 256; same 1e-4 parity bars, ~2x faster scorer)")
    ap.add_argument("--retrieval-loss", default=None, choices=["softmax", "bpr", "hinge"],
                    help="the retrieval loss over the step's candidates: softmax (the in-batch sampled softmax, default), bpr "
                         "(pairwise logistic) or hinge (pairwise hinge with --pairwise-margin), on the same logits (overrides "
                         "model.retrieval.loss.kind); exact f32, single-GPU trainer only")
    ap.add_argument("--pairwise-margin", type=float, default=None, metavar="M",
                    help="margin of the pairwise hinge loss (default model.retrieval.loss.margin, else 1.0)")
    ap.add_argument("--pairwise-reduction", default=None, choices=["mean", "sum"],
                    help="mean: every query's sum over its negatives is divided by their number (default); sum: it is not")
    ap.add_argument("--normalize-embeddings", action="store_true",
                    help="L2-normalise both towers' outputs before the scorer (cosine scoring; overrides "
                         "model.retrieval.normalize_embeddings to true); single-GPU trainer only")
    ap.add_argument("--epochs", type=int, default=None, help="override model.training.epochs")
    ap.add_argument("--batch-size", type=int, default=None, help="override model.training.batch_size")
    ap.add_argument("--val-fraction", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--save", default=None, help="write a checkpoint (torch.save of tensors) here at the end "
                                                 "(distributed: one file per rank, <path>.rank<r>of<N>)")
    ap.add_argument("--resume", default=None, help="continue from a checkpoint written by --save (distributed: the "
                                                   "<path>.rank<r>of<N> files of the same world size)")
    ap.add_argument("--distributed", action="store_true",
                    help="use the row-sharded multi-GPU trainer (implied when WORLD_SIZE > 1); batch_size is per rank")
    ap.add_argument("--negatives", default="local", choices=["local", "global"],
                    help="distributed: in-batch negatives of the rank's own batch (what tfrs.tasks.Retrieval sees under a "
                         "data-parallel strategy) or of the all-gathered global batch")
    return ap.parse_args(argv)


def retrieval_loss_settings(args, doc: dict, distributed: bool) -> dict:
    """{kind, margin, reduction} of the run: the ``model.retrieval.loss`` block overridden by --retrieval-loss / --pairwise-margin /
    --pairwise-reduction, with the refusals of a pairwise loss (bf16x3 scorer precision, the row-sharded trainer)."""
    rloss = cfgmod.retrieval_loss_from_dict(doc)
    for key, arg in (("kind", args.retrieval_loss), ("margin", args.pairwise_margin), ("reduction", args.pairwise_reduction)):
        if arg is not None:
            rloss[key] = arg
    if not np.isfinite(rloss["margin"]):
        raise SystemExit("--pairwise-margin must be a finite number")
    if rloss["kind"] == "softmax":
        if args.pairwise_margin is not None or args.pairwise_reduction is not None:
            raise SystemExit("--pairwise-margin / --pairwise-reduction need a pairwise loss: --retrieval-loss bpr | hinge (or "
                             "model.retrieval.loss.kind)")
        return rloss
    if args.scorer_precision != "f32":
        raise SystemExit(f"--retrieval-loss {rloss['kind']} needs --scorer-precision f32: the pairwise kernels are exact f32 only")
    if distributed:
        raise NotImplementedError("a pairwise retrieval loss (bpr / hinge) is not implemented for the row-sharded (--distributed) "
                                  "trainer")
    return rloss


def main(argv=None) -> int:
    args = parse(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    doc = cfgmod.load_yaml(args.config)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    distributed = args.distributed or world > 1
    normalize = args.normalize_embeddings or bool(((doc.get("model") or {}).get("retrieval") or {}).get("normalize_embeddings", False))
    if distributed and normalize:
        raise NotImplementedError("normalize_embeddings is not implemented for the row-sharded (--distributed) trainer")
    title_cfg = ((doc.get("model") or {}).get("features") or {}).get("title") or {}
    title_buckets = int(title_cfg.get("buckets", 0)) if args.title_buckets is None else args.title_buckets
    if distributed and title_buckets:
        raise NotImplementedError("the title feature is not implemented for the row-sharded (--distributed) trainer")
    hist_cfg = ((doc.get("model") or {}).get("features") or {}).get("history") or {}
    history_len = int(hist_cfg.get("max_items", 0)) if args.history_len is None else args.history_len
    if distributed and history_len:
        raise NotImplementedError("the user-history feature is not implemented for the row-sharded (--distributed) trainer")
    numeric = cfgmod.numeric_features_from_dict(doc)
    side_source = numeric["source"] if args.side_features is None else args.side_features
    if distributed and (side_source != "none" or args.user_features or args.item_features):
        raise NotImplementedError("the numeric side features are not implemented for the row-sharded (--distributed) trainer")
    ranking = cfgmod.ranking_from_dict(doc)
    rating_weight = ranking["weight"] if args.rating_weight is None else args.rating_weight
    rating_hidden = ranking["hidden_dim"] if args.rating_hidden is None else args.rating_hidden
    if not (rating_weight >= 0.0 and np.isfinite(rating_weight)):
        raise SystemExit("--rating-weight must be a finite number >= 0")
    if not (32 <= rating_hidden <= 256 and rating_hidden % 32 == 0):
        raise SystemExit("--rating-hidden must be a multiple of 32 in 32..256")
    if args.rating_hidden is not None and not rating_weight > 0:
        raise SystemExit("--rating-hidden needs a rating head: --rating-weight W > 0 (or model.ranking.weight)")
    if distributed and rating_weight > 0:
        raise NotImplementedError("the rating head is not implemented for the row-sharded (--distributed) trainer")
    cross_layers = cfgmod.cross_from_dict(doc)["layers"] if args.cross_layers is None else args.cross_layers
    if not 0 <= cross_layers <= 3:
        raise SystemExit("--cross-layers must be in 0..3")
    if distributed and cross_layers:
        raise NotImplementedError("the cross layers are not implemented for the row-sharded (--distributed) trainer")
    norm = cfgmod.layer_norm_from_dict(doc)
    layer_norm = args.layer_norm or norm["enabled"]
    layer_norm_eps = norm["epsilon"] if args.layer_norm_epsilon is None else args.layer_norm_epsilon
    if not (layer_norm_eps > 0 and np.isfinite(layer_norm_eps)):
        raise SystemExit("--layer-norm-epsilon must be a finite number > 0")
    if args.layer_norm_epsilon is not None and not layer_norm:
        raise SystemExit("--layer-norm-epsilon needs --layer-norm (or model.layer_norm.enabled)")
    if distributed and layer_norm:
        raise NotImplementedError("layer normalisation is not implemented for the row-sharded (--distributed) trainer")
    when = cfgmod.time_features_from_dict(doc)
    if args.time_features is not None or args.time_buckets is not None:
        fields = when["fields"] if args.time_features is None else \
            [f for f in args.time_features.split(",") if f and f != "none"]
        buckets = args.time_buckets if args.time_buckets is not None else when["buckets"] if "period" in fields else 0
        try:
            when = cfgmod.check_time_features(list(fields), buckets, "--time-features / --time-buckets")
        except ValueError as e:
            raise SystemExit(str(e))
    if distributed and when["fields"]:
        raise NotImplementedError("the time context features are not implemented for the row-sharded (--distributed) trainer")
    sched = cfgmod.optimization_from_dict(doc)
    for key, arg in (("global_clipnorm", args.global_clipnorm), ("warmup_steps", args.lr_warmup_steps), ("decay", args.lr_decay),
                     ("min_ratio", args.lr_min_ratio)):
        if arg is not None:
            sched[key] = arg
    if args.lr_decay_steps is not None:
        if args.lr_decay_steps != "auto" and not args.lr_decay_steps.isdigit():
            raise SystemExit("--lr-decay-steps must be a non-negative integer or 'auto'")
        sched["decay_steps"] = "auto" if args.lr_decay_steps == "auto" else int(args.lr_decay_steps)
    if not (sched["global_clipnorm"] >= 0.0 and np.isfinite(sched["global_clipnorm"])):
        raise SystemExit("--global-clipnorm must be a finite number >= 0")
    if sched["warmup_steps"] < 0:
        raise SystemExit("--lr-warmup-steps must be >= 0")
    if not 0.0 <= sched["min_ratio"] <= 1.0:
        raise SystemExit("--lr-min-ratio must be in [0, 1]")
    if distributed and sched["global_clipnorm"] > 0:
        raise NotImplementedError("gradient clipping (global_clipnorm) is not implemented for the row-sharded (--distributed) trainer")
    if distributed and (sched["warmup_steps"] > 0 or sched["decay"] != "none"):
        raise NotImplementedError("a learning-rate schedule is not implemented for the row-sharded (--distributed) trainer")
    rloss = retrieval_loss_settings(args, doc, distributed)
    sampling = args.candidate_sampling or ((doc.get("model") or {}).get("retrieval") or {}).get("candidate_sampling", "in_batch")
    if distributed and sampling == "mixed":
        raise NotImplementedError("candidate_sampling 'mixed' is not implemented for the row-sharded (--distributed) trainer")
    bias = cfgmod.sampling_bias_from_dict(doc)
    for key, arg in (("estimator", args.sampling_bias_estimator), ("alpha", args.freq_alpha), ("hashes", args.freq_hashes),
                     ("slots", args.freq_slots)):
        if arg is not None:
            bias[key] = arg
    if bias["estimator"] == "streaming" and args.correct_sampling_bias:
        raise SystemExit("--sampling-bias-estimator streaming and --correct-sampling-bias both turn the logQ correction on, from "
                         "the streaming estimator and from a count over the training split: pick one")
    if distributed and bias["estimator"] == "streaming":
        raise NotImplementedError("the streaming frequency estimator is not implemented for the row-sharded (--distributed) trainer")
    if distributed and args.optimizer == "adam":
        raise NotImplementedError("optimizer 'adam' is not implemented for the row-sharded (--distributed) trainer")
    if distributed and args.optimizer == "rowwise_adagrad":
        raise NotImplementedError("optimizer 'rowwise_adagrad' is not implemented for the row-sharded (--distributed) trainer")
    if distributed:
        import torch.distributed as dist
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if world > 1 or "LOCAL_RANK" in os.environ:
            args.device = f"cuda:{local_rank}"
        torch.cuda.set_device(torch.device(args.device))
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29511")):
            os.environ.setdefault(k, v)
        if not dist.is_initialized():
            dist.init_process_group("nccl", device_id=torch.device(args.device))
    if args.synthetic:
        from . import ops
        dev = torch.device(args.device)
        u = torch.empty(args.synthetic, dtype=torch.int64, device=dev)
        i = torch.empty(args.synthetic, dtype=torch.int64, device=dev)
        ops.fill_ids_(u, args.seed, 3, args.synthetic_users, "Z")
        ops.fill_ids_(i, args.seed, 4, args.synthetic_items, "Z")
        user_idx, item_idx = u.cpu().numpy(), i.cpu().numpy()
        n_users, n_items = args.synthetic_users, args.synthetic_items
        cat = None
        if args.category_buckets:
            c = torch.empty(args.synthetic, dtype=torch.int64, device=dev)
            ops.fill_ids_(c, args.seed, 6, args.category_buckets, "Z")
            cat = c.cpu().numpy()
    else:
        user_idx, item_idx = datamod.read_interactions(args.data)
        n_users, n_items = int(user_idx.max()) + 1, int(item_idx.max()) + 1
        cat = None
        if args.category_buckets:
            cv = datamod.read_category_values(args.data)
            if cv is None:
                raise SystemExit(f"--category-buckets: {args.data} has none of the columns {datamod.CATEGORY_COLUMNS}")
            cat = datamod.category_buckets(cv[0], cv[1], args.category_buckets, torch.device(args.device))
    cfg, loop = cfgmod.model_config_from_dict(doc, n_users, n_items, optimizer=args.optimizer)
    cfg.n_category_buckets = args.category_buckets
    cfg.scorer_precision = args.scorer_precision
    cfg.retrieval_loss, cfg.pairwise_margin, cfg.pairwise_reduction = rloss["kind"], float(rloss["margin"]), rloss["reduction"]
    cfg.normalize_embeddings = normalize
    cfg.adam_beta1, cfg.adam_beta2, cfg.adam_epsilon = args.adam_beta1, args.adam_beta2, args.adam_epsilon
    cfg.n_title_buckets = title_buckets
    cfg.rating_weight, cfg.rating_hidden = float(rating_weight), int(rating_hidden)
    cfg.cross_layers = int(cross_layers)
    cfg.layer_norm, cfg.layer_norm_epsilon = bool(layer_norm), float(layer_norm_eps)
    if args.title_max_tokens is not None:
        cfg.title_max_tokens = args.title_max_tokens
    if args.title_pooling is not None:
        cfg.title_pooling = args.title_pooling
    cfg.user_history_len = history_len
    if args.history_pooling is not None:
        cfg.history_pooling = args.history_pooling
    if args.history_heads is not None:
        cfg.history_heads = args.history_heads
    if args.batch_size:
        cfg.batch_size = args.batch_size
    cfg.sampling_bias_estimator = bias["estimator"]
    cfg.freq_alpha, cfg.freq_hashes, cfg.freq_slots = float(bias["alpha"]), int(bias["hashes"]), int(bias["slots"])
    if args.candidate_sampling is not None:
        cfg.candidate_sampling = args.candidate_sampling
    if cfg.candidate_sampling == "mixed":
        if args.sampled_negatives is not None:
            cfg.n_sampled_negatives = args.sampled_negatives
        elif "num_sampled_negatives" not in ((doc.get("model") or {}).get("retrieval") or {}):   # default: as many as the batch
            cfg.n_sampled_negatives = cfg.batch_size
        if args.negative_sampler is not None:
            cfg.negative_sampler = args.negative_sampler
        if args.unigram_power is not None:
            cfg.unigram_power = args.unigram_power
    else:
        cfg.n_sampled_negatives = 0
        if args.sampled_negatives:
            raise SystemExit("--sampled-negatives needs --candidate-sampling mixed")
    epochs = args.epochs if args.epochs is not None else loop["epochs"]
    n = len(user_idx)
    n_val = int(n * args.val_fraction)
    rng = np.random.default_rng(args.seed)
    perm = rng.permutation(n)
    tr_idx, va_idx = perm[n_val:], perm[:n_val]
    log.info("users %d items %d interactions %d (train %d, val %d); batch %d; optimizer %s", n_users, n_items, n,
             len(tr_idx), len(va_idx), cfg.batch_size, cfg.optimizer)
    # time context features: every pair's int64 timestamp; the periods cut the range of the TRAINING split's finite timestamps
    cfg.time_fields, cfg.time_buckets = when["fields"], when["buckets"]
    stamps = None
    if cfg.time_fields:
        if args.synthetic:                  # synthetic interactions carry no timestamp: five years from 2001-09-09, from the run's seed
            from . import ops
            t = torch.empty(n, dtype=torch.int64, device=torch.device(args.device))
            ops.fill_ids_(t, args.seed, 61, 5 * 365 * 86400, "U")
            stamps = t.cpu().numpy() + 1_000_000_000
        else:
            ts = datamod.read_timestamps(args.data)
            if ts is None:
                raise SystemExit(f"--time-features: {args.data} has no column {datamod.TIMESTAMP_COLUMN!r}")
            stamps = datamod.timestamps_to_int64(ts)
        seen = stamps[tr_idx][stamps[tr_idx] != datamod.TIME_MISSING]
        if not seen.size:
            raise SystemExit("--time-features: no training pair has a finite timestamp")
        cfg.time_min, cfg.time_max = int(seen.min()), int(seen.max())
        if cfg.time_max - cfg.time_min >= 2 ** 40:
            raise SystemExit(f"--time-features: the training timestamps span {cfg.time_max - cfg.time_min} s; whole seconds since the "
                             "epoch are expected (a range below 2^40)")
        log.info("time features %s (period buckets %d) over [%d, %d]", cfg.time_fields, cfg.time_buckets, cfg.time_min, cfg.time_max)
    histories = None
    if cfg.user_history_len:                # the TRAINING pairs only, in the order of the timestamps (else: of the file)
        rows = np.sort(tr_idx)
        ts = None if args.synthetic else datamod.read_timestamps(args.data)
        histories = datamod.user_histories(user_idx[rows], item_idx[rows], n_users, cfg.user_history_len,
                                           None if ts is None else ts[rows])
    # numeric side features: an external matrix per side, else the rating statistics of the TRAINING pairs
    side_features = {"user": None, "item": None}
    need_stats = side_source == "rating_stats" and not (args.user_features and args.item_features)
    rating = None
    if need_stats or cfg.rating_weight > 0:
        if args.synthetic:                  # synthetic interactions carry no rating: stars 1..5 from the run's seed
            rating = np.random.default_rng(args.seed + 1).integers(1, 6, size=n).astype(np.float64)
        else:
            rating = datamod.read_ratings(args.data)
            if rating is None:
                raise SystemExit(f"{'--rating-weight' if cfg.rating_weight > 0 else '--side-features rating_stats'}: {args.data} "
                                 f"has no column {datamod.RATING_COLUMN!r}")
    if need_stats:
        side_features["user"], side_features["item"] = datamod.rating_features(user_idx[tr_idx], item_idx[tr_idx], rating[tr_idx],
                                                                               n_users, n_items)
    for side, path, rows in (("user", args.user_features, n_users), ("item", args.item_features, n_items)):
        if path:
            x = np.load(path)
            if x.ndim != 2 or x.shape[0] != rows or not 1 <= x.shape[1] <= 32:
                raise SystemExit(f"--{side}-features: {path} must hold a [{rows}, 1..32] matrix, got shape {tuple(x.shape)}")
            side_features[side] = x.astype(np.float32)
    cfg.n_user_features = 0 if side_features["user"] is None else side_features["user"].shape[1]
    cfg.n_item_features = 0 if side_features["item"] is None else side_features["item"].shape[1]
    if args.feature_clip is not None:
        cfg.feature_clip = args.feature_clip
    if distributed:
        # every rank computed the same split; it trains on every world-th pair, cut so all ranks run the same number
        # of (collective) steps
        from .sharded import ShardedTwoTowerTrainer
    # whole (global) batches only — the kernels' buffers are sized for one batch size — then every world-th pair
    per = cfg.batch_size * world
    tr_idx = tr_idx[:len(tr_idx) // per * per][rank::world]
    va_idx = va_idx[:len(va_idx) // per * per][rank::world]
    if len(tr_idx) < cfg.batch_size:
        raise SystemExit(f"only {len(tr_idx)} training interactions per rank for batch_size {cfg.batch_size}")
    cfg.global_clipnorm = float(sched["global_clipnorm"])
    cfg.lr_warmup_steps, cfg.lr_decay, cfg.lr_min_ratio = int(sched["warmup_steps"]), sched["decay"], float(sched["min_ratio"])
    if sched["decay_steps"] == "auto":          # the whole run behind the warm-up: epochs x steps per epoch - warmup_steps
        cfg.lr_decay_steps = max(epochs * (len(tr_idx) // cfg.batch_size) - cfg.lr_warmup_steps, 1)
    else:
        cfg.lr_decay_steps = int(sched["decay_steps"])
    if cfg.lr_schedule_on or cfg.global_clipnorm > 0:
        log.info("global_clipnorm %g; learning rate: peak %g, warm-up %d steps, decay %s over %d steps, floor %g x peak",
                 cfg.global_clipnorm, cfg.learning_rate, cfg.lr_warmup_steps, cfg.lr_decay, cfg.lr_decay_steps, cfg.lr_min_ratio)
    if distributed:
        trainer = ShardedTwoTowerTrainer(cfg, args.device, seed=args.seed, negatives=args.negatives)
    else:
        trainer = TwoTowerTrainer(cfg, args.device, seed=args.seed)
    if histories is not None:
        trainer.set_user_histories(torch.from_numpy(histories).to(trainer.dev))
    if side_features["user"] is not None:       # the normalisation is adapted from the matrix (Keras Normalization.adapt)
        trainer.set_user_features(side_features["user"])
    if side_features["item"] is not None:
        trainer.set_item_features(side_features["item"])
    if cfg.n_title_buckets:
        if args.synthetic:                  # tokens from the id generator
            trainer.set_item_titles(trainer.synthetic_item_titles(args.seed))
        else:
            titles = datamod.read_item_titles(args.data, item_idx, n_items)
            trainer.set_item_titles(datamod.title_tokens(titles, cfg.n_title_buckets, cfg.title_max_tokens, trainer.dev))

    def total(x: torch.Tensor) -> float:        # sum over ranks of a device scalar
        if distributed:
            dist.all_reduce(x)
        return x.item()
    train_it = datamod.BatchIterator(user_idx[tr_idx], item_idx[tr_idx], cfg.batch_size, trainer.dev, args.seed,
                                     category_bucket=None if cat is None else cat[tr_idx],
                                     ratings=rating[tr_idx] if cfg.rating_weight > 0 else None,
                                     timestamps=None if stamps is None else stamps[tr_idx])
    val_it = datamod.BatchIterator(user_idx[va_idx], item_idx[va_idx], cfg.batch_size, trainer.dev, args.seed, shuffle=False,
                                   category_bucket=None if cat is None else cat[va_idx],
                                   ratings=rating[va_idx] if cfg.rating_weight > 0 else None,
                                   timestamps=None if stamps is None else stamps[va_idx])

    item_prob = None
    mixed = cfg.candidate_sampling == "mixed"
    if args.correct_sampling_bias or (mixed and cfg.negative_sampler == "unigram"):
        # P(item j is drawn as an in-batch candidate) = its share of the training pairs
        counts = torch.from_numpy(np.bincount(item_idx[tr_idx], minlength=n_items).astype(np.float64)).to(trainer.dev)
        if distributed:                     # the candidates' frequencies over ALL ranks' training pairs
            dist.all_reduce(counts)
        item_prob = (counts / counts.sum()).to(torch.float32)
        if mixed:       # the trainer owns the correction: the sampler launch writes the mixture's probability of every candidate
            trainer.set_item_frequencies(item_prob)
        if mixed or not args.correct_sampling_bias:
            item_prob = None

    def kw(batch):
        k = {"category_ids": batch[2]} if cat is not None else {}
        if stamps is not None:              # the pairs' timestamps come last
            k["timestamps"], batch = batch[-1], batch[:-1]
        if cfg.rating_weight > 0:           # the pairs' ratings ride behind the ids (NaN: no label)
            k["ratings"] = batch[-1]
        if item_prob is not None:
            k["candidate_sampling_probability"] = item_prob[batch[1]]
        return k
    stopper, history, first_epoch = EarlyStopping(loop["patience"]), [], 0
    if args.resume:
        path = f"{args.resume}.rank{rank}of{world}" if distributed else args.resume
        ck = torch.load(path, map_location=trainer.dev, weights_only=True)       # plain tensors / numbers only
        trainer.load_state_dict(ck)
        first_epoch = int(ck.get("epoch", 0))
        if "early_stopping" in ck:
            stopper.load_state_dict(ck["early_stopping"])
        log.info("resumed from %s (epoch %d, step %d)", path, first_epoch, trainer.step_index)
    if cfg.rating_weight > 0 and not args.resume:        # a fresh head starts from the constant predictor: the mean training rating
        finite = rating[tr_idx][np.isfinite(rating[tr_idx])]
        if finite.size:
            trainer.init_rating_bias(float(finite.mean()))
    for epoch in range(first_epoch, epochs):
        t0 = time.perf_counter()
        tot = torch.zeros((), device=trainer.dev, dtype=torch.float64)
        for batch in train_it:
            tot.add_(trainer.step(batch[0], batch[1], **kw(batch)).view(()))      # (one mixed-precision add: f64 += f32)
        torch.cuda.synchronize()
        trainer.check_ids()
        dt = time.perf_counter() - t0
        rec = {"epoch": epoch + 1, "train_loss_per_pair": total(tot) / (len(train_it) * cfg.batch_size * world),
               "pairs_per_sec": len(train_it) * cfg.batch_size * world / dt}
        # of the epoch's last step (the norm is read behind the synchronise above: no extra one)
        rec["lr"] = cfg.learning_rate if distributed else trainer.learning_rate
        if cfg.global_clipnorm > 0:
            rec["grad_norm"] = trainer.grad_norm.item()
        if len(val_it) and (epoch + 1) % loop["validation_freq"] == 0:
            vt = torch.zeros((), device=trainer.dev, dtype=torch.float64)
            vse = torch.zeros((), device=trainer.dev, dtype=torch.float64)
            vcount = torch.zeros((), device=trainer.dev, dtype=torch.float64)
            for batch in val_it:
                vt.add_(trainer.evaluate(batch[0], batch[1], **kw(batch)).view(()))
                if cfg.rating_weight > 0:
                    vse.add_(trainer.eval_rating_se); vcount.add_(trainer.eval_rating_count)
            rec["val_loss_per_pair"] = total(vt) / (len(val_it) * cfg.batch_size * world)
            if cfg.rating_weight > 0:       # RMSE over the held-out pairs with a finite rating (early stopping stays on the loss above)
                rec["val_rating_rmse"] = float(np.sqrt(vse.item() / max(vcount.item(), 1.0)))
            stop = stopper.update(rec["val_loss_per_pair"])
        else:
            stop = False
        history.append(rec)
        log.info(json.dumps(rec))
        last_epoch = epoch + 1
        if stop:                                         # early stopping (configs/data_config.yaml:65)
            log.info("early stop: no validation improvement for %d evaluations", stopper.bad)
            break
    final = {"history": history}
    if loop["top_k_eval"] and len(val_it):
        # retrieval quality on the held-out pairs against the WHOLE item corpus (configs/data_config.yaml:71 top_k_eval)
        from .metrics import FactorizedTopK
        metric = FactorizedTopK(ks=tuple(loop["top_k_eval"]), temperature=cfg.temperature)
        item_cat = None
        if cat is not None:             # an item's category = the bucket of its first interaction (items never seen: bucket 0)
            item_cat = torch.from_numpy(datamod.item_categories(item_idx, cat, n_items)).to(trainer.dev)
        corpus = trainer.item_corpus_embeddings(item_cat)
        for batch in val_it:
            trainer.evaluate_topk(batch[0], batch[1], metric, corpus, **({} if stamps is None else {"timestamps": batch[-1]}))
        if distributed and metric._n:           # every rank ranked its own held-out pairs: sum the tallies
            dist.all_reduce(metric._hits); dist.all_reduce(metric._dcg)
            metric._n *= world
        final["val_metrics"] = {k: float(v) for k, v in metric.result().items()}
        log.info(json.dumps(final["val_metrics"]))
    if args.save:
        path = f"{args.save}.rank{rank}of{world}" if distributed else args.save
        ck = trainer.state_dict()
        ck.update(epoch=last_epoch if history else first_epoch, early_stopping=stopper.state_dict())
        torch.save(ck, path)
        log.info("saved checkpoint to %s", path)
    if rank == 0:
        print(json.dumps(final))
    if distributed:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
