"""``python -m two_tower_amazon_recommender_amd.recommend`` — the top-k items of every requested user from a checkpoint
written by ``train.py --save``: the model is rebuilt from the checkpoint's ``config``, the whole item corpus goes through
the item tower once, and users are answered in batches by ``serving.BruteForce`` (one fused score-and-select pass over
the corpus per batch; no [users x items] score matrix) or, with ``--index ivf``, by the approximate ``serving.IVF``
(``--nlist`` k-means lists, ``--nprobe`` of them scanned per user; ``--nprobe`` = ``--nlist`` is exact), or, with
``--index int8``, by ``serving.Int8BruteForce`` (an int8 scan of the whole corpus, the best ``--rerank`` x k candidates of
every user re-scored exactly), or, with ``--index ivf-int8``, by ``serving.Int8IVF`` (the int8 scan over the ``--nprobe``
probed lists only, with the same re-rank).

    python -m two_tower_amazon_recommender_amd.recommend --checkpoint ck.pt --data interactions.parquet \\
        --all-users --exclude-seen --k 10 --out recs.parquet

Output parquet: one row per (user, rank) with columns user_idx, rank (0 = best), item_idx, score.  A user with fewer
than k unexcluded items gets fewer rows.  For a model trained with the rating head (``train.py --rating-weight``),
``--predict-ratings`` adds the column predicted_rating - the head's prediction for every returned (user, item) - and
``--rank-by rating`` re-orders each user's k retrieved items by it (retrieve, then rank; the item set is the retrieval's).

``--diversify LAMBDA`` re-ranks every user's list by Maximal Marginal Relevance (``serving.MMR`` around the chosen index):
the index is asked for ``--diversify-pool`` x k candidates and k of them are picked greedily, LAMBDA x relevance against
(1 - LAMBDA) x the largest cosine to an item already picked (1.0 = the plain top-k, 0.0 = diversity only);
``--max-per-category M`` also allows at most M items of one category per user (the category of an item's first interaction
in ``--data``).  The rank column is then the diversified order and the scores need not descend.
"""
from __future__ import annotations

import argparse
import glob
import logging
import os
import re
import sys

import numpy as np

log = logging.getLogger("recommend")
MAX_K = 256                         # TT_TOPK_MAX_K of include/twotower_hip.h
_SHARDED = re.compile(r"\.rank\d+of\d+$")


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Top-k item recommendations from a trained two-tower checkpoint (HIP kernels).")
    ap.add_argument("--checkpoint", required=True, help="a checkpoint written by train.py --save (single-GPU form)")
    ap.add_argument("--k", type=int, default=10, help=f"items per user (1..{MAX_K})")
    who = ap.add_mutually_exclusive_group(required=True)
    who.add_argument("--users-file", default=None, help="a .npy of user_idx values to recommend for")
    who.add_argument("--all-users", action="store_true", help="recommend for every user row of the model")
    ap.add_argument("--data", default=None, help="interaction parquet (user_idx / item_idx columns): needed by "
                                                 "--exclude-seen and by models trained with category buckets")
    ap.add_argument("--exclude-seen", action="store_true", help="never recommend an item the user interacted with in --data")
    ap.add_argument("--out", default="recs.parquet", help="output parquet (user_idx, rank, item_idx, score)")
    ap.add_argument("--batch-users", type=int, default=4096, help="users per top-k call (bounds peak device memory)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--index", choices=("brute", "ivf", "int8", "ivf-int8"), default="brute",
                    help="brute: exact top-k over the whole corpus; ivf: approximate inverted-file index; int8: quantised "
                         "scan of the whole corpus with an exact re-rank; ivf-int8: the quantised scan over the probed lists "
                         "of an inverted-file index")
    ap.add_argument("--nlist", type=int, default=None, help="--index ivf / ivf-int8: number of k-means lists (default 1024, at most the "
                                                             "number of items)")
    ap.add_argument("--nprobe", type=int, default=None, help=f"--index ivf / ivf-int8: lists scanned per user (1..min({MAX_K}, nlist); "
                                                              "default 32)")
    ap.add_argument("--seed", type=int, default=0, help="--index ivf / ivf-int8: k-means seed")
    ap.add_argument("--rerank", type=int, default=None, help="--index int8 / ivf-int8: candidates re-scored exactly per user, as a multiple "
                                                              f"of --k (default 4; at least 32 and at most {MAX_K} candidates)")
    ap.add_argument("--predict-ratings", action="store_true",
                    help="add a predicted_rating column: the rating head's prediction for every returned (user, item); needs a "
                         "checkpoint trained with --rating-weight")
    ap.add_argument("--rank-by", choices=("score", "rating"), default="score",
                    help="score: the retrieval order (default); rating: each user's k retrieved items re-ordered by the "
                         "predicted rating, best first (implies --predict-ratings)")
    ap.add_argument("--at-time", default=None, metavar="SECONDS|YYYY-MM-DD",
                    help="models trained with --time-features: the time the recommendations are asked for - whole seconds since the "
                         "epoch, or a UTC date (its midnight); default: the checkpoint's time_max, the newest training timestamp")
    ap.add_argument("--diversify", type=float, default=None, metavar="LAMBDA",
                    help="re-rank every user's list by Maximal Marginal Relevance: LAMBDA in [0, 1] weighs relevance against the "
                         "cosine to the items already picked (1.0: the plain top-k; 0.0: diversity only)")
    ap.add_argument("--diversify-pool", type=int, default=None, metavar="P",
                    help=f"--diversify: candidates the index is asked for per user, as a multiple of --k (default 4; at least 32 "
                         f"and at most {MAX_K} candidates)")
    ap.add_argument("--max-per-category", type=int, default=None, metavar="M",
                    help="at most M items of one category per user (the category column of --data, an item's category being that "
                         "of its first interaction); implies --diversify 1.0 when that flag is absent")
    args = ap.parse_args(argv)
    if args.at_time is not None:
        try:
            args.at_time = parse_time(args.at_time)
        except ValueError:
            ap.error(f"--at-time must be whole seconds since the epoch or a date YYYY-MM-DD, got {args.at_time!r}")
    args.predict_ratings = args.predict_ratings or args.rank_by == "rating"
    if not 1 <= args.k <= MAX_K:
        ap.error(f"--k must be in [1, {MAX_K}], got {args.k}")
    if args.batch_users < 1:
        ap.error("--batch-users must be positive")
    if args.index not in ("ivf", "ivf-int8") and (args.nlist is not None or args.nprobe is not None):
        ap.error("--nlist / --nprobe need --index ivf or --index ivf-int8")
    if args.index not in ("int8", "ivf-int8") and args.rerank is not None:
        ap.error("--rerank needs --index int8 or --index ivf-int8")
    if args.index in ("int8", "ivf-int8"):
        args.rerank = 4 if args.rerank is None else args.rerank
        if args.rerank < 1:
            ap.error(f"--rerank must be positive, got {args.rerank}")
    if args.index in ("ivf", "ivf-int8"):
        args.nlist = 1024 if args.nlist is None else args.nlist
        args.nprobe = min(32, args.nlist) if args.nprobe is None else args.nprobe
        if args.nlist < 1:
            ap.error(f"--nlist must be positive, got {args.nlist}")
        if not 1 <= args.nprobe <= min(MAX_K, args.nlist):
            ap.error(f"--nprobe must be in [1, min({MAX_K}, --nlist {args.nlist})], got {args.nprobe}")
    if args.max_per_category is not None:
        if args.max_per_category < 1:
            ap.error(f"--max-per-category must be positive, got {args.max_per_category}")
        if args.data is None:
            ap.error("--max-per-category needs --data (the interactions that give every item its category)")
        if args.diversify is None:
            args.diversify = 1.0
    if args.diversify is not None and not 0.0 <= args.diversify <= 1.0:         # (NaN fails both comparisons)
        ap.error(f"--diversify must be in [0, 1], got {args.diversify}")
    if args.diversify_pool is not None:
        if args.diversify is None:
            ap.error("--diversify-pool needs --diversify or --max-per-category")
        if args.diversify_pool < 1:
            ap.error(f"--diversify-pool must be positive, got {args.diversify_pool}")
    elif args.diversify is not None:
        args.diversify_pool = 4
    if args.exclude_seen and args.data is None:
        ap.error("--exclude-seen needs --data (the interactions that define what each user has seen)")
    if _SHARDED.search(args.checkpoint) or (not os.path.exists(args.checkpoint)
                                            and glob.glob(glob.escape(args.checkpoint) + ".rank*of*")):
        ap.error(f"{args.checkpoint}: a per-rank checkpoint of the sharded trainer (*.rankRofW) is not supported; "
                 "recommend reads the single-GPU form written by train.py --save without --distributed")
    if not os.path.exists(args.checkpoint):
        ap.error(f"--checkpoint {args.checkpoint}: no such file")
    return args


def parse_time(text: str) -> int:
    """Whole seconds since the epoch from "SECONDS" or a UTC date "YYYY-MM-DD" (its midnight)."""
    import datetime
    try:
        return int(text)
    except ValueError:
        day = datetime.date.fromisoformat(text)
        return (day - datetime.date(1970, 1, 1)).days * 86400


def seen_csr(user_idx: np.ndarray, item_idx: np.ndarray, n_users: int):
    """(starts int64 [n_users + 1], items int64): user u's interacted items are items[starts[u]:starts[u + 1]]."""
    order = np.argsort(user_idx, kind="stable")
    items = item_idx[order].astype(np.int64, copy=False)
    starts = np.searchsorted(user_idx[order], np.arange(n_users + 1), side="left").astype(np.int64)
    return starts, items


def batch_exclusions(starts: np.ndarray, items: np.ndarray, users: np.ndarray):
    """CSR (offsets [len(users) + 1], indices) of the users' seen items, in the order of ``users``."""
    lo, hi = starts[users], starts[users + 1]
    n = hi - lo
    offsets = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum(n, out=offsets[1:])
    # position j of the result reads items[lo[user of j] + (j - offsets[user of j])]
    seg = np.repeat(np.arange(len(users)), n)
    idx = items[lo[seg] + (np.arange(offsets[-1]) - offsets[seg])] if offsets[-1] else np.zeros(0, dtype=np.int64)
    return offsets, idx


def main(argv=None) -> int:
    args = parse(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    import torch
    import pyarrow as pa
    import pyarrow.parquet as pq
    from . import data as datamod
    from .serving import IVF, MMR, BruteForce, Int8BruteForce, Int8IVF
    from .trainer import TwoTowerConfig, TwoTowerTrainer

    dev = torch.device(args.device)
    ck = torch.load(args.checkpoint, map_location=dev, weights_only=True)
    if not isinstance(ck, dict) or "config" not in ck:
        raise SystemExit(f"{args.checkpoint}: not a checkpoint written by train.py --save (no 'config')")
    cfg = TwoTowerConfig(**ck["config"])
    if args.predict_ratings and not cfg.rating_weight > 0:
        raise SystemExit(f"{args.checkpoint}: the model has no rating head (trained without --rating-weight): "
                         "--predict-ratings / --rank-by rating cannot be answered")
    if args.at_time is not None and not cfg.time_fields:
        raise SystemExit(f"{args.checkpoint}: the model has no time features (trained without --time-features): --at-time has no meaning")
    at_time = None if not cfg.time_fields else cfg.time_max if args.at_time is None else args.at_time
    cfg.dropout_rate = 0.0
    cfg.candidate_sampling, cfg.n_sampled_negatives = "in_batch", 0      # serving scores the whole corpus: nothing is sampled
    cfg.sampling_bias_estimator = "none"                                  # ... and nothing is corrected: no sketch is allocated
    trainer = TwoTowerTrainer(cfg, dev)
    trainer.load_state_dict(ck)
    del ck

    user_idx = item_idx = None
    if args.data is not None:
        user_idx, item_idx = datamod.read_interactions(args.data)
    item_cat = None
    if cfg.n_category_buckets > 0:
        if args.data is None:
            raise SystemExit("the checkpoint's model has category buckets: --data is needed to rebuild item categories")
        cv = datamod.read_category_values(args.data)
        if cv is None:
            raise SystemExit(f"{args.data} has none of the columns {datamod.CATEGORY_COLUMNS} the model's categories need")
        cat = datamod.category_buckets(cv[0], cv[1], cfg.n_category_buckets, dev)
        item_cat = torch.from_numpy(datamod.item_categories(item_idx, cat, cfg.n_items)).to(dev)

    if args.all_users:
        users = np.arange(cfg.n_users, dtype=np.int64)
    else:
        users = np.asarray(np.load(args.users_file), dtype=np.int64).reshape(-1)
        if users.size and (users.min() < 0 or users.max() >= cfg.n_users):
            raise SystemExit(f"{args.users_file}: user ids must be in [0, {cfg.n_users})")
    k = min(args.k, cfg.n_items)
    if args.index in ("ivf", "ivf-int8"):
        if args.nlist > cfg.n_items:
            raise SystemExit(f"--nlist {args.nlist} exceeds the model's {cfg.n_items} items")
        if args.index == "ivf":
            bf = IVF(k=k, nlist=args.nlist, nprobe=args.nprobe, seed=args.seed)
        else:
            bf = Int8IVF(k=k, nlist=args.nlist, nprobe=args.nprobe, seed=args.seed, rerank=args.rerank)
    elif args.index == "int8":
        bf = Int8BruteForce(k=k, rerank=args.rerank)
    else:
        bf = BruteForce(k=k)
    if args.diversify is None:
        bf.index_from_trainer(trainer, item_cat, at_time)
    else:
        item_groups = None
        if args.max_per_category is not None:
            cv = datamod.read_category_values(args.data)
            if cv is None:
                raise SystemExit(f"{args.data} has none of the columns {datamod.CATEGORY_COLUMNS} --max-per-category needs")
            item_groups = torch.from_numpy(datamod.item_category_groups(item_idx, cv[0], cfg.n_items)).to(dev)
        bf = MMR(bf, lambda_=args.diversify, pool=args.diversify_pool,
                 max_per_group=args.max_per_category or 0).index_from_trainer(trainer, item_cat, at_time, groups=item_groups)
    seen = seen_csr(user_idx, item_idx, cfg.n_users) if args.exclude_seen else None

    cols = {"user_idx": [], "rank": [], "item_idx": [], "score": []}
    group = []                          # the request position of every row's user (a user may be asked for twice)
    for s in range(0, len(users), args.batch_users):
        ub = users[s:s + args.batch_users]
        ut = torch.from_numpy(ub).to(dev)
        if seen is not None:
            off, idx = batch_exclusions(seen[0], seen[1], ub)
            scores, items = bf.query_with_exclusions(ut, (torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev)))
        else:
            scores, items = bf(ut)
        scores, items = scores.cpu().numpy(), items.cpu().numpy()
        keep = items >= 0
        cols["user_idx"].append(np.repeat(ub, k).reshape(-1, k)[keep])
        cols["rank"].append(np.tile(np.arange(k, dtype=np.int32), (len(ub), 1))[keep])
        cols["item_idx"].append(items[keep])
        cols["score"].append(scores[keep])
        group.append(np.repeat(np.arange(s, s + len(ub), dtype=np.int64), k).reshape(-1, k)[keep])
    out = {name: np.concatenate(v) if v else np.zeros(0) for name, v in cols.items()}
    if args.predict_ratings and len(out["user_idx"]):
        ui, ii = torch.from_numpy(out["user_idx"]).to(dev), torch.from_numpy(out["item_idx"].astype(np.int64)).to(dev)
        when = None if at_time is None else torch.full((len(ui),), at_time, dtype=torch.int64, device=dev)
        pred = trainer.predict_ratings(ui, ii, None if item_cat is None else item_cat[ii], timestamps=when).cpu().numpy()
        out["predicted_rating"] = pred
        if args.rank_by == "rating":    # inside every user's rows: best predicted rating first, ties in retrieval order
            grp = np.concatenate(group)
            order = np.lexsort((out["rank"], -pred.astype(np.float64), grp))
            out = {name: v[order] for name, v in out.items()}
            grp = grp[order]
            first = np.flatnonzero(np.r_[True, grp[1:] != grp[:-1]])
            out["rank"] = (np.arange(len(grp)) - np.repeat(first, np.diff(np.r_[first, len(grp)]))).astype(np.int32)
    elif args.predict_ratings:
        out["predicted_rating"] = np.zeros(0, dtype=np.float32)
    trainer.check_ids()
    table = pa.table(out)
    pq.write_table(table, args.out)
    log.info("wrote %d recommendations for %d users to %s", table.num_rows, len(users), args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
