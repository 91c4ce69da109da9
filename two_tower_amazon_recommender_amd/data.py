"""Training-input reader: the parquet the reference's ``prepare_training_data.py:216-218`` writes
(``combined_interactions.parquet`` with int64 ``user_idx`` / ``item_idx``) or the preprocessor's
``user_id_encoded`` / ``item_id_encoded`` columns (``src/data/preprocessor.py:481-482``).
``mappings.pkl`` (``prepare_training_data.py:229-234``) is NOT read: loading a pickle executes code; the
row counts come from the id columns (max + 1), which is what the sorted-enumerate encoding guarantees."""
from __future__ import annotations

import re

import numpy as np
import torch

ID_COLUMNS = (("user_idx", "item_idx"), ("user_id_encoded", "item_id_encoded"))
# the pair's category: `category` (prepare_training_data.py:47), `main_category` / `category_encoded`
# (preprocessor.py:478-489).  It feeds the hashed category feature (BASELINE configs[4]).
CATEGORY_COLUMNS = ("category", "main_category", "category_encoded")


def read_interactions(path) -> tuple[np.ndarray, np.ndarray]:
    import pyarrow.parquet as pq
    names = pq.read_schema(path).names
    for ucol, icol in ID_COLUMNS:
        if ucol in names and icol in names:
            tbl = pq.read_table(path, columns=[ucol, icol])
            u = tbl.column(ucol).to_numpy().astype(np.int64, copy=False)
            i = tbl.column(icol).to_numpy().astype(np.int64, copy=False)
            if u.size and (u.min() < 0 or i.min() < 0):
                raise ValueError("negative ids in the interaction file")
            return u, i
    raise KeyError(f"{path}: none of the id column pairs {ID_COLUMNS} found (columns: {names})")


def read_category_values(path):
    """(codes int64 [n_rows], distinct values as str) of the first category column present, or None.
    Integer columns are taken by their decimal representation; nulls become "Unknown" (preprocessor.py:480)."""
    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.parquet as pq
    names = pq.read_schema(path).names
    for col in CATEGORY_COLUMNS:
        if col in names:
            arr = pq.read_table(path, columns=[col]).column(col).combine_chunks()
            if not pa.types.is_string(arr.type) and not pa.types.is_large_string(arr.type):
                arr = pc.cast(arr, pa.string())
            arr = pc.fill_null(arr, "Unknown")
            enc = pc.dictionary_encode(arr)
            if isinstance(enc, pa.ChunkedArray):
                enc = enc.combine_chunks()
            return enc.indices.to_numpy().astype(np.int64, copy=False), [str(v) for v in enc.dictionary.to_pylist()]
    return None


def category_buckets(codes: np.ndarray, values: list, n_buckets: int, device) -> np.ndarray:
    """Bucket of every row: the DISTINCT strings (a few dozen) are hashed on the GPU (tt_hash_bucket_u8), rows take
    their value's bucket."""
    from . import ops
    b = ops.hash_buckets(ops.strings_to_padded_bytes(values).to(device), n_buckets).cpu().numpy()
    return b[codes]


def item_categories(item_idx: np.ndarray, category_bucket: np.ndarray, n_items: int) -> np.ndarray:
    """Category bucket of every item row (int64 [n_items]): the bucket of the item's first interaction; items never seen
    get bucket 0."""
    out = np.zeros(n_items, dtype=np.int64)
    first = np.unique(item_idx, return_index=True)
    out[first[0]] = category_bucket[first[1]]
    return out


def item_category_groups(item_idx: np.ndarray, category_codes: np.ndarray, n_items: int) -> np.ndarray:
    """Group id of every item row (int32 [n_items]) for a per-category cap (``serving.MMR``): the category CODE
    (``read_category_values``) of the item's first interaction; -1 - never capped - for items never seen.  Ids outside
    [0, n_items) are ignored."""
    out = np.full(n_items, -1, dtype=np.int32)
    items, first = np.unique(item_idx, return_index=True)
    keep = (items >= 0) & (items < n_items)
    out[items[keep]] = category_codes[first[keep]]
    return out


TIMESTAMP_COLUMN = "timestamp"  # prepare_training_data.py:93-94: written as a number


def read_timestamps(path):
    """The ``timestamp`` column of the interaction file as float64 [n_rows] (nulls: -inf, the oldest), or None when the file
    has no such column."""
    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.parquet as pq
    if TIMESTAMP_COLUMN not in pq.read_schema(path).names:
        return None
    col = pq.read_table(path, columns=[TIMESTAMP_COLUMN]).column(TIMESTAMP_COLUMN).combine_chunks()
    ts = pc.fill_null(pc.cast(col, pa.float64()), float("-inf")).to_numpy(zero_copy_only=False).astype(np.float64, copy=False)
    return np.where(np.isnan(ts), -np.inf, ts)          # (pd.to_numeric(errors="coerce") leaves NaN where it could not parse)


TIME_MISSING = -2 ** 63          # a pair without a timestamp (``ops.TIME_MISSING``)


def timestamps_to_int64(ts) -> np.ndarray:
    """The float64 timestamps of ``read_timestamps`` as the int64 whole seconds the time context features take: the floor of a
    finite value, ``TIME_MISSING`` for a non-finite one (a null or unparsable entry: -inf there)."""
    ts = np.asarray(ts, dtype=np.float64)
    ok = np.isfinite(ts) & (np.abs(ts) < 2.0 ** 62)
    out = np.full(ts.shape, TIME_MISSING, dtype=np.int64)
    out[ok] = np.floor(ts[ok]).astype(np.int64)
    return out


def user_histories(user_idx: np.ndarray, item_idx: np.ndarray, n_users: int, max_items: int, timestamp=None) -> np.ndarray:
    """int32 [n_users, max_items] token matrix of ``set_user_histories``: every user's LAST ``max_items`` interactions in the
    order of ``timestamp`` (ties, or no timestamps at all: file position), oldest first, left-aligned, padded with -1.  A
    repeated item is kept as often as it occurs; a user with no pair is all -1.  Vectorised: one lexsort and a rank within
    the user's group."""
    user_idx, item_idx = np.asarray(user_idx), np.asarray(item_idx)
    if len(user_idx) != len(item_idx):
        raise ValueError("user_idx and item_idx differ in length")
    if max_items < 1:
        raise ValueError("max_items must be >= 1")
    out = np.full((n_users, max_items), -1, dtype=np.int32)
    n = len(user_idx)
    if n == 0:
        return out
    if user_idx.min() < 0 or user_idx.max() >= n_users:
        raise ValueError("user_idx outside [0, n_users)")
    if item_idx.min() < 0 or item_idx.max() >= 2 ** 31:
        raise ValueError("item_idx outside [0, 2^31): the history tokens are int32")
    pos = np.arange(n)
    if timestamp is None:
        order = np.argsort(user_idx, kind="stable")                       # by user, file position inside
    else:
        timestamp = np.asarray(timestamp)
        if len(timestamp) != n:
            raise ValueError("timestamp and user_idx differ in length")
        order = np.lexsort((pos, timestamp, user_idx))                    # by user, then timestamp, then file position
    u = user_idx[order]
    cnt = np.bincount(u, minlength=n_users)
    start = np.cumsum(cnt) - cnt                                          # first sorted position of every user's group
    rank = pos - start[u]                                                 # 0 = the user's oldest interaction
    col = rank - np.maximum(cnt[u] - max_items, 0)                        # the last max_items of them, left-aligned
    keep = col >= 0
    out[u[keep], col[keep]] = item_idx[order][keep].astype(np.int32)
    return out


RATING_COLUMN = "rating"        # prepare_training_data.py:96-98: every interaction carries its rating


def read_ratings(path):
    """The ``rating`` column of the interaction file as float64 [n_rows] (nulls: NaN), or None when the file has no such column."""
    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.parquet as pq
    if RATING_COLUMN not in pq.read_schema(path).names:
        return None
    col = pq.read_table(path, columns=[RATING_COLUMN]).column(RATING_COLUMN).combine_chunks()
    return pc.fill_null(pc.cast(col, pa.float64()), float("nan")).to_numpy(zero_copy_only=False).astype(np.float64, copy=False)


def _rating_stats(idx: np.ndarray, rating: np.ndarray, n_rows: int) -> np.ndarray:
    """f64 [n_rows, 5]: count, mean, std (ddof 1), min, max of ``rating`` per value of ``idx``, rounded to 3 decimals; NaN where
    the statistic does not exist (no rating: all but the count; one rating: the std).  One lexsort and bincounts."""
    out = np.full((n_rows, 5), np.nan)
    cnt = np.bincount(idx, minlength=n_rows)
    out[:, 0] = cnt
    has = cnt > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.bincount(idx, weights=rating, minlength=n_rows) / cnt
        dev = rating - mean[idx]
        std = np.sqrt(np.bincount(idx, weights=dev * dev, minlength=n_rows) / (cnt - 1))
    out[:, 1] = mean
    out[cnt > 1, 2] = std[cnt > 1]
    order = np.lexsort((rating, idx))                                     # by id, the ratings ascending inside
    r = rating[order]
    end = np.cumsum(cnt)
    out[has, 3] = r[(end - cnt)[has]]
    out[has, 4] = r[(end - 1)[has]]
    return np.round(out, 3)


def rating_features(user_idx, item_idx, rating, n_users: int, n_items: int) -> tuple[np.ndarray, np.ndarray]:
    """The reference's engineered rating columns (src/data/preprocessor.py create_user_features / create_item_features:
    ``groupby(id)["rating"].agg(["count", "mean", "std", "min", "max"]).round(3)``) as the numeric side features of the two
    towers: (user [n_users, 5], item [n_items, 5]) f32, columns count, mean, std, min, max.  Pass the TRAINING pairs only.  Pairs
    whose rating is not finite are left out.  An id with no rating has count 0; every entry that does not exist (its other
    columns, the std of a single rating) takes its column's mean over the entries that do - so its normalised value is 0 -
    or 0 when the column has none."""
    user_idx, item_idx, rating = np.asarray(user_idx), np.asarray(item_idx), np.asarray(rating, dtype=np.float64)
    if not (len(user_idx) == len(item_idx) == len(rating)):
        raise ValueError("user_idx, item_idx and rating differ in length")
    keep = np.isfinite(rating)
    user_idx, item_idx, rating = user_idx[keep], item_idx[keep], rating[keep]
    outs = []
    for idx, rows, name in ((user_idx, n_users, "user_idx"), (item_idx, n_items, "item_idx")):
        if len(idx) and (idx.min() < 0 or idx.max() >= rows):
            raise ValueError(f"{name} outside [0, {rows})")
        st = _rating_stats(idx.astype(np.int64), rating, rows)
        finite = np.isfinite(st)
        with np.errstate(invalid="ignore"):
            fill = np.where(finite.any(axis=0), np.where(finite, st, 0.0).sum(axis=0) / np.maximum(finite.sum(axis=0), 1), 0.0)
        outs.append(np.where(finite, st, fill[None, :]).astype(np.float32))
    return outs[0], outs[1]


TITLE_COLUMN = "title"          # prepare_training_data.py:52-62: every interaction carries its item's title
_TOKEN = re.compile(r"[a-z0-9]+")


def read_item_titles(path, item_idx: np.ndarray, n_items: int) -> list:
    """The title (str) of every item row: the ``title`` column of the item's first interaction; an item never seen, or a
    missing title, gives ""."""
    import pyarrow.parquet as pq
    names = pq.read_schema(path).names
    if TITLE_COLUMN not in names:
        raise KeyError(f"{path}: no {TITLE_COLUMN!r} column (columns: {names})")
    col = pq.read_table(path, columns=[TITLE_COLUMN]).column(TITLE_COLUMN).to_pylist()
    out = [""] * n_items
    items, first = np.unique(item_idx, return_index=True)
    for i, r in zip(items.tolist(), first.tolist()):
        v = col[r]
        out[i] = "" if v is None else str(v)
    return out


def title_token_rows(titles, max_tokens: int, width: int = 32):
    """Pure CPU: (rows uint8 [n, max_tokens, width], valid bool [n, max_tokens]).  A title is lower-cased and cut into its
    runs of [a-z0-9]; the first ``max_tokens`` tokens are kept, each one's UTF-8 bytes cut to ``width`` and zero-padded (the row
    format of ``ops.hash_buckets``).  An empty title gives no valid slot."""
    n = len(titles)
    rows = np.zeros((n, max_tokens, width), dtype=np.uint8)
    valid = np.zeros((n, max_tokens), dtype=bool)
    for i, t in enumerate(titles):
        for k, tok in enumerate(_TOKEN.findall(str(t).lower())[:max_tokens]):
            b = tok.encode("utf-8")[:width]
            rows[i, k, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            valid[i, k] = True
    return rows, valid


def title_tokens(titles, n_buckets: int, max_tokens: int, device, width: int = 32, chunk: int = 65536) -> torch.Tensor:
    """int32 [n, max_tokens] token matrix of ``set_item_titles``: every token row hashed on the GPU (``ops.hash_buckets``:
    FNV-1a-64 mod n_buckets), empty slots -1.  ``chunk`` titles are tokenised and hashed at a time."""
    from . import ops
    out = torch.full((len(titles), max_tokens), -1, dtype=torch.int32, device=device)
    for s in range(0, len(titles), chunk):
        rows, valid = title_token_rows(titles[s:s + chunk], max_tokens, width)
        h = ops.hash_buckets(torch.from_numpy(rows.reshape(-1, width)).to(device), n_buckets).view(-1, max_tokens)
        out[s:s + chunk] = torch.where(torch.from_numpy(valid).to(device), h, -1).to(torch.int32)
    return out


class BatchIterator:
    """Shuffled fixed-size batches of (user_idx, item_idx), resident on the device; the last partial batch
    of an epoch is dropped (the kernels' buffers are sized for one batch size)."""

    def __init__(self, user_idx: np.ndarray, item_idx: np.ndarray, batch_size: int, device, seed: int = 42, shuffle=True,
                 category_bucket: np.ndarray | None = None, ratings: np.ndarray | None = None, timestamps: np.ndarray | None = None):
        if len(user_idx) != len(item_idx):
            raise ValueError("user_idx and item_idx differ in length")
        if category_bucket is not None and len(category_bucket) != len(user_idx):
            raise ValueError("category_bucket and user_idx differ in length")
        self.u = torch.from_numpy(np.ascontiguousarray(user_idx)).to(device)
        self.i = torch.from_numpy(np.ascontiguousarray(item_idx)).to(device)
        # with a category column the iterator yields (user, item, category bucket) triples
        self.c = None if category_bucket is None else torch.from_numpy(np.ascontiguousarray(category_bucket)).to(device)
        # with ratings (the rating head's labels; NaN = none) every batch carries a trailing f32 [batch] entry
        if ratings is not None and len(ratings) != len(user_idx):
            raise ValueError("ratings and user_idx differ in length")
        self.r = None if ratings is None else torch.from_numpy(np.ascontiguousarray(ratings, dtype=np.float32)).to(device)
        # with timestamps (the time context features; int64 seconds, TIME_MISSING = none) an int64 [batch] entry comes LAST
        if timestamps is not None and len(timestamps) != len(user_idx):
            raise ValueError("timestamps and user_idx differ in length")
        self.t = None if timestamps is None else torch.from_numpy(np.ascontiguousarray(timestamps, dtype=np.int64)).to(device)
        self.batch_size, self.shuffle = batch_size, shuffle
        # the epoch's permutation is drawn ON THE DEVICE (r04): torch.randperm of 5.9 M indices on the host took ~0.1 s of a
        # 0.53 s epoch of 720 cfg3-sized steps - the CLI reported 11.2 M pairs/s for a step loop that runs at 14.0 M
        self.gen = torch.Generator(device=self.u.device).manual_seed(seed)
        self.n_batches = len(user_idx) // batch_size

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        n = self.u.numel()
        c, r, t = self.c, self.r, self.t
        if self.shuffle:
            perm = torch.randperm(n, generator=self.gen, device=self.u.device)
            u, i = self.u[perm], self.i[perm]
            c = None if c is None else c[perm]
            r = None if r is None else r[perm]
            t = None if t is None else t[perm]
        else:
            u, i = self.u, self.i
        b = self.batch_size
        for k in range(self.n_batches):
            sl = slice(k * b, (k + 1) * b)
            batch = (u[sl], i[sl]) if c is None else (u[sl], i[sl], c[sl])
            batch = batch if r is None else batch + (r[sl],)
            yield batch if t is None else batch + (t[sl],)
