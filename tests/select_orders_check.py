"""Designed arrival orders for the four copies of the retrieval selection scheme (topk::Select in csrc/topk_select.h under
topk_select_kernel; topk::select_run_ids under ivf_select_kernel; i8_scan_kernel in csrc/topk_i8.hip; ivf_i8_select_kernel in
csrc/ivf_i8.hip), shared by test_select_orders_cpu.py and test_gpu_select_orders.py: the scenario builder, the corner asserts and
the NumPy reference.

SCORES ARE EXACT BY CONSTRUCTION.  A scenario holds a few integer PATTERNS T[p][j] (pattern p, arrival position j, |T| <= 16000).
Candidate row j carries pattern p as two base-127 digits in coordinates (2p, 2p + 1): hi = T // 127 in [-127, 127] and
lo = T % 127 in [0, 126], both int8 codes, times the row's power-of-two scale 2^sexp[j].  Query row r picks ONE pattern and a
sign s in {+1, -1, 0}: coordinates (2p, 2p + 1) = (127 s, s), so its score against row j is s * T[p][j] * 2^sexp[j].  Every query
also holds 1 at coordinate D - 2 (where only the IVF centroids are non-zero: centroid l holds nlist - l there, so the probed lists
are lists 0 .. nprobe - 1) and 127 at coordinate D - 1 (where every candidate and centroid is zero), which makes the int8 query
quantiser return the integers themselves with scale 1.  Every product and every partial sum is then (an integer below 2^24) times
a power of two: the f32 MFMA chain, whatever its order, and the int32 dot product are both exact, key * qscale is exact, and the
expected answer needs no GPU and no tolerance.  ``Scenario.check_exact`` asserts the bound for every scenario.

THE REFERENCE (``expected``) is scheme-independent: per query the f64 scores, minus the excluded and the unprobed candidates,
``np.lexsort((ids, -score))[:k]``, tail (-inf, -1); for the int8 entry points both stages (the k1 best by key, then - with c - the k
best of those by the exact score).  ``expected_py`` restates it with plain Python ``sorted`` from the patterns themselves (not from
the encoded arrays), so the two also check the encoding.

THE CORNER ASSERTS (``Scenario.check_corners``) prove from the data alone that the arrival pattern a scenario is named after is
really in it.  They use ``simulate``, a small model of ONE wave of the scheme: a candidate survives against the k-th best as of the
last flush, and every non-empty queue is merged when some row of the 32-row block holds more than K_QUEUE - TILE survivors.  The
model serves these asserts only, never the expected output.  Its constants mirror the sources; test_select_orders_cpu.py reads them
back out of the .hip / .h files and fails when they drift."""
import functools

import numpy as np

# ---- mirrored constants (checked against the sources by test_select_orders_cpu.py)
TILE = 32                        # candidates per tile = query rows per wave (the 32x32 MFMA accumulator)
K_QUEUE = 48                     # topk::kQueue
MAX_K = 256                      # TT_TOPK_MAX_K
MERGE_FAN = 16                   # topk::kMergeFan: lists per topk_merge_kernel workgroup
TARGET_WAVES = 2048              # kTargetWaves of topk.hip, topk_i8.hip and ivf.hip
MAX_SPLITS = 4096                # kMaxSplits
MIN_COLS_F32 = 512               # kMinColsPerSplit of topk.hip
MIN_COLS_I8 = 2048               # kMinColsPerSplit of topk_i8.hip
I8_RING = 4                      # i8::kRing: tile buffers of the int8 scans
IVF_MIN_ROWS_PER_CHUNK = 64      # kMinRowsPerChunk of ivf.hip
IVF_MAX_CHUNKS = 64              # kMaxChunks
IVF_CHUNK_WS_CAP = 1 << 30       # kChunkWsCap

EXACT = 1 << 24                  # integers below this are exact in f32
BASE = 127                       # digit base of a pattern value
T_MAX = 16000                    # |pattern value| bound (hi digit within [-127, 127])
DECOY = 15000                    # |pattern value| of the rows of the unprobed IVF list
N_DECOY = 4

ENTRIES = ("topk", "ivf", "topk_i8", "topk_i8_c", "ivf_i8", "ivf_i8_c")       # _c: with the f32 corpus (exact re-rank)
F32_ENTRIES = ("topk", "ivf")
I8_ENTRIES = ("topk_i8", "topk_i8_c", "ivf_i8", "ivf_i8_c")
IVF_ENTRIES = ("ivf", "ivf_i8", "ivf_i8_c")


# ---------------------------------------------------------------------------------------------------- the plans, mirrored
def corpus_splits(nq, nc, min_cols):
    """(nsplit, candidates per split) of topk_plan / i8_plan."""
    rblocks = (nq + TILE - 1) // TILE
    ns = (TARGET_WAVES + rblocks - 1) // rblocks
    ns = max(1, min(ns, (nc + min_cols - 1) // min_cols, MAX_SPLITS))
    cps = ((nc + ns - 1) // ns + 31) & ~31
    return (nc + cps - 1) // cps, cps


def ivf_chunks(nq, nlist, n, list_k, nprobe):
    """S of ivf_probe_plan: chunks per list."""
    P = nq * nprobe
    est = max(min(P, nlist), (P + 31) // 32)
    S = (TARGET_WAVES + est - 1) // est
    S = min(S, (n // nlist + IVF_MIN_ROWS_PER_CHUNK - 1) // IVF_MIN_ROWS_PER_CHUNK, IVF_MAX_CHUNKS,
            IVF_CHUNK_WS_CAP // (P * list_k * 8))
    return max(S, 1)


def merge_rounds(nl):
    rounds = 0
    while True:
        nl = (nl + MERGE_FAN - 1) // MERGE_FAN
        rounds += 1
        if nl <= 1:
            return rounds


# ---------------------------------------------------------------------------------------------------- the model of one wave
def simulate(scores, ids, k, excl=None, tie_to_lower_id=True):
    """One wave of the scheme over ``scores`` [R <= 32 rows, n] in arrival order with candidate ids ``ids`` [n]: per-tile records
    surv[r, t] (survivors of tile t after the exclusions), qn[r, t] (queue length after the push, before a flush), flush[t],
    m_before[r, t] and tot[r, t] (list length before, list + queue entries at, the flush of tile t; 0 where the row was skipped),
    full[r, t] (the list was full BEFORE tile t) and the final lists.  ``tie_to_lower_id`` = False flips the id half of the
    THRESHOLD test only (the mutation the suite must notice); the merge keeps the true order."""
    R, n = scores.shape
    assert R <= TILE
    nt = (n + TILE - 1) // TILE
    excl = [frozenset()] * R if excl is None else [frozenset(int(i) for i in e) for e in excl]
    lst = [[] for _ in range(R)]
    que = [[] for _ in range(R)]
    thr = [None] * R
    rec = dict(surv=np.zeros((R, nt), int), qn=np.zeros((R, nt), int), flush=np.zeros(nt, bool), m_before=np.zeros((R, nt), int),
               tot=np.zeros((R, nt), int), full=np.zeros((R, nt), bool))

    def flush(t):
        for r in range(R):
            if not que[r]:
                continue
            if t is not None:
                rec["m_before"][r, t] = len(lst[r])
                rec["tot"][r, t] = len(lst[r]) + len(que[r])
            lst[r] = sorted(lst[r] + que[r])[:k]
            que[r] = []
            if len(lst[r]) == k:
                thr[r] = lst[r][-1]

    for t in range(nt):
        for r in range(R):
            rec["full"][r, t] = thr[r] is not None
            for j in range(TILE * t, min(TILE * t + TILE, n)):
                s, i = float(scores[r, j]), int(ids[j])
                if thr[r] is not None:
                    ts, ti = -thr[r][0], thr[r][1]
                    if not (s > ts or (s == ts and (i < ti if tie_to_lower_id else i > ti))):
                        continue
                if i in excl[r]:
                    continue
                que[r].append((-s, i))
                rec["surv"][r, t] += 1
            rec["qn"][r, t] = len(que[r])
            assert len(que[r]) <= K_QUEUE, "the model's queue overflows"
        if any(len(q) > K_QUEUE - TILE for q in que):
            rec["flush"][t] = True
            flush(t)
    flush(None)
    rec["lists"] = lst
    return rec


# ---------------------------------------------------------------------------------------------------- scenarios
class Scenario:
    """name, doc; dim, k, k1 (stage-1 length of the calls with c); T int64 [npat, n] the patterns by arrival position; Tc the
    patterns of the f32 corpus (T unless the re-rank is to reorder); sexp int [n] scale exponents; rows ((pattern, sign, tag), ..)
    the queries; ids int64 [n] the original id of every position (arange: the scenario runs through the whole-corpus entry points
    too); list_lens the probed IVF lists; decoys: an unprobed IVF list of N_DECOY rows that would win follows them; excl: per
    query a tuple of excluded ids, or None; entries: the entry points that can express it; corners: names in CORNERS."""

    def __init__(self, name, doc, dim, k, T, rows, corners, sexp=None, ids=None, list_lens=None, decoys=True, excl=None,
                 entries=None, k1=None, Tc=None, single_wave=True):
        self.name, self.doc, self.dim, self.k = name, doc, dim, k
        self.T = np.atleast_2d(np.asarray(T, dtype=np.int64))
        self.Tc = self.T if Tc is None else np.atleast_2d(np.asarray(Tc, dtype=np.int64))
        self.n = self.T.shape[1]
        self.sexp = np.zeros(self.n, dtype=np.int64) if sexp is None else np.asarray(sexp, dtype=np.int64)
        self.rows = tuple(rows)
        self.nq = len(self.rows)
        identity = ids is None
        self.ids = np.arange(self.n, dtype=np.int64) if identity else np.asarray(ids, dtype=np.int64)
        self.list_lens = (self.n,) if list_lens is None else tuple(list_lens)
        self.decoys = decoys
        self.excl = None if excl is None else tuple(tuple(int(i) for i in e) for e in excl)
        self.k1 = k if k1 is None else k1
        self.single_wave = single_wave
        if entries is None:
            entries = ENTRIES if identity and list_lens is None else IVF_ENTRIES
        self.entries = tuple(entries)
        self.corners = tuple(corners)
        for a in (self.T, self.Tc, self.sexp, self.ids):
            a.setflags(write=False)
        assert self.Tc.shape == self.T.shape and self.sexp.shape == (self.n,) and self.ids.shape == (self.n,), name
        assert sorted(self.ids.tolist()) == list(range(self.n)), f"{name}: ids must be a permutation of 0..n-1 (distinct)"
        assert sum(self.list_lens) == self.n and 2 * self.T.shape[0] <= dim - 2, name
        assert np.abs(self.T).max() <= T_MAX and np.abs(self.Tc).max() <= T_MAX and np.abs(self.sexp).max() <= 2, name
        assert 1 <= k <= self.k1 <= min(MAX_K, self.n), name
        assert all(0 <= p < self.T.shape[0] and s in (-1, 0, 1) for p, s, _ in self.rows), name
        assert set(self.entries) <= set(ENTRIES) and self.doc and all(c in CORNERS for c in self.corners), name

    def __repr__(self):
        return f"Scenario({self.name})"

    # ---- rows by tag
    def row(self, tag):
        hit = [r for r, (_, _, t) in enumerate(self.rows) if t == tag]
        assert hit, f"{self.name}: no row tagged {tag}"
        return hit[0]

    # ---- the arrays handed to the entry points
    def queries(self):
        q = np.zeros((self.nq, self.dim), dtype=np.float32)
        for r, (p, s, _) in enumerate(self.rows):
            q[r, 2 * p], q[r, 2 * p + 1] = BASE * s, s
        q[:, self.dim - 2] = 1
        q[:, self.dim - 1] = 127
        return q

    def _digits(self, T):
        codes = np.zeros((T.shape[1], self.dim), dtype=np.int8)
        hi, lo = np.divmod(T, BASE)
        assert np.abs(hi).max() <= 127 and lo.min() >= 0, self.name
        codes[:, 0:2 * T.shape[0]:2] = hi.T
        codes[:, 1:2 * T.shape[0]:2] = lo.T
        return codes

    def codes(self):
        """int8 [n, D] by arrival position."""
        return self._digits(self.T)

    def scales(self):
        return np.exp2(self.sexp).astype(np.float32)

    def corpus(self):
        """f32 [n, D] by arrival position: the digits of Tc times the row's scale."""
        return self._digits(self.Tc).astype(np.float32) * self.scales()[:, None]

    @functools.cached_property
    def ivf(self):
        """The IVF layout: the probed lists (arrival positions in order), then - decoys - one unprobed list of N_DECOY rows with
        ids n .. n + 3 and pattern values +-DECOY, then empty lists until the average list has at most IVF_MIN_ROWS_PER_CHUNK
        rows (one chunk per list).  dict: centroids, list_offsets, list_vectors, list_codes, list_scales, list_ids, c (f32 rows in
        ORIGINAL id order), nprobe, nlist, n."""
        T, Tc, sexp, ids = self.T, self.Tc, self.sexp, self.ids
        lens = list(self.list_lens)
        if self.decoys:
            sign = np.array([1, 1, -1, -1])[:N_DECOY]
            dec = np.broadcast_to(sign * DECOY, (T.shape[0], N_DECOY))
            T, Tc = np.concatenate([T, dec], axis=1), np.concatenate([Tc, dec], axis=1)
            sexp = np.concatenate([sexp, np.zeros(N_DECOY, dtype=np.int64)])
            ids = np.concatenate([ids, self.n + np.arange(N_DECOY)])
            lens.append(N_DECOY)
        n = len(ids)
        nlist = max(len(lens), n // IVF_MIN_ROWS_PER_CHUNK + 1)
        lens += [0] * (nlist - len(lens))
        scales = np.exp2(sexp).astype(np.float32)
        vec = self._digits(Tc).astype(np.float32) * scales[:, None]
        cent = np.zeros((nlist, self.dim), dtype=np.float32)
        cent[:, self.dim - 2] = nlist - np.arange(nlist)
        c = np.zeros_like(vec)
        c[ids] = vec
        out = dict(centroids=cent, list_offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), list_vectors=vec,
                   list_codes=self._digits(T), list_scales=scales, list_ids=ids.astype(np.int32), c=c,
                   nprobe=len(self.list_lens), nlist=nlist, n=n)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return out

    def c_original(self):
        """f32 [n, D] in ORIGINAL id order (what the whole-corpus entry points take as c: there the id is the position)."""
        assert (self.ids == np.arange(self.n)).all(), self.name
        return self.corpus()

    # ---- exactness
    def check_exact(self):
        """Every |q| . |integer digits| sum is below 2^24, every operand is an integer times a power of two, and the query is its
        own int8 code row with scale 1."""
        q = self.queries()
        assert (q == np.rint(q)).all() and (np.abs(q).max(axis=1) == 127).all() and np.abs(q).max() <= 127, self.name
        L = self.ivf
        for codes in (self.codes(), self._digits(self.Tc), L["list_codes"]):
            bound = np.abs(q).astype(np.int64) @ np.abs(codes.astype(np.int64)).T
            assert bound.max() < EXACT, f"{self.name}: |q| . |codes| reaches {bound.max()}"
        for vec, scales in ((self.corpus(), self.scales()), (L["list_vectors"], L["list_scales"]), (L["centroids"], None)):
            ints = vec if scales is None else vec / scales[:, None]
            assert (ints == np.rint(ints)).all(), f"{self.name}: a corpus value is no integer times its row's scale"
            assert (np.abs(q).astype(np.float64) @ np.abs(ints).astype(np.float64).T).max() < EXACT, self.name
        for s in (self.scales(), L["list_scales"]):
            m, _ = np.frexp(s)
            assert (m == 0.5).all(), f"{self.name}: scales must be powers of two"
        assert (L["c"][L["list_ids"]] == L["list_vectors"]).all(), self.name

    # ---- the model's view: one wave per 32-row block over the whole arrival order
    def wave_scores(self):
        """f64 [nq, n]: s * T[p][j] * 2^sexp[j], the score of every (query, arrival position) in the int8 and - Tc is T - f32 streams."""
        out = np.zeros((self.nq, self.n))
        for r, (p, s, _) in enumerate(self.rows):
            out[r] = s * self.T[p] * np.exp2(self.sexp)
        return out

    @functools.cached_property
    def sims(self):
        sc = self.wave_scores()
        return [simulate(sc[b:b + TILE], self.ids, self.k, None if self.excl is None else self.excl[b:b + TILE])
                for b in range(0, self.nq, TILE)]

    def check_single_wave(self):
        """Every entry point that runs the scenario hands the whole arrival order of a list to ONE wave."""
        L = self.ivf
        if "topk" in self.entries:
            assert corpus_splits(self.nq, self.n, MIN_COLS_F32)[0] == 1, f"{self.name}: the f32 corpus is split"
        if "topk_i8" in self.entries:
            assert corpus_splits(self.nq, self.n, MIN_COLS_I8)[0] == 1, f"{self.name}: the int8 corpus is split"
        for kk in (self.k, self.k1):
            assert ivf_chunks(self.nq, L["nlist"], L["n"], kk, L["nprobe"]) == 1, f"{self.name}: the IVF lists are chunked"

    def check_corners(self):
        if self.single_wave:
            self.check_single_wave()
        for c in self.corners:
            assert CORNERS[c][1](self), f"{self.name}: corner '{c}' ({CORNERS[c][0]}) is not in the data"


def _tile_rows(s, t):
    return min(TILE, s.n - TILE * t)


def _after_full(s, r, pred, at_least=2):
    """pred(rec, row, t) holds on every tile before which row r's list was full, and there are at_least such tiles."""
    rec, rr = s.sims[r // TILE], r % TILE
    ts = [t for t in range(rec["flush"].size) if rec["full"][rr, t]]
    return len(ts) >= at_least and all(pred(rec, rr, t) for t in ts)


def _any_tile(s, pred, rows=None):
    for b, rec in enumerate(s.sims):
        for rr in range(rec["surv"].shape[0]):
            if rows is not None and b * TILE + rr not in rows:
                continue
            for t in range(rec["flush"].size):
                if pred(rec, rr, t):
                    return True
    return False


def _c_ascending(s):
    r = s.row("asc")
    return _after_full(s, r, lambda rec, rr, t: rec["surv"][rr, t] == _tile_rows(s, t) and
                       (rec["flush"][t] or _tile_rows(s, t) <= K_QUEUE - TILE))


def _c_fifth_slot(s):
    return _any_tile(s, lambda rec, rr, t: rec["tot"][rr, t] == s.k + TILE == MAX_K + TILE and rec["tot"][rr, t] > 4 * 64)


def _c_descending(s):
    return _after_full(s, s.row("desc"), lambda rec, rr, t: rec["surv"][rr, t] == 0 and rec["qn"][rr, t] == 0)


def _c_tied_first(s):
    r = s.row("tied")
    return (len(set(s.wave_scores()[r].tolist())) == 1 and (np.diff(s.ids) > 0).all() and
            _after_full(s, r, lambda rec, rr, t: rec["surv"][rr, t] == 0))


def _c_tied_last(s):
    r = s.row("tied")
    return (len(set(s.wave_scores()[r].tolist())) == 1 and (np.diff(s.ids) < 0).all() and
            _after_full(s, r, lambda rec, rr, t: rec["surv"][rr, t] == _tile_rows(s, t)))


def _full_then(first, qn_next, flush_first):
    def check(s):
        r = s.row("full")

        def pred(rec, rr, t):
            return (t + 1 < rec["flush"].size and rec["full"][rr, t] and          # (the queue is empty when tile t arrives)
                    (t == 0 or rec["flush"][t - 1] or rec["qn"][rr, t - 1] == 0) and
                    rec["surv"][rr, t] == first and rec["qn"][rr, t] == first and bool(rec["flush"][t]) == flush_first and
                    rec["surv"][rr, t + 1] == TILE and rec["qn"][rr, t + 1] == qn_next and rec["flush"][t + 1])
        return _any_tile(s, pred, rows={r})
    return check


def _c_divergent(s):
    for rec in s.sims:
        for t in np.flatnonzero(rec["flush"]):
            qn = rec["qn"][:, t]
            if rec["full"][:, t].all() and (qn == 0).any() and ((qn > 0) & (qn <= K_QUEUE - TILE)).any() and (qn > K_QUEUE - TILE).any():
                return True
    return False


def _c_carried(s):
    """the sawtooth row enters someone else's flush with a partly filled queue, list already full"""
    r = s.row("saw")
    return _any_tile(s, lambda rec, rr, t: rec["full"][rr, t] and rec["flush"][t] and 0 < rec["qn"][rr, t] <= K_QUEUE - TILE, rows={r})


def _c_mid_flush(s):
    return s.k % TILE != 0 and _any_tile(s, lambda rec, rr, t: rec["flush"][t] and rec["m_before"][rr, t] < s.k < rec["tot"][rr, t])


def _plateau(s):
    """(positions of the tie group at the cut, winners among them, losers among them) of the row tagged plateau."""
    r = s.row("plateau")
    sc = s.wave_scores()[r]
    order = np.lexsort((s.ids, -sc))
    cut = sc[order[s.k - 1]]
    if sc[order[s.k]] != cut:
        return None
    grp = np.flatnonzero(sc == cut)
    win = np.intersect1d(grp, order[:s.k])
    return grp, win, np.setdiff1d(grp, win)


def _c_plateau_inside(s):
    p = _plateau(s)
    return p is not None and len(p[0]) > TILE and len(p[1]) and len(p[2]) and p[2].min() == p[1].max() + 1 and \
        p[1].max() // TILE == p[2].min() // TILE and p[1].max() % TILE not in (0, TILE - 1)


def _c_plateau_across(s):
    p = _plateau(s)
    return p is not None and len(p[0]) > TILE and len(p[1]) and len(p[2]) and p[2].min() == p[1].max() + 1 and \
        p[1].max() % TILE == TILE - 1


def _c_plateau_later_wins(s):
    p = _plateau(s)
    return p is not None and len(p[0]) > TILE and len(p[1]) and len(p[2]) and p[1].max() > p[2].min() + TILE


def _ntiles(s):
    return (s.n + TILE - 1) // TILE


def _c_excl_second(s):
    r = s.row("asc")
    e = set(s.excl[r])
    return e == set(range(0, s.n, 2)) and _after_full(s, r, lambda rec, rr, t: rec["surv"][rr, t] == _tile_rows(s, t) // 2)


def _c_excl_topk(s):
    r = s.row("asc")
    sc = s.wave_scores()[r]
    return set(np.lexsort((s.ids, -sc))[:s.k].tolist()) <= set(s.excl[r]) and s.n - len(set(s.excl[r])) >= s.k


def _c_excl_few(s):
    r = s.row("asc")
    left = s.n - len(set(s.excl[r]) & set(range(s.n)))
    return 0 < left < s.k


def _lists_entering_merge(s, entry):
    if entry == "topk":
        return corpus_splits(s.nq, s.n, MIN_COLS_F32)[0]
    if entry == "topk_i8":
        return corpus_splits(s.nq, s.n, MIN_COLS_I8)[0]
    L = s.ivf
    return L["nprobe"] * ivf_chunks(s.nq, L["nlist"], L["n"], s.k, L["nprobe"])


def _c_two_rounds(s):
    return all(MERGE_FAN < _lists_entering_merge(s, e) <= MERGE_FAN ** 2 and merge_rounds(_lists_entering_merge(s, e)) == 2
               for e in s.entries if not e.endswith("_c"))


def _c_tie_first_split(s):
    r = s.row("tied")
    sc = s.wave_scores()[r]
    cps = corpus_splits(s.nq, s.n, MIN_COLS_I8 if "topk_i8" in s.entries else MIN_COLS_F32)[1]
    return len(set(sc.tolist())) == 1 and s.k <= cps and (np.lexsort((s.ids, -sc))[:s.k] < cps).all()


def _c_tie_last_list(s):
    r = s.row("tied")
    sc = s.wave_scores()[r]
    last = s.n - s.list_lens[-1]
    return len(set(sc.tolist())) == 1 and s.ivf["nprobe"] == s.ivf["nlist"] and (np.lexsort((s.ids, -sc))[:s.k] >= last).all()


def _c_decoys(s):
    """some row's best candidate overall is a row of the unprobed list"""
    L = s.ivf
    if not s.decoys or L["nprobe"] >= L["nlist"]:
        return False
    sc = s.queries().astype(np.float64) @ L["list_vectors"].astype(np.float64).T
    return (sc.argmax(axis=1) >= s.n).any()


CORNERS = {
    "ascending": ("a row whose every candidate beats the threshold once the list is full: a flush on every tile", _c_ascending),
    "fifth_entry_slot": ("a flush of m + qn = 256 + 32 entries: the fifth entry slot per lane", _c_fifth_slot),
    "descending": ("a row where nothing survives once the list is full: qn == 0, skipped by every flush", _c_descending),
    "tied_low_ids_first": ("all scores equal, ids ascending: nothing survives, by the id rule alone", _c_tied_first),
    "tied_low_ids_last": ("all scores equal, ids descending: everything survives, by the id rule alone", _c_tied_last),
    "full_16_then_48": ("list full, a tile of 16 survivors (qn == 16, no flush), then 32 more: qn == 48 == kQueue",
                        _full_then(16, K_QUEUE, False)),
    "full_17_flushes": ("list full, a tile of 17 survivors: flush; then 32 more: qn == 32", _full_then(17, TILE, True)),
    "full_15_then_47": ("list full, a tile of 15 survivors (no flush), then 32 more: qn == 47", _full_then(15, K_QUEUE - 1, False)),
    "divergent_rows": ("one flush with full lists where one row has qn == 0, one 0 < qn <= 16 and one qn > 16", _c_divergent),
    "carried_queue": ("a sawtooth row carries a partly filled queue into someone else's flush", _c_carried),
    "threshold_mid_flush": ("k % 32 != 0 and a flush takes the list from m < k past k: entries are discarded as the threshold is set",
                            _c_mid_flush),
    "k_is_1": ("k == 1", lambda s: s.k == 1),
    "k_is_max": ("k == TT_TOPK_MAX_K", lambda s: s.k == MAX_K),
    "k_is_n": ("k == number of candidates", lambda s: s.k == s.n and not s.excl),
    "plateau_cut_inside_tile": ("a tie group longer than a tile straddles the cut; last winner and first loser share a tile",
                                _c_plateau_inside),
    "plateau_cut_across_tiles": ("a tie group longer than a tile straddles the cut, which falls on a tile boundary", _c_plateau_across),
    "plateau_later_wins": ("a tie-group member arriving more than a tile after a loser of its group wins (list ids not ascending)",
                           _c_plateau_later_wins),
    "tiles_even": ("an even tile count", lambda s: _ntiles(s) % 2 == 0),
    "tiles_odd": ("an odd tile count", lambda s: _ntiles(s) % 2 == 1),
    "last_tile_one_row": ("the last tile holds exactly one row", lambda s: s.n % TILE == 1),
    "ring_mod_0": ("tile count = 0 mod the int8 ring", lambda s: _ntiles(s) % I8_RING == 0 and _ntiles(s) > I8_RING),
    "ring_mod_1": ("tile count = 1 mod the int8 ring", lambda s: _ntiles(s) % I8_RING == 1 and _ntiles(s) > I8_RING),
    "ring_mod_2": ("tile count = 2 mod the int8 ring", lambda s: _ntiles(s) % I8_RING == 2 and _ntiles(s) > I8_RING),
    "ring_mod_3": ("tile count = 3 mod the int8 ring", lambda s: _ntiles(s) % I8_RING == 3 and _ntiles(s) > I8_RING),
    "prefetch_dim": ("D <= 128: the two-buffer prefetch of the f32 streams", lambda s: s.dim in (32, 64, 128)),
    "no_prefetch_dim": ("D == 256: no prefetch in the f32 streams", lambda s: s.dim == 256),
    "row_block_of_one": ("nq == 33: the second block's lone row is an ascending row (rows_lds == 1)",
                         lambda s: s.nq == TILE + 1 and s.rows[TILE][2] == "asc" and _c_ascending_row(s, TILE)),
    "single_query": ("nq == 1", lambda s: s.nq == 1),
    "excl_every_second": ("every second candidate of the ascending row is excluded and does not count towards the queue",
                          _c_excl_second),
    "excl_final_topk": ("the ascending row's whole unrestricted top-k is excluded", _c_excl_topk),
    "excl_leaves_fewer_than_k": ("the exclusions leave fewer than k candidates: tail padding", _c_excl_few),
    "merge_two_rounds": ("more than 16 lists enter topk_merge_kernel: two rounds", _c_two_rounds),
    "tie_winners_first_split": ("all tied: every winner comes from the first corpus split", _c_tie_first_split),
    "tie_winners_last_list": ("all tied, nprobe == nlist: every winner comes from the last list", _c_tie_last_list),
    "unprobed_decoys": ("the unprobed list holds some row's best candidate", _c_decoys),
    "rerank_reorders": ("k1 > k and the f32 corpus orders the stage-1 candidates differently from their keys",
                        lambda s: s.k1 > s.k and not (s.T == s.Tc).all()),
}


def _c_ascending_row(s, r):
    return _after_full(s, r, lambda rec, rr, t: rec["surv"][rr, t] == _tile_rows(s, t))


# ---- patterns (by arrival position)
def ramp(n):
    """strictly ascending (so its negative strictly descends)"""
    return np.arange(n, dtype=np.int64) - n // 2


def wide_ramp(n):
    """ascending in short plateaus, for corpora longer than the value range"""
    return np.arange(n, dtype=np.int64) * 30000 // n - 15000


def sawtooth(n):
    """1 .. 5 new maxima per tile at scattered offsets, everything else low and descending: a few survivors per tile"""
    T = -5000 - np.arange(n, dtype=np.int64)
    for t in range((n + TILE - 1) // TILE):
        for i, o in enumerate((3, 7, 12, 20, 29)[:1 + t % 5]):
            if TILE * t + o < n:
                T[TILE * t + o] = 1000 + 8 * t + i
    return T


WAVE4 = ((0, 1, "asc"), (0, -1, "desc"), (0, 0, "tied"), (1, 1, "saw"))


def wave4(n):
    return np.stack([ramp(n), sawtooth(n)])


def full_queue(first):
    """k = 32.  Tile 0 fills the list (flush).  Tile 1: ``first`` survivors at scattered offsets, the rest below the threshold.
    Tile 2: 32 survivors.  Tile 3: 16 survivors.  Tile 4: one row, a survivor.  Pattern 1 (the neighbour row) descends strictly."""
    rng = np.random.default_rng(first)
    T = np.zeros(4 * TILE + 1, dtype=np.int64)
    T[0:32] = 1000 + rng.permutation(32)
    T[32:64] = -np.arange(32)
    T[32 + np.sort(rng.choice(32, first, replace=False))] = 2000 + np.arange(first)
    T[64:96] = 3000 + rng.permutation(32)
    T[96:128] = -100 - np.arange(32)
    T[96 + np.sort(rng.choice(32, 16, replace=False))] = 4000 + np.arange(16)
    T[128] = 5000
    return np.stack([T, -ramp(len(T))])


def plateau(h1, n=300):
    """h1 high values, a plateau of 100 (value 8 written as 8 x 1, 4 x 2 and 16 x 0.5), 90 low values, 30 - h1 more high values,
    a second stretch of the plateau, low values: the cut at k = 50 keeps 30 high values and the plateau's first 20 arrivals
    (positions h1 .. h1 + 19).  Returns (T, sexp)."""
    T = -100 - np.arange(n, dtype=np.int64)
    sexp = np.zeros(n, dtype=np.int64)
    T[:h1] = 200 + np.arange(h1)
    for lo, hi in ((h1, h1 + 100), (220, 260)):
        j = np.arange(lo, hi)
        sexp[j] = (j % 3) - 1                       # scales 0.5, 1, 2
        T[j] = np.where(sexp[j] == -1, 16, np.where(sexp[j] == 0, 8, 4))
    T[200:200 + 30 - h1] = 300 + np.arange(30 - h1)
    return T[None, :], sexp


def descending_ids(n):
    return np.arange(n, dtype=np.int64)[::-1].copy()


@functools.lru_cache(maxsize=None)
def scenarios():
    """Every scenario, in a fixed order; each passes its exactness bound and corner asserts when built."""
    S = []

    def add(*a, **kw):
        S.append(Scenario(*a, **kw))

    add("ascending_kmax", "one ascending row at k = 256: every tile flushes and replaces 32 entries of a full list (m + qn = 288)",
        32, MAX_K, ramp(512), [(0, 1, "asc")],
        ["ascending", "fifth_entry_slot", "k_is_max", "single_query", "tiles_even", "ring_mod_0", "unprobed_decoys"])
    add("descending", "one descending row at k = 100: nothing survives after the first k; m goes 96 -> 100 in one flush",
        128, 100, ramp(512), [(0, -1, "desc")], ["descending", "threshold_mid_flush", "single_query", "unprobed_decoys"])
    add("tied_ids_ascending", "all scores equal, ids ascending: the first k arrivals win by the id rule alone",
        32, 100, wave4(300), [(0, 0, "tied"), (0, 1, "asc")], ["tied_low_ids_first", "threshold_mid_flush", "ascending"])
    add("tied_ids_descending", "all scores equal, list ids descending: every arrival displaces the threshold by the id rule alone",
        32, 100, wave4(300), WAVE4, ["tied_low_ids_last", "threshold_mid_flush"], ids=descending_ids(300))
    for first, corner in ((16, "full_16_then_48"), (17, "full_17_flushes"), (15, "full_15_then_47")):
        add(f"full_queue_{first}", f"a full list, then a tile with exactly {first} survivors, then one with 32 ({CORNERS[corner][0]})",
            64, 32, full_queue(first), [(0, 1, "full"), (1, 1, "desc")], [corner, "descending", "last_tile_one_row", "ring_mod_1"])
    add("divergent_wave", "32 rows in one wave: ascending (flushes every tile), descending (skipped), tied, sawtooth (carried queues)",
        32, 40, wave4(417), WAVE4 * 8,
        ["divergent_rows", "carried_queue", "ascending", "descending", "tied_low_ids_first", "threshold_mid_flush", "last_tile_one_row",
         "ring_mod_2"])
    add("k_is_1", "k = 1: the list is one entry, full after the first tile", 32, 1, wave4(200), WAVE4, ["k_is_1", "ascending", "descending"])
    add("k_is_n", "k equals the number of candidates: the list fills on the very last row", 128, 77, wave4(77), WAVE4, ["k_is_n", "tiles_odd"])
    for h1, corner in ((10, "plateau_cut_inside_tile"), (12, "plateau_cut_across_tiles")):
        T, sexp = plateau(h1)
        add(corner.replace("cut_", ""), f"{CORNERS[corner][0]}; high values arriving later push plateau members out again",
            32, 50, T, [(0, 1, "plateau"), (0, -1, "plain"), (0, 0, "tied")], [corner, "threshold_mid_flush"], sexp=sexp)
    T, sexp = plateau(10)
    add("plateau_ids_shuffled", "the plateau with shuffled list ids: tied members with lower ids arrive long after the list is full",
        32, 50, T, [(0, 1, "plateau"), (0, -1, "plain"), (0, 0, "tied")], ["plateau_later_wins"], sexp=sexp,
        ids=np.random.default_rng(11).permutation(300))
    one = "last_tile_one_row"
    for n, dim, extra in ((256, 32, ["tiles_even", "ring_mod_0", "prefetch_dim"]),
                          (129, 128, ["tiles_odd", "ring_mod_1", "prefetch_dim", one]),
                          (161, 32, ["tiles_even", "ring_mod_2", "prefetch_dim", one]),
                          (193, 128, ["tiles_odd", "ring_mod_3", "prefetch_dim", one]),
                          (161, 256, ["tiles_even", "ring_mod_2", "no_prefetch_dim", one]),
                          (193, 64, ["tiles_odd", "ring_mod_3", "prefetch_dim", one]),
                          (160, 128, ["tiles_odd", "ring_mod_1", "prefetch_dim"])):
        add(f"tiles_n{n}_d{dim}", f"{(n + 31) // 32} tiles at D = {dim}, the last of {(n - 1) % 32 + 1} row(s): the arms of the f32 prefetch, "
            "the phases of the int8 ring", dim, 40, wave4(n), WAVE4, extra + ["ascending", "carried_queue"])
    add("row_blocks_33", "33 queries: a full block of mixed rows, then a block whose lone row ascends (the IVF searches cut the blocks "
        "by arrival in the bucket instead)",
        32, 40, wave4(200), WAVE4 * 8 + ((0, 1, "asc"),), ["row_block_of_one", "divergent_rows"])
    n = 300
    asc_top = list(range(n - 40, n))
    add("excl_every_second", "the ascending row without every second candidate: 16 survivors per tile, so it flushes every second tile",
        32, 40, wave4(n), WAVE4[:2], ["excl_every_second", "descending"], excl=[range(0, n, 2), [n // 2, n // 2 - 1, 10 ** 6, -3]])
    add("excl_final_topk", "the ascending row without its whole final top-k (and the descending row without its first arrivals)",
        32, 40, wave4(n), WAVE4[:2], ["excl_final_topk"], excl=[asc_top + [5, 6], range(0, 50)])
    add("excl_all_but_few", "the ascending row keeps 7 candidates: tail padding; the tied row keeps all",
        32, 40, wave4(n), (WAVE4[0], WAVE4[2]), ["excl_leaves_fewer_than_k"], excl=[[j for j in range(n) if j % 43 != 1], []])
    Tm = np.stack([wide_ramp(8704), np.full(8704, 5, dtype=np.int64)])
    Tm[1, 300 * np.arange(25) + 17] = 100 + np.arange(25)
    rows_m = [(0, 0, "tied"), (1, 1, "plateau"), (0, 1, "asc"), (0, -1, "desc")]
    add("merge_topk_17_splits", "17 corpus splits of 512 enter two merge rounds: all tied (winners all from split 0), a corpus-wide "
        "plateau under 25 scattered high values",
        32, 40, Tm, rows_m, ["merge_two_rounds", "tie_winners_first_split"], entries=("topk",), single_wave=False)
    Tm8 = np.stack([wide_ramp(34816), np.full(34816, 5, dtype=np.int64)])
    Tm8[1, 1200 * np.arange(25) + 17] = 100 + np.arange(25)
    add("merge_topk_i8_17_splits", "the same through the int8 scan: 17 splits of 2048",
        32, 40, Tm8, rows_m, ["merge_two_rounds", "tie_winners_first_split"], entries=("topk_i8", "topk_i8_c"), single_wave=False)
    Tl = np.stack([ramp(680), np.full(680, 5, dtype=np.int64)])
    Tl[1, 27 * np.arange(25) + 3] = 100 + np.arange(25)
    add("merge_ivf_17_lists", "17 probed lists of 40 (nprobe == nlist) enter two merge rounds; ids descend, so a tie's winners all come "
        "from the last list",
        32, 40, Tl, rows_m, ["merge_two_rounds", "tie_winners_last_list"], ids=descending_ids(680), list_lens=[40] * 17, decoys=False,
        single_wave=False)
    add("rerank_reorders", "k1 = 64 > k = 10 with an f32 corpus that reverses the key order: stage 2 picks the stage-1 tail",
        32, 10, wave4(300), WAVE4, ["rerank_reorders"], k1=64, Tc=-wave4(300), entries=("topk_i8_c", "ivf_i8_c"))
    names = [s.name for s in S]
    assert len(set(names)) == len(names)
    return tuple(S)


def cases():
    """(scenario, entry) for every entry point that can express the scenario."""
    return [(s, e) for s in scenarios() for e in s.entries]


# ---------------------------------------------------------------------------------------------------- the reference
def _entry_arrays(s, entry):
    """(q f64, rows f64 [N, D], codes, scales, ids int64 [N], probed bool [nq, N], k1)."""
    q = s.queries().astype(np.float64)
    if entry in IVF_ENTRIES:
        L = s.ivf
        cs = q @ L["centroids"].astype(np.float64).T
        lists = np.repeat(np.arange(L["nlist"]), np.diff(L["list_offsets"]))
        probed = np.zeros((s.nq, L["n"]), dtype=bool)
        for r in range(s.nq):
            probed[r] = np.isin(lists, np.lexsort((np.arange(L["nlist"]), -cs[r]))[:L["nprobe"]])
        return q, L["list_vectors"].astype(np.float64), L["list_codes"], L["list_scales"], L["list_ids"].astype(np.int64), probed
    return q, s.c_original().astype(np.float64), s.codes(), s.scales(), np.arange(s.n, dtype=np.int64), np.ones((s.nq, s.n), dtype=bool)


def _best(score, ids, cand, k):
    return cand[np.lexsort((ids[cand], -score[cand]))[:k]]


@functools.lru_cache(maxsize=None)
def expected(s, entry):
    """(scores f32 [nq, k], ids int64 [nq, k]) of ``entry`` on scenario ``s``; read-only, computed once."""
    q, rows, codes, scales, ids, probed = _entry_arrays(s, entry)
    exact = q @ rows.T
    key = (q @ codes.astype(np.float64).T) * scales.astype(np.float64)[None, :]
    S = np.full((s.nq, s.k), -np.inf, dtype=np.float32)
    I = np.full((s.nq, s.k), -1, dtype=np.int64)
    for r in range(s.nq):
        allowed = probed[r].copy()
        if s.excl is not None:
            allowed &= ~np.isin(ids, np.asarray(s.excl[r], dtype=np.int64))
        cand = np.flatnonzero(allowed)
        if entry in F32_ENTRIES:
            pos, sc = _best(exact[r], ids, cand, s.k), exact[r]
        elif entry.endswith("_c"):
            pos, sc = _best(exact[r], ids, _best(key[r], ids, cand, s.k1), s.k), exact[r]
        else:
            pos, sc = _best(key[r], ids, cand, s.k), key[r]
        assert (sc[pos].astype(np.float32).astype(np.float64) == sc[pos]).all(), f"{s.name}: a score is not an f32"
        S[r, :len(pos)] = sc[pos] + 0.0                        # (an exact zero is +0, as an accumulator that starts at +0 leaves it)
        I[r, :len(pos)] = ids[pos]
    S.setflags(write=False)
    I.setflags(write=False)
    return S, I


def expected_py(s, entry):
    """The same answer from the patterns themselves with plain Python ``sorted``: lists [nq][k] of (score, id)."""
    ivf = entry in IVF_ENTRIES
    n_dec = N_DECOY if ivf and s.decoys else 0
    out = []
    for r, (p, sign, _) in enumerate(s.rows):
        ex = set() if s.excl is None else set(s.excl[r])
        cand = []
        for j in range(s.n):                                  # every probed list holds arrival positions only; decoys are unprobed
            i = int(s.ids[j])
            if i in ex:
                continue
            scale = 2.0 ** int(s.sexp[j])
            cand.append((sign * int(s.T[p, j]) * scale, sign * int(s.Tc[p, j]) * scale, i))
        assert n_dec == 0 or s.ivf["nprobe"] < s.ivf["nlist"]
        if entry in F32_ENTRIES:
            best = sorted((-e, i) for _, e, i in cand)[:s.k]
        elif entry.endswith("_c"):
            stage1 = sorted((-kk, i, e) for kk, e, i in cand)[:s.k1]
            best = sorted((-e, i) for _, i, e in stage1)[:s.k]
        else:
            best = sorted((-kk, i) for kk, _, i in cand)[:s.k]
        best = [(-a, i) for a, i in best]
        out.append(best + [(float("-inf"), -1)] * (s.k - len(best)))
    return out
