"""Global-norm gradient clipping restated for the tests (NumPy, no GPU, no product code).

The binding definition (tf.clip_by_global_norm as Keras applies it: a dense parameter contributes its gradient tensor, an
embedding table its IndexedSlices.values - one row per looked-up occurrence, duplicates NOT merged):

    sumsq = sum over dense segments, over e, of (sum over slabs of slab[s][e])^2
          + sum over row buffers, over rows r, of f_r * |row r|^2
    norm  = sqrtf(sumsq)        scale = c / fmaxf(norm, c)        (exactly 1 when norm <= c; NaN when norm is not finite)

A row buffer is (grads [rows, dim], weight, slot_ids, mode) and f_r = weight + w(mode): "rows" 0; the bag modes count n_r = the
entries >= 0 of slot_ids[r, :] and add n_r ("sum"), 1 / n_r ("mean") or 1 ("sqrtn"), 0 for an empty bag; "mask" adds 1 where
slot_ids[r] >= 0.  A dense segment is (slabs, count, n_slabs, stride): slab s holds ``count`` floats from s * stride on.

``global_norm`` is that in f64; ``kernel_norm_f32`` restates the SUMMATION ORDER of csrc/clip.hip in f32 (per-thread sums over
the chunks a workgroup walks, the wave butterfly, the four waves through LDS, the partials in f64) for the tolerance margin;
``problem`` builds the inputs the GPU test and the margin test share."""
import numpy as np

MODES = ("rows", "sum", "mean", "sqrtn", "mask")
ROWS = (1, 3, 65, 257)
DIMS = (4, 36, 128, 260)
SLOTS = (1, 5)
DENSE = ((33, 33, 3), (37, 40, 1), (4096, 4096, 5))          # (count, stride, n_slabs)
DENSE_EXTRA = ((38, 40, 2),)                                  # 16-byte loads with a scalar tail over two slabs


def row_factors(rows: int, weight: float, slot_ids, mode: str, dtype=np.float64) -> np.ndarray:
    f = np.full(rows, weight, dtype=dtype)
    if mode == "rows":
        return f
    ids = np.asarray(slot_ids)
    if mode == "mask":
        return f + (ids.reshape(rows) >= 0).astype(dtype)
    n = (ids.reshape(rows, -1) >= 0).sum(axis=1).astype(dtype)
    w = {"sum": n, "mean": dtype(1.0) / np.maximum(n, dtype(1.0)), "sqrtn": np.ones_like(n)}[mode]
    return f + np.where(n > 0, w, dtype(0.0))


def dense_sum(slabs, count: int, n_slabs: int, stride: int, dtype=np.float64) -> np.ndarray:
    flat = np.asarray(slabs).reshape(-1)
    g = flat[:count].astype(dtype)
    for s in range(1, n_slabs):                              # slab order, starting AT slab 0 (the optimizer's order)
        g = g + flat[s * stride:s * stride + count].astype(dtype)
    return g


def sumsq(row_buffers, dense) -> float:
    tot = 0.0
    for grads, weight, slot_ids, mode in row_buffers:
        g = np.asarray(grads)
        f = row_factors(g.shape[0], weight, slot_ids, mode)
        keep = f != 0                                        # a row that does not count is not read: it may hold anything
        tot += float((f[keep] * (g[keep].astype(np.float64) ** 2).sum(axis=1)).sum())
    for slabs, count, n_slabs, stride in dense:
        tot += float((dense_sum(slabs, count, n_slabs, stride) ** 2).sum())
    return tot


def global_norm(row_buffers, dense) -> float:
    return float(np.sqrt(sumsq(row_buffers, dense)))


def scale_of(norm, c) -> np.float32:
    """The scale in f32 as defined: c / fmaxf(norm, c), NaN for a norm that is not finite."""
    norm, c = np.float32(norm), np.float32(c)
    if not np.isfinite(norm):
        return np.float32(np.nan)
    return np.float32(c / max(norm, c))


def brute_force_sumsq(row_buffers, dense) -> float:
    """Every occurrence row written out one by one: weight copies of the row as it stands, and per kept slot of a bag the row
    times the pooling's scale (sum 1, mean 1/n, sqrtn 1/sqrt(n)); a masked slot row once where it was kept."""
    tot = 0.0
    for grads, weight, slot_ids, mode in row_buffers:
        g = np.asarray(grads).astype(np.float64)
        occ = []
        for r in range(g.shape[0]):
            assert float(weight) == int(weight)
            occ += [g[r]] * int(weight)
            if mode == "mask":
                if np.asarray(slot_ids).reshape(-1)[r] >= 0:
                    occ.append(g[r])
            elif mode != "rows":
                ids = np.asarray(slot_ids).reshape(g.shape[0], -1)[r]
                n = int((ids >= 0).sum())
                inv = {"sum": 1.0, "mean": 1.0 / max(n, 1), "sqrtn": 1.0 / np.sqrt(max(n, 1))}[mode]
                occ += [inv * g[r] for j in ids if j >= 0]
        tot += sum(float(v @ v) for v in occ)
    for slabs, count, n_slabs, stride in dense:
        flat = np.asarray(slabs).reshape(-1).astype(np.float64)
        for e in range(count):
            tot += sum(flat[s * stride + e] for s in range(n_slabs)) ** 2
    return tot


# --------------------------------------------------------------------------------------- the kernel's order, in f32
THREADS, DENSE_CHUNK, ROWS_PER_GROUP, MAX_GRID = 256, 1024, 4, 1024
f32 = np.float32


def _rows_chunk(acc, grads, f, k):
    rows, dim = grads.shape
    dim4 = dim // 4
    glog2 = 0
    while (1 << glog2) < dim4 and glog2 < 6:
        glog2 += 1
    G, groups = 1 << glog2, THREADS >> glog2
    t = np.arange(THREADS)
    lane, grp = t & (G - 1), t >> glog2
    g4 = grads.reshape(rows, dim4, 4)
    for r in range(ROWS_PER_GROUP):
        row = (k * ROWS_PER_GROUP + r) * groups + grp
        live = row < rows
        rr = np.minimum(row, rows - 1)
        p = np.zeros(THREADS, dtype=f32)
        for c0 in range(0, dim4, G):
            c = lane + c0
            ok = live & (c < dim4)
            v = g4[rr, np.minimum(c, dim4 - 1)]
            for e in range(4):
                p = np.where(ok, p + v[:, e] * v[:, e], p)
        fr = f[rr]
        acc = np.where(live & (fr != 0), acc + fr * p, acc)
    return acc


def _dense_chunk(acc, slabs, count, n_slabs, stride, k):
    flat = np.asarray(slabs, dtype=f32).reshape(-1)
    t = np.arange(THREADS)
    e0 = k * DENSE_CHUNK

    def summed(e, ok):
        ee = np.where(ok, e, 0)
        g = flat[ee]
        for s in range(1, n_slabs):
            g = g + flat[s * stride + ee]
        return g
    if n_slabs == 1 or stride % 4 == 0:                       # 16-byte loads: a thread owns 4 consecutive elements
        for j in range(4):
            e = e0 + 4 * t + j
            ok = e < count
            g = summed(e, ok)
            acc = np.where(ok, acc + g * g, acc)
        return acc
    for u in range(DENSE_CHUNK // THREADS):
        e = e0 + t + u * THREADS
        ok = e < count
        g = summed(e, ok)
        acc = np.where(ok, acc + g * g, acc)
    return acc


def kernel_partials_f32(row_buffers, dense) -> np.ndarray:
    chunks = []
    for grads, weight, slot_ids, mode in row_buffers:
        g = np.ascontiguousarray(grads, dtype=f32)
        rows, dim = g.shape
        if rows == 0:
            continue
        f = row_factors(rows, weight, slot_ids, mode, dtype=f32)      # (the kernel's 1 / n is an f32 division)
        glog2 = 0
        while (1 << glog2) < dim // 4 and glog2 < 6:
            glog2 += 1
        per = (THREADS >> glog2) * ROWS_PER_GROUP
        chunks += [("rows", g, f, k) for k in range(-(-rows // per))]
    for slabs, count, n_slabs, stride in dense:
        chunks += [("dense", slabs, count, n_slabs, stride, k) for k in range(-(-count // DENSE_CHUNK))]
    grid = min(len(chunks), MAX_GRID)
    partials = np.zeros(grid, dtype=f32)
    lanes = np.arange(THREADS)
    for w in range(grid):
        acc = np.zeros(THREADS, dtype=f32)
        for ch in chunks[w::grid]:
            acc = _rows_chunk(acc, *ch[1:]) if ch[0] == "rows" else _dense_chunk(acc, *ch[1:])
        s = 1
        while s < 64:                                         # the wave butterfly: every lane ends with the wave's sum
            acc = acc + acc[lanes ^ s]
            s <<= 1
        partials[w] = ((acc[0] + acc[64]) + acc[128]) + acc[192]
    return partials


def kernel_norm_f32(row_buffers, dense) -> np.float32:
    p = kernel_partials_f32(row_buffers, dense).astype(np.float64)
    red = np.zeros(THREADS)
    for t in range(min(THREADS, len(p))):
        for v in p[t::THREADS]:
            red[t] += v
    off = THREADS // 2
    while off:
        red[:off] += red[off:2 * off]
        off >>= 1
    with np.errstate(over="ignore"):
        return np.sqrt(f32(red[0]))


# --------------------------------------------------------------------------------------- the shared inputs
def problem(rows: int, dim: int, seed: int = 0):
    """ONE call mixing every mode at L in SLOTS over [rows, dim] row buffers with the dense segments of DENSE (+ DENSE_EXTRA):
    (row_buffers, dense) as ``global_norm`` takes them.  Slot ids are -1 with probability 0.4 and row 1 (where there is one) is
    an empty bag / a skipped slot; the "rows" buffers carry the weights 1 and 2; the mask buffers hold rows * L slot rows."""
    rng = np.random.default_rng(1000003 * rows + 1009 * dim + seed)
    bufs = []
    for L in SLOTS:
        for mode in MODES:
            n = rows * L if mode == "mask" else rows
            g = (rng.standard_normal((n, dim)) * 0.05).astype(np.float32)
            ids = None
            if mode != "rows":
                shape = (n,) if mode == "mask" else (rows, L)
                ids = rng.integers(0, 50, shape).astype(np.int64)
                ids[rng.random(shape) < 0.4] = -1
                if n > 1:
                    ids[1] = -1
            weight = {"rows": float(L > 1) + 1.0, "mask": 0.0}.get(mode, float(L > 1))
            bufs.append((g, weight, ids, mode))
    dense = []
    for count, stride, n_slabs in DENSE + DENSE_EXTRA:
        slabs = (rng.standard_normal((n_slabs, stride)) * 0.02).astype(np.float32)
        dense.append((slabs, count, n_slabs, stride))
    return bufs, dense
