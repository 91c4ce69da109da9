"""The designed arrival orders of select_orders_check.py without a GPU: every scenario builds, keeps its exactness bound and holds
the corners it is named after; the lexsort reference equals a plain ``sorted`` restatement; the model's constants equal the ones in
the kernel sources; and the wave model itself ends on the reference's lists, and stops doing so when the id half of its threshold
test is flipped."""
import pathlib
import re

import numpy as np
import pytest

import int8_check
import select_orders_check as so

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc"
SCENARIOS = so.scenarios()
BY_NAME = {s.name: s for s in SCENARIOS}
KERNEL_OF = {"topk": "topk", "ivf": "ivf", "topk_i8": "topk_i8", "topk_i8_c": "topk_i8", "ivf_i8": "ivf_i8", "ivf_i8_c": "ivf_i8"}
IVF_ONLY = {"tied_low_ids_last", "plateau_later_wins", "tie_winners_last_list", "unprobed_decoys"}
CORPUS_ONLY = {"tie_winners_first_split"}
I8_ONLY = {"rerank_reorders"}


@pytest.mark.parametrize("s", SCENARIOS, ids=lambda s: s.name)
def test_scenario_is_exact_and_holds_its_corners(s):
    s.check_exact()
    s.check_corners()
    assert s.nq <= 33 and s.doc


@pytest.mark.parametrize("s", SCENARIOS, ids=lambda s: s.name)
def test_queries_quantise_to_themselves(s):
    q = s.queries()
    codes, scale = int8_check.np_quantize(q)
    assert (scale == np.float32(1.0)).all(), s.name
    assert (codes.astype(np.float32) == q).all(), s.name
    # ... and the power-of-two scales rebuild the f32 corpus from the codes exactly
    if (s.T == s.Tc).all():
        assert (s.codes().astype(np.float32) * s.scales()[:, None] == s.corpus()).all(), s.name


@pytest.mark.parametrize("s,entry", so.cases(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_reference_equals_sorted_restatement(s, entry):
    S, I = so.expected(s, entry)
    py = so.expected_py(s, entry)
    assert S.shape == I.shape == (s.nq, s.k) and S.dtype == np.float32 and I.dtype == np.int64
    for r in range(s.nq):
        assert I[r].tolist() == [i for _, i in py[r]], f"{s.name} / {entry}: ids of query {r}"
        assert S[r].astype(np.float64).tolist() == [float(v) for v, _ in py[r]], f"{s.name} / {entry}: scores of query {r}"
        valid = I[r] >= 0
        assert valid[:valid.sum()].all() and np.isneginf(S[r][~valid]).all(), f"{s.name} / {entry}: padding is a suffix"


def test_every_pattern_reaches_every_copy_of_the_scheme():
    used = {c for s in SCENARIOS for c in s.corners}
    assert used == set(so.CORNERS), set(so.CORNERS) - used
    for corner in so.CORNERS:
        if corner in IVF_ONLY:
            want = {"ivf", "ivf_i8"}
        elif corner in CORPUS_ONLY:
            want = {"topk", "topk_i8"}
        elif corner in I8_ONLY:
            want = {"topk_i8", "ivf_i8"}
        else:
            want = {"topk", "ivf", "topk_i8", "ivf_i8"}
        have = {KERNEL_OF[e] for s in SCENARIOS if corner in s.corners for e in s.entries}
        assert want <= have, f"corner '{corner}' never reaches {sorted(want - have)}"
    # the int8 entry points run both finishes
    assert {"topk_i8", "topk_i8_c", "ivf_i8", "ivf_i8_c"} <= {e for _, e in so.cases()}


@pytest.mark.parametrize("s", [s for s in SCENARIOS if s.single_wave and (s.T == s.Tc).all()], ids=lambda s: s.name)
def test_wave_model_ends_on_the_reference(s):
    """The model is used for the corner asserts only; that it ends on the scheme-independent answer shows it is a faithful
    model of a correct selection."""
    entry = "topk" if "topk" in s.entries else "ivf"
    S, I = so.expected(s, entry)
    for b, rec in enumerate(s.sims):
        for rr, lst in enumerate(rec["lists"]):
            r = b * so.TILE + rr
            assert [i for _, i in lst] == I[r][I[r] >= 0].tolist(), f"{s.name}: query {r}"
            assert [-v for v, _ in lst] == S[r][I[r] >= 0].astype(np.float64).tolist(), f"{s.name}: query {r}"


@pytest.mark.parametrize("name", ["tied_ids_descending", "plateau_ids_shuffled"])
def test_flipped_id_rule_at_the_threshold_changes_the_answer(name):
    """With list ids that do not ascend, a candidate that ties the threshold and has the lower id arrives later: a threshold
    test that sends ties to the HIGHER id drops it, and no later merge can bring it back."""
    s = BY_NAME[name]
    sc = s.wave_scores()
    good = so.simulate(sc, s.ids, s.k)["lists"]
    bad = so.simulate(sc, s.ids, s.k, tie_to_lower_id=False)["lists"]
    assert good != bad, name
    # with ascending ids (the whole-corpus kernels) the flipped test admits more but rejects nothing it should keep
    t = BY_NAME["tied_ids_ascending"]
    assert so.simulate(t.wave_scores(), t.ids, t.k)["lists"] == so.simulate(t.wave_scores(), t.ids, t.k, tie_to_lower_id=False)["lists"]


def test_a_later_trigger_would_overflow_the_queue():
    """kQueue - 31 instead of kQueue - 32: the row with 17 survivors is not flushed and the next tile's 32 make 49 > kQueue."""
    s = BY_NAME["full_queue_17"]
    rec, rr = s.sims[0], s.row("full")
    t = int(np.flatnonzero((rec["surv"][rr] == 17) & rec["full"][rr])[0])
    assert rec["qn"][rr, t] == 17 and rec["surv"][rr, t + 1] == so.TILE and 17 + so.TILE > so.K_QUEUE
    s = BY_NAME["full_queue_16"]
    rec, rr = s.sims[0], s.row("full")
    assert rec["qn"][rr].max() == so.K_QUEUE


def _const(path, name):
    text = path.read_text()
    m = re.findall(rf"constexpr\s+(?:int|int64_t)\s+{name}\s*=\s*([^;]+);", text)
    assert len(m) == 1, f"{path.name}: {name} defined {len(m)} times"
    expr = m[0].replace("int64_t(1)", "1").strip()
    assert re.fullmatch(r"[0-9 <()]+", expr), f"{path.name}: {name} = {expr}"
    return eval(expr)                                    # digits, blanks, parentheses and shifts only


def test_model_constants_equal_the_sources():
    sel, topk, i8, ivf, ivf_i8 = (CSRC / n for n in ("topk_select.h", "topk.hip", "topk_i8.hip", "ivf.hip", "ivf_i8.hip"))
    assert _const(sel, "kQueue") == so.K_QUEUE
    assert _const(sel, "kMergeFan") == so.MERGE_FAN
    assert _const(CSRC / "quant_i8.h", "kRing") == so.I8_RING
    assert _const(topk, "kMinColsPerSplit") == so.MIN_COLS_F32 and _const(i8, "kMinColsPerSplit") == so.MIN_COLS_I8
    for f in (topk, i8, ivf):
        assert _const(f, "kTargetWaves") == so.TARGET_WAVES, f.name
    for f in (topk, i8):
        assert _const(f, "kMaxSplits") == so.MAX_SPLITS, f.name
    assert _const(ivf, "kMinRowsPerChunk") == so.IVF_MIN_ROWS_PER_CHUNK and _const(ivf, "kMaxChunks") == so.IVF_MAX_CHUNKS
    assert _const(ivf, "kChunkWsCap") == so.IVF_CHUNK_WS_CAP
    m = re.findall(r"#define\s+TT_TOPK_MAX_K\s+(\d+)", (ROOT / "include" / "twotower_hip.h").read_text())
    assert [int(v) for v in m] == [so.MAX_K]
    # the four copies of the overflow trigger and of the 32-row tile
    trig = {f.name: re.findall(r"__ballot\(qn > kQueue - (\d+)\)", f.read_text()) for f in (sel, i8, ivf_i8)}
    assert trig == {"topk_select.h": [str(so.TILE)] * 2, "topk_i8.hip": [str(so.TILE)], "ivf_i8.hip": [str(so.TILE)]}, trig
    tiles = {f.name: len(re.findall(r"ntiles = __builtin_amdgcn_readfirstlane\(\(int\)\(\(c_end - c_begin \+ 31\) >> 5\)\)", f.read_text()))
             for f in (sel, i8, ivf_i8)}
    assert tiles == {"topk_select.h": 2, "topk_i8.hip": 1, "ivf_i8.hip": 1}, tiles
    # the split and chunk rules the mirrors restate
    assert re.search(r"by_rows = \(n / nlist \+ kMinRowsPerChunk - 1\) / kMinRowsPerChunk", ivf.read_text())
    for f in (topk, i8):
        assert re.search(r"cps = \(cps \+ 31\) & ~\(int64_t\)31", f.read_text()), f.name


def test_plan_mirrors():
    assert so.corpus_splits(32, 512, so.MIN_COLS_F32) == (1, 512) and so.corpus_splits(33, 513, so.MIN_COLS_F32)[0] == 2
    assert so.corpus_splits(4, 8704, so.MIN_COLS_F32) == (17, 512) and so.corpus_splits(4, 34816, so.MIN_COLS_I8) == (17, 2048)
    assert so.ivf_chunks(1, 1, 512, 40, 1) == 8 and so.ivf_chunks(1, 9, 516, 40, 1) == 1
    assert [so.merge_rounds(n) for n in (1, 16, 17, 256, 257)] == [1, 1, 2, 2, 3]
