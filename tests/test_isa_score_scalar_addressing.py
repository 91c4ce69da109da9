"""ISA guard: the plain train step's two scorer kernels keep loop-invariant addressing off the vector ALU (CPU only).

Helper: tests/isa_audit/audit_score_valu.py (the counting rule of tests/test_isa_score_valu.py: one trip of the barrier loop with
the most MFMAs; `v_mfma*` = MFMA, `v_accvgpr*` not counted, `v_exp* / v_log* / v_rcp*` = transcendental, every other `v_*` =
plain VALU).  The exact-f32 scorer measured no MFMA / VALU co-execution, so whatever a trip issues on the
vector ALU beside its arithmetic on live values is time added to the MFMAs.  Before this test the main loops of

    score_kernel<128, 7, false, false, 8, 0>   pass 2, two tile steps per trip:  169 plain VALU, 130 of them live arithmetic
    score_kernel<128, 6, false, false, 4, 0>   pass 1, one tile step per trip:   153 plain VALU, 133 of them live arithmetic

spent the rest - 39 and 20 - on values that are wave-uniform or compile-time constants: 64-bit vector induction pointers for the
per-tile bases (`v_lshl_add_u64`, `v_add_co` / `v_addc` pairs, `v_mov_b64`), 64-bit vector compares for the positive-tile test,
the other half-row's lane address rebuilt on every tile, per-tile LDS ring adds, and (pass 2) the per-tile staging of the row terms
`a_c` / `s_c`, two global loads and an exec-masked LDS write per tile.  The bounds:

    pass 2 fast, dim 128:  at most 138 plain VALU per trip  (the 130 of live arithmetic + 8)
    pass 1 fast, dim 128:  at most 137 plain VALU per trip  (the 133 of live arithmetic + 4)

MFMAs (128) and transcendentals (32 / 17) unchanged, no scratch, no more registers than the general kernels (182 / 218), no 64-bit
vector address arithmetic left in either main loop, every global load of both main loops in the `saddr` form (a 32-bit VGPR offset
beside an SGPR-pair base), and both tile loops of pass 2 with at least 4 global loads fewer per two-tile trip than the 40 they had
(the row terms come from the workgroup's LDS array).  The general kernels' pinned counts are tests/test_isa_score_valu.py's.
"""
import importlib.util
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc"
AUDIT = ROOT / "tests" / "isa_audit"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

FAST_P1, FAST_P2 = "score_kernel<128, 6, false, false, 4, 0>", "score_kernel<128, 7, false, false, 8, 0>"
PER_TILE_P2 = "score_kernel<128, 8, false, false, 8, 0>"       # pass 2 for splits longer than the LDS row-term array
MAX_VALU = {FAST_P2: 130 + 8, FAST_P1: 133 + 4}
MFMA = {FAST_P2: 128, FAST_P1: 128}
TRANS = {FAST_P2: 32, FAST_P1: 17}
MAX_VGPRS = {FAST_P2: 182, FAST_P1: 218}
P2_LOADS_BEFORE = 40
VECTOR_ADDRESS_OPS = ("v_lshl_add_u64", "v_add_co_u32", "v_addc_co_u32", "v_mov_b64", "v_lshlrev_b64",
                      "v_cmp_gt_u64", "v_cmp_lt_i64", "v_cmp_gt_i64")


def _audit():
    spec = importlib.util.spec_from_file_location("audit_score_valu", AUDIT / "audit_score_valu.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def scorer(tmp_path_factory):
    """(audit module, {kernel: body lines}, {kernel: counts}, {kernel: (vgprs, scratch)}) of one build of score.hip."""
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_score_scalar") / "score.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(CSRC / "score.hip")], check=True, capture_output=True, timeout=900)
    audit = _audit()
    lines = open(out).read().split("\n")
    found = list(audit._L.kernels(lines, "score_kernel"))
    bodies = dict(zip(audit._L.demangle([n for n, _ in found]), (b for _, b in found)))
    rep = {name: audit.audit(body) for name, body in bodies.items() if name in (FAST_P1, FAST_P2, PER_TILE_P2)}
    for name, r in rep.items():
        audit.show(name, r)
    res, cur = {}, {}
    for line in lines:
        m = re.match(r"\s+\.(name|private_segment_fixed_size|vgpr_count):\s+(\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "vgpr_count":
            res[cur["name"]] = (int(cur["vgpr_count"]), int(cur["private_segment_fixed_size"]))
            cur = {}
    names = list(res)
    return audit, bodies, rep, dict(zip(audit._L.demangle(names), (res[n] for n in names)))


def _main_span(audit, body):
    """Line numbers of the main loop: the barrier loop with the fewest plain VALU among those with the most MFMAs."""
    spans = audit.barrier_loops(body)
    counts = [audit.classify(body, s) for s in spans]
    top = max(c["mfma"] for c in counts)
    return min((s for s, c in zip(spans, counts) if c["mfma"] == top), key=lambda s: audit.classify(body, s)["valu"])


def test_main_loops_hold_the_live_arithmetic_and_little_else(scorer):
    _, _, rep, _ = scorer
    for name, cap in MAX_VALU.items():
        loops, main = rep[name]["loops"], rep[name]["main"]
        assert len(loops) == 2, (name, len(loops))                       # the main loop and the tail loop
        print(name, {k: v for k, v in main.items() if k != "ops"})
        assert main["loads"] >= 2, (name, main)                           # the loop that was found IS one that streams K
        assert main["valu"] <= cap, (name, main["valu"], cap, main["ops"])
        assert main["mfma"] == MFMA[name] and main["trans"] == TRANS[name], (name, main["mfma"], main["trans"])


def test_no_vector_address_arithmetic_and_only_saddr_loads_in_the_main_loops(scorer):
    audit, bodies, rep, _ = scorer
    for name in (FAST_P1, FAST_P2, PER_TILE_P2):
        main = rep[name]["main"]
        left = {op: n for op, n in main["ops"].items() if op.startswith(VECTOR_ADDRESS_OPS)}
        assert not left, (name, left)
        body = bodies[name]
        loads = [t for t in (audit._L._instr(body[k]) for k in _main_span(audit, body)) if t and t.startswith("global_load")]
        assert len(loads) == main["loads"] >= 2, (name, len(loads), main["loads"])
        for t in loads:                                                    # global_load_dword v1, v2, s[4:5] offset:128
            assert re.match(r"global_load_\w+\s+v\S+,\s+v\d+,\s+s\[\d+:\d+\]", t), (name, t)


def test_pass_2_reads_its_row_terms_from_lds(scorer):
    _, _, rep, _ = scorer
    for c in rep[FAST_P2]["loops"]:                                        # main loop and tail loop, two tile steps per trip
        assert c["mfma"] == 128, c["mfma"]
        assert 2 <= c["loads"] <= P2_LOADS_BEFORE - 4, c["loads"]
    # the per-tile form still stages them beside the tile
    assert rep[PER_TILE_P2]["main"]["loads"] == P2_LOADS_BEFORE, rep[PER_TILE_P2]["main"]["loads"]


def test_no_scratch_and_no_more_registers_than_the_general_kernels(scorer):
    _, _, _, res = scorer
    for name, cap in MAX_VGPRS.items():
        print(name, res[name])
        assert res[name][1] == 0, (name, res[name])
        assert res[name][0] <= cap, (name, res[name], cap)
    assert res[PER_TILE_P2][1] == 0 and res[PER_TILE_P2][0] <= MAX_VGPRS[FAST_P2], res[PER_TILE_P2]
