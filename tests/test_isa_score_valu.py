"""ISA guard for the vector work in the scorer's tile loops (CPU only; helper: tests/isa_audit/audit_score_valu.py).

The exact-f32 scorer runs its MFMAs at the vector ALU's packed-f32 rate and measured no MFMA / VALU co-execution (DESIGN.md
section 4): every vector instruction of a tile loop is issue time on top of the MFMAs.  The plain train step (no sampling
probability, no ids, no hard negatives) therefore runs two instantiations of its own, chosen on the host in launch_score:

    score_kernel<D, 6, false, false, 4, 0>   pass 1 (loss + dq) without a column bias          (general: <D, 4, ...>), D = 64 / 128
    score_kernel<D, 7, false, false, 8, 0>   pass 2 (dc) without a row bias or row scale       (general: <D, 5, ...>)

whose MAIN tile loop runs full tiles only - no clamps, no zeroing selects, no mask on the stored dot products - and whose TAIL
loop (the last 2-4 tiles of a split) is the general step.

The rule for counting (audit_score_valu.classify), applied to one trip of a loop that holds an s_barrier and MFMAs, by the first
word of each instruction: `v_mfma*` = MFMA; `v_accvgpr*` not counted; `v_exp* / v_log* / v_rcp*` = transcendental; every other
`v_*` = plain VALU.  A trip of the pass-2 loop is TWO tile steps (128 MFMAs at dim 128), a trip of the pass-1 loop is one.

The parent's counts by this rule (its only tile loop, dim 128) are pinned below as PARENT; the general instantiations must still
show exactly these - the negative control: a green test cannot mean "the classifier counts nothing" - and the fast forms' main
loops must be below them by at least what the dead arguments cost:

    pass 2:  326 - 2 x (32 mask_S + 16 `+ a_r` + 8 packed `* s_r`) = 214 plain VALU at most
    pass 1:  192 - 16 (store_tile's row selects)                   = 176 plain VALU at most

with the transcendentals (32 and 17) and the MFMAs (128 and 128) unchanged, no scratch anywhere, and no more registers than the
general kernels use (182 and 218).
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

# what the default cfg3 step (batch 8192, dim 128, exact f32) dispatches, and the general kernels of the same passes
FAST_P1, FAST_P2 = "score_kernel<128, 6, false, false, 4, 0>", "score_kernel<128, 7, false, false, 8, 0>"
GEN_P1, GEN_P2 = "score_kernel<128, 4, false, false, 4, 0>", "score_kernel<128, 5, false, false, 8, 0>"
PARENT = {GEN_P1: dict(mfma=128, valu=192, trans=17), GEN_P2: dict(mfma=128, valu=326, trans=32)}
MAX_VALU = {FAST_P1: 192 - 16, FAST_P2: 326 - 2 * (32 + 16 + 8)}
MAX_VGPRS = {FAST_P1: 218, FAST_P2: 182}
KNOWN_SCRATCH = {"score_kernel<128, 4, true, true, 8, 1>": 44}          # (pinned in test_isa_audit.py as well)


def _audit():
    spec = importlib.util.spec_from_file_location("audit_score_valu", AUDIT / "audit_score_valu.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def scorer(tmp_path_factory):
    """(loop report, {kernel: (vgpr_count, scratch bytes per lane)}) of one build of score.hip, flags as test_isa_score_loads."""
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_score_valu") / "score.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(CSRC / "score.hip")], check=True, capture_output=True, timeout=900)
    audit = _audit()
    rep = audit.report(out)
    for name in (GEN_P1, FAST_P1, GEN_P2, FAST_P2):          # (shown with `pytest -s`; DESIGN.md's numbers come from these lines)
        if name in rep:
            audit.show(name, rep[name])
    # the kernel descriptors' metadata at the end of the listing: .name / .private_segment_fixed_size / .vgpr_count
    res, cur = {}, {}
    for line in open(out):
        m = re.match(r"\s+\.(name|private_segment_fixed_size|vgpr_count):\s+(\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "vgpr_count":
            res[cur["name"]] = (int(cur["vgpr_count"]), int(cur["private_segment_fixed_size"]))
            cur = {}
    names = list(res)
    plain = audit._L.demangle(names)
    return rep, {p: res[n] for p, n in zip(plain, names)}


def test_general_kernels_still_show_the_parents_counts(scorer):
    rep, _ = scorer
    for name, want in PARENT.items():
        assert len(rep[name]["loops"]) == 1, (name, len(rep[name]["loops"]))
        got = rep[name]["main"]
        assert {k: got[k] for k in want} == want, (name, got)
        assert got["loads"] >= 2, (name, got)


def test_fast_forms_main_loops_drop_the_dead_vector_work(scorer):
    rep, _ = scorer
    for fast, gen in ((FAST_P1, GEN_P1), (FAST_P2, GEN_P2)):
        assert fast in rep, fast
        loops, main = rep[fast]["loops"], rep[fast]["main"]
        assert len(loops) == 2, (fast, len(loops))                          # the main loop and the tail loop
        print(fast, {k: v for k, v in main.items() if k != "ops"})
        assert main["loads"] >= 2, (fast, main)                              # the loop that was found IS one that streams K
        assert main["valu"] <= MAX_VALU[fast], (fast, main["valu"], MAX_VALU[fast], main["ops"])
        assert main["trans"] == PARENT[gen]["trans"], (fast, main["trans"])
        assert main["mfma"] == PARENT[gen]["mfma"], (fast, main["mfma"])
        # the tail loop does the same matrix and transcendental work per trip
        tail = [c for c in loops if c is not main][0]
        assert tail["mfma"] == main["mfma"] and tail["trans"] == main["trans"], (fast, tail)


def test_fast_forms_exist_for_every_dim_they_are_dispatched_at(scorer):
    rep, _ = scorer
    for d in (64, 128):
        assert f"score_kernel<{d}, 6, false, false, 4, 0>" in rep, d
    for d in (32, 64, 128):
        assert f"score_kernel<{d}, 7, false, false, 8, 0>" in rep, d
    assert "score_kernel<256, 7, false, false, 4, 0>" in rep
    # pass 1 has no fast form at dim 256 (the general kernel already fills the register file; a second loop body spilled) and
    # none at dim 32 (one staged float4 per thread and tile: without the bias load the loop would hold a single global load)
    assert not any(re.match(r"score_kernel<(32|256), 6,", n) for n in rep)
    for name, r in rep.items():
        if re.match(r"score_kernel<\d+, [67],", name):
            main = r["main"]
            gen = rep[re.sub(r"(<\d+), ([67]),", lambda m: f"{m.group(1)}, {int(m.group(2)) - 2},", name)]["main"]
            assert main["mfma"] == gen["mfma"] and main["trans"] == gen["trans"], (name, main, gen)
            assert main["valu"] < gen["valu"], (name, main["valu"], gen["valu"])


def test_no_scorer_kernel_has_scratch_and_the_fast_forms_fit_the_general_kernels_registers(scorer):
    _, res = scorer
    assert len(res) >= 100, len(res)
    seen = 0
    for name, (vgprs, scratch) in res.items():
        if not name.startswith("score_kernel"):
            continue
        seen += 1
        assert scratch <= KNOWN_SCRATCH.get(name, 0), (name, scratch)
    assert seen >= 100, seen
    for name, cap in MAX_VGPRS.items():
        print(name, res[name])
        assert res[name][0] <= cap, (name, res[name], cap)
    assert res[GEN_P1][0] == 218 and res[GEN_P2][0] == 182, (res[GEN_P1], res[GEN_P2])      # the caps ARE the general kernels' counts
