"""ISA guard for the scorer's tile loop (CPU only; helper: tests/isa_audit/audit_score_loads.py).

Memory operations return in order, so a wave may wait for an older load with `s_waitcnt vmcnt(N)` and keep its N younger loads in
flight - if the compiler KNOWS that N younger loads were issued.  With one load of the loop under a condition (a lane mask or a
uniform `if`) it assumes the load was skipped and waits with `vmcnt(0)`, which drains every prefetch.  The scorer's loads are
therefore unconditional, from clamped addresses, and masked by selects where they are consumed (csrc/score.hip, "staging").

Asserted for the tile loop of EVERY score_kernel instantiation: no global / buffer load inside an exec-mask region.  For the dc pass
of the exact-f32 training entry (`<D, 5, false, false, 8, 0>`, D = 32 / 64 / 128) in addition: at least one partial wait and fewer
full waits than the parent's four.

The tree before this test, by the same rule and the same hipcc (loads in the loop / of them in an exec-mask region / vmcnt(0) /
partial waits / branches in the loop (on exec) / instructions in the loop):

    score_kernel< 32, 4, false, false, 4, 0>    3 /  3 / 3 / 0 /  39 (27) /  459
    score_kernel< 64, 4, false, false, 4, 0>    4 /  4 / 3 / 0 /  43 (30) /  544
    score_kernel<128, 4, false, false, 4, 0>    6 /  6 / 2 / 0 /  42 (30) /  641      (222 VGPRs)
    score_kernel< 32, 5, false, false, 8, 0>   38 / 38 / 6 / 0 / 109 (85) /  985
    score_kernel< 64, 5, false, false, 8, 0>   38 / 38 / 6 / 0 / 109 (85) / 1019
    score_kernel<128, 5, false, false, 8, 0>   40 / 40 / 4 / 0 / 114 (88) / 1118      (203 VGPRs)
    score_kernel<128, 0, false, false, 4, 0>    0 /  0 / 1 / 0 /  29 (23) /  422      (its staging loads sat in blocks the listing
                                                                                        does not attribute to the loop)
    all 112 instantiations: 84 with at least one load of the loop in an exec-mask region, none with a partial wait

and with it: 2 / 0 / 1 / 1, 3 / 0 / 1 / 2, 5 / 0 / 1 / 4 (218 VGPRs) for the three `<D, 4, ...>`, 38 / 0 / 0 / 22, 38 / 0 / 0 / 22 and
40 / 0 / 0 / 24 (182 VGPRs; 13 branches, 811 instructions) for the three `<D, 5, ...>`, 5 / 0 / 1 / 4 for `<128, 0, ...>`; no
instantiation has a load of the loop in an exec-mask region.  The one vmcnt(0) left in the 4-wave kernels stands in front of the
ds_write of the staged tile's youngest load, where nothing younger is in flight.
"""
import importlib.util
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc"
AUDIT = ROOT / "tests" / "isa_audit"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

TRAIN_F32 = [f"score_kernel<{d}, {mode}, false, false, {waves}, 0>" for d in (32, 64, 128) for mode, waves in ((4, 4), (5, 8))]
VALIDATION = "score_kernel<128, 0, false, false, 4, 0>"
DC_PASS = [n for n in TRAIN_F32 if ", 5, " in n]
PARENT_DC_FULL_WAITS = 4          # `s_waitcnt vmcnt(0)` in the dc-pass loop of score_kernel<128, 5, false, false, 8, 0> before this test


def _audit():
    spec = importlib.util.spec_from_file_location("audit_score_loads", AUDIT / "audit_score_loads.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _isa(out_dir, src: pathlib.Path):
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = out_dir / f"{src.stem}.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(src)], check=True, capture_output=True, timeout=900)
    return out


@pytest.fixture(scope="module")
def scorer_report(tmp_path_factory):
    audit = _audit()
    rep = audit.report(_isa(tmp_path_factory.mktemp("isa_score_loads"), CSRC / "score.hip"))
    for name in TRAIN_F32 + [VALIDATION]:                  # (shown with `pytest -s`; DESIGN.md's numbers come from these lines)
        if name in rep:
            audit.show(name, rep[name])
    return rep


def test_no_load_of_a_scorer_tile_loop_sits_in_an_exec_mask_region(scorer_report):
    rep = scorer_report
    assert len(rep) >= 100, len(rep)                       # (112-128 instantiations, by build flags)
    for name in TRAIN_F32 + [VALIDATION]:
        assert name in rep, name
        assert rep[name]["loads"] >= 2, (name, rep[name]["loads"])          # the loop that was found IS the one that streams K
        assert rep[name]["guarded"] == 0, (name, rep[name]["guarded"], rep[name]["loads"])
    # the instantiations with accidental-hit ids / hard negatives, the other modes, dim 256 and bf16x3 came out clean too
    bad = {n: (r["guarded"], r["loads"]) for n, r in rep.items() if r["guarded"]}
    assert not bad, bad
    assert all(r["loads"] >= 2 for r in rep.values()), {n: r["loads"] for n, r in rep.items() if r["loads"] < 2}


def test_dc_pass_waits_leave_the_prefetched_dot_products_in_flight(scorer_report):
    for name in DC_PASS:
        r = scorer_report[name]
        assert r["partial"] >= 1, (name, r["waits"])
        assert r["vmcnt0"] < PARENT_DC_FULL_WAITS, (name, r["waits"])
        # every wait of the loop - the consumption of tile t at the top of a step, the staged tile's ds_write behind GEMM2 - has the
        # 16 dot-product loads of a later tile behind it
        assert all(w["vmcnt"] >= 16 for w in r["waits"]), (name, r["waits"])


def test_load_audit_flags_a_guarded_load_in_a_barrier_loop(tmp_path):
    """The negative control: without it a green audit could mean 'the script finds nothing, ever'."""
    rep = _audit().report(_isa(tmp_path, AUDIT / "audit_score_loads_negative_control.hip"))
    assert len(rep) == 1
    (r,) = rep.values()
    assert r["loads"] == 1 and r["guarded"] == 1, r
    assert r["vmcnt0"] >= 1 and r["partial"] == 0, r
