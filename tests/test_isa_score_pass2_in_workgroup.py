"""ISA guard for the dc pass with the query splits inside the workgroup (CPU only; helpers: tests/isa_audit/).

`score_colfrag_kernel<128>` (csrc/score.hip, MODE_BWD_S_WG) runs the per-tile arithmetic of the dc pass's per-tile-staging fast form
(MODE_BWD_S_NR_T) on a PRIVATE LDS tile per wave: a wave's LDS operations execute in order, so its tile loop - two tile steps per
trip, the stored dot products of the two tiles in two register sets - holds no workgroup barrier; the kernel's barriers stand in
front of the in-workgroup split sum and in the loss sum of its first workgroup.  The next tile arrives as four chunks of four
float4 per lane, two chunks in flight, each written behind the quarter of GEMM2 that read its rows for the last time.  Asserted on
the built listing (the counting rule of audit_score_valu.classify; the numbers are in profiles/score_pass2_in_workgroup_isa.txt):

  * no scratch, at most 256 registers (8 waves per workgroup, one workgroup per CU: two waves per SIMD);
  * the MFMA loops: the paired loop with 128 MFMAs and 32 transcendentals per trip (two tile steps of 64 and 16); a loop for an odd
    last tile, if the compiler keeps one as a loop, with 64 and 16; no s_barrier in any of them;
  * per tile step 16 loads of the tile, 16 of the stored dot products and 2 row terms, none in an exec-mask region, every one in
    the `saddr` form (an SGPR-pair base beside a 32-bit VGPR offset);
  * no `s_waitcnt vmcnt(0)` in the loops: every wait leaves the younger chunk in flight.
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

KERNEL = "score_colfrag_kernel<128>"
LOADS_PER_STEP = 16 + 16 + 2       # the tile's four chunks, the dot-product block two tiles ahead, a_c and s_c of the next tile


def _mod(name):
    spec = importlib.util.spec_from_file_location(name, AUDIT / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mfma_loops(L, body):
    """Line-number lists (execution order) of every annotated loop of the body that holds an MFMA."""
    blocks = L._blocks(body)
    out = []
    for n, _, hdr, is_hdr in blocks:
        if not is_hdr:
            continue
        mine = [(a, b) for a, b, h, _ in blocks if h == hdr]
        idx = [k for a, b in mine if a >= n for k in range(a, b)] + [k for a, b in mine if a < n for k in range(a, b)]
        if any(re.match(r"\s+v_mfma", body[k]) for k in idx):
            out.append(idx)
    return out


def _loads_and_waits(L, body, span):
    """(global loads, those in an exec-mask region, those not in the saddr form, [vmcnt of every wait]) of one loop."""
    loads, guarded, vaddr, waits, depth = 0, 0, 0, [], 0
    for k in span:
        t = L._instr(body[k])
        if t is None:
            continue
        op = t.split()[0]
        if op == "s_and_saveexec_b64":
            depth += 1
        elif op == "s_or_b64" and re.match(r"s_or_b64\s+exec\s*,", t):
            depth = max(0, depth - 1)
        elif re.match(r"(global|buffer)_load", op):
            loads += 1
            guarded += 1 if depth > 0 else 0
            vaddr += 0 if re.match(r"global_load_\w+\s+v\S+,\s+v\d+,\s+s\[\d+:\d+\]", t) else 1
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", t)
            if m:
                waits.append(int(m.group(1)))
    return loads, guarded, vaddr, waits


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_score_colfrag") / "score.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(CSRC / "score.hip")], check=True, capture_output=True, timeout=900)
    V = _mod("audit_score_valu")
    L = V._L
    lines = open(out).read().split("\n")
    found = list(L.kernels(lines, "score_colfrag_kernel"))
    bodies = dict(zip(L.demangle([n for n, _ in found]), (b for _, b in found)))
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
    return V, L, bodies, dict(zip(L.demangle(names), (res[n] for n in names)))


def _loops(V, L, body):
    """[(span, counts, tile steps per trip)] of the MFMA loops"""
    out = []
    for span in _mfma_loops(L, body):
        c = V.classify(body, span)
        out.append((span, c, c["mfma"] // 64))
    return out


def test_no_scratch_and_two_waves_per_simd(listing):
    _, _, bodies, res = listing
    assert KERNEL in bodies and KERNEL in res, sorted(bodies)
    vgprs, scratch = res[KERNEL]
    print(KERNEL, "vgprs", vgprs, "scratch", scratch)
    assert scratch == 0, scratch
    assert vgprs <= 256, vgprs


def test_tile_loops_hold_no_barrier_and_64_mfmas_per_tile_step(listing):
    V, L, bodies, _ = listing
    body = bodies[KERNEL]
    loops = _loops(V, L, body)
    assert loops and any(steps == 2 for _, _, steps in loops), [s for _, _, s in loops]      # the paired loop
    for span, c, steps in loops:
        print({k: v for k, v in c.items() if k != "ops"})
        assert steps in (1, 2) and c["mfma"] == 64 * steps and c["trans"] == 16 * steps, (c["mfma"], c["trans"])
        assert not any(re.match(r"\s+s_barrier", body[k]) for k in span)


def test_loop_loads_are_unguarded_saddr_and_no_wait_drains_the_stream(listing):
    V, L, bodies, _ = listing
    body = bodies[KERNEL]
    for span, _, steps in _loops(V, L, body):
        loads, guarded, vaddr, waits = _loads_and_waits(L, body, span)
        print("tile steps", steps, "loads", loads, "guarded", guarded, "not saddr", vaddr, "vmcnt waits", waits)
        assert loads == LOADS_PER_STEP * steps, (steps, loads)
        assert guarded == 0 and vaddr == 0, (steps, guarded, vaddr)
        assert waits and min(waits) >= 4, (steps, waits)                  # the younger chunk's four loads stay in flight
