"""ISA audit for the scorer's tile loops: what does a trip of the loop issue besides its MFMAs?

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -S --cuda-device-only -o score.s csrc/score.hip
    python tests/isa_audit/audit_score_valu.py score.s ['<128, 7, false, false, 8, 0>' ...]

The f32-input MFMA runs at the vector ALU's packed-f32 rate and the exact-f32 scorer measured no MFMA / VALU co-execution
(DESIGN.md section 4), so every vector instruction of the tile loop is issue time on top of the MFMAs.  For every loop of a kernel
that holds an `s_barrier` and at least one MFMA (by the listing's own loop annotations, as audit_score_loads.tile_loop finds
them) the audit counts, by the first word of each instruction:

  mfma      v_mfma*
  acc       v_accvgpr*                       (moves between the two register files; not counted as VALU)
  trans     v_exp* / v_log* / v_rcp*         (the quarter-rate transcendental unit)
  valu      every other v_* instruction      ("plain VALU": compares, selects, address arithmetic, packed f32 included)
  lds       ds_*
  vmem      global_* / buffer_*              (loads and stores)
  loads     global_load* / buffer_load*
  salu      s_* except s_waitcnt / s_nop / s_barrier / branches
  lines     all instructions

A kernel whose tile loop is cut in two (the fast forms: a main loop over full tiles, a tail loop with the masking) reports both;
`main` is the barrier loop with the fewest plain VALU instructions among those with the most MFMAs.
"""
import importlib.util
import pathlib
import re
import sys

_HERE = pathlib.Path(__file__).resolve().parent


def _loads_mod():
    spec = importlib.util.spec_from_file_location("audit_score_loads", _HERE / "audit_score_loads.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_L = _loads_mod()


def barrier_loops(body):
    """Line-number lists (execution order) of every annotated loop of the kernel body that holds an s_barrier and an MFMA."""
    blocks = _L._blocks(body)
    out = []
    for n, _, hdr, is_hdr in blocks:
        if not is_hdr:
            continue
        mine = [(a, b) for a, b, h, _ in blocks if h == hdr]
        idx = [k for a, b in mine if a >= n for k in range(a, b)] + [k for a, b in mine if a < n for k in range(a, b)]
        if any(re.match(r'\s+s_barrier', body[k]) for k in idx) and any(re.match(r'\s+v_mfma', body[k]) for k in idx):
            out.append(idx)
    return out


def classify(body, span):
    rep = {'mfma': 0, 'acc': 0, 'trans': 0, 'valu': 0, 'lds': 0, 'vmem': 0, 'loads': 0, 'salu': 0, 'lines': 0, 'ops': {}}
    for k in span:
        t = _L._instr(body[k])
        if t is None:
            continue
        op = t.split()[0]
        rep['lines'] += 1
        if op.startswith('v_mfma'):
            rep['mfma'] += 1
        elif op.startswith('v_accvgpr'):
            rep['acc'] += 1
        elif re.match(r'v_(exp|log|rcp)', op):
            rep['trans'] += 1
        elif op.startswith('v_'):
            rep['valu'] += 1
            rep['ops'][op] = rep['ops'].get(op, 0) + 1
        elif op.startswith('ds_'):
            rep['lds'] += 1
        elif re.match(r'(global|buffer)_', op):
            rep['vmem'] += 1
            rep['loads'] += 1 if re.match(r'(global|buffer)_load', op) else 0
        elif op.startswith('s_') and not re.match(r's_(waitcnt|nop|barrier|cbranch|branch)', op):
            rep['salu'] += 1
    return rep


def audit(body):
    """{'main': counts, 'loops': [counts of every barrier loop]} for one kernel body; None without a barrier loop."""
    loops = [classify(body, span) for span in barrier_loops(body)]
    if not loops:
        return None
    top = max(r['mfma'] for r in loops)
    main = min((r for r in loops if r['mfma'] == top), key=lambda r: r['valu'])
    return {'main': main, 'loops': loops}


def report(path, prefix='score_kernel'):
    lines = open(path).read().split('\n')
    found = list(_L.kernels(lines, prefix))
    names = _L.demangle([n for n, _ in found])
    out = {}
    for name, (_, body) in zip(names, found):
        r = audit(body)
        if r is not None:
            out[name] = r
    return out


def show(name, r):
    for i, c in enumerate(r['loops']):
        tag = 'main' if c is r['main'] else 'loop'
        print(f"{name} [{tag} {i}]: {c['lines']} instructions: {c['mfma']} MFMAs, {c['valu']} plain VALU, {c['trans']} trans, "
              f"{c['acc']} accvgpr, {c['lds']} LDS, {c['vmem']} global ({c['loads']} loads), {c['salu']} SALU")
        print('    ' + ', '.join(f"{k} x {v}" for k, v in sorted(c['ops'].items(), key=lambda kv: -kv[1])))


def main():
    rep = report(sys.argv[1])
    pats = sys.argv[2:]
    for name in sorted(rep):
        if pats and not any(p in name for p in pats):
            continue
        show(name, rep[name])
    return 0


if __name__ == '__main__':
    sys.exit(main())
