"""ISA audit for the scorer's tile loop: are its global loads issued where the compiler can count them?

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -S --cuda-device-only -o score.s csrc/score.hip
    python tests/isa_audit/audit_score_loads.py score.s ['<128, 5, false, false, 8, 0>' ...]

Memory operations return in order, so a wave can wait for an OLDER load with `s_waitcnt vmcnt(N)` and leave its N younger loads in
flight - but only if the compiler knows that N younger loads were issued.  One younger load under a condition (a lane mask or a
uniform branch) and it has to assume the load was skipped: the wait becomes `vmcnt(0)` and drains every prefetch.  A load written
as `x = ok ? p[i] : 0` is compiled into an exec-mask region of its own (v_cmp, s_and_saveexec_b64, s_cbranch_execz, the load,
s_or_b64 exec), so the audit reports, for the tile loop of a kernel (the loop with the most MFMAs that holds an s_barrier):

  loads         global_load / buffer_load instructions in the loop
  guarded       ... of them inside an exec-mask region (between an s_and_saveexec_b64 and the s_or_b64 exec that closes it)
  waits         every s_waitcnt with a vmcnt in the loop, with its position: loads and MFMAs issued before it in listing order
  branches      s_cbranch_* / s_branch in the loop, and how many of them are s_cbranch_exec*
  lines         instructions in the loop
"""
import re
import subprocess
import sys


def kernels(lines, prefix='score_kernel'):
    """(mangled name, body lines) of every kernel of the listing whose name holds `prefix`."""
    i = 0
    while i < len(lines):
        m = re.match(r'^(_Z\S*' + prefix + r'\S*):', lines[i])
        if m:
            j = i
            while j < len(lines) and not lines[j].startswith('.Lfunc_end'):
                j += 1
            yield m.group(1), lines[i:j]
            i = j
        i += 1


def demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    res = []
    for n in out[:len(names)]:
        n = re.sub(r'\(anonymous namespace\)::', '', n)
        res.append(re.sub(r'\(.*', '', n).replace('void ', ''))
    return res


def _instr(line):
    t = line.split(';')[0].strip()
    if not t or t.startswith('.') or t.endswith(':'):
        return None
    return t


def _blocks(body):
    """(first line, last line + 1, loop header the block belongs to or None, is a loop header) of every basic block."""
    starts = [n for n, l in enumerate(body) if re.match(r'^(\.LBB\d+_\d+:|; %bb\.\d+:)', l)]
    out = []
    for i, n in enumerate(starts):
        end = starts[i + 1] if i + 1 < len(starts) else len(body)
        head = ' '.join(body[n:min(n + 3, end)])
        label = re.match(r'^\.(LBB\d+_\d+):', body[n])
        if 'Loop Header' in body[n] and label:
            out.append((n, end, '.' + label.group(1), True))
        else:
            m = re.search(r'in Loop: Header=(BB\d+_\d+)', head)
            out.append((n, end, '.L' + m.group(1) if m else None, False))
    return out


def tile_loop(body):
    """Line numbers of the tile loop in execution order (from its header on; hipcc lays some of its blocks out in front of the
    header): among the loops that hold an s_barrier the one with the most MFMAs, by the listing's own loop annotations
    ("=>This Loop Header", "in Loop: Header=BBn_m").  None if no loop holds a barrier."""
    blocks = _blocks(body)
    best = None
    for n, _, hdr, is_hdr in blocks:
        if not is_hdr:
            continue
        mine = [(a, b) for a, b, h, _ in blocks if h == hdr]
        idx = [k for a, b in mine if a >= n for k in range(a, b)] + [k for a, b in mine if a < n for k in range(a, b)]
        if not any(re.match(r'\s+s_barrier', body[k]) for k in idx):
            continue
        mf = sum(1 for k in idx if re.match(r'\s+v_mfma', body[k]))
        if best is None or mf > best[0]:
            best = (mf, idx)
    return None if best is None else best[1]


def audit(body):
    """The report described in the module docstring for one kernel body; None if the kernel has no barrier loop."""
    span = tile_loop(body)
    if span is None:
        return None
    rep = {'loads': 0, 'guarded': 0, 'waits': [], 'branches': 0, 'exec_branches': 0, 'lines': 0, 'mfma': 0, 'ds_write': 0}
    depth = 0
    for k in span:
        t = _instr(body[k])
        if t is None:
            continue
        rep['lines'] += 1
        op = t.split()[0]
        if op == 's_and_saveexec_b64':
            depth += 1
        elif op == 's_or_b64' and re.match(r's_or_b64\s+exec\s*,', t):
            depth = max(0, depth - 1)
        elif re.match(r'(global|buffer)_load', op):
            rep['loads'] += 1
            rep['guarded'] += 1 if depth > 0 else 0
        elif op.startswith('v_mfma'):
            rep['mfma'] += 1
        elif op.startswith('ds_write'):
            rep['ds_write'] += 1
        elif op == 's_waitcnt':
            m = re.search(r'vmcnt\((\d+)\)', t)
            if m:
                rep['waits'].append({'vmcnt': int(m.group(1)), 'loads_before': rep['loads'], 'mfma_before': rep['mfma'],
                                     'ds_write_before': rep['ds_write'], 'guarded': depth > 0})
        elif op.startswith('s_cbranch') or op == 's_branch':
            rep['branches'] += 1
            rep['exec_branches'] += 1 if op.startswith('s_cbranch_exec') else 0
    rep['vmcnt0'] = sum(1 for w in rep['waits'] if w['vmcnt'] == 0)
    rep['partial'] = sum(1 for w in rep['waits'] if w['vmcnt'] > 0)
    return rep


def report(path, prefix='score_kernel'):
    """{demangled kernel name: audit report} for every kernel of the listing with a barrier loop."""
    lines = open(path).read().split('\n')
    found = list(kernels(lines, prefix))
    names = demangle([n for n, _ in found])
    out = {}
    for name, (_, body) in zip(names, found):
        r = audit(body)
        if r is not None:
            out[name] = r
    return out


def show(name, r):
    print(f"{name}: loop of {r['lines']} instructions, {r['mfma']} MFMAs, {r['loads']} global loads ({r['guarded']} in an exec-mask "
          f"region), {r['branches']} branches ({r['exec_branches']} on exec), vmcnt(0) x {r['vmcnt0']}, partial waits x {r['partial']}")
    for w in r['waits']:
        print(f"    s_waitcnt vmcnt({w['vmcnt']:2d})  after {w['loads_before']:2d} loads, {w['mfma_before']:3d} MFMAs, "
              f"{w['ds_write_before']:2d} ds_write of the loop{'  [inside an exec-mask region]' if w['guarded'] else ''}")


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
