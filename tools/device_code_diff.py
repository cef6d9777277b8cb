"""Compare the gfx950 device code of two source trees, kernel symbol by kernel symbol (no GPU needed).

    python tools/device_code_diff.py TREE_A TREE_B --out DIR [-D NAME[=VALUE] ...] [--jobs 8] UNIT [UNIT ...]

TREE_A / TREE_B: two checkouts of this repository (e.g. the parent commit's and the working tree).  UNIT: a translation
unit of csrc/ without its extension (lfgc_bwd_ch8, lfgc_backward, ...); a unit that only one tree has is compiled there.
Each unit is compiled with this tree's build.FLAGS plus -S --offload-device-only -Rpass-analysis=kernel-resource-usage
(and the -D given), the assembly and the remarks are kept under DIR/A and DIR/B, and every kernel symbol is compared on
  * its instruction text: the lines between the kernel's label and its descriptor, comments stripped, local labels
    renamed in order of first appearance;
  * the .amdhsa_* fields of its descriptor other than .amdhsa_kernarg_size;
  * its resource remarks (registers, scratch, occupancy, spills, LDS).
A symbol is matched by name across all units of a tree, so a kernel that moved to another unit, or that several units
used to hold a copy of, is still compared.  Per symbol one of
  identical   all three equal
  permuted    same opcode histogram and same remarks (operands or order differ)
  moved       anything else; instruction counts and remarks of both sides are listed
  only in A / only in B
The table goes to stdout and to DIR/report.md, the same data to DIR/report.json.  It compares two builds and nothing else.
"""
import argparse
import collections
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CSRC = os.path.join('latent_feature_grid_compression_amd', 'csrc')
REMARK = re.compile(r'remark:\s+(.+?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]')
LOCAL_LABEL = re.compile(r'\.L[A-Za-z0-9_$.]+')
REGS = ('VGPRs', 'AGPRs', 'TotalSGPRs')
SCRATCH, OCCUPANCY = 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]'


def parse_asm(text):
    """{symbol: {'lines': [...], 'desc': {field: value}}} for every .amdhsa_kernel of one assembly file."""
    lines = text.splitlines()
    label_at = {}
    for i, l in enumerate(lines):
        m = re.match(r'([A-Za-z_$][\w$.]*):', l)
        if m:
            label_at.setdefault(m.group(1), i)
    kernels = {}
    for i, l in enumerate(lines):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', l)
        if not m:
            continue
        sym = m.group(1)
        desc = {}
        for d in lines[i + 1:]:
            if d.strip().startswith('.end_amdhsa_kernel'):
                break
            f = d.split(';')[0].split()
            if len(f) >= 2 and f[0].startswith('.amdhsa_') and f[0] != '.amdhsa_kernarg_size':
                desc[f[0]] = ' '.join(f[1:])
        body, names = [], {}
        for b in lines[label_at[sym] + 1:i]:
            b = b.split(';')[0].strip()
            if b.startswith('.section'):
                break
            if b:
                body.append(LOCAL_LABEL.sub(lambda t: names.setdefault(t.group(0), '.L%d' % len(names)), b))
        kernels[sym] = {'lines': body, 'desc': desc}
    return kernels


def parse_remarks(text):
    """{symbol: {remark name: value}} from the compiler's kernel-resource-usage remarks."""
    out, cur = {}, None
    for m in REMARK.finditer(text):
        if m.group(1) == 'Function Name':
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def opcodes(lines):
    return collections.Counter(l.split()[0] for l in lines if not l.endswith(':') and not l.startswith('.'))


def n_instructions(lines):
    return sum(opcodes(lines).values())


def classify(a, b):
    if a['lines'] == b['lines'] and a['desc'] == b['desc'] and a['remarks'] == b['remarks']:
        return 'identical'
    if opcodes(a['lines']) == opcodes(b['lines']) and a['remarks'] == b['remarks']:
        return 'permuted'
    return 'moved'


def compile_unit(hipcc, flags, tree, unit, out_dir):
    src = os.path.join(tree, CSRC, unit + '.hip')
    if not os.path.exists(src):
        return unit, None
    asm = os.path.join(out_dir, unit + '.s')
    r = subprocess.run([hipcc] + flags + ['-S', '--offload-device-only', '-Rpass-analysis=kernel-resource-usage', src, '-o', asm],
                       capture_output=True, text=True)
    with open(os.path.join(out_dir, unit + '.remarks.txt'), 'w') as f:
        f.write(r.stderr)
    if r.returncode != 0:
        sys.exit('hipcc failed for %s:\n%s' % (src, r.stderr[-4000:]))
    kernels = parse_asm(open(asm).read())
    remarks = parse_remarks(r.stderr)
    for sym, k in kernels.items():
        k['remarks'] = remarks.get(sym, {})
    return unit, kernels


def build_side(hipcc, flags, tree, units, out_dir, jobs):
    """{symbol: {unit: kernel}} of one tree."""
    os.makedirs(out_dir, exist_ok=True)
    side = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        for unit, kernels in ex.map(lambda u: compile_unit(hipcc, flags, tree, u, out_dir), units):
            for sym, k in (kernels or {}).items():
                side.setdefault(sym, {})[unit] = k
    return side


def demangle(symbols):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    for cand in ('/opt/rocm/llvm/bin/llvm-cxxfilt', '/opt/rocm/lib/llvm/bin/llvm-cxxfilt'):
        tool = tool or (cand if os.path.exists(cand) else None)
    if not tool or not symbols:
        return {s: s for s in symbols}
    r = subprocess.run([tool], input='\n'.join(symbols) + '\n', capture_output=True, text=True)
    names = r.stdout.splitlines()
    return dict(zip(symbols, names)) if r.returncode == 0 and len(names) == len(symbols) else {s: s for s in symbols}


def compare(side_a, side_b):
    """One row per symbol.  A symbol with copies in several units is compared copy by copy (same unit where both trees
    have it there, else against the other tree's first copy) and gets the worst verdict."""
    rank = {'identical': 0, 'permuted': 1, 'moved': 2}
    rows = []
    for sym in sorted(set(side_a) | set(side_b)):
        ca, cb = side_a.get(sym, {}), side_b.get(sym, {})
        row = {'symbol': sym, 'units_a': sorted(ca), 'units_b': sorted(cb)}
        if not ca or not cb:
            row['status'] = 'only in A' if ca else 'only in B'
            only = next(iter((ca or cb).values()))
            row['a' if ca else 'b'] = {'instructions': n_instructions(only['lines']), 'remarks': only['remarks']}
        else:
            first_a, first_b = ca[sorted(ca)[0]], cb[sorted(cb)[0]]
            pairs = [(ca[u], cb.get(u, first_b)) for u in sorted(ca)] + [(first_a, cb[u]) for u in sorted(cb) if u not in ca]
            verdicts = [(classify(x, y), x, y) for x, y in pairs]
            status, x, y = max(verdicts, key=lambda v: rank[v[0]])
            row['status'] = status
            row['a'] = {'instructions': n_instructions(x['lines']), 'remarks': x['remarks']}
            row['b'] = {'instructions': n_instructions(y['lines']), 'remarks': y['remarks']}
        rows.append(row)
    return rows


def cell(row, key):
    vals = []
    for s in ('a', 'b'):
        if s in row:
            r = row[s]['remarks']
            vals.append(str(row[s]['instructions']) if key == 'instructions' else
                        '/'.join(r.get(k, '?') for k in REGS) if key == 'regs' else r.get(key, '?'))
    return vals[0] if len(set(vals)) == 1 else ' -> '.join(vals)


def report(rows, names, title):
    out = ['# ' + title, '']
    counts = collections.Counter(r['status'] for r in rows)
    out.append(', '.join('%d %s' % (counts[s], s) for s in ('identical', 'permuted', 'moved', 'only in A', 'only in B') if counts[s])
               or 'no kernel symbols')
    out += ['', '| kernel | status | instructions | VGPR/AGPR/SGPR | scratch B/lane | occupancy | units A | units B |',
            '|---|---|---|---|---|---|---|---|']
    for r in sorted(rows, key=lambda r: (r['units_b'] or r['units_a'], names[r['symbol']])):
        out.append('| `%s` | %s | %s | %s | %s | %s | %s | %s |' % (
            names[r['symbol']], r['status'], cell(r, 'instructions'), cell(r, 'regs'), cell(r, SCRATCH), cell(r, OCCUPANCY),
            ' '.join(r['units_a']) or '-', ' '.join(r['units_b']) or '-'))
    return '\n'.join(out) + '\n'


def main():
    from latent_feature_grid_compression_amd import build
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('tree_a')
    ap.add_argument('tree_b')
    ap.add_argument('units', nargs='+')
    ap.add_argument('--out', required=True, help='directory for the assembly, the remarks and the report')
    ap.add_argument('-D', dest='defines', action='append', default=[])
    ap.add_argument('--jobs', type=int, default=8)
    args = ap.parse_args()
    flags = build.FLAGS + ['-D' + d for d in args.defines]
    sides = [build_side(build._hipcc(), flags, os.path.abspath(t), args.units, os.path.join(args.out, s), args.jobs)
             for t, s in ((args.tree_a, 'A'), (args.tree_b, 'B'))]
    rows = compare(*sides)
    names = demangle(sorted(r['symbol'] for r in rows))
    text = report(rows, names, 'device code, A = %s against B = %s%s' % (
        args.tree_a, args.tree_b, ''.join(' -D' + d for d in args.defines)))
    with open(os.path.join(args.out, 'report.md'), 'w') as f:
        f.write(text)
    with open(os.path.join(args.out, 'report.json'), 'w') as f:
        json.dump([dict(r, name=names[r['symbol']]) for r in rows], f, indent=1)
    sys.stdout.write(text)


if __name__ == '__main__':
    main()
