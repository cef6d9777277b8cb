"""A/B timing of forward-kernel variants on ONE box (devices differ by several per cent, so variants are only ever
compared inside one gpurun call): builds the library once per -D set, then times the headline launch with each,
interleaved over a few rounds.

    python tools/ab_forward.py build name1=DEF1,DEF2 name2=DEF3 ...     # here (hipcc); "name=" = no defines
    python tools/ab_forward.py run [--precision f16x2] [--workload headline] [--rounds 3] [--steps 10] [--warmup 3]   # on the GPU box

A library put into the directory by hand (liblfgc_ab_<name>.so, e.g. the parent commit's build) is timed with the rest.
The first bench run that fails ends the whole A/B: nothing more is started on a device that may have faulted.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get('LFGC_AB_DIR') or os.path.join(ROOT, 'tools', 'microbench', 'ablate')

if sys.argv[1] == 'build':
    from latent_feature_grid_compression_amd.build import build_variant
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        if f.startswith('liblfgc_ab_') and f.endswith('.so'):
            os.remove(os.path.join(OUT, f))
    for spec in sys.argv[2:]:
        name, _, defs = spec.partition('=')
        build_variant(os.path.join(OUT, 'liblfgc_ab_%s.so' % name), [d for d in defs.split(',') if d])
else:
    args = sys.argv[2:]
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d      # noqa: E731
    rounds = int(opt('--rounds', 3))
    extra = ['--steps', opt('--steps', '10'), '--warmup', opt('--warmup', '3')]
    for k in ('--precision', '--workload'):
        if k in args:
            extra += [k, args[args.index(k) + 1]]
    names = sorted(f[len('liblfgc_ab_'):-3] for f in os.listdir(OUT) if f.startswith('liblfgc_ab_') and f.endswith('.so'))
    res = {n: [] for n in names}
    val = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            env = dict(os.environ, LFGC_LIB_PATH=os.path.join(OUT, 'liblfgc_ab_%s.so' % n))
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--no-cpu-baseline', '--no-check'] + extra,
                               env=env, capture_output=True, text=True, timeout=240)
            line = [l for l in r.stdout.splitlines() if l.startswith('{')]
            if r.returncode != 0 or not line:
                print(n, 'exit', r.returncode, r.stderr[-400:], flush=True)
                sys.exit(1)
            j = json.loads(line[-1])
            res[n].append(j['roofline']['kernel_ms'])
            val[n].append(j['value'])
            print('# %-26s kernel_ms %.3f' % (n, res[n][-1]), flush=True)
    for n in names:
        print('%-28s kernel_ms median %.3f  min %.3f  max %.3f  all %s | value median %.1f  all %s' %
              (n, statistics.median(res[n]), min(res[n]), max(res[n]), ' '.join('%.3f' % v for v in res[n]),
               statistics.median(val[n]), ' '.join('%.1f' % v for v in val[n])), flush=True)
