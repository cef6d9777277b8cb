"""Time of one direct-volume-rendered frame of the cfg-3 synthetic model (visualization/Render.py):
a 1024^2 pinhole view of the 256^3 volume's box at the default step (half a voxel), without and with headlight shading.

    python tools/bench_render.py [--size 1024] [--frames 3] [--precision f16x2] [--iso VALUE]     # on the GPU box

With --iso VALUE a third mode follows: a first-hit isosurface frame (Render.isosurface, normals included) of the same
model and rays at that isovalue, timed the same way next to the two DVR frames, with the number of bracketed rays.

With --skip the unshaded frame is then rendered with and without empty-space skipping (Render.BrickRanges), alternating
in the same run: time to build the ranges (forward and reduction), occupied share of the bricks, samples, skipped
blocks, live rays per block, ms per frame of both, GPU time of the skip kernel, the difference of the two images, and
Render.brick_range_excess of this model and of cfg 3 after a short training run on bench.py's smooth volume -- the two
measurements Render.NET_SKIP_MARGIN is derived from (twice the larger, rounded up to one significant digit).

With --tf2d (or --modes tf2d alone) the headlight frame is rendered under the 1-D table, under the same table repeated
along a gradient axis and under TransferFunction2D.from_ramp of it (ramp between the quartiles of the model's |gradient|),
alternating in the same run, the ramp frame also with empty-space skipping; before that Render.joint_histogram_from_net of
the model at 256^3 is split into gradient evaluation and binning, and the binning kernel is timed alone.

With --preint (or --modes preint alone) the unshaded and the headlight frame are rendered under the midpoint rule and with
pre-integrated classification (render(..., preintegrated=True)) at steps h, 2h, 4h and 8h, h the default half voxel, the
two rules alternating in the same run: ms per frame, samples, GPU time of each rule's composite kernel and image_psnr
against ONE reference image, the midpoint rule at h/4; then the largest step at which the pre-integrated frame still has
the PSNR of the midpoint frame at h.  The same follows for cfg 3 after --skip-trained-steps train steps on bench.py's
smooth volume (0: left out).

Prints, per mode: ms per frame (wall clock around whole frames, synchronised), samples evaluated and samples/s, the
live-ray count per block of 32 steps, the share of GPU time in the ray kernels against the network evaluation (HIP events
around every launch of one extra, instrumented frame), and the rate of ops.forward_raw alone on the same positions in the
same launch sizes, measured in the same run.  Then one JSON summary line.  A tool, not a test, and nothing of bench.py.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--precision', default='f16x2')
    ap.add_argument('--opacity-limit', type=float, default=0.999)
    ap.add_argument('--iso', type=float, default=None, help='also time an isosurface frame at this isovalue')
    ap.add_argument('--modes', default='', help='comma-separated subset of unshaded,headlight,isosurface to time (default: all); tf2d: the --tf2d report')
    ap.add_argument('--zero-below', type=float, default=0.5,
                    help='share of the value range, from its lower end, over which the table has no extinction (the scene: 0.5)')
    ap.add_argument('--skip', action='store_true', help='also compare the unshaded frame with and without empty-space skipping')
    ap.add_argument('--brick', type=int, default=8, help='--skip: brick edge in cells')
    ap.add_argument('--skip-margin', default=None,
                    help="--skip: margin of the brick ranges; default Render.NET_SKIP_MARGIN, 'auto' = the margin derived in this run")
    ap.add_argument('--skip-trained-steps', type=int, default=113,
                    help='--skip: train steps of the second model brick_range_excess is measured on (0: leave it out)')
    ap.add_argument('--tf2d', action='store_true',
                    help='also time the headlight frame under TransferFunction2D.from_ramp of the table, and the joint histogram')
    ap.add_argument('--tf2d-kg', type=int, default=64, help='--tf2d: rows of the gradient axis')
    ap.add_argument('--preint', action='store_true',
                    help='also compare the midpoint rule and pre-integrated classification at steps h, 2h, 4h and 8h')
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from latent_feature_grid_compression_amd import ops
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    from latent_feature_grid_compression_amd.visualization import Render

    dev = torch.device('cuda:0')
    m = bench.build_model(bench.WORKLOADS['headline'], seed=2003, device=dev).eval()
    m.precision = args.precision
    ds = IndexDataset((256, 256, 256), 16, build_index_table=False)
    step = 1.0 / float(ds.max_dim)
    scales = ds.scales.tolist()
    box = ([-s for s in scales], scales)
    # grey-to-warm ramp, extinction 0 below the middle of the value range and rising to 12 per unit length above it
    v = np.linspace(0.0, 1.0, 9)
    ramp = 2.0 * v - 1.0 if args.zero_below == 0.5 else (v - args.zero_below) / (1.0 - args.zero_below)
    table = np.stack([0.3 + 0.7 * v, 0.3 + 0.4 * v, 0.4 - 0.3 * v, 12.0 * np.clip(ramp, 0.0, 1.0)], 1)
    tf = Render.TransferFunction(table)
    o, d = Render.pinhole_rays((2.6, 1.7, 1.4), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 35.0, args.size, args.size, device=dev)
    with torch.no_grad():
        desc, grid_cl, packed = m._descriptor(), m._decoded_channel_last(), m._packed()

    def plain(pos):
        with torch.no_grad():
            return ops.forward_raw(desc, grid_cl, packed, pos=pos, clamp=True, precision=args.precision)[0]

    def shaded(pos):
        val, g = m.value_and_gradient(pos)
        return val.view(-1), g

    def plain_or_shaded(pos, gradient=False):
        return shaded(pos) if gradient else plain(pos)

    def frame(mode, fn, **kw):
        if mode == 'isosurface':
            return Render.isosurface(fn, o, d, args.iso, step, box[0], box[1], **kw)
        return Render.render(fn, o, d, tf, step, box[0], box[1], opacity_limit=args.opacity_limit,
                             shading=None if mode == 'unshaded' else 'headlight', **kw)

    summary = {'size': args.size, 'step': step, 'precision': args.precision, 'opacity_limit': args.opacity_limit,
               'zero_below': args.zero_below}
    modes = [('unshaded', plain), ('headlight', shaded)] + ([('isosurface', plain_or_shaded)] if args.iso is not None else [])
    if args.modes:
        modes = [x for x in modes if x[0] in args.modes.split(',')]
    ray_ops = ('ray_clip', 'ray_samples', 'ray_composite', 'ray_compact', 'ray_iso_scan', 'ray_iso_refine', 'ray_iso_finish')
    for mode, fn in modes:
        stats = {}
        frame(mode, fn, stats=stats)                                                       # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.frames):
            t0 = time.perf_counter()
            img = frame(mode, fn)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        # one instrumented frame: an event pair around every launch group
        spans = {name[4:]: [] for name in ray_ops}
        spans['value_fn'] = []
        kept = []

        def timed(name, f):
            def g(*a, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = f(*a, **k)
                e1.record()
                spans[name].append((e0, e1))
                return r
            return g

        def fn_kept(pos, *a, **k):
            kept.append(pos)
            return fn(pos, *a, **k)
        saved = {name: getattr(ops, name) for name in ray_ops}
        try:
            for name in ray_ops:
                setattr(ops, name, timed(name[4:], saved[name]))
            seen = [float('inf'), float('-inf')]

            def fn_range(pos, *a, **k):                       # the value range of the march, outside the timed span
                r = timed_fn(pos, *a, **k)
                if mode == 'isosurface' and not k.get('gradient'):
                    lo, hi = torch.aminmax(r)
                    seen[0], seen[1] = min(seen[0], float(lo)), max(seen[1], float(hi))
                return r
            timed_fn = timed('value_fn', fn_kept)
            frame(mode, fn_range if mode == 'isosurface' else timed_fn)
        finally:
            for name in ray_ops:
                setattr(ops, name, saved[name])
        torch.cuda.synchronize()
        gpu = {k: float(sum(a.elapsed_time(b) for a, b in v_)) for k, v_ in spans.items()}
        new = sum(v_ for k, v_ in gpu.items() if k != 'value_fn')
        # ops.forward_raw alone on the same positions, launch by launch
        for p in kept[:2]:
            plain(p)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for p in kept:
            plain(p)
        e1.record()
        torch.cuda.synchronize()
        fwd_ms = e0.elapsed_time(e1)
        n = stats['samples'] + stats.get('refine_samples', 0)
        best = min(ms)
        print('[%s] %.1f ms per frame (best of %d: %s)' % (mode, best, len(ms), ' '.join('%.1f' % x for x in ms)))
        print('[%s] %d samples in %d blocks of 32 steps, %d launches: %.2f Gsamples/s over the frame' % (
            mode, n, stats['blocks'], len(kept), n / best / 1e6))
        print('[%s] live rays per block: %s' % (mode, ' '.join(str(x) for x in stats['live'])))
        split = ', '.join('%s %.2f' % (k, v_) for k, v_ in gpu.items() if k != 'value_fn' and spans[k])
        print('[%s] GPU time of the instrumented frame: value_fn %.1f ms, ray kernels %.1f ms (%s) = %.1f %% of value_fn'
              % (mode, gpu['value_fn'], new, split, 100.0 * new / gpu['value_fn']))
        print('[%s] ops.forward_raw alone on the same positions: %.1f ms = %.2f Gsamples/s' % (mode, fwd_ms, n / fwd_ms / 1e6))
        if mode == 'isosurface':
            print('[%s] iso %g: %d rays bracketed of %d that hit the box; %d samples in the march, %d in %d bisections, at the '
                  'hit points and for the normals; values seen in [%.4f, %.4f]'
                  % (mode, args.iso, stats['bracketed'], stats['live'][0] if stats['live'] else 0, stats['samples'],
                     stats['refine_samples'], 8, seen[0], seen[1]), flush=True)
        else:
            print('[%s] image: mean opacity %.3f, %d of %d rays hit' % (mode, float(img[:, 3].mean()),
                                                                      stats['live'][0] if stats['live'] else 0, o.shape[0]), flush=True)
        summary[mode] = {'frame_ms': ms, 'samples': n, 'blocks': stats['blocks'], 'live': stats['live'], 'gpu_ms': gpu,
                         'ray_kernels_ms': new, 'forward_alone_ms': fwd_ms}
        if mode == 'isosurface':
            summary[mode].update(iso=args.iso, bracketed=stats['bracketed'], refine_samples=stats['refine_samples'])
        del kept, img
        torch.cuda.empty_cache()
    if args.skip:
        summary['skip'] = skip_report(args, m, ds, tf, o, d, step, box, plain)
    if args.tf2d or 'tf2d' in args.modes.split(','):
        summary['tf2d'] = tf2d_report(args, m, ds, tf, o, d, step, box, shaded)
    if args.preint or 'preint' in args.modes.split(','):
        summary['preint'] = preint_report(args, m, ds, tf, o, d)
    print(json.dumps(summary), flush=True)


def one_digit_up(x: float) -> float:
    """x rounded up to one significant digit (0 stays 0)."""
    import math
    if not x > 0.0:
        return 0.0
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


def skip_report(args, m, ds, tf, o, d, step, box, plain) -> dict:
    """--skip: the unshaded frame with and without empty-space skipping (Render.BrickRanges), alternating in one run."""
    import statistics
    import torch
    import bench
    from latent_feature_grid_compression_amd import ops
    from latent_feature_grid_compression_amd.visualization import Render
    dev = o.device
    Render.BrickRanges.from_net(ds, m, brick=args.brick)                                   # warm-up
    build = {}
    t0 = time.perf_counter()
    ranges = Render.BrickRanges.from_net(ds, m, brick=args.brick, timings=build)
    build['wall_ms'] = (time.perf_counter() - t0) * 1e3
    excess = Render.brick_range_excess(ranges, plain)
    # the second model of the margin's derivation: cfg 3 after a short training run on the smooth volume
    trained = None
    if args.skip_trained_steps > 0:
        ctx = bench.cfg3_train_setup(dev, args.precision)
        for _ in range(args.skip_trained_steps):
            ctx['step']()
        tm = ctx['model'].eval()
        with torch.no_grad():
            tdesc, tgrid, tpacked = tm._descriptor(), tm._decoded_channel_last(), tm._packed()

        def trained_fn(pos):
            with torch.no_grad():
                return ops.forward_raw(tdesc, tgrid, tpacked, pos=pos, clamp=True, precision=args.precision)[0]
        t_ranges = Render.BrickRanges.from_net(ctx['ds'], tm, brick=args.brick)
        trained = {'steps': args.skip_trained_steps, 'excess': Render.brick_range_excess(t_ranges, trained_fn),
                   'value_range': [float(t_ranges.minmax[..., 0].min()), float(t_ranges.minmax[..., 1].max())]}
        del ctx, tm, tdesc, tgrid, tpacked, t_ranges
        torch.cuda.empty_cache()
    derived = one_digit_up(2.0 * max(excess, trained['excess'] if trained else 0.0))
    margin = ranges.default_margin if args.skip_margin is None else (derived if args.skip_margin == 'auto' else float(args.skip_margin))
    occ = ranges.occupancy(tf, margin)

    def frame(skip, stats=None):
        return Render.render(plain, o, d, tf, step, box[0], box[1], opacity_limit=args.opacity_limit, stats=stats,
                             skip=ranges if skip else None, skip_margin=margin if skip else None)
    st = {False: {}, True: {}}
    img = {k: frame(k, st[k]) for k in (False, True)}                                      # warm-up, stats and the two images
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(args.frames):                                                           # alternating, same process
        for k in (False, True):
            t0 = time.perf_counter()
            frame(k)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    spans, saved = [], ops.ray_skip

    def timed_skip(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        saved(*a, **k)
        e1.record()
        spans.append((e0, e1))
    try:
        ops.ray_skip = timed_skip
        frame(True)
    finally:
        ops.ray_skip = saved
    torch.cuda.synchronize()
    skip_ms = float(sum(a.elapsed_time(b) for a, b in spans))
    diff = float((img[True] - img[False]).abs().max())
    out = {'brick': args.brick, 'margin': margin, 'derived_margin': derived, 'build_ms': build, 'excess_random': excess,
           'trained': trained, 'bricks': int(occ.numel()), 'occupied_share': float(occ.float().mean()),
           'samples': [st[False]['samples'], st[True]['samples']], 'skipped_blocks': st[True]['skipped_blocks'],
           'blocks': [st[False]['blocks'], st[True]['blocks']], 'live': st[True]['live'],
           'frame_ms': [ms[False], ms[True]], 'skip_kernel_ms': skip_ms, 'skip_launches': len(spans), 'max_abs': diff,
           'psnr_dB': Render.image_psnr(img[True], img[False])}
    fmt = lambda v: 'min %.1f median %.1f max %.1f' % (min(v), statistics.median(v), max(v))      # noqa: E731
    print('[skip] ranges of %s bricks of %d^3 cells: %.2f ms forward + %.2f ms reduction on the GPU in %d slabs (%.1f ms wall)'
          % (tuple(occ.shape), args.brick, build['forward_ms'], build['reduce_ms'], build['slabs'], build['wall_ms']))
    print('[skip] brick_range_excess: %.3e (this model)%s -> derived margin %g; margin used %g'
          % (excess, '' if trained is None else ', %.3e (cfg 3 after %d train steps on the smooth volume, values in [%.3f, %.3f])'
             % (trained['excess'], trained['steps'], *trained['value_range']), derived, margin))
    print('[skip] %.1f %% of the bricks occupied; samples %d -> %d (%.1f %%), %d blocks of 32 steps skipped'
          % (100.0 * out['occupied_share'], out['samples'][0], out['samples'][1], 100.0 * out['samples'][1] / max(out['samples'][0], 1),
             out['skipped_blocks']))
    print('[skip] live rays per block with skipping: %s' % ' '.join(str(x) for x in out['live']))
    print('[skip] ms per frame over %d alternating frames: without %s; with %s' % (args.frames, fmt(ms[False]), fmt(ms[True])))
    print('[skip] GPU time of the skip kernel: %.2f ms in %d launches; the two frames differ by max abs %.3e, PSNR %.1f dB'
          % (skip_ms, len(spans), diff, out['psnr_dB']), flush=True)
    return out


def tf2d_report(args, m, ds, tf, o, d, step, box, shaded) -> dict:
    """--tf2d (or --modes tf2d): the headlight frame under the 1-D table, under the same table repeated along the gradient
    axis (the same image: the lookup's cost alone) and under TransferFunction2D.from_ramp of it (extinction ramped from
    the lower to the upper quartile of the model's |gradient|), alternating in one run; the ramp frame with and without
    empty-space skipping; and Render.joint_histogram_from_net of the model, split into gradient evaluation and binning."""
    import statistics
    import torch
    from latent_feature_grid_compression_amd import ops
    from latent_feature_grid_compression_amd.visualization import Render
    dev = o.device
    n_vox = int(ds.n_voxels)
    # ---- the joint histogram: one untimed pass for g_max and the warm-up, then the timed binning pass
    _, g_max = Render.joint_histogram_from_net(ds, m, bins=(64, 64))
    spans, saved = [], ops.joint_histogram

    def timed_hist(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = saved(*a, **k)
        e1.record()
        spans.append((e0, e1))
        return r
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        ops.joint_histogram = timed_hist
        e0.record()
        counts, _ = Render.joint_histogram_from_net(ds, m, bins=(64, 64), g_max=g_max)
        e1.record()
    finally:
        ops.joint_histogram = saved
    torch.cuda.synchronize()
    total_ms = e0.elapsed_time(e1)
    bin_ms = float(sum(a.elapsed_time(b) for a, b in spans))
    assert int(counts.sum()) == n_vox
    by_g = counts.sum(0).double().cumsum(0) / n_vox                  # the marginal of |gradient|: its quartiles
    edge = lambda q: float((int((by_g < q).sum()) + 1) * g_max / counts.shape[1])      # noqa: E731
    g_lo, g_hi = edge(0.25), edge(0.75)
    hist = {'voxels': n_vox, 'g_max': g_max, 'g_lo': g_lo, 'g_hi': g_hi, 'total_ms': total_ms, 'binning_ms': bin_ms,
            'launches': len(spans), 'binning_GBps': 16.0 * n_vox / bin_ms / 1e6}
    print('[tf2d] joint histogram of %d voxels, 64 x 64 bins: %.2f ms on the GPU, of which binning %.3f ms in %d launches = '
          '%.0f GB/s at 16 B per sample (%.1f %% of 8 TB/s); |gradient| max %.3f, quartiles %.3f and %.3f'
          % (n_vox, total_ms, bin_ms, len(spans), hist['binning_GBps'], hist['binning_GBps'] / 80.0, g_max, g_lo, g_hi))
    # the binning kernel alone, one launch over 2^24 samples: spread over all bins, and all in one bin (LDS atomics collide)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    n_syn = 1 << 24
    syn = {'spread': (2.0 * torch.rand(n_syn, generator=gen, device=dev) - 1.0, 0.3 * torch.randn((n_syn, 3), generator=gen, device=dev)),
           'one_bin': (torch.zeros(n_syn, device=dev), torch.zeros((n_syn, 3), device=dev))}
    for name, (sv, sg) in syn.items():
        acc = ops.joint_histogram(sv, sg, (64, 64), -1.0, 1.0, 1.0)                        # warm-up
        best = float('inf')
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.joint_histogram(sv, sg, (64, 64), -1.0, 1.0, 1.0, acc)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        hist['one_launch_%s_ms' % name], hist['one_launch_%s_GBps' % name] = best, 16.0 * n_syn / best / 1e6
        print('[tf2d] binning alone, one launch of 2^24 samples, %s: %.3f ms = %.0f GB/s (%.1f %% of 8 TB/s)'
              % (name, best, hist['one_launch_%s_GBps' % name], hist['one_launch_%s_GBps' % name] / 80.0))
    del syn, sv, sg
    torch.cuda.empty_cache()
    # ---- frames
    flat =Render.TransferFunction2D(tf.table.unsqueeze(1).repeat(1, args.tf2d_kg, 1), tf.v_min, tf.v_max, g_max)
    ramp = Render.TransferFunction2D.from_ramp(tf, g_lo, g_hi, args.tf2d_kg, g_max)
    ranges = Render.BrickRanges.from_net(ds, m, brick=args.brick)
    margin = ranges.default_margin if args.skip_margin in (None, 'auto') else float(args.skip_margin)
    kinds = {'headlight': (tf, None), 'tf2d_flat': (flat, None), 'tf2d': (ramp, None), 'tf2d_skip': (ramp, ranges)}

    def frame(kind, stats=None):
        table, skip = kinds[kind]
        return Render.render(shaded, o, d, table, step, box[0], box[1], opacity_limit=args.opacity_limit, shading='headlight',
                             stats=stats, skip=skip, skip_margin=margin if skip is not None else None)
    st = {k: {} for k in kinds}
    img = {k: frame(k, st[k]) for k in kinds}                                              # warm-up, stats and the images
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    for _ in range(args.frames):                                                           # alternating, same process
        for k in kinds:
            t0 = time.perf_counter()
            frame(k)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    comp = {}
    for k, name in (('headlight', 'ray_composite'), ('tf2d_flat', 'ray_composite2d'), ('tf2d', 'ray_composite2d')):
        spans, saved = [], getattr(ops, name)

        def timed(*a, _f=saved, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _f(*a, **kw)
            e1.record()
            spans.append((e0, e1))
        try:
            setattr(ops, name, timed)
            frame(k)
        finally:
            setattr(ops, name, saved)
        torch.cuda.synchronize()
        comp[k] = float(sum(a.elapsed_time(b) for a, b in spans))
    fmt = lambda v: 'min %.1f median %.1f max %.1f' % (min(v), statistics.median(v), max(v))      # noqa: E731
    out = {'kg': args.tf2d_kg, 'histogram': hist, 'frame_ms': ms, 'samples': {k: st[k]['samples'] for k in kinds},
           'composite_kernel_ms': comp, 'skipped_blocks': st['tf2d_skip']['skipped_blocks'], 'skip_margin': margin,
           'flat_equals_headlight': bool(torch.equal(img['tf2d_flat'], img['headlight'])),
           'skip_max_abs': float((img['tf2d_skip'] - img['tf2d']).abs().max()),
           'mean_opacity': {k: float(img[k][:, 3].mean()) for k in kinds}}
    for k in kinds:
        print('[tf2d] %-10s ms per frame over %d alternating frames: %s; %d samples, mean opacity %.3f'
              % (k, args.frames, fmt(ms[k]), st[k]['samples'], out['mean_opacity'][k]))
    print('[tf2d] spread of the headlight frames: %.1f ms; median tf2d_flat - headlight %.1f ms; the flat 2-D image equals the '
          'headlight image: %s' % (max(ms['headlight']) - min(ms['headlight']),
                                   statistics.median(ms['tf2d_flat']) - statistics.median(ms['headlight']), out['flat_equals_headlight']))
    print('[tf2d] GPU time of the composite kernel over a frame: %s'
          % ', '.join('%s %.2f ms' % (k, v) for k, v in comp.items()))
    print('[tf2d] skipping under the ramp table (margin %g): %d blocks skipped, samples %d -> %d, images differ by max abs %.3e'
          % (margin, out['skipped_blocks'], st['tf2d']['samples'], st['tf2d_skip']['samples'], out['skip_max_abs']), flush=True)
    return out


def preint_report(args, m, ds, tf, o, d) -> dict:
    """--preint (or --modes preint): the midpoint rule against pre-integrated classification over the step, on this model
    and on cfg 3 after a short training run on the smooth volume; the reference image of either is the midpoint rule at a
    quarter of the default step."""
    import statistics
    import torch
    import bench
    from latent_feature_grid_compression_amd import ops
    from latent_feature_grid_compression_amd.visualization import Render
    mults = (1, 2, 4, 8)
    kinds = [(mult, pre) for mult in mults for pre in (False, True)]
    fmt = lambda v: 'min %.1f median %.1f max %.1f' % (min(v), statistics.median(v), max(v))      # noqa: E731

    def table_of(name, model, dataset):
        h = 1.0 / float(dataset.max_dim)
        scales = dataset.scales.tolist()
        lo, hi = [-s for s in scales], scales
        out = {'h': h}
        for mode in ('unshaded', 'headlight'):
            shading = None if mode == 'unshaded' else 'headlight'

            def frame(mult, pre, stats=None):
                return Render.render_from_net(dataset, model, o, d, tf, step=h * mult, opacity_limit=args.opacity_limit,
                                              shading=shading, stats=stats, preintegrated=pre)
            ref = frame(0.25, False)
            st = {k: {} for k in kinds}
            img = {k: frame(*k, st[k]) for k in kinds}                                     # warm-up, stats and the images
            torch.cuda.synchronize()
            ms = {k: [] for k in kinds}
            for _ in range(args.frames):                                                   # alternating, same process
                for k in kinds:
                    t0 = time.perf_counter()
                    frame(*k)
                    torch.cuda.synchronize()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            rows = []
            for k in kinds:
                name_op = 'ray_composite_preint' if k[1] else 'ray_composite'
                spans, saved = [], getattr(ops, name_op)

                def timed(*a, _f=saved, **kw):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _f(*a, **kw)
                    e1.record()
                    spans.append((e0, e1))
                try:
                    setattr(ops, name_op, timed)
                    frame(*k)
                finally:
                    setattr(ops, name_op, saved)
                torch.cuda.synchronize()
                rows.append({'step_over_h': k[0], 'preintegrated': k[1], 'frame_ms': ms[k], 'samples': st[k]['samples'],
                             'composite_kernel_ms': float(sum(a.elapsed_time(b) for a, b in spans)),
                             'psnr_dB': Render.image_psnr(img[k], ref), 'mean_opacity': float(img[k][:, 3].mean())})
            at_h = next(r for r in rows if r['step_over_h'] == 1 and not r['preintegrated'])
            match = [r for r in rows if r['preintegrated'] and r['psnr_dB'] >= at_h['psnr_dB']]
            best = max(match, key=lambda r: r['step_over_h']) if match else None
            out[mode] = {'rows': rows, 'midpoint_at_h_psnr_dB': at_h['psnr_dB'],
                         'largest_matching_step_over_h': best['step_over_h'] if best else None,
                         'frame_ms_there': statistics.median(best['frame_ms']) if best else None}
            for r in rows:
                print('[preint] %s %-9s step %dh %-14s %s ms; %d samples; composite kernel %.2f ms; PSNR %.2f dB against the '
                      'midpoint rule at h/4; mean opacity %.3f'
                      % (name, mode, r['step_over_h'], 'pre-integrated' if r['preintegrated'] else 'midpoint', fmt(r['frame_ms']),
                         r['samples'], r['composite_kernel_ms'], r['psnr_dB'], r['mean_opacity']))
            print('[preint] %s %s: the midpoint rule at h has %.2f dB; the largest step at which the pre-integrated frame still has '
                  'that: %s' % (name, mode, at_h['psnr_dB'], 'none' if best is None else '%dh, %.1f ms per frame (midpoint at h: %.1f)'
                                % (best['step_over_h'], out[mode]['frame_ms_there'], statistics.median(at_h['frame_ms']))),
                  flush=True)
            del img, ref
            torch.cuda.empty_cache()
        return out

    report = {'steps_over_h': list(mults), 'reference': 'midpoint rule at h/4', 'random': table_of('random', m, ds)}
    if args.skip_trained_steps > 0:
        ctx = bench.cfg3_train_setup(o.device, args.precision)
        for _ in range(args.skip_trained_steps):
            ctx['step']()
        tm = ctx['model'].eval()
        tm.precision = args.precision
        report['trained'] = dict(table_of('trained', tm, ctx['ds']), steps=args.skip_trained_steps)
    return report


if __name__ == '__main__':
    main()
