"""Time of one direct-volume-rendered frame of the cfg-3 synthetic model (visualization/Render.py):
a 1024^2 pinhole view of the 256^3 volume's box at the default step (half a voxel), without and with headlight shading.

    python tools/bench_render.py [--size 1024] [--frames 3] [--precision f16x2]          # on the GPU box

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
    table = np.stack([0.3 + 0.7 * v, 0.3 + 0.4 * v, 0.4 - 0.3 * v, 12.0 * np.clip(2.0 * v - 1.0, 0.0, 1.0)], 1)
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

    summary = {'size': args.size, 'step': step, 'precision': args.precision, 'opacity_limit': args.opacity_limit}
    for mode, fn in (('unshaded', plain), ('headlight', shaded)):
        kw = dict(opacity_limit=args.opacity_limit, shading=None if mode == 'unshaded' else 'headlight')
        stats = {}
        Render.render(fn, o, d, tf, step, box[0], box[1], stats=stats, **kw)             # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.frames):
            t0 = time.perf_counter()
            img = Render.render(fn, o, d, tf, step, box[0], box[1], **kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        # one instrumented frame: an event pair around every launch group
        spans = {'clip': [], 'samples': [], 'composite': [], 'compact': [], 'value_fn': []}
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

        def fn_kept(pos):
            kept.append(pos)
            return fn(pos)
        saved = (ops.ray_clip, ops.ray_samples, ops.ray_composite, ops.ray_compact)
        try:
            ops.ray_clip, ops.ray_samples = timed('clip', saved[0]), timed('samples', saved[1])
            ops.ray_composite, ops.ray_compact = timed('composite', saved[2]), timed('compact', saved[3])
            Render.render(timed('value_fn', fn_kept), o, d, tf, step, box[0], box[1], **kw)
        finally:
            ops.ray_clip, ops.ray_samples, ops.ray_composite, ops.ray_compact = saved
        torch.cuda.synchronize()
        gpu = {k: float(sum(a.elapsed_time(b) for a, b in v_)) for k, v_ in spans.items()}
        new = gpu['clip'] + gpu['samples'] + gpu['composite'] + gpu['compact']
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
        n = stats['samples']
        best = min(ms)
        print('[%s] %.1f ms per frame (best of %d: %s)' % (mode, best, len(ms), ' '.join('%.1f' % x for x in ms)))
        print('[%s] %d samples in %d blocks of 32 steps, %d launches: %.2f Gsamples/s over the frame' % (
            mode, n, stats['blocks'], len(kept), n / best / 1e6))
        print('[%s] live rays per block: %s' % (mode, ' '.join(str(x) for x in stats['live'])))
        print('[%s] GPU time of the instrumented frame: value_fn %.1f ms, ray kernels %.1f ms (clip %.2f, samples %.1f, '
              'composite %.1f, compact %.1f) = %.1f %% of value_fn' % (mode, gpu['value_fn'], new, gpu['clip'], gpu['samples'],
                                                                   gpu['composite'], gpu['compact'], 100.0 * new / gpu['value_fn']))
        print('[%s] ops.forward_raw alone on the same positions: %.1f ms = %.2f Gsamples/s' % (mode, fwd_ms, n / fwd_ms / 1e6))
        print('[%s] image: mean opacity %.3f, %d of %d rays hit' % (mode, float(img[:, 3].mean()), stats['live'][0] if stats['live'] else 0,
                                                                  o.shape[0]), flush=True)
        summary[mode] = {'frame_ms': ms, 'samples': n, 'blocks': stats['blocks'], 'live': stats['live'], 'gpu_ms': gpu,
                         'ray_kernels_ms': new, 'forward_alone_ms': fwd_ms}
        del kept, img
        torch.cuda.empty_cache()
    print(json.dumps(summary), flush=True)


if __name__ == '__main__':
    main()
