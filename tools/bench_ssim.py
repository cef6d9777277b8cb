"""Time and memory of the SSIM kernel beside the torch composition it replaces, on one GPU in one run.

    python tools/bench_ssim.py [--edge 256] [--train-steps 50] [--reps 5] [--rounds 5] [--precision f16x2]

The pair is the cfg-3 model's eval-mode reconstruction of bench.py's smooth synthetic volume (edge^3) and that volume.  Three
settings: a uniform window of 7 at stride 1, the same at stride 2, a Gaussian window of 11 at stride 1.  Per setting

  kernel   ops.ssim_plane_sums on the resident pair (one call: plane sums, no map)
  torch    the composition: the five fields x, y, xx, yy, xy in fp64, each filtered by three separable conv3d passes, the
           formula on the results, .mean().  Where the build has no fp64 conv3d the passes are sums of shifted strided slices
           (the tool says which it used).

alternate for --rounds rounds after one warm-up each, --reps calls between two device events per round; the median is
reported with the range.  Peak memory is torch's allocator peak above the resident pair during one call of each.  The two
means are compared.  Then one field_from_net_fused of the same volume for scale, and Similarity.ssim_from_net and
volume_ssim end to end (wall clock, synchronised).  Ends with one JSON line.  A tool, not a test, and nothing of bench.py;
no threshold.
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
    ap.add_argument('--edge', type=int, default=256)
    ap.add_argument('--train-steps', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5, help='calls between the two events of one timing')
    ap.add_argument('--rounds', type=int, default=5, help='timings per contender, the two alternating')
    ap.add_argument('--precision', default='f16x2', choices=['f16x2', 'fp32', 'f16'])
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import bench
    from latent_feature_grid_compression_amd import ops
    from latent_feature_grid_compression_amd.visualization import OutputToVTK as V
    from latent_feature_grid_compression_amd.visualization import Similarity as S

    dev = torch.device('cuda:0')
    shape = (args.edge,) * 3
    ctx = bench.cfg3_train_setup(dev, args.precision, vol_shape=shape)
    for _ in range(args.train_steps):
        ctx['step']()
    model, vol, ds = ctx['model'].eval(), ctx['vol'], ctx['ds']
    model.precision = args.precision
    with torch.no_grad():
        pred = V.field_from_net_fused(ds, model).contiguous()
    L = float(vol.max()) - float(vol.min())
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    print('[pair] %d^3, cfg 3 after %d train steps, data range %.4f, PSNR %.2f dB'
          % (args.edge, args.train_steps, L, float(V.calculate_deviation_statistics(pred, vol, verbose=False)[0])), flush=True)

    def event_ms(fn, reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / reps

    def peak_mb(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize()
        return out, (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20

    def conv_pass(f, g, s, axis):
        view, stride = [1, 1, 1, 1, 1], [1, 1, 1]
        view[2 + axis], stride[axis] = -1, s
        return F.conv3d(f, g.view(view), stride=tuple(stride))

    def slice_pass(f, g, s, axis):
        m = (f.shape[2 + axis] - g.numel()) // s + 1
        out = None
        for t in range(g.numel()):
            term = f.narrow(2 + axis, t, (m - 1) * s + 1)
            term = term[(slice(None),) * (2 + axis) + (slice(None, None, s),)] * g[t]
            out = term if out is None else out + term
        return out

    one_pass = conv_pass
    try:
        conv_pass(torch.zeros(1, 1, 8, 8, 8, dtype=torch.float64, device=dev), torch.ones(3, dtype=torch.float64, device=dev), 1, 0)
        torch.cuda.synchronize()
    except RuntimeError as e:
        print('[torch] no fp64 conv3d in this build (%s): the passes are sums of shifted slices' % str(e).splitlines()[0], flush=True)
        one_pass = slice_pass
    composition = 'conv3d' if one_pass is conv_pass else 'slices'

    def torch_ssim(g, s):
        x, y = pred.double()[None, None], vol.double()[None, None]

        def filt(f):
            for axis in (2, 1, 0):
                f = one_pass(f, g, s, axis)
            return f
        mx, my, xx, yy, xy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
        vx, vy, vxy = xx - mx * mx, yy - my * my, xy - mx * my
        return (((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))).mean()

    rows = []
    for name, w, s, gaussian in (('uniform 7, stride 1', 7, 1, False), ('uniform 7, stride 2', 7, 2, False),
                                 ('Gaussian 11, stride 1', 11, 1, True)):
        g_host = S.ssim_weights(w, gaussian, 1.5)
        g_dev = torch.from_numpy(g_host).to(dev)
        weights, strides = [g_host] * 3, (s, s, s)
        windows = 1
        for m in ops.ssim_window_counts(shape, (w, w, w), strides):
            windows *= m
        contenders = (('kernel', lambda: ops.ssim_plane_sums(pred, vol, weights, strides, c1, c2)[0]),
                      ('torch', lambda: torch_ssim(g_dev, s)))
        row = {'setting': name, 'windows': windows, 'composition': composition}
        means = {}
        for who, fn in contenders:                               # warm-up and peak memory, one call each
            out, row[who + '_peak_MB'] = peak_mb(fn)
            means[who] = S._fold(out, windows) if who == 'kernel' else float(out)
        times = {who: [] for who, _ in contenders}
        for _ in range(args.rounds):                             # the two alternate, so that a drift of the clock hits both
            for who, fn in contenders:
                times[who].append(event_ms(fn, args.reps))
        for who, _ in contenders:
            t = sorted(times[who])
            row[who + '_ms'], row[who + '_ms_range'] = t[len(t) // 2], (t[0], t[-1])
        row['mean_kernel'], row['mean_torch'] = means['kernel'], means['torch']
        rows.append(row)
        print('[%s] %d windows | kernel %.3f ms (%.3f - %.3f), peak %.1f MB | torch (%s) %.3f ms (%.3f - %.3f), peak %.1f MB | '
              'mean SSIM %.12f against %.12f, difference %.1e'
              % (name, windows, row['kernel_ms'], *row['kernel_ms_range'], row['kernel_peak_MB'], composition, row['torch_ms'],
                 *row['torch_ms_range'], row['torch_peak_MB'], means['kernel'], means['torch'], abs(means['kernel'] - means['torch'])),
              flush=True)
        torch.cuda.empty_cache()

    with torch.no_grad():
        fwd = sorted(event_ms(lambda: V.field_from_net_fused(ds, model), args.reps) for _ in range(args.rounds))
    print('[scale] one field_from_net_fused of the volume: %.3f ms (%.3f - %.3f)' % (fwd[len(fwd) // 2], fwd[0], fwd[-1]), flush=True)

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    end_to_end = {}
    for who, fn in (('volume_ssim', lambda: S.volume_ssim(pred, vol)), ('ssim_from_net', lambda: S.ssim_from_net(ds, model, vol)),
                    ('ssim_from_net, 2^22-voxel slabs', lambda: S.ssim_from_net(ds, model, vol, max_slab_voxels=1 << 22))):
        (value, end_to_end[who]), peak = peak_mb(lambda fn=fn: wall(fn))
        print('[end to end] %s: %.12f in %.2f ms wall clock, peak %.1f MB above the resident pair' % (who, value, end_to_end[who], peak),
              flush=True)
    print(json.dumps({'edge': args.edge, 'train_steps': args.train_steps, 'rows': rows, 'field_from_net_fused_ms': fwd[len(fwd) // 2],
                      'end_to_end_ms': end_to_end}))


if __name__ == '__main__':
    main()
