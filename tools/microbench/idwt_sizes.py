"""Last wavelet level in isolation at cfg 3 (d=33 -> 64) and cfg 5 (d=65 -> 128), C=32: the channel-first level kernels,
the layout conversions, and the fused channel-last level kernels that replace each pair; db2, then the Haar level of the
same output size (d=32 -> 64, d=64 -> 128: the same bytes, an eighth of the FMAs).  Then the same level with the drop
layers' factors folded in (DROP): the channel-first DROP kernels and the channel-last DROP builds that replace them plus
the conversion.  MB = coefficient + grid bytes (each touched once); the two-kernel form moves the grid three times; the
DROP synthesis reads 7 d^3 factors on top (1 / C of the coefficient bytes), the DROP adjoint reads the coefficients again
(as many bytes as it writes) and the factors.

    python tools/microbench/idwt_sizes.py [--repeats N]     (default 3; the rows are measured round-robin, N times)

Prints median us with [min .. max] over the repeats."""
import sys, os, statistics, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from latent_feature_grid_compression_amd import ops
from latent_feature_grid_compression_amd.wavelet_transform.Torch_Wavelet_Transform import WaveletFilter3d
dev = torch.device('cuda:0')
filters = {w: WaveletFilter3d(w).filter_rev.to(dev) for w in ('db2', 'haar')}
repeats = int(sys.argv[sys.argv.index('--repeats') + 1]) if '--repeats' in sys.argv else 3


def timed(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for wav, C, d, t in (('db2', 32, 33, 64), ('db2', 32, 65, 128), ('haar', 32, 32, 64), ('haar', 32, 64, 128)):
    frev = filters[wav]
    lll = torch.randn(C, d, d, d, device=dev); hf = torch.randn(C, 7, d, d, d, device=dev); g = torch.randn(C, t, t, t, device=dev)
    mh = torch.rand(7, d, d, d, device=dev) * 0.95 + 0.05        # the last level of a multi-level model: detail factor only
    zero = torch.zeros(7, d, d, d, device=dev)                   # the caller's zero fill is not timed (shared by all levels)
    g_cl = ops.to_channel_last(g)
    mb = 4 * C * (8 * d ** 3 + t ** 3) / 1e6
    mb_f = mb + 4 * 7 * d ** 3 / 1e6                             # + factors
    mb_a = mb + 4 * (C + 2) * 7 * d ** 3 / 1e6                   # + coefficients again, factors, factor gradient
    rows = (('synthesis (channel-first)', mb, lambda: ops.idwt_level(lll, hf, frev, (t, t, t))),
            ('to_channel_last', mb, lambda: ops.to_channel_last(g)),
            ('synthesis channel-last', mb, lambda: ops.idwt_level_cl(lll, hf, frev, (t, t, t))),
            ('adjoint (channel-first)', mb, lambda: ops.idwt_level_bwd(g, frev, (d, d, d))),
            ('to_channel_first', mb, lambda: ops.to_channel_first(g_cl, C)),
            ('adjoint channel-last', mb, lambda: ops.idwt_level_cl_bwd(g_cl, C, frev, (d, d, d))),
            ('DROP synthesis (channel-first)', mb_f, lambda: ops.idwt_level_drop(lll, hf, None, None, mh, None, frev, (t, t, t))),
            ('DROP synthesis channel-last', mb_f, lambda: ops.idwt_level_cl_drop(lll, hf, None, None, mh, None, frev, (t, t, t))),
            ('DROP adjoint (channel-first)', mb_a, lambda: ops.idwt_level_drop_bwd(g, frev, None, hf, None, mh, False, zero, (d, d, d))),
            ('DROP adjoint channel-last', mb_a, lambda: ops.idwt_level_cl_drop_bwd(g_cl, C, frev, None, hf, None, mh, False, zero, (d, d, d))))
    us = {name: [] for name, _, _ in rows}
    for _ in range(repeats):
        for name, _, fn in rows:
            us[name].append(timed(fn))
    for name, m, _ in rows:
        med = statistics.median(us[name])
        print('%-4s d=%d %-31s %8.1f us [%7.1f .. %7.1f]  %6.1f MB  %5.2f TB/s' % (wav, d, name, med, min(us[name]), max(us[name]), m, m / med))
    med = lambda k: statistics.median(us[k])
    print('%-4s d=%d DROP channel-last / (DROP channel-first + layout pass): synthesis %.2f, adjoint %.2f' % (
        wav, d, med('DROP synthesis channel-last') / (med('DROP synthesis (channel-first)') + med('to_channel_last')),
        med('DROP adjoint channel-last') / (med('DROP adjoint (channel-first)') + med('to_channel_first'))))
    print('%-4s d=%d DROP / plain channel-last: synthesis time x%.3f (bytes x%.3f), adjoint time x%.3f (bytes x%.3f)' % (
        wav, d, med('DROP synthesis channel-last') / med('synthesis channel-last'), mb_f / mb,
        med('DROP adjoint channel-last') / med('adjoint channel-last'), mb_a / mb))
