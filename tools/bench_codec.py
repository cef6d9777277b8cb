"""File sizes and store / restore times of the checkpoint codec with and without its entropy stage, and with the per-cell
mask (``channel_mask=True``) on top of it, for cfg-3- and cfg-5-shaped models (64^3 and 128^3 x 32 channels,
MLP 4 x 128).

    python tools/bench_codec.py [--cfg 3 5] [--keep 0.5 0.1 0.03] [--bits 4 8] [--repeats 2]
                                [--prune coefficient cell cell-smooth]                                # on the GPU box

THE COEFFICIENTS ARE SYNTHETIC: iid Laplace noise and an untrained MLP, pruned until the given fraction is kept --
  coefficient   the smallest coefficients by magnitude (over all tensors) set to zero: no pipeline of this project produces
                this pattern, it is the hardest case for the mask coder;
  cell          whole cells set to zero, the smallest by the magnitude of the cell's channel vector (over all tensors): what
                the drop layers do, which multiply a tensor (C, ...) by one factor per cell;
  cell-smooth   whole cells again, the kept ones where a smooth random field (low-pass filtered noise, per tensor) exceeds
                its quantile: a spatially clustered support.
A trained, pruned model has its own clustering and more peaked label histograms, so its gain is a number to measure on that
model, not to read off this table.

Per model: bytes of the plain, the entropy and the per-cell pair (parameter file + mask file), wall-clock seconds of
store_model_parameters and restore_model for each kind (synchronised, best of --repeats), the seconds the rANS encoder and
decoder alone take on the model's mask, and -- summed over the model's tensors -- the seconds of the four per-cell entries
beside codec_compact / codec_expand of the same tensors, and the rate of codec_support on the largest tensor alone (20
launches between two events).  Then one JSON summary line.  A tool, not a test, and nothing of
bench.py; no threshold.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GRID = {3: 64, 5: 128}
KINDS = {'plain': {}, 'entropy': {'entropy': True}, 'channel': {'entropy': True, 'channel_mask': True}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', type=int, nargs='+', default=[3, 5], choices=sorted(GRID))
    ap.add_argument('--keep', type=float, nargs='+', default=[0.5, 0.1, 0.03])
    ap.add_argument('--bits', type=int, nargs='+', default=[4, 8])
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--prune', nargs='+', default=['coefficient', 'cell', 'cell-smooth'],
                    choices=['coefficient', 'cell', 'cell-smooth'])
    args = ap.parse_args()

    import torch
    from latent_feature_grid_compression_amd import ops
    from latent_feature_grid_compression_amd.model.model_utils import restore_model, setup_model, store_model_parameters

    dev = torch.device('cuda:0')

    def best_of(fn):
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return out, min(times)

    def smooth_field(shape, gen):
        """Low-pass filtered noise over the last three extents of `shape`, one field per leading index."""
        noise = torch.randn(shape, generator=gen, device=dev)
        axes = [torch.fft.fftfreq(n, device=dev) for n in shape[-3:]]
        r2 = axes[0][:, None, None] ** 2 + axes[1][None, :, None] ** 2 + axes[2][None, None, :] ** 2
        return torch.fft.ifftn(torch.fft.fftn(noise, dim=(-3, -2, -1)) * torch.exp(-400.0 * r2), dim=(-3, -2, -1)).real

    def keep_masks(prune, dense, keep, gen):
        """One 0/1 tensor per coefficient tensor, broadcastable to it."""
        if prune == 'coefficient':
            mags = torch.cat([d.abs().reshape(-1) for d in dense])
            thr = torch.kthvalue(mags, max(1, int(round((1 - keep) * mags.numel()))))[0]
            return [(d.abs() > thr).float() for d in dense]
        if prune == 'cell':
            norms = [d.pow(2).sum(0, keepdim=True) for d in dense]
            flat = torch.cat([v.reshape(-1) for v in norms])
            thr = torch.kthvalue(flat, max(1, int(round((1 - keep) * flat.numel()))))[0]
            return [(v > thr).float() for v in norms]
        masks = []
        for d in dense:
            field = smooth_field(d.shape[1:], gen).unsqueeze(0)
            thr = torch.kthvalue(field.reshape(-1), max(1, int(round((1 - keep) * field.numel()))))[0]
            masks.append((field > thr).float())
        return masks

    def entry_times(m, C):
        """Seconds of the per-cell entries and of codec_compact / codec_expand, each summed over the model's tensors."""
        t = dict.fromkeys(['support', 'pack_flags', 'compact_support', 'expand_support', 'compact', 'expand'], 0.0)
        grids = [p.detach().reshape(-1) for p in m.feature_grid]
        flags = []
        for g in grids:
            f, dt = best_of(lambda: ops.codec_support(g, C))
            flags.append(f)
            t['support'] += dt
        support, t['pack_flags'] = best_of(lambda: ops.codec_pack_flags(torch.cat(flags)))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        offset = 0
        for g, f in zip(grids, flags):
            V, dt = best_of(lambda: ops.codec_compact_support(g, C, f))
            t['compact_support'] += dt
            back, dt = best_of(lambda: ops.codec_expand_support(support, offset, C, f.numel(), V, V.shape[1], status))
            t['expand_support'] += dt
            assert torch.equal(back == 0, g == 0), 'the per-cell entries did not reproduce the pruning pattern'
            offset += f.numel()
            nz, dt = best_of(lambda: ops.codec_compact(g))
            t['compact'] += dt
            mask = ops.codec_mask(g)
            _, dt = best_of(lambda: ops.codec_expand(mask, 0, g.numel(), nz))
            t['expand'] += dt
        assert int(status.item()) == 0
        # the pass that reads everything, on the largest tensor alone: 20 launches back to back between two events
        g = max(grids, key=lambda v: v.numel())
        ops.codec_support(g, C)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(20):
            ops.codec_support(g, C)
        end.record()
        torch.cuda.synchronize()
        t['support_largest'] = start.elapsed_time(end) / 20e3
        t['support_largest_GBs'] = g.numel() * 4 / t['support_largest'] / 1e9
        return t

    rows = []
    print('synthetic coefficients (iid Laplace; pruned per coefficient, per cell, or per cell of a smooth field), untrained MLP '
          '-- see the module docstring', flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for cfg in args.cfg:
            torch.manual_seed(100 + cfg)
            m = setup_model(3, 128, 1, 4, 'fourier', 2, '', 0.1, 0.9, 'db2', 32, GRID[cfg], '').to(dev)
            C = int(m.feature_grid[0].shape[0])
            gen = torch.Generator(device=dev).manual_seed(200 + cfg)
            dense = []
            for p in m.feature_grid:
                u = torch.rand(p.shape, generator=gen, device=dev) - 0.5
                dense.append(-torch.sign(u) * torch.log1p(-2 * u.abs()))
            n_coefficients = sum(d.numel() for d in dense)
            for prune in args.prune:
                for keep in args.keep:
                    with torch.no_grad():
                        for p, d, k in zip(m.feature_grid, dense, keep_masks(prune, dense, keep, gen)):
                            p.copy_(d * k)
                    mask = ops.codec_mask(torch.cat([p.detach().reshape(-1) for p in m.feature_grid]))
                    stream, t_enc = best_of(lambda: ops.codec_rans_encode(mask))
                    _, t_dec = best_of(lambda: ops.codec_rans_decode(stream))
                    entries = entry_times(m, C)
                    print('cfg %d, %s, %5.1f %% kept, entries over all tensors: %s' % (
                        cfg, prune, 100 * keep, ', '.join(('%s %.0f' if k.endswith('GBs') else '%s %.6f s') % (k, v)
                                                          for k, v in entries.items())), flush=True)
                    for bits in args.bits:
                        row = {'cfg': cfg, 'prune': prune, 'coefficients': int(n_coefficients), 'keep': keep, 'bits': bits,
                               'mask_bytes': int(mask.numel()), 'mask_stream_bytes': int(stream.numel()),
                               'mask_encode_s': t_enc, 'mask_decode_s': t_dec, 'entries_s': entries}
                        for kind, kwargs in KINDS.items():
                            path = os.path.join(tmp, 'cfg%d_%s' % (cfg, kind))
                            _, row[kind + '_store_s'] = best_of(lambda: store_model_parameters(m, path, bits, **kwargs))
                            back, row[kind + '_restore_s'] = best_of(lambda: restore_model(path))
                            for a, b in zip(m.feature_grid, back.feature_grid):
                                assert torch.equal(a == 0, b == 0), 'the pruning pattern did not survive'
                            row[kind + '_param_bytes'] = os.path.getsize(path)
                            row[kind + '_mask_bytes'] = os.path.getsize(path + '_mask.bnr')
                            row[kind + '_bytes'] = row[kind + '_param_bytes'] + row[kind + '_mask_bytes']
                            with open(path + '_mask.bnr', 'rb') as f:
                                row[kind + '_mask_mode'] = f.read(1)[0] if kind != 'plain' else None
                        row['ratio'] = row['entropy_bytes'] / row['plain_bytes']
                        row['channel_ratio'] = row['channel_bytes'] / row['plain_bytes']
                        rows.append(row)
                        print('cfg %d, %5.1f %% kept, %d bits: plain %11d B (mask %9d), entropy %11d B (mask %9d), ratio %.3f '
                              '| store %.3f -> %.3f s, restore %.3f -> %.3f s | mask alone: encode %.4f s, decode %.4f s'
                              % (cfg, 100 * keep, bits, row['plain_bytes'], row['plain_mask_bytes'], row['entropy_bytes'],
                                 row['entropy_mask_bytes'], row['ratio'], row['plain_store_s'], row['entropy_store_s'],
                                 row['plain_restore_s'], row['entropy_restore_s'], t_enc, t_dec), flush=True)
                        print('    %s-pruned, channel_mask=True: %11d B (mask %9d, mode %d), ratio %.3f | store %.3f s, restore %.3f s'
                              % (prune, row['channel_bytes'], row['channel_mask_bytes'], row['channel_mask_mode'],
                                 row['channel_ratio'], row['channel_store_s'], row['channel_restore_s']), flush=True)
                        for kind in KINDS:
                            os.remove(os.path.join(tmp, 'cfg%d_%s' % (cfg, kind)))
                            os.remove(os.path.join(tmp, 'cfg%d_%s_mask.bnr' % (cfg, kind)))
            del m, dense
            torch.cuda.empty_cache()
    print(json.dumps({'synthetic': True, 'rows': rows}))


if __name__ == '__main__':
    main()
