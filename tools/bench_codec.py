"""File sizes and store / restore times of the checkpoint codec with and without its entropy stage, for
cfg-3- and cfg-5-shaped models (64^3 and 128^3 x 32 channels, MLP 4 x 128).

    python tools/bench_codec.py [--cfg 3 5] [--keep 0.5 0.1 0.03] [--bits 4 8] [--repeats 2]          # on the GPU box

THE COEFFICIENTS ARE SYNTHETIC: iid Laplace noise, the smallest by magnitude (over all tensors) set to zero until the given
fraction is kept, and an untrained MLP.  A trained, pruned model has spatially clustered masks and more peaked label
histograms, so its gain is a number to measure on that model, not to read off this table.

Per model: bytes of the plain and of the entropy pair (parameter file + mask file), their ratio,
wall-clock seconds of store_model_parameters and restore_model for both kinds (synchronised, best of --repeats), and the
seconds the rANS encoder and decoder alone take on the model's mask.  Then one JSON summary line.  A tool, not a test, and
nothing of bench.py; no threshold.
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', type=int, nargs='+', default=[3, 5], choices=sorted(GRID))
    ap.add_argument('--keep', type=float, nargs='+', default=[0.5, 0.1, 0.03])
    ap.add_argument('--bits', type=int, nargs='+', default=[4, 8])
    ap.add_argument('--repeats', type=int, default=2)
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

    rows = []
    print('synthetic coefficients (iid Laplace, magnitude-pruned), untrained MLP -- see the module docstring', flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for cfg in args.cfg:
            torch.manual_seed(100 + cfg)
            m = setup_model(3, 128, 1, 4, 'fourier', 2, '', 0.1, 0.9, 'db2', 32, GRID[cfg], '').to(dev)
            gen = torch.Generator(device=dev).manual_seed(200 + cfg)
            dense = []
            for p in m.feature_grid:
                u = torch.rand(p.shape, generator=gen, device=dev) - 0.5
                dense.append(-torch.sign(u) * torch.log1p(-2 * u.abs()))
            mags = torch.cat([d.abs().reshape(-1) for d in dense])
            for keep in args.keep:
                thr = torch.kthvalue(mags, max(1, int(round((1 - keep) * mags.numel()))))[0]
                with torch.no_grad():
                    for p, d in zip(m.feature_grid, dense):
                        p.copy_(d * (d.abs() > thr).float())
                mask = ops.codec_mask(torch.cat([p.detach().reshape(-1) for p in m.feature_grid]))
                stream, t_enc = best_of(lambda: ops.codec_rans_encode(mask))
                _, t_dec = best_of(lambda: ops.codec_rans_decode(stream))
                for bits in args.bits:
                    row = {'cfg': cfg, 'coefficients': int(mags.numel()), 'keep': keep, 'bits': bits,
                           'mask_bytes': int(mask.numel()), 'mask_stream_bytes': int(stream.numel()),
                           'mask_encode_s': t_enc, 'mask_decode_s': t_dec}
                    for kind in ('plain', 'entropy'):
                        path = os.path.join(tmp, 'cfg%d_%s' % (cfg, kind))
                        _, row[kind + '_store_s'] = best_of(lambda: store_model_parameters(m, path, bits, entropy=kind == 'entropy'))
                        back, row[kind + '_restore_s'] = best_of(lambda: restore_model(path))
                        for a, b in zip(m.feature_grid, back.feature_grid):
                            assert torch.equal(a == 0, b == 0), 'the pruning pattern did not survive'
                        row[kind + '_param_bytes'] = os.path.getsize(path)
                        row[kind + '_mask_bytes'] = os.path.getsize(path + '_mask.bnr')
                        row[kind + '_bytes'] = row[kind + '_param_bytes'] + row[kind + '_mask_bytes']
                    row['ratio'] = row['entropy_bytes'] / row['plain_bytes']
                    rows.append(row)
                    print('cfg %d, %5.1f %% kept, %d bits: plain %11d B (mask %9d), entropy %11d B (mask %9d), ratio %.3f '
                          '| store %.3f -> %.3f s, restore %.3f -> %.3f s | mask alone: encode %.4f s, decode %.4f s'
                          % (cfg, 100 * keep, bits, row['plain_bytes'], row['plain_mask_bytes'], row['entropy_bytes'],
                             row['entropy_mask_bytes'], row['ratio'], row['plain_store_s'], row['entropy_store_s'],
                             row['plain_restore_s'], row['entropy_restore_s'], t_enc, t_dec), flush=True)
                    for kind in ('plain', 'entropy'):
                        os.remove(os.path.join(tmp, 'cfg%d_%s' % (cfg, kind)))
                        os.remove(os.path.join(tmp, 'cfg%d_%s_mask.bnr' % (cfg, kind)))
            del m, dense, mags
            torch.cuda.empty_cache()
    print(json.dumps({'synthetic': True, 'rows': rows}))


if __name__ == '__main__':
    main()
