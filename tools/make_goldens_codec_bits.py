"""Recorded results for the codec's other label widths (tests/test_hip_codec_bits.py), produced by the REFERENCE's own
``kmeans_quantization`` (model/model_utils.py:73-76: scikit-learn KMeans(n_clusters=2^bits, n_init=4)) in the build
container:

    python tools/make_goldens_codec_bits.py        -> tests/golden/codec_bits_mse.json

Two inputs: the non-zero values of ``sd.feature_grid.2`` of tests/golden/codec_small.npz, and a Laplace tensor the test
regenerates from its seed.  Stored: the mean squared error (fp64) of the reference's codebook per label width -- recorded
results only.  The reference's clustering is unseeded; numpy's global seed is fixed here, and the test allows the same
margin as tests/test_hip_codec.py::test_store_writes_the_reference_format.  Widths 14 and 16 are not recorded:
scikit-learn does not finish k = 16 384 on 50 000 points in useful time.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_standins                                            # noqa: E402

_ref_standins.install()
GOLD = _ref_standins.GOLD

from model.model_utils import kmeans_quantization               # noqa: E402

BITS = (2, 4, 6, 10, 12)
LAPLACE_SEED, LAPLACE_SCALE, LAPLACE_N = 7, 0.05, 50000


def inputs():
    g = np.load(os.path.join(GOLD, 'codec_small.npz'))
    grid = g['sd.feature_grid.2'].reshape(-1)
    return {'codec_small.feature_grid.2': grid[grid != 0].astype(np.float32),
            'laplace': np.random.default_rng(LAPLACE_SEED).laplace(0, LAPLACE_SCALE, LAPLACE_N).astype(np.float32)}


def main():
    out = {'bits': list(BITS), 'laplace': {'seed': LAPLACE_SEED, 'scale': LAPLACE_SCALE, 'n': LAPLACE_N}, 'n': {}, 'mse': {}}
    for name, x in inputs().items():
        out['n'][name] = int(x.size)
        out['mse'][name] = {}
        for bits in BITS:
            np.random.seed(9001 + bits)
            labels, centres = kmeans_quantization(x.reshape(-1, 1), 1 << bits)
            rec = np.asarray(centres, dtype=np.float32)[np.asarray(labels)]
            mse = float(np.mean((rec.astype(np.float64) - x.astype(np.float64)) ** 2))
            out['mse'][name][str(bits)] = mse
            print(name, x.size, 'bits', bits, 'mse', mse, flush=True)
    with open(os.path.join(GOLD, 'codec_bits_mse.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
