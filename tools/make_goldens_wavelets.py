"""Generate the wavelet-basis fixtures tests/golden/wavelets_*.npz / wavelets_levels.json from the REFERENCE's own
Python modules (build container only).

    python tools/make_goldens_wavelets.py

Same approach as tools/make_goldens.py (the reference is imported, never copied), with a ``pywt`` stand-in of its own
that serves what the other filter lengths need:
  * ``Wavelet('haar')`` / ``Wavelet('db1')``: PyWavelets' Haar bank (+-1/sqrt(2));
  * ``Wavelet(name, filter_bank=...)`` objects carrying fixed, seeded test banks of length 6 and 8 (the reference
    accepts pywt.Wavelet instances, Torch_Wavelet_Transform.py:11-14, and its ops do not need an orthogonal bank);
  * ``dwt_max_level`` by PyWavelets' rule floor(log2(n / (L - 1))) (0 when n < L - 1).
tools/_ref_standins.py and the db2 fixtures are left as they are.
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.normpath(os.path.join(HERE, '..', 'tests', 'golden'))

if not os.path.isdir(REF):
    sys.exit('tools/make_goldens_wavelets.py needs the reference checkout at /root/reference (build container only)')

S = 0.7071067811865476
HAAR_BANK = [[S, S], [-S, S], [S, S], [S, -S]]     # pywt 'haar' / 'db1': dec_lo, dec_hi, rec_lo, rec_hi


def test_bank(L):
    """Seeded, non-orthogonal bank of length L (dec_lo, dec_hi, rec_lo, rec_hi), taps in [-1, 1]."""
    rng = np.random.Generator(np.random.PCG64(600 + L))
    return [[float(v) for v in rng.uniform(-1.0, 1.0, L)] for _ in range(4)]


class _Wavelet:
    def __init__(self, name, filter_bank=None):
        if filter_bank is None:
            assert name in ('haar', 'db1'), name
            filter_bank = HAAR_BANK
        self.name = name
        self.filter_bank = tuple(list(x) for x in filter_bank)
        self.dec_len = len(self.filter_bank[0])


def _dwt_max_level(data_len, filter_len):
    flen = filter_len.dec_len if isinstance(filter_len, _Wavelet) else int(filter_len)
    if data_len < flen - 1:
        return 0
    return int(math.floor(math.log2(data_len / (flen - 1))))


pywt_mod = types.ModuleType('pywt')
pywt_mod.Wavelet = _Wavelet
pywt_mod.dwt_max_level = _dwt_max_level
sys.modules['pywt'] = pywt_mod
pyevtk_mod = types.ModuleType('pyevtk')
pyevtk_hl = types.ModuleType('pyevtk.hl')
pyevtk_hl.imageToVTK = lambda *a, **k: None
pyevtk_mod.hl = pyevtk_hl
sys.modules['pyevtk'] = pyevtk_mod
sys.modules['pyevtk.hl'] = pyevtk_hl

sys.path.insert(0, REF)
from model.model_utils import setup_model                       # noqa: E402
from model.Feature_Grid_Model import Feature_Grid_Model         # noqa: E402
from model.Feature_Embedding import FourierEmbedding            # noqa: E402
from wavelet_transform.Torch_Wavelet_Transform import WaveletFilter3d   # noqa: E402

torch.set_num_threads(4)


def rng_for(seed):
    return np.random.Generator(np.random.PCG64(seed))


def wavelet(L):
    return 'haar' if L == 2 else _Wavelet('test%d' % L, test_bank(L))


def special_positions(rng, n_random, G):
    """Cube corners, points on every face, cell centres / boundaries, random interior."""
    pts = [[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]
    for a in range(3):
        for s in (-1.0, 1.0):
            for _ in range(4):
                p = rng.uniform(-1, 1, 3)
                p[a] = s
                pts.append(p.tolist())
    for k in (0, 1, G // 2, G - 1):
        c = (2.0 * k + 1.0) / G - 1.0
        pts.append([c, -c, 0.123])
        pts.append([2.0 * k / G - 1.0, 0.3, -0.7])
    pts = np.asarray(pts, np.float32)
    return torch.from_numpy(np.concatenate([pts, rng.uniform(-1, 1, (n_random, 3)).astype(np.float32)], 0))


def gen_filters_and_levels():
    out = {}
    for L in (2, 6, 8):
        f = WaveletFilter3d(wavelet(L))
        out['bank_%d' % L] = np.asarray(wavelet(L).filter_bank if L != 2 else HAAR_BANK, np.float64)
        out['filter_fwd_%d' % L] = f.filter_fwd.numpy()
        out['filter_rev_%d' % L] = f.filter_rev.numpy()
    np.savez_compressed(os.path.join(GOLD, 'wavelets_filters.npz'), **out)
    table = {}
    emb = FourierEmbedding(2, 3)
    for L in (2, 6, 8):
        filt = WaveletFilter3d(wavelet(L))
        for G in (8, 15, 16, 17, 32, 64):
            m = Feature_Grid_Model(emb, torch.zeros(1, G, G, G), None, filt, hidden_channel=4, num_layer=1)
            table['L%d_G%d' % (L, G)] = {'num_levels': int(len(m.shape_array)),
                                         'shape_array': np.asarray(m.shape_array).tolist(),
                                         'coeff_shapes': [list(p.shape) for p in m.feature_grid]}
    with open(os.path.join(GOLD, 'wavelets_levels.json'), 'w') as f:
        json.dump(table, f, indent=1)


def gen_roundtrips():
    emb = FourierEmbedding(2, 3)
    for L in (2, 6, 8):
        filt = WaveletFilter3d(wavelet(L))
        out = {}
        for G in (15, 16, 17):
            rng = rng_for(700 + 10 * L + G)
            grid = torch.from_numpy(rng.random((2, G, G, G), dtype=np.float32))
            m = Feature_Grid_Model(emb, grid, None, filt, hidden_channel=4, num_layer=1)
            out['G%d.input' % G] = grid.numpy()
            out['G%d.shape_array' % G] = np.asarray(m.shape_array)
            out['G%d.decoded' % G] = m.decode_volume().detach().numpy()
            out['G%d.n' % G] = np.asarray(len(m.feature_grid))
            for i, p in enumerate(m.feature_grid):
                out['G%d.coeff%d' % (G, i)] = p.detach().numpy()
        # non-cubic single level through the filter directly (odd/even mix; pins the pad-slot quirk)
        rng = rng_for(790 + L)
        data = torch.from_numpy(rng.random((1, 2, 9, 12, 7), dtype=np.float32))
        coeffs, shape = filt.encode(data)
        out.update(nc_input=data.numpy(), nc_coeffs=coeffs.numpy(), nc_shape=np.asarray(shape),
                   nc_decoded=filt.decode(coeffs, shape).numpy())
        np.savez_compressed(os.path.join(GOLD, 'wavelets_roundtrip_L%d.npz' % L), **out)


def seeded_model(drop_type, C, G, H, NL, seed):
    model = setup_model(3, H, 1, NL, 'fourier', 2, drop_type, 0.025, 0.75, 'haar', C, G, '')
    rng = rng_for(seed)
    grid = torch.from_numpy(rng.random((C, G, G, G), dtype=np.float32))
    feats, _ = model.encode_volume(grid)
    with torch.no_grad():
        for p, f in zip(model.feature_grid, feats):
            p.copy_(f)
        for lin in list(model.net_layers) + [model.final_layer]:
            bound = 1.0 / np.sqrt(lin.in_features)
            lin.weight.copy_(torch.from_numpy(rng.uniform(-bound, bound, lin.weight.shape).astype(np.float32)))
            lin.bias.copy_(torch.from_numpy(rng.uniform(-bound, bound, lin.bias.shape).astype(np.float32)))
        if drop_type:
            for layer in model.drop:
                layer.betas.copy_(torch.from_numpy(rng.uniform(0.2, 1.5, layer.betas.shape).astype(np.float32)))
    return model, rng


def fwd_bwd(model, rng, G, n_random):
    model.train()
    pos = special_positions(rng, n_random, G)
    pos_req = pos.clone().requires_grad_(True)
    y = model(pos_req)
    target = torch.from_numpy(rng.uniform(-1, 1, (pos.shape[0],)).astype(np.float32))
    loss = torch.nn.functional.mse_loss(y.squeeze(-1), target)
    model.zero_grad()
    loss.backward()
    out = {'sd.' + k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    out.update(shape_array=np.asarray(model.shape_array), pos=pos.numpy(), y=y.detach().numpy(),
               target=target.numpy(), loss=np.asarray(loss.item(), np.float64), grad_pos=pos_req.grad.numpy(),
               decoded=model.decode_volume().detach().numpy())
    for k, p in model.named_parameters():
        if p.grad is not None:
            out['grad.' + k] = p.grad.numpy()
    return out


def gen_models():
    C, G, H, NL = 4, 16, 16, 3
    model, rng = seeded_model('', C, G, H, NL, 2101)
    out = fwd_bwd(model, rng, G, 300)
    out['meta'] = np.asarray([C, G, H, NL, 2])
    np.savez_compressed(os.path.join(GOLD, 'wavelets_haar_model.npz'), **out)
    model, rng = seeded_model('smallify', C, G, H, NL, 2102)
    out = fwd_bwd(model, rng, G, 300)
    out['meta'] = np.asarray([C, G, H, NL, 2])
    np.savez_compressed(os.path.join(GOLD, 'wavelets_haar_smallify.npz'), **out)


if __name__ == '__main__':
    gen_filters_and_levels()
    gen_roundtrips()
    gen_models()
    for f in sorted(os.listdir(GOLD)):
        if f.startswith('wavelets_'):
            print('%-36s %8d bytes' % (f, os.path.getsize(os.path.join(GOLD, f))))
