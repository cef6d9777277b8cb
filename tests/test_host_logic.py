"""CPU tests: the C-ABI library loads and exports every symbol include/lfgc.h declares (no compute calls
without a GPU), the host-side mirror of the reference interface (constructor, attribute names, state_dict
keys/shapes/order, filter buffers, shape arrays) matches the reference fixtures, the HIP path refuses CPU
tensors, and the multi-rank reconstruction driver (slab partition + one all-gather) is exercised with
world_size 2 over gloo."""
import ctypes
import json
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def built_lib():
    from latent_feature_grid_compression_amd.build import build
    return build(verbose=False)


def test_library_exports_every_declared_symbol(built_lib):
    header = open(os.path.join(ROOT, 'include', 'lfgc.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(lfgc_[a-z0-9_]+)\s*\(', header))
    assert len(declared) >= 15
    lib = ctypes.CDLL(built_lib)
    for name in sorted(declared):
        assert hasattr(lib, name), 'liblfgc.so does not export %s' % name
    from latent_feature_grid_compression_amd import _lib
    assert set(_lib.SIGNATURES) == declared          # the ctypes binding covers the whole header
    lib.lfgc_version.restype = ctypes.c_int
    assert lib.lfgc_version() == 100


def test_pure_host_entry_points(built_lib):
    """Entry points that touch no device: plan sizes, support matrix, error strings, argument validation."""
    from latent_feature_grid_compression_amd import _lib
    lib = _lib.load()
    ok = _lib.MlpDesc(32, 128, 4, 2, 3, 1)
    assert lib.lfgc_mlp_supported(ctypes.byref(ok)) == 1
    for bad in (_lib.MlpDesc(64, 128, 4, 2, 3, 1), _lib.MlpDesc(32, 256, 4, 2, 3, 1), _lib.MlpDesc(32, 128, 9, 2, 3, 1),
                _lib.MlpDesc(32, 128, 4, 3, 3, 1), _lib.MlpDesc(32, 128, 4, 2, 2, 1), _lib.MlpDesc(32, 128, 4, 2, 3, 2)):
        assert lib.lfgc_mlp_supported(ctypes.byref(bad)) == 0
        assert lib.lfgc_packed_bytes(ctypes.byref(bad)) == -3
    assert lib.lfgc_grid_channel_stride(22) == 24 and lib.lfgc_grid_channel_stride(32) == 32
    # packed blob: forward blocks + final + transposed blocks (csrc/lfgc_common.h)
    HP, K0P, K0R, L = 128, 48, 64, 4
    fwd = HP * (K0P + 4) + HP + (L - 1) * (HP * (HP + 4) + HP) + HP + 4
    tr = K0R * (HP + 4) + (L - 1) * HP * (HP + 4)
    h16 = 32 + 8 * HP + HP + HP * (48 + 4) + HP + (L - 1) * (HP * (HP + 4) + HP)   # 2 x 16 scales + biases / pi + scaled head weights + f16-split blocks (K0P16 = 48)
    assert lib.lfgc_packed_bytes(ctypes.byref(ok)) == 4 * (fwd + tr + h16 + tr)     # + f16-split transposed images
    # stash: whole workgroup batches of 8 x 32 samples, 64 lanes x (KS0 + L*16*MT) floats per tile
    assert lib.lfgc_stash_bytes(ctypes.byref(ok), 1) == 4 * 8 * 64 * (24 + 4 * 64)
    assert lib.lfgc_stash_bytes(ctypes.byref(ok), 32768) == 4 * 1024 * 64 * (24 + 4 * 64)
    assert lib.lfgc_backward_workspace_bytes(ctypes.byref(ok), 0) >= 0
    assert lib.lfgc_error_string(0) == b'ok'
    assert b'NULL' in lib.lfgc_error_string(-1)
    # NULL / shape errors are reported before anything is launched
    assert lib.lfgc_idwt_level_f32(None, None, None, None, None, 1, 1, 1, 1, 1, 1, 1, None) == -1
    assert lib.lfgc_penalty_sums_f32(None, 0, None, None) == -1 and lib.lfgc_drop_apply_f32(None, None, 0.0, None, 1, 1, None) == -1
    assert lib.lfgc_forward_f32(ctypes.byref(ok), None, None, 1, 1, 1, None, 0, 0, None, None, None, None) == -1
    assert lib.lfgc_gt_interp_f32(None, None, None, None, None, 0, 1, 1, 1, None, None) == -1
    # channel-last level: NULL, then the shapes it hands back to the two-kernel form (-3) -- dense stencil (no taps),
    # a channel stride that is not C rounded up to 8 (-2), arrays of 2^30 bytes and more
    taps = (ctypes.c_float * 8)(*[0.5] * 8)
    one = ctypes.c_void_p(16)                            # any non-NULL address: nothing is launched on these paths
    assert lib.lfgc_idwt_level_cl_f32(None, None, taps, None, 1, 8, 1, 1, 1, 1, 1, 1, None) == -1
    assert lib.lfgc_idwt_level_cl_f32(one, one, None, one, 4, 8, 3, 3, 3, 6, 6, 6, None) == -3
    assert lib.lfgc_idwt_level_cl_f32(one, one, taps, one, 4, 16, 3, 3, 3, 6, 6, 6, None) == -2
    assert lib.lfgc_idwt_level_cl_f32(one, one, taps, one, 32, 32, 200, 200, 200, 400, 400, 400, None) == -3
    assert lib.lfgc_idwt_level_cl_bwd_f32(one, None, one, one, 4, 8, 3, 3, 3, 6, 6, 6, None) == -3
    assert lib.lfgc_idwt_level_cl_bwd_f32(one, taps, one, one, 4, 8, 3, 3, 3, 9, 6, 6, None) == -2     # t > 2 d + 2
    assert lib.lfgc_lattice_sample_f32(0, None, 1, None, None, None, None, None, None, None, None) == -1


def test_forward_plan_has_no_two_tile_variant(built_lib, monkeypatch):
    """The two-tiles-per-wave kernel and its LFGC_FWD_X2 switch are gone: at the headline net on the lattice whose plan
    the switch used to change (32 channels x 128 wide, (72, 64, 256), slab x 3..70: 34 304 z-run tiles), the plan is the
    8-wave z-run launch with the reserved field x2 at 0, with or without the variable set.  Host only: the query reads
    the grid's shape and nothing else, so a stand-in with the shape of the decoded 64^3 grid takes the tensor's place."""
    from types import SimpleNamespace
    from latent_feature_grid_compression_amd import _lib, ops
    for k in [k for k in os.environ if k.startswith('LFGC_') and k != 'LFGC_LIB_PATH']:
        monkeypatch.delenv(k)
    desc = _lib.MlpDesc(32, 128, 4, 2, 3, 1)
    grid_cl = SimpleNamespace(shape=(64, 64, 64, 32), is_cuda=True)
    plan = lambda: ops.forward_plan(desc, grid_cl, lattice=((72, 64, 256), 3, 70, 32), precision='f16x2', want_stash=False)
    default = plan()
    monkeypatch.setenv('LFGC_FWD_X2', '1')
    with_switch = plan()
    assert default == with_switch
    for p in (default, with_switch):
        assert p.x2 == 0 and p.zrun == 1
        assert (p.CH, p.MT, p.resident, p.ntiles) == (32, 4, 0, 67 * 64 * 8)
        assert p.redo is not None and p.redo.x2 == 0


def test_philox_restatement_matches_published_vectors():
    """Random123's kat_vectors for philox4x32-10: the checker of test_fused_lattice_sampler is itself pinned."""
    from philox_ref import philox4x32_10
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array([ctr], np.uint32), np.array(key, np.uint32))[0]
        assert tuple(int(v) for v in got) == want


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    from latent_feature_grid_compression_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_lib.LfgcError, match='no CPU fallback'):
        _lib.load()


def test_module_mirrors_reference_interface():
    from latent_feature_grid_compression_amd.model.model_utils import setup_model
    from latent_feature_grid_compression_amd.model.Feature_Grid_Model import Feature_Grid_Model
    from latent_feature_grid_compression_amd import _lib
    g = np.load(os.path.join(GOLD, 'fwd_cfg1_c16g16h32l2.npz'))
    m = setup_model(3, 32, 1, 2, 'fourier', 2, '', 0.1, 0.9, 'db2', 16, 16, '')
    assert isinstance(m, Feature_Grid_Model)
    ref_keys = [k[3:] for k in g.files if k.startswith('sd.')]
    sd = m.state_dict()
    assert sorted(sd.keys()) == sorted(ref_keys)
    # order as the reference registers them: filter buffers, feature_grid.*, net_layers.*, final_layer.*
    assert list(sd.keys())[:2] == ['filter.filter_fwd', 'filter.filter_rev']
    assert [n for n, _ in m.named_parameters()] == ['feature_grid.0', 'feature_grid.1', 'feature_grid.2',
                                                    'net_layers.0.weight', 'net_layers.0.bias', 'net_layers.1.weight',
                                                    'net_layers.1.bias', 'final_layer.weight', 'final_layer.bias']
    for k in ref_keys:
        assert tuple(sd[k].shape) == g['sd.' + k].shape, k
    assert np.array_equal(sd['filter.filter_fwd'].numpy(), g['sd.filter.filter_fwd'])
    assert np.array_equal(sd['filter.filter_rev'].numpy(), g['sd.filter.filter_rev'])
    assert np.array_equal(m.shape_array, g['shape_array'])
    assert (m.input_channel, m.hidden_width, m.output_channel, m.num_layer, m.d_in) == (31, 32, 1, 2, 3)
    assert all(isinstance(d, torch.nn.Identity) for d in m.drop) and len(m.drop) == 3
    m.load_state_dict({k: torch.from_numpy(g['sd.' + k]) for k in ref_keys})      # reference checkpoints load
    assert float(m.save_dropvalues_on_grid('cpu')) == 0.0 and m.remove_drop_layers('cpu') is None
    with pytest.raises(_lib.LfgcError, match='no CPU fallback'):
        m(torch.zeros(8, 3))                                                        # the hot path is GPU-only


def test_host_encode_matches_reference_coefficients():
    """Init-time encode_volume on host tensors reproduces the reference's coefficient tensors and level shapes."""
    from latent_feature_grid_compression_amd.model.Feature_Grid_Model import Feature_Grid_Model
    from latent_feature_grid_compression_amd.model.Feature_Embedding import FourierEmbedding
    from latent_feature_grid_compression_amd.wavelet_transform.Torch_Wavelet_Transform import WaveletFilter3d, dwt_max_level
    for G in (15, 16, 17):
        g = np.load(os.path.join(GOLD, 'dwt_roundtrip_%d.npz' % G))
        m = Feature_Grid_Model(FourierEmbedding(2, 3), torch.from_numpy(g['input']), None, WaveletFilter3d('db2'),
                               hidden_channel=4, num_layer=1)
        assert np.array_equal(m.shape_array, g['shape_array'])
        for i, p in enumerate(m.feature_grid):
            assert np.array_equal(p.detach().numpy(), g['coeff%d' % i]), (G, i)
    with open(os.path.join(GOLD, 'levels_table.json')) as f:
        table = json.load(f)
    with open(os.path.join(GOLD, 'pywt_db2.json')) as f:
        pw = json.load(f)
    for n, lv in pw['dwt_max_level_flen4'].items():
        assert dwt_max_level(int(n), 4) == lv
    m = Feature_Grid_Model(FourierEmbedding(2, 3), torch.zeros(1, 64, 64, 64), None, WaveletFilter3d('db2'),
                           hidden_channel=4, num_layer=1)
    assert np.asarray(m.shape_array).tolist() == table['64']['shape_array']
    m3 = Feature_Grid_Model(FourierEmbedding(2, 3), torch.zeros(1, 128, 128, 128), None, WaveletFilter3d('db2'),
                            hidden_channel=4, num_layer=1, num_levels=3)              # BASELINE cfg 5: 3 levels on 128^3
    assert np.asarray(m3.shape_array).tolist() == table['128_levels3']['shape_array']
    assert [list(p.shape) for p in m3.feature_grid] == table['128_levels3']['coeff_shapes']


def test_embedder_and_dataset_arithmetic():
    from latent_feature_grid_compression_amd.model.Feature_Embedding import FourierEmbedding
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    g = np.load(os.path.join(GOLD, 'fwd_c4g15h16l3.npz'))
    emb = FourierEmbedding(2, 3)
    assert emb.out_dim == 12
    assert np.array_equal(emb.embed(torch.from_numpy(g['pos'])).numpy(), g['x0'][:, 3:15])
    gi = np.load(os.path.join(GOLD, 'gt_interp.npz'))
    ds = IndexDataset(torch.from_numpy(gi['vol_a']), 16)
    raw, norm = ds.positions_for(torch.from_numpy(gi['item_raw_a']))
    assert np.array_equal(norm.numpy(), gi['item_norm_a'])
    big = IndexDataset((1024, 1024, 1024), 16, build_index_table=False)       # no 12.9 GB table
    r, nrm = big[0]
    assert r.shape == (16, 3) and float(nrm.abs().max()) <= 1.0


def test_slab_partition_properties():
    from latent_feature_grid_compression_amd.visualization.OutputToVTK import slab_partition
    for res in (255, 256, 150, 33, 1024, 70):
        for world in (1, 2, 3, 4, 8):
            parts = slab_partition(res, world, 32)
            assert len(parts) == world and parts[0][0] == 0 and parts[-1][1] == res
            for (b0, e0), (b1, e1) in zip(parts[:-1], parts[1:]):
                assert e0 == b1 and b0 % 32 == 0 and b1 % 32 == 0 and e0 >= b0
            tiles = [((e - b) + 31) // 32 for b, e in parts]
            assert max(tiles) - min(tiles) <= 1


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, res, out_dir, chunks=None, gather='all'):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    from latent_feature_grid_compression_amd.visualization.OutputToVTK import reconstruct_volume_sharded
    ds = IndexDataset(res, 16, build_index_table=False)
    calls = []

    def slab_fn(b, e, out_view):            # stands in for the fused HIP forward of the slab
        calls.append((b, e))
        x = torch.arange(b, e, dtype=torch.float32).view(-1, 1, 1)
        y = torch.arange(res[1], dtype=torch.float32).view(1, -1, 1)
        z = torch.arange(res[2], dtype=torch.float32).view(1, 1, -1)
        out_view.copy_(x * 10000 + y * 100 + z)

    tm = {}
    vol = reconstruct_volume_sharded(ds, None, 32, slab_fn=slab_fn, device=torch.device('cpu'), chunks=chunks,
                                     gather=gather, root=world - 1 if gather == 'root' else 0, timings=tm)
    assert tm['world_size'] == world and tm['gather'] == gather
    torch.save({'vol': None if vol is None else vol.clone(), 'calls': calls}, os.path.join(out_dir, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('gather', ['all', 'root'])
@pytest.mark.parametrize('res,world,chunks', [((70, 9, 11), 2, None), ((33, 5, 4), 2, None), ((64, 6, 6), 2, 1),
                                              ((200, 4, 5), 2, 3), ((255, 3, 3), 3, None),
                                              ((64, 6, 6), 2, None), ((128, 3, 3), 4, None)])   # pieces finer than a tile plane
def test_sharded_reconstruction_gloo(tmp_path, res, world, chunks, gather):
    """world_size 2..4 over gloo: the slabs tile the volume exactly once; with gather='all' every rank holds the whole
    volume, with gather='root' only the root (here the LAST rank) does -- received straight into views of it, ragged
    slabs (70 = 2x32+6, 255 = 7x32+31) through the padding scratch."""
    port = _free_port()
    mp.spawn(_gloo_worker, args=(world, port, res, str(tmp_path), chunks, gather), nprocs=world, join=True)
    x = torch.arange(res[0], dtype=torch.float32).view(-1, 1, 1)
    y = torch.arange(res[1], dtype=torch.float32).view(1, -1, 1)
    z = torch.arange(res[2], dtype=torch.float32).view(1, 1, -1)
    expect = x * 10000 + y * 100 + z
    seen = []
    for r in range(world):
        d = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r), weights_only=True)
        if gather == 'all' or r == world - 1:
            assert torch.equal(d['vol'], expect), r                 # every rank (or the root alone) holds the whole volume
        else:
            assert d['vol'] is None
        seen += [tuple(c) for c in d['calls']]
    seen.sort()                                                    # the pieces tile [0, X) exactly once
    assert seen[0][0] == 0 and seen[-1][1] == res[0]
    assert all(a[1] == b[0] for a, b in zip(seen[:-1], seen[1:]))


def _replay_setup_model(case):
    """Replay, against this package, the constructor calls the reference's own model_utils.setup_model made with this
    package's modules registered under the reference's module names (tests/golden/swap_setup_model.json, recorded by
    tools/make_goldens_swap.py): same classes, same positional / keyword arguments, same order."""
    from latent_feature_grid_compression_amd.model.Feature_Grid_Model import Feature_Grid_Model
    from latent_feature_grid_compression_amd.model.Feature_Embedding import FourierEmbedding
    from latent_feature_grid_compression_amd.model.Smallify_Dropout import SmallifyDropout
    from latent_feature_grid_compression_amd.wavelet_transform.Torch_Wavelet_Transform import WaveletFilter3d
    classes = {c.__name__: c for c in (Feature_Grid_Model, FourierEmbedding, SmallifyDropout, WaveletFilter3d)}
    made = {}

    def dec(v):
        if isinstance(v, dict) and 'size' in v:
            return torch.Size(v['size'])
        if isinstance(v, dict) and 'tensor' in v:
            return torch.empty(v['tensor']).uniform_(0, 1)
        if isinstance(v, dict) and 'object' in v:
            return made[v['object']]
        return v
    for call in case['calls']:
        made[call['class']] = classes[call['class']](*[dec(a) for a in call['args']],
                                                     **{k: dec(v) for k, v in call['kwargs'].items()})
    return made['Feature_Grid_Model']


def test_reference_factory_builds_our_module_after_module_swap():
    """INTEGRATION.md route A: with our modules registered under the reference's module names, the reference's
    own setup_model constructs the HIP-backed module (host logic only).  Replayed from the recorded calls: the model
    has the shapes, parameter order and state_dict keys the reference's factory saw, its pruning layers plug in where
    the reference's pruning loss looks for them, and a state_dict round trip works."""
    from latent_feature_grid_compression_amd.model.Feature_Grid_Model import Feature_Grid_Model
    from latent_feature_grid_compression_amd.model.model_utils import get_net_weights_biases
    from latent_feature_grid_compression_amd.model.Smallify_Dropout import SmallifyDropout
    with open(os.path.join(GOLD, 'swap_setup_model.json')) as f:
        cases = json.load(f)
    assert set(cases) == {'smallify', 'no_drop'}
    for name, case in cases.items():
        torch.manual_seed(0)
        m = _replay_setup_model(case)
        assert type(m) is Feature_Grid_Model
        assert case['model_class'] == Feature_Grid_Model.__module__ + '.Feature_Grid_Model'
        assert type(m.drop[0]).__name__ == case['drop_class'], name
        assert [list(p.shape) for p in m.feature_grid] == case['feature_grid_shapes'], name
        w, b = get_net_weights_biases(m)
        assert [list(t.shape) for t in w] == case['weight_shapes'] and [list(t.shape) for t in b] == case['bias_shapes']
        assert list(m.state_dict().keys()) == case['state_dict_keys'], name
        # what the reference's SmallifyLoss walks (model.apply): the pruning layers' l1_loss and the grid tensors
        seen = []
        m.apply(lambda mod: seen.append(mod) if isinstance(mod, SmallifyDropout) else None)
        assert len(seen) == (len(case['feature_grid_shapes']) if case['drop_class'] == 'SmallifyDropout' else 0), name
        assert all(callable(getattr(mod, 'l1_loss', None)) for mod in seen)
        assert torch.isfinite(sum(torch.sum(torch.abs(f) ** 2) for f in m.feature_grid))
        m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})


def test_ward_init_host_function():
    """lfgc_codec_ward_init_host (host C++, no device): greedy adjacent Ward merging == a straightforward Python heap
    version; n <= k returns the values themselves; unsorted input is rejected."""
    import ctypes
    import heapq
    from latent_feature_grid_compression_amd import _lib
    lib = _lib.load()
    fp = ctypes.POINTER(ctypes.c_float)
    rng = np.random.default_rng(8)
    x = np.sort(np.concatenate([rng.standard_normal(700) * 0.05, rng.standard_normal(60) * 3])).astype(np.float32)
    k = 64
    out = np.empty(k, np.float32)
    assert lib.lfgc_codec_ward_init_host(x.ctypes.data_as(fp), x.size, k, out.ctypes.data_as(fp)) == 0
    cnt, su = [1.0] * x.size, [float(v) for v in x]
    nxt = list(range(1, x.size)) + [-1]
    prv = list(range(-1, x.size - 1))
    alive, ver = [True] * x.size, [0] * x.size
    cost = lambda a, b: cnt[a] * cnt[b] / (cnt[a] + cnt[b]) * (su[a] / cnt[a] - su[b] / cnt[b]) ** 2
    heap = [(cost(i, i + 1), i, i + 1, 0, 0) for i in range(x.size - 1)]
    heapq.heapify(heap)
    n = x.size
    while n > k:
        c, a, b, va, vb = heapq.heappop(heap)
        if not (alive[a] and alive[b]) or ver[a] != va or ver[b] != vb or nxt[a] != b:
            continue
        cnt[a] += cnt[b]; su[a] += su[b]; alive[b] = False; ver[a] += 1
        nxt[a] = nxt[b]
        if nxt[b] != -1:
            prv[nxt[b]] = a
            heapq.heappush(heap, (cost(a, nxt[a]), a, nxt[a], ver[a], ver[nxt[a]]))
        if prv[a] != -1:
            heapq.heappush(heap, (cost(prv[a], a), prv[a], a, ver[prv[a]], ver[a]))
        n -= 1
    ref = np.asarray([su[i] / cnt[i] for i in range(x.size) if alive[i]], np.float32)
    assert np.array_equal(out, ref)
    few = np.asarray([-1.0, 0.25, 0.5], np.float32)
    out4 = np.empty(4, np.float32)
    assert lib.lfgc_codec_ward_init_host(few.ctypes.data_as(fp), 3, 4, out4.ctypes.data_as(fp)) == 0
    assert out4.tolist() == [-1.0, 0.25, 0.5, 0.5]
    bad = np.asarray([1.0, 0.0], np.float32)
    assert lib.lfgc_codec_ward_init_host(bad.ctypes.data_as(fp), 2, 1, out4.ctypes.data_as(fp)) == -2


SWAPPED = ('model.Feature_Grid_Model', 'model.Feature_Embedding', 'wavelet_transform.Torch_Wavelet_Transform',
           'data.Interpolation', 'model.Dropout_Layer', 'model.Smallify_Dropout', 'model.Straight_Through_Dropout',
           'model.Variational_Dropout_Layer', 'model.model_utils')


def test_every_name_the_reference_imports_from_the_swapped_modules_exists():
    """INTEGRATION.md route A registers this package's modules under the reference's module names: every
    ``from <swapped module> import a, b`` in the reference's own sources must then resolve (the reference's imports
    are recorded in tests/golden/swap_imports.json by tools/make_goldens_swap.py)."""
    import importlib
    with open(os.path.join(GOLD, 'swap_imports.json')) as f:
        imports = json.load(f)
    checked = [(mod, name, fn) for mod, name, fn in imports if mod in SWAPPED]
    assert {mod for mod, _, _ in checked} >= {'model.Feature_Grid_Model', 'model.model_utils', 'model.Smallify_Dropout'}
    missing = []
    for mod, name, fn in checked:
        ours = importlib.import_module('latent_feature_grid_compression_amd.' + mod)
        if not hasattr(ours, name):
            missing.append('%s.%s (%s)' % (mod, name, fn))
    assert not missing, missing


def test_channel_last_level_entries_agree_on_argument_errors(built_lib):
    """The argument-error rows of tests/test_cl_drop_host.py (all but the C > 32 ones, where the two pairs differ on
    purpose) through every channel-last level entry: the plain `_len` pair and the drop pair with NULL factors return the
    same code, and the 4-tap aliases the code of `_len` with 4.  Every row returns before anything is launched (dummy
    addresses, no device work)."""
    from latent_feature_grid_compression_amd import _lib
    lib = _lib.load()
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
    one, nan = ctypes.c_void_p(16), float('nan')
    taps8 = (ctypes.c_float * 16)(*[0.5] * 16)
    ok_shape = (4, 8, 3, 3, 3, 6, 6, 6)
    rows = []                 # (expected, pointers a b c [forward: lll hf out; adjoint: d_out d_lll d_hf], taps, L, shape)
    for L in (2, 4):
        for missing in range(3):              # a required pointer is missing
            rows.append((E_NULL, [None if i == missing else one for i in range(3)], taps8, L, ok_shape))
        rows += [(E_SHAPE, [one] * 3, taps8, L, shape) for shape in (
            (4, 16, 3, 3, 3, 6, 6, 6), (9, 8, 3, 3, 3, 6, 6, 6),           # stride is not C rounded up to 8
            (4, 8, 3, 3, 3, 2 * 3 + L - 1, 6, 6), (4, 8, 3, 3, 3, 6, 2 * 3 + L - 1, 6), (4, 8, 3, 3, 3, 6, 6, 0))]   # t_a
        rows.append((E_UNSUPPORTED, [one] * 3, None, L, ok_shape))           # dense stencil
        rows += [(E_UNSUPPORTED, [one] * 3, taps8, L, shape) for shape in (  # arrays of 2^30 bytes and more
            (32, 32, 200, 200, 200, 400, 400, 400), (32, 32, 110, 110, 110, 6, 6, 6))]
    rows += [(E_UNSUPPORTED, [one] * 3, taps8, L, ok_shape) for L in (0, 1, 3, 6, 8)]
    for want, (a, b, c), taps, L, shape in rows:
        fwd = (lib.lfgc_idwt_level_cl_len_f32(a, b, taps, L, c, *shape, None),
               lib.lfgc_idwt_level_cl_drop_len_f32(a, b, None, nan, None, nan, taps, L, c, *shape, None))
        bwd = (lib.lfgc_idwt_level_cl_bwd_len_f32(a, taps, L, b, c, *shape, None),
               lib.lfgc_idwt_level_cl_drop_bwd_len_f32(a, taps, L, None, None, None, None, b, c, None, None, None, *shape, None))
        if L == 4:
            fwd += (lib.lfgc_idwt_level_cl_f32(a, b, taps, c, *shape, None),)
            bwd += (lib.lfgc_idwt_level_cl_bwd_f32(a, taps, b, c, *shape, None),)
        assert set(fwd) == {want} and set(bwd) == {want}, (want, fwd, bwd, L, shape)


def test_public_level_and_decode_signatures():
    """The wrappers that tests, tools and the model call by position keep the signatures they had before the level
    wrappers were folded into one synthesis and one adjoint function."""
    import inspect
    from latent_feature_grid_compression_amd import ops
    want = {
        'idwt_level': '(lll: torch.Tensor, hf: torch.Tensor, filter_rev: torch.Tensor, target: Sequence[int]) -> torch.Tensor',
        'idwt_level_bwd': '(d_out: torch.Tensor, filter_rev: torch.Tensor, d: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]',
        'idwt_level_cl': '(lll: torch.Tensor, hf: torch.Tensor, filter_rev: torch.Tensor, target: Sequence[int]) -> torch.Tensor',
        'idwt_level_cl_bwd': '(d_out_cl: torch.Tensor, C: int, filter_rev: torch.Tensor, d: Sequence[int]) '
                             '-> Tuple[torch.Tensor, torch.Tensor]',
        'idwt_level_drop': '(lll, hf, mul_l, thr_l, mul_h, thr_h, filter_rev, target) -> torch.Tensor',
        'idwt_level_drop_bwd': '(d_out, filter_rev, lll, hf, mul_l, mul_h, want_dml, want_dmh, d, penalty_ptrs=None)',
        'idwt_level_cl_drop': '(lll, hf, mul_l, thr_l, mul_h, thr_h, filter_rev, target) -> torch.Tensor',
        'idwt_level_cl_drop_bwd': '(d_out_cl, C, filter_rev, lll, hf, mul_l, mul_h, want_dml, want_dmh, d, penalty_ptrs=None)',
        'decode_levels': '(coeffs: Sequence[torch.Tensor], shape_array, filter_rev: torch.Tensor, channel_last: bool) '
                         '-> torch.Tensor',
        'decode_levels_drop': '(coeffs, factors, thresholds, shape_array, filter_rev, channel_last: bool) -> torch.Tensor',
        'dwt_level': '(data: torch.Tensor, filter_fwd: torch.Tensor) -> torch.Tensor',
        'DecodeVolumeFn.forward': '(ctx, filter_rev, shape_array, channel_last, *coeffs)',
        'DecodeVolumeDropFn.forward': '(ctx, filter_rev, shape_array, channel_last, thresholds, n, *tensors)',
        'DecodeVolumePenaltyFn.forward': '(ctx, filter_rev, shape_array, channel_last, thresholds, n, l1_flags, *tensors)',
    }
    for name, sig in want.items():
        obj = ops
        for part in name.split('.'):
            obj = getattr(obj, part)
        assert str(inspect.signature(obj)).replace("'", '') == sig, name      # annotations are kept as strings
