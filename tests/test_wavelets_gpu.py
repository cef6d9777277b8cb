"""GPU tests of the wavelet bases beyond db2: every even filter length L in {2, 4, 6, 8} through one decode level, its
adjoint, the forward DWT, the drop variants and the penalty fold, against the oracle's conv_transpose3d / conv3d
arithmetic (oracle/ref_torch.py); the Haar channel-last last level; the 4-tap *_len_f32 entries against the plain ones;
and a whole Haar model (plain and Smallify, eager and graph-replayed) against the reference-captured fixtures."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from oracle import ref_drop as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
LENGTHS = (2, 4, 6, 8)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def rel_err(y, ref):
    y = np.asarray(y, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    return np.abs(y - ref).max() / max(np.abs(ref).max(), 1e-30)


def filters(L):
    """(filter_fwd, filter_rev) fp32 CPU: db2 from the oracle's recipe, the others as captured from the reference."""
    if L == 4:
        return R.build_filters(3)
    with np.load(os.path.join(GOLD, 'wavelets_filters.npz')) as z:
        return torch.from_numpy(z['filter_fwd_%d' % L]), torch.from_numpy(z['filter_rev_%d' % L])


def level_cases(L):
    """(C, d, t): odd, even, non-cubic, 1^3 and one large level (the sliding-window kernel for 4 taps); t at the full
    size 2d + L - 2 and cropped."""
    full = lambda d: tuple(2 * v + L - 2 for v in d)
    return [(3, (5, 5, 5), (9, 9, 9)), (2, (6, 6, 6), full((6, 6, 6))), (5, (4, 7, 5), (8, 13, 9)),
            (4, (3, 8, 6), full((3, 8, 6))), (3, (1, 1, 1), (2, 2, 2)), (2, (1, 1, 1), full((1, 1, 1))),
            (3, (20, 24, 18), (40, 47, 36))]


def oracle_level(lll, hf, frev, t):
    data = torch.cat([lll.unsqueeze(0).unsqueeze(2), hf.unsqueeze(0)], dim=2)
    return R.wavelet_decode(data, t, frev)[0]


@pytest.mark.parametrize('L', LENGTHS)
def test_one_level_decode_and_adjoint_against_oracle(dev, L):
    from latent_feature_grid_compression_amd import ops
    _, frev = filters(L)
    for C, d, t in level_cases(L):
        rng = np.random.default_rng(L * 1000 + C * 10 + d[0])
        lll = torch.from_numpy(rng.standard_normal((C,) + d).astype(np.float32))
        hf = torch.from_numpy(rng.standard_normal((C, 7) + d).astype(np.float32))
        g = torch.from_numpy(rng.standard_normal((C,) + t).astype(np.float32))
        ref_in = [lll.clone().requires_grad_(True), hf.clone().requires_grad_(True)]
        ref = oracle_level(*ref_in, frev, t)
        (ref * g).sum().backward()
        got = ops.idwt_level(lll.to(dev), hf.to(dev), frev.to(dev), t)
        assert rel_err(got.cpu().numpy(), ref.detach().numpy()) <= 1e-6, (L, C, d, t)
        d_l, d_h = ops.idwt_level_bwd(g.to(dev), frev.to(dev), d)
        # 5e-6 absolute as for db2; the seeded 6- and 8-tap test banks (taps up to 1, up to 512 of them) give gradients
        # of magnitude 10 and more, so there the bound is relative to the largest one
        for got, want in ((d_l, ref_in[0].grad), (d_h, ref_in[1].grad)):
            bound = 5e-6 * max(1.0, float(want.abs().max()))
            assert np.abs(got.cpu().numpy() - want.numpy()).max() <= bound, (L, C, d, t)


@pytest.mark.parametrize('L', LENGTHS)
def test_dwt_encode_against_oracle(dev, L):
    from latent_feature_grid_compression_amd import ops
    ffwd, _ = filters(L)
    for n in ((9, 12, 7), (16, 16, 16), (15, 15, 15), (2, 2, 2), (3, 5, 2), (33, 20, 17)):
        rng = np.random.default_rng(L * 100 + n[0])
        x = torch.from_numpy(rng.standard_normal((3,) + n).astype(np.float32))
        ref, _ = R.wavelet_encode(x.unsqueeze(0), ffwd)
        got = ops.dwt_level(x.to(dev), ffwd.to(dev))
        assert got.shape == ref.shape[1:], (L, n)
        assert rel_err(got.cpu().numpy(), ref[0].numpy()) <= 1e-6, (L, n)


@pytest.mark.parametrize('L', [2, 6, 8])
def test_roundtrip_fixtures(dev, L):
    """Model-level encode (levels down to 1^3 for Haar) and decode against the reference's captured round trips."""
    from latent_feature_grid_compression_amd import ops
    z = np.load(os.path.join(GOLD, 'wavelets_roundtrip_L%d.npz' % L))
    ffwd, frev = (f.to(dev) for f in filters(L))
    for G in (15, 16, 17):
        n = int(z['G%d.n' % G])
        data = torch.from_numpy(z['G%d.input' % G]).to(dev)
        coeffs = []
        for _ in range(n - 1):
            c = ops.dwt_level(data, ffwd)
            coeffs.append(c[:, 1:])
            data = c[:, 0].contiguous()
        coeffs = [data] + coeffs[::-1]
        for i, c in enumerate(coeffs):
            assert rel_err(c.cpu().numpy(), z['G%d.coeff%d' % (G, i)]) <= 1e-5, (G, i)
        want = [torch.from_numpy(z['G%d.coeff%d' % (G, i)]).to(dev) for i in range(n)]
        for cl in (False, True):
            out = ops.decode_levels(want, z['G%d.shape_array' % G], frev, channel_last=cl)
            if cl:
                out = ops.to_channel_first(out, want[0].shape[0])
            assert rel_err(out.cpu().numpy(), z['G%d.decoded' % G]) <= 1e-5, (G, cl)


CL_CASES = [   # the ragged shapes of the db2 channel-last test (tests/test_hip_forward.py), t = 2d or 2d - 1
    (1, (3, 4, 5)), (5, (6, 7, 9)), (8, (9, 9, 9)), (13, (5, 12, 7)), (16, (17, 17, 17)), (22, (4, 35, 6)),
    (24, (10, 11, 12)), (30, (8, 9, 40)), (32, (17, 18, 16)), (32, (33, 33, 33)), (3, (1, 1, 1)), (32, (2, 70, 3)),
    (40, (5, 6, 7)), (32, (2, 64, 64)), (16, (2, 64, 64)), (8, (3, 60, 60)), (32, (65, 65, 65)),
]


@pytest.mark.parametrize('C,d', CL_CASES)
def test_haar_channel_last_level(dev, C, d):
    from latent_feature_grid_compression_amd import ops
    rng = np.random.default_rng(C * 1000 + d[0] + 7)
    _, frev = filters(2)
    frev_d = frev.to(dev)
    ts = [tuple(2 * v for v in d), tuple(2 * v - 1 for v in d), (2 * d[0], 2 * d[1] - 1, 2 * d[2])]
    for t in ts:
        lll = torch.from_numpy(rng.standard_normal((C,) + d).astype(np.float32))
        hf = torch.from_numpy(rng.standard_normal((C, 7) + d).astype(np.float32))
        want = ops.to_channel_last(ops.idwt_level(lll.to(dev), hf.to(dev), frev_d, t))
        got = ops.idwt_level_cl(lll.to(dev), hf.to(dev), frev_d, t)
        assert got.shape == want.shape
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 2e-6 * scale, t
        cs = got.shape[-1]
        if cs > C:
            assert float(got[..., C:].abs().max()) == 0.0
        g_cl = torch.from_numpy(rng.standard_normal(tuple(t) + (cs,)).astype(np.float32)).to(dev)
        w_l, w_h = ops.idwt_level_bwd(ops.to_channel_first(g_cl, C), frev_d, d)
        g_l, g_h = ops.idwt_level_cl_bwd(g_cl, C, frev_d, d)
        s = float(max(w_l.abs().max(), w_h.abs().max()))
        assert float((g_l - w_l).abs().max()) <= 2e-6 * s, t
        assert float((g_h - w_h).abs().max()) <= 2e-6 * s, t
        if C <= 8 and max(d) <= 12:          # small cases: also straight against the oracle
            ref_in = [lll.clone().requires_grad_(True), hf.clone().requires_grad_(True)]
            ref = oracle_level(*ref_in, frev, t)
            assert rel_err(ops.to_channel_first(got, C).cpu().numpy(), ref.detach().numpy()) <= 1e-6
            g_cf = ops.to_channel_first(g_cl, C).cpu()
            (ref * g_cf).sum().backward()
            assert np.abs(g_l.cpu().numpy() - ref_in[0].grad.numpy()).max() <= 5e-6
            assert np.abs(g_h.cpu().numpy() - ref_in[1].grad.numpy()).max() <= 5e-6


def test_channel_last_entry_refuses_long_filters(dev):
    from latent_feature_grid_compression_amd import ops, _lib
    lib = _lib.load()
    for L in (6, 8):
        taps = (ctypes.c_float * (2 * L))(*([0.5] * (2 * L)))
        lll = torch.zeros((2, 3, 3, 3), device=dev)
        hf = torch.zeros((2, 7, 3, 3, 3), device=dev)
        out = torch.zeros((4, 4, 4, 8), device=dev)
        rc = lib.lfgc_idwt_level_cl_len_f32(lll.data_ptr(), hf.data_ptr(), taps, L, out.data_ptr(), 2, 8, 3, 3, 3, 4, 4, 4,
                                            ops._stream(lll))
        assert rc == ops._E_UNSUPPORTED
        # the wrapper composes the channel-first level with the layout pass instead
        _, frev = filters(L)
        got = ops.idwt_level_cl(torch.randn(2, 3, 3, 3, device=dev), torch.randn(2, 7, 3, 3, 3, device=dev),
                                frev.to(dev), (4, 4, 4))
        assert got.shape == (4, 4, 4, 8)
    # a dense (non-separable) filter of another length has no kernel
    rc = lib.lfgc_idwt_level_len_f32(lll.data_ptr(), hf.data_ptr(), out.data_ptr(), None, 2, out.data_ptr(), 2, 3, 3, 3,
                                     4, 4, 4, ops._stream(lll))
    assert rc == ops._E_UNSUPPORTED


@pytest.mark.parametrize('L', LENGTHS)
@pytest.mark.parametrize('thr', [None, 0.5])
def test_drop_level_and_penalty_fold_against_oracle(dev, L, thr):
    """The drop variants (plain and masked straight-through factors) and the penalty fold of the adjoint
    (oracle/ref_drop.py: l1 of the factors, grid L2), through DecodeVolumePenaltyFn with one wavelet level."""
    from latent_feature_grid_compression_amd import ops
    _, frev = filters(L)
    for C, d, t in ((5, (6, 7, 9), tuple(min(a, 2 * v + L - 2) for a, v in zip((13, 15, 19), (6, 7, 9)))),
                    (3, (4, 5, 3), tuple(2 * v + L - 2 for v in (4, 5, 3))), (2, (1, 1, 1), (2, 2, 2))):
        rng = np.random.default_rng(L * 100 + C)
        lll = torch.from_numpy(rng.standard_normal((C,) + d).astype(np.float32))
        hf = torch.from_numpy(rng.standard_normal((C, 7) + d).astype(np.float32))
        ml = torch.from_numpy(rng.uniform(-1.0, 1.0, d).astype(np.float32))
        mh = torch.from_numpy(rng.uniform(-1.0, 1.0, (7,) + d).astype(np.float32))
        w = torch.from_numpy(rng.standard_normal((C,) + t).astype(np.float32))
        pw = torch.tensor([0.7, -1.3, 0.4, 2.1])            # weights of the 4 penalty sums in the loss

        def apply(x, m):
            if thr is None:
                return x * m.unsqueeze(0)
            return (x * (m >= thr) - x * m).detach() + x * m

        ref_in = [x.clone().requires_grad_(True) for x in (lll, hf, ml, mh)]
        ref = oracle_level(apply(ref_in[0], ref_in[2]), apply(ref_in[1], ref_in[3]), frev, t)
        pen = torch.stack([D.grid_l2_penalty([ref_in[0]]), D.grid_l2_penalty([ref_in[1]]),
                           D.l1_penalty(ref_in[2]), D.l1_penalty(ref_in[3])])
        ((ref * w).sum() + (pen * pw).sum()).backward()

        got_in = [x.to(dev).requires_grad_(True) for x in (lll, hf, ml, mh)]
        grid, gpen = ops.DecodeVolumePenaltyFn.apply(frev.to(dev), [t], False, [thr, thr], 2, [True, True], *got_in)
        assert rel_err(grid.detach().cpu().numpy(), ref.detach().numpy()) <= 1e-5, (L, C, d)
        assert rel_err(gpen.detach().cpu().numpy(), pen.detach().numpy()) <= 2e-6, (L, C, d)
        ((grid * w.to(dev)).sum() + (gpen * pw.to(dev)).sum()).backward()
        for got, want in zip(got_in, ref_in):
            assert rel_err(got.grad.cpu().numpy(), want.grad.numpy()) <= 2e-5, (L, C, d)


def test_len_entries_bit_equal_plain_4tap(dev):
    """filter_len = 4 through the *_len_f32 entries is the plain 4-tap entry bit for bit (separable and dense)."""
    from latent_feature_grid_compression_amd import ops, _lib
    lib = _lib.load()
    ffwd, frev = (f.to(dev) for f in R.build_filters(3))
    rng = np.random.default_rng(44)
    C, d, t = 6, (9, 10, 11), (17, 20, 21)
    lll = torch.from_numpy(rng.standard_normal((C,) + d).astype(np.float32)).to(dev)
    hf = torch.from_numpy(rng.standard_normal((C, 7) + d).astype(np.float32)).to(dev)
    ml = torch.from_numpy(rng.uniform(0, 1, d).astype(np.float32)).to(dev)
    mh = torch.from_numpy(rng.uniform(0, 1, (7,) + d).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((C,) + t).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.standard_normal((C,) + t).astype(np.float32)).to(dev)
    s = ops._stream(lll)
    for taps in (ops.filter_taps(frev), None):
        a, b = torch.empty((C,) + t, device=dev), torch.empty((C,) + t, device=dev)
        assert lib.lfgc_idwt_level_f32(lll.data_ptr(), hf.data_ptr(), frev.data_ptr(), taps, a.data_ptr(), C, *d, *t, s) == 0
        assert lib.lfgc_idwt_level_len_f32(lll.data_ptr(), hf.data_ptr(), frev.data_ptr(), taps, 4, b.data_ptr(), C, *d, *t, s) == 0
        assert torch.equal(a, b)
        assert lib.lfgc_idwt_level_drop_f32(lll.data_ptr(), hf.data_ptr(), ml.data_ptr(), float('nan'), mh.data_ptr(), 0.5,
                                            frev.data_ptr(), taps, a.data_ptr(), C, *d, *t, s) == 0
        assert lib.lfgc_idwt_level_drop_len_f32(lll.data_ptr(), hf.data_ptr(), ml.data_ptr(), float('nan'), mh.data_ptr(),
                                                0.5, frev.data_ptr(), taps, 4, b.data_ptr(), C, *d, *t, s) == 0
        assert torch.equal(a, b)
        out = [torch.empty((C,) + d, device=dev) for _ in range(4)] + [torch.empty((C, 7) + d, device=dev) for _ in range(4)]
        dm = [torch.zeros(d, device=dev), torch.zeros(d, device=dev), torch.zeros((7,) + d, device=dev),
              torch.zeros((7,) + d, device=dev)]
        assert lib.lfgc_idwt_level_bwd_f32(g.data_ptr(), frev.data_ptr(), taps, out[0].data_ptr(), out[4].data_ptr(), C, *d, *t, s) == 0
        assert lib.lfgc_idwt_level_bwd_len_f32(g.data_ptr(), frev.data_ptr(), taps, 4, out[1].data_ptr(), out[5].data_ptr(),
                                               C, *d, *t, s) == 0
        assert lib.lfgc_idwt_level_drop_bwd_f32(g.data_ptr(), frev.data_ptr(), taps, lll.data_ptr(), hf.data_ptr(),
                                                ml.data_ptr(), mh.data_ptr(), out[2].data_ptr(), out[6].data_ptr(),
                                                dm[0].data_ptr(), dm[2].data_ptr(), None, C, *d, *t, s) == 0
        assert lib.lfgc_idwt_level_drop_bwd_len_f32(g.data_ptr(), frev.data_ptr(), taps, 4, lll.data_ptr(), hf.data_ptr(),
                                                    ml.data_ptr(), mh.data_ptr(), out[3].data_ptr(), out[7].data_ptr(),
                                                    dm[1].data_ptr(), dm[3].data_ptr(), None, C, *d, *t, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[0], out[1]) and torch.equal(out[4], out[5])
        assert torch.equal(out[2], out[3]) and torch.equal(out[6], out[7])
        # the factor gradients are float-atomic sums over the channels: equal up to the order of the adds
        assert rel_err(dm[1].cpu().numpy(), dm[0].cpu().numpy()) <= 1e-6
        assert rel_err(dm[3].cpu().numpy(), dm[2].cpu().numpy()) <= 1e-6
        cs = ops.grid_channel_stride(C)
        if taps is not None:
            a, b = torch.empty(t + (cs,), device=dev), torch.empty(t + (cs,), device=dev)
            assert lib.lfgc_idwt_level_cl_f32(lll.data_ptr(), hf.data_ptr(), taps, a.data_ptr(), C, cs, *d, *t, s) == 0
            assert lib.lfgc_idwt_level_cl_len_f32(lll.data_ptr(), hf.data_ptr(), taps, 4, b.data_ptr(), C, cs, *d, *t, s) == 0
            assert torch.equal(a, b)
            gcl = a.contiguous()
            for i in range(4):
                out[i].zero_()
            assert lib.lfgc_idwt_level_cl_bwd_f32(gcl.data_ptr(), taps, out[0].data_ptr(), out[4].data_ptr(), C, cs, *d, *t, s) == 0
            assert lib.lfgc_idwt_level_cl_bwd_len_f32(gcl.data_ptr(), taps, 4, out[1].data_ptr(), out[5].data_ptr(), C, cs,
                                                      *d, *t, s) == 0
            assert torch.equal(out[0], out[1]) and torch.equal(out[4], out[5])
        n = t
        e, f = torch.empty((C, 8) + tuple(ops.dwt_out_shape(n)), device=dev), torch.empty((C, 8) + tuple(ops.dwt_out_shape(n)), device=dev)
        fw_taps = ops.filter_taps(ffwd) if taps is not None else None
        assert lib.lfgc_dwt_level_f32(x.data_ptr(), ffwd.data_ptr(), fw_taps, e.data_ptr(), C, *n, s) == 0
        assert lib.lfgc_dwt_level_len_f32(x.data_ptr(), ffwd.data_ptr(), fw_taps, 4, f.data_ptr(), C, *n, s) == 0
        assert torch.equal(e, f)


def _load_model(z, drop_type, dev):
    from latent_feature_grid_compression_amd.model.model_utils import setup_model
    C, G, H, NL, _ = (int(v) for v in z['meta'])
    m = setup_model(3, H, 1, NL, 'fourier', 2, drop_type, 0.025, 0.75, 'haar', C, G, '')
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd.')}
    m.load_state_dict(sd)
    assert np.array_equal(np.asarray(m.shape_array), z['shape_array'])
    return m.to(dev).train()


@pytest.mark.parametrize('fixture,drop_type', [('wavelets_haar_model', ''), ('wavelets_haar_smallify', 'smallify')])
@pytest.mark.parametrize('precision', ['fp32', 'f16x2'])
def test_haar_model_against_reference(dev, fixture, drop_type, precision):
    z = np.load(os.path.join(GOLD, fixture + '.npz'))
    m = _load_model(z, drop_type, dev)
    m.precision = precision
    assert len(m.feature_grid) == len(z['shape_array']) + 1 and tuple(m.feature_grid[0].shape[1:]) == (1, 1, 1)
    pos = torch.from_numpy(z['pos']).to(dev).requires_grad_(True)
    y = m(pos)
    assert rel_err(y.detach().cpu().numpy(), z['y']) <= 1e-5
    loss = torch.nn.functional.mse_loss(y.squeeze(-1), torch.from_numpy(z['target']).to(dev))
    m.zero_grad()
    loss.backward()
    tol = 2e-5 if precision == 'fp32' else 2e-4
    assert rel_err(pos.grad.cpu().numpy(), z['grad_pos']) <= tol
    for k, p in m.named_parameters():
        if 'grad.' + k in z.files:
            assert p.grad is not None, k
            assert rel_err(p.grad.cpu().numpy(), z['grad.' + k]) <= tol, k


def test_haar_smallify_graph_replay_equals_eager(dev):
    """One captured Haar + Smallify train step (forward, loss with the Smallify penalties, backward, fused Adam),
    replayed, does what the same eager steps do."""
    from latent_feature_grid_compression_amd.model.Smallify_Dropout import SmallifyLoss
    z = np.load(os.path.join(GOLD, 'wavelets_haar_smallify.npz'))
    pos = torch.from_numpy(z['pos']).to(dev)
    target = torch.from_numpy(z['target']).to(dev)
    crit = SmallifyLoss(1e-6, 1e-8)
    warm, K = 2, 3

    def setup():
        m = _load_model(z, 'smallify', dev)
        opt = torch.optim.Adam(m.parameters(), lr=0.008, capturable=True, fused=True)

        def step():
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(m(pos).squeeze(-1), target) + crit(m)
            loss.backward()
            opt.step()
            return loss
        return m, opt, step

    ma, opt_a, step_a = setup()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager_a = [float(step_a().detach()) for _ in range(warm)]
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    opt_a.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        loss_a = step_a()
    replay = []
    for _ in range(K):
        graph.replay()
        replay.append(float(loss_a.detach()))
    torch.cuda.synchronize()

    mb, _, step_b = setup()
    losses_b = [float(step_b().detach()) for _ in range(warm + K)]
    torch.cuda.synchronize()
    for a, b in zip(eager_a + replay, losses_b):
        assert abs(a - b) <= 1e-5 * abs(b), (eager_a, replay, losses_b)
    # coefficient gradients are float-atomic sums (order-dependent in the last bits) and Adam's first steps move an
    # entry by ~lr g/|g|: all but 1e-3 of the entries agree to 1e-4 of the tensor's largest, none by more than 2 lr steps
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        diff = (pa.detach() - pb.detach()).abs()
        scale = float(pb.detach().abs().max()) or 1.0
        assert float((diff > 1e-4 * scale).float().mean()) <= 1e-3, k
        assert float(diff.max()) <= 2 * 0.008 * (warm + K), k
