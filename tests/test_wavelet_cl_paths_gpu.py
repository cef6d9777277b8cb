"""GPU tests of every launch path of the channel-last last-level kernels (csrc/lfgc_wavelet_cl.hip: idwt_cl_kernel,
analysis_cl_kernel) against the oracle run in float64, under the componentwise bound of tests/wavelet_bound.py:
|got - ref64| <= c * 2^-24 * mag for EVERY element, pad channels of the grid exactly zero, with the max-normalised bounds
of tests/test_wavelet_paths_gpu.py (1e-6 forward, 5e-6 * max(1, max|ref|) adjoint) kept beside it.

c is derived, not measured: both kernels contract x, then y, then z with 2K-term fmaf chains over the 1-D bank (the z
chain split between the carry registers and the step that completes it: the same 2K terms), which is the count of the
channel-first separable kernels: c = c_separable(K) = 6K + 12.  A factor gradient is an LDS sum over the CW channels of a
workgroup plus C / CW float atomics, at most C additions: c_factor_gradient(c, C).

Each case first asserts its plan (ops.idwt_level_cl_plan / ops.idwt_level_cl_bwd_plan with the current device's CU count
and the diagnostics knobs as the case sets them: the launchers consume the struct these queries fill) against the rules
restated in tests/wavelet_bound.py, so a change of the selection that would leave an instantiation untested fails here;
tests/test_wavelet_cl_plans_host.py holds the same rules on the CPU for other CU counts.

Paths (W.CL_ROWS; both bases -- db2 cropped by one on one axis, Haar at its full level -- plain and DROP with both
factors): the synthesis with 32-, 16- and 8-channel workgroups as selected and as forced onto the other plane size and
stride, one and three channel groups, one cell of one plane; the adjoint with 16- and 8-channel workgroups on 32- and
64-cell tiles, the second cell group ragged and wholly empty; the masked rule, the penalty fold, the deterministic slice
mode; the streaming-store builds bit for bit against the cached ones; 7 z steps forced into 1, 2, 3 and 7 chunks bit for
bit (factor gradients, float atomics, to their bound); and C = 40 and 48 through the C ABI of the plain pair.

Worst measured ratios err / (2^-24 mag) per path are recorded in DESIGN.md (section 3.2.1); every case prints its own."""
import os

import numpy as np
import pytest
import torch

import wavelet_bound as W

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
PAD_FILL = 7.0


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))      # the fp64 oracle runs on the CPU
    return torch.device('cuda:0')


class knobs:
    """The diagnostics switches of the channel-last level for the duration of a block (kw: cw, nt, ng, nchunks)."""

    def __init__(self, **kv):
        self.kv = {W.CL_KNOBS[k]: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        for k, v in self.kv.items():
            assert k not in os.environ, k
            os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k in self.kv:
            os.environ.pop(k, None)


def check(tag, name, got, ref, mag, c, max_bound):
    """Both bounds on one tensor; prints the worst componentwise ratio."""
    got = got.detach().cpu().numpy()
    ratio = W.worst_ratio(got, ref, mag)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print('%s | %s: worst %.2f units of 2^-24 mag (bound %d), max|err| %.3g' % (tag, name, ratio, c, err))
    assert ratio <= c, (tag, name, ratio, c)
    assert err <= max_bound, (tag, name, err, max_bound)


def assert_plans(dev, case, kn, cw=None, acw=None, ng=None):
    """Both directions' plans on this device, knobs as set by the caller, against the restated rules; returns them."""
    from latent_feature_grid_compression_amd import ops
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    drop = case.ml is not None or case.mh is not None
    bdrop = drop or (case.pen is not None and (case.pen[0] != 0 or case.pen[1] != 0))
    f = ops.idwt_level_cl_plan(case.L, case.C, case.d, case.t, has_drop=drop)
    b = ops.idwt_level_cl_bwd_plan(case.L, case.C, case.d, case.t, has_drop=bdrop)
    assert vars(f) == W.cl_expected_plan(False, case.L, case.C, case.d, case.t, drop, cus, **kn), (f, cus)
    assert vars(b) == W.cl_expected_plan(True, case.L, case.C, case.d, case.t, bdrop, cus, **kn), (b, cus)
    assert cw is None or f.cw == cw, f
    assert acw is None or (b.cw, b.cells) == (acw, 32 * ng), b
    return f, b


def forward(dev, case):
    """The level through the ops wrappers -> (t0,t1,t2,Cs) on the device."""
    from latent_feature_grid_compression_amd import ops
    to = lambda x: None if x is None else x.to(dev)
    if case.ml is None and case.mh is None:
        out = ops.idwt_level_cl(to(case.lll), to(case.hf), case.frev.to(dev), case.t)
    else:
        out = ops.idwt_level_cl_drop(to(case.lll), to(case.hf), to(case.ml), case.thr, to(case.mh), case.thr, case.frev.to(dev), case.t)
    cs = (case.C + 7) // 8 * 8
    assert tuple(out.shape) == tuple(case.t) + (cs,)
    return out


def check_forward(tag, case, out):
    if out.shape[-1] > case.C:
        assert float(out[..., case.C:].abs().max()) == 0.0, (tag, 'pad channels')
    ref, mag = case.ref['out']
    check(tag, 'out', out[..., :case.C].permute(3, 0, 1, 2), ref, mag, W.c_separable(case.L // 2), 1e-6 * float(np.abs(ref).max()))


def adjoint(dev, case, deterministic=False):
    """The adjoint through the ops wrappers: the gradient grid's pad channels hold 7.0 and must be ignored."""
    from latent_feature_grid_compression_amd import ops
    to = lambda x: None if x is None else x.to(dev)
    cs = (case.C + 7) // 8 * 8
    g_cl = torch.full(tuple(case.t) + (cs,), PAD_FILL)
    g_cl[..., :case.C] = case.g.permute(1, 2, 3, 0)
    g_cl, frev_d = g_cl.to(dev), case.frev.to(dev)
    drop = case.ml is not None or case.mh is not None
    if not drop and case.pen is None:
        assert not deterministic
        return ops.idwt_level_cl_bwd(g_cl, case.C, frev_d, case.d) + (None, None)
    ptrs, keep = None, None
    if case.pen is not None:
        keep = torch.tensor(case.pen, dtype=torch.float32, device=dev)
        ptrs = [keep[i:i + 1].data_ptr() if case.pen[i] != 0 else 0 for i in range(4)]
    args = (frev_d, to(case.lll), to(case.hf), to(case.ml), to(case.mh), case.ml is not None, case.mh is not None, case.d, ptrs)
    if deterministic:
        grads = ops._adjoint(g_cl, case.C, *args, True, deterministic=True)
    else:
        grads = ops.idwt_level_cl_drop_bwd(g_cl, case.C, *args)
    torch.cuda.synchronize()
    return grads


def check_adjoint(tag, case, grads, only=None):
    c = W.c_separable(case.L // 2)
    cf = W.c_factor_gradient(c, case.C)
    for name, got, cc in (('d_lll', grads[0], c), ('d_hf', grads[1], c), ('d_ml', grads[2], cf), ('d_mh', grads[3], cf)):
        if name in case.ref:
            assert got is not None, name
            if only is None or name in only:
                ref, mag = case.ref[name]
                check(tag, name, got, ref, mag, cc, 5e-6 * max(1.0, float(np.abs(ref).max())))
        else:
            assert got is None, name


def run_row(dev, name, L, variant, pen=None, deterministic=False):
    _name, C, d, kn, cw, acw, ng = W.CL_ROW[name]
    case = W.cl_case(L, C, d, variant, pen)
    tag = '%s L=%d %s%s%s' % (name, L, variant, ' penalties' if pen else '', ' deterministic' if deterministic else '')
    with knobs(**kn):
        f, b = assert_plans(dev, case, kn, cw, acw, ng)
        print('%s | plans: synthesis cw %d x %d groups, %d tiles, %d chunks of %d; adjoint cw %d, %d cells, %d tiles, %d chunks of %d'
              % (tag, f.cw, f.ngroups, f.ptiles, f.nchunks, f.zchunk, b.cw, b.cells, b.ptiles, b.nchunks, b.zchunk))
        out = forward(dev, case)
        grads = adjoint(dev, case, deterministic)
        again = adjoint(dev, case, True) if deterministic else None
    check_forward(tag, case, out)
    check_adjoint(tag, case, grads)
    if deterministic:
        assert all(torch.equal(x, y) for x, y in zip(grads, again)), tag
    return f, b


# ---- every row, both bases, plain and with both factors ------------------------------------------------------------------

@pytest.mark.parametrize('variant', ['plain', 'drop'])
@pytest.mark.parametrize('L', [4, 2], ids=['db2', 'haar'])
@pytest.mark.parametrize('name', [r[0] for r in W.CL_ROWS])
def test_rows(dev, name, L, variant):
    run_row(dev, name, L, variant)


@pytest.mark.parametrize('L', [4, 2], ids=['db2', 'haar'])
@pytest.mark.parametrize('name', W.CL_MASKED_ROWS)
def test_rows_with_the_masked_rule(dev, name, L):
    """Threshold 0.5 on both factors: the straight-through value forward, the soft factor's gradient backward."""
    run_row(dev, name, L, 'masked')


@pytest.mark.parametrize('L', [4, 2], ids=['db2', 'haar'])
def test_row_with_penalty_fold(dev, L):
    """The L2 penalty of both coefficient tensors and the L1 penalty of both factors folded into the adjoint (three
    channel groups: the L1 term is added by group 0 only); an L2 penalty alone takes the DROP build as well."""
    _f, b = run_row(dev, 'cw8_three_groups', L, 'drop', pen=W.CL_PENALTY)
    assert b.ngroups == 3
    _f, b = run_row(dev, 'cw8_three_groups', L, 'plain', pen=[0.7, -1.3, 0.0, 0.0])
    assert b.drop


@pytest.mark.parametrize('L', [4, 2], ids=['db2', 'haar'])
@pytest.mark.parametrize('name', ['cw8_three_groups', 'cw16_stride32'])
def test_rows_deterministic_slices(dev, name, L):
    """One slice per channel group (3 of 8 channels, 2 of 16), folded in slice order: same bound, and bit-reproducible."""
    _f, b = run_row(dev, name, L, 'drop', deterministic=True)
    assert b.ngroups == {'cw8_three_groups': 3, 'cw16_stride32': 2}[name]


def test_drop_changes_the_slots_of_the_db2_adjoint(dev):
    """db2 with 32-cell tiles: the DROP build of the adjoint holds 2 instead of 3 (16 channels) and 5 instead of 6 (8
    channels) workgroups per CU, which enters the z chunking.  Both plans are asserted against the whole rule by every
    row above; here against the slot counts by name, on this device's CU count."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for name in ('cw16_stride16', 'cw8_one_group', 'cw8_three_groups', 'cw16_stride32'):
        _n, C, d, kn, _cw, acw, ng = W.CL_ROW[name]
        assert ng == 1 and not kn
        t = W.cl_target(4, d)
        for drop in (False, True):
            case = W.cl_case(4, C, d, 'drop' if drop else 'plain')
            _f, b = assert_plans(dev, case, {})
            slots = {(16, False): 3, (16, True): 2, (8, False): 6, (8, True): 5}[(acw, drop)]
            assert b.zchunk == W.cl_pick_zchunk(b.ptiles * b.ngroups, d[0], slots, cus)


# ---- streaming stores ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant', ['plain', 'drop'])
@pytest.mark.parametrize('L', [4, 2], ids=['db2', 'haar'])
@pytest.mark.parametrize('name,cw', [('cw8_one_group', 8), ('cw16_stride16', 16), ('cw32_forced_small_plane', 32)])
def test_streaming_stores_write_the_same_grid(dev, name, cw, L, variant):
    _name, C, d, kn, _cw, _acw, _ng = W.CL_ROW[name]
    case = W.cl_case(L, C, d, variant)
    outs = []
    for nt in (0, 1):
        k = dict(kn, nt=nt)
        with knobs(**k):
            f, _b = assert_plans(dev, case, k, cw)
            assert f.nt is bool(nt)
            outs.append(forward(dev, case))
    assert torch.equal(outs[0], outs[1])
    check_forward('%s L=%d %s streaming' % (name, L, variant), case, outs[1])


# ---- z chunks ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant', ['plain', 'drop'])
@pytest.mark.parametrize('L', [4, 2], ids=['db2', 'haar'])
@pytest.mark.parametrize('name,C,plane', W.CL_CHUNK_ROWS, ids=[r[0] for r in W.CL_CHUNK_ROWS])
def test_z_chunks_synthesis(dev, name, C, plane, L, variant):
    """7 cell slices in chunks of 7, 4+3, 3+3+1 and 1: every chunk after the first replays the fmaf sequence of its K - 1
    warm-up planes into the carry registers, so the four grids are equal bit for bit."""
    d = W.cl_chunk_shape(L, plane, adjoint=False)
    case = W.cl_case(L, C, d, variant, adjoint=False)
    outs = []
    for n in W.CL_NCHUNKS:
        with knobs(nchunks=n):
            f, _b = assert_plans(dev, case, {'nchunks': n}, W.CL_ROW[name][4])
            assert (f.zchunk, f.nchunks) == (-(-7 // n), n)
            outs.append(forward(dev, case))
    for n, o in zip(W.CL_NCHUNKS[1:], outs[1:]):
        assert torch.equal(outs[0], o), n
    check_forward('%s L=%d %s 3 chunks of 3+3+1' % (name, L, variant), case, outs[2])


@pytest.mark.parametrize('variant', ['plain', 'drop'])
@pytest.mark.parametrize('L', [4, 2], ids=['db2', 'haar'])
@pytest.mark.parametrize('name,C,plane', W.CL_CHUNK_ROWS, ids=[r[0] for r in W.CL_CHUNK_ROWS])
def test_z_chunks_adjoint(dev, name, C, plane, L, variant):
    """d0 = 7 coefficient planes in the same four chunkings: d_lll and d_hf bit for bit; the factor gradients are float
    atomics over the channel groups and are held to their bound in every chunking."""
    d = W.cl_chunk_shape(L, plane, adjoint=True)
    case = W.cl_case(L, C, d, variant)
    runs = []
    for n in W.CL_NCHUNKS:
        with knobs(nchunks=n):
            _f, b = assert_plans(dev, case, {'nchunks': n}, None, W.CL_ROW[name][5], 1)
            assert (b.zchunk, b.nchunks) == (-(-7 // n), n)
            runs.append(adjoint(dev, case))
    for n, r in zip(W.CL_NCHUNKS, runs):
        assert torch.equal(runs[0][0], r[0]) and torch.equal(runs[0][1], r[1]), n
        check_adjoint('%s L=%d %s adjoint %d chunks' % (name, L, variant, n), case, r, only=None if n == 3 else ('d_ml', 'd_mh'))


# ---- C > 32 through the plain pair -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('L', [4, 2], ids=['db2', 'haar'])
@pytest.mark.parametrize('C,d', W.CL_WIDE)
def test_plain_pair_takes_more_than_32_channels(dev, C, d, L):
    """include/lfgc.h: the plain pair takes any C (the drop pair refuses C > 32).  The ops wrappers never send such a
    level (nobody has timed it), so this goes through the C ABI: stride 40 = five groups of 8 in both directions, stride
    48 = six groups of 8 in the synthesis and three of 16 in the adjoint."""
    from latent_feature_grid_compression_amd import ops, _lib
    lib = _lib.load()
    assert not ops._cl_level_ok(C, d, W.cl_target(L, d), True, L)
    case = W.cl_case(L, C, d, 'plain')
    f, b = assert_plans(dev, case, {})
    assert (f.cw, f.ngroups) == (8, C // 8) and (b.cw, b.ngroups) == ((8, 5) if C == 40 else (16, 3))
    frev_d = case.frev.to(dev)
    taps = ops.filter_taps(frev_d)
    lll, hf = case.lll.to(dev).contiguous(), case.hf.to(dev).contiguous()
    out = torch.full(tuple(case.t) + (C,), SENTINEL, device=dev)
    g_cl = case.g.permute(1, 2, 3, 0).contiguous().to(dev)
    d_l, d_h = torch.full((C,) + tuple(d), SENTINEL, device=dev), torch.full((C, 7) + tuple(d), SENTINEL, device=dev)
    s = ops._stream(lll)
    assert lib.lfgc_idwt_level_cl_len_f32(lll.data_ptr(), hf.data_ptr(), taps, L, out.data_ptr(), C, C, *d, *case.t, s) == 0
    assert lib.lfgc_idwt_level_cl_bwd_len_f32(g_cl.data_ptr(), taps, L, d_l.data_ptr(), d_h.data_ptr(), C, C, *d, *case.t, s) == 0
    torch.cuda.synchronize()
    tag = 'wide C=%d L=%d' % (C, L)
    check_forward(tag, case, out)
    check_adjoint(tag, case, (d_l, d_h, None, None))
    # the drop pair refuses the same level on the host, nothing launched
    nan = float('nan')
    ml = torch.ones(tuple(d), device=dev)
    keep = out.clone()
    assert lib.lfgc_idwt_level_cl_drop_len_f32(lll.data_ptr(), hf.data_ptr(), ml.data_ptr(), nan, None, nan, taps, L, out.data_ptr(),
                                               C, C, *d, *case.t, s) == -3
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
