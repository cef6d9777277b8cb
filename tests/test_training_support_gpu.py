"""GPU tests of the small kernels that run around every training step (csrc/lfgc_drop.hip, csrc/lfgc_misc.hip), each at
the sizes where its launch changes shape -- one element, a wave, a workgroup +-1, the cap of its grid so that the grid-stride
loop takes a second pass, 16 terms or layers in one launch -- against the references of tests/training_support_ref.py, which
tests/test_training_support_host.py pins on the CPU.  Every output the caller owns is a prefix of a larger buffer whose tail
holds a sentinel bit pattern that must survive; "bit for bit" compares uint32 / uint64 views, so signed zeros count (and NaNs
compare equal: where the drop layer's reference is a NaN the kernel must give a NaN, of whatever sign and payload).

1. penalty sums (one fp32 ulp of the exactly rounded fp64 sum, and for L1 / L2 n 2^-53 of it in fp64 through the C-ABI)
   at every size on tensors whose sum is of order n, so that every element shows in it, and again on the same tensors with
   +-3e19 in them, where the L2 sum stays finite in fp64 while its fp32 rounding is +inf by definition; gradients (L1, L2
   bit for bit; D_KL to one fp32 ulp of the fp64 derivative + the smallest denormal); 16 terms in one launch equal 16
   launches.
2. the Smallify sign-variance tracker, single and 16-layer launch, bit for bit with oracle/ref_drop.py on CPU tensors over
   three steps, betas including +-0, denormals, +-inf and NaNs of both signs.
3. the stand-alone drop layer: value and d_x bit for bit, d_mul within C 2^-24 sum |g x| of fp64.
4. the slice fold, bit for bit with a sequential fp32 accumulation.
5. the ground-truth sampler and the fused MSE, bit for bit with oracle/ref_torch.py's trilinear_f_interpolation on the CPU.
6. the deviation statistics: sums within n 2^-52 of exactly rounded fp64 sums, min / max exact, accumulation across calls.
7. the lattice kernels on lattices of 3.38e9 and 6.76e9 voxels and with a draw counter beyond 2^32.

Kernel and wrapper changes these tests led to:
* sign_variance_kernel / sign_variance_multi_kernel returned NaN for a NaN beta; the reference's torch.sign gives 0, so
  they now compute (b > 0) - (b < 0) for every input.
* penalty_grads_kernel formed sigmoid' as s (1 - s); 1 - s as an fp64 difference costs the D_KL gradient its fp32 accuracy
  in the upper tail (1.1 of the bound at log alpha = 30, 20 at 24: test_training_support_host.py).  It now computes
  e / (1 + e)^2 with e = exp(-|x|).
* ops.deviation_partial, lattice_sample, lattice_positions and gt_interp raised on an empty batch (an empty tensor's
  address is NULL, which the entries refuse before they look at n); they now return without a launch.

Worst observed error as a fraction of its bound, MI355X (each test prints its own):
  penalty sums: fp32 0 (the same fp32 as the exactly rounded sum at every size and kind); fp64 L1 / L2 without +-3e19
  1.1e-3 at most (L2, n = 1025), 1.3e-6 at most beyond the grid cap, 0 at 27 of the 33 cases; with +-3e19 1.2e-6 at most;
  16 terms on one tensor 0; D_KL gradients 0.50 (the final rounding to fp32), 16 mixed terms 0.50; drop d_mul 0.97 at C = 1 (one rounding against a half-ulp bound), 0.61
  at C = 3, 0.095 at C = 32; fused MSE loss 0; deviation sums 0.011 at most (n = 64), 4e-5 beyond the grid cap.  The rest is
  bit for bit.  The tracker's reference gave 0 for a NaN beta on the GPU machine's torch as well."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import training_support_ref as R
from oracle import ref_drop as D
from oracle import ref_torch as T
from test_hip_forward import dev  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5                  # a quiet NaN with a payload no kernel produces
TAIL = 64
WAVE_SIZES = [1, 255, 256, 257, 1000]


def _api():
    from latent_feature_grid_compression_amd import _lib, ops
    return _lib.load(), _lib, ops


def canaried(n, dtype=torch.float32):
    """(prefix view of n elements, whole buffer): the buffer is TAIL elements longer and holds SENTINEL in every 32-bit word."""
    words = 2 if dtype in (torch.float64, torch.int64) else 1
    buf = torch.full(((n + TAIL) * words,), SENTINEL, dtype=torch.int32, device='cuda').view(dtype)
    return buf[:n], buf


def tail_intact(buf, n):
    tail = buf[n:].contiguous().view(torch.int32).cpu().numpy()
    return tail.size >= TAIL and bool((tail == SENTINEL).all())


def dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.itemsize == 8:
        return a.shape == b.shape and np.array_equal(R.bits64(a), R.bits64(b))
    return a.shape == b.shape and np.array_equal(R.bits32(a), R.bits32(b))


def same_bits_or_both_nan(got, want):
    """Bit for bit where the reference is a number; a NaN (of any sign and payload: IEEE 754 leaves both to the hardware,
    and x86 and gfx950 choose differently) exactly where the reference has one."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and same_bits(got[~nan], want[~nan])


# ---- 1. penalties ---------------------------------------------------------------------------------------------------------

WEIGHTS = {R.L1: -0.75, R.L2: 1.5, R.DKL: 0.37}


@functools.lru_cache(maxsize=None)
def term_inputs(kind, n, huge=False):
    """`huge`: the L1 / L2 tensor with +-3e19 in it.  Its sum checks that the accumulator is fp64 and cannot see anything
    else (one fp64 ulp of 6e19 is 8192), so every size is run on the tensor without them as well."""
    a, b = R.penalty_inputs(kind, n, huge=huge)
    return a, b, dev_f32(a), (dev_f32(b) if b is not None else None)


def capi_penalty(specs, weights, extra_doubles=8):
    """lfgc_penalty_sums_f32 + lfgc_penalty_grads_f32 on caller-owned buffers.  specs: [(kind, a_dev, b_dev)].  Returns the
    fp64 sums, [(grad_a, grad_b)] as host arrays, and whether every canary survived."""
    lib, _lib, ops = _api()
    k = len(specs)
    terms = (_lib.PenaltyTerm * k)()
    for t, (kind, a, b) in enumerate(specs):
        terms[t].a, terms[t].b, terms[t].n, terms[t].kind = a.data_ptr(), (b.data_ptr() if b is not None else None), a.numel(), kind
    doubles = k * (1 + _lib.PENALTY_BLOCKS)
    sums_all = torch.full(((doubles + extra_doubles) * 2,), SENTINEL, dtype=torch.int32, device='cuda').view(torch.float64)
    _lib.check(lib.lfgc_penalty_sums_f32(terms, k, sums_all.data_ptr(), stream()), 'lfgc_penalty_sums_f32')
    intact = bool((sums_all[doubles:].view(torch.int32).cpu().numpy() == SENTINEL).all()) and extra_doubles >= 8
    d_sums = dev_f32(weights)
    ga = [canaried(a.numel()) for _, a, _ in specs]
    gb = [canaried(a.numel()) if kind == R.DKL else None for kind, a, _ in specs]
    pa, _k1 = _lib.ptr_array([g[0].data_ptr() for g in ga])
    pb, _k2 = _lib.ptr_array([g[0].data_ptr() if g is not None else 0 for g in gb])
    _lib.check(lib.lfgc_penalty_grads_f32(terms, k, d_sums.data_ptr(), pa, pb, stream()), 'lfgc_penalty_grads_f32')
    grads = []
    for (kind, a, _), g_a, g_b in zip(specs, ga, gb):
        intact = intact and tail_intact(g_a[1], a.numel()) and (g_b is None or tail_intact(g_b[1], a.numel()))
        grads.append((host(g_a[0]), host(g_b[0]) if g_b is not None else None))
    return host(sums_all[:k]), grads, intact, host(sums_all[:doubles])


def ops_penalty(specs, weights):
    """The same through ops.PenaltyFn: fp32 sums and the gradients autograd hands back."""
    _, _, ops = _api()
    tensors = []
    for kind, a, b in specs:
        tensors += [a.clone().requires_grad_(True)] + ([b.clone().requires_grad_(True)] if kind == R.DKL else [])
    out = ops.penalty_sums([kind for kind, _, _ in specs], tensors)
    out.backward(dev_f32(weights))
    it = iter(tensors)
    grads = []
    for kind, _, _ in specs:
        g_a = host(next(it).grad)
        grads.append((g_a, host(next(it).grad) if kind == R.DKL else None))
    return host(out), grads


@functools.lru_cache(maxsize=None)
def single_term(kind, n, weight, huge=False):
    """One term launched alone, through the C-ABI and through ops (which must agree bit for bit)."""
    _, _, a, b = term_inputs(kind, n, huge)
    sums64, grads, intact, _ = capi_penalty([(kind, a, b)], [weight])
    sums32, grads_ops = ops_penalty([(kind, a, b)], [weight])
    assert intact
    with np.errstate(over='ignore'):
        assert same_bits(sums32, sums64.astype(np.float32))
    assert same_bits(grads[0][0], grads_ops[0][0]) and (kind != R.DKL or same_bits(grads[0][1], grads_ops[0][1]))
    return sums64[0], sums32[0], grads[0]


@functools.lru_cache(maxsize=None)
def reference_sums(kind, n, huge=False):
    a, b, _, _ = term_inputs(kind, n, huge)
    return R.penalty_sum64(kind, a, b), R.penalty_sum(kind, a, b)


def check_sum(kind, n, sum64, sum32, huge=False):
    """-> the worst error as a fraction of its bound."""
    a = term_inputs(kind, n, huge)[0]
    ref64, ref32 = reference_sums(kind, n, huge)
    assert np.isfinite(sum64)
    frac = 0.0
    if np.isfinite(ref32):
        assert np.isfinite(sum32)
        frac = abs(float(sum32) - float(ref32)) / (R.ULP32 * abs(float(ref32))) if ref32 != 0 else float(sum32 != 0)
    else:       # an L2 term holding 3e19: the exactly rounded fp32 sum IS +inf; the kernel's fp64 sum must not be
        assert kind == R.L2 and huge and np.abs(a).max() > 1e19 and same_bits(np.float32(sum32), ref32)
    assert frac <= 1.0, (kind, n, sum32, ref32)
    if kind != R.DKL:       # exact fp64 terms: only the n - 1 additions round
        f64 = abs(sum64 - ref64) / (n * 2.0 ** -53 * ref64) if ref64 else float(sum64 != 0)
        assert f64 <= 1.0, (kind, n, sum64, ref64)
        frac = max(frac, f64)
    return frac


def check_grads(kind, n, weight, grads, huge=False):
    a, b, _, _ = term_inputs(kind, n, huge)
    ref_a, ref_b = R.penalty_grads(kind, a, b, weight)
    assert np.isfinite(grads[0]).all()                                  # L2 of 3e19 too: 2 g v = 9e19 is an fp32
    if kind != R.DKL:
        assert grads[1] is None and same_bits(grads[0], ref_a)
        return 0.0
    frac = 0.0
    for got, ref in zip(grads, (ref_a, ref_b)):
        assert np.isfinite(got).all()
        f = np.abs(got.astype(np.float64) - ref) / R.dkl_grad_bound(ref)
        assert f.max() <= 1.0, (n, int(f.argmax()), got[f.argmax()], ref[f.argmax()])
        frac = max(frac, float(f.max()))
    return frac


@pytest.mark.parametrize('n', R.SUM_SIZES)
@pytest.mark.parametrize('kind', [R.L1, R.L2, R.DKL], ids=lambda k: R.KIND_NAMES[k])
def test_penalty_sum_every_launch_shape(dev, kind, n):
    """n > 1024*1024 gives penalty_sums_kernel's grid-stride loop its second pass (1024 workgroups of 1024 elements).  The
    L1 / L2 tensors hold no +-3e19 here: the sum is of order n, the fp64 bound n 2^-53 ref far below one ordinary term, so an
    element lost in a tail or a pass, or an fp32 accumulator, shows."""
    sum64, sum32, _ = single_term(kind, n, WEIGHTS[kind])
    assert np.isfinite(sum32)
    frac = check_sum(kind, n, sum64, sum32)
    print('penalty sum %s n=%d: %.3g of the bound' % (R.KIND_NAMES[kind], n, frac))


@pytest.mark.parametrize('n', R.SUM_SIZES[1:])
@pytest.mark.parametrize('kind', [R.L1, R.L2], ids=lambda k: R.KIND_NAMES[k])
def test_penalty_sum_is_taken_in_fp64(dev, kind, n):
    """The same tensors with +-3e19 in them: 3e19^2 is beyond fp32, so the L2 sum is finite only in an fp64 accumulator
    (and +inf once rounded to fp32, as the exactly rounded sum is).  These sums see +-3e19 and nothing else."""
    sum64, sum32, _ = single_term(kind, n, WEIGHTS[kind], True)
    frac = check_sum(kind, n, sum64, sum32, True)
    print('penalty sum with +-3e19 %s n=%d: %.3g of the bound' % (R.KIND_NAMES[kind], n, frac))


@pytest.mark.parametrize('n', R.GRAD_SIZES)
@pytest.mark.parametrize('kind', [R.L1, R.L2, R.DKL], ids=lambda k: R.KIND_NAMES[k])
def test_penalty_gradients_every_launch_shape(dev, kind, n):
    """n > 2048*256 gives penalty_grads_kernel's loop its second pass.  Per element, so +-3e19 hides nothing: L1 / L2 run
    on the tensors that hold them."""
    huge = kind != R.DKL
    for weight in (WEIGHTS[kind], 0.0):
        sum64, sum32, grads = single_term(kind, n, weight, huge)
        frac = check_grads(kind, n, weight, grads, huge)
        check_sum(kind, n, sum64, sum32, huge)
        print('penalty gradient %s n=%d g=%g: %.3g of the bound' % (R.KIND_NAMES[kind], n, weight, frac))


# (kind, n, upstream weight, +-3e19 in the tensor)
MIXED = [(R.L1, 257, -0.75, False), (R.DKL, 255, 0.37, False), (R.L2, 1, 1.5, False), (R.L2, (1 << 20) + 1025, 0.0, False),
         (R.L1, 1, 0.0, False), (R.DKL, 524289, -1.25, False), (R.L2, 256, -2.0, True), (R.L1, 1 << 20, 0.3, False),
         (R.DKL, 1, 0.0, False), (R.L1, 1025, -0.75, True), (R.L2, 4097, 1.5, False), (R.DKL, 257, 0.37, False),
         (R.L1, 1023, 2.0, False), (R.L2, 524288 + 257, 1.5, True), (R.DKL, 1024, -1.25, False), (R.L2, 255, 0.5, False)]


def test_sixteen_mixed_terms_in_one_launch_equal_sixteen_launches(dev):
    """The block_start mapping with LFGC_PENALTY_MAX_TERMS terms of mixed kinds and unequal sizes: every result equals the
    same term launched alone (and so the reference), and a second launch repeats the first bit for bit."""
    assert len(MIXED) == 16
    specs = [(kind,) + term_inputs(kind, n, huge)[2:] for kind, n, _, huge in MIXED]
    weights = [w for _, _, w, _ in MIXED]
    sums64, grads, intact, everything = capi_penalty(specs, weights)
    assert intact
    sums32, grads_ops = ops_penalty(specs, weights)
    worst = 0.0
    for t, (kind, n, w, huge) in enumerate(MIXED):
        alone64, alone32, alone_grads = single_term(kind, n, w, huge)
        assert same_bits(sums64[t], alone64) and same_bits(sums32[t], alone32), (t, kind, n)
        for got in (grads[t], grads_ops[t]):
            assert same_bits(got[0], alone_grads[0]) and (kind != R.DKL or same_bits(got[1], alone_grads[1])), (t, kind, n)
        worst = max(worst, check_sum(kind, n, alone64, alone32, huge), check_grads(kind, n, w, alone_grads, huge))
    again64, again_grads, intact, everything2 = capi_penalty(specs, weights)
    assert intact and same_bits(everything, everything2)                # results and per-workgroup partials alike
    for a, b in zip(grads, again_grads):
        assert same_bits(a[0], b[0]) and (a[1] is None or same_bits(a[1], b[1]))
    print('16 mixed penalty terms: %.3g of the bound' % worst)


def test_sixteen_full_terms_fill_the_scratch_to_its_last_double(dev):
    """16 terms on one tensor of 2^20 + 1 elements: 16 x 1024 workgroups, so the partials reach the last double of
    LFGC_PENALTY_SUMS_DOUBLES(16) -- and stop there."""
    lib, _lib, _ = _api()
    n = (1 << 20) + 1
    _, _, a, _ = term_inputs(R.L1, n)
    kinds = [R.L1 if t % 2 else R.L2 for t in range(16)]
    sums64, grads, intact, everything = capi_penalty([(k, a, None) for k in kinds], [1.0] * 16)
    assert intact and everything.size == 16 * (1 + _lib.PENALTY_BLOCKS) == 16400
    assert not (everything.view(np.uint32) == SENTINEL).any()           # every double up to the last was written
    alone = {kind: capi_penalty([(kind, a, None)], [1.0])[0][0] for kind in (R.L1, R.L2)}
    ref = {kind: R.penalty_sum64(kind, term_inputs(R.L1, n)[0]) for kind in (R.L1, R.L2)}
    worst = 0.0
    for t, kind in enumerate(kinds):                                    # the tensor holds no +-3e19: the bound sees every element
        assert same_bits(sums64[t], alone[kind]), t
        worst = max(worst, abs(sums64[t] - ref[kind]) / (n * 2.0 ** -53 * ref[kind]))
        if t >= 2:
            assert same_bits(grads[t][0], grads[t - 2][0])
    assert 0.5 * n < ref[R.L1] < n and worst <= 1.0
    print('16 full penalty terms: %.3g of the bound' % worst)


# ---- 2. sign-variance tracker --------------------------------------------------------------------------------------------------

def tracker_betas(n, step, seed=0):
    rng = np.random.default_rng(17 * n + step + 7919 * seed)
    b = rng.standard_normal(n).astype(np.float32)
    edge = np.array([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf], np.float32)
    edge = np.concatenate([edge, np.array([0x7FC00000, 0xFFC00000, 0x7F800001], np.uint32).view(np.float32)])
    # first in line, and so the only edge value at n = 1: 0.0 at step 0, the positive NaN at step 1, the negative at step 2
    order = np.roll(np.arange(edge.size), (0, 3, 2)[step % 3])
    assert (step % 3 == 0) == (not np.isnan(edge[order[0]])) and (step % 3 == 2) == bool(np.signbit(edge[order[0]]))
    k = min(edge.size, n)
    b[(np.arange(k) * 29) % n] = edge[order][:k]
    return b


def tracker_reference(layers, momentum, steps=3):
    """[(ema, emavar)] per layer after `steps` steps of oracle/ref_drop.py on CPU tensors; state starts as the tracker's."""
    out = []
    for n, seed in layers:
        ema, emavar = D.sign_variance_init(torch.from_numpy(tracker_betas(n, 0, seed)))
        emavar = emavar + 0.125
        for s in range(steps):
            ema, emavar = D.sign_variance_update(ema, emavar, torch.from_numpy(tracker_betas(n, s, seed)), momentum)
        out.append((ema.numpy(), emavar.numpy()))
    return out


def tracker_state(layers):
    state = []
    for n, seed in layers:
        ema0, var0 = D.sign_variance_init(torch.from_numpy(tracker_betas(n, 0, seed)))
        e, eb = canaried(n)
        v, vb = canaried(n)
        e.copy_(ema0.cuda())
        v.copy_((var0 + 0.125).cuda())
        state.append((e, eb, v, vb))
    return state


@pytest.mark.parametrize('momentum', [0.025, 0.0, 1.0])
@pytest.mark.parametrize('n', WAVE_SIZES)
def test_tracker_single_launch_bit_for_bit(dev, n, momentum):
    _, _, ops = _api()
    (e, eb, v, vb), = tracker_state([(n, 0)])
    for s in range(3):
        ops.sign_variance_update(dev_f32(tracker_betas(n, s)), e, v, momentum)
        (re, rv), = tracker_reference([(n, 0)], momentum, s + 1)
        assert same_bits(host(e), re) and same_bits(host(v), rv), (n, momentum, s)
        assert np.isfinite(re).all() and np.isfinite(rv).all()          # a NaN beta does not reach the state
    assert tail_intact(eb, n) and tail_intact(vb, n)


@pytest.mark.parametrize('n_layers', [16, 2])
@pytest.mark.parametrize('momentum', [0.025, 1.0])
def test_tracker_multi_launch_equals_single_launches(dev, n_layers, momentum):
    """16 layers with sizes cycling through 1, 255, 256, 257, 1000: the block_start lookup at every boundary."""
    _, _, ops = _api()
    layers = [(WAVE_SIZES[t % len(WAVE_SIZES)], t) for t in range(n_layers)]
    multi, single = tracker_state(layers), tracker_state(layers)
    for s in range(3):
        betas = [dev_f32(tracker_betas(n, s, seed)) for n, seed in layers]
        ops.sign_variance_update_multi(betas, [m[0] for m in multi], [m[2] for m in multi], momentum)
        for b, st in zip(betas, single):
            ops.sign_variance_update(b, st[0], st[2], momentum)
        ref = tracker_reference(layers, momentum, s + 1)
        for t, (m, st, (re, rv)) in enumerate(zip(multi, single, ref)):
            assert same_bits(host(m[0]), host(st[0])) and same_bits(host(m[2]), host(st[2])), (t, s)
            assert same_bits(host(m[0]), re) and same_bits(host(m[2]), rv), (t, s)
    for (n, _), m in zip(layers, multi):
        assert tail_intact(m[1], n) and tail_intact(m[3], n)


# ---- 3. stand-alone drop layer ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('thr', [None, 0.5])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1021])
@pytest.mark.parametrize('C', [1, 3, 32])
def test_drop_layer_value_and_gradients(dev, C, n, thr):
    lib, _lib, ops = _api()
    x, mul, g = R.drop_inputs(C, n, thr)
    want = R.drop_value(x, mul, thr)
    want_dx, want_dm, bound = R.drop_grads(x, mul, g)
    worst = 0.0
    for need_dm in (True, False):
        tx, tm = dev_f32(x).requires_grad_(True), dev_f32(mul).requires_grad_(need_dm)
        out = ops.DropApplyFn.apply(tx, tm, thr)
        assert same_bits_or_both_nan(host(out), want)
        out.backward(dev_f32(g))
        assert same_bits_or_both_nan(host(tx.grad), want_dx)
        if need_dm:
            err = np.abs(host(tm.grad).astype(np.float64) - want_dm)
            ok = np.isfinite(want_dm)
            assert (err[ok] <= bound[ok]).all() and np.isfinite(host(tm.grad)[ok]).all()
            worst = max(worst, float((err[ok] / bound[ok]).max()))
        else:
            assert tm.grad is None
    # the entries on caller-owned buffers: the same bits, and nothing past the last element
    dx, dm, dg = dev_f32(x), dev_f32(mul), dev_f32(g)
    o, ob = canaried(C * n)
    thr_c = float('nan') if thr is None else thr
    _lib.check(lib.lfgc_drop_apply_f32(dx.data_ptr(), dm.data_ptr(), thr_c, o.data_ptr(), C, n, stream()), 'lfgc_drop_apply_f32')
    assert same_bits_or_both_nan(host(o).reshape(C, n), want)
    assert tail_intact(ob, C * n)
    for need_dm in (True, False):
        gx, gxb = canaried(C * n)
        gm, gmb = canaried(n)
        _lib.check(lib.lfgc_drop_apply_bwd_f32(dg.data_ptr(), dx.data_ptr(), dm.data_ptr(), gx.data_ptr(),
                                               gm.data_ptr() if need_dm else None, C, n, stream()), 'lfgc_drop_apply_bwd_f32')
        assert same_bits_or_both_nan(host(gx).reshape(C, n), want_dx) and tail_intact(gxb, C * n)
        if need_dm:
            assert same_bits(host(gm), host(tm_grad_of(ops, x, mul, g, thr))) and tail_intact(gmb, n)
        else:
            assert tail_intact(gmb, 0)                                  # NULL d_mul: the buffer was never handed over
    print('drop d_mul C=%d n=%d: %.3g of the bound' % (C, n, worst))


def tm_grad_of(ops, x, mul, g, thr):
    tx, tm = dev_f32(x).requires_grad_(True), dev_f32(mul).requires_grad_(True)
    ops.DropApplyFn.apply(tx, tm, thr).backward(dev_f32(g))
    return tm.grad


# ---- 4. slice fold ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('gap', [0, 3])
@pytest.mark.parametrize('n', WAVE_SIZES)
@pytest.mark.parametrize('nslices', [1, 2, 7, 32])
def test_slice_fold_bit_for_bit(dev, nslices, n, gap):
    lib, _lib, _ = _api()
    stride = n + gap
    rng = np.random.default_rng(100 * nslices + n + gap)
    buf = np.full(nslices * stride, np.nan, np.float32)
    for s in range(nslices):                                            # magnitudes that differ: the order of the adds shows
        buf[s * stride:s * stride + n] = rng.standard_normal(n).astype(np.float32) * np.float32(4.0 ** (s % 9))
    d = dev_f32(buf)
    out, ob = canaried(n)
    _lib.check(lib.lfgc_sum_slices_f32(d.data_ptr(), nslices, stride, n, out.data_ptr(), stream()), 'lfgc_sum_slices_f32')
    want = R.sum_slices(buf, nslices, stride, n)
    assert np.isfinite(want).all() and same_bits(host(out), want) and tail_intact(ob, n)
    assert same_bits(host(d), buf)                                      # the slices were left alone


# ---- 5. ground-truth sampler and fused MSE ----------------------------------------------------------------------------------------

VOLUMES = [(2, 2, 2), (5, 7, 3), (20, 21, 22)]
BOXES = ['origin', 'offset']


def box_of(shape, box):
    if box == 'origin':
        return np.zeros(3, np.float32), np.asarray(shape, np.float32) - 1
    return np.float32([-0.75, 0.3, 1.1]), np.float32([1.25, 2.9, 3.6])


@functools.lru_cache(maxsize=None)
def gt_case(shape, box, n):
    """Positions inside the box (every lattice point, points one ulp to either side of lattice coordinates, uniform ones),
    the reference's ground truth for them on the CPU, and a prediction."""
    rng = np.random.default_rng(sum(shape) * 31 + n + (box == 'offset'))
    f = rng.standard_normal(shape).astype(np.float32)
    mn, mx = box_of(shape, box)
    res = np.asarray(shape, np.float32)
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    lattice = (mn + (idx / (res - 1)) * (mx - mn)).astype(np.float32)
    near = np.concatenate([np.nextafter(lattice, np.float32(np.inf)), np.nextafter(lattice, np.float32(-np.inf))])
    uniform = (mn + rng.uniform(0, 1, (max(n, 64), 3)).astype(np.float32) * (mx - mn)).astype(np.float32)
    p = np.concatenate([lattice, near, uniform])
    group = np.repeat([0, 1, 2], [len(lattice), len(near), len(uniform)])
    # the reference is defined where its own fp32 lattice coordinate stays inside the volume
    tp = torch.from_numpy(p)
    norm = (((tp - torch.from_numpy(mn)) / (torch.from_numpy(mx) - torch.from_numpy(mn))) * (torch.from_numpy(res) - 1)).numpy()
    inside = ((norm >= 0) & (norm <= res - 1)).all(1)
    p, group = p[inside], group[inside]
    assert len(p) >= len(lattice) // 2 and (p[:, 0] == mx[0]).any()          # the last index of an axis is among them
    order = rng.permutation(len(p))                                     # every size gets the mix, not the first lattice points
    p, group = p[order], group[order]
    if n >= 255:        # still there after the cut: lattice points, one with a last index; their neighbours; uniform points
        assert set(group[:n].tolist()) == {0, 1, 2} and (p[:n][group[:n] == 0] == mx).any()
    p = np.ascontiguousarray(np.resize(p, (n, 3)) if n > len(p) else p[:n])
    gt = T.trilinear_f_interpolation(torch.from_numpy(p), torch.from_numpy(f), torch.from_numpy(mn), torch.from_numpy(mx),
                                     torch.from_numpy(res)).numpy()
    pred = (gt + rng.standard_normal(n).astype(np.float32) * np.float32(0.1)).astype(np.float32)
    return f, mn, mx, res, p, gt, pred


@pytest.mark.parametrize('n', [1, 255, 256, 257, 65537])
@pytest.mark.parametrize('box', BOXES)
@pytest.mark.parametrize('shape', VOLUMES, ids=lambda s: 'x'.join(map(str, s)))
def test_ground_truth_and_fused_mse(dev, shape, box, n):
    """n = 65537 gives 257 partials: the second pass of mse_fold_kernel."""
    lib, _lib, ops = _api()
    f, mn, mx, res, p, gt, pred = gt_case(shape, box, n)
    assert np.isfinite(gt).all()
    dp, df, dpred = dev_f32(p), dev_f32(f), dev_f32(pred)
    assert same_bits(host(ops.gt_interp(dp, df, mn, mx, res)), gt)
    # the fused entry on caller-owned buffers
    gt_out, gt_buf = canaried(n)
    d_pred, d_buf = canaried(n)
    loss, loss_buf = canaried(1)
    ws_bytes = int(lib.lfgc_gt_mse_workspace_bytes(n))
    assert ws_bytes == (n + 255) // 256 * 8
    ws, ws_buf = canaried(ws_bytes // 8, torch.float64)
    _lib.check(lib.lfgc_gt_mse_f32(dp.data_ptr(), df.data_ptr(), f3(mn), f3(mx), f3(res), n, shape[0], shape[1], shape[2],
                                   dpred.data_ptr(), gt_out.data_ptr(), d_pred.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                   ws_bytes, stream()), 'lfgc_gt_mse_f32')
    want_d, want_loss = R.mse_reference(pred, gt)
    assert same_bits(host(gt_out), gt) and same_bits(host(d_pred), want_d)
    frac = abs(float(host(loss)[0]) - float(want_loss)) / (R.ULP32 * float(want_loss))
    assert frac <= 1.0 and np.isfinite(host(loss)[0])
    assert tail_intact(gt_buf, n) and tail_intact(d_buf, n) and tail_intact(loss_buf, 1) and tail_intact(ws_buf, ws_bytes // 8)
    # the autograd node: the same loss, and its gradient under the unit seed and under a seed of 3
    for seed in ('unit', 3.0):
        tpred = dev_f32(pred).requires_grad_(True)
        node = ops.gt_mse_loss(tpred, dp, df, mn.tolist(), mx.tolist(), res.tolist())
        assert same_bits(host(node), host(loss)[0])
        if seed == 'unit':
            node.backward(ops.unit_grad(dev))
            assert same_bits(host(tpred.grad), want_d)
        else:
            node.backward(torch.tensor(seed, device=dev))
            assert same_bits(host(tpred.grad), want_d * np.float32(seed))
    print('fused MSE loss %s %s n=%d: %.3g of the bound' % (shape, box, n, frac))


def test_ground_truth_of_an_empty_batch(dev):
    _, _, ops = _api()
    f, mn, mx, res, p, gt, pred = gt_case((5, 7, 3), 'origin', 1)
    out = ops.gt_interp(dev_f32(p)[:0], dev_f32(f), mn, mx, res)
    assert out.shape == (0,) and out.is_cuda


# ---- 6. deviation statistics ---------------------------------------------------------------------------------------------------

DEV_SIZES = [1, 63, 64, 65, 255, 256, 257, 262144, 262145, 262144 + 257, 1 << 20]
GT_KINDS = ['mixed', 'negative', 'constant']


@functools.lru_cache(maxsize=None)
def deviation_case(n, kind):
    rng = np.random.default_rng(n + 7 * GT_KINDS.index(kind))
    gt = rng.standard_normal(n).astype(np.float32)
    if kind == 'negative':
        gt = -np.abs(gt) - np.float32(0.5)
    elif kind == 'constant':
        gt = np.full(n, -1.75, np.float32)
    pred = (gt + rng.standard_normal(n).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    return pred, gt, R.deviation(pred, gt)


def check_deviation(acc, ref, n):
    assert same_bits(acc[2:], ref[2:])                                  # min and max: exact
    frac = np.abs(acc[:2] - ref[:2]) / (n * 2.0 ** -52 * ref[:2])
    assert (frac <= 1.0).all(), (acc, ref)
    return float(frac.max())


@pytest.mark.parametrize('kind', GT_KINDS)
@pytest.mark.parametrize('n', DEV_SIZES)
def test_deviation_partial_every_launch_shape(dev, n, kind):
    """n > 1024*256 gives deviation_kernel's grid-stride loop its second pass; an all-negative ground truth sends negative
    doubles through the compare-and-swap minimum and maximum."""
    _, _, ops = _api()
    pred, gt, ref = deviation_case(n, kind)
    acc = ops.deviation_partial(dev_f32(pred), dev_f32(gt))
    frac = check_deviation(host(acc), ref, n)
    print('deviation sums n=%d %s: %.3g of the bound' % (n, kind, frac))


def test_deviation_accumulates_into_a_passed_in_acc(dev):
    lib, _lib, ops = _api()
    parts = [deviation_case(262145, 'negative'), deviation_case(257, 'mixed'), deviation_case(1, 'constant')]
    acc, buf = canaried(4, torch.float64)
    acc.copy_(torch.tensor([0.0, 0.0, float('inf'), float('-inf')], dtype=torch.float64))
    for pred, gt, _ in parts:
        assert ops.deviation_partial(dev_f32(pred), dev_f32(gt), acc).data_ptr() == acc.data_ptr()
    pred, gt = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    ref = R.deviation(pred, gt)
    check_deviation(host(acc), ref, pred.size)
    one = ops.deviation_partial(dev_f32(pred), dev_f32(gt))
    check_deviation(host(one), ref, pred.size)
    # n = 0 leaves acc alone: through ops (an empty tensor) and through the entry (valid pointers, n = 0)
    before = host(acc).copy()
    ops.deviation_partial(dev_f32(pred)[:0], dev_f32(gt)[:0], acc)
    dp = dev_f32(pred)
    _lib.check(lib.lfgc_deviation_partial_f32(dp.data_ptr(), dp.data_ptr(), 0, acc.data_ptr(), stream()), 'lfgc_deviation_partial_f32')
    assert same_bits(host(acc), before) and tail_intact(buf, 4)
    fresh = ops.deviation_partial(dev_f32(pred)[:0], dev_f32(gt)[:0])
    assert host(fresh).tolist() == [0.0, 0.0, float('inf'), float('-inf')]


def test_calculate_deviation_statistics_against_the_oracle(dev):
    from latent_feature_grid_compression_amd.visualization import OutputToVTK as V
    for kind in GT_KINDS[:2]:
        pred, gt, _ = deviation_case(262145, kind)
        got = V.calculate_deviation_statistics(dev_f32(pred), dev_f32(gt), verbose=False)
        want = T.deviation_statistics(torch.from_numpy(pred), torch.from_numpy(gt))
        assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)


# ---- 7. lattice kernels beyond 2^31 and 2^32 voxels -----------------------------------------------------------------------------

BIG = [(2049, 1500, 1100), (4099, 1500, 1100)]


@functools.lru_cache(maxsize=None)
def dataset(res):
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    ds = IndexDataset(res, 16, build_index_table=False)
    assert ds.volume_indices is None and ds.n_voxels == res[0] * res[1] * res[2]
    return ds, ds.min_idx.tolist(), ds.max_idx.tolist(), ds.scales.tolist()


def r3(res):
    return (ctypes.c_int32 * 3)(*[int(v) for v in res])


def f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


@pytest.mark.parametrize('res', BIG, ids=lambda s: 'x'.join(map(str, s)))
def test_lattice_positions_of_64_bit_flat_indices(dev, res):
    lib, _lib, ops = _api()
    ds, mn, mx, sc = dataset(res)
    assert ds.n_voxels > (1 << 31) and (res[0] < 4000 or ds.n_voxels > (1 << 32))
    flat = R.lattice_flat_indices(res)
    raw_t, norm_t = ds.positions_for(ds.lattice_from_flat(torch.from_numpy(flat)))
    d_flat = torch.from_numpy(flat).cuda()
    raw, norm = ops.lattice_positions(d_flat, res, mn, mx, sc)
    assert same_bits(host(raw), raw_t.numpy()) and same_bits(host(norm), norm_t.numpy())
    raw_d, norm_d = ds.positions_from_flat(d_flat)                      # the dataset's own route to the same kernel
    assert same_bits(host(raw_d), raw_t.numpy()) and same_bits(host(norm_d), norm_t.numpy())
    n = flat.size
    raw_c, raw_buf = canaried(3 * n)
    norm_c, norm_buf = canaried(3 * n)
    _lib.check(lib.lfgc_lattice_positions_f32(d_flat.data_ptr(), n, r3(res), f3(mn), f3(mx), f3(sc), raw_c.data_ptr(),
                                              norm_c.data_ptr(), stream()), 'lfgc_lattice_positions_f32')
    assert same_bits(host(raw_c).reshape(-1, 3), raw_t.numpy()) and same_bits(host(norm_c).reshape(-1, 3), norm_t.numpy())
    assert tail_intact(raw_buf, 3 * n) and tail_intact(norm_buf, 3 * n)
    empty = ops.lattice_positions(d_flat[:0], res, mn, mx, sc)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


@pytest.mark.parametrize('step', [0, (1 << 32) + 5])
@pytest.mark.parametrize('n', [1, 255, 256, 257])
@pytest.mark.parametrize('res', BIG + [(20, 21, 22)], ids=lambda s: 'x'.join(map(str, s)))
def test_lattice_sampler_draw_positions_and_counter(dev, res, n, step):
    """n = 257 runs the ticket with two workgroups; step = 2^32 + 5 makes Philox counter word 3 non-zero."""
    lib, _lib, ops = _api()
    ds, mn, mx, sc = dataset(res)
    seed = 0x0123456789ABCDEF
    state = torch.tensor([step, 0], dtype=torch.int64, device=dev)
    raw, norm, flat = ops.lattice_sample(state, n, seed, res, mn, mx, sc, want_flat=True)
    want = R.lattice_draw(n, step, seed, ds.n_voxels)
    assert np.array_equal(host(flat), want)
    raw_t, norm_t = ds.positions_for(ds.lattice_from_flat(torch.from_numpy(want)))
    assert same_bits(host(raw), raw_t.numpy()) and same_bits(host(norm), norm_t.numpy())
    assert host(state).tolist() == [step + 1, 0]
    # the next draw, on caller-owned buffers, without the index output
    raw_c, raw_buf = canaried(3 * n)
    norm_c, norm_buf = canaried(3 * n)
    _lib.check(lib.lfgc_lattice_sample_f32(seed, state.data_ptr(), n, r3(res), f3(mn), f3(mx), f3(sc), raw_c.data_ptr(),
                                           norm_c.data_ptr(), None, stream()), 'lfgc_lattice_sample_f32')
    raw_t, norm_t = ds.positions_for(ds.lattice_from_flat(torch.from_numpy(R.lattice_draw(n, step + 1, seed, ds.n_voxels))))
    assert same_bits(host(raw_c).reshape(-1, 3), raw_t.numpy()) and same_bits(host(norm_c).reshape(-1, 3), norm_t.numpy())
    assert tail_intact(raw_buf, 3 * n) and tail_intact(norm_buf, 3 * n)
    assert host(state).tolist() == [step + 2, 0]
    # n = 0 leaves the state alone: through ops and through the entry
    empty = ops.lattice_sample(state, 0, seed, res, mn, mx, sc, want_flat=True)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 3), (0,)]
    _lib.check(lib.lfgc_lattice_sample_f32(seed, state.data_ptr(), 0, r3(res), f3(mn), f3(mx), f3(sc), raw_c.data_ptr(),
                                           norm_c.data_ptr(), None, stream()), 'lfgc_lattice_sample_f32')
    assert host(state).tolist() == [step + 2, 0] and tail_intact(raw_buf, 3 * n)
