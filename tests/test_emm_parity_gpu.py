"""K2 (far_emm_pv_f16s / far_emm_pv_f16 / far_emm_pv_f32 + far_emm_contract_f32, far_emm_bwd_f16) on the GPU, held to float64 per
output block in every score regime and key tail (tests/emm_inputs.py states the rule and the cases; tests/test_emm_parity_cpu.py
shows on the float64 reference alone that the cases are what they claim and that the whole-tensor assertion of
tests/test_emm_gpu.py cannot see what this rule sees).

Every measured figure is printed first ('[parity] ...', '[k2 bwd] ...'); profiles/k2_parity.txt records a run."""
import functools
import math

import pytest
import torch

from tests import emm_inputs as ei

pytestmark = pytest.mark.gpu
Z = 2
LOG2E = 1.0 / math.log(2.0)


@functools.lru_cache(maxsize=None)
def _case(N, regime, Zc=Z):
    """Inputs on the GPU with their float64 / fp32 references, computed once per (N, regime) and shared (nobody writes to them)."""
    q, k, v, pos = ei.emm_case(Zc, N, regime, ei.case_seed(N, regime), device='cuda')
    return (q, k, v, pos), ei.reference(q, k, v, pos, torch.float64, sums=True), ei.reference(q, k, v, pos, torch.float32)


def _clean_flag():
    from far_amd import ops
    ops.overflow_flag('cuda').zero_()


# ---- 1. forward against float64, per block ------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ei.REGIMES)
@pytest.mark.parametrize('N', ei.KEY_COUNTS)
def test_forward_per_block(N, regime):
    """ops.emm_bilinear in the default split form and with exact_f32=True: T and F meet the per-block rule (tests/emm_inputs.py:
    check_blocks), max(3 dev32_b, floor_b), the overflow flag stays clear, the results are finite.  Floors: 2^-20 S plus the fp32
    accumulation error of the 64-term score carried through the exponent of P (score_floor_T), for both forms; the split form adds
    the fp16 resolution of p and of v~ / colsum (split_floor_T).  Each term is derived from the code and the number formats, none from
    a kernel's error.  Why 2^-20 S alone cannot stand: against max(3 dev32_b, 2^-20 S_b) one MI355X run gave as worst ratios exact_f32
    T 0.62 flat, 1.37 peaked, 6.07 shifted (N = 320, a block at 1e-5 max|T|), 1.49 negative; split T 1.82 flat (one-row block), 2.61
    peaked, 2.69 negative (N = 1, where dev32 = 0), and in the shifted regime rows whose every P is below 2^-39 come out 0 (error = |T|
    ~ 1e-17).
    The exact_f32 path (far_dual_softmax_stats_f32 + far_emm_pv_f32) guards every row and key against N and refuses no key count: it
    runs at N = 1 and 33 like everywhere else."""
    from far_amd import ops
    (q, k, v, pos), r64, r32 = _case(N, regime)
    for form, kw in (('split', {}), ('exact_f32', {'exact_f32': True})):
        split = form == 'split'
        _clean_flag()
        F, T = ops.emm_bilinear(q, k, v, pos, ei.SCALE, **kw)
        assert not ops.activation_overflowed('cuda'), form
        assert T.shape == (Z, N, 70) and F.shape == (Z, 70, 70)
        assert torch.isfinite(T).all() and torch.isfinite(F).all(), form
        errs = []
        for check, got in ((ei.check_T, T), (ei.check_F, F)):
            try:
                check(f'k2 {form} {regime} N{N}', got, r64, r32, split=split)
            except ei.BlockParityError as e:
                errs.append(str(e))
        assert not errs, '\n'.join(errs)


# ---- 2. plain fp16 operands ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [33, 65, 129, 221])
def test_plain_fp16_operands(N):
    """far_emm_pv_f16: the 16-bit-operand class, 3e-3 max|.| against float64 (the bar of tests/test_emm_gpu.py), finite, and a
    different result from the split one."""
    from far_amd import ops
    (q, k, v, pos), r64, _ = _case(N, 'flat')
    F, T = ops.emm_bilinear(q, k, v, pos, ei.SCALE, plain16=True)
    Fs, Ts = ops.emm_bilinear(q, k, v, pos, ei.SCALE)
    eT = float((T.double() - r64['T']).abs().max() / r64['T'].abs().max())
    eF = float((F.double() - r64['F']).abs().max() / r64['F'].abs().max())
    print(f'[parity] k2 plain16 flat N{N}: max|T - f64| / max|T| {eT:.3e}  max|F - f64| / max|F| {eF:.3e}  bar 3e-3')
    assert torch.isfinite(T).all() and torch.isfinite(F).all()
    assert eT < 3e-3 and eF < 3e-3
    assert not torch.equal(T, Ts) and not torch.equal(F, Fs)


# ---- 3. the statistics the backward reads -------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ei.REGIMES)
@pytest.mark.parametrize('N', [33, 129, 221])
def test_softmax_statistics(N, regime):
    """far_emm_pv_f16s_copy_stats: rs = (R, sum_j 2^(x - R)) per query row with R an integer at or above the row maximum, cs =
    (max, sum) per key column, x = s log2(e).  reference + log2(sum) must equal logsumexp(s) / ln 2 within max(3 dev32, 2^-20
    max|lse|) per element, dev32 the fp32 torch logsumexp's own deviation from float64.  R is compared with the float64 row maximum
    up to that same bar (a maximum is known no better than the scores), and must be its ceiling, not merely above it: a larger
    reference would cost the one-exp product its range."""
    from far_amd.ops import head
    (q, k, v, pos), r64, r32 = _case(N, regime)
    _, rs, cs = head._emm_pv(q, k, v, pos, ei.SCALE, want_stats=True)
    assert rs.shape == cs.shape == (Z, N, 2)
    assert torch.isfinite(rs).all() and torch.isfinite(cs).all()
    for name, st, dim in (('rowstat', rs, -1), ('colstat', cs, -2)):
        lse = torch.logsumexp(r64['s'], dim=dim) * LOG2E
        lse32 = torch.logsumexp(r32['s'], dim=dim) * LOG2E
        dev32 = float((lse32.double() - lse).abs().max())
        floor = ei.FLOOR * float(lse.abs().max())
        bar = max(ei.FACTOR * dev32, floor)
        got = st[..., 0].double() + torch.log2(st[..., 1].double())
        d = float((got - lse).abs().max())
        print(f'[parity] k2 {name} {regime} N{N}: kernel-vs-ref {d:.3e}  dev32 {dev32:.3e}  bar {bar:.3e}  ratio {d / bar:.2f} '
              f'({"floor 2^-20 max|lse| decides" if floor > ei.FACTOR * dev32 else "3 x dev32"})')
        assert d <= bar, (name, d, bar)
        assert bool((st[..., 1] > 0).all()), name
        mx = r64['s'].amax(dim=dim) * LOG2E
        if name == 'rowstat':
            R = st[..., 0].double()
            assert torch.equal(R, R.round()), 'row reference is not an integer'
            assert bool((R >= mx - bar).all()), 'row reference below the row maximum'
            assert bool((R < mx + 1 + bar).all()), 'row reference is not the ceiling of the row maximum'
        else:
            assert float((st[..., 0].double() - mx).abs().max()) <= bar, 'column maximum'


# ---- 4. plane layout at ragged N ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,h,N', [(2, 4, 221), (1, 4, 65)])
def test_planes_layout_at_ragged_n(B, h, N):
    """ops.emm_bilinear_planes (q | k | v planes of the fused projection, q rotated by B images) is bit-equal to ops.emm_bilinear on
    the permuted contiguous copies.  shifted: u is shared by all problems, so every (query image, key image) pairing is shifted."""
    from far_amd import ops
    q, k, v, pos = ei.emm_case(2 * B * h, N, 'shifted', ei.case_seed(N, 'shifted') + 50, device='cuda')
    planes = torch.cat([t.reshape(h, 2 * B, N, 64) for t in (q, k, v)], 0).contiguous()        # (3 h, 2 B, N, 64)
    F, T = ops.emm_bilinear_planes(planes, pos, ei.SCALE, B)
    qq, kk, vv = (planes[t * h:(t + 1) * h].permute(1, 0, 2, 3) for t in range(3))             # (2B, h, N, 64): [image, head]
    qq = torch.cat([qq[B:], qq[:B]], 0)                                                        # direction d: queries of image 1 - d
    qq, kk, vv = (t.reshape(2 * B * h, N, 64).contiguous() for t in (qq, kk, vv))
    Fr, Tr = ops.emm_bilinear(qq, kk, vv, pos, ei.SCALE)
    assert torch.isfinite(T).all() and torch.isfinite(F).all()
    assert torch.equal(T, Tr) and torch.equal(F, Fr)
    r64 = ei.reference(qq, kk, vv, pos, torch.float64, sums=True)
    ei.check_T(f'k2 planes shifted B{B} h{h} N{N}', T, r64, ei.reference(qq, kk, vv, pos, torch.float32), split=True)


# ---- 5. batch independence and repeatability ----------------------------------------------------------------------------
@pytest.mark.parametrize('N', [129, 221])
def test_problem_bits_do_not_depend_on_the_batch(N):
    from far_amd import ops
    q, k, v, pos = ei.emm_case(5, N, 'peaked', ei.case_seed(N, 'peaked') + 60, device='cuda')
    F5, T5 = ops.emm_bilinear(q, k, v, pos, ei.SCALE)
    for z in (0, 4):
        F1, T1 = ops.emm_bilinear(q[z:z + 1].contiguous(), k[z:z + 1].contiguous(), v[z:z + 1].contiguous(), pos, ei.SCALE)
        assert torch.equal(T1, T5[z:z + 1]) and torch.equal(F1, F5[z:z + 1]), (N, z)


def test_ten_launches_are_bit_identical_alone_and_next_to_a_busy_stream():
    """(Z, N) = (8, 640): ten launches bit-identical to the first, alone, and again while a second stream runs a loop of large K9
    Linear launches (the form of tests/test_vit_attention_gpu.py: waves of another kernel share the CUs)."""
    from far_amd import ops
    q, k, v, pos = ei.emm_case(8, 640, 'peaked', 5, device='cuda')
    F0, T0 = (t.clone() for t in ops.emm_bilinear(q, k, v, pos, ei.SCALE))
    assert torch.isfinite(T0).all() and torch.isfinite(F0).all()
    for it in range(10):
        F, T = ops.emm_bilinear(q, k, v, pos, ei.SCALE)
        assert torch.equal(T, T0) and torch.equal(F, F0), f'alone, launch {it}'
    g = torch.Generator(device='cuda').manual_seed(6)
    big = torch.randn(1 << 17, 256, device='cuda', generator=g)
    pc = ops.PackedConv(torch.randn(256, 256, device='cuda', generator=g) / 16)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    keep = []
    for it in range(10):
        with torch.cuda.stream(side):
            for _ in range(4):
                keep.append(ops.linear_f16s(big, pc))
            del keep[:-4]
        F, T = ops.emm_bilinear(q, k, v, pos, ei.SCALE)
        assert torch.equal(T, T0) and torch.equal(F, F0), f'next to the busy stream, launch {it}'
    side.synchronize()
    torch.cuda.synchronize()


# ---- 6. overflow flag ---------------------------------------------------------------------------------------------------
def test_overflow_flag():
    """|q|, |k| > 4094 is beyond the 2^4-scaled split: the flag rises, and the other problem of the batch stays finite."""
    from far_amd import ops
    (q, k, v, pos), _, _ = _case(65, 'flat')
    for which in range(2):
        t = [q.clone(), k.clone()]
        t[which][1, 17, 40] = 1.0e4
        _clean_flag()
        F, T = ops.emm_bilinear(t[0], t[1], v, pos, ei.SCALE)
        assert ops.activation_overflowed('cuda'), which
        assert torch.isfinite(T[0]).all() and torch.isfinite(F[0]).all(), which
    _clean_flag()
    ops.emm_bilinear(q, k, v, pos, ei.SCALE)
    assert not ops.activation_overflowed('cuda')


# ---- 7. backward, per problem -------------------------------------------------------------------------------------------
ZB = 3


@functools.lru_cache(maxsize=None)
def _backward(N, regime):
    """ops.emm_bilinear_train and the float64 / fp32 autograd of the torch composition on Z = 3 problems whose upstream gradient is
    scaled by 2^(6 (z - 1)): problem 0 is 2^12 below problem 2 (ops/head.py places the kernel's fp16 quantities by scale factors
    taken from the statistics of the problems)."""
    from far_amd import ops
    q, k, v, pos = ei.emm_case(ZB, N, regime, ei.case_seed(N, regime) + 70, device='cuda')
    g = torch.Generator().manual_seed(N)
    dF = (torch.randn(ZB, 70, 70, generator=g) * (2.0 ** (6 * (torch.arange(ZB) - 1))).view(ZB, 1, 1).float()).cuda()
    a = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ops.emm_bilinear_train(a[0], a[1], a[2], pos, ei.SCALE).backward(dF)
    grads = {}
    for dt in (torch.float64, torch.float32):
        r = [t.to(dt).clone().requires_grad_(True) for t in (q, k, v)]
        ei.reference(r[0], r[1], r[2], pos, dt)['F'].backward(dF.to(dt))
        grads[dt] = [t.grad for t in r]
    return (q, k, v, pos, dF), [t.grad for t in a], grads[torch.float64], grads[torch.float32]


def _fro(got, ref, scale_ref=None):
    """Relative Frobenius error per problem; where the reference gradient is exactly zero, relative to `scale_ref`."""
    num = (got.double() - ref).flatten(1).norm(dim=1)
    den = ref.flatten(1).norm(dim=1)
    if scale_ref is not None:
        den = torch.where(den > 0, den, scale_ref.flatten(1).norm(dim=1))
    return (num / den).tolist()


def _cancelling(q, k, v, pos, dF):
    """scale (2 P dP) k and its transpose times q: the first of the three terms of ds = 2 P dP - R u - C v carried into dq and dk."""
    r = ei.reference(q, k, v, pos, torch.float64)
    dP2 = 2.0 * r['P'] * ((r['vt'] @ dF.double()) @ r['vt'].transpose(1, 2))                 # 2 P dP, dP_ab = (v~ dF)_a . v~_b
    return ei.SCALE * dP2 @ k.double(), ei.SCALE * dP2.transpose(1, 2) @ q.double()


@pytest.mark.parametrize('N', [1, 33, 65, 129, 221])
def test_backward_per_problem(N):
    """flat regime, relative Frobenius error PER PROBLEM against float64 autograd: dq, dk < 5e-3, dv < 1e-5 (the bars documented in
    tests/test_train_kernels_gpu.py), on problems whose upstream gradients differ by 2^12.
    N = 1: P = 1 whatever s is, so the float64 dq and dk are exactly zero (ds = 2 P dP - R u - C v = 2 dP - dP - dP) and a relative
    error has no denominator; there the error is taken relative to the term that cancels, scale * (2 P dP) k resp. its transpose
    times q -- what an fp16-operand kernel that forms the three terms separately can be held to.

    Measured on an MI355X (profiles/k2_parity.txt): dq, dk 1.0 - 1.9e-3 at N >= 33 and <= 7.2e-4 at N = 1 in all three problems, dv
    <= 8.4e-7.  With plain fp16 q, k in the recomputed scores (an error of about |s| 2^-11 in the exponent) this test found dq, dk at
    4.4e-3 ... 8.6e-3 in every problem, 1.39e-2 in the small-gradient problem at N = 33 -- not through the shared alpha of
    ops/head.py (one alpha per problem changed no printed digit: a power-of-two scale changes no bit while nothing underflows):
    far_emm_bwd_f16 now forms its scores from split-fp16 q, k like the forward."""
    (q, k, v, pos, dF), got, g64, _ = _backward(N, 'flat')
    canc = _cancelling(q, k, v, pos, dF) + (None,)
    bars = {'q': 5e-3, 'k': 5e-3, 'v': 1e-5}
    errs = {}
    for name, x, y, c in zip('qkv', got, g64, canc):
        assert torch.isfinite(x).all(), name
        errs[name] = _fro(x, y, c)
        print(f'[k2 bwd] flat Z={ZB} N={N} d{name}: relative Frobenius error per problem (dF x 2^-6, 1, 2^6) '
              + '  '.join(f'{e:.3e}' for e in errs[name]) + f'  bar {bars[name]:g}')
    for name in 'qkv':
        assert max(errs[name]) < bars[name], (name, errs[name])


@pytest.mark.parametrize('regime', ei.REGIMES)
@pytest.mark.parametrize('N', [65, 221])
def test_backward_dv_per_block(N, regime):
    """dv~ = T dF^T + T' dF is fp32-grade (T, T' from the split forward, two fp32 products): dv meets the per-block rule on 32 rows x
    [0, 32), [32, 64), r32 the fp32 autograd of the torch composition, the floor that of T and T' (tests/emm_inputs.py: split_floor_T;
    T' is the forward with q and k exchanged, i.e. on s^T) carried through the two products: floor_T |dF|^T + floor_T' |dF|.
    dq, dk outside the flat regime carry no bar: finite, and the per-problem error is printed and recorded, not asserted.  What
    decides it is how much of ds = 2 P dP - R u - C v cancels: dP comes from fp16 A, v~ (2^-11), u and v from fp32, so the error is
    about 1e-4 of the FIRST term, and where a softmax is one-hot (2 P dP - R u is then ~0 row by row) the gradient is a small
    remainder of it.  The line prints that ratio, |scale (2 P dP) k| / |dq|: in the shifted regime it is 1542 / 377 / 3.4 for the
    three problems at N = 65 and 4.4 / 2.3 / 1420 at N = 221, and the measured errors follow it (9.1e-2 / 2.6e-2 / 1.9e-3 and
    6.9e-4 / 5.5e-4 / 2.7e-1), not the scale of dF.  It is not underflow under the shared alpha of ops/head.py either: with one
    alpha per problem every figure of every regime stays the same to the printed digit."""
    (q, k, v, pos, dF), got, g64, g32 = _backward(N, regime)
    for name, x, y, c in zip('qk', got, g64, _cancelling(q, k, v, pos, dF)):
        assert torch.isfinite(x).all(), name
        ratio = (c.flatten(1).norm(dim=1) / y.flatten(1).norm(dim=1)).tolist()
        print(f'[k2 bwd] {regime} Z={ZB} N={N} d{name}: relative Frobenius error per problem (dF x 2^-6, 1, 2^6) '
              + '  '.join(f'{e:.3e}' for e in _fro(x, y)) + '  first term / gradient ' + ' '.join(f'{a:.3g}' for a in ratio)
              + '  (recorded, no bar)')
    r = ei.reference(q, k, v, pos, torch.float64, sums=True)
    ad = dF.double().abs()
    floor = ei.split_floor_T(r['s'], r['sig'], r['vt']) @ ad.transpose(1, 2) \
        + ei.split_floor_T(r['s'].transpose(1, 2), r['sig'].transpose(1, 2), r['vt']) @ ad
    ei.check_blocks(f'k2 bwd dv {regime} N{N}', got[2], g64[2], g32[2], floor[:, :, :64], ei.row_groups(N),
                    ei.COL_GROUPS[:2], floor_name='split floor')
