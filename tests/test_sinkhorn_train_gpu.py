"""ops.sinkhorn_pos_conf (far_sinkhorn_pos_conf_f16s / far_sinkhorn_pos_conf_bwd_f16) on the GPU against float64 autograd of the
unrolled definition (tests/test_sinkhorn_gpu.py: oracle, restated below in torch so that autograd differentiates it) on the same
inputs.

Bars.  Forward: the Sinkhorn tests' 2e-5 on confidences (ATOL_CONF, their `_bar` rule: where the fp32 restatement deviates more on
a test's inputs, its deviation is the bar).  Gradients: relative Frobenius error of dF0 and dF1, relative error of d bin_score,
against max(1e-3, dev32): 1e-3 is the class tests/test_train_kernels_gpu.py documents for K1's fp16-operand backward (both
gradient contractions run on plain fp16 operands, 2^-11 per operand), dev32 the same error of the SAME definition differentiated by
torch autograd in fp32 on the GPU.  Gradients of the mean-reduced focal loss are ~1e-5 at these amplitudes: every bar is relative.
Measured values are printed; profiles/sinkhorn_train_parity.txt keeps a run."""
import numpy as np
import pytest
import torch

from tests.test_sinkhorn_gpu import ATOL_CONF, _bar, _dev, features, oracle, restatement32

pytestmark = pytest.mark.gpu

C = 256
HW0, HW1 = (24, 32), (20, 28)          # L = 768, S = 560: L != S, neither a multiple of 64 or 128
GRAD_BAR = 1e-3


def definition(f0, f1, alpha, T, m0=None, m1=None):
    """The unrolled definition in torch (dtype and device of f0): -> P (N, L+1, S+1)."""
    N, L, _ = f0.shape
    S = f1.shape[1]
    s = torch.einsum('nlc,nsc->nls', f0, f1) / C
    if m0 is not None:
        s = s.masked_fill(~(m0[:, :, None] & m1[:, None, :]), -1e9)
    a = alpha.reshape(1, 1, 1)
    Zc = torch.cat([torch.cat([s, a.expand(N, L, 1)], 2), a.expand(N, 1, S + 1)], 1)
    one = torch.ones((), dtype=f0.dtype, device=f0.device)
    norm = -torch.log(one * (L + S))
    lmu = torch.cat([norm.expand(L), torch.log(one * S)[None] + norm])
    lnu = torch.cat([norm.expand(S), torch.log(one * L)[None] + norm])
    u = torch.zeros(N, L + 1, dtype=f0.dtype, device=f0.device)
    v = torch.zeros(N, S + 1, dtype=f0.dtype, device=f0.device)
    for _ in range(T):
        u = lmu - torch.logsumexp(Zc + v[:, None, :], 2)
        v = lnu - torch.logsumexp(Zc + u[:, :, None], 1)
    return (Zc + u[:, :, None] + v[:, None, :] - norm).exp()


def entries(P, pb, pi, pj):
    return P[:, :-1, :-1][pb, pi, pj], P[:, :-1, -1], P[:, -1, :-1]


def focal_objective(pos, bin0, bin1, ids, masks, neg_weight=1.0):
    """far_amd.losses.coarse_focal_loss_sinkhorn (pinned to the reference by golden G22) on the three groups of entries."""
    from far_amd import losses
    data = {'conf_pos': pos, 'conf_bin0': bin0, 'conf_bin1': bin1, 'spv_b_ids': ids[0], 'spv_i_ids': ids[1], 'spv_j_ids': ids[2],
            'spv_gt_count': int(ids[0].numel())}
    if masks is not None:
        data.update(mask0=masks[0][:, None, :], mask1=masks[1][:, None, :])        # (N, 1, L): flatten(-2) gives (N, L)
    return losses.coarse_focal_loss_sinkhorn(data, neg_weight=neg_weight)


def make_case(N, masked, seed, extra=40):
    """Features with planted pairs; positions = most planted pairs (unmasked ones) + off-pairs, some sharing a row or a column with a
    planted pair, one position twice."""
    L, S = HW0[0] * HW0[1], HW1[0] * HW1[1]
    f0, f1, pairs = features(N, L, S, seed=seed, share=0.8)
    rng = np.random.default_rng(1000 + seed)
    m0 = m1 = None
    if masked:
        m0 = np.zeros((N,) + HW0, bool)
        m1 = np.zeros((N,) + HW1, bool)
        for n in range(N):
            m0[n, :HW0[0] - 2 * (n + 1), :HW0[1] - 3 * n] = True
            m1[n, :HW1[0] - n, :HW1[1] - 2 * (n + 1)] = True
        m0, m1 = m0.reshape(N, L), m1.reshape(N, S)
    b, i, j = [], [], []
    for n, (src, dst) in enumerate(pairs):
        keep = rng.random(len(src)) < 0.8
        ii, jj = src[keep], dst[keep]
        oi = np.concatenate([rng.integers(0, L, extra), ii[:extra // 4]])           # off-pairs; the last ones share a row with a pair
        oj = np.concatenate([rng.integers(0, S, extra - extra // 4), jj[:extra // 4], rng.integers(0, S, extra // 4)])
        ii, jj = np.concatenate([ii, oi, ii[:1]]), np.concatenate([jj, oj, jj[:1]])
        if masked:
            ok = m0[n, ii] & m1[n, jj]
            ii, jj = ii[ok], jj[ok]
        b.append(np.full(len(ii), n)); i.append(ii); j.append(jj)
    perm = rng.permutation(sum(len(x) for x in b))                                  # positions in no particular order
    ids = tuple(torch.from_numpy(np.concatenate(x)[perm]).long() for x in (b, i, j))
    return f0, f1, ids, (m0, m1) if masked else None


def reference_grads(f0, f1, alpha, T, ids, masks, objective, dtype, device):
    """autograd of the definition: -> (pos, bin0, bin1, df0, df1, dalpha) as float64 numpy."""
    t0 = torch.from_numpy(f0).to(device=device, dtype=dtype).requires_grad_(True)
    t1 = torch.from_numpy(f1).to(device=device, dtype=dtype).requires_grad_(True)
    a = torch.tensor(float(alpha), dtype=dtype, device=device, requires_grad=True)
    mm = None if masks is None else tuple(torch.from_numpy(m).to(device) for m in masks)
    P = definition(t0, t1, a, T, *(mm or (None, None)))
    idd = tuple(x.to(device) for x in ids)
    e = entries(P, *idd)
    objective(*e, idd, mm).backward()
    return tuple(x.detach().double().cpu().numpy() for x in (*e, t0.grad, t1.grad, a.grad))


def kernel_grads(f0, f1, alpha, T, ids, masks, objective):
    from far_amd import ops
    t0 = torch.from_numpy(f0).cuda().requires_grad_(True)
    t1 = torch.from_numpy(f1).cuda().requires_grad_(True)
    a = torch.tensor(float(alpha), device='cuda', requires_grad=True)
    mm = None if masks is None else tuple(torch.from_numpy(m).cuda() for m in masks)
    idd = tuple(x.cuda() for x in ids)
    e = ops.sinkhorn_pos_conf(t0, t1, a, T, *idd, *(mm or (None, None)))
    objective(*e, idd, mm).backward()
    torch.cuda.synchronize()
    return tuple(x.detach().double().cpu().numpy() for x in (*e, t0.grad, t1.grad, a.grad))


def _rel(got, ref):
    d = float(np.linalg.norm(np.ravel(got) - np.ravel(ref)))
    n = float(np.linalg.norm(np.ravel(ref)))
    return d / n if n > 0 else d


def _arbitrary(seed, scale=1.0):
    def objective(pos, bin0, bin1, ids, masks):
        g = torch.Generator().manual_seed(seed)
        w = [torch.randn(x.shape, generator=g).to(device=x.device, dtype=x.dtype) * scale for x in (pos, bin0, bin1)]
        return (pos * w[0]).sum() + (bin0 * w[1]).sum() + (bin1 * w[2]).sum()
    return objective


def _compare(name, got, ref, r32):
    """forward within the Sinkhorn bar, gradients within max(1e-3, dev32); -> the three measured gradient errors."""
    for k, what in enumerate(('conf_pos', 'conf_bin0', 'conf_bin1')):
        _bar(f'{name} {what}', _dev(got[k], ref[k]), ATOL_CONF, _dev(r32[k], ref[k]))
    errs, bad = [], []
    for k, what in ((3, 'dF0'), (4, 'dF1'), (5, 'd bin_score')):
        assert np.isfinite(got[k]).all(), what
        e, e32 = _rel(got[k], ref[k]), _rel(r32[k], ref[k])
        arm = 'dev32' if e32 > GRAD_BAR else 'derived'
        print(f'[{name}] {what}: relative error {e:.3e}   bar {max(GRAD_BAR, e32):.1e} ({arm} arm; fp32 autograd {e32:.3e})   '
              f'|reference| {float(np.linalg.norm(np.ravel(ref[k]))):.3e}')
        if not e <= max(GRAD_BAR, e32):
            bad.append(f'{name} {what}: {e:.3e} > {max(GRAD_BAR, e32):.1e}')
        errs.append(e)
    assert not bad, '; '.join(bad)
    return errs


CASES = [  # N, T, masked, bin_score, upstream
    (1, 3, False, 1.0, 'focal'),
    (3, 3, True, 1.0, 'focal'),
    (1, 0, False, 1.0, 'arbitrary'),
    (3, 1, False, -0.5, 'arbitrary'),
    (1, 6, True, -0.5, 'focal'),
    (3, 6, False, 1.0, 'arbitrary'),
    (1, 1, True, 1.0, 'arbitrary'),
    (3, 0, True, -0.5, 'focal'),
    (1, 3, False, -0.5, 'arbitrary'),
]


@pytest.mark.parametrize('N, T, masked, alpha, upstream', CASES)
def test_forward_and_gradients_match_float64_autograd(N, T, masked, alpha, upstream):
    seed = 100 + 7 * N + T + (50 if masked else 0)
    f0, f1, ids, masks = make_case(N, masked, seed)
    objective = (lambda *a: focal_objective(*a, neg_weight=0.7)) if upstream == 'focal' else _arbitrary(seed, 1e-3)
    ref = reference_grads(f0, f1, alpha, T, ids, masks, objective, torch.float64, 'cpu')
    r32 = reference_grads(f0, f1, alpha, T, ids, masks, objective, torch.float32, 'cuda')
    got = kernel_grads(f0, f1, alpha, T, ids, masks, objective)
    name = f'N={N} T={T} masks={masked} bin={alpha} {upstream}'
    assert got[0].shape == (ids[0].numel(),) and got[1].shape == (N, f0.shape[1]) and got[2].shape == (N, f1.shape[1])
    _compare(name, got, ref, r32)
    if masked:      # a masked row / column receives exactly zero
        assert (got[3][~masks[0]] == 0).all() and (got[4][~masks[1]] == 0).all()
    # the definition agrees with the numpy oracle the inference tests use
    A, _, _ = oracle(f0, f1, alpha, T, *(masks or (None, None)))
    assert _dev(ref[1], A[:, :-1, -1]) < 1e-9


def test_dustbin_entries_are_the_bits_of_inference():
    """The forward runs the matcher's own iterations: its dustbin column / row equal those of ops.coarse_match_sinkhorn's
    conf_matrix_with_bin bit for bit (same potentials, same expression)."""
    from far_amd import ops
    f0, f1, ids, masks = make_case(2, True, 5)
    t0, t1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
    m0, m1 = (torch.from_numpy(m.astype(np.uint8)).cuda() for m in masks)
    for T, alpha in ((3, 1.0), (0, -0.5), (5, 2.5)):
        bs = torch.tensor(alpha, device='cuda')
        inf = ops.coarse_match_sinkhorn(t0, t1, bs, T, 0.2, 2, HW0, HW1, 8.0, m0, m1, want_conf=True)['conf_matrix_with_bin']
        with torch.no_grad():
            pos, bin0, bin1 = ops.sinkhorn_pos_conf(t0, t1, bs, T, *(x.cuda() for x in ids), m0, m1)
        assert torch.equal(bin0, inf[:, :-1, -1]) and torch.equal(bin1, inf[:, -1, :-1]), (T, alpha)
        ref = inf[:, :-1, :-1][tuple(x.cuda() for x in ids)]
        assert float(((pos - ref).abs() / ref.abs().clamp(min=1.0)).max()) <= ATOL_CONF        # relative above 1 (T = 0: nothing is normalised)


@pytest.mark.parametrize('log2_scale', [-30, 0, 12])
def test_gradient_scale(log2_scale):
    """Upstream gradients scaled by 2^k: the same relative error (a power of two commutes with every operation of the backward, and
    the fp16 operand of the second contraction is normalised by the largest adjoint weight) -- the lesson of
    tests/test_train_kernels_gpu.py: test_backward_kernels_keep_their_precision_at_any_gradient_scale."""
    f0, f1, ids, masks = make_case(2, False, 21)
    base = _arbitrary(77, 1e-3)
    ref = reference_grads(f0, f1, 1.0, 3, ids, None, base, torch.float64, 'cpu')
    r32 = reference_grads(f0, f1, 1.0, 3, ids, None, base, torch.float32, 'cuda')
    e0 = _compare('scale 2^0', kernel_grads(f0, f1, 1.0, 3, ids, None, base), ref, r32)
    sc = 2.0 ** log2_scale
    got = kernel_grads(f0, f1, 1.0, 3, ids, None, _arbitrary(77, 1e-3 * sc))
    got = got[:3] + tuple(g / sc for g in got[3:])
    ek = _compare(f'scale 2^{log2_scale}', got, ref, r32)
    for a, b in zip(e0, ek):
        assert abs(a - b) <= 0.05 * a + 1e-9, (e0, ek)


def test_masked_rows_hold_anything():
    """Masked rows and columns get exactly zero gradient, and what they hold -- NaN, inf -- reaches no output: every output equals,
    bit for bit, that of the same call with those rows zeroed."""
    from far_amd import ops
    f0, f1, ids, masks = make_case(2, True, 33)
    ids = list(ids)
    # a position on a masked cell too: P = 0 there, no gradient
    bad_i = int(np.nonzero(~masks[0][0])[0][0])
    ids[0] = torch.cat([ids[0], torch.tensor([0])]); ids[1] = torch.cat([ids[1], torch.tensor([bad_i])])
    ids[2] = torch.cat([ids[2], torch.tensor([3])])
    obj = _arbitrary(5, 1e-3)
    z0, z1 = f0.copy(), f1.copy()
    z0[~masks[0]] = 0; z1[~masks[1]] = 0
    clean = kernel_grads(z0, z1, 1.0, 3, ids, masks, obj)
    p0, p1 = f0.copy(), f1.copy()
    p0[~masks[0]] = np.nan
    p1[~masks[1]] = np.inf
    p1[1, np.nonzero(~masks[1][1])[0][::2]] = -np.inf
    dirty = kernel_grads(p0, p1, 1.0, 3, ids, masks, obj)
    ops.overflow_flag('cuda').zero_()           # the operand preparation reports the non-finite features, as in inference
    for k, (a, b) in enumerate(zip(clean, dirty)):
        assert np.isfinite(b).all(), k
        np.testing.assert_array_equal(a, b, err_msg=str(k))
    assert clean[0][-1] == 0
    assert (dirty[3][~masks[0]] == 0).all() and (dirty[4][~masks[1]] == 0).all()
    assert np.abs(dirty[3][masks[0]]).max() > 0 and np.abs(dirty[4][masks[1]]).max() > 0


def test_empty_and_edge_cases():
    from far_amd import ops
    L, S = HW0[0] * HW0[1], HW1[0] * HW1[1]
    f0, f1, ids, _ = make_case(1, False, 41)
    none = tuple(torch.zeros(0, dtype=torch.long) for _ in range(3))
    # M = 0: the dustbin entries still carry a gradient
    obj = _arbitrary(9, 1e-3)
    ref = reference_grads(f0, f1, 1.0, 3, none, None, obj, torch.float64, 'cpu')
    r32 = reference_grads(f0, f1, 1.0, 3, none, None, obj, torch.float32, 'cuda')
    got = kernel_grads(f0, f1, 1.0, 3, none, None, obj)
    assert got[0].shape == (0,)
    _compare('M = 0', got, ref, r32)
    # M = 0 and nothing upstream on the dustbins: zero gradients
    t0 = torch.from_numpy(f0).cuda().requires_grad_(True)
    t1 = torch.from_numpy(f1).cuda().requires_grad_(True)
    a = torch.tensor(1.0, device='cuda', requires_grad=True)
    pos, bin0, bin1 = ops.sinkhorn_pos_conf(t0, t1, a, 3, *(x.cuda() for x in none))
    (pos.sum() + 0.0 * bin0.sum()).backward()
    assert float(t0.grad.abs().max()) == 0 and float(t1.grad.abs().max()) == 0 and float(a.grad) == 0
    # N = 0
    e0 = torch.zeros(0, L, C, device='cuda', requires_grad=True)
    e1 = torch.zeros(0, S, C, device='cuda', requires_grad=True)
    pos, bin0, bin1 = ops.sinkhorn_pos_conf(e0, e1, a, 3, *(x.cuda() for x in none))
    assert pos.shape == (0,) and bin0.shape == (0, L) and bin1.shape == (0, S)
    (pos.sum() + bin0.sum() + bin1.sum()).backward()
    assert e0.grad.shape == (0, L, C) and e1.grad.shape == (0, S, C)
    # refused: another width, more iterations than the kernels stage, CPU tensors
    with pytest.raises(NotImplementedError):
        ops.sinkhorn_pos_conf(torch.zeros(1, 8, 128, device='cuda'), torch.zeros(1, 8, 128, device='cuda'), a, 3, *(x.cuda() for x in none))
    with pytest.raises(NotImplementedError):
        ops.sinkhorn_pos_conf(t0, t1, a, 65, *(x.cuda() for x in none))
    from far_amd import _lib
    with pytest.raises(_lib.FarHipError):
        ops.sinkhorn_pos_conf(t0.detach().cpu(), t1.detach().cpu(), a.detach().cpu(), 3, *none)


def test_out_of_range_positions_are_ignored_not_read():
    """A position outside the grid gets confidence 0 and moves no gradient (the kernels check every index before they use it)."""
    from far_amd import ops
    f0, f1, ids, _ = make_case(1, False, 43)
    L, S = f0.shape[1], f1.shape[1]
    bad = (torch.tensor([0, 0, 5, -1]), torch.tensor([L, 3, 0, 0]), torch.tensor([0, S + 7, 0, 0]))
    both = tuple(torch.cat([a, b]) for a, b in zip(ids, bad))
    obj = _arbitrary(3, 1e-3)
    a = kernel_grads(f0, f1, 1.0, 3, ids, None, obj)
    b = kernel_grads(f0, f1, 1.0, 3, both, None, lambda pos, b0, b1, i_, m_: obj(pos[:-4], b0, b1, i_, m_) + pos[-4:].sum())
    assert (b[0][-4:] == 0).all()
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)
