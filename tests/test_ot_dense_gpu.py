"""ops.sinkhorn_dense_focal_loss (far_sinkhorn_dense_focal_f16s / far_sinkhorn_dense_focal_bwd_f16) on the GPU against float64
autograd of the materialising definition: tests/test_sinkhorn_train_gpu.py:definition (the unrolled optimal-transport iterations in
torch) followed by far_amd.losses.coarse_focal_loss_dense_torch (the dense focal loss, pinned to the reference by golden G23) on
conf = P[:, :L, :S].

Bars (the `_bar` rule of the Sinkhorn tests: where the fp32 autograd of the SAME composition on the GPU, dev32, deviates more from
float64 on a test's inputs, its deviation is the bar).  Loss: relative 1e-5, the project's confidence bar.  dF0 / dF1: relative
Frobenius 1e-3, d bin_score: relative 1e-3 -- the class tests/test_train_kernels_gpu.py documents for K1's fp16-operand backward.
Measured values are printed; profiles/ot_dense_parity.txt keeps a run.

Inputs: tests.test_sinkhorn_gpu.features(share = 0.8); the labels are a random 80 % of the planted pairs, so the unlabelled planted
pairs are confident NEGATIVES (p > 0.5: the 1 / (1 - p) side of the loss).  No fp32 evaluation resolves an entry with
1e-6 < 1 - p < 1e-3 (1 - p carries 2^-24 absolute), the reference's own included, so every case asserts on its float64 matrix that
this regime is empty -- and, from three iterations on, that confident negatives exist (after ONE iteration no entry is above 0.5
on these inputs: the counts are printed).

Labels are a multiset: each label is one positive term and leaves the negative sum once, all M count in the normalisers
(pos_weight / M, neg_weight / (N L S - M)); a label out of range or on a masked cell adds nothing.  For distinct labels in range that
is coarse_focal_loss_dense_torch (asserted in float64 below); `multiset_loss` states it for the two tests that need it."""
import functools

import numpy as np
import pytest
import torch

from tests.test_sinkhorn_gpu import features
from tests.test_sinkhorn_train_gpu import definition

pytestmark = pytest.mark.gpu

C = 256
SHAPES = {  # name: N, grid 0, grid 1
    '1x35x72': (1, (5, 7), (8, 9)),              # one partial tile each way
    '2x192x136': (2, (12, 16), (8, 17)),         # S no multiple of 32, 64 or 128
    '1x768x560': (1, (24, 32), (20, 28)),        # several tiles both ways; the sparse tests' shape
}
EQUAL = dict(alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0)
NEG_HEAVY = dict(alpha=0.25, gamma=2.0, pos_weight=0.3, neg_weight=300.0)
LOSS_BAR, GRAD_BAR = 1e-5, 1e-3


@functools.lru_cache(maxsize=None)
def make(name, seed=0, masked=False, amp=3.75):
    """-> f0, f1, ids (distinct labels: 80 % of the planted pairs, unmasked ones), masks or None.  Masks as
    tests.test_sinkhorn_train_gpu.make_case builds them (valid extents shrinking with the pair index)."""
    N, hw0, hw1 = SHAPES[name]
    L, S = hw0[0] * hw0[1], hw1[0] * hw1[1]
    f0, f1, pairs = features(N, L, S, amp=amp, seed=seed, share=0.8)
    rng = np.random.default_rng(1000 + seed)
    m0 = m1 = None
    if masked:
        m0 = np.zeros((N,) + hw0, bool)
        m1 = np.zeros((N,) + hw1, bool)
        for n in range(N):
            m0[n, :hw0[0] - 2 * (n + 1), :hw0[1] - 3 * n] = True
            m1[n, :hw1[0] - n, :hw1[1] - 2 * (n + 1)] = True
        m0, m1 = m0.reshape(N, L), m1.reshape(N, S)
    b, i, j = [], [], []
    for n, (src, dst) in enumerate(pairs):
        keep = rng.random(len(src)) < 0.8
        ii, jj = src[keep], dst[keep]
        if masked:
            ok = m0[n, ii] & m1[n, jj]
            ii, jj = ii[ok], jj[ok]
        b.append(np.full(len(ii), n)); i.append(ii); j.append(jj)
    perm = rng.permutation(sum(len(x) for x in b))
    ids = tuple(torch.from_numpy(np.concatenate(x)[perm]).long() for x in (b, i, j))
    return f0, f1, ids, (m0, m1) if masked else None


def multiset_loss(conf, ids, alpha, gamma, pos_weight, neg_weight, weight=None):
    """The loss with the labels as a multiset (module docstring); ids: in range."""
    M = int(ids[0].numel())
    q = torch.clamp(conf, 1e-6, 1 - 1e-6)
    neg = -alpha * torch.pow(q, gamma) * (1 - q).log()
    pos = -alpha * torch.pow(1 - q, gamma) * q.log()
    if weight is not None:
        neg, pos = neg * weight, pos * weight
    c_neg = neg_weight / (conf.numel() - M)
    c_pos = pos_weight / M if M else 0.0
    return c_neg * (neg.sum() - neg[ids].sum()) + c_pos * pos[ids].sum()


def torch_leg(f0, f1, alpha, T, ids, masks, focal, dtype, device, no_gt=False, loss_fn=None):
    """autograd of definition + dense focal loss -> (loss, dF0, dF1, d bin_score, conf) as float64 numpy."""
    from far_amd import losses
    t0 = torch.from_numpy(f0).to(device=device, dtype=dtype).requires_grad_(True)
    t1 = torch.from_numpy(f1).to(device=device, dtype=dtype).requires_grad_(True)
    a = torch.tensor(float(alpha), dtype=dtype, device=device, requires_grad=True)
    mm = None if masks is None else tuple(torch.from_numpy(m).to(device) for m in masks)
    conf = definition(t0, t1, a, T, *(mm or (None, None)))[:, :-1, :-1]
    weight = None if mm is None else (mm[0][:, :, None] & mm[1][:, None, :]).to(dtype)
    idd = tuple(x.to(device) for x in ids)
    if loss_fn is None:
        loss = losses.coarse_focal_loss_dense_torch(conf, idd, no_gt, weight=weight, **focal)
    else:
        loss = loss_fn(conf, idd, weight=weight, **focal)
    loss.backward()
    return tuple(x.detach().double().cpu().numpy() for x in (loss, t0.grad, t1.grad, a.grad, conf))


def kernel_leg(f0, f1, alpha, T, ids, masks, focal, no_gt=False, upstream=1.0):
    from far_amd import ops
    t0 = torch.from_numpy(f0).cuda().requires_grad_(True)
    t1 = torch.from_numpy(f1).cuda().requires_grad_(True)
    a = torch.tensor(float(alpha), device='cuda', requires_grad=True)
    mm = (None, None) if masks is None else tuple(torch.from_numpy(m).cuda() for m in masks)
    loss = ops.sinkhorn_dense_focal_loss(t0, t1, a, T, *(x.cuda() for x in ids), focal['alpha'], focal['gamma'], focal['pos_weight'],
                                         focal['neg_weight'], *mm, no_gt=no_gt)
    assert loss.shape == () and loss.dtype == torch.float32
    (loss * upstream).backward()
    torch.cuda.synchronize()
    return tuple(x.detach().double().cpu().numpy() for x in (loss, t0.grad, t1.grad, a.grad))


def _rel(got, ref):
    d = float(np.linalg.norm(np.ravel(got) - np.ravel(ref)))
    n = float(np.linalg.norm(np.ravel(ref)))
    return d / n if n > 0 else d


def regimes(tag, conf, ids, masks, need_confident=True):
    """Prints where the float64 entries lie; asserts that none is in the regime no fp32 evaluation resolves."""
    live = np.ones(conf.shape, bool) if masks is None else (masks[0][:, :, None] & masks[1][:, None, :])
    neg = live.copy()
    neg[tuple(x.numpy() for x in ids)] = False
    p = conf[neg]
    near = int(((1 - conf[live] > 1e-6) & (1 - conf[live] < 1e-3)).sum())
    conf_neg, tiny = int((p > 0.5).sum()), int((p < 1e-6).sum())
    print(f'[{tag}] negatives: {p.size}, of them p > 0.5: {conf_neg}, p < 1e-6: {tiny}; max p = {conf[live].max():.4f}; '
          f'entries with 1e-6 < 1 - p < 1e-3: {near}')
    assert near == 0, f'{tag}: {near} entries in the regime that fp32 cannot resolve'
    if need_confident:
        assert conf_neg > 0, f'{tag}: no confident negative'


def compare(tag, got, ref, r32):
    """loss within max(1e-5, dev32) relative, the three gradients within max(1e-3, dev32)."""
    bad = []
    for k, what, bar in ((0, 'loss', LOSS_BAR), (1, 'dF0', GRAD_BAR), (2, 'dF1', GRAD_BAR), (3, 'd bin_score', GRAD_BAR)):
        assert np.isfinite(got[k]).all(), what
        e, e32 = _rel(got[k], ref[k]), _rel(r32[k], ref[k])
        print(f'[{tag}] {what}: relative error {e:.3e}   bar {max(bar, e32):.1e} (derived {bar:.0e}, fp32 autograd {e32:.3e})   '
              f'|reference| {float(np.linalg.norm(np.ravel(ref[k]))):.3e}')
        if not e <= max(bar, e32):
            bad.append(f'{tag} {what}: {e:.3e} > {max(bar, e32):.1e}')
    assert not bad, '; '.join(bad)


def three_legs(tag, f0, f1, alpha, T, ids, masks, focal, no_gt=False, need_confident=True, loss_fn=None, kernel_ids=None):
    ref = torch_leg(f0, f1, alpha, T, ids, masks, focal, torch.float64, 'cpu', no_gt, loss_fn)
    r32 = torch_leg(f0, f1, alpha, T, ids, masks, focal, torch.float32, 'cuda', no_gt, loss_fn)
    got = kernel_leg(f0, f1, alpha, T, kernel_ids or ids, masks, focal, no_gt)
    regimes(tag, ref[4], ids if not no_gt else tuple(torch.zeros(0, dtype=torch.long) for _ in range(3)), masks, need_confident)
    compare(tag, got, ref, r32)
    return got, ref


@pytest.mark.parametrize('alpha', [1.0, -0.5])
@pytest.mark.parametrize('T', [1, 3, 6])
@pytest.mark.parametrize('name', list(SHAPES))
def test_loss_and_gradients_match_float64_autograd(name, T, alpha):
    f0, f1, ids, _ = make(name, seed=3)
    for wname, focal in (('equal', EQUAL), ('0.3/300', NEG_HEAVY)):
        three_legs(f'{name} T={T} bin={alpha} weights {wname}', f0, f1, alpha, T, ids, None, focal, need_confident=T >= 3)


def test_amplitude_6():
    f0, f1, ids, _ = make('1x768x560', seed=4, amp=6.0)
    three_legs('1x768x560 amp 6 T=3', f0, f1, 1.0, 3, ids, None, NEG_HEAVY)


@pytest.mark.parametrize('name', ['1x35x72', '2x192x136'])
def test_padded_masks(name):
    f0, f1, ids, masks = make(name, seed=5, masked=True)
    for T, focal in ((3, EQUAL), (1, NEG_HEAVY)):
        got, _ = three_legs(f'{name} masked T={T}', f0, f1, 1.0, T, ids, masks, focal, need_confident=T >= 3)
        assert (~masks[0]).any() and (~masks[1]).any()
        assert (got[1][~masks[0]] == 0).all() and (got[2][~masks[1]] == 0).all()          # masked rows / columns: exactly 0
        assert np.abs(got[1][masks[0]]).max() > 0 and np.abs(got[2][masks[1]]).max() > 0


def test_zero_iterations_everything_is_clamped():
    """skh_iters = 0: P = exp(Zc - norm) > 1 everywhere, every entry is clamped from above: a constant loss, gradients exactly zero (as
    float64 gives).  The fp32 reference cannot form 1 - (1 - 1e-6) (dev32 ~ 1e-3 on the loss); the kernels add the constant in float64."""
    f0, f1, ids, _ = make('2x192x136', seed=6)
    ref = torch_leg(f0, f1, 1.0, 0, ids, None, EQUAL, torch.float64, 'cpu')
    r32 = torch_leg(f0, f1, 1.0, 0, ids, None, EQUAL, torch.float32, 'cuda')
    got = kernel_leg(f0, f1, 1.0, 0, ids, None, EQUAL)
    assert ref[4].min() > 1.0
    e, e32 = _rel(got[0], ref[0]), _rel(r32[0], ref[0])
    print(f'[T = 0] loss: relative error {e:.3e}   bar {max(LOSS_BAR, e32):.1e} (fp32 autograd {e32:.3e})')
    assert e <= max(LOSS_BAR, e32)
    for k in (1, 2, 3):
        assert np.abs(ref[k]).max() == 0 and np.abs(got[k]).max() == 0


@pytest.mark.parametrize('masked', [False, True])
def test_no_ground_truth(masked):
    f0, f1, ids, masks = make('2x192x136', seed=7, masked=masked)
    none = tuple(torch.zeros(0, dtype=torch.long) for _ in range(3))
    got, _ = three_legs(f'no ground truth masked={masked}', f0, f1, 1.0, 3, ids, masks, NEG_HEAVY, no_gt=True)
    again = kernel_leg(f0, f1, 1.0, 3, none, masks, NEG_HEAVY, no_gt=True)               # M = 0 labels with no_gt: the same call
    for x, y in zip(got, again):
        np.testing.assert_array_equal(x, y)


def test_multiset_form_is_the_dense_loss_for_distinct_labels():
    from far_amd import losses
    f0, f1, ids, masks = make('2x192x136', seed=5, masked=True)
    conf = definition(torch.from_numpy(f0).double(), torch.from_numpy(f1).double(), torch.tensor(1.0).double(), 3,
                      *(torch.from_numpy(m) for m in masks))[:, :-1, :-1]
    w = (torch.from_numpy(masks[0])[:, :, None] & torch.from_numpy(masks[1])[:, None, :]).double()
    a = losses.coarse_focal_loss_dense_torch(conf, ids, False, weight=w, **NEG_HEAVY)
    b = multiset_loss(conf, ids, weight=w, **NEG_HEAVY)
    assert abs(float(a) - float(b)) <= 1e-12 * abs(float(a))


def test_a_label_given_twice():
    """One label twice: two positive terms, M + 1 in the normalisers (module docstring)."""
    f0, f1, ids, _ = make('1x35x72', seed=8)
    twice = tuple(torch.cat([x, x[:1]]) for x in ids)
    three_legs('label twice', f0, f1, 1.0, 3, twice, None, EQUAL, need_confident=False, loss_fn=multiset_loss)


def test_out_of_range_labels_are_ignored_not_read():
    """Labels outside the grid add nothing and are never used as an index; they count in M.  The float64 leg: the multiset form on the
    labels in range, its two weights scaled to the normalisers of M + 4 labels."""
    f0, f1, ids, _ = make('1x35x72', seed=9)
    L, S = f0.shape[1], f1.shape[1]
    M, n = int(ids[0].numel()), L * S
    bad = (torch.tensor([0, 0, 5, -1]), torch.tensor([L, 3, 0, 0]), torch.tensor([0, S + 7, 0, 0]))
    both = tuple(torch.cat([a, b]) for a, b in zip(ids, bad))
    focal = dict(EQUAL, pos_weight=EQUAL['pos_weight'] * M / (M + 4), neg_weight=EQUAL['neg_weight'] * (n - M) / (n - M - 4))
    ref = torch_leg(f0, f1, 1.0, 3, ids, None, focal, torch.float64, 'cpu', loss_fn=multiset_loss)
    r32 = torch_leg(f0, f1, 1.0, 3, ids, None, focal, torch.float32, 'cuda', loss_fn=multiset_loss)
    got = kernel_leg(f0, f1, 1.0, 3, both, None, EQUAL)
    compare('out-of-range labels', got, ref, r32)


def test_gamma_is_a_run_time_number():
    f0, f1, ids, _ = make('2x192x136', seed=10)
    got, ref = three_legs('gamma 1.5', f0, f1, 1.0, 3, ids, None, dict(NEG_HEAVY, gamma=1.5))
    two = kernel_leg(f0, f1, 1.0, 3, ids, None, NEG_HEAVY)
    assert got[0] != two[0]


@pytest.mark.parametrize('log2_scale', [-12, 12])
def test_upstream_power_of_two_scales_every_gradient_exactly(log2_scale):
    f0, f1, ids, masks = make('2x192x136', seed=5, masked=True)
    base = kernel_leg(f0, f1, 1.0, 3, ids, masks, NEG_HEAVY)
    sc = 2.0 ** log2_scale
    got = kernel_leg(f0, f1, 1.0, 3, ids, masks, NEG_HEAVY, upstream=sc)
    assert np.abs(base[1]).max() > 0 and base[3] != 0
    for k in (1, 2, 3):
        np.testing.assert_array_equal(got[k], base[k] * sc)


def test_two_runs_give_the_same_bits():
    for name, masked in (('1x768x560', False), ('2x192x136', True)):
        f0, f1, ids, masks = make(name, seed=11, masked=masked)
        a = kernel_leg(f0, f1, -0.5, 3, ids, masks, NEG_HEAVY)
        b = kernel_leg(f0, f1, -0.5, 3, ids, masks, NEG_HEAVY)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def test_a_pair_does_not_depend_on_the_rest_of_the_batch():
    """Pair 0's feature gradients in a batch of two = those of pair 0 alone, bit for bit.  The normalisers are the batch's: with as
    many labels on pair 1 as on pair 0, N L S - M and M both double from the one-pair run to the batch, so the one-pair run is given
    HALF of neg_weight and of pos_weight -- a power of two, the two runs then use the same floats."""
    f0, f1, ids, _ = make('2x192x136', seed=12)
    b, i, j = (x.numpy() for x in ids)
    k0, k1 = np.nonzero(b == 0)[0], np.nonzero(b == 1)[0]
    m = min(len(k0), len(k1))
    sel = np.sort(np.concatenate([k0[:m], k1[:m]]))
    two = tuple(torch.from_numpy(x[sel]) for x in (b, i, j))
    one = tuple(torch.from_numpy(x[np.sort(k0[:m])]) for x in (b, i, j))
    batch = kernel_leg(f0, f1, 1.0, 3, two, None, NEG_HEAVY)
    half = dict(NEG_HEAVY, pos_weight=NEG_HEAVY['pos_weight'] / 2, neg_weight=NEG_HEAVY['neg_weight'] / 2)
    alone = kernel_leg(f0[:1], f1[:1], 1.0, 3, one, None, half)
    assert np.abs(alone[1]).max() > 0
    np.testing.assert_array_equal(batch[1][0], alone[1][0])
    np.testing.assert_array_equal(batch[2][0], alone[2][0])


def test_no_tensor_of_the_matrix_size_is_allocated():
    """1x768x560: forward + backward raise the allocator's peak by less than ONE fp32 L x S matrix above the workspace."""
    from far_amd import _lib, ops
    f0n, f1n, ids, _ = make('1x768x560', seed=3)
    L, S = f0n.shape[1], f1n.shape[1]
    f0 = torch.from_numpy(f0n).cuda().requires_grad_(True)
    f1 = torch.from_numpy(f1n).cuda().requires_grad_(True)
    a = torch.tensor(1.0, device='cuda', requires_grad=True)
    idd = tuple(x.cuda() for x in ids)
    ws = _lib.load().far_sinkhorn_dense_focal_workspace_bytes(1, L, S, C, 3, int(ids[0].numel()))
    assert 0 < ws
    ops.overflow_flag(f0.device)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    loss = ops.sinkhorn_dense_focal_loss(f0, f1, a, 3, *idd, **NEG_HEAVY)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f'[ot dense memory] forward + backward at 768 x 560: peak + {peak} B, workspace {ws} B, one fp32 L x S matrix {4 * L * S} B')
    assert torch.isfinite(loss) and float(f0.grad.abs().max()) > 0
    assert peak - ws < 4 * L * S, (peak, ws)
    with torch.no_grad():                                  # validation: the forward alone
        v = ops.sinkhorn_dense_focal_loss(f0, f1, a, 3, *idd, **NEG_HEAVY)
    assert torch.equal(v, loss.detach()) and not v.requires_grad


def test_refusals_and_empty_inputs():
    from far_amd import ops
    f0n, f1n, ids, _ = make('1x35x72', seed=8)
    f0, f1 = torch.from_numpy(f0n).cuda(), torch.from_numpy(f1n).cuda()
    a = torch.tensor(1.0, device='cuda', requires_grad=True)
    idd = tuple(x.cuda() for x in ids)
    with pytest.raises(NotImplementedError):
        ops.sinkhorn_dense_focal_loss(f0, f1, a, 49, *idd, **EQUAL)
    with pytest.raises(NotImplementedError):
        ops.sinkhorn_dense_focal_loss(f0[..., :128].contiguous(), f1[..., :128].contiguous(), a, 3, *idd, **EQUAL)
    e0 = torch.zeros(0, 35, C, device='cuda', requires_grad=True)
    e1 = torch.zeros(0, 72, C, device='cuda', requires_grad=True)
    none = tuple(torch.zeros(0, dtype=torch.long, device='cuda') for _ in range(3))
    z = ops.sinkhorn_dense_focal_loss(e0, e1, a, 3, *none, **EQUAL)
    assert float(z) == 0 and z.requires_grad
    z.backward()
    assert e0.grad.shape == (0, 35, C) and float(a.grad) == 0
