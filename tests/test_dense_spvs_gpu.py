"""Dense coarse supervision on the GPU (ops.coarse_dense_focal_loss: far_coarse_dense_focal_f16s / far_coarse_dense_focal_bwd_f16)
against float64 torch autograd of the loss on a dense float64 conf_matrix (tests/vendor_ops.conf_matrix +
losses.coarse_focal_loss_dense_torch; golden G23 pins that formula to the reference, tests/test_dense_spvs_cpu.py).

Bars: the loss within 1e-5 relative (the project's confidence bar against float64), dF0 / dF1 within 1e-3 relative Frobenius (K1's
training-gradient contract, dual_softmax_bwd_f16.hip).  Measured values: profiles/dense_spvs_parity.txt.

The inputs: f1 holds noisy copies of f0's rows at permuted columns (confident mutual matches, p > 1 - 1e-6 in float64), some rows of
f0 are near-duplicates of each other at three distances (their 2 x 2 blocks of entries share the mass: p from ~1e-3 to ~0.5), all
other entries are far below 1e-6.  The labels are a strict subset of the correlated pairs, so confident negatives exist.  One regime
is left out on purpose: 1e-6 < 1 - p < ~1e-3.  There dLoss/dp ~ 1 / (1 - p) turns the 1e-7 absolute resolution of an fp32 p (of any
fp32 softmax, the reference's included) into more than 1e-3 of W; no fp32 evaluation can meet the gradient bar there."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 0.1
LOSS_BAR = 1e-5
GRAD_BAR = 1e-3
FOCAL = dict(alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0)
# the negatives' mean divides by ~N L S, the positives' by M: with equal weights the positives carry the gradient.  The second
# setting lets the dense negative part dominate it.
NEG_HEAVY = dict(alpha=0.25, gamma=2.0, pos_weight=0.3, neg_weight=300.0)
SHAPES = {'2x48x48': (2, (6, 8), (6, 8)), '1x35x72': (1, (5, 7), (8, 9)), '3x192x192': (3, (12, 16), (12, 16))}


def make_inputs(N, L, S, seed, amp=2.0):
    """-> f0 (N, L, 256), f1 (N, S, 256) fp32 numpy, labels (pb, pi, pj) int64 numpy."""
    rng = np.random.default_rng(seed)
    f0 = (amp * rng.standard_normal((N, L, 256))).astype(np.float32)
    f1 = (amp * rng.standard_normal((N, S, 256))).astype(np.float32)
    pb, pi, pj = [], [], []
    K = min(L, S) - 3                                     # a few rows and columns stay without a partner
    for n in range(N):
        rows, cols = rng.permutation(L)[:K], rng.permutation(S)[:K]
        for k, d in zip(range(0, 12, 2), (0.05, 0.3, 0.5, 0.05, 0.3, 0.5)):      # six pairs of near-duplicate rows
            f0[n, rows[k + 1]] = f0[n, rows[k]] + d * rng.standard_normal(256).astype(np.float32)
        f1[n, cols] = f0[n, rows] + 0.02 * rng.standard_normal((K, 256)).astype(np.float32)
        lab = np.concatenate([np.arange(0, 12, 3), 12 + rng.permutation(K - 12)[:int(0.6 * (K - 12))]])   # a strict subset
        pb += [n] * len(lab); pi += rows[lab].tolist(); pj += cols[lab].tolist()
    order = np.lexsort((pi, pb))                          # (b, i) order, as torch.where emits the labels
    return f0, f1, tuple(np.asarray(a, np.int64)[order] for a in (pb, pi, pj))


def make_masks(N, hw0, hw1):
    m0 = np.zeros((N,) + hw0, bool)
    m1 = np.zeros((N,) + hw1, bool)
    for n in range(N):                                    # per-sample valid extents differ
        m0[n, :hw0[0] - (n % 2), :hw0[1] - 2 * ((n + 1) % 2)] = True
        m1[n, :hw1[0] - 1 - (n % 2), :hw1[1] - (n % 2)] = True
    return m0, m1


def torch_loss(f0, f1, ids, no_gt, focal, m0=None, m1=None):
    """The definition: dense conf_matrix + the torch form of the loss, in the dtype of f0."""
    from far_amd import losses
    from tests import vendor_ops
    N, L, S = f0.shape[0], f0.shape[1], f1.shape[1]
    conf = vendor_ops.conf_matrix(f0, f1, T, None if m0 is None else m0.reshape(N, L), None if m1 is None else m1.reshape(N, S))
    weight = None if m0 is None else (m0.reshape(N, L)[..., None] * m1.reshape(N, S)[:, None]).to(conf.dtype)
    loss = losses.coarse_focal_loss_dense_torch(conf, ids, no_gt, focal['alpha'], focal['gamma'], focal['pos_weight'],
                                                focal['neg_weight'], weight)
    return loss, conf


def run_torch(f0n, f1n, ids, no_gt, focal, dtype, masks=None):
    f0 = torch.from_numpy(f0n).cuda().to(dtype).requires_grad_(True)
    f1 = torch.from_numpy(f1n).cuda().to(dtype).requires_grad_(True)
    m = (None, None) if masks is None else tuple(torch.from_numpy(a).cuda() for a in masks)
    loss, conf = torch_loss(f0, f1, ids, no_gt, focal, *m)
    loss.backward()
    return float(loss.detach()), f0.grad.double(), f1.grad.double(), conf.detach()


def run_hip(f0n, f1n, ids, no_gt, focal, masks=None, split_g=None):
    from far_amd import ops
    from far_amd.ops import coarse
    f0 = torch.from_numpy(f0n).cuda().requires_grad_(True)
    f1 = torch.from_numpy(f1n).cuda().requires_grad_(True)
    m = (None, None) if masks is None else tuple(torch.from_numpy(a).cuda() for a in masks)
    keep = coarse.DENSE_FOCAL_SPLIT_G
    if split_g is not None:
        coarse.DENSE_FOCAL_SPLIT_G = split_g
    try:
        loss = ops.coarse_dense_focal_loss(f0, f1, *ids, T, focal['alpha'], focal['gamma'], focal['pos_weight'], focal['neg_weight'],
                                           m[0], m[1], no_gt=no_gt)
        assert loss.shape == () and loss.dtype == torch.float32
        loss.backward()
    finally:
        coarse.DENSE_FOCAL_SPLIT_G = keep
    return loss.detach().clone(), f0.grad.clone(), f1.grad.clone()


@functools.lru_cache(maxsize=None)
def case(name, masked=False):
    """Inputs of one shape: features, labels on the GPU, masks (computed once, shared, never modified)."""
    N, hw0, hw1 = SHAPES[name]
    L, S = hw0[0] * hw0[1], hw1[0] * hw1[1]
    f0n, f1n, lab = make_inputs(N, L, S, seed=N * 1000 + L + S)
    ids = tuple(torch.from_numpy(a).cuda() for a in lab)
    masks = make_masks(N, hw0, hw1) if masked else None
    return f0n, f1n, ids, masks


def rel(x, y):
    return float((x.double() - y).norm() / y.norm())


def compare(tag, f0n, f1n, ids, no_gt, focal, masks=None, regimes=True):
    ref = run_torch(f0n, f1n, ids, no_gt, focal, torch.float64, masks)
    if regimes:
        conf = ref[3]
        neg = torch.ones_like(conf, dtype=torch.bool)
        neg[ids] = False
        if masks is not None:
            N = conf.shape[0]
            w = torch.from_numpy(masks[0]).cuda().reshape(N, -1)[..., None] & torch.from_numpy(masks[1]).cuda().reshape(N, -1)[:, None]
            neg &= w
        n_lo, n_hi = int((conf[neg] < 1e-6).sum()), int((conf[neg] > 1 - 1e-6).sum())
        n_mid = int(neg.sum()) - n_lo - n_hi
        print(f'[dense {tag}] negatives: {n_lo} below 1e-6, {n_mid} inside the clamp, {n_hi} above 1 - 1e-6; labels {ids[0].numel()}')
        assert n_lo > 0 and n_mid > 0 and n_hi > 0
        danger = int(((1 - conf > 1e-6) & (1 - conf < 1e-3)).sum())
        assert danger == 0, danger                      # the regime the module docstring leaves out stays empty
    r32 = run_torch(f0n, f1n, ids, no_gt, focal, torch.float32, masks)
    out = {}
    for form, split in (('hi+lo G', True), ('fp16 G', False)):
        loss, g0, g1 = run_hip(f0n, f1n, ids, no_gt, focal, masks, split_g=split)
        out[form] = (abs(float(loss) - ref[0]) / abs(ref[0]), rel(g0, ref[1]), rel(g1, ref[2]), loss, g0, g1)
    e32 = (abs(r32[0] - ref[0]) / abs(ref[0]), rel(r32[1], ref[1]), rel(r32[2], ref[2]))
    for form, e in list(out.items()) + [('fp32 torch dense', e32)]:
        print(f'[dense {tag}] {form:17s} loss {e[0]:.2e}  dF0 {e[1]:.2e}  dF1 {e[2]:.2e}   (float64 loss {ref[0]:.6e})')
    return out, ref


@pytest.mark.parametrize('name', list(SHAPES))
@pytest.mark.parametrize('weights', ['equal', 'neg_heavy'])
def test_loss_and_gradients_match_float64(name, weights):
    from far_amd.ops import coarse
    f0n, f1n, ids, _ = case(name)
    out, _ = compare(f'{name} {weights}', f0n, f1n, ids, False, FOCAL if weights == 'equal' else NEG_HEAVY)
    e = out['hi+lo G' if coarse.DENSE_FOCAL_SPLIT_G else 'fp16 G']
    # measured on MI355X (profiles/dense_spvs_parity.txt): loss 3.0e-8 .. 3.4e-6; dF0 / dF1 3.8e-4 .. 5.9e-4 with G as an fp16 hi + lo pair,
    # 5.4e-4 .. 8.5e-4 with G as one fp16 (both meet the bar; the pair is the default).  fp32 torch dense autograd on the same inputs:
    # loss 2.4e-4 .. 9.5e-4, gradients 5e-6 .. 2e-5
    assert e[0] < LOSS_BAR, e[0]
    assert e[1] < GRAD_BAR and e[2] < GRAD_BAR, e[1:3]


def test_gamma_is_a_run_time_number():
    f0n, f1n, ids, _ = case('2x48x48')
    for gamma in (2.0, 1.5):
        out, _ = compare(f'2x48x48 gamma={gamma}', f0n, f1n, ids, False, dict(NEG_HEAVY, gamma=gamma), regimes=False)
        e = out['hi+lo G']
        assert e[0] < LOSS_BAR and e[1] < GRAD_BAR and e[2] < GRAD_BAR, (gamma, e[:3])
    a = run_hip(f0n, f1n, ids, False, dict(NEG_HEAVY, gamma=2.0))
    b = run_hip(f0n, f1n, ids, False, dict(NEG_HEAVY, gamma=1.5))
    assert float(a[0]) != float(b[0])


@pytest.mark.parametrize('masked', [False, True])
def test_no_ground_truth(masked):
    """M = 0 labels and spvs_coarse's dummy label (0, 0, 0) both give the no-ground-truth value of the definition (G23's
    nogt / nogt_weight cases pin it to the reference): finite, and the positive term contributes nothing."""
    f0n, f1n, ids, masks = case('2x48x48', masked)
    empty = tuple(torch.zeros(0, dtype=torch.int64).cuda() for _ in range(3))
    dummy = tuple(torch.zeros(1, dtype=torch.int64).cuda() for _ in range(3))
    focal = dict(NEG_HEAVY, pos_weight=5.0)
    ref = run_torch(f0n, f1n, empty, True, focal, torch.float64, masks)
    ref0 = run_torch(f0n, f1n, empty, True, dict(focal, pos_weight=0.0), torch.float64, masks)
    assert ref[0] == ref0[0]
    got = [run_hip(f0n, f1n, lab, True, focal, masks) for lab in (empty, dummy)]
    for loss, g0, g1 in got:
        assert torch.isfinite(loss) and torch.isfinite(g0).all() and torch.isfinite(g1).all()
        e = (abs(float(loss) - ref[0]) / abs(ref[0]), rel(g0, ref[1]), rel(g1, ref[2]))
        print(f'[dense no-gt masked={masked}] loss {e[0]:.2e}  dF0 {e[1]:.2e}  dF1 {e[2]:.2e}')
        assert e[0] < LOSS_BAR and e[1] < GRAD_BAR and e[2] < GRAD_BAR, e
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)
    other = run_hip(f0n, f1n, empty, True, dict(focal, pos_weight=0.0), masks)     # pos_weight has no say without ground truth
    assert torch.equal(other[0], got[0][0]) and torch.equal(other[1], got[0][1])


@pytest.mark.parametrize('name', ['2x48x48', '1x35x72'])
def test_padded_masks(name):
    f0n, f1n, ids, masks = case(name, True)
    out, _ = compare(f'{name} masked', f0n, f1n, ids, False, NEG_HEAVY, masks)
    e = out['hi+lo G']
    assert e[0] < LOSS_BAR and e[1] < GRAD_BAR and e[2] < GRAD_BAR, e[:3]
    N = f0n.shape[0]
    for g, m in ((e[4], masks[0]), (e[5], masks[1])):
        dead = ~torch.from_numpy(m).cuda().reshape(N, -1)
        assert int(dead.sum()) > 0 and float(g[dead].abs().max()) == 0.0          # rows of masked cells: exactly 0
        assert float(g[~dead].abs().max()) > 0


def test_two_runs_give_the_same_bits():
    f0n, f1n, ids, masks = case('3x192x192')
    a = run_hip(f0n, f1n, ids, False, NEG_HEAVY)
    b = run_hip(f0n, f1n, ids, False, NEG_HEAVY)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    f0n, f1n, ids, masks = case('2x48x48', True)
    a = run_hip(f0n, f1n, ids, False, FOCAL, masks)
    b = run_hip(f0n, f1n, ids, False, FOCAL, masks)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_no_tensor_of_the_matrix_size_is_allocated():
    """N = 1 at 60 x 80: forward + backward raise the allocator's peak by less than ONE fp32 L x S matrix (92.16 MB)."""
    from far_amd import ops
    L = 4800
    f0n, f1n, lab = make_inputs(1, L, L, seed=5)
    ids = tuple(torch.from_numpy(a).cuda() for a in lab)
    f0 = torch.from_numpy(f0n).cuda().requires_grad_(True)
    f1 = torch.from_numpy(f1n).cuda().requires_grad_(True)
    ops.overflow_flag(f0.device)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    loss = ops.coarse_dense_focal_loss(f0, f1, *ids, T, **FOCAL)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f'[dense memory] forward + backward at 60 x 80: peak + {peak / 1e6:.2f} MB (one fp32 L x S matrix: {4 * L * L / 1e6:.2f} MB)')
    assert torch.isfinite(loss) and float(f0.grad.abs().max()) > 0
    assert peak < 4 * L * L, peak
    with torch.no_grad():                                  # validation: the forward alone, nothing kept for a backward
        v = ops.coarse_dense_focal_loss(f0, f1, *ids, T, **FOCAL)
    assert torch.equal(v, loss.detach()) and not v.requires_grad


def test_train_step_in_the_model():
    """pipeline.train_step of a sparse_spvs = False model runs on the new path (no conf_matrix) and its parameter gradients agree
    with the vendor dense leg (materialize_conf: tests/vendor_ops.conf_matrix + the torch loss, fp32 autograd) within the bar of the
    in-model K1 test (tests/test_train_kernels_gpu.py); the same model with sparse_spvs = True is untouched by it."""
    from far_amd import synth
    from far_amd.config import RunCfg, far_train_config
    from far_amd.loftr import LoFTR
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import train_step
    cfg = far_train_config()
    cfg['loftr']['loss']['neg_weight'] = 300.0            # the dense negative part carries a visible share of the gradient
    m = LoFTR(cfg['loftr'])
    synth.load_synthetic(m, seed=0)
    m = m.cuda().train()
    base = synth.synth_training_batch(1, seed=79, device='cuda')
    keys = ['backbone.layer3_outconv.weight', 'loftr_coarse.layers.0.q_proj.weight', 'loftr_coarse.layers.5.mlp.2.weight',
            'loftr_coarse.layers.3.norm1.bias', 'backbone.conv1.weight']
    P = dict(m.named_parameters())

    def step(sparse_spvs, materialize):
        cfg['loftr']['match_coarse']['sparse_spvs'] = sparse_spvs
        m.coarse_matching.config['sparse_spvs'] = sparse_spvs
        m.coarse_matching.materialize_conf = materialize
        loss_fn = LoFTRLoss(cfg).train()
        batch = dict(base)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        train_step(m, batch, loss_fn, RunCfg('prior_ransac', 2), H=256, seed=0)
        batch['loss'].backward()
        torch.cuda.synchronize()
        return batch, {k: P[k].grad.detach().double().clone() for k in keys}

    b_sparse, g_sparse = step(True, False)
    assert b_sparse['conf_matrix'] is None and b_sparse.get('conf_pos') is not None and 'conf_dense' not in b_sparse
    b_new, g_new = step(False, False)
    assert b_new['conf_matrix'] is None and b_new.get('conf_dense') is not None and 'conf_pos' not in b_new
    b_ref, g_ref = step(False, True)
    assert b_ref['conf_matrix'] is not None and 'conf_dense' not in b_ref
    lc_new, lc_ref = float(b_new['loss_scalars']['loss_c']), float(b_ref['loss_scalars']['loss_c'])
    print(f'[dense in model] loss_c {lc_new:.8f} vs vendor dense leg {lc_ref:.8f}; sparse-supervision loss_c '
          f'{float(b_sparse["loss_scalars"]["loss_c"]):.8f}')
    assert len(b_new['b_ids']) == len(b_ref['b_ids'])
    assert abs(lc_new - lc_ref) < 1e-4 * abs(lc_ref), (lc_new, lc_ref)
    assert lc_new != float(b_sparse['loss_scalars']['loss_c'])
    for k in keys:
        r = float((g_new[k] - g_ref[k]).norm() / g_ref[k].norm())
        print(f'[dense in model] {k}: |grad| = {float(g_ref[k].norm()):.3e}, relative Frobenius difference {r:.3e}')
        assert r < 3e-3, (k, r)
    b_again, g_again = step(True, False)                  # sparse supervision after the dense steps: the gradients it gave before
    for k in keys:
        assert torch.equal(g_sparse[k], g_again[k]), k
