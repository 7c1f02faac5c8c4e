"""Training an optimal-transport model (match_type 'sinkhorn') end to end on the GPU: pipeline.train_step + LoFTRLoss + AdamW, the
coarse term against dense autograd of the definition on the same coarse features, padded masks, validation with and without the
prefilter -- and the dual-softmax training step next to it, unchanged."""
import copy

import numpy as np
import pytest
import torch

from far_amd import synth
from far_amd.config import RunCfg, far_train_config

pytestmark = pytest.mark.gpu

FEAT_GAIN = 4.0        # the synthetic checkpoint's coarse features are ~unit scale; scaled so that the matcher is confident
GRAD_BAR = 1e-3        # tests/test_sinkhorn_train_gpu.py


def _ot_config(**kw):
    cfg = far_train_config()
    cfg['loftr']['match_coarse'].update(match_type='sinkhorn', **kw)
    return cfg


def _ot_model(cfg, gain=FEAT_GAIN):
    """The synthetic checkpoint of the dual-softmax model (tests/test_sinkhorn_gpu.py: _ot_model) with bin_score = 1; the coarse
    features are scaled on their way into the matcher and kept (with their gradient) for the caller."""
    from far_amd.loftr import LoFTR
    m = LoFTR(cfg['loftr'])
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if k != 'coarse_matching.bin_score'}
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synthetic_state_dict(shapes, 0).items()}, strict=False)
    assert res.missing_keys == ['coarse_matching.bin_score'] and not res.unexpected_keys
    with torch.no_grad():
        m.coarse_matching.bin_score.fill_(1.0)
    m = m.cuda()
    captured = {}

    def hook(mod, args):
        a0, a1 = args[0] * gain, args[1] * gain
        if a0.requires_grad:
            a0.retain_grad(); a1.retain_grad()
        captured['f0'], captured['f1'] = a0, a1
        return (a0, a1) + tuple(args[2:])
    m.coarse_matching.register_forward_pre_hook(hook)
    return m, captured


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def test_train_step_two_pairs_and_optimizer_step():
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import train_step
    cfg = _ot_config()
    m, _ = _ot_model(cfg)
    m.train()
    loss_fn = LoFTRLoss(cfg).train()
    base = synth.synth_training_batch(2, seed=77, device='cuda')
    state = copy.deepcopy(m.state_dict())
    runs = []
    for _ in range(2):
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        batch = dict(base)
        torch.manual_seed(5)
        train_step(m, batch, loss_fn, RunCfg('prior_ransac', 2), H=512, seed=0)
        batch['loss'].backward()
        torch.cuda.synchronize()
        runs.append((batch['loss'].detach().clone(), _grads(m)))
    L = 4800
    assert batch['conf_matrix'] is None and 'conf_matrix_with_bin' not in batch
    assert batch['conf_pos'].shape == base['spv_b_ids'].shape and batch['conf_pos'].requires_grad
    assert batch['conf_bin0'].shape == (2, L) and batch['conf_bin1'].shape == (2, L)
    assert len(batch['b_ids']) == int(2 * L * m.coarse_matching.train_coarse_percent)      # sampled / padded (:205-240)
    assert torch.isfinite(batch['loss']).all() and set(batch['loss_scalars']) >= {'loss', 'loss_c', 'loss_f', 'loss_rot', 'loss_tr'}
    print(f'[ot train_step] loss {float(batch["loss"]):.6f}  loss_c {float(batch["loss_scalars"]["loss_c"]):.6f}  '
          f'd bin_score {float(m.coarse_matching.bin_score.grad):.4e}')
    g = runs[1][1]
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(g['coarse_matching.bin_score'].abs()) > 0
    for k in g:
        if k.startswith('loftr_coarse.') or k.startswith('backbone.layer3'):
            assert float(g[k].abs().max()) > 0, k
    # two runs from the same state: the same bits
    assert torch.equal(runs[0][0], runs[1][0])
    for k in g:
        assert torch.equal(runs[0][1][k], g[k]), k
    before = float(m.coarse_matching.bin_score.detach())
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    opt.step()
    assert float(m.coarse_matching.bin_score.detach()) != before


def test_coarse_term_and_feature_gradients_match_dense_autograd():
    """The coarse term of the model's training forward and its gradient w.r.t. the coarse features (and bin_score) against
    conf_matrix_with_bin + the reference-style loss composed densely with torch autograd on the same features: float64 is the
    reference, the fp32 composition gives dev32 -- the max(1e-3, dev32) rule of tests/test_sinkhorn_train_gpu.py."""
    from far_amd import losses
    from tests.test_sinkhorn_train_gpu import definition
    cfg = _ot_config()
    cfg['loftr']['regress_rt'] = False
    m, cap = _ot_model(cfg)
    m.train()
    base = synth.synth_training_batch(2, seed=78, device='cuda')
    data = {k: base[k] for k in ('image0', 'image1', 'spv_b_ids', 'spv_i_ids', 'spv_j_ids')}
    torch.manual_seed(5)
    m(data, train=True)
    lc = cfg['loftr']['loss']
    loss = losses.coarse_focal_loss_sinkhorn(data, lc['focal_alpha'], lc['focal_gamma'], lc['pos_weight'], lc['neg_weight'])
    loss.backward()
    got = (float(loss), cap['f0'].grad.double(), cap['f1'].grad.double(), m.coarse_matching.bin_score.grad.double())
    ids = (data['spv_b_ids'], data['spv_i_ids'], data['spv_j_ids'])

    def dense(dtype):
        f0 = cap['f0'].detach().to(dtype).requires_grad_(True)
        f1 = cap['f1'].detach().to(dtype).requires_grad_(True)
        a = m.coarse_matching.bin_score.detach().to(dtype).requires_grad_(True)
        P = definition(f0, f1, a, m.coarse_matching.skh_iters)
        d = {'conf_matrix_with_bin': P, 'spv_b_ids': ids[0], 'spv_i_ids': ids[1], 'spv_j_ids': ids[2], 'spv_gt_count': int(ids[0].numel())}
        l_ = losses.coarse_focal_loss_sinkhorn(d, lc['focal_alpha'], lc['focal_gamma'], lc['pos_weight'], lc['neg_weight'])
        l_.backward()
        return float(l_), f0.grad.double(), f1.grad.double(), a.grad.double()
    ref, r32 = dense(torch.float64), dense(torch.float32)
    rel = lambda x, y: float((x - y).norm() / y.norm())
    e_loss, e32_loss = abs(got[0] - ref[0]) / abs(ref[0]), abs(r32[0] - ref[0]) / abs(ref[0])
    print(f'[ot coarse term] loss {got[0]:.8f} vs float64 {ref[0]:.8f}: relative {e_loss:.2e} (fp32 composition {e32_loss:.2e})')
    assert e_loss <= max(2e-5, e32_loss)
    bad = []
    for k, what in ((1, 'd feat_c0'), (2, 'd feat_c1'), (3, 'd bin_score')):
        e, e32 = rel(got[k], ref[k]), rel(r32[k], ref[k])
        print(f'[ot coarse term] {what}: relative error {e:.3e}   bar {max(GRAD_BAR, e32):.1e} (fp32 composition {e32:.3e})   '
              f'|reference| {float(ref[k].norm()):.3e}')
        if not e <= max(GRAD_BAR, e32):
            bad.append(what)
    assert not bad, bad


def test_padded_mask_batch_of_two_image_sizes_trains():
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import train_step
    cfg = _ot_config()
    m, _ = _ot_model(cfg)
    m.train()
    loss_fn = LoFTRLoss(cfg).train()
    base = synth.synth_training_batch(2, seed=78, device='cuda')
    # valid extents at the coarse grid, as tests/test_pipeline_gpu.py: test_train_step_with_padded_masks
    ext0, ext1 = [(52, 80), (60, 64)], [(60, 70), (48, 80)]
    m0 = torch.zeros(2, 60, 80, dtype=torch.bool, device='cuda')
    m1 = torch.zeros(2, 60, 80, dtype=torch.bool, device='cuda')
    batch = dict(base)
    batch['image0'], batch['image1'] = base['image0'].clone(), base['image1'].clone()
    for n in range(2):
        m0[n, :ext0[n][0], :ext0[n][1]] = True
        m1[n, :ext1[n][0], :ext1[n][1]] = True
        batch['image0'][n, :, 8 * ext0[n][0]:, :] = 0; batch['image0'][n, :, :, 8 * ext0[n][1]:] = 0
        batch['image1'][n, :, 8 * ext1[n][0]:, :] = 0; batch['image1'][n, :, :, 8 * ext1[n][1]:] = 0
    keep = m0.flatten(1)[base['spv_b_ids'], base['spv_i_ids']] & m1.flatten(1)[base['spv_b_ids'], base['spv_j_ids']]
    for k in ('spv_b_ids', 'spv_i_ids', 'spv_j_ids'):
        batch[k] = base[k][keep]
    batch['mask0'], batch['mask1'] = m0, m1
    torch.manual_seed(5)
    train_step(m, batch, loss_fn, RunCfg('prior_ransac', 2), H=512, seed=0)
    assert batch['conf_matrix'] is None and batch['conf_pos'].shape == batch['spv_b_ids'].shape
    b, i, j = batch['b_ids'], batch['i_ids'], batch['j_ids']
    assert bool(m0.flatten(1)[b, i].all()) and bool(m1.flatten(1)[b, j].all())
    a0 = torch.tensor([e[0] * e[1] for e in ext0]); a1 = torch.tensor([e[0] * e[1] for e in ext1])
    assert len(b) == int(int(torch.minimum(a0, a1).sum()) * m.coarse_matching.train_coarse_percent)     # compute_max_candidates :46-57
    assert torch.isfinite(batch['loss']).all()
    batch['loss'].backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(m.coarse_matching.bin_score.grad.abs()) > 0
    print(f'[ot padded masks] loss {float(batch["loss"]):.6f}  loss_c {float(batch["loss_scalars"]["loss_c"]):.6f}')


@pytest.mark.parametrize('prefilter', [False, True])
def test_val_step_returns_the_coarse_loss(prefilter):
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import val_step
    from tests.test_val_gpu import _val_batch
    cfg = _ot_config(skh_prefilter=prefilter)
    m, cap = _ot_model(cfg)
    m.eval()
    batch, base = _val_batch(2, seed=31)
    ret = val_step(m, batch, LoFTRLoss(cfg).eval(), RunCfg('prior_ransac', 2), H=512, seed=0)
    lc = float(ret['loss_scalars']['loss_c'])
    print(f'[ot val_step prefilter={prefilter}] loss_c {lc:.6f}  matches {len(batch["b_ids"])}')
    assert np.isfinite(lc) and lc > 0
    assert batch['conf_matrix'] is None and 'conf_matrix_with_bin' not in batch
    assert batch['conf_pos'].shape == batch['spv_b_ids'].shape and not batch['conf_pos'].requires_grad
    assert batch['conf_bin0'].shape == (2, 4800) and batch['conf_bin1'].shape == (2, 4800)
    # against the matcher's own matrix on the same features
    from far_amd import ops
    cm = m.coarse_matching
    cw = ops.coarse_match_sinkhorn(cap['f0'], cap['f1'], cm.bin_score, cm.skh_iters, cm.thr, cm.border_rm, batch['hw0_c'], batch['hw1_c'],
                                   8.0, prefilter=prefilter, want_conf=True)['conf_matrix_with_bin']
    ref = cw[:, :-1, :-1][batch['spv_b_ids'], batch['spv_i_ids'], batch['spv_j_ids']]
    assert float((batch['conf_pos'] - ref).abs().max()) <= 2e-5
    assert torch.equal(batch['conf_bin0'], cw[:, :-1, -1]) and torch.equal(batch['conf_bin1'], cw[:, -1, :-1])
    if prefilter:
        print(f'[ot val_step] positives the prefilter zeroed: {int((batch["conf_pos"] == 0).sum())} of {batch["conf_pos"].numel()}')
        assert torch.equal(batch['conf_pos'], ref)


def test_dual_softmax_train_step_is_unchanged():
    """The regression guard: the dual-softmax training step next to the new path -- gradients bit-identical over two runs, and none
    of the optimal-transport keys in its data."""
    from far_amd.loftr import LoFTR
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import train_step
    cfg = far_train_config()
    m = LoFTR(cfg['loftr'])
    synth.load_synthetic(m, seed=0)
    m = m.cuda().train()
    loss_fn = LoFTRLoss(cfg).train()
    base = synth.synth_training_batch(2, seed=77, device='cuda')
    state = copy.deepcopy(m.state_dict())
    runs = []
    for _ in range(2):
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        batch = dict(base)
        torch.manual_seed(5)
        train_step(m, batch, loss_fn, RunCfg('prior_ransac', 2), H=512, seed=0)
        batch['loss'].backward()
        torch.cuda.synchronize()
        runs.append((batch['loss'].detach().clone(), _grads(m)))
    assert 'conf_bin0' not in batch and 'conf_bin1' not in batch and batch['conf_pos'].shape == base['spv_b_ids'].shape
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_gradients_in_eval_mode_with_the_prefilter_are_refused():
    """The reference's loss reads the FILTERED matrix when the prefilter ran (evaluation mode); ops.sinkhorn_pos_conf differentiates
    the unfiltered one, so that combination raises instead of mixing the two.  Without the prefilter, evaluation mode with
    gradients takes the training branch."""
    from far_amd.loftr.stages import CoarseMatching
    g = torch.Generator(device='cuda').manual_seed(3)
    f0 = (3.0 * torch.randn(1, 12 * 16, 256, device='cuda', generator=g)).requires_grad_(True)
    f1 = (3.0 * torch.randn(1, 12 * 16, 256, device='cuda', generator=g)).requires_grad_(True)
    ids = torch.arange(8, device='cuda')
    data = lambda: {'hw0_c': (12, 16), 'hw1_c': (12, 16), 'hw0_i': (96, 128), 'hw1_i': (96, 128), 'bs': 1,
                    'spv_b_ids': torch.zeros_like(ids), 'spv_i_ids': ids, 'spv_j_ids': ids}
    cfg = _ot_config(skh_prefilter=True)['loftr']['match_coarse']
    with pytest.raises(NotImplementedError, match='skh_prefilter'):
        CoarseMatching(cfg).cuda().eval()(f0, f1, data())
    d = data()
    CoarseMatching(_ot_config()['loftr']['match_coarse']).cuda().eval()(f0, f1, d)
    assert d['conf_pos'].requires_grad and d['conf_matrix'] is None
