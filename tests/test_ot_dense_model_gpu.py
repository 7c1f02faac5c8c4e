"""Training an optimal-transport model with DENSE coarse supervision (match_type 'sinkhorn', sparse_spvs = False: the loftr_ot_dense
configurations) end to end on the GPU, in the manner of tests/test_sinkhorn_train_model_gpu.py but on 96 x 128 images (coarse grid
12 x 16): pipeline.train_step + LoFTRLoss(cfg, ot_dense=True) + AdamW, the coarse term against the materialised definition on the same
coarse features, padded masks, validation with and without the prefilter -- and the sparse-supervision step next to it, unchanged."""
import copy

import numpy as np
import pytest
import torch

from far_amd import synth
from far_amd.config import RunCfg, far_train_config
from tests.test_sinkhorn_train_model_gpu import _grads, _ot_model

pytestmark = pytest.mark.gpu

H, W, HC, WC = 96, 128, 12, 16
DISP = (8, 16, 24)               # one disparity per band of 32 rows, multiples of the coarse cell
GRAD_BAR = 1e-3                  # tests/test_sinkhorn_train_gpu.py
K_SMALL = np.array([[103.594, 0, 64.], [0, 103.594, 48.], [0, 0, 1.]])          # synth.MP3D_K scaled to 128 x 96


def _config(sparse_spvs=False, **kw):
    cfg = far_train_config()
    # 2 pairs x 192 cells: the reference's sampling sizes (20 % of the candidates, at least 200 padded) do not fit a 12 x 16 grid
    cfg['loftr']['match_coarse'].update(match_type='sinkhorn', sparse_spvs=sparse_spvs, train_coarse_percent=0.4, train_pad_num_gt_min=8, **kw)
    cfg['loftr']['loss']['neg_weight'] = 300.0            # the dense negative part carries a visible share of the gradient
    cfg['loftr']['regress_rt'] = False                    # the pose head's position embedding is tied to the 60 x 80 grid
    return cfg


def _batch(B, seed, device='cuda'):
    """synth.synth_training_batch at 96 x 128: the banded pairs with their supervision in spvs_coarse's form."""
    im0, im1 = synth.synth_image_pair(B, seed=seed, hw=(H, W), disparities=DISP)
    ys, xs = np.meshgrid(np.arange(HC), np.arange(WC), indexing='ij')
    d_c = (np.array(DISP)[np.minimum(ys // (HC // len(DISP)), len(DISP) - 1)] // 8)
    ok = xs - d_c >= 0
    ii = (ys * WC + xs)[ok].astype(np.int64)
    jj = (ys * WC + xs - d_c)[ok].astype(np.int64)
    grid = (np.stack([xs, ys], -1).reshape(1, HC * WC, 2) * 8).astype(np.float32)
    w_pt0 = grid - np.stack([8 * d_c, 0 * d_c], -1).reshape(1, HC * WC, 2).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = -1.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    K = t(np.stack([K_SMALL] * B))
    return {'image0': t(im0), 'image1': t(im1), 'K0': K, 'K1': K.clone(), 'dataset_name': ['mp3d'], 'T_0to1': t(T)[None].repeat(B, 1, 1),
            'spv_b_ids': torch.arange(B, device=device).repeat_interleave(len(ii)), 'spv_i_ids': t(ii).repeat(B),
            'spv_j_ids': t(jj).repeat(B), 'spv_w_pt0_i': t(w_pt0).repeat(B, 1, 1), 'spv_pt1_i': t(grid).repeat(B, 1, 1)}


def _dense_torch(f0, f1, bin_score, iters, data, lc, masks=None, conf=None):
    """The materialised form: definition -> conf = P[:, :L, :S] -> losses.coarse_focal_loss_dense_torch."""
    from far_amd import losses
    from tests.test_sinkhorn_train_gpu import definition
    if conf is None:
        conf = definition(f0, f1, bin_score, iters, *(masks or (None, None)))[:, :-1, :-1]
    weight = None if masks is None else (masks[0][:, :, None] & masks[1][:, None, :]).to(conf.dtype)
    ids = (data['spv_b_ids'], data['spv_i_ids'], data['spv_j_ids'])
    return losses.coarse_focal_loss_dense_torch(conf, ids, losses.has_no_ground_truth(data), lc['focal_alpha'], lc['focal_gamma'],
                                                lc['pos_weight'], lc['neg_weight'], weight)


def test_train_step_two_pairs_and_optimizer_step():
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import train_step
    cfg = _config()
    m, _ = _ot_model(cfg)
    m.train()
    loss_fn = LoFTRLoss(cfg, ot_dense=True).train()
    base = _batch(2, seed=77)
    state = copy.deepcopy(m.state_dict())
    runs = []
    for _ in range(2):
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        batch = dict(base)
        torch.manual_seed(5)
        train_step(m, batch, loss_fn, RunCfg('prior_ransac', 2), H=256, seed=0)
        batch['loss'].backward()
        torch.cuda.synchronize()
        runs.append((batch['loss'].detach().clone(), _grads(m)))
    assert batch['conf_matrix'] is None
    for k in ('conf_matrix_with_bin', 'conf_pos', 'conf_bin0', 'conf_bin1'):
        assert k not in batch, k
    h = batch['conf_dense']
    assert h['match_type'] == 'sinkhorn' and h['feat_c0'].requires_grad and h['bin_score'] is m.coarse_matching.bin_score
    assert h['feat_c0'].shape == (2, HC * WC, 256) and h['skh_iters'] == m.coarse_matching.skh_iters and h['mask0'] is None
    assert torch.isfinite(batch['loss']).all() and set(batch['loss_scalars']) >= {'loss', 'loss_c', 'loss_f'}
    print(f'[ot dense train_step] loss {float(batch["loss"]):.6f}  loss_c {float(batch["loss_scalars"]["loss_c"]):.6f}  '
          f'd bin_score {float(m.coarse_matching.bin_score.grad):.4e}')
    g = runs[1][1]
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(g['coarse_matching.bin_score'].abs()) > 0
    for k in g:
        if k.startswith('loftr_coarse.') or k.startswith('backbone.layer3'):
            assert float(g[k].abs().max()) > 0, k
    assert torch.equal(runs[0][0], runs[1][0])                     # two runs from the same state: the same bits
    for k in g:
        assert torch.equal(runs[0][1][k], g[k]), k
    before = float(m.coarse_matching.bin_score.detach())
    torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.0).step()
    assert float(m.coarse_matching.bin_score.detach()) != before


def test_coarse_term_and_gradients_match_the_materialised_definition():
    """The coarse term of the model's training forward against the materialised definition on the same coarse features: float64 is
    the reference for the term and its gradients w.r.t. the coarse features and bin_score, the fp32 composition gives e32 / dev32
    (loss <= max(2e-5, e32), gradients <= max(1e-3, dev32)).  The parameter gradients: the kernels' coarse term and the fp32
    materialised one, each propagated through the SAME model graph -- a linear map of the feature gradients, held to the same bar."""
    from far_amd import losses
    cfg = _config()
    m, cap = _ot_model(cfg)
    m.train()
    base = _batch(2, seed=78)
    data = {k: base[k] for k in ('image0', 'image1', 'spv_b_ids', 'spv_i_ids', 'spv_j_ids')}
    torch.manual_seed(5)
    m(data, train=True)
    lc = cfg['loftr']['loss']
    cm = m.coarse_matching
    loss = losses.coarse_focal_loss_dense(data, lc['focal_alpha'], lc['focal_gamma'], lc['pos_weight'], lc['neg_weight'])
    keys = ['backbone.layer3_outconv.weight', 'loftr_coarse.layers.0.q_proj.weight', 'loftr_coarse.layers.5.mlp.2.weight',
            'loftr_coarse.layers.3.norm1.bias', 'backbone.conv1.weight', 'coarse_matching.bin_score']
    P = dict(m.named_parameters())
    leaves = [cap['f0'], cap['f1']] + [P[k] for k in keys]
    g_k = torch.autograd.grad(loss, leaves, retain_graph=True)
    l32 = _dense_torch(cap['f0'], cap['f1'], cm.bin_score, cm.skh_iters, data, lc)
    g_32 = torch.autograd.grad(l32, leaves, retain_graph=False)
    f0 = cap['f0'].detach().double().requires_grad_(True)
    f1 = cap['f1'].detach().double().requires_grad_(True)
    a = cm.bin_score.detach().double().requires_grad_(True)
    l64 = _dense_torch(f0, f1, a, cm.skh_iters, data, lc)
    l64.backward()
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    e_loss, e32 = abs(float(loss) - float(l64)) / abs(float(l64)), abs(float(l32) - float(l64)) / abs(float(l64))
    print(f'[ot dense coarse term] loss {float(loss):.8f} vs float64 {float(l64):.8f}: relative {e_loss:.2e} (fp32 composition {e32:.2e})')
    assert e_loss <= max(2e-5, e32)
    bad, dev32 = [], 0.0
    for what, got, r32, ref in (('d feat_c0', g_k[0], g_32[0], f0.grad), ('d feat_c1', g_k[1], g_32[1], f1.grad),
                                ('d bin_score', g_k[-1], g_32[-1], a.grad)):
        e, d32 = rel(got, ref), rel(r32, ref)
        dev32 = max(dev32, d32)
        print(f'[ot dense coarse term] {what}: relative error {e:.3e}   bar {max(GRAD_BAR, d32):.1e} (fp32 composition {d32:.3e})   '
              f'|reference| {float(ref.norm()):.3e}')
        if not e <= max(GRAD_BAR, d32):
            bad.append(what)
    for k, got, r32 in zip(keys[:-1], g_k[2:-1], g_32[2:-1]):
        e = rel(got, r32)
        print(f'[ot dense coarse term] {k}: |grad| {float(r32.norm()):.3e}, relative difference to the materialised fp32 run {e:.3e}')
        if not e <= max(GRAD_BAR, dev32):
            bad.append(k)
    assert not bad, bad


def test_padded_mask_batch_of_two_image_sizes_trains():
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import train_step
    cfg = _config()
    m, _ = _ot_model(cfg)
    m.train()
    loss_fn = LoFTRLoss(cfg, ot_dense=True).train()
    base = _batch(2, seed=78)
    ext0, ext1 = [(10, 16), (12, 13)], [(12, 14), (10, 16)]       # valid extents at the coarse grid
    m0 = torch.zeros(2, HC, WC, dtype=torch.bool, device='cuda')
    m1 = torch.zeros(2, HC, WC, dtype=torch.bool, device='cuda')
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
    train_step(m, batch, loss_fn, RunCfg('prior_ransac', 2), H=256, seed=0)
    h = batch['conf_dense']
    assert batch['conf_matrix'] is None and h['mask0'].dtype == torch.uint8 and h['mask0'].shape == (2, HC * WC)
    b, i, j = batch['b_ids'], batch['i_ids'], batch['j_ids']
    assert bool(m0.flatten(1)[b, i].all()) and bool(m1.flatten(1)[b, j].all())
    assert torch.isfinite(batch['loss']).all()
    batch['loss'].backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(m.coarse_matching.bin_score.grad.abs()) > 0
    print(f'[ot dense padded masks] loss {float(batch["loss"]):.6f}  loss_c {float(batch["loss_scalars"]["loss_c"]):.6f}')


def _val_batch(B, seed):
    """The pairs of _batch with the scene that explains them (fronto-parallel planes at depth f / d per band, two cameras one unit
    apart along x), so that the depth-based supervision applies: tests/test_val_gpu.py: _val_batch at 96 x 128."""
    base = _batch(B, seed)
    depth = np.empty((H, W), np.float32)
    for k, d in enumerate(DISP):
        depth[(H // len(DISP)) * k:(H // len(DISP)) * (k + 1)] = K_SMALL[0, 0] / d
    dep = torch.from_numpy(depth).cuda()[None].repeat(B, 1, 1)
    batch = {k: base[k] for k in ('image0', 'image1', 'dataset_name', 'T_0to1')}
    batch.update(depth0=dep, depth1=dep.clone(), T_1to0=torch.linalg.inv(base['T_0to1']), K0=base['K0'].float(), K1=base['K1'].float(),
                 pair_names=[tuple(f's/a{b}' for b in range(B)), tuple(f's/b{b}' for b in range(B))])
    return batch


@pytest.mark.parametrize('prefilter', [False, True])
def test_val_step_returns_the_coarse_loss(prefilter):
    from far_amd import ops
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import val_step
    cfg = _config(skh_prefilter=prefilter)
    m, cap = _ot_model(cfg)
    m.eval()
    batch = _val_batch(2, seed=31)
    ret = val_step(m, batch, LoFTRLoss(cfg, ot_dense=True).eval(), RunCfg('prior_ransac', 2), H=256, seed=0)
    got = float(ret['loss_scalars']['loss_c'])
    cm, lc = m.coarse_matching, cfg['loftr']['loss']
    assert 'conf_pos' not in batch and 'conf_matrix_with_bin' not in batch
    with torch.no_grad():
        if prefilter:          # the loss saw the matcher's materialised FILTERED matrix
            assert 'conf_dense' not in batch and batch['conf_matrix'].shape == (2, HC * WC, HC * WC)
            cw = ops.coarse_match_sinkhorn(cap['f0'], cap['f1'], cm.bin_score, cm.skh_iters, cm.thr, cm.border_rm, batch['hw0_c'],
                                           batch['hw1_c'], 8.0, prefilter=True, want_conf=True)['conf_matrix']
            assert torch.equal(batch['conf_matrix'], cw)
            ref = float(_dense_torch(None, None, None, None, batch, lc, conf=cw.double()))
            bar = 1e-6         # the same torch expression on the same fp32 matrix, evaluated in float64
        else:                  # the forward kernels on the handle
            h = batch['conf_dense']
            assert batch['conf_matrix'] is None and not h['feat_c0'].requires_grad and not h['bin_score'].requires_grad
            ref = float(_dense_torch(cap['f0'].double(), cap['f1'].double(), cm.bin_score.double(), cm.skh_iters, batch, lc))
            r32 = float(_dense_torch(cap['f0'], cap['f1'], cm.bin_score, cm.skh_iters, batch, lc))
            bar = max(2e-5, abs(r32 - ref) / abs(ref))
    print(f'[ot dense val_step prefilter={prefilter}] loss_c {got:.8f} vs torch float64 {ref:.8f}: relative {abs(got - ref) / abs(ref):.2e} '
          f'(bar {bar:.1e})  matches {len(batch["b_ids"])}')
    assert np.isfinite(got) and got > 0
    assert abs(got - ref) <= bar * abs(ref)


def test_sparse_supervision_step_is_unchanged():
    """A sparse_spvs = True optimal-transport step next to the new path: the keys of the sparse path and no handle, its entries the
    bits of a direct ops.sinkhorn_pos_conf call on the same features, gradients bit-identical over two runs."""
    from far_amd import ops
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import train_step
    cfg = _config(sparse_spvs=True)
    m, cap = _ot_model(cfg)
    m.train()
    loss_fn = LoFTRLoss(cfg).train()
    base = _batch(2, seed=77)
    state = copy.deepcopy(m.state_dict())
    runs = []
    for _ in range(2):
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        batch = dict(base)
        torch.manual_seed(5)
        train_step(m, batch, loss_fn, RunCfg('prior_ransac', 2), H=256, seed=0)
        batch['loss'].backward()
        torch.cuda.synchronize()
        runs.append((batch['loss'].detach().clone(), _grads(m)))
    assert 'conf_dense' not in batch and batch['conf_matrix'] is None and 'conf_matrix_with_bin' not in batch
    assert batch['conf_pos'].shape == base['spv_b_ids'].shape and batch['conf_pos'].requires_grad
    assert batch['conf_bin0'].shape == (2, HC * WC) and batch['conf_bin1'].shape == (2, HC * WC)
    with torch.no_grad():
        cm = m.coarse_matching
        direct = ops.sinkhorn_pos_conf(cap['f0'], cap['f1'], cm.bin_score, cm.skh_iters, base['spv_b_ids'], base['spv_i_ids'], base['spv_j_ids'])
    for a, b in zip(direct, (batch['conf_pos'], batch['conf_bin0'], batch['conf_bin1'])):
        assert torch.equal(a, b.detach())
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_gradients_in_eval_mode_with_the_prefilter_are_still_refused():
    from far_amd.loftr.stages import CoarseMatching
    g = torch.Generator(device='cuda').manual_seed(3)
    f0 = (3.0 * torch.randn(1, HC * WC, 256, device='cuda', generator=g)).requires_grad_(True)
    f1 = (3.0 * torch.randn(1, HC * WC, 256, device='cuda', generator=g)).requires_grad_(True)
    ids = torch.arange(8, device='cuda')
    data = lambda: {'hw0_c': (HC, WC), 'hw1_c': (HC, WC), 'hw0_i': (H, W), 'hw1_i': (H, W), 'bs': 1,
                    'spv_b_ids': torch.zeros_like(ids), 'spv_i_ids': ids, 'spv_j_ids': ids}
    with pytest.raises(NotImplementedError, match='skh_prefilter'):
        CoarseMatching(_config(skh_prefilter=True)['loftr']['match_coarse']).cuda().eval()(f0, f1, data())
    cm = CoarseMatching(_config()['loftr']['match_coarse']).cuda().eval()
    cm.materialize_conf = True
    with pytest.raises(NotImplementedError, match='materialize_conf'):
        cm(f0, f1, data())
    cm.materialize_conf = False
    d = data()
    cm(f0, f1, d)                                                 # evaluation mode with gradients, no prefilter: the training branch
    assert d['conf_matrix'] is None and d['conf_dense']['feat_c0'] is f0 and 'conf_pos' not in d
