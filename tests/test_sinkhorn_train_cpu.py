"""Training through the optimal-transport matcher, the parts that need no GPU: the loss's sinkhorn branch against the reference's
own LoFTRLoss.compute_coarse_loss (golden G22, tools/make_goldens.py: g22_sinkhorn_loss), what LoFTRLoss accepts and refuses, and
the C ABI of the training kernels."""
import os

import numpy as np
import pytest
import torch

from far_amd import _lib, losses
from far_amd.config import far_train_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_sinkhorn_loss.npz')
RTOL = 1e-6            # fp32 against fp32 on identical inputs, the same operations


def _ot_train_config(**loss):
    cfg = far_train_config()
    cfg['loftr']['match_coarse']['match_type'] = 'sinkhorn'
    cfg['loftr']['loss'].update(loss)
    return cfg


@pytest.mark.parametrize('tag', ['plain', 'weight', 'nogt_pair', 'nogt_pair_weight', 'nogt', 'nogt_weight'])
@pytest.mark.parametrize('form', ['conf_matrix_gt', 'spv_ids', 'sparse_entries'])
def test_sinkhorn_loss_equals_the_reference(tag, form):
    """The dense matrix indexed through conf_matrix_gt, through spv ids, and the three groups of entries handed over as the GPU path
    hands them (conf_pos / conf_bin0 / conf_bin1): one value, the reference's."""
    g = np.load(GOLDEN)
    lc = far_train_config()['loftr']['loss']
    conf = torch.from_numpy(g['conf'])
    gt = torch.from_numpy({'nogt_pair': g['gt_pair'], 'nogt': np.zeros_like(g['gt'])}.get(tag.replace('_weight', ''), g['gt'])).float()
    data = {}
    if tag.endswith('weight'):
        data.update(mask0=torch.from_numpy(g['mask0']), mask1=torch.from_numpy(g['mask1']))
    b, i, j = torch.where(gt == 1)
    count = int(b.numel())
    if count == 0:                                # spvs_coarse's dummy entry (supervision.py:122-128)
        b = i = j = torch.zeros(1, dtype=torch.long)
    if form == 'conf_matrix_gt':
        data.update(conf_matrix_with_bin=conf, conf_matrix_gt=gt)
    elif form == 'spv_ids':
        data.update(conf_matrix_with_bin=conf, spv_b_ids=b, spv_i_ids=i, spv_j_ids=j, spv_gt_count=count)
    else:
        data.update(conf_pos=conf[b, i, j], conf_bin0=conf[:, :-1, -1].contiguous(), conf_bin1=conf[:, -1, :-1].contiguous(),
                    spv_b_ids=b, spv_i_ids=i, spv_j_ids=j, spv_gt_count=count)
    got = float(losses.coarse_focal_loss_sinkhorn(data, lc['focal_alpha'], lc['focal_gamma'], lc['pos_weight'], float(g['neg_weight'])))
    ref = float(g['loss_' + tag])
    print(f'[g22 {tag} {form}] {got:.9g} vs reference {ref:.9g}: relative {abs(got - ref) / abs(ref):.2e}')
    assert abs(got - ref) <= RTOL * abs(ref)


def test_loss_module_runs_the_sinkhorn_branch_and_gradients_reach_all_three_groups():
    g = np.load(GOLDEN)
    lf = losses.LoFTRLoss(_ot_train_config(neg_weight=float(g['neg_weight']), rt_weight_tr=0.0, rt_weight_rot=0.0)).train()
    conf = torch.from_numpy(g['conf'])
    b, i, j = torch.where(torch.from_numpy(g['gt']) == 1)
    pos = conf[b, i, j].clone().requires_grad_(True)
    bin0 = conf[:, :-1, -1].clone().requires_grad_(True)
    bin1 = conf[:, -1, :-1].clone().requires_grad_(True)
    data = {'conf_matrix': None, 'conf_pos': pos, 'conf_bin0': bin0, 'conf_bin1': bin1, 'spv_b_ids': b, 'spv_i_ids': i, 'spv_j_ids': j,
            'spv_gt_count': int(b.numel()), 'expec_f': torch.zeros(4, 3) + 0.5, 'expec_f_gt': torch.zeros(4, 2)}
    lf(data)
    assert abs(float(data['loss_scalars']['loss_c']) - float(g['loss_plain'])) <= RTOL * float(g['loss_plain'])
    data['loss'].backward()
    for t in (pos, bin0, bin1):
        assert torch.isfinite(t.grad).all() and float(t.grad.abs().sum()) > 0
    # a row with ground truth is not a negative: no gradient on its dustbin entry
    assert float(bin0.grad[b, i].abs().max()) == 0 and float(bin1.grad[b, j].abs().max()) == 0


@pytest.mark.parametrize('weighted', [False, True])
def test_empty_labels_on_the_sparse_entries_path_give_the_no_ground_truth_value(weighted):
    """M = 0 labels without the dummy entry (what an empty spv_*_ids hands over): the positive term and its gradient vanish, as the
    dummy positive's do in the reference (c_pos_w = 0, :65-70); the value is the golden's no-ground-truth one up to the dummy's
    weight[0, 0, 0] = 0 (which only the weighted case has: there row 0 / column 0 of pair 0 lose one weight, not all)."""
    g = np.load(GOLDEN)
    lc = far_train_config()['loftr']['loss']
    conf = torch.from_numpy(g['conf'])
    e = torch.zeros(0, dtype=torch.long)
    pos = torch.zeros(0, requires_grad=True)
    bin0 = conf[:, :-1, -1].clone().requires_grad_(True)
    data = {'conf_pos': pos, 'conf_bin0': bin0, 'conf_bin1': conf[:, -1, :-1].contiguous(), 'spv_b_ids': e, 'spv_i_ids': e,
            'spv_j_ids': e, 'spv_gt_count': 0}
    if weighted:
        data.update(mask0=torch.from_numpy(g['mask0']), mask1=torch.from_numpy(g['mask1']))
    loss = losses.coarse_focal_loss_sinkhorn(data, lc['focal_alpha'], lc['focal_gamma'], lc['pos_weight'], float(g['neg_weight']))
    ref = float(g['loss_nogt_weight' if weighted else 'loss_nogt'])
    assert torch.isfinite(loss) and abs(float(loss.detach()) - ref) <= RTOL * abs(ref)
    loss.backward()
    assert pos.grad.shape == (0,) and torch.isfinite(bin0.grad).all() and float(bin0.grad.abs().sum()) > 0


def test_loss_constructs_for_ot_training_and_keeps_its_refusals():
    lf = losses.LoFTRLoss(_ot_train_config())
    assert lf.match_type == 'sinkhorn' and lf.c_neg_w == far_train_config()['loftr']['loss']['neg_weight']
    with pytest.raises(NotImplementedError):
        losses.LoFTRLoss(_ot_train_config(coarse_type='cross_entropy'))
    cfg = _ot_train_config()
    cfg['loftr']['match_coarse']['sparse_spvs'] = False
    with pytest.raises(NotImplementedError):
        losses.LoFTRLoss(cfg)
    cfg = far_train_config()
    cfg['loftr']['loss']['coarse_type'] = 'cross_entropy'
    with pytest.raises(NotImplementedError):
        losses.LoFTRLoss(cfg)
    cfg = far_train_config()
    cfg['loftr']['match_coarse']['match_type'] = 'hungarian'
    with pytest.raises(NotImplementedError):
        losses.LoFTRLoss(cfg)


def test_training_abi_is_bound():
    lib = _lib.load()
    assert lib.far_abi_version() == _lib.EXPECTED_ABI == 8             # pure additions
    for name in ('far_sinkhorn_pos_conf_workspace_bytes', 'far_sinkhorn_pos_conf_f16s', 'far_sinkhorn_pos_conf_bwd_f16'):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    n = lib.far_sinkhorn_pos_conf_workspace_bytes(32, 4800, 4800, 256, 3)
    # the four operand planes, and every (u^t, v^t) of the T + 1 = 4 states
    assert n > 4 * 32 * 4864 * 256 * 2 + 2 * 4 * 32 * (4864 + 4864) * 4
    assert lib.far_sinkhorn_pos_conf_workspace_bytes(32, 4800, 4800, 128, 3) == 0
    assert lib.far_sinkhorn_pos_conf_workspace_bytes(0, 4800, 4800, 256, 3) == 0
    assert lib.far_sinkhorn_pos_conf_workspace_bytes(1, 4800, 4800, 256, -1) == 0
    assert lib.far_sinkhorn_pos_conf_workspace_bytes(1, 48, 35, 256, 0) > 0


def test_ops_and_module_refuse_cpu_tensors():
    """No differentiable Sinkhorn form exists off the GPU: the op raises FarHipError as every op does, the module in training mode
    NotImplementedError naming Sinkhorn -- with the sparse labels in data too."""
    from far_amd import ops
    from far_amd.config import far_eval_config
    from far_amd.loftr.stages import CoarseMatching
    f = torch.zeros(1, 4, 256)
    ids = torch.zeros(1, dtype=torch.long)
    with pytest.raises(_lib.FarHipError):
        ops.sinkhorn_pos_conf(f, f, torch.tensor(1.0), 3, ids, ids, ids)
    cfg = far_eval_config()['match_coarse']
    cfg.update(match_type='sinkhorn')
    cm = CoarseMatching(cfg).train()
    data = {'hw0_c': (2, 2), 'hw1_c': (2, 2), 'hw0_i': (16, 16), 'spv_b_ids': ids, 'spv_i_ids': ids, 'spv_j_ids': ids}
    with pytest.raises(NotImplementedError, match='Sinkhorn'):
        cm(f, f, data)
