"""Dense coarse supervision (sparse_spvs = False, dual_softmax, focal), the parts that need no GPU: the torch form of the loss against
the reference's own LoFTRLoss.compute_coarse_loss (golden G23, tools/make_goldens.py: g23_dense_focal), what LoFTRLoss accepts and
refuses, and the C ABI of the kernels."""
import os

import numpy as np
import pytest
import torch

from far_amd import _lib, losses
from far_amd.config import far_train_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g23_dense_focal.npz')
RTOL = 1e-6            # fp32 against fp32 on identical inputs, the same operations (the G22 test's tolerance)


def _dense_config(**loss):
    cfg = far_train_config()
    cfg['loftr']['match_coarse']['sparse_spvs'] = False
    cfg['loftr']['loss'].update(loss)
    return cfg


def _data(g, tag, form, conf):
    gt = torch.from_numpy(np.zeros_like(g['gt']) if tag.startswith('nogt') else g['gt']).float()
    data = {'conf_matrix': conf}
    if tag.endswith('weight'):
        data.update(mask0=torch.from_numpy(g['mask0']), mask1=torch.from_numpy(g['mask1']))
    if form == 'conf_matrix_gt':
        data['conf_matrix_gt'] = gt
    else:
        b, i, j = torch.where(gt == 1)
        count = int(b.numel())
        if count == 0 and form == 'spv_ids':              # spvs_coarse's dummy entry (supervision.py:122-128)
            b = i = j = torch.zeros(1, dtype=torch.long)
        data.update(spv_b_ids=b, spv_i_ids=i, spv_j_ids=j, spv_gt_count=count)
    return data


@pytest.mark.parametrize('tag', ['plain', 'weight', 'nogt', 'nogt_weight'])
@pytest.mark.parametrize('form', ['conf_matrix_gt', 'spv_ids', 'spv_ids_empty'])
def test_dense_focal_loss_and_gradient_equal_the_reference(tag, form):
    """The positives given as conf_matrix_gt, as spv ids (with the dummy entry when there is no ground truth) and as an empty id
    list: one value and one gradient w.r.t. conf, the reference's."""
    g = np.load(GOLDEN)
    lc = far_train_config()['loftr']['loss']
    conf = torch.from_numpy(g['conf']).clone().requires_grad_(True)
    loss = losses.coarse_focal_loss_dense(_data(g, tag, form, conf), lc['focal_alpha'], lc['focal_gamma'], lc['pos_weight'],
                                          float(g['neg_weight']))
    loss.backward()
    loss = loss.detach()
    ref, gref = float(g['loss_' + tag]), torch.from_numpy(g['grad_' + tag])
    dg = float((conf.grad - gref).abs().max()) / float(gref.abs().max())
    print(f'[g23 {tag} {form}] {float(loss):.9g} vs reference {ref:.9g}: relative {abs(float(loss) - ref) / abs(ref):.2e}; '
          f'gradient max|d| / max|ref| = {dg:.2e}')
    assert abs(float(loss) - ref) <= RTOL * abs(ref)
    assert dg <= RTOL
    assert torch.equal(conf.grad == 0, gref == 0)         # the clamp and the zero weights cut the same entries off


def test_loss_module_constructs_for_dense_supervision_and_runs_the_dense_branch():
    g = np.load(GOLDEN)
    lf = losses.LoFTRLoss(_dense_config(neg_weight=float(g['neg_weight']), rt_weight_tr=0.0, rt_weight_rot=0.0)).train()
    assert lf.match_type == 'dual_softmax' and not lf.sparse_spvs
    conf = torch.from_numpy(g['conf']).clone().requires_grad_(True)
    data = _data(g, 'weight', 'spv_ids', conf)
    data.update(expec_f=torch.zeros(4, 3) + 0.5, expec_f_gt=torch.zeros(4, 2))
    lf(data)
    assert abs(float(data['loss_scalars']['loss_c']) - float(g['loss_weight'])) <= RTOL * float(g['loss_weight'])
    data['loss'].backward()
    assert torch.isfinite(conf.grad).all() and float(conf.grad.abs().sum()) > 0


def test_loss_module_keeps_its_refusals():
    with pytest.raises(NotImplementedError):
        losses.LoFTRLoss(_dense_config(coarse_type='cross_entropy'))
    cfg = _dense_config()
    cfg['loftr']['match_coarse']['match_type'] = 'sinkhorn'
    with pytest.raises(NotImplementedError):
        losses.LoFTRLoss(cfg)
    cfg = _dense_config()
    cfg['loftr']['match_coarse']['match_type'] = 'hungarian'
    with pytest.raises(NotImplementedError):
        losses.LoFTRLoss(cfg)
    cfg = far_train_config()
    cfg['loftr']['loss']['coarse_type'] = 'cross_entropy'
    with pytest.raises(NotImplementedError):
        losses.LoFTRLoss(cfg)


def test_dense_abi_is_bound_and_the_workspace_holds_no_matrix():
    lib = _lib.load()
    assert lib.far_abi_version() == _lib.EXPECTED_ABI == 8             # pure additions
    for name in ('far_coarse_dense_focal_workspace_bytes', 'far_coarse_dense_focal_f16s', 'far_coarse_dense_focal_bwd_f16'):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    L = S = 4800
    n = lib.far_coarse_dense_focal_workspace_bytes(1, L, S, 256, 1500)
    assert 0 < n < 4 * L * S, n                                         # less than ONE fp32 L x S matrix
    assert n > 4 * 4864 * 256 * 2                                       # the four operand planes are in it
    assert lib.far_coarse_dense_focal_workspace_bytes(1, L, S, 128, 1500) == 0
    assert lib.far_coarse_dense_focal_workspace_bytes(0, L, S, 256, 1500) == 0
    assert lib.far_coarse_dense_focal_workspace_bytes(1, L, S, 256, -1) == 0
    assert lib.far_coarse_dense_focal_workspace_bytes(1, 35, 72, 256, 0) > 0


# The workspace sizes of the four K1 training families at (Z, L, S), C = 256, as literals: the forward call leaves its planes and
# statistics in the workspace for the backward call, so the carving (k1_train_f16s.h: Carver, pad128) must not drift.
K1_SHAPES = [(1, 35, 72), (2, 48, 48), (1, 130, 70), (3, 192, 192), (32, 4800, 4800)]
K1_M = (0, 1500)
K1_T = (0, 3, 48)
COARSE_TRAIN_WS = [440832, 873216, 658944, 2659072, 610579456]
COARSE_DENSE_WS = [(441856, 459520), (875008, 892672), (659968, 677632), (2661376, 2679040), (610606080, 610623744)]       # [shape][M]
SINKHORN_POS_WS = [(439296, 455680, 732672), (877568, 910336, 1464832), (658432, 683008, 1098240), (2630656, 2728960, 4389888),
                   (532939776, 552864256, 889086976)]                                                                        # [shape][T]
SINKHORN_DENSE_WS = [((442624, 466176), (459008, 482560), (736000, 759552)),                                                 # [shape][T][M]
                     ((882944, 906496), (915712, 939264), (1470208, 1493760)),
                     ((662784, 686336), (687360, 710912), (1102592, 1126144)),
                     ((2644224, 2667776), (2742528, 2766080), (4403456, 4427008)),
                     ((535440896, 535464448), (555365376, 555388928), (891588096, 891611648))]


def test_k1_training_workspace_sizes_are_pinned():
    lib = _lib.load()
    for n, (Z, L, S) in enumerate(K1_SHAPES):
        assert lib.far_coarse_train_workspace_bytes(Z, L, S, 256) == COARSE_TRAIN_WS[n], (Z, L, S)
        for m, M in enumerate(K1_M):
            assert lib.far_coarse_dense_focal_workspace_bytes(Z, L, S, 256, M) == COARSE_DENSE_WS[n][m], (Z, L, S, M)
        for t, T in enumerate(K1_T):
            assert lib.far_sinkhorn_pos_conf_workspace_bytes(Z, L, S, 256, T) == SINKHORN_POS_WS[n][t], (Z, L, S, T)
            for m, M in enumerate(K1_M):
                assert lib.far_sinkhorn_dense_focal_workspace_bytes(Z, L, S, 256, T, M) == SINKHORN_DENSE_WS[n][t][m], (Z, L, S, T, M)
    # the refusals: another width, an empty batch, a negative label count, more iterations than the staged column terms allow
    assert lib.far_coarse_train_workspace_bytes(1, 35, 72, 128) == 0 and lib.far_coarse_train_workspace_bytes(0, 35, 72, 256) == 0
    assert lib.far_coarse_dense_focal_workspace_bytes(1, 35, 72, 128, 0) == 0 and lib.far_coarse_dense_focal_workspace_bytes(0, 35, 72, 256, 0) == 0
    assert lib.far_coarse_dense_focal_workspace_bytes(1, 35, 72, 256, -1) == 0
    assert lib.far_sinkhorn_pos_conf_workspace_bytes(1, 35, 72, 128, 3) == 0 and lib.far_sinkhorn_pos_conf_workspace_bytes(0, 35, 72, 256, 3) == 0
    assert lib.far_sinkhorn_pos_conf_workspace_bytes(1, 35, 72, 256, 49) == 0
    assert lib.far_sinkhorn_dense_focal_workspace_bytes(1, 35, 72, 128, 3, 0) == 0 and lib.far_sinkhorn_dense_focal_workspace_bytes(0, 35, 72, 256, 3, 0) == 0
    assert lib.far_sinkhorn_dense_focal_workspace_bytes(1, 35, 72, 256, 3, -1) == 0
    assert lib.far_sinkhorn_dense_focal_workspace_bytes(1, 35, 72, 256, 49, 0) == 0


def test_op_refuses_cpu_tensors_and_other_widths():
    from far_amd import ops
    ids = torch.zeros(1, dtype=torch.long)
    with pytest.raises(_lib.FarHipError):
        ops.coarse_dense_focal_loss(torch.zeros(1, 4, 256), torch.zeros(1, 4, 256), ids, ids, ids, 0.1, 0.25, 2.0, 1.0, 1.0)
