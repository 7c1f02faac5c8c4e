"""Dense supervision of the optimal-transport matcher (match_type 'sinkhorn', sparse_spvs = False), the parts that need no GPU: what
LoFTRLoss accepts and refuses, the loss module on a dense conf_matrix against the reference's own CoarseMatching +
LoFTRLoss.compute_coarse_loss (golden G24, tools/make_goldens.py: g24_ot_dense), and the C ABI of the kernels."""
import os

import numpy as np
import pytest
import torch

from far_amd import _lib, losses
from far_amd.config import far_train_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g24_ot_dense.npz')
RTOL_LOSS = 1e-6
# The golden's gradients are the reference's fp32 autograd through three unrolled Sinkhorn iterations; the float64 run of the same
# composition differs from it by that fp32 chain's own error: measured 3e-6 ... 6e-5 (relative Frobenius) on the GPU tests' inputs
# (tests/test_ot_dense_gpu.py prints it as `fp32 autograd`), here on the 48 x 35 grids 1.5e-5 ... 2.4e-5 (printed).  2e-4 is three times
# the largest of those.
RTOL_GRAD = 2e-4


def _ot_dense_config(**loss):
    cfg = far_train_config()
    cfg['loftr']['match_coarse'].update(match_type='sinkhorn', sparse_spvs=False)
    cfg['loftr']['loss'].update(loss)
    return cfg


def test_loss_constructs_with_the_keyword_and_keeps_its_refusals():
    lf = losses.LoFTRLoss(_ot_dense_config(), ot_dense=True)
    assert lf.match_type == 'sinkhorn' and not lf.sparse_spvs
    with pytest.raises(NotImplementedError, match='ot_dense'):
        losses.LoFTRLoss(_ot_dense_config())
    with pytest.raises(TypeError):
        losses.LoFTRLoss(_ot_dense_config(), True)                      # keyword only
    for kw in ({}, {'ot_dense': True}):
        with pytest.raises(NotImplementedError):
            losses.LoFTRLoss(_ot_dense_config(coarse_type='cross_entropy'), **kw)
    cfg = _ot_dense_config()
    cfg['loftr']['match_coarse']['match_type'] = 'hungarian'
    with pytest.raises(NotImplementedError):
        losses.LoFTRLoss(cfg, ot_dense=True)
    # the keyword changes nothing for the configurations the plain constructor accepts
    assert losses.LoFTRLoss(far_train_config(), ot_dense=True).sparse_spvs


def _float64_run(g, tag):
    """The loss module (LoFTRLoss(cfg, ot_dense=True), its dense branch on data['conf_matrix']) on the conf that the torch definition
    gives in float64 from G24's inputs -> loss, dF0, dF1, d bin_score."""
    from tests.test_sinkhorn_train_gpu import definition
    masked = tag.endswith('weight')
    t0 = torch.from_numpy(g['f0']).double().requires_grad_(True)
    t1 = torch.from_numpy(g['f1']).double().requires_grad_(True)
    a = torch.tensor(float(g['bin_score']), dtype=torch.float64, requires_grad=True)
    m0, m1 = torch.from_numpy(g['mask0']), torch.from_numpy(g['mask1'])
    conf = definition(t0, t1, a, int(g['skh_iters']), *((m0, m1) if masked else (None, None)))[:, :-1, :-1]
    gt = np.zeros_like(g['gt']) if tag.startswith('nogt') else (g['gt_weight'] if masked else g['gt'])
    b, i, j = torch.where(torch.from_numpy(gt) == 1)
    count = int(b.numel())
    if count == 0:
        b = i = j = torch.zeros(1, dtype=torch.long)
    data = {'conf_matrix': conf, 'spv_b_ids': b, 'spv_i_ids': i, 'spv_j_ids': j, 'spv_gt_count': count,
            'expec_f': torch.zeros(4, 3, dtype=torch.float64) + 0.5, 'expec_f_gt': torch.zeros(4, 2, dtype=torch.float64)}
    if masked:
        data.update(mask0=m0.reshape(2, 6, 8), mask1=m1.reshape(2, 5, 7))
    lf = losses.LoFTRLoss(_ot_dense_config(neg_weight=float(g['neg_weight']), rt_weight_tr=0.0, rt_weight_rot=0.0), ot_dense=True).train()
    lf(data)
    loss_c = data['loss_scalars']['loss_c']
    lc = far_train_config()['loftr']['loss']
    direct = losses.coarse_focal_loss_dense(data, lc['focal_alpha'], lc['focal_gamma'], lc['pos_weight'], float(g['neg_weight']))
    assert float(direct.detach()) == float(loss_c)
    direct.backward()
    return float(loss_c), t0.grad.numpy(), t1.grad.numpy(), float(a.grad)


@pytest.mark.parametrize('tag', ['plain', 'weight', 'nogt', 'nogt_weight'])
def test_loss_module_on_a_dense_conf_matrix_equals_the_reference(tag):
    g = np.load(GOLDEN)
    loss, df0, df1, dbin = _float64_run(g, tag)
    ref = float(g['loss_' + tag])
    rel = lambda x, y: float(np.linalg.norm(np.ravel(x) - np.ravel(y)) / np.linalg.norm(np.ravel(y)))
    e = [rel(df0, g['df0_' + tag]), rel(df1, g['df1_' + tag]), abs(dbin - float(g['dbin_' + tag])) / abs(float(g['dbin_' + tag]))]
    print(f'[g24 {tag}] loss {loss:.9g} vs reference {ref:.9g}: relative {abs(loss - ref) / abs(ref):.2e}; the fp32 reference against this '
          f'float64 run: dF0 {e[0]:.2e}  dF1 {e[1]:.2e}  d bin_score {e[2]:.2e}')
    assert abs(loss - ref) <= RTOL_LOSS * abs(ref)
    assert max(e) <= RTOL_GRAD, e


def test_ot_dense_abi_is_bound_and_the_workspace_holds_no_matrix():
    lib = _lib.load()
    assert lib.far_abi_version() == _lib.EXPECTED_ABI == 8             # pure additions
    names = ('far_sinkhorn_dense_focal_workspace_bytes', 'far_sinkhorn_dense_focal_f16s', 'far_sinkhorn_dense_focal_bwd_f16')
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'far_hip.h')).read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name + '(' in header, name
    L = S = 4800
    n = lib.far_sinkhorn_dense_focal_workspace_bytes(1, L, S, 256, 3, 1500)
    assert 0 < n < 4 * L * S, n                                         # less than ONE fp32 L x S matrix
    assert n > 4 * 4864 * 256 * 2 + 2 * 4 * (4864 + 4864) * 4            # the four operand planes, every (u^t, v^t) of the T + 1 states
    assert n > lib.far_sinkhorn_pos_conf_workspace_bytes(1, L, S, 256, 3)
    assert lib.far_sinkhorn_dense_focal_workspace_bytes(1, L, S, 128, 3, 1500) == 0
    assert lib.far_sinkhorn_dense_focal_workspace_bytes(0, L, S, 256, 3, 1500) == 0
    assert lib.far_sinkhorn_dense_focal_workspace_bytes(1, L, S, 256, -1, 1500) == 0
    assert lib.far_sinkhorn_dense_focal_workspace_bytes(1, L, S, 256, 49, 1500) == 0
    assert lib.far_sinkhorn_dense_focal_workspace_bytes(1, 35, 72, 256, 0, 0) > 0


def test_op_and_module_refuse_cpu_tensors():
    from far_amd import ops
    from far_amd.config import far_eval_config
    from far_amd.loftr.stages import CoarseMatching
    f = torch.zeros(1, 4, 256)
    ids = torch.zeros(1, dtype=torch.long)
    with pytest.raises(_lib.FarHipError):
        ops.sinkhorn_dense_focal_loss(f, f, torch.tensor(1.0), 3, ids, ids, ids, 0.25, 2.0, 1.0, 1.0)
    cfg = far_eval_config()['match_coarse']
    cfg.update(match_type='sinkhorn', sparse_spvs=False)
    cm = CoarseMatching(cfg).train()
    data = {'hw0_c': (2, 2), 'hw1_c': (2, 2), 'hw0_i': (16, 16), 'spv_b_ids': ids, 'spv_i_ids': ids, 'spv_j_ids': ids}
    with pytest.raises(NotImplementedError, match='Sinkhorn'):
        cm(f, f, data)
