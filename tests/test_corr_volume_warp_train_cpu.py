"""K12 training without a GPU: the new entry points are exported and bound (ABI 8), their size queries answer, the float64 yardstick
(tests/cvw_train_ref.py) reproduces golden G29 (the reference's own CorrelationVolumeWarping, tools/make_golden_cvw_train.py), the
module refuses what K12 does not implement, CPU tensors raise, and RegressionModel still refuses to train."""
import os

import numpy as np
import pytest
import torch

from far_amd import _lib, mapfree, ops
from tests import cvw_train_ref as cr
from tests import mapfree_reg_inputs as mi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g29_cvw_train.npz')
NEW = ('far_corr_volume_warp_train_saved_bytes', 'far_corr_volume_warp_bwd_workspace_bytes', 'far_corr_volume_warp_train_f32',
       'far_corr_volume_warp_bwd_f32')


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    assert lib.far_abi_version() == 8 and _lib.EXPECTED_ABI == 8
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'far_hip.h')).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and name + '(' in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for name in ('corr_volume_warp_train', 'corr_volume_warp_bwd', 'corr_volume_warp'):
        assert callable(getattr(ops, name))
    assert issubclass(mapfree.CorrelationVolumeWarping, torch.nn.Module)


def test_size_queries_need_no_gpu():
    lib = _lib.load()
    for fn in (lib.far_corr_volume_warp_train_saved_bytes, lib.far_corr_volume_warp_bwd_workspace_bytes):
        sizes = [fn(B, HW) for B, HW in ((1, 35), (2, 35), (2, 391), (32, 6256))]
        assert sizes[0] > 0 and sizes == sorted(set(sizes))
        assert fn(0, 35) == 0 and fn(1, 0) == 0
    assert lib.far_corr_volume_warp_train_saved_bytes(32, 6256) >= 32 * 6256 * 12       # maximum, sum, arg-max per row
    assert lib.far_corr_volume_warp_bwd_workspace_bytes(32, 6256) < 32 * 6256 * 6256     # nothing of size HW^2


@pytest.mark.parametrize('tag', ['64', '32'])
def test_yardstick_reproduces_g29(tag):
    g = np.load(GOLDEN)
    assert set(g.files) == {'vol0', 'vol1', 'dagg', 'agg32', 'dvol0_32', 'dvol1_32', 'agg64', 'dvol0_64', 'dvol1_64'}
    assert g['vol0'].shape == (2, 32, 7, 5) and g['dagg'].shape == (2, 67, 7, 5)
    assert cr.min_gap(torch.from_numpy(g['vol0']), torch.from_numpy(g['vol1'])) >= cr.MIN_GAP
    dtype = torch.float64 if tag == '64' else torch.float32
    got = cr.grads(g['vol0'], g['vol1'], g['dagg'], dtype)
    for name, x in zip(('agg', 'dvol0_', 'dvol1_'), got):
        want = g[name + tag]
        assert x.dtype == dtype and want.dtype == (np.float64 if tag == '64' else np.float32)
        d = float(np.abs(x.numpy() - want).max())
        print(f'[g29] {name.rstrip("_")} ({tag}): restatement-vs-reference {d:.3e}  max |ref| {np.abs(want).max():.3e}')
        if tag == '64':
            assert d <= 1e-12 * float(np.abs(want).max())
        else:
            np.testing.assert_allclose(x.numpy(), want, rtol=2e-5, atol=2e-6)


REFUSED = [('POSITION_ENCODER_IM1', True), ('NORMALISE_DOT', True), ('RESIDUAL_ATT', True), ('CV_OUTLAYERS', 8), ('CV_HALF_CHANNELS', True),
           ('UPSAMPLE_POS_ENC', 4), ('DUSTBIN', True), ('POSITION_ENCODER', False), ('MAX_SCORE_CHANNEL', False)]


@pytest.mark.parametrize('option, value', REFUSED, ids=[r[0] for r in REFUSED])
def test_module_refuses_unsupported_options_by_name(option, value):
    cfg = mi.config(**{'AGGREGATOR.' + option: value})
    with pytest.raises(NotImplementedError, match=rf"\b{option} {'on' if value else 'off'}\b") as e:
        mapfree.CorrelationVolumeWarping(cfg.AGGREGATOR, 32)
    assert 'K12 (far_corr_volume_warp_f32) is CorrelationVolumeWarping with POSITION_ENCODER and MAX_SCORE_CHANNEL and nothing else' in str(e.value)
    with pytest.raises(NotImplementedError) as r:                       # one helper: the model refuses in the same words
        mapfree.RegressionModel(cfg, use_loftr_preds=True, use_vanilla_transformer=True)
    assert str(r.value).split(':', 1)[1] == str(e.value).split(':', 1)[1]


def test_module_shape_and_channels():
    m = mapfree.CorrelationVolumeWarping(mi.config().AGGREGATOR, 32)
    assert m.num_out_layers == 67 and len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
    for ch in (16, 64):
        with pytest.raises(NotImplementedError, match='32 volume channels'):
            mapfree.CorrelationVolumeWarping(mi.config().AGGREGATOR, ch)


def test_cpu_tensors_raise_far_hip_error():
    vol = torch.zeros(1, 32, 7, 5)
    with pytest.raises(_lib.FarHipError, match='GPU'):
        ops.corr_volume_warp_train(vol.clone().requires_grad_(True), vol)
    with pytest.raises(_lib.FarHipError, match='GPU'):
        ops.corr_volume_warp_train(vol, vol)
    with pytest.raises(_lib.FarHipError, match='GPU'):
        ops.corr_volume_warp_bwd(vol, vol, torch.zeros(1, 67, 7, 5), torch.zeros(35 * 12, dtype=torch.uint8), torch.zeros(1, 67, 7, 5))
    with pytest.raises(_lib.FarHipError, match='GPU'):
        mapfree.CorrelationVolumeWarping(mi.config().AGGREGATOR, 32)(vol.clone().requires_grad_(True), vol)


def test_regression_model_still_refuses_training():
    m = mapfree.RegressionModel(mi.config(), use_loftr_preds=True, use_vanilla_transformer=True)
    data = {'image0_reg': torch.zeros(1, 3, 32, 32), 'image1_reg': torch.zeros(1, 3, 32, 32),
            'loftr_rt': torch.eye(3, 4).expand(1, 3, 4).contiguous(), 'inliers': torch.ones(1, 1)}
    with pytest.raises(NotImplementedError, match='training is not built'):
        m.train()(data)
    m.eval()
    m.pose_regressor[4].weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='training is not built'):
        m.encode(data['image0_reg'])
    m.requires_grad_(False)
    vol = torch.zeros(1, 32, 92, 68, requires_grad=True)
    with pytest.raises(NotImplementedError, match=r'no backward kernels for K27 / K28 / K12'):
        m.regress(vol, vol, data['loftr_rt'], data['inliers'])
