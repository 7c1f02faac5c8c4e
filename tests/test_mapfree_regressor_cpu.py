"""The Map-free regressor (far_amd.mapfree.RegressionModel) without a GPU: the fp32 restatement of tests/mapfree_reg_ref.py reproduces
golden G28 (the reference's own classes, tools/make_golden_mapfree_reg.py), the state dict has the reference's names and shapes, every
refusal raises as documented, and construction / load_state_dict need no GPU."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from far_amd import _lib, mapfree
from tests import mapfree_reg_inputs as mi
from tests import mapfree_reg_ref as rr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g28_mapfree_regressor.npz')


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def restated_fp32():
    """The fp32 restatement on G28's inputs, on the CPU, once: taps and (R, t) for use_prior False / True."""
    m = mi.seeded_fill(rr.RefRegressionModel(False))
    im0, im1 = mi.seeded_images()
    out = {}
    with torch.no_grad():
        vol0, vol1 = m.encode(im0), m.encode(im1)
        feats = m.features(vol0, vol1, out=out)
        res = {'vol': mi.tap_volume(torch.cat([vol0, vol1])), 'x3': mi.tap_x3(out['x3'])}
        for prior in (False, True):
            m.use_prior = prior
            R, t = m.gate(feats, *mi.seeded_solver_outputs(prior=prior))
            tag = 'prior' if prior else 'noprior'
            res[f'R_{tag}'], res[f't_{tag}'] = R, t
    return res


@pytest.mark.parametrize('key', ['vol', 'x3', 'R_noprior', 't_noprior', 'R_prior', 't_prior'])
def test_restatement_reproduces_g28(key):
    want = torch.from_numpy(golden()[key])
    got = restated_fp32()[key]
    assert got.shape == want.shape
    d = float((got - want).abs().max())
    bar = 1e-5 * float(want.abs().max())
    print(f'[g28] {key}: restatement-vs-reference {d:.3e}  bar {bar:.3e}')
    assert d <= bar


def test_state_dict_is_the_references_manifest():
    manifest = json.loads(str(golden()['manifest']))
    assert not any(k.startswith('matcher.') for k in manifest)          # the generator's stand-in matcher has no parameters
    m = mapfree.RegressionModel(mi.config(), use_loftr_preds=True, use_vanilla_transformer=True)
    sd = m.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == manifest
    prefixes = {k.split('.')[0] for k in sd}
    assert prefixes == {'encoder', 'head', 'transformer', 'pose_regressor', 'moe_predictor'}
    assert {k.split('.')[1] for k in sd if k.startswith('head.')} == {'resblock1', 'resblock2', 'resblock3'}
    assert {k.split('.')[1] for k in sd if k.startswith(('pose_regressor.', 'moe_predictor.'))} == {'0', '2', '4'}
    assert {k.split('.')[2] for k in sd if k.startswith('transformer.layers.')} == {str(i) for i in range(6)}
    # the restatement carries the same names
    assert {k: list(v.shape) for k, v in rr.RefRegressionModel().state_dict().items()} == manifest


def test_reference_state_dict_strips_the_matcher_only():
    m = mapfree.RegressionModel(mi.config(), use_loftr_preds=True, use_vanilla_transformer=True, use_prior=True)
    sd = dict(mi.seeded_fill(rr.RefRegressionModel()).state_dict())
    ckpt = dict(sd)
    ckpt['matcher.backbone.conv1.weight'] = torch.zeros(3)
    ckpt['matcher.loftr_coarse.layers.0.q_proj.weight'] = torch.zeros(2, 2)
    assert mapfree.reference_state_dict(ckpt).keys() == sd.keys()
    assert mapfree.reference_state_dict({'state_dict': ckpt, 'epoch': 3}).keys() == sd.keys()
    res = m.load_state_dict(mapfree.reference_state_dict(ckpt), strict=True)      # on the CPU
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        m.load_state_dict(ckpt, strict=True)                                       # matcher.* is not the regressor's


def test_construction_needs_no_gpu_and_registers_no_matcher():
    marker = object()
    m = mapfree.RegressionModel(mi.config(), use_loftr_preds=True, use_vanilla_transformer=True, matcher=marker)
    assert m.matcher is marker and 'matcher' not in dict(m.named_children())
    assert all(p.device.type == 'cpu' and not p.requires_grad for p in m.parameters())
    assert not m.training and m.use_prior is False
    assert (m.H, m.H2, m.pose_size, m.num_corr_size) == (256 * 12 * 9, 512, 9, 3)
    assert m.moe_predictor[0].weight.shape == (512, 27669) and m.pose_regressor[0].weight.shape == (512, 27648)
    assert m.head.resblock1.conv1.weight.shape == (64, 67, 3, 3)
    assert isinstance(m.pose_solver, mapfree.EssentialMatrixSolver) and m.pose_solver.ransac_pix_threshold == 2.0


KW = dict(use_loftr_preds=True, use_vanilla_transformer=True)
REFUSED = [
    ({'ENCODER.TYPE': 'ResNet'}, {}, 'encoder'),
    ({'ENCODER.BLOCK_TYPE': 0}, {}, 'BLOCK_TYPE'),
    ({'ENCODER.NUM_BLOCKS': '2-2-2'}, {}, 'NUM_BLOCKS'),
    ({'ENCODER.NOT_CONCAT': True}, {}, 'NOT_CONCAT'),
    ({'ENCODER.NUM_OUT_LAYERS': 128}, {}, 'NUM_OUT_LAYERS'),
    ({'AGGREGATOR.TYPE': 'CorrelationVolumeWarpingQKV'}, {}, 'aggregator'),
    ({'AGGREGATOR.DUSTBIN': True}, {}, 'DUSTBIN'),
    ({'AGGREGATOR.NORMALISE_DOT': True}, {}, 'NORMALISE_DOT'),
    ({'AGGREGATOR.POSITION_ENCODER_IM1': True}, {}, 'POSITION_ENCODER_IM1'),
    ({'AGGREGATOR.CV_OUTLAYERS': 8}, {}, 'CV_OUTLAYERS'),
    ({'AGGREGATOR.MAX_SCORE_CHANNEL': False}, {}, 'MAX_SCORE_CHANNEL'),
    ({'HEAD.TYPE': 'ProcrustesResBlockMLP'}, {}, 'head'),
    ({'HEAD.BATCH_NORM': False}, {}, 'BATCH_NORM'),
    ({}, {'use_superglue_preds': True}, 'use_superglue_preds'),
    ({}, {'use_vanilla_transformer': False}, 'use_vanilla_transformer'),
    ({'TRAINING.LAMBDA': 0.}, {}, 'LAMBDA'),
]


@pytest.mark.parametrize('over, kw, word', REFUSED, ids=[r[2] for r in REFUSED])
def test_refusals_name_what_is_missing(over, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        mapfree.RegressionModel(mi.config(**over), **{**KW, **kw})


def _cpu_data(batch=1, size=(32, 32)):
    return {'image0_reg': torch.zeros(batch, 3, *size), 'image1_reg': torch.zeros(batch, 3, *size),
            'loftr_rt': torch.eye(3, 4).expand(batch, 3, 4).contiguous(), 'inliers': torch.ones(batch, 1)}


def test_training_is_refused():
    m = mapfree.RegressionModel(mi.config(), **KW)
    data = _cpu_data()
    with pytest.raises(NotImplementedError, match='training is not built'):
        m.train()(data)
    m.eval()
    m.pose_regressor[4].weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='training is not built'):
        m.encode(data['image0_reg'])
    m.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='training is not built'):
        m.encode(data['image0_reg'].clone().requires_grad_(True))
    vol = torch.zeros(1, 32, 92, 68, requires_grad=True)
    with pytest.raises(NotImplementedError, match='training is not built'):
        m.regress(vol, vol, data['loftr_rt'], data['inliers'])


def test_cpu_tensors_raise_far_hip_error():
    m = mapfree.RegressionModel(mi.config(), **KW)
    data = _cpu_data()
    with pytest.raises(_lib.FarHipError, match='GPU'):
        m(data)
    with pytest.raises(_lib.FarHipError, match='GPU'):
        m.encode(data['image0_reg'])
    vol = torch.zeros(1, 32, 92, 68)
    with pytest.raises(_lib.FarHipError, match='GPU'):
        m.regress(vol, vol, data['loftr_rt'], data['inliers'])
    with torch.no_grad(), pytest.raises(_lib.FarHipError, match='GPU'):
        m.train()(data)                                       # without gradients .train() is no training: the CPU tensors decide


def test_argument_errors():
    m = mapfree.RegressionModel(mi.config(), **KW)
    data = _cpu_data()
    del data['loftr_rt']
    with pytest.raises(ValueError, match='matcher'):
        m(data)                                               # neither cached solver outputs nor a matcher
