"""The optimal-transport matcher's module side without a GPU: construction, the bin_score parameter and the state dict, the
cases it refuses, the C ABI it binds."""
import pytest
import torch

from far_amd import _lib
from far_amd.config import far_eval_config


def _ot_config(**kw):
    cfg = far_eval_config()
    cfg['match_coarse'].update(match_type='sinkhorn', **kw)
    return cfg


def test_sinkhorn_matcher_constructs_with_its_parameter():
    from far_amd.loftr.stages import CoarseMatching
    cfg = _ot_config(skh_init_bin_score=1.5, skh_iters=5, skh_prefilter=True)['match_coarse']
    cm = CoarseMatching(cfg)
    assert isinstance(cm.bin_score, torch.nn.Parameter) and cm.bin_score.requires_grad
    assert cm.bin_score.shape == () and float(cm.bin_score.detach()) == 1.5
    assert cm.skh_iters == 5 and cm.skh_prefilter is True
    assert list(cm.state_dict()) == ['bin_score']
    with pytest.raises(NotImplementedError):
        CoarseMatching(dict(cfg, match_type='hungarian'))


def test_state_dicts_and_lightning_prefix():
    from far_amd.loftr import LoFTR
    ds = LoFTR(far_eval_config())
    ot = LoFTR(_ot_config())
    assert len(ds.state_dict()) == 240
    sd = ot.state_dict()
    assert len(sd) == 241 and 'coarse_matching.bin_score' in sd
    assert float(sd['coarse_matching.bin_score']) == far_eval_config()['match_coarse']['skh_init_bin_score']
    # a Lightning checkpoint (keys 'matcher.*') loads strictly
    ckpt = {'matcher.' + k: v.clone() for k, v in sd.items()}
    ckpt['matcher.coarse_matching.bin_score'] = torch.tensor(2.25)
    res = ot.load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(ot.coarse_matching.bin_score.detach()) == 2.25


def test_sinkhorn_refuses_training_and_16bit_operands():
    from far_amd.loftr import LoFTR
    from far_amd.loftr.stages import CoarseMatching
    cm = CoarseMatching(_ot_config()['match_coarse']).train()
    f = torch.zeros(1, 4, 256)
    data = {'hw0_c': (2, 2), 'hw1_c': (2, 2), 'hw0_i': (16, 16)}
    with pytest.raises(NotImplementedError, match='Sinkhorn'):
        cm(f, f, data)
    m = LoFTR(_ot_config())
    for mode in ('fp16', 'mixed16', ('k1',)):
        with pytest.raises(NotImplementedError, match='Sinkhorn'):
            m.set_precision(mode)
    assert m.precision_stages == ()
    m.set_precision('fp16-fine')                     # stages without K1 are unaffected
    assert m.precision_stages == ('fpn',)
    LoFTR(far_eval_config()).set_precision('fp16')   # the dual-softmax model keeps every mode


def test_sinkhorn_abi_is_bound():
    lib = _lib.load()
    assert _lib.EXPECTED_ABI == 8 == lib.far_abi_version()
    assert 'far_coarse_match_sinkhorn_f16s' in _lib.SIGNATURES
    n = lib.far_coarse_match_sinkhorn_f16s_workspace_bytes(32, 4800, 4800, 256)
    assert n >= 4 * 32 * 4864 * 256 * 2                 # the four split-fp16 operand planes
    assert lib.far_coarse_match_sinkhorn_f16s_workspace_bytes(32, 4800, 4800, 128) == 0
