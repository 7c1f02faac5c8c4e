"""Training through LoFTR's full softmax attention without a GPU: the C ABI of the training forward and the backward, the opt-in
switch on the modules and the model, and what keeps raising."""
import re

import pytest
import torch

from far_amd import _lib
from far_amd.config import far_eval_config

NEW = ('far_full_attention_train_f16s', 'far_full_attention_bwd_f16s', 'far_full_attention_bwd_workspace_bytes')


def test_new_symbols_are_declared_exported_and_bound():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'far_hip.h')).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype == _lib.SIGNATURES[name][0], name
    assert _lib.EXPECTED_ABI == lib.far_abi_version()        # load() refuses any other library; the build id ties it to these sources


def test_backward_workspace_query_needs_no_gpu():
    ws = _lib.load().far_full_attention_bwd_workspace_bytes
    n = ws(2, 100, 500, 8, 32)
    assert n > 0
    assert n >= 2 * 8 * 100 * 4 + 2 * 8 * 2 * 100 * 32 * 4        # delta, and the partial dq of the split key axis (nsplit = 2)
    assert ws(2, 200, 150, 8, 32) >= 2 * 8 * 200 * 4               # no split: the maxima and delta only
    assert ws(2, 200, 150, 8, 32) < 2 * 8 * 200 * 4 + 4096
    assert ws(4, 100, 500, 8, 32) >= 2 * n - 2048                  # linear in the batch
    assert ws(2, 100, 500, 8, 24) == 0 and ws(0, 100, 500, 8, 32) == 0


# (N, L, S, H, D) -> bytes of the forward's and the backward's workspace: every branch of the split plan (key axis split for the
# forward and dq, query axis split for dk / dv, the ns <= ntile / 4 and ns <= 8 limits, fewer than 8 tiles, the one-wave form of
# the forward alone and of both, 64 workgroups or more per image without a split)
K22_WORKSPACE = {
    (2, 300, 1200, 8, 32): (1305600, 1248256),
    (2, 1200, 300, 8, 32): (0, 2534656),
    (1, 127, 4799, 3, 32): (414720, 391936),
    (1, 40, 4800, 1, 16): (23040, 20992),
    (3, 25, 25, 8, 16): (0, 2816),
    (2, 33, 32, 8, 32): (0, 2560),
    (64, 4800, 4800, 8, 32): (0, 9830912),
}
K23_BWD_WORKSPACE = {(2, 576, 576, 3, 64): 14336, (3, 130, 65, 3, 64): 6144}


def test_workspace_sizes_are_pinned():
    lib = _lib.load()
    for shape, (fwd, bwd) in K22_WORKSPACE.items():
        assert lib.far_full_attention_workspace_bytes(*shape) == fwd, shape
        assert lib.far_full_attention_bwd_workspace_bytes(*shape) == bwd, shape
    for shape, n in K23_BWD_WORKSPACE.items():
        assert lib.far_vit_attention_bwd_workspace_bytes(*shape) == n, shape


def test_switch_defaults_and_setter():
    from far_amd.loftr import LoFTR
    from far_amd.loftr.transformer import FullAttention, LoFTREncoderLayer
    assert LoFTREncoderLayer.full_training is False and FullAttention.full_training is False
    cfg = far_eval_config()
    cfg['coarse']['attention'] = 'full'
    m = LoFTR(cfg)
    keys = list(m.state_dict())
    layers = [l for l in m.modules() if isinstance(l, LoFTREncoderLayer)]
    assert any(l.full for l in layers) and any(not l.full for l in layers)
    assert not any(l.full_training for l in layers)
    assert m.set_full_attention_training() is m
    for l in layers:
        assert l.full_training is l.full
        assert getattr(l.attention, 'full_training', False) is l.full
        assert ('full_training' in l.__dict__) == l.full                      # linear layers are untouched
    assert list(m.state_dict()) == keys
    m.set_full_attention_training(False)
    assert not any(l.full_training or getattr(l.attention, 'full_training', False) for l in layers)
    assert LoFTREncoderLayer.full_training is False and FullAttention.full_training is False


def test_cpu_tensors_and_dropout_keep_raising():
    from far_amd import ops
    from far_amd.loftr.transformer import FullAttention, LoFTREncoderLayer
    x = torch.zeros(1, 4, 256, requires_grad=True)
    with pytest.raises(_lib.FarHipError):
        ops.full_attention_train(x, x, x, 8)
    q = torch.zeros(1, 4, 8, 32)
    att = FullAttention()
    with pytest.raises(NotImplementedError, match='FullAttention'):           # off by default
        att(q.clone().requires_grad_(), q, q)
    att.full_training = True
    with pytest.raises(_lib.FarHipError):                                     # on: CPU tensors still have no path
        att(q.clone().requires_grad_(), q, q)
    drop = FullAttention(use_dropout=True).train()
    drop.full_training = True
    with pytest.raises(NotImplementedError):
        drop(q, q, q)
    with pytest.raises(NotImplementedError):
        drop(q.clone().requires_grad_(), q, q)
    layer = LoFTREncoderLayer(256, 8, 'full').train()
    layer.full_training = layer.attention.full_training = True
    with pytest.raises(_lib.FarHipError):
        layer(x, x)
