"""Training the 8-Point-ViT without a GPU: the C ABI of K23's training forward and backward, the workspace query, the opt-in switch
on the modules and the model, what keeps raising on CPU tensors, and pose_loss against the reference's two-line formula."""
import os
import re

import pytest
import torch

from far_amd import _lib
from tests import vit8pt_inputs as vi

NEW = ('far_vit_attention_train_f16s', 'far_vit_attention_bwd_workspace_bytes', 'far_vit_attention_bwd_f16s')


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'far_hip.h')).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype == _lib.SIGNATURES[name][0], name
    assert _lib.EXPECTED_ABI == lib.far_abi_version() == 8                   # a pure addition: the version stays
    # the training forward is the inference entry point's argument list plus `float* lse`
    a, b = _lib.SIGNATURES['far_vit_attention_f16s'][1], _lib.SIGNATURES['far_vit_attention_train_f16s'][1]
    assert len(b) == len(a) + 1 and b[:len(a) - 2] == a[:-2]


def test_backward_workspace_query_needs_no_gpu():
    ws = _lib.load().far_vit_attention_bwd_workspace_bytes
    n = ws(2, 576, 576, 3, 64)
    assert n >= 2 * 3 * 576 * 4 + 2 * 2 * 4                                   # delta (Z, H, L) and the two maxima per image
    assert n < 2 * 3 * 576 * 4 + 2 * 1024                                     # ... and nothing of size (L, S)
    assert ws(2, 1, 1, 3, 64) > 0 and ws(2, 33, 40, 1, 64) > 0
    for Z in (1, 3, 4, 64):
        assert ws(Z, 576, 576, 3, 64) * 2 == n * Z                            # linear in Z
    assert ws(2, 576, 576, 3, 32) == 0 and ws(0, 576, 576, 3, 64) == 0


def test_switch_defaults_and_setter():
    from far_amd.vit8pt import Attention, Block, FusionTransformer, ViTEss
    assert Attention.block_training is False and Block.block_training is False and FusionTransformer.block_training is False
    m = ViTEss(vi.vit_args(transformer_depth=3))
    keys = list(m.state_dict())
    blocks = [b for b in m.fusion_transformer.blocks if isinstance(b, Block)]
    assert len(blocks) == 2
    assert not m.fusion_transformer.block_training and not any(b.block_training or b.attn.block_training for b in blocks)
    assert m.set_block_training() is m
    assert m.fusion_transformer.block_training and all(b.block_training and b.attn.block_training for b in blocks)
    assert list(m.state_dict()) == keys
    assert m.set_block_training(False) is m
    assert not m.fusion_transformer.block_training and not any(b.block_training or b.attn.block_training for b in blocks)
    assert Attention.block_training is False and Block.block_training is False and FusionTransformer.block_training is False


def test_cpu_tensors_raise_on_every_new_front_end():
    from far_amd import ops
    from far_amd.vit8pt import ViTEss
    x = torch.zeros(1, 4, 192, requires_grad=True)
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention_train(x, x, x, 3)
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention_train_qkv(torch.zeros(1, 4, 576, requires_grad=True), 3)
    y = torch.zeros(1, 4, 192)
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention_bwd(y, y, y, y, torch.zeros(1, 3, 4), y, 3)
    m = ViTEss(vi.vit_args(transformer_depth=2)).set_block_training().train()
    with pytest.raises(_lib.FarHipError):                                    # on: CPU tensors still have no path
        m.forward_features(torch.zeros(2, 576, 192), None, torch.zeros(1), torch.eye(4)[None])
    with pytest.raises(_lib.FarHipError):
        m.fusion_transformer.blocks[0](torch.zeros(2, 576, 192))
    m.set_block_training(False)
    with pytest.raises(NotImplementedError, match='set_block_training'):     # off: the refusal names the kernel and the setter
        m.fusion_transformer.blocks[0](torch.zeros(2, 576, 192))
    with pytest.raises(NotImplementedError, match='far_vit_attention_f16s'):
        m.fusion_transformer.blocks[0](torch.zeros(2, 576, 192))


@pytest.mark.parametrize('losson6d', [False, True])
def test_pose_loss_is_the_two_line_formula(losson6d):
    from far_amd.vit8pt import pose_loss
    g = torch.Generator().manual_seed(3)
    B, J = 5, 3
    outs = (torch.randn(B, 3, generator=g), torch.randn(B, J, 3, generator=g), torch.randn(B, 3, 3, generator=g),
            torch.randn(B, 6, generator=g))
    gt_tran = torch.randn(B, 3, generator=g)
    gt_rot = torch.randn(B, 6, generator=g) if losson6d else torch.randn(B, J, 3, generator=g)
    w_tr, w_rot = 0.7, 1.9
    want = w_tr * torch.pow(outs[0] - gt_tran, 2).mean() + w_rot * torch.pow((outs[3] if losson6d else outs[1]) - gt_rot, 2).mean()
    got = pose_loss(outs, gt_tran, gt_rot, w_tr, w_rot, losson6d=losson6d)
    assert got.shape == () and torch.equal(got, want)
    leaf = [t.clone().requires_grad_() for t in outs]
    pose_loss(leaf, gt_tran, gt_rot, w_tr, w_rot, losson6d=losson6d).backward()
    assert leaf[0].grad is not None and (leaf[3] if losson6d else leaf[1]).grad is not None
    assert leaf[2].grad is None and (leaf[1] if losson6d else leaf[3]).grad is None
