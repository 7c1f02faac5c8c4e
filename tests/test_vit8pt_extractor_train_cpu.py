"""CPU checks of training the 8-Point-ViT extractor's final block.

The float64 yardstick of tests/test_vit8pt_extractor_train_gpu.py runs tests/vit8pt_extractor_ref.py's FinalConv in .train(); golden G27
(tools/make_golden_vit8pt_extractor_train.py: the reference's own ResidualBlock(128, 192, 'batch', kernel_size=5) in .train(), fp32
autograd, on the seeded case of tests/vit8pt_extractor_train_ref.py) pins that to the reference at 1e-5 relative, the README's parity
line for float64-against-reference vectors: max|restatement - fixture| <= 1e-5 max|fixture| per tensor.  The three convolution bias
gradients are mathematically zero under batch statistics (the fixture holds the reference's fp32 rounding noise): they are held to
1e-5 of the largest gradient of the BatchNorm bias behind them.  The switch itself (ViTEss.set_extractor_training) needs no GPU either,
nor do the sizes K24 asks its callers for."""
import os

import numpy as np
import pytest
import torch

from tests import vit8pt_extractor_ref as er
from tests import vit8pt_extractor_train_ref as etr
from tests import vit8pt_inputs as vi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g27_vit8pt_final_block_train.npz')
REL = 1e-5
NORM_BEHIND = {'conv1': 'norm1', 'conv2': 'norm2', 'downsample.0': 'norm3'}


def test_final_block_in_train_mode_is_the_reference_arithmetic():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    blk = er.FinalConv()
    x, gy = etr.block_case(etr.block_fill(blk))
    got = etr.block_run(blk.double(), x, gy)
    assert int(blk.norm1.num_batches_tracked) == int(blk.norm2.num_batches_tracked) == int(blk.norm3.num_batches_tracked) == 1
    assert set(got) == set(g.files) - {'seed', 'note'} and int(g['seed']) == etr.SEED
    assert 0.2 < float((got['y'] > 0).double().mean()) < 0.8
    for k in sorted(got):
        want = torch.from_numpy(g[k]).double()
        assert want.shape == got[k].shape, k
        conv = k[2:-5] if k.startswith('d_') and k.endswith('.bias') and k[2:-5] in NORM_BEHIND else None
        scale = float(want.abs().max()) if conv is None else float(np.abs(g[f'd_{NORM_BEHIND[conv]}.bias']).max())
        d = float((got[k] - want).abs().max())
        print(f'[g27] {k}: max|restatement - reference| {d:.3e}  bar {REL * scale:.3e}')
        assert scale > 0 and d <= REL * scale, k
    for c in NORM_BEHIND:                                                    # ~ 0 in float64: fourteen orders below the other gradients
        assert float(got[f'd_{c}.bias'].abs().max()) <= 1e-10


def test_the_setter_and_the_refusals():
    from far_amd.vit8pt import ViTEss
    m = ViTEss(vi.vit_args(), extractor=True)
    keys = list(m.state_dict())
    final = [p for p in m.extractor_final_conv.parameters()]
    assert not any(p.requires_grad for p in final)
    assert m.set_extractor_training() is m and m.extractor_training is True
    assert all(p.requires_grad for p in final) and not any(p.requires_grad for p in m.resnet.parameters())
    assert list(m.state_dict()) == keys
    for part in ('all', 'resnet', 'front'):
        with pytest.raises(NotImplementedError, match='K25'):
            m.set_extractor_training(part)
    images = torch.zeros(1, 2, 3, 8, 8)
    m.eval()
    with pytest.raises(NotImplementedError, match='set_extractor_training'):     # gradients wanted with the block in .eval()
        m.extract_features(images)
    m.train()
    m.resnet.conv1.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='set_extractor_training'):     # the front does not train
        m.extract_features(images)
    m.resnet.conv1.weight.requires_grad_(False)
    assert m.set_extractor_training(on=False) is m and m.extractor_training is False
    assert not any(p.requires_grad for p in final)
    m.extractor_final_conv.norm2.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='set_extractor_training'):     # a final-block parameter, the switch off
        m.extract_features(images)
    with pytest.raises(NotImplementedError, match='forward_features'):            # a model without the extractor: as forward(images)
        ViTEss(vi.vit_args()).set_extractor_training()


def test_k24_image_and_wgrad_workspace_sizes_are_pinned():
    """The packed image is 25 taps x Cin x Cout x (hi + lo) fp16 in either direction; the weight gradient's workspace is 256 bytes (the
    gradient scale) + one fp32 slab [25][Cout][Cin] per pixel range of its plan.  Literals, as the library gave them before the forward
    and the dgrad came to share conv_valid_f16s.h: the slab plan must not drift."""
    from far_amd import _lib
    lib = _lib.load()
    pinned = {(1, 5, 5, 32, 32): (102656, 102400), (3, 9, 11, 32, 192): (614656, 614400), (3, 28, 28, 128, 192): (44237056, 2457600),
              (64, 28, 28, 128, 192): (103219456, 2457600), (64, 28, 28, 192, 192): (103219456, 3686400),
              (2, 28, 28, 64, 160): (12288256, 1024000)}
    for (N, H, W, cin, cout), (ws, image) in pinned.items():
        assert lib.far_conv_valid_wgrad_ws_bytes(N, H, W, cin, cout, 5) == ws, (N, H, W, cin, cout)
        assert lib.far_conv_valid_packed_bytes(cin, cout, 5) == image == 100 * cin * cout, (cin, cout)
    for refused in ((3, 9, 11, 32, 192, 3), (3, 9, 11, 48, 192, 5), (0, 9, 11, 32, 192, 5), (3, 4, 11, 32, 192, 5)):      # ksize 3, Cin 48, N = 0, H = 4
        assert lib.far_conv_valid_wgrad_ws_bytes(*refused) == 0, refused
    assert lib.far_conv_valid_packed_bytes(32, 192, 3) == 0 and lib.far_conv_valid_packed_bytes(48, 192, 5) == 0
