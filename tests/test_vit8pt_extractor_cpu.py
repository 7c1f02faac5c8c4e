"""far_amd.vit8pt with its extractor (ViTEss(..., extractor=True)), the parts that need no GPU: the module's state dict against the
reference's names, reference_state_dict, the frozen-extractor rules -- and the float64 restatement (tests/vit8pt_extractor_ref.py)
against golden G26, which pins the yardstick of the GPU tests to the reference's own run, with the conditions the seeded fill
(tests/vit8pt_extractor_inputs.py) promises."""
import os

import numpy as np
import pytest
import torch

from tests import vit8pt_extractor_inputs as ei
from tests import vit8pt_extractor_ref as er
from tests import vit8pt_inputs as vi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g26_vit8pt_extractor.npz')


def _bn(prefix, c):
    return {prefix + '.weight': (c,), prefix + '.bias': (c,), prefix + '.running_mean': (c,), prefix + '.running_var': (c,),
            prefix + '.num_batches_tracked': ()}


def expected_extractor_entries():
    """The extractor's state-dict entries, written out: name -> shape."""
    e = {'resnet.conv1.weight': (64, 3, 7, 7)}
    e.update(_bn('resnet.bn1', 64))
    for layer, cin, cout in (('layer1', 64, 64), ('layer2', 64, 128)):
        for i in (0, 1):
            p = f'resnet.{layer}.{i}'
            e[p + '.conv1.weight'] = (cout, cin if i == 0 else cout, 3, 3)
            e[p + '.conv2.weight'] = (cout, cout, 3, 3)
            e.update(_bn(p + '.bn1', cout))
            e.update(_bn(p + '.bn2', cout))
    e['resnet.layer2.0.downsample.0.weight'] = (128, 64, 1, 1)
    e.update(_bn('resnet.layer2.0.downsample.1', 128))
    f = 'extractor_final_conv'
    e.update({f + '.conv1.weight': (192, 128, 3, 3), f + '.conv1.bias': (192,), f + '.conv2.weight': (192, 192, 5, 5), f + '.conv2.bias': (192,),
              f + '.downsample.0.weight': (192, 128, 5, 5), f + '.downsample.0.bias': (192,)})
    for n in ('norm1', 'norm2', 'norm3', 'downsample.1'):
        e.update(_bn(f'{f}.{n}', 192))
    return e


def test_state_dict_with_and_without_the_keyword():
    from far_amd.vit8pt import ViTEss
    plain = ViTEss(vi.vit_args())
    m = ViTEss(vi.vit_args(), extractor=True)
    sd0, sd = plain.state_dict(), m.state_dict()
    assert not any(k.startswith(ei.EXTRACTOR) for k in sd0)                   # without the keyword: today's keys
    assert not hasattr(plain, 'resnet') and not hasattr(plain, 'extractor_final_conv')
    want = expected_extractor_entries()
    got = {k: tuple(v.shape) for k, v in sd.items() if k.startswith(ei.EXTRACTOR)}
    assert got == want
    assert {k: tuple(v.shape) for k, v in sd.items() if not k.startswith(ei.EXTRACTOR)} == {k: tuple(v.shape) for k, v in sd0.items()}
    fc = m.extractor_final_conv
    assert fc.downsample[1] is fc.norm3
    assert isinstance(m.resnet.conv1, torch.nn.Conv2d) and m.resnet.conv1.stride == (2, 2) and m.resnet.conv1.padding == (3, 3)
    assert m.resnet.layer2[0].conv1.stride == (2, 2) and m.resnet.layer2[0].downsample[0].stride == (2, 2)
    assert fc.conv1.padding == (1, 1) and fc.conv2.padding == (0, 0) and fc.downsample[0].padding == (0, 0)
    # the restatement the GPU tests compare with has the same entries
    ref = er.RefViTEssImages(vi.vit_args())
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}


def test_reference_state_dict_round_trip():
    from far_amd.vit8pt import ViTEss, reference_state_dict
    ref = er.RefViTEssImages(vi.vit_args())
    ei.filled(ref)
    ckpt = dict(ref.state_dict())                                             # a released checkpoint: the whole ResNet18
    ckpt.update({'resnet.layer3.0.conv1.weight': torch.zeros(256, 128, 3, 3), 'resnet.layer3.0.bn1.running_mean': torch.zeros(256),
                 'resnet.layer4.1.conv2.weight': torch.zeros(512, 512, 3, 3), 'resnet.layer4.1.bn2.num_batches_tracked': torch.tensor(0)})
    m = ViTEss(vi.vit_args(), extractor=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(ckpt, strict=True)
    res = m.load_state_dict(reference_state_dict(ckpt, extractor=True), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    plain = ViTEss(vi.vit_args())
    kept = reference_state_dict(ckpt)
    assert not any(k.startswith(ei.EXTRACTOR) for k in kept)
    res = plain.load_state_dict(kept, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_the_extractor_is_frozen_and_refuses_cpu_tensors_and_training():
    from far_amd._lib import FarHipError
    from far_amd.vit8pt import ViTEss
    m = ViTEss(vi.vit_args(), extractor=True)
    ext = [p for n, p in m.named_parameters() if n.startswith(ei.EXTRACTOR)]
    assert ext and not any(p.requires_grad for p in ext)
    assert all(p.requires_grad for n, p in m.named_parameters() if not n.startswith(ei.EXTRACTOR))
    images = torch.zeros(1, 2, 3, 8, 8)
    with pytest.raises(FarHipError):
        m(images)                                                             # CPU tensors: no eager fallback
    with pytest.raises(ValueError):
        m.extract_features(torch.zeros(2, 3, 8, 8))
    m.extractor_final_conv.conv2.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='extractor'):
        m.extract_features(images)
    m.extractor_final_conv.conv2.weight.requires_grad_(False)
    # a model without the keyword: as before
    plain = ViTEss(vi.vit_args())
    with pytest.raises(NotImplementedError, match='forward_features'):
        plain(images)
    with pytest.raises(NotImplementedError, match='forward_features'):
        plain.extract_features(images)


@pytest.fixture(scope='module')
def restated():
    ref = er.RefViTEssImages(vi.vit_args())
    inp = ei.filled(ref)
    ref.pose_mean, ref.pose_std = inp['pose_mean'], inp['pose_std']
    return ref.as_dtype(torch.float64), inp


def test_the_restatement_reproduces_g26_and_the_fill_conditions_hold(restated):
    from far_amd.vit8pt import update_intrinsics
    r64, inp = restated
    g = np.load(GOLDEN)
    assert int(g['seed']) == ei.SEED
    for (h, w), images in zip(ei.SIZES, inp['images']):
        tag = f'{h}x{w}'
        assert float(images.min()) >= 0 and float(images.max()) <= 255 and torch.equal(images, images.round())
        taps = []
        f64 = r64.extract_features(images, taps)
        assert f64.shape == (2 * ei.B, 576, 192)
        # the fill's promises, on the float64 restatement
        assert len(taps) == 12
        for i, (share, amax) in enumerate(taps):
            print(f'[G26 {tag}] ReLU {i}: positive share {share:.3f}  max |.| {amax:.1f}')
            assert ei.RELU_SHARE[0] <= share <= ei.RELU_SHARE[1], (tag, i, share)
            assert amax <= ei.ACT_MAX, (tag, i, amax)
        # the reference's fp32 run against the float64 restatement.  The bound is fp32's: 2^-24 per operation, sums of up to 4800
        # terms (5 x 5 x 192), so about sqrt(4800) 2^-24 = 4e-6 of the output scale per layer in the random-sign model; 1e-5 max|.|
        # (1e-4 for the four outputs behind the 26880-wide head) bounds the reference's own rounding and nothing else
        want = torch.from_numpy(g[f'features_{tag}']).double()
        d = float((ei.tap(f64) - want).abs().max())
        sc = float(f64.abs().max())
        print(f'[G26 {tag}] features: reference fp32 vs float64 restatement {d:.3e}  (max |.| {sc:.3f})')
        assert want.shape == ei.tap(f64).shape and d <= 1e-5 * sc
        grid = tuple(float(v) for v in update_intrinsics(images.shape, ei.image_intrinsics(images.shape))[0, 0])
        out = r64.forward_features(f64, grid, inp['loftr_num_corr'], inp['loftr_preds'])
        for name, t in zip(ei.OUTPUTS, out):
            ref = g[f'{name}_{tag}']
            d = float(np.abs(t.numpy() - ref).max())
            print(f'[G26 {tag}] {name}: reference fp32 vs float64 restatement {d:.3e}')
            assert t.shape == ref.shape and d <= 1e-4 * float(np.abs(ref).max()), name
