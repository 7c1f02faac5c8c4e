"""far_amd.vit8pt from images on the GPU (ViTEss(..., extractor=True)) on the seeded fill of tests/vit8pt_extractor_inputs.py, against
the float64 restatement (tests/vit8pt_extractor_ref.py, pinned to the reference's run by tests/test_vit8pt_extractor_cpu.py) and
against golden G26.

Bars: the extractor's features under the project's parity rule (tests/test_full_attention_gpu.py: _bar), at most
max(3 x dev32, 2^-20 max|out|) from float64 with dev32 the fp32 restatement's own deviation on the same GPU in the same run; the four
regression outputs at the project's bar for regression outputs, 1e-3 max|reference|."""
import os

import numpy as np
import pytest
import torch

from tests import vit8pt_extractor_inputs as ei
from tests import vit8pt_extractor_ref as er
from tests import vit8pt_inputs as vi
from tests.test_full_attention_gpu import _bar

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g26_vit8pt_extractor.npz')
_CACHE = {}


def setup(batch=ei.B):
    """-> (far_amd ViTEss with its extractor on the GPU, the seeded RefViTEssImages (fp32, CPU), inputs on the GPU)."""
    if batch not in _CACHE:
        from far_amd.vit8pt import ViTEss
        ref = er.RefViTEssImages(vi.vit_args())
        inp = ei.filled(ref, batch)
        ref.pose_mean, ref.pose_std = inp['pose_mean'], inp['pose_std']
        m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'], extractor=True)
        m.load_state_dict(ref.state_dict(), strict=True)
        gpu = {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in inp.items()}
        _CACHE[batch] = (m.eval().cuda(), ref, gpu)
    return _CACHE[batch]


def test_extract_features_against_float64_and_the_golden():
    m, ref, inp = setup()
    g = np.load(GOLDEN)
    r64, r32 = ref.as_dtype(torch.float64, 'cuda'), ref.as_dtype(torch.float32, 'cuda')
    for (h, w), images in zip(ei.SIZES, inp['images']):
        tag = f'{h}x{w}'
        intr = ei.image_intrinsics(images.shape).cuda()
        keep_i, keep_k = images.clone(), intr.clone()
        with torch.no_grad():
            feats, grid = m.extract_features(images, intr)
        assert feats.shape == (2 * ei.B, 576, 192) and feats.dtype == torch.float32 and not feats.requires_grad
        assert torch.equal(images, keep_i) and torch.equal(intr, keep_k)          # inputs are left as they are
        assert torch.equal(grid, m.update_intrinsics(images.shape, intr))
        assert m.extract_features(images)[1] is None
        f64, f32 = r64.extract_features(images), r32.extract_features(images)
        _bar(f'vit8pt extractor @ {tag}', feats, f64, float((f32.double() - f64).abs().max()))
        want = torch.from_numpy(g[f'features_{tag}']).cuda()
        _bar(f'vit8pt extractor @ {tag} vs the reference fp32 taps', ei.tap(feats), want, float((want.double() - ei.tap(f64)).abs().max()), 4.0)


def test_forward_from_images_against_the_golden():
    from far_amd import ops
    m, ref, inp = setup()
    g = np.load(GOLDEN)
    for (h, w), images in zip(ei.SIZES, inp['images']):
        tag = f'{h}x{w}'
        intr = ei.image_intrinsics(images.shape).cuda()
        keep = images.clone()
        ops.overflow_flag('cuda').zero_()
        with torch.no_grad():
            out = m(images, intr, loftr_num_corr=inp['loftr_num_corr'], loftr_preds=inp['loftr_preds'])
        assert not ops.activation_overflowed('cuda')
        assert torch.equal(images, keep)
        for name, t in zip(ei.OUTPUTS, out):
            want = g[f'{name}_{tag}']
            sc = float(np.abs(want).max())
            d = float(np.abs(t.cpu().numpy() - want).max())
            print(f'[vit8pt from images {tag}] {name}: max |got - reference| / max|reference| = {d / sc:.3e}')
            assert t.shape == want.shape and d <= 1e-3 * sc, name
        # forward(images) is forward_features(extract_features(images)): the same bits
        with torch.no_grad():
            out2 = m.forward_features(*m.extract_features(images, intr), inp['loftr_num_corr'], inp['loftr_preds'])
        for a, b in zip(out, out2):
            assert torch.equal(a, b)


def test_pairs_have_the_same_bits_alone_and_in_a_batch_of_three():
    m, _, inp = setup(batch=3)
    images = inp['images'][0]                                                 # (3, 2, 3, 37, 53)
    intr = ei.image_intrinsics(images.shape, 3).cuda()
    with torch.no_grad():
        out3 = m(images, intr, loftr_num_corr=inp['loftr_num_corr'], loftr_preds=inp['loftr_preds'])
        f3 = m.extract_features(images)[0]
        for b in range(3):
            s = slice(b, b + 1)
            assert torch.equal(m.extract_features(images[s])[0], f3[2 * b:2 * b + 2]), b
            out1 = m(images[s], intr[s], loftr_num_corr=inp['loftr_num_corr'][s], loftr_preds=inp['loftr_preds'][s])
            for name, a3, a1 in zip(ei.OUTPUTS, out3, out1):
                assert torch.equal(a3[s], a1), (b, name)


def test_train_mode_and_block_training_leave_the_extractor_frozen():
    m, _, inp = setup()
    images = inp['images'][0]
    with torch.no_grad():
        f0 = m.extract_features(images)[0]
    stats = {k: v.clone() for k, v in m.state_dict().items() if 'running_' in k or 'num_batches' in k}
    m.train()
    try:
        f1 = m.extract_features(images)[0]                                    # gradients enabled, frozen parameters: allowed
        assert torch.equal(f0, f1) and not f1.requires_grad                   # running statistics whatever .train() says
        for k, v in stats.items():
            assert torch.equal(m.state_dict()[k], v), k
        m.resnet.layer1[0].conv1.weight.requires_grad_(True)
        with pytest.raises(NotImplementedError, match='extractor'):
            m.extract_features(images)
        with torch.no_grad():
            assert torch.equal(m.extract_features(images)[0], f0)
    finally:
        m.resnet.layer1[0].conv1.weight.requires_grad_(False)
        m.eval()


def test_a_model_without_the_keyword_behaves_as_before():
    from far_amd.vit8pt import ViTEss, reference_state_dict
    m, ref, inp = setup()
    plain = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'])
    plain.load_state_dict(reference_state_dict(ref.state_dict()), strict=True)
    plain = plain.eval().cuda()
    images = inp['images'][0]
    with pytest.raises(NotImplementedError, match='forward_features'):
        plain(images)
    with torch.no_grad():
        feats, grid = m.extract_features(images, ei.image_intrinsics(images.shape).cuda())
        a = plain.forward_features(feats, grid, inp['loftr_num_corr'], inp['loftr_preds'])
        b = m.forward_features(feats, grid, inp['loftr_num_corr'], inp['loftr_preds'])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
