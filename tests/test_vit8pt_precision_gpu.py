"""ViTEss.set_precision on the GPU: each 16-bit-operand stage alone and the whole 'fp16' mode on the models of
tests/test_vit8pt_gpu.py (trunk + head, golden G25) and tests/test_vit8pt_extractor_gpu.py (from images, golden G26), which carry the
reference's weights; the yardstick is the reference's recorded outputs.

The 16-bit stages are NARROWER THAN THE REFERENCE and are not held to its bars.  Per case and output, with e = max|got - recorded| /
max|recorded|: the outputs are finite, differ from the fp32-mode outputs, and e32 < e16.  The bar for e16 does not come from the new
kernels: the torch restatement of the model (tests/vit8pt_ref.py, tests/vit8pt_extractor_ref.py) runs under
torch.autocast('cuda', dtype=torch.float16) on the same GPU in the same run, t16 is ITS deviation from the same recorded outputs, and
e16 <= 3 t16 -- the factor 3 is the project's margin over a torch yardstick (tests/test_full_attention_gpu.py: _bar).  Every e32,
e16, t16 is printed ('[precision] ...'; profiles/vit8pt_fp16_parity.txt records a run)."""
import os

import numpy as np
import pytest
import torch

from tests import vit8pt_extractor_inputs as ei
from tests import vit8pt_extractor_ref as er
from tests import vit8pt_inputs as vi
from tests import vit8pt_ref as vr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OUTPUTS = ('tran_preds_unnorm', 'rot_preds', 'rot_preds_mtx', 'rot_preds_6d')
TRUNK_STAGES = ('blocks_dense', 'blocks_attn', 'cross')
_CACHE = {}


def _trunk_model(batch=vi.B):
    """This module's own copies (the models of the other test modules stay untouched): -> (ViTEss, RefViTEss, GPU inputs)."""
    key = ('trunk', batch)
    if key not in _CACHE:
        from far_amd.vit8pt import ViTEss
        ref = vr.RefViTEss(vi.vit_args())
        inp = vi.seeded_inputs(vi.seeded_fill(ref), batch)
        ref.pose_mean, ref.pose_std = inp['pose_mean'], inp['pose_std']
        m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'])
        m.load_state_dict(ref.state_dict(), strict=True)
        _CACHE[key] = (m.eval().cuda(), ref, {k: v.cuda() for k, v in inp.items()})
    return _CACHE[key]


def _image_model(batch=ei.B):
    key = ('images', batch)
    if key not in _CACHE:
        from far_amd.vit8pt import ViTEss
        ref = er.RefViTEssImages(vi.vit_args())
        inp = ei.filled(ref, batch)
        ref.pose_mean, ref.pose_std = inp['pose_mean'], inp['pose_std']
        m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'], extractor=True)
        m.load_state_dict(ref.state_dict(), strict=True)
        gpu = {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in inp.items()}
        _CACHE[key] = (m.eval().cuda(), ref, gpu)
    return _CACHE[key]


def _dev(outs, want):
    """Per output: max|got - recorded| / max|recorded|."""
    return [float(np.abs(t.detach().float().cpu().numpy() - w).max()) / float(np.abs(w).max()) for t, w in zip(outs, want)]


def _check(tag, stages, run, run_ref16, want):
    """run(): the model's outputs in its current mode; run_ref16(): the restatement's under fp16 autocast; want: the recorded outputs."""
    m = run.model
    try:
        m.set_precision('fp32')
        with torch.no_grad():
            o32 = run()
            m.set_precision(stages)
            o16 = run()
        t16 = _CACHE.get(('t16', tag))
        if t16 is None:
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
                t16 = _CACHE[('t16', tag)] = _dev(run_ref16(), want)
        e32, e16 = _dev(o32, want), _dev(o16, want)
        for name, a, b, x32, x16, y16 in zip(OUTPUTS, o32, o16, e32, e16, t16):
            print(f'[precision] {tag} {m.precision_stages} {name}: e32 {x32:.3e}  e16 {x16:.3e}  t16 (torch fp16 autocast) {y16:.3e}  '
                  f'e16 / t16 {x16 / y16:.2f}  bar 3')
        for name, a, b, x32, x16, y16 in zip(OUTPUTS, o32, o16, e32, e16, t16):
            assert torch.isfinite(b).all(), name
            assert not torch.equal(a, b), name
            assert x32 < x16, name
            assert x16 <= 3 * y16, name
    finally:
        m.set_precision('fp32')


def _trunk_runs():
    m, ref, inp = _trunk_model()
    run = lambda: m.forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
    run.model = m
    r32 = _CACHE.setdefault(('ref32', 'trunk'), ref.as_dtype(torch.float32, 'cuda'))
    run_ref = lambda: r32.forward_features(inp['features'], vi.VIT_INTRINSICS, inp['loftr_num_corr'], inp['loftr_preds'])
    g = np.load(os.path.join(GOLDEN, 'g25_vit8pt.npz'))
    return run, run_ref, [g[n] for n in OUTPUTS]


def _image_runs():
    m, ref, inp = _image_model()
    (h, w), images = ei.SIZES[0], inp['images'][0]                            # 37 x 53
    intr = ei.image_intrinsics(images.shape).cuda()
    run = lambda: m(images, intr, loftr_num_corr=inp['loftr_num_corr'], loftr_preds=inp['loftr_preds'])
    run.model = m
    r32 = _CACHE.setdefault(('ref32', 'images'), ref.as_dtype(torch.float32, 'cuda'))
    grid = tuple(float(v) for v in m.update_intrinsics(images.shape, ei.image_intrinsics(images.shape))[0, 0])
    run_ref = lambda: r32.forward_images(images, grid, inp['loftr_num_corr'], inp['loftr_preds'])
    g = np.load(os.path.join(GOLDEN, 'g26_vit8pt_extractor.npz'))
    return run, run_ref, [g[f'{n}_{h}x{w}'] for n in OUTPUTS]


@pytest.mark.parametrize('stages', [('blocks_dense',), ('blocks_attn',), ('cross',), TRUNK_STAGES], ids=lambda s: '+'.join(s))
def test_trunk_stages_against_the_recorded_outputs(stages):
    _check('forward_features', stages, *_trunk_runs())


@pytest.mark.parametrize('stages', [('extractor',), 'fp16'], ids=lambda s: s if isinstance(s, str) else '+'.join(s))
def test_from_images_against_the_recorded_outputs(stages):
    _check('forward(images) 37x53', stages, *_image_runs())


def test_round_trip_restores_the_bits_of_an_untouched_model():
    from tests.test_vit8pt_extractor_gpu import setup as setup_images
    from tests.test_vit8pt_gpu import setup as setup_trunk
    for mine, untouched in ((_trunk_runs()[0], setup_trunk()[0]), (_image_runs()[0], setup_images()[0])):
        m = mine.model
        assert 'precision_stages' not in untouched.__dict__                   # set_precision was never called on it
        mode = 'fp16' if m.has_extractor else TRUNK_STAGES
        with torch.no_grad():
            mine()                                                            # the fp32 images exist before the switch ...
            m.set_precision(mode)
            o16 = mine()                                                      # ... the fp16 ones are built next to them ...
            m.set_precision('fp32')
            back = mine()                                                     # ... and the fp32 ones are found again
        if m.has_extractor:
            inp = _image_model()[2]
            images = inp['images'][0]
            with torch.no_grad():
                want = untouched(images, ei.image_intrinsics(images.shape).cuda(), loftr_num_corr=inp['loftr_num_corr'],
                                 loftr_preds=inp['loftr_preds'])
        else:
            inp = _trunk_model()[2]
            with torch.no_grad():
                want = untouched.forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
        for name, a, b, c in zip(OUTPUTS, back, want, o16):
            assert torch.equal(a, b), name
            assert not torch.equal(a, c), name


def test_pairs_have_the_same_bits_alone_and_in_a_batch_of_three():
    m, _, inp = _trunk_model(batch=3)
    args = lambda s: (inp['features'][2 * s.start:2 * s.stop], inp['intrinsics'][s], inp['loftr_num_corr'][s], inp['loftr_preds'][s])
    mi, _, inpi = _image_model(batch=3)
    images = inpi['images'][0]
    intr = ei.image_intrinsics(images.shape, 3).cuda()
    try:
        m.set_precision(TRUNK_STAGES)
        mi.set_precision('fp16')
        with torch.no_grad():
            out3 = m.forward_features(*args(slice(0, 3)))
            img3 = mi(images, intr, loftr_num_corr=inpi['loftr_num_corr'], loftr_preds=inpi['loftr_preds'])
            for b in range(3):
                s = slice(b, b + 1)
                for name, a3, a1 in zip(OUTPUTS, out3, m.forward_features(*args(s))):
                    assert torch.equal(a3[s], a1), (b, name)
                out1 = mi(images[s], intr[s], loftr_num_corr=inpi['loftr_num_corr'][s], loftr_preds=inpi['loftr_preds'][s])
                for name, a3, a1 in zip(OUTPUTS, img3, out1):
                    assert torch.equal(a3[s], a1), (b, name, 'from images')
    finally:
        m.set_precision('fp32')
        mi.set_precision('fp32')


def test_gradients_are_refused_and_no_grad_runs():
    m, _, inp = _trunk_model()
    call = lambda: m.forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
    try:
        m.set_precision('fp32')
        with torch.no_grad():
            o32 = call()
        m.set_precision(TRUNK_STAGES).set_block_training()
        with pytest.raises(NotImplementedError, match='set_precision'):
            call()                                                            # parameters need gradients
        with torch.no_grad():
            o16 = call()                                                      # the stages apply whatever the training switch says
        m.set_block_training(False)
        with pytest.raises(NotImplementedError, match='set_precision'):
            call()
        with torch.no_grad():
            again = call()
        for a, b, c in zip(o16, again, o32):
            assert torch.equal(a, b) and not torch.equal(a, c)
    finally:
        m.set_precision('fp32').set_block_training(False)
    mi, _, inpi = _image_model()
    images = inpi['images'][0]
    try:
        mi.set_precision('fp16').set_extractor_training().train()
        with pytest.raises(NotImplementedError, match='set_precision'):
            mi.extract_features(images)
        with torch.no_grad():
            assert mi.extract_features(images)[0].shape == (2 * ei.B, 576, 192)
    finally:
        mi.set_precision('fp32').set_extractor_training(on=False).eval()
