"""The Map-free regressor on the GPU: the new kernels (K27 far_stem_conv_rgb_f16s, K28 far_upsample2x_pad_f32 / far_elu_f32) against
float64 torch, and far_amd.mapfree.RegressionModel on the seeded fill of tests/mapfree_reg_inputs.py against the float64 restatement
(tests/mapfree_reg_ref.py, pinned to the reference's run by tests/test_mapfree_regressor_cpu.py) and against golden G28.

Bars: the project's parity rule (tests/test_full_attention_gpu.py: _bar), at most max(3 x dev32, 2^-20 max|out|) from float64 with dev32
the fp32 torch composition's own deviation on the same GPU in the same run (factor 4 against the reference's stored fp32 taps); R and t
at the project's bar for regression outputs, 1e-3 max|reference|."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mapfree_reg_inputs as mi
from tests import mapfree_reg_ref as rr
from tests.test_determinism_gpu import _repeat
from tests.test_full_attention_gpu import _bar

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g28_mapfree_regressor.npz')
KW = dict(use_loftr_preds=True, use_vanilla_transformer=True)
_CACHE = {}


def setup():
    """-> (far_amd RegressionModel on the GPU, the seeded restatement in float64 and in fp32 on the GPU)."""
    if not _CACHE:
        from far_amd.mapfree import RegressionModel
        ref = mi.seeded_fill(rr.RefRegressionModel())
        m = RegressionModel(mi.config(), **KW)
        m.load_state_dict(ref.state_dict(), strict=True)
        r64 = mi.seeded_fill(rr.RefRegressionModel()).double().cuda()
        _CACHE['m'] = (m.cuda(), r64, ref.cuda())
    return _CACHE['m']


def _dev(a32, a64):
    return float((a32.double() - a64).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# K27
# ---------------------------------------------------------------------------------------------------------------------
def _stem_case(seed=5):
    from far_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5).cuda()
    scale, shift = (0.5 + torch.rand(64, generator=g)).cuda(), (0.3 * torch.randn(64, generator=g)).cuda()
    return ops.PackedStemRGB(w, scale, shift), w, scale, shift, g


def _stem_ref(img, w, scale, shift, dtype):
    y = F.conv2d(img.to(dtype), w.to(dtype), None, 2, 3) * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    return F.relu(y).permute(0, 2, 3, 1)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('size', [(37, 29), (9, 70), (64, 33)])
def test_stem_kernel_against_float64(size, n):
    from far_amd import ops
    pack, w, scale, shift, g = _stem_case()
    img = torch.randn(n, 3, *size, generator=g).cuda()
    keep = img.clone()
    ops.overflow_flag('cuda').zero_()
    y = ops.stem_conv_rgb(img, pack)
    assert y.shape == (n, (size[0] - 1) // 2 + 1, (size[1] - 1) // 2 + 1, 64) and torch.equal(img, keep)
    assert not ops.activation_overflowed('cuda')
    r64 = _stem_ref(img, w, scale, shift, torch.float64)
    _bar(f'K27 stem {size} x {n}', y, r64, _dev(_stem_ref(img, w, scale, shift, torch.float32), r64))
    for i in range(n):                                                   # image i alone: the same bits
        assert torch.equal(ops.stem_conv_rgb(img[i:i + 1].contiguous(), pack), y[i:i + 1]), i


def test_stem_kernel_reports_an_input_beyond_the_operand_range():
    from far_amd import ops
    pack, w, scale, shift, g = _stem_case()
    img = torch.randn(2, 3, 37, 29, generator=g).cuda()
    img[1, 2, 20, 11] = 5000.0                                           # > 65504 / 2^4
    ops.overflow_flag('cuda').zero_()
    ops.stem_conv_rgb(img, pack)
    assert ops.activation_overflowed('cuda')                             # (and the read cleared it)
    with ops.activation_exponent(0):                                     # 16 x the range: clean, and still at the bar
        y = ops.stem_conv_rgb(img, pack)
    assert not ops.activation_overflowed('cuda')
    r64 = _stem_ref(img, w, scale, shift, torch.float64)
    _bar('K27 stem at activation exponent 0', y, r64, _dev(_stem_ref(img, w, scale, shift, torch.float32), r64))


def test_encode_is_rerun_wider_by_the_guard():
    from far_amd import ops
    from far_amd.mapfree import RegressionModel
    m = RegressionModel(mi.config(), **KW)
    m.load_state_dict(setup()[2].state_dict(), strict=True)
    m = m.cuda()
    img = mi.seeded_images((37, 29), 1)[0].cuda()
    img[0, 1, 5, 7] = 5000.0
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        vol = m.encode(img)
    assert m.act_exp < ops._CONV_ACT_EXP and any('activation exponent' in str(w.message) for w in rec)
    assert torch.isfinite(vol).all() and not ops.activation_overflowed('cuda')
    with torch.no_grad():
        r64 = setup()[1].encode(img.double())
    assert float((vol.double() - r64).abs().max()) <= 1e-3 * float(r64.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# K28
# ---------------------------------------------------------------------------------------------------------------------
GLUE = [((3, 2), (6, 4)), ((3, 2), (5, 4)), ((6, 4), (10, 8))]          # (lo size, skip size): no pad; one row; two rows


@pytest.mark.parametrize('C', [32, 1024])
@pytest.mark.parametrize('lo_size, skip_size', GLUE)
def test_glue_kernels_against_float64(lo_size, skip_size, C):
    from far_amd import ops
    g = torch.Generator().manual_seed(11)
    N = 2
    lo = torch.randn(N, *lo_size, C, generator=g).cuda()
    skip = torch.randn(N, *skip_size, C // 2, generator=g).cuda()
    H, W = 2 * lo_size[0], 2 * lo_size[1]
    nchw = lambda t: t.permute(0, 3, 1, 2)
    up64 = F.interpolate(nchw(lo).double(), scale_factor=2, mode='bilinear', align_corners=True)
    up32 = F.interpolate(nchw(lo), scale_factor=2, mode='bilinear', align_corners=True)
    dy, dx = H - skip_size[0], W - skip_size[1]
    pad64 = F.pad(nchw(skip).double(), (dx // 2, dx - dx // 2, dy // 2, dy - dy // 2))
    up, padded = ops.upsample2x_pad(lo, skip)
    assert up.shape == (N, H, W, C) and padded.shape == (N, H, W, C // 2)
    if (dy, dx) == (0, 0):
        assert padded is skip                                            # nothing to pad: the skip map itself
    _bar(f'K28 upsample {lo_size} C {C}', nchw(up), up64, _dev(up32, up64))
    _bar(f'K28 pad {skip_size} -> {(H, W)} C {C // 2}', nchw(padded), pad64, 0.0)
    assert torch.equal(nchw(padded).double(), pad64)                     # a copy: exact
    # either half alone gives the same bits
    assert torch.equal(ops.upsample2x_pad(lo)[0], up) and ops.upsample2x_pad(lo)[1] is None
    alone = ops.upsample2x_pad(None, skip, size=(H, W))
    assert alone[0] is None and torch.equal(alone[1], padded)


def test_elu_against_float64():
    from far_amd import ops
    g = torch.Generator().manual_seed(12)
    x = torch.cat([torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, -30.0, 30.0, -1.0, 1.0, -88.0, -1e-7, 1e-7]),
                   3 * torch.randn(100003, generator=g)]).cuda()
    r64 = F.elu(x.double())
    dev32 = _dev(F.elu(x), r64)
    y = ops.elu(x)
    _bar('K28 elu', y, r64, dev32)
    assert float(y[0]) == 0.0 and float(y[6]) == pytest.approx(-1.0, abs=1e-7) and float(y[7]) == 30.0
    z = x.clone()
    assert ops.elu(z, inplace=True) is z and torch.equal(z, y)
    # an odd count behind an offset: the scalar tail and the unaligned form
    assert torch.equal(ops.elu(x[1:10002]), y[1:10002])


# ---------------------------------------------------------------------------------------------------------------------
# The model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(37, 29), (50, 33), (64, 48)])
def test_encode_against_float64_alone_and_in_a_batch(size):
    m, r64, r32 = setup()
    img = torch.cat(mi.seeded_images(size, 2))[:3].contiguous().cuda()   # three images
    keep = img.clone()
    vol = m.encode(img)
    h, w = 4 * -(-size[0] // 16), 4 * -(-size[1] // 16)
    assert vol.shape == (3, 32, h, w) and vol.dtype == torch.float32 and not vol.requires_grad and torch.equal(img, keep)
    with torch.no_grad():
        v64, v32 = r64.encode(img.double()), r32.encode(img)
    _bar(f'encode @ {size}', vol, v64, _dev(v32, v64))
    for i in range(3):
        assert torch.equal(m.encode(img[i:i + 1]), vol[i:i + 1]), i


def test_regress_against_float64():
    m, r64, r32 = setup()
    v0, v1 = (t.cuda() for t in mi.seeded_volumes())
    rt, inl = (t.cuda() for t in mi.seeded_solver_outputs())
    taps, o64, o32 = {}, {}, {}
    R, t = m.regress(v0, v1, rt, inl, taps)
    with torch.no_grad():
        R64, t64 = r64.regress(v0.double(), v1.double(), rt, inl, o64)
        r32.regress(v0, v1, rt, inl, o32)
    assert R.shape == (mi.B, 6) and t.shape == (mi.B, 3)
    _bar('regress: x3', taps['x3'], o64['x3'], _dev(o32['x3'], o64['x3']))
    _bar('regress: transformer output', taps['transformer'], o64['transformer'], _dev(o32['transformer'], o64['transformer']))
    for name, a, b in (('R', R, R64), ('t', t, t64)):
        d, sc = float((a.double() - b).abs().max()), float(b.abs().max())
        print(f'[regress] {name}: max |got - float64| / max|float64| = {d / sc:.3e}')
        assert d <= 1e-3 * sc, name
    with pytest.raises(ValueError, match='12 x 9'):
        m.regress(v0[:, :, :80].contiguous(), v1[:, :, :80].contiguous(), rt, inl)


def _data(batch=mi.B, prior=False):
    im0, im1 = mi.seeded_images(batch=batch)
    rt, inl = mi.seeded_solver_outputs(batch, prior=prior)
    return {'image0_reg': im0.cuda(), 'image1_reg': im1.cuda(), 'loftr_rt': rt.cuda(), 'inliers': inl.cuda()}


@pytest.mark.parametrize('prior', [False, True], ids=['noprior', 'prior'])
def test_whole_model_against_the_golden(prior):
    from far_amd import ops
    m, r64, _ = setup()
    g = np.load(GOLDEN)
    tag = 'prior' if prior else 'noprior'
    m.use_prior = prior
    try:
        data = _data(prior=prior)
        keep = {k: v.clone() for k, v in data.items()}
        ops.overflow_flag('cuda').zero_()
        R, t = m(data)
        assert not ops.activation_overflowed('cuda') and m.act_exp == ops._CONV_ACT_EXP
        assert all(torch.equal(data[k], v) for k, v in keep.items())              # inputs are left as they are
        assert data['R'] is R and data['t'] is t and R.shape == (mi.B, 6) and t.shape == (mi.B, 3)
        for name, got in (('R', R), ('t', t)):
            want = g[f'{name}_{tag}']
            d, sc = float(np.abs(got.cpu().numpy() - want).max()), float(np.abs(want).max())
            print(f'[mapfree regressor {tag}] {name}: max |got - reference| / max|reference| = {d / sc:.3e}')
            assert d <= 1e-3 * sc, name
        # forward is regress(encode(.), encode(.)): the same bits
        vol0, vol1 = m.encode(data['image0_reg']), m.encode(data['image1_reg'])
        taps = {}
        R2, t2 = m.regress(vol0, vol1, data['loftr_rt'], data['inliers'], taps)
        assert torch.equal(R, R2) and torch.equal(t, t2)
        if not prior:                                                             # the taps do not depend on the prior
            with torch.no_grad():
                v64 = torch.cat([r64.encode(data['image0_reg'].double()), r64.encode(data['image1_reg'].double())])
                o64 = {}
                r64.features(v64[:mi.B], v64[mi.B:], out=o64)
            want = torch.from_numpy(g['vol']).cuda()
            _bar('encoder volume vs the reference fp32 taps', mi.tap_volume(torch.cat([vol0, vol1])), want,
                 _dev(want, mi.tap_volume(v64)), 4.0)
            want = torch.from_numpy(g['x3']).cuda()
            _bar('x3 vs the reference fp32 taps', mi.tap_x3(taps['x3']), want, _dev(want, mi.tap_x3(o64['x3'])), 4.0)
    finally:
        m.use_prior = False


@pytest.mark.parametrize('prior', [False, True], ids=['noprior', 'prior'])
def test_a_pair_has_the_same_bits_alone_and_in_a_batch_of_three(prior):
    m, _, _ = setup()
    m.use_prior = prior
    try:
        data = _data(3, prior)
        R3, t3 = m(dict(data))
        R1, t1 = m({k: v[1:2] for k, v in data.items()})
        assert torch.equal(R3[1:2], R1) and torch.equal(t3[1:2], t1)
    finally:
        m.use_prior = False


def test_forward_through_match_and_solve():
    """forward with the matcher and the solver in the loop: far_amd.loftr.LoFTR on upstream_loftr_config() with seeded weights."""
    from far_amd import mapfree, synth
    from far_amd.loftr import LoFTR
    matcher = LoFTR(mapfree.upstream_loftr_config()).eval()
    synth.load_synthetic(matcher, seed=0)
    matcher = matcher.cuda()
    m = mapfree.RegressionModel(mi.config(), use_prior=True, matcher=matcher, **KW)
    m.load_state_dict(setup()[2].state_dict(), strict=True)
    m = m.cuda()
    B = 2
    im0, im1 = mi.seeded_images(batch=B)
    g0, g1 = synth.synth_image_pair(B, seed=23, hw=(544, 720))
    K = torch.tensor([[590.0, 0, 360.], [0, 610.0, 272.], [0, 0, 1.]]).expand(B, 3, 3).contiguous().cuda()
    data = {'image0_reg': im0.cuda(), 'image1_reg': im1.cuda(), 'image0': torch.from_numpy(g0).cuda(), 'image1': torch.from_numpy(g1).cuda(),
            'K_color0': K, 'K_color1': K.clone()}
    priors = []
    solve = m.pose_solver.solve_batch
    m.pose_solver.solve_batch = lambda *a, **k: (priors.append(a[5] if len(a) > 5 else k.get('priorRT')), solve(*a, **k))[1]
    R, t = m(data)
    assert R.shape == (B, 6) and t.shape == (B, 3) and torch.isfinite(R).all() and torch.isfinite(t).all()
    assert data['loftr_rt'].shape == (B, 3, 4) and data['inliers'].shape == (B, 3)
    assert len(priors) == 2 and priors[0] is None and np.asarray(priors[1]).shape == (B, 3, 4)
    # the second solve received [rotation_6d_to_matrix(R) | t] of the FIRST loop: replay that loop from the cached first solve
    m1 = mapfree.RegressionModel(mi.config(), use_prior=True, **KW)
    m1.load_state_dict(m.state_dict(), strict=True)
    m1 = m1.cuda()
    first = {'image0_reg': data['image0_reg'], 'image1_reg': data['image1_reg']}
    match = {k: data[k] for k in ('image0', 'image1', 'K_color0', 'K_color1')}
    mapfree.match_and_solve(matcher, match, m.pose_solver.__class__(mi.config().SOLVER, True), None, use_prior=True)
    first.update(loftr_rt=match['loftr_rt'], inliers=match['inliers'])
    vol0, vol1 = m1.encode(first['image0_reg']), m1.encode(first['image1_reg'])
    R1, t1 = m1.regress(vol0, vol1, first['loftr_rt'], first['inliers'])
    want = torch.cat([mapfree.rotation_6d_to_matrix(R1), t1.unsqueeze(2)], dim=-1).cpu().numpy()
    assert np.array_equal(np.asarray(priors[1]), want)


def test_stem_and_encode_are_bit_identical_next_to_a_busy_stream():
    from far_amd import ops
    m, _, _ = setup()
    pack, _, _, _, g = _stem_case()
    img = torch.randn(8, 3, 360, 270, generator=g).cuda()
    _repeat(lambda: ops.stem_conv_rgb(img, pack), 'K27 stem')
    small = torch.cat(mi.seeded_images((64, 48), 2)).contiguous().cuda()
    _repeat(lambda: m.encode(small), 'encode @ 64 x 48')
