"""The kernels of the 8-Point-ViT's extractor at operator level: K24 (ops.conv_valid, the 5x5 unpadded convolution), K25 (ops.stem_rgb),
K26 (ops.maxpool3x3s2), and the 64-channel layers K9 / K17 had never run (ops.conv_nhwc).

Inputs are signed.  Bar: the project's parity rule (tests/test_full_attention_gpu.py: _bar) -- at most max(3 x dev32, 2^-20 max|out|)
from a float64 torch computation, with dev32 the fp32 torch computation's own deviation on the same GPU in the same run.  The max-pool
is exact (torch.equal).  Every new kernel: 20 launches at the workload's shape for 4 images bit-identical while a second stream runs
K9 work (the form of tests/test_determinism_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

from tests import vit8pt_extractor_ref as er
from tests.test_full_attention_gpu import _bar

pytestmark = pytest.mark.gpu
LAUNCHES = 20


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _bn(c, g):
    """A folded inference BatchNorm: (scale, shift) with signed shifts."""
    return 0.5 + torch.rand(c, device='cuda', generator=g), 0.3 * torch.randn(c, device='cuda', generator=g)


def _conv_ref(x, w, bias, scale, shift, res, relu, dtype, stride=1, padding=0):
    """act((conv(x) + bias) scale + shift (+ res)) on NHWC tensors, computed in `dtype` by torch."""
    y = F.conv2d(x.permute(0, 3, 1, 2).to(dtype), w.to(dtype), None if bias is None else bias.to(dtype), stride, padding).permute(0, 2, 3, 1)
    if scale is not None:
        y = y * scale.to(dtype) + shift.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return torch.relu(y) if relu else y


def _check_conv_valid(hw, cin, cout, seed):
    from far_amd import ops
    (H, W), N = hw, 3
    g = _gen(seed)
    x = torch.randn(N, H, W, cin, device='cuda', generator=g) * 3
    w = torch.randn(cout, cin, 5, 5, device='cuda', generator=g) * (2.0 / (25 * cin)) ** 0.5
    bias = 0.2 * torch.randn(cout, device='cuda', generator=g)
    scale, shift = _bn(cout, g)
    res = torch.randn(N, H - 4, W - 4, cout, device='cuda', generator=g)
    ops.overflow_flag('cuda').zero_()
    got = ops.conv_valid(x, ops.PackedConvValid(w))
    assert got.shape == (N, H - 4, W - 4, cout)
    r64 = _conv_ref(x, w, None, None, None, None, False, torch.float64)
    r32 = _conv_ref(x, w, None, None, None, None, False, torch.float32)
    _bar(f'conv_valid {cin}->{cout} @ {H}x{W} bare', got, r64, float((r32.double() - r64).abs().max()))
    pack = ops.PackedConvValid(w, scale, shift + scale * bias)
    got = ops.conv_valid(x, pack, residual=res, act='relu')
    r64 = _conv_ref(x, w, bias, scale, shift, res, True, torch.float64)
    r32 = _conv_ref(x, w, bias, scale, shift, res, True, torch.float32)
    _bar(f'conv_valid {cin}->{cout} @ {H}x{W} bias + BN + residual + ReLU', got, r64, float((r32.double() - r64).abs().max()))
    assert 0.2 < float((got > 0).float().mean()) < 0.8                      # the ReLU cuts
    assert not ops.activation_overflowed('cuda')
    # image n's output does not depend on the batch it is in
    assert torch.equal(ops.conv_valid(x[1:2].contiguous(), pack, residual=res[1:2].contiguous(), act='relu'), got[1:2])


@pytest.mark.parametrize('cin', [32, 128, 192])
@pytest.mark.parametrize('hw', [(9, 11), (5, 5), (28, 28)])
def test_conv_valid_against_float64(hw, cin):
    """9 x 11 -> 5 x 7 (partial tiles in both directions), 5 x 5 -> 1 x 1, 28 x 28 -> 24 x 24 (the workload); bare, and with bias + BN
    fold + residual + ReLU."""
    _check_conv_valid(hw, cin, 192, 1000 * hw[0] + cin)


@pytest.mark.parametrize('cin,cout', [(32, 32), (64, 160)])
def test_conv_valid_partial_n_tiles_against_float64(cin, cout):
    """Cout = 32 and 160 are no six full N-tiles (every other case has 192): a wave without an N-tile, waves with one or two of three."""
    _check_conv_valid((9, 11), cin, cout, 9000 + cin + 7 * cout)


def test_conv_valid_small_and_large_launches_have_the_same_bits():
    """A launch of fewer than 128 24-row workgroups takes the kernel's 8-row form: 64 images (192 workgroups, 24-row form) against
    the same images two at a time (18 workgroups, 8-row form) -- image n's output does not depend on the batch it is in."""
    from far_amd import ops
    g = _gen(64)
    x = torch.randn(64, 28, 28, 128, device='cuda', generator=g) * 3
    pack = ops.PackedConvValid(torch.randn(192, 128, 5, 5, device='cuda', generator=g) * 0.03, *_bn(192, g))
    res = torch.randn(64, 24, 24, 192, device='cuda', generator=g)
    big = ops.conv_valid(x, pack, residual=res, act='relu')
    for n in (0, 31, 62):
        assert torch.equal(ops.conv_valid(x[n:n + 2], pack, residual=res[n:n + 2], act='relu'), big[n:n + 2]), n


def test_conv_valid_refusals_and_range_guard():
    from far_amd import ops
    from far_amd._lib import FarHipError
    g = _gen(7)
    w = torch.randn(192, 32, 5, 5, device='cuda', generator=g) * 0.05
    pack = ops.PackedConvValid(w)
    for bad in (torch.randn(192, 48, 5, 5, device='cuda'), torch.randn(192, 32, 3, 3, device='cuda'), torch.randn(100, 32, 5, 5, device='cuda'),
                torch.randn(192, 32, 5, 5)):
        with pytest.raises(FarHipError):
            ops.PackedConvValid(bad)
    for shape in ((1, 4, 9, 32), (1, 9, 4, 32), (1, 9, 9, 64)):
        with pytest.raises(FarHipError):
            ops.conv_valid(torch.randn(*shape, device='cuda'), pack)
    with pytest.raises(FarHipError):
        ops.conv_valid(torch.randn(1, 9, 9, 32), pack)                                 # a CPU tensor: no eager fallback
    with pytest.raises(FarHipError):
        ops.conv_valid(torch.randn(1, 9, 9, 32, device='cuda'), pack, residual=torch.randn(1, 9, 9, 192, device='cuda'))
    x = torch.randn(2, 9, 9, 32, device='cuda', generator=g)
    ops.overflow_flag('cuda').zero_()
    ops.conv_valid(x, pack)
    assert not ops.activation_overflowed('cuda')
    x[1, 4, 4, 7] = 1.0e5                                                              # beyond 4094 at the default exponent
    y = ops.conv_valid(x, pack)
    assert ops.activation_overflowed('cuda')
    assert torch.isfinite(y[0]).all() and not torch.isfinite(y[1]).all()
    with ops.activation_exponent(-4):                                                  # 16 x the range: the same input passes
        y = ops.conv_valid(x, pack)
    assert not ops.activation_overflowed('cuda') and torch.isfinite(y).all()
    r64 = _conv_ref(x, w, None, None, None, None, False, torch.float64)
    assert float((y.double() - r64).abs().max()) <= 1e-5 * float(r64.abs().max())


def _stem_ref(images, w, scale, shift, dtype, pad_value=None):
    """relu(bn(conv7x7 s2 p3(resize224(normalise(flip(images)))))) of (B, 2, 3, H, W) images as NHWC in `dtype`; pad_value: pad with this raw pixel value
    instead of zero in normalised space (the WRONG form, to show that the border rows can tell)."""
    x = er.normalised_input(images, dtype)
    if pad_value is None:
        x = F.pad(x, (3, 3, 3, 3))
    else:
        z = er.normalised_input(torch.full((1, 2, 3, 1, 1), float(pad_value), device=images.device), dtype)[0, :, 0, 0]
        x = torch.stack([F.pad(x[:, c], (3, 3, 3, 3), value=float(z[c])) for c in range(3)], 1)
    y = F.conv2d(x, w.to(dtype), None, 2).permute(0, 2, 3, 1) * scale.to(dtype) + shift.to(dtype)
    return torch.relu(y)


@pytest.mark.parametrize('hw', [(37, 53), (224, 224), (300, 260)])
def test_stem_rgb_against_float64(hw):
    from far_amd import ops
    H, W = hw
    g = _gen(H)
    images = torch.randint(0, 256, (2, 3, H, W), device='cuda', generator=g).float()
    keep = images.clone()
    w = torch.randn(64, 3, 7, 7, device='cuda', generator=g) * (2.0 / 147) ** 0.5
    scale, shift = _bn(64, g)
    got = ops.stem_rgb(images, ops.PackedStemRGB(w, scale, shift))
    assert got.shape == (2, 112, 112, 64) and torch.equal(images, keep)
    r64 = _stem_ref(images.view(1, 2, 3, H, W), w, scale, shift, torch.float64)
    r32 = _stem_ref(images.view(1, 2, 3, H, W), w, scale, shift, torch.float32)
    dev32 = float((r32.double() - r64).abs().max())
    _bar(f'stem_rgb @ {H}x{W}', got, r64, dev32)
    assert 0.2 < float((got > 0).float().mean()) < 0.8
    # the first and last output rows and columns: there the zero padding IN NORMALISED SPACE decides -- a padding of raw zeros
    # (the normalisation folded into the weights) is far outside the bar on exactly these
    wrong = _stem_ref(images.view(1, 2, 3, H, W), w, scale, shift, torch.float64, pad_value=0.0)
    for name, sl in (('first row', (slice(None), 0)), ('last row', (slice(None), -1)), ('first column', (slice(None), slice(None), 0)),
                     ('last column', (slice(None), slice(None), -1))):
        d = _bar(f'stem_rgb @ {H}x{W} {name}', got[sl], r64[sl], dev32)
        assert float((wrong[sl] - r64[sl]).abs().max()) > 1000 * max(d, 3 * dev32), name
    # the resize tables are torch's own
    rows, cols = ops.resize_tables(H, W, 'cuda')
    idx = torch.arange(H * W, device='cuda', dtype=torch.float32).view(1, 1, H, W)
    assert torch.equal(F.interpolate(idx, size=224)[0, 0].long(), rows.long()[:, None] * W + cols.long()[None, :])
    # image n alone: the same bits
    assert torch.equal(ops.stem_rgb(images[1:2].contiguous(), ops.PackedStemRGB(w, scale, shift)), got[1:2])


def test_stem_rgb_refusals():
    from far_amd import ops
    from far_amd._lib import FarHipError
    w = torch.randn(64, 3, 7, 7, device='cuda')
    one = torch.ones(64, device='cuda')
    pack = ops.PackedStemRGB(w, one, one)
    with pytest.raises(FarHipError):
        ops.PackedStemRGB(torch.randn(64, 1, 7, 7, device='cuda'), one, one)
    with pytest.raises(FarHipError):
        ops.stem_rgb(torch.zeros(1, 3, 8, 8), pack)
    with pytest.raises(FarHipError):
        ops.stem_rgb(torch.zeros(1, 1, 8, 8, device='cuda'), pack)


@pytest.mark.parametrize('shape', [(2, 7, 9, 64), (2, 112, 112, 64)])
def test_maxpool_is_exact(shape):
    from far_amd import ops
    x = torch.randn(*shape, device='cuda', generator=_gen(shape[1]))
    x[0, 0, 0] = -5.0                                                        # a corner below zero: the padding must not win
    got = ops.maxpool3x3s2(x)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert got.shape == want.shape and torch.equal(got, want)
    assert float(got.min()) < 0
    from far_amd._lib import FarHipError
    with pytest.raises(FarHipError):
        ops.maxpool3x3s2(torch.randn(1, 8, 8, 6, device='cuda'))


@pytest.mark.parametrize('kind', ['3x3', '3x3 stride 2', '1x1 in_stride 2'])
def test_64_channel_layers_through_conv_nhwc(kind):
    """layer1's 64 -> 64 stride-1 3x3, layer2.0's 64 -> 128 stride-2 3x3 and its 1x1 stride-2 shortcut at 14 x 14: channel counts the
    backbone (narrowest: 128) never ran."""
    from far_amd import ops
    g = _gen(64 + len(kind))
    x = torch.randn(2, 14, 14, 64, device='cuda', generator=g) * 2
    cout, ks, st = (64, 3, 1) if kind == '3x3' else ((128, 3, 2) if kind == '3x3 stride 2' else (128, 1, 2))
    w = torch.randn(cout, 64, ks, ks, device='cuda', generator=g) * (2.0 / (64 * ks * ks)) ** 0.5
    scale, shift = _bn(cout, g)
    ho = (14 - 1) // st + 1
    res = torch.randn(2, ho, ho, cout, device='cuda', generator=g) if ks == 3 else None
    ops.overflow_flag('cuda').zero_()
    with torch.no_grad():
        if ks == 3:
            got = ops.conv_nhwc(x, ops.PackedConv(w, scale, shift, stride=st), residual=res, act='relu')
        else:
            got = ops.conv_nhwc(x, ops.PackedConv(w, scale, shift), in_stride=2)
    assert not ops.activation_overflowed('cuda')
    r64 = _conv_ref(x, w, None, scale, shift, res, ks == 3, torch.float64, st, ks // 2)
    r32 = _conv_ref(x, w, None, scale, shift, res, ks == 3, torch.float32, st, ks // 2)
    assert got.shape == r64.shape
    _bar(f'conv_nhwc 64 channels, {kind}', got, r64, float((r32.double() - r64).abs().max()))


class _K9Neighbour:
    """A second stream that runs K9 work (a 128 -> 196 stride-2 3x3 convolution of 8 images x 120 x 160) per call."""

    def __init__(self):
        from far_amd import ops
        g = _gen(9)
        self.side = torch.cuda.Stream()
        self.x = torch.randn(8, 120, 160, 128, device='cuda', generator=g)
        self.pc = ops.PackedConv(torch.randn(196, 128, 3, 3, device='cuda', generator=g) * 0.03, stride=2)
        torch.cuda.synchronize()

    def kick(self):
        from far_amd import ops
        with torch.cuda.stream(self.side), torch.no_grad():
            ops.conv_nhwc(self.x, self.pc, act='relu')

    def done(self):
        self.side.synchronize()
        torch.cuda.synchronize()


def _repeat(fn, what):
    nb = _K9Neighbour()
    first = fn().clone()
    for it in range(LAUNCHES):
        nb.kick()
        out = fn()
        if not torch.equal(out, first):
            raise AssertionError(f'{what}: differs at launch {it}: max |diff| {float((out - first).abs().max()):.3e}')
    nb.done()


def test_new_kernels_are_bit_identical_next_to_k9_work():
    from far_amd import ops
    g = _gen(20)
    x = torch.randn(4, 28, 28, 128, device='cuda', generator=g) * 3
    pd = ops.PackedConvValid(torch.randn(192, 128, 5, 5, device='cuda', generator=g) * 0.03, *_bn(192, g))
    p2 = ops.PackedConvValid(torch.randn(192, 192, 5, 5, device='cuda', generator=g) * 0.03, *_bn(192, g))
    x2 = torch.randn(4, 28, 28, 192, device='cuda', generator=g) * 3
    res = torch.randn(4, 24, 24, 192, device='cuda', generator=g)
    _repeat(lambda: ops.conv_valid(x, pd, residual=res, act='relu'), 'K24 128 -> 192 @ 4 x 28 x 28')
    _repeat(lambda: ops.conv_valid(x2, p2, act='relu'), 'K24 192 -> 192 @ 4 x 28 x 28')
    x64 = torch.randn(64, 28, 28, 128, device='cuda', generator=g) * 3                       # the 24-row form (192 workgroups)
    _repeat(lambda: ops.conv_valid(x64, pd, act='relu'), 'K24 128 -> 192 @ 64 x 28 x 28')
    images = torch.randint(0, 256, (4, 3, 300, 260), device='cuda', generator=g).float()
    ps = ops.PackedStemRGB(torch.randn(64, 3, 7, 7, device='cuda', generator=g) * 0.1, *_bn(64, g))
    _repeat(lambda: ops.stem_rgb(images, ps), 'K25 @ 4 x 300 x 260')
    y = torch.randn(4, 112, 112, 64, device='cuda', generator=g)
    _repeat(lambda: ops.maxpool3x3s2(y), 'K26 @ 4 x 112 x 112 x 64')
