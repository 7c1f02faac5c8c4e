"""K24's backward at operator level: ops.conv_valid_dgrad, ops.conv_valid_wgrad (the input and weight gradients of the 5x5 unpadded
convolution) and ops.conv_valid_train (the autograd.Function over K24 and the two).

Inputs are signed, from seeded device generators; gradients dy ~ 1e-3 randn (as test_conv_wgrad_random_shapes_sweep).  Bar: the
project's parity rule (tests/test_full_attention_gpu.py: _bar) -- at most max(3 x dev32, 2^-20 max|r64|) from float64 torch autograd of
F.conv2d, with dev32 the deviation of fp32 torch autograd on the same GPU in the same run.  Shapes: 5 x 5 (one output pixel: every input
pixel receives one tap, dw is the plain outer product), 9 x 11 (partial tiles in both directions, 35 output pixels), 28 x 28 (the
workload), channels 32 / 128 / 192 -> 192 (dgrad's output channel count is Cin: 32 and 128 leave N-tiles of its workgroups empty),
and 32 -> 32, 64 -> 160 at 9 x 11 (the only cases whose Cout is not six full N-tiles)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_extractor_kernels_gpu import _gen, _repeat
from tests.test_full_attention_gpu import _bar

pytestmark = pytest.mark.gpu
COUT = 192


def _autograd(x, w, dy, dtype):
    """(dx, dw) of y = conv5x5_valid(x, w) under torch autograd in `dtype`; NHWC x / dy / dx."""
    xd = x.permute(0, 3, 1, 2).to(dtype).requires_grad_(True)
    wd = w.to(dtype).requires_grad_(True)
    y = F.conv2d(xd, wd)
    dx, dw = torch.autograd.grad(y, (xd, wd), dy.permute(0, 3, 1, 2).to(dtype))
    return dx.permute(0, 2, 3, 1).contiguous(), dw


@functools.lru_cache(maxsize=None)
def _case(N, H, W, cin, cout=COUT):
    """Inputs and both references of one shape, computed once and shared by the tests (never modified)."""
    g = _gen(100000 * N + 1000 * H + cin + (0 if cout == COUT else 7 * cout))
    x = torch.randn(N, H, W, cin, device='cuda', generator=g) * 3
    w = torch.randn(cout, cin, 5, 5, device='cuda', generator=g) * (2.0 / (25 * cin)) ** 0.5
    dy = 1e-3 * torch.randn(N, H - 4, W - 4, cout, device='cuda', generator=g)
    dx64, dw64 = _autograd(x, w, dy, torch.float64)
    dx32, dw32 = _autograd(x, w, dy, torch.float32)
    return x, w, dy, dx64, dw64, float((dx32.double() - dx64).abs().max()), float((dw32.double() - dw64).abs().max())


@pytest.mark.parametrize('cin', [32, 128, 192])
@pytest.mark.parametrize('hw', [(5, 5), (9, 11), (28, 28)])
def test_conv_valid_dgrad_against_float64(hw, cin):
    from far_amd import ops
    (H, W), N = hw, 3
    x, w, dy, dx64, _, dev32, _ = _case(N, H, W, cin)
    ops.overflow_flag('cuda').zero_()
    got = ops.conv_valid_dgrad(dy, w)
    assert got.shape == (N, H, W, cin)
    _bar(f'conv_valid_dgrad {cin}->192 @ {N}x{H}x{W}', got, dx64, dev32)
    assert not ops.activation_overflowed('cuda')
    # image n's dx does not depend on the batch it is in (one launch form for every size); a ready-made image gives the same bits.
    # The gradient scale is the batch's, as in a training step: it is an input of the kernel (one image alone would derive its own
    # power of two from its own maximum, and the fp16 lo plane of small entries rounds differently under another one).
    fwd = ops.PackedConvValid(w)
    pd = ops.PackedConvValid(w, dgrad=True, pack_scale=fwd.pack_scale)
    sc = ops.grad_scale(dy)
    assert torch.equal(ops.conv_valid_dgrad(dy, pd, dy_scale=sc), got)
    assert torch.equal(ops.conv_valid_dgrad(dy[1:2].contiguous(), pd, dy_scale=sc), got[1:2])


def test_conv_valid_dgrad_many_images_equal_two_at_a_time():
    """64 images at once (the training batch) against the same images two at a time: the same bits."""
    from far_amd import ops
    g = _gen(64)
    w = torch.randn(192, 128, 5, 5, device='cuda', generator=g) * 0.03
    dy = 1e-3 * torch.randn(64, 24, 24, 192, device='cuda', generator=g)
    fwd = ops.PackedConvValid(w)
    pd = ops.PackedConvValid(w, dgrad=True, pack_scale=fwd.pack_scale)
    sc = ops.grad_scale(dy)                                   # the batch's scale: a part of the batch alone would choose its own
    big = ops.conv_valid_dgrad(dy, pd, dy_scale=sc)
    for n in (0, 31, 62):
        assert torch.equal(ops.conv_valid_dgrad(dy[n:n + 2], pd, dy_scale=sc), big[n:n + 2]), n


@pytest.mark.parametrize('cin', [32, 128, 192])
@pytest.mark.parametrize('nhw', [(3, 5, 5), (1, 5, 5), (3, 9, 11), (3, 28, 28), (5, 28, 28)])
def test_conv_valid_wgrad_against_float64(nhw, cin):
    """N = 1 at 5 x 5: dw is one outer product; N = 5 at 28 x 28: 240 strip rows in more than twenty pixel ranges of the two-stage sum."""
    from far_amd import ops
    N, H, W = nhw
    x, w, dy, _, dw64, _, dev32 = _case(N, H, W, cin)
    ops.overflow_flag('cuda').zero_()
    got = ops.conv_valid_wgrad(x, dy)
    assert got.shape == (COUT, cin, 5, 5)
    _bar(f'conv_valid_wgrad {cin}->192 @ {N}x{H}x{W}', got, dw64, dev32)
    assert not ops.activation_overflowed('cuda')
    assert torch.equal(ops.conv_valid_wgrad(x, dy, dy_scale=ops.grad_scale(dy), act_exp=4), got)


@pytest.mark.parametrize('cin,cout', [(32, 32), (64, 160)])
def test_partial_n_tiles_against_float64(cin, cout):
    """Cout = 32 and 160 (every other case has 192): the dgrad reduces over one and five chunks instead of six; the wgrad's last pair of
    co tiles has one tile only; Cin = 32 / 64 leave N-tiles of the dgrad's workgroups empty."""
    from far_amd import ops
    N, H, W = 3, 9, 11
    x, w, dy, dx64, dw64, dev32x, dev32w = _case(N, H, W, cin, cout)
    ops.overflow_flag('cuda').zero_()
    dx = ops.conv_valid_dgrad(dy, w)
    assert dx.shape == (N, H, W, cin)
    _bar(f'conv_valid_dgrad {cin}->{cout} @ {N}x{H}x{W}', dx, dx64, dev32x)
    dw = ops.conv_valid_wgrad(x, dy)
    assert dw.shape == (cout, cin, 5, 5)
    _bar(f'conv_valid_wgrad {cin}->{cout} @ {N}x{H}x{W}', dw, dw64, dev32w)
    assert not ops.activation_overflowed('cuda')
    # image n's dx does not depend on the batch it is in (under the batch's gradient scale, as above)
    pd = ops.PackedConvValid(w, dgrad=True, pack_scale=ops.PackedConvValid(w).pack_scale)
    sc = ops.grad_scale(dy)
    assert torch.equal(ops.conv_valid_dgrad(dy, pd, dy_scale=sc), dx)
    assert torch.equal(ops.conv_valid_dgrad(dy[1:2].contiguous(), pd, dy_scale=sc), dx[1:2])
    assert torch.equal(ops.conv_valid_wgrad(x, dy, dy_scale=sc, act_exp=4), dw)


@pytest.mark.parametrize('which', ['dgrad', 'wgrad'])
def test_scale_invariance(which):
    """dy times 2^-20 and times 2^10: the same relative error within a factor of 2 -- the device-side gradient scale places any
    magnitude in the split's window."""
    from far_amd import ops
    x, w, dy, dx64, dw64, _, _ = _case(3, 9, 11, 128)
    errs = []
    for e in (0, -20, 10):
        s = 2.0 ** e
        got, ref = (ops.conv_valid_dgrad(dy * s, w), dx64 * s) if which == 'dgrad' else (ops.conv_valid_wgrad(x, dy * s), dw64 * s)
        errs.append(float((got.double() - ref).abs().max()) / float(ref.abs().max()))
        print(f'[scale] {which} dy x 2^{e}: relative error {errs[-1]:.3e}')
    assert all(torch.isfinite(torch.tensor(errs))) and errs[0] > 0
    for v in errs[1:]:
        assert errs[0] / 2 <= v <= errs[0] * 2, errs


def test_new_kernels_are_bit_identical_next_to_k9_work():
    from far_amd import ops
    g = _gen(21)
    for cin in (128, 192):
        x = torch.randn(4, 28, 28, cin, device='cuda', generator=g) * 3
        w = torch.randn(192, cin, 5, 5, device='cuda', generator=g) * 0.03
        dy = 1e-3 * torch.randn(4, 24, 24, 192, device='cuda', generator=g)
        fwd = ops.PackedConvValid(w)
        pd = ops.PackedConvValid(w, dgrad=True, pack_scale=fwd.pack_scale)
        sc = ops.grad_scale(dy)
        _repeat(lambda: ops.conv_valid_dgrad(dy, pd, dy_scale=sc), f'K24 dgrad {cin} -> 192 @ 4 x 28 x 28')
        _repeat(lambda: ops.conv_valid_wgrad(x, dy, dy_scale=sc), f'K24 wgrad {cin} -> 192 @ 4 x 28 x 28')


def test_conv_valid_train_gradients_and_pack_refresh():
    from far_amd import ops
    g = _gen(31)
    x = (torch.randn(2, 9, 11, 128, device='cuda', generator=g) * 3).requires_grad_(True)
    w = (torch.randn(192, 128, 5, 5, device='cuda', generator=g) * 0.03).requires_grad_(True)
    dy = 1e-3 * torch.randn(2, 5, 7, 192, device='cuda', generator=g)
    cache = ops.PackCache()
    y = ops.conv_valid_train(x, w, cache, 'layer')
    assert torch.equal(y, ops.conv_valid(x.detach(), ops.PackedConvValid(w)))
    y.backward(dy)
    assert torch.equal(x.grad, ops.conv_valid_dgrad(dy, w.detach()))
    assert torch.equal(w.grad, ops.conv_valid_wgrad(x.detach(), dy))
    images = (cache.get(('layer', 'valid'), [w], None), cache.get(('layer', 'valid', 'dgrad'), [w], None))
    with torch.no_grad():                                                  # an optimizer step: in place, 8 x the magnitude
        w.mul_(8.0).add_(0.01 * torch.randn(w.shape, device='cuda', generator=g))
    x.grad = None
    y = ops.conv_valid_train(x, w, cache, 'layer')
    assert torch.equal(y, ops.conv_valid(x.detach(), ops.PackedConvValid(w)))
    y.backward(dy)
    assert torch.equal(x.grad, ops.conv_valid_dgrad(dy, w.detach()))       # a freshly packed dgrad image of the NEW weight
    now = (cache.get(('layer', 'valid'), [w], None), cache.get(('layer', 'valid', 'dgrad'), [w], None))
    assert now[0] is images[0] and now[1] is images[1]                     # refreshed in place, not rebuilt
    assert now[1].pack_scale.data_ptr() == now[0].pack_scale.data_ptr()


def test_refusals():
    from far_amd import ops
    from far_amd._lib import FarHipError
    g = _gen(8)
    w = torch.randn(192, 32, 5, 5, device='cuda', generator=g) * 0.05
    x = torch.randn(2, 9, 9, 32, device='cuda', generator=g)
    dy = torch.randn(2, 5, 5, 192, device='cuda', generator=g)
    cache = ops.PackCache()
    ops.conv_valid_dgrad(dy, w), ops.conv_valid_wgrad(x, dy), ops.conv_valid_train(x, w, cache, 'ok')      # the good case passes
    with pytest.raises(FarHipError):                                                   # Cin = 48
        ops.conv_valid_dgrad(dy, torch.randn(192, 48, 5, 5, device='cuda'))
    with pytest.raises(FarHipError):
        ops.conv_valid_wgrad(torch.randn(2, 9, 9, 48, device='cuda'), dy)
    with pytest.raises(FarHipError):
        ops.conv_valid_train(torch.randn(2, 9, 9, 48, device='cuda'), torch.randn(192, 48, 5, 5, device='cuda'), cache, 'c48')
    with pytest.raises(FarHipError):                                                   # a 3x3 weight
        ops.conv_valid_dgrad(dy, torch.randn(192, 32, 3, 3, device='cuda'))
    with pytest.raises(FarHipError):
        ops.conv_valid_train(x, torch.randn(192, 32, 3, 3, device='cuda'), cache, 'k3')
    with pytest.raises(FarHipError):                                                   # H = 4
        ops.conv_valid_wgrad(torch.randn(2, 4, 9, 32, device='cuda'), torch.randn(2, 0, 5, 192, device='cuda'))
    with pytest.raises(FarHipError):
        ops.conv_valid_train(torch.randn(2, 4, 9, 32, device='cuda'), w, cache, 'h4')
    with pytest.raises(FarHipError):                                                   # CPU tensors: no eager fallback
        ops.conv_valid_dgrad(dy.cpu(), w)
    with pytest.raises(FarHipError):
        ops.conv_valid_dgrad(dy, w.cpu())
    with pytest.raises(FarHipError):
        ops.conv_valid_wgrad(x.cpu(), dy.cpu())
    with pytest.raises(FarHipError):
        ops.conv_valid_train(x.cpu(), w.cpu(), cache, 'cpu')
    for bad in ((2, 5, 4, 192), (2, 6, 5, 192), (1, 5, 5, 192), (2, 5, 5, 100)):       # dy that is not (N, H - 4, W - 4, Cout)
        with pytest.raises(FarHipError):
            ops.conv_valid_wgrad(x, torch.randn(*bad, device='cuda'))
    with pytest.raises(FarHipError):
        ops.conv_valid_dgrad(torch.randn(2, 5, 5, 160, device='cuda'), w)
    with pytest.raises(FarHipError):
        ops.conv_valid_dgrad(dy, ops.PackedConvValid(w))                               # a forward image is no dgrad image


def test_wgrad_range_guard():
    from far_amd import ops
    x, w, dy, _, dw64, _, _ = _case(3, 9, 11, 32)
    x = x.clone()
    ops.overflow_flag('cuda').zero_()
    ops.conv_valid_wgrad(x, dy)
    assert not ops.activation_overflowed('cuda')
    x[1, 4, 4, 7] = 1.0e5                                                              # beyond 4094 at the default exponent
    dw = ops.conv_valid_wgrad(x, dy)
    assert ops.activation_overflowed('cuda') and not torch.isfinite(dw).all()
    with ops.activation_exponent(-4):                                                  # 16 x the range: the same input passes
        dw = ops.conv_valid_wgrad(x, dy)
    assert not ops.activation_overflowed('cuda') and torch.isfinite(dw).all()
    r64 = _autograd(x, w, dy, torch.float64)[1]
    assert float((dw.double() - r64).abs().max()) <= 1e-5 * float(r64.abs().max())
