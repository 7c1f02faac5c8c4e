"""K24 on plain fp16 operands (far_conv_valid_f16; ops.conv_valid with a PackedConvValid(split=False)) on the GPU.

Not a parity kernel: it is narrower than the reference.  Two bars.

Sharp bar, against the kernel's own definition.  The operands are rounded as the kernel rounds them -- x^ = fp16(x 2^act_exp) 2^-act_exp,
w^ = fp16(w s) / s with s = pack.pack_scale[0], the power of two the pack chose -- and the reference is the float64 conv2d(x^, w^) with
the epilogue.  Products of two fp16 values are exact in fp32, so only the order of the fp32 accumulation is left to differ: the bar is
the project's parity rule (tests/test_full_attention_gpu.py: _bar), max(3 x dev32, 2^-20 max|out|), dev32 being fp32 torch conv2d on
the SAME rounded operands against float64 in the same run.  An indexing slip cannot hide under a 16-bit tolerance.

Class bar, the project's own for plain-fp16 kernels (tests/test_attn_block_gpu.py, tests/test_emm_gpu.py), against float64 of the
UNROUNDED operands: es < e < 3e-3 of the output scale, es the split kernel's figure in the same run, and the result differs from the
split result.

Every shape with and without residual + ReLU (the second with a folded BatchNorm).  Every measured figure is printed ('[parity] ...';
profiles/vit8pt_fp16_parity.txt records a run)."""
import pytest
import torch

from tests.test_extractor_kernels_gpu import _bn, _conv_ref, _gen
from tests.test_full_attention_gpu import _bar

pytestmark = pytest.mark.gpu
ACT_EXP = 4
SHAPES = [(1, 5, 5, 32, 32),          # one output pixel
          (3, 13, 9, 64, 96),         # tile tails in both axes
          (2, 28, 28, 128, 192),      # production, the 8-row form
          (2, 28, 28, 192, 192),
          (2, 12, 20, 32, 224),       # an N-tile tail beyond one workgroup's six tiles
          (64, 28, 28, 128, 192)]     # the 24-row form
_CACHE = {}


def _rounded(x, act_exp=ACT_EXP):
    return (x * 2.0 ** act_exp).half().float() * 2.0 ** -act_exp


def _case(shape):
    """Seeded operands of one shape, the plain and split packs (bare, and with BN fold for the residual + ReLU form) and the three
    bare convolutions every check of the shape shares: float64 and fp32 of the rounded operands, float64 of the unrounded ones."""
    if shape not in _CACHE:
        from far_amd import ops
        N, H, W, cin, cout = shape
        g = _gen(1000 * H + 10 * cin + cout + N)
        x = torch.randn(N, H, W, cin, device='cuda', generator=g) * 3
        w = torch.randn(cout, cin, 5, 5, device='cuda', generator=g) * (2.0 / (25 * cin)) ** 0.5
        scale, shift = _bn(cout, g)
        res = torch.randn(N, H - 4, W - 4, cout, device='cuda', generator=g)
        c = dict(x=x, w=w, scale=scale, shift=shift, res=res)
        for split in (False, True):
            c['bare', split] = ops.PackedConvValid(w, split=split)
            c['full', split] = ops.PackedConvValid(w, scale, shift, split=split)
        s = c['bare', False].pack_scale[0]
        assert torch.equal(c['full', False].pack_scale, c['bare', False].pack_scale)
        xr, wr = _rounded(x), (w * s).half().float() / s
        c['r64'] = _conv_ref(xr, wr, None, None, None, None, False, torch.float64)
        c['r32'] = _conv_ref(xr, wr, None, None, None, None, False, torch.float32)
        c['u64'] = _conv_ref(x, w, None, None, None, None, False, torch.float64)
        _CACHE.clear()                                                    # one shape's tensors at a time
        _CACHE[shape] = c
    return _CACHE[shape]


def _epilogue(y, c, full):
    if not full:
        return y
    return torch.relu(y * c['scale'].to(y.dtype) + c['shift'].to(y.dtype) + c['res'].to(y.dtype))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sharp_and_class_bars(shape):
    from far_amd import ops
    assert ops.activation_exponent_value() == ACT_EXP
    c = _case(shape)
    N, H, W, cin, cout = shape
    for full in (False, True):
        what = 'BN + residual + ReLU' if full else 'bare'
        name = f'conv_valid f16 {cin}->{cout} @ {H}x{W} N{N} {what}'
        kw = dict(residual=c['res'], act='relu') if full else {}
        ops.overflow_flag('cuda').zero_()
        got = ops.conv_valid(c['x'], c['full' if full else 'bare', False], **kw)
        assert not ops.activation_overflowed('cuda'), name                  # the plain kernel's own launch
        gots = ops.conv_valid(c['x'], c['full' if full else 'bare', True], **kw)
        assert got.shape == (N, H - 4, W - 4, cout)
        r64, r32, u64 = _epilogue(c['r64'], c, full), _epilogue(c['r32'], c, full), _epilogue(c['u64'], c, full)
        _bar(name, got, r64, float((r32.double() - r64).abs().max()))
        sc = float(u64.abs().max())
        e, es = float((got.double() - u64).abs().max()) / sc, float((gots.double() - u64).abs().max()) / sc
        print(f'[parity] {name} class: plain vs float64 {e:.3e}  split {es:.3e}  bar 3e-3')
        assert es < e < 3e-3, name
        assert not torch.equal(got, gots), name
        if full and got.numel() >= 1000:
            assert 0.2 < float((got > 0).float().mean()) < 0.8, name        # the ReLU cuts


def test_both_launch_forms_and_an_image_alone_have_the_same_bits():
    """64 images take the 24-row form (192 workgroups), one or two images the 8-row form: image n has the same bits in all of them."""
    from far_amd import ops
    c = _case(SHAPES[-1])
    x, res, pack = c['x'], c['res'], c['full', False]
    big = ops.conv_valid(x, pack, residual=res, act='relu')
    assert torch.equal(ops.conv_valid(x[:1], pack, residual=res[:1], act='relu'), big[:1])
    for n in (31, 62):
        assert torch.equal(ops.conv_valid(x[n:n + 2], pack, residual=res[n:n + 2], act='relu'), big[n:n + 2]), n


def test_ten_launches_are_bit_identical_next_to_a_busy_stream():
    from far_amd import ops
    c = _case(SHAPES[-1])
    pack = c['full', False]
    cases = [(c['x'], c['res']), (c['x'][:2], c['res'][:2])]                 # the 24-row and the 8-row form
    first = [ops.conv_valid(x, pack, residual=r, act='relu').clone() for x, r in cases]
    g = _gen(6)
    big = torch.randn(1 << 17, 256, device='cuda', generator=g)
    pc = ops.PackedConv(torch.randn(256, 256, device='cuda', generator=g) / 16)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    keep = []
    for it in range(10):
        with torch.cuda.stream(side):
            for _ in range(4):
                keep.append(ops.linear_f16s(big, pc))
            del keep[:-4]
        for (x, r), want in zip(cases, first):
            assert torch.equal(ops.conv_valid(x, pack, residual=r, act='relu'), want), f'launch {it}, {x.shape[0]} images'
    side.synchronize()
    torch.cuda.synchronize()


def test_refresh_repacks_in_place():
    from far_amd import ops
    g = _gen(11)
    w = torch.randn(64, 32, 5, 5, device='cuda', generator=g) * 0.05
    x = torch.randn(2, 9, 11, 32, device='cuda', generator=g)
    pack = ops.PackedConvValid(w.clone(), split=False)
    ptr = pack.packed.data_ptr()
    w2 = 2.5 * torch.randn(64, 32, 5, 5, device='cuda', generator=g)
    assert pack.refresh(w2) is pack and pack.packed.data_ptr() == ptr and pack.packed.numel() == 64 * 32 * 25 * 2
    assert torch.equal(ops.conv_valid(x, pack), ops.conv_valid(x, ops.PackedConvValid(w2, split=False)))


def test_overflow_flag_refusals_and_empty_batch():
    from far_amd import ops
    from far_amd._lib import FarHipError
    g = _gen(7)
    w = torch.randn(192, 32, 5, 5, device='cuda', generator=g) * 0.05
    pack = ops.PackedConvValid(w, split=False)
    x = torch.randn(2, 9, 9, 32, device='cuda', generator=g)
    ops.overflow_flag('cuda').zero_()
    ops.conv_valid(x, pack)
    assert not ops.activation_overflowed('cuda')
    x[1, 4, 4, 7] = 1.0e5                                                              # beyond 4094 at the default exponent
    y = ops.conv_valid(x, pack)
    assert ops.activation_overflowed('cuda')
    assert torch.isfinite(y[0]).all() and not torch.isfinite(y[1]).all()
    ops.overflow_flag('cuda').zero_()
    with ops.activation_exponent(-4):                                                  # 256 x the range: the same input passes
        y = ops.conv_valid(x, pack)
    assert not ops.activation_overflowed('cuda') and torch.isfinite(y).all()
    assert ops.conv_valid(torch.zeros(0, 9, 9, 32, device='cuda'), pack).shape == (0, 5, 5, 192)      # N = 0
    for shape in ((1, 4, 9, 32), (1, 9, 4, 32), (1, 9, 9, 64)):
        with pytest.raises(FarHipError):
            ops.conv_valid(torch.randn(*shape, device='cuda'), pack)
    for bad in (torch.randn(192, 48, 5, 5, device='cuda'), torch.randn(192, 32, 3, 3, device='cuda'), torch.randn(100, 32, 5, 5, device='cuda')):
        with pytest.raises(FarHipError):
            ops.PackedConvValid(bad, split=False)
    with pytest.raises(FarHipError):                                                   # forward only
        ops.PackedConvValid(w, split=False, dgrad=True, pack_scale=pack.pack_scale)
    with pytest.raises(FarHipError):                                                   # ... and the dgrad launch refuses a forward image
        ops.conv_valid_dgrad(torch.zeros(1, 5, 5, 192, device='cuda'), pack)
