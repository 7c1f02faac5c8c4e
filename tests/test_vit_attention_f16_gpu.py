"""K23 on plain fp16 operands (far_vit_attention_f16; ops.vit_attention / ops.vit_attention_planes with plain16=True) on the GPU.

Not a parity kernel: it is narrower than the reference.  Two bars.

Derived bar, against the kernel's own definition.  The operands are rounded as the kernel rounds them, x^ = fp16(x 2^act_exp) 2^-act_exp,
and the float64 composition (tests/vit8pt_ref.py: attention_ref) of the ROUNDED operands is the reference: max|out - ref| <=
2^-10 max|v^|.  The scores and the row sum are fp32 on exact products of the rounded operands; the only further rounding is fp16(p),
relative 2^-11 per term, so |d out| <= sum|dp||v| / sum p <= 2^-11 max|v|; the factor 2 covers the fp32 accumulation.  Every shape in
three regimes (tests/test_vit_attention_gpu.py): flat, peaked, shifted (the last key is the maximum).  The kernel's key tile is 64,
as K23's: the shapes with S = 65 and S = 129 are the one-key-past-a-full-tile cases.

Class bar, the project's own for plain-fp16 kernels (tests/test_attn_block_gpu.py, tests/test_emm_gpu.py), against float64 of the
UNROUNDED inputs: es < e < 3e-3 with e = max|out - ref64| / max|ref64| and es the split kernel's figure in the same run, and the
result differs from the split result -- asserted for every shape in all three regimes.  (Rounding q and k to fp16 moves a score s
by about |s| 2^-11 sqrt(2 / 64) and its probability by that factor's exponential, so the figure grows with the score scale: the
peaked regime, scores of scale 9, is the one nearest the bar.)  Every measured figure is printed ('[parity] ...'; profiles/vit8pt_fp16_parity.txt records a run)."""
import pytest
import torch

from tests.test_vit_attention_gpu import REGIMES, _inputs
from tests.vit8pt_ref import attention_ref

pytestmark = pytest.mark.gpu
SHAPES = [(2, 1, 1, 3), (2, 33, 40, 3), (2, 130, 65, 3), (2, 64, 129, 3), (2, 40, 576, 1), (2, 576, 576, 3)]
ACT_EXP = 4                                                                   # the default activation exponent


def _rounded(x, act_exp=ACT_EXP):
    """fp16(x 2^act_exp) 2^-act_exp, exactly as the kernel forms its operands (round to nearest even)."""
    return (x * 2.0 ** act_exp).half().float() * 2.0 ** -act_exp


@pytest.mark.parametrize('Z,L,S,H', SHAPES)
def test_derived_and_class_bars(Z, L, S, H):
    from far_amd import ops
    assert ops.activation_exponent_value() == ACT_EXP
    for i, regime in enumerate(REGIMES):
        name = f'vit attention f16 {regime} Z{Z} L{L} S{S} H{H}'
        q, k, v = _inputs(Z, L, S, H, regime, seed=7 * L + S + i)
        ops.overflow_flag('cuda').zero_()
        out = ops.vit_attention(q, k, v, H, plain16=True)
        outs = ops.vit_attention(q, k, v, H)
        assert not ops.activation_overflowed('cuda'), name
        assert out.shape == (Z, L, H * 64) and torch.isfinite(out).all(), name
        vr = _rounded(v)
        ref = attention_ref(_rounded(q), _rounded(k), vr, H, torch.float64)
        d, bar = float((out.double() - ref).abs().max()), 2.0 ** -10 * float(vr.abs().max())
        r64 = attention_ref(q, k, v, H, torch.float64)
        sc = float(r64.abs().max())
        e, es = float((out.double() - r64).abs().max()) / sc, float((outs.double() - r64).abs().max()) / sc
        print(f'[parity] {name}: kernel-vs-float64-of-rounded-operands {d:.3e}  bar 2^-10 max|v^| {bar:.3e}  ratio {d / bar:.3f};  '
              f'class: plain vs float64 {e:.3e}  split {es:.3e}  bar 3e-3')
        assert d <= bar, name
        assert not torch.equal(out, outs), name
        assert es < e < 3e-3, name


def test_planes_layout_is_the_same_kernel():
    from far_amd import ops
    H, Z, N = 3, 2, 200
    planes = torch.randn(3 * H, Z, N, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2)) * 1.5
    cat = lambda p: p.permute(1, 2, 0, 3).reshape(Z, N, H * 64).contiguous()
    q, k, v = cat(planes[:H]), cat(planes[H:2 * H]), cat(planes[2 * H:])
    out = ops.vit_attention_planes(planes, H, plain16=True)
    assert out.shape == (Z, N, H * 64) and torch.equal(out, ops.vit_attention(q, k, v, H, plain16=True))
    assert not torch.equal(out, ops.vit_attention_planes(planes, H))


def test_image_bits_do_not_depend_on_the_batch():
    from far_amd import ops
    for L, S in ((576, 576), (130, 65)):
        q, k, v = _inputs(5, L, S, 3, 'peaked', seed=L)
        out5 = ops.vit_attention(q, k, v, 3, plain16=True)
        for z in (0, 4):
            assert torch.equal(ops.vit_attention(q[z:z + 1], k[z:z + 1], v[z:z + 1], 3, plain16=True), out5[z:z + 1]), (L, S, z)
    # Z * H a multiple of 8 takes the other block -> (image, head, row block) map: image 0 still has the bits it has alone
    q, k, v = _inputs(8, 576, 576, 3, 'peaked', seed=1)
    assert torch.equal(ops.vit_attention(q, k, v, 3, plain16=True)[:1], ops.vit_attention(q[:1], k[:1], v[:1], 3, plain16=True))


def test_ten_launches_are_bit_identical_alone_and_next_to_a_busy_stream():
    """(576, 576) at Z = 8: 10 launches bit-identical to the first, alone, and again while a second stream runs a loop of large K9
    Linear launches (the construction of tests/test_vit_attention_gpu.py)."""
    from far_amd import ops
    q, k, v = _inputs(8, 576, 576, 3, 'peaked', seed=5)
    first = ops.vit_attention(q, k, v, 3, plain16=True).clone()
    for it in range(10):
        assert torch.equal(ops.vit_attention(q, k, v, 3, plain16=True), first), f'alone, launch {it}'
    g = torch.Generator(device='cuda').manual_seed(6)
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
        assert torch.equal(ops.vit_attention(q, k, v, 3, plain16=True), first), f'next to the busy stream, launch {it}'
    side.synchronize()
    torch.cuda.synchronize()


def test_overflow_flag():
    from far_amd import ops
    q, k, v = _inputs(2, 100, 100, 3, 'flat', seed=9)
    for which in range(3):
        t = [q.clone(), k.clone(), v.clone()]
        t[which][1, 17, 70] = 1.0e5                                       # beyond 65504 / 2^4
        ops.overflow_flag('cuda').zero_()
        ops.vit_attention(*t, 3, plain16=True)
        assert ops.activation_overflowed('cuda'), which
    ops.overflow_flag('cuda').zero_()
    ops.vit_attention(q, k, v, 3, plain16=True)
    assert not ops.activation_overflowed('cuda')
    with ops.activation_exponent(-4):                                     # 256 x the range: 1e5 is an ordinary value
        t = v.clone()
        t[1, 17, 70] = 1.0e5
        out = ops.vit_attention(q, k, t, 3, plain16=True)
        assert not ops.activation_overflowed('cuda') and torch.isfinite(out).all()


def test_refusals_and_empty_batch():
    from far_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1, 40, 96, device='cuda')
    with pytest.raises(_lib.FarHipError, match='64'):                     # head dim 32 belongs to K22
        ops.vit_attention(x, x, x, 3, plain16=True)
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention_planes(torch.zeros(9, 1, 40, 32, device='cuda'), 3, plain16=True)
    out = torch.zeros(1, 40, 96, device='cuda')
    rc = lib.far_vit_attention_f16(x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 40, 40, 3, 32, 40 * 96, 32, 96, 40 * 96, 32, 96, 4,
                                   out.data_ptr(), None, None)
    assert rc == -22
    y = torch.zeros(1, 40, 192, device='cuda')
    assert lib.far_vit_attention_f16(y.data_ptr(), y.data_ptr(), y.data_ptr(), 0, 40, 40, 3, 64, 40 * 192, 64, 192, 40 * 192, 64, 192, 4,
                                     y.data_ptr(), None, None) == 0        # Z = 0 returns at once
    z = torch.zeros(0, 40, 192, device='cuda')
    assert ops.vit_attention(z, z, z, 3, plain16=True).shape == (0, 40, 192)


def test_inputs_that_need_gradients_raise():
    from far_amd import ops
    q, k, v = _inputs(1, 40, 40, 3, 'flat')
    for i in range(3):
        t = [q, k, v]
        t[i] = t[i].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=r'far_vit_attention_f16\)'):
            ops.vit_attention(*t, 3, plain16=True)
    planes = torch.zeros(9, 1, 40, 64, device='cuda', requires_grad=True)
    with pytest.raises(NotImplementedError, match=r'far_vit_attention_f16\)'):
        ops.vit_attention_planes(planes, 3, plain16=True)
    with torch.no_grad():                                                 # no graph is recorded: the inference call it is
        assert ops.vit_attention(q.clone().requires_grad_(True), k, v, 3, plain16=True).shape == q.shape
