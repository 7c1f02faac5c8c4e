"""K23 (far_vit_attention_f16s, ops.vit_attention / ops.vit_attention_planes): the head-dim-64 softmax self-attention of the
8-Point-ViT's Blocks on the GPU, against the float64 torch composition (tests/vit8pt_ref.py: attention_ref).

Parity rule, the project's one for split-fp16 attention (tests/test_full_attention_gpu.py: _bar): the kernel's maximum deviation from
float64 is at most max(3 x dev32, 2^-20 max|out|), dev32 being the fp32 torch composition's own deviation from float64 on the same
inputs, computed next to it in the same run.  Every measured pair is printed ('[parity] ...'; profiles/vit8pt_parity.txt records a
run).  Regimes: flat (randn q, k), peaked (q, k x 3: rows rescale after the first tile), shifted (the maximum-score key is the LAST
key, so every row rescales in the last tile)."""
import pytest
import torch

from tests.test_full_attention_gpu import _bar
from tests.vit8pt_ref import attention_ref

pytestmark = pytest.mark.gpu
REGIMES = ('flat', 'peaked', 'shifted')


def _inputs(Z, L, S, H, regime, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    C = H * 64
    q = torch.randn(Z, L, C, device='cuda', generator=g)
    k = torch.randn(Z, S, C, device='cuda', generator=g)
    v = torch.randn(Z, S, C, device='cuda', generator=g)
    if regime == 'peaked':
        q, k = 3 * q, 3 * k
    elif regime == 'shifted':
        u = torch.randn(C, device='cuda', generator=g)          # |u_head|^2 ~ 64: q . k_last / 8 ~ 48 against N(0, ~1.4) elsewhere
        q = q + u
        k[:, -1] = 6 * u
    return q, k, v


def _parity(name, q, k, v, H):
    from far_amd import ops
    ops.overflow_flag('cuda').zero_()
    out = ops.vit_attention(q, k, v, H)
    assert not ops.activation_overflowed('cuda'), name
    r64 = attention_ref(q, k, v, H, torch.float64)
    r32 = attention_ref(q, k, v, H, torch.float32)
    _bar(name, out, r64, float((r32.double() - r64).abs().max()))
    return out


@pytest.mark.parametrize('Z,L,S,H', [(2, 576, 576, 3), (2, 1, 1, 3), (2, 33, 40, 3), (2, 130, 65, 3), (2, 64, 129, 3), (2, 40, 576, 1)])
def test_operator_against_float64(Z, L, S, H):
    """The production shape; one query and one key; one partial key tile; a query tail across a workgroup boundary with a one-key
    tail tile; two full tiles and a one-key third; one head."""
    for i, regime in enumerate(REGIMES):
        _parity(f'vit attention {regime} Z{Z} L{L} S{S} H{H}', *_inputs(Z, L, S, H, regime, seed=7 * L + S + i), H)


def test_planes_layout_is_the_same_kernel():
    """The head planes the qkv Linear writes (3h, Z, N, 64) and the concatenated form give the same bits (strides only differ)."""
    from far_amd import ops
    H, Z, N = 3, 2, 200
    planes = torch.randn(3 * H, Z, N, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2)) * 1.5
    cat = lambda p: p.permute(1, 2, 0, 3).reshape(Z, N, H * 64).contiguous()
    q, k, v = cat(planes[:H]), cat(planes[H:2 * H]), cat(planes[2 * H:])
    out = ops.vit_attention_planes(planes, H)
    assert out.shape == (Z, N, H * 64) and torch.equal(out, ops.vit_attention(q, k, v, H))
    r64 = attention_ref(q, k, v, H, torch.float64)
    r32 = attention_ref(q, k, v, H, torch.float32)
    _bar('vit attention planes Z2 N200 H3', out, r64, float((r32.double() - r64).abs().max()))


def test_image_bits_do_not_depend_on_the_batch():
    from far_amd import ops
    for L, S in ((576, 576), (130, 65)):
        q, k, v = _inputs(5, L, S, 3, 'peaked', seed=L)
        out5 = ops.vit_attention(q, k, v, 3)
        for z in (0, 4):
            assert torch.equal(ops.vit_attention(q[z:z + 1], k[z:z + 1], v[z:z + 1], 3), out5[z:z + 1]), (L, S, z)
    # Z * H a multiple of 8 takes the other block -> (image, head, row block) map: image 0 still has the bits it has alone
    q, k, v = _inputs(8, 576, 576, 3, 'peaked', seed=1)
    assert torch.equal(ops.vit_attention(q, k, v, 3)[:1], ops.vit_attention(q[:1], k[:1], v[:1], 3))


def test_ten_launches_are_bit_identical_alone_and_next_to_a_busy_stream():
    """(576, 576) at Z = 8: 10 launches bit-identical to the first, alone, and again while a second stream runs a loop of large K9
    Linear launches (waves of another kernel share the CUs)."""
    from far_amd import ops
    q, k, v = _inputs(8, 576, 576, 3, 'peaked', seed=5)
    first = ops.vit_attention(q, k, v, 3).clone()
    for it in range(10):
        assert torch.equal(ops.vit_attention(q, k, v, 3), first), f'alone, launch {it}'
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
        assert torch.equal(ops.vit_attention(q, k, v, 3), first), f'next to the busy stream, launch {it}'
    side.synchronize()
    torch.cuda.synchronize()


def test_overflow_flag():
    from far_amd import ops
    q, k, v = _inputs(2, 100, 100, 3, 'flat', seed=9)
    for which in range(3):
        t = [q.clone(), k.clone(), v.clone()]
        t[which][1, 17, 70] = 1.0e5                                       # beyond 65504 / 2^4
        ops.overflow_flag('cuda').zero_()
        ops.vit_attention(*t, 3)
        assert ops.activation_overflowed('cuda'), which
    ops.overflow_flag('cuda').zero_()
    ops.vit_attention(q, k, v, 3)
    assert not ops.activation_overflowed('cuda')
    with ops.activation_exponent(-4):                                     # 256 x the range: 1e5 is an ordinary value
        t = v.clone()
        t[1, 17, 70] = 1.0e5
        out = ops.vit_attention(q, k, t, 3)
        assert not ops.activation_overflowed('cuda') and torch.isfinite(out).all()


def test_refusals():
    from far_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1, 40, 96, device='cuda')
    with pytest.raises(_lib.FarHipError, match='64'):                     # head dim 32 belongs to K22
        ops.vit_attention(x, x, x, 3)
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention_planes(torch.zeros(9, 1, 40, 32, device='cuda'), 3)
    out = torch.zeros(1, 40, 96, device='cuda')
    rc = lib.far_vit_attention_f16s(x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 40, 40, 3, 32, 40 * 96, 32, 96, 40 * 96, 32, 96, 4,
                                    out.data_ptr(), None, None)
    assert rc == -22
    y = torch.zeros(1, 40, 192, device='cuda')
    with pytest.raises(_lib.FarHipError):                                 # ... and K22 keeps refusing head dim 64
        ops.full_attention(y, y, y, 3)
    rc = lib.far_full_attention_f16s(y.data_ptr(), y.data_ptr(), y.data_ptr(), 1, 40, 40, 3, 64, None, None, 4, y.data_ptr(), None, None, None)
    assert rc == -22
    z = torch.zeros(0, 40, 192, device='cuda')
    assert ops.vit_attention(z, z, z, 3).shape == (0, 40, 192)
    c = torch.zeros(1, 40, 192)
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention(c, c, c, 3)


def test_inputs_that_need_gradients_raise():
    from far_amd import ops
    q, k, v = _inputs(1, 40, 40, 3, 'flat')
    for i in range(3):
        t = [q, k, v]
        t[i] = t[i].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match='far_vit_attention_f16s'):
            ops.vit_attention(*t, 3)
    planes = torch.zeros(9, 1, 40, 64, device='cuda', requires_grad=True)
    with pytest.raises(NotImplementedError, match='K23'):
        ops.vit_attention_planes(planes, 3)
    with torch.no_grad():                                                 # no graph is recorded: the inference call it is
        assert ops.vit_attention(q.clone().requires_grad_(True), k, v, 3).shape == q.shape
