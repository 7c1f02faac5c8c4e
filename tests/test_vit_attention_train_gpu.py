"""Training through K23 (far_vit_attention_train_f16s / far_vit_attention_bwd_f16s; ops.vit_attention_train, vit_attention_train_qkv,
vit_attention_bwd) on the GPU.

Reference of every gradient: float64 torch autograd of the definition (tests/vit8pt_ref.py: attention_ref, differentiable as
written).  dev32 is the same definition differentiated in fp32 on the GPU.
Bars: `out` has the bits of ops.vit_attention; the row statistic lse2 is within the project's parity rule
(tests/test_full_attention_gpu.py: _bar, max(3 dev32, 2^-20 max|ref|)) of the float64 log2-sum-exp, dev32 being the fp32 torch
log-sum-exp's own deviation; each of dq, dk, dv has a relative Frobenius error of at most max(1e-3, dev32) -- the project's class for
backward kernels with 16-bit operands, the bar of tests/test_full_attention_train_gpu.py.
Inputs: q, k ~ amp N(0, 1), v, g ~ N(0, 1) from one seeded numpy generator; amp = 1, 2, 2.94 take the softmax from flat to near
one-hot (max |score| ~ 6, 22, 48).  Shapes: the kernels own 128 rows per workgroup and walk tiles of 64 -- the forward's boundaries --
so the forward test's shapes cross every boundary of both backward kernels (130 and 129 owned rows: a workgroup boundary with a
short tail; 65, 129, 130 walked rows: a one- or two-row tail tile).
Every measured value is printed ('[vit train parity] ...'; profiles/vit8pt_train_parity.txt records a run)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_full_attention_gpu import _bar
from tests.test_vit_attention_gpu import REGIMES, _inputs
from tests.vit8pt_ref import attention_ref

pytestmark = pytest.mark.gpu
GRAD_BAR = 1e-3

# (Z, L, S, amp, H): each shape is the smallest that reaches its code path
CASES = {
    'one': (2, 1, 1, 1.0, 3),                # dq = dk = 0: the comparison falls back to the absolute difference
    'partial': (2, 33, 40, 2.94, 3),         # one partial tile on both sides
    'tails': (2, 130, 65, 2.94, 3),          # an owned-row tail across a workgroup boundary, a one-row tail tile
    'three': (2, 64, 129, 1.0, 3),           # two full tiles and a one-row third
    'short-q': (2, 40, 576, 2.0, 3),         # a short owned side for the dq kernel
    'short-k': (2, 576, 40, 2.0, 3),         # ... and for the dk / dv kernel
    'production': (2, 576, 576, 2.94, 3),
    'one-head': (2, 130, 65, 2.0, 1),
    'xcd-map': (8, 130, 65, 2.0, 3),         # Z H a multiple of 8: the other branch of the block map
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    Z, L, S, amp, H = CASES[name]
    rng = np.random.default_rng(2300 + list(CASES).index(name))
    C = H * 64
    q = (amp * rng.standard_normal((Z, L, C))).astype(np.float32)
    k = (amp * rng.standard_normal((Z, S, C))).astype(np.float32)
    v = rng.standard_normal((Z, S, C)).astype(np.float32)
    g = rng.standard_normal((Z, L, C)).astype(np.float32)
    return tuple(torch.from_numpy(a).cuda() for a in (q, k, v, g)) + (H,)


def rel(got, ref):
    n = float(ref.double().norm())
    d = float((got.double() - ref.double()).norm())
    return d / n if n > 0 else d


def def_grads(q, k, v, g, H, dtype):
    Q, K, V = (t.to(dtype).clone().requires_grad_() for t in (q, k, v))
    out = attention_ref(Q, K, V, H, dtype)
    return (out.detach(),) + torch.autograd.grad(out, (Q, K, V), g.to(dtype))


def lse2_ref(q, k, H, dtype):
    """log2 sum_s 2^(log2(e) q . k / 8) per (image, head, row) in `dtype` -> (Z, H, L)."""
    Z, L, C = q.shape
    qh = q.to(dtype).view(Z, L, H, 64).permute(0, 2, 1, 3)
    kh = k.to(dtype).view(Z, k.shape[1], H, 64).permute(0, 2, 1, 3)
    return torch.logsumexp(qh @ kh.transpose(-2, -1) / 8, dim=-1) / math.log(2.0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 (out, dq, dk, dv) and the fp32 definition's own relative Frobenius deviations, computed once and left unchanged."""
    q, k, v, g, H = inputs(name)
    r64 = def_grads(q, k, v, g, H, torch.float64)
    r32 = def_grads(q, k, v, g, H, torch.float32)
    return r64, tuple(rel(a, b) for a, b in zip(r32[1:], r64[1:]))


def kernel_grads(q, k, v, g, H):
    from far_amd import ops
    Q, K, V = (t.clone().requires_grad_() for t in (q, k, v))
    out = ops.vit_attention_train(Q, K, V, H)
    return (out.detach(),) + torch.autograd.grad(out, (Q, K, V), g)


def compare(name, got, ref, dev):
    errs = []
    for nm, a, b, d32 in zip(('dq', 'dk', 'dv'), got, ref, dev):
        e = rel(a, b)
        bar = max(GRAD_BAR, d32)
        print(f'[vit train parity] {name} {nm}: rel Frobenius {e:.3e}  dev32 {d32:.3e}  |ref| {float(b.norm()):.1f}  bar {bar:.1e}')
        errs.append((nm, e, bar))
    for nm, e, bar in errs:
        assert np.isfinite(e) and e <= bar, (name, nm, e, bar)
    return [e for _, e, _ in errs]


def check_lse(name, q, k, v, H):
    """The raw training forward's row statistic against the float64 log2-sum-exp -> out."""
    from far_amd.ops import attention as at
    Z, L, S = q.shape[0], q.shape[1], k.shape[1]
    out, lse, _ = at._vit_train_forward(q, k, v, Z, L, S, H)
    r64 = lse2_ref(q, k, H, torch.float64)
    r32 = lse2_ref(q, k, H, torch.float32)
    d = _bar(f'lse2 {name}', lse, r64, float((r32.double() - r64).abs().max()))
    print(f'[vit train parity] {name} lse2: max |kernel - float64| {d:.3e}  max|ref| {float(r64.abs().max()):.2f}')
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_forward_statistic_and_gradients(name):
    from far_amd import ops
    q, k, v, g, H = inputs(name)
    r64, dev = reference(name)
    ops.overflow_flag('cuda').zero_()
    out, dq, dk, dv = kernel_grads(q, k, v, g, H)
    raw = check_lse(name, q, k, v, H)
    assert not ops.activation_overflowed('cuda')
    inference = ops.vit_attention(q, k, v, H)
    assert torch.equal(out, inference) and torch.equal(raw, inference)     # the training forward is the inference kernel's bits
    compare(name, (dq, dk, dv), r64[1:], dev)


@pytest.mark.parametrize('Z,L,S,H', [(2, 576, 576, 3), (2, 130, 65, 3)])
def test_statistic_on_the_forward_tests_regimes(Z, L, S, H):
    """flat, peaked, shifted (every row rescales in the LAST tile): the statistic follows the late rescale."""
    for i, regime in enumerate(REGIMES):
        q, k, v = _inputs(Z, L, S, H, regime, seed=7 * L + S + i)
        check_lse(f'{regime} Z{Z} L{L} S{S}', q, k, v, H)


def test_qkv_form_has_the_bits_of_the_three_slices():
    from far_amd import ops
    H, C = 3, 192
    for Z, N in ((2, 130), (2, 576)):
        gen = torch.Generator(device='cuda').manual_seed(N)
        qkv = torch.randn(Z, N, 3 * C, device='cuda', generator=gen) * 1.5
        g = torch.randn(Z, N, C, device='cuda', generator=gen)
        X = qkv.clone().requires_grad_()
        out = ops.vit_attention_train_qkv(X, H)
        (dqkv,) = torch.autograd.grad(out, X, g)
        assert dqkv.shape == qkv.shape and dqkv.is_contiguous()
        q, k, v = (qkv[..., t * C:(t + 1) * C].contiguous() for t in range(3))
        o2, dq, dk, dv = kernel_grads(q, k, v, g, H)
        assert torch.equal(out.detach(), o2)
        for t, d in enumerate((dq, dk, dv)):
            assert torch.equal(dqkv[..., t * C:(t + 1) * C], d), (N, t)
        # the reference's layout: reshape(B, N, 3, H, 64)
        r = qkv.double().reshape(Z, N, 3, H, 64)
        want = attention_ref(r[:, :, 0].reshape(Z, N, C), r[:, :, 1].reshape(Z, N, C), r[:, :, 2].reshape(Z, N, C), H)
        assert float((out.detach().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())


@pytest.mark.parametrize('log2_scale', [-20, 10])
def test_gradient_scale(log2_scale):
    """Upstream gradients scaled by 2^k: the same relative error -- g and ds are normalised by powers of two taken from the image's
    max |g| on the device (the assertion of tests/test_full_attention_train_gpu.py: test_gradient_scale)."""
    q, k, v, g, H = inputs('tails')
    r64, dev = reference('tails')
    e0 = compare('scale 2^0', kernel_grads(q, k, v, g, H)[1:], r64[1:], dev)
    sc = 2.0 ** log2_scale
    got = tuple(t / sc for t in kernel_grads(q, k, v, g * sc, H)[1:])
    ek = compare(f'scale 2^{log2_scale}', got, r64[1:], dev)
    for a, b in zip(e0, ek):
        assert abs(a - b) <= 0.05 * a + 1e-9, (e0, ek)


@pytest.mark.parametrize('name', ['tails', 'production'])
def test_determinism_and_batch_independence(name):
    q, k, v, g, H = inputs(name)
    first = kernel_grads(q, k, v, g, H)
    for _ in range(4):
        for a, b in zip(first, kernel_grads(q, k, v, g, H)):
            assert torch.equal(a, b)
    for n in range(2):                                                        # an image alone = the image inside the batch
        alone = kernel_grads(q[n:n + 1], k[n:n + 1], v[n:n + 1], g[n:n + 1], H)
        for a, b in zip(first, alone):
            assert torch.equal(a[n:n + 1], b), (name, n)


def test_memory_stays_below_one_score_tensor():
    from far_amd import ops
    Z, L, S, H = 2, 1200, 1200, 3
    gen = torch.Generator(device='cuda').manual_seed(3)
    q, k, v, g = (torch.randn(Z, n, H * 64, device='cuda', generator=gen) for n in (L, S, S, L))
    q.requires_grad_(); k.requires_grad_(); v.requires_grad_()
    ops.vit_attention_train(q, k, v, H).backward(g)                           # warm: the flag, workspaces of the allocator
    q.grad = k.grad = v.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ops.vit_attention_train(q, k, v, H).backward(g)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    scores = Z * H * L * S * 4
    print(f'[vit train parity] memory: forward + backward peak {used / 2**20:.1f} MiB; one (Z, H, L, S) fp32 score tensor '
          f'{scores / 2**20:.1f} MiB')
    assert used < scores


def test_edge_cases():
    from far_amd import _lib, ops
    for shape_q, shape_k in (((0, 40, 192), (0, 50, 192)), ((2, 0, 192), (2, 50, 192)), ((2, 40, 192), (2, 0, 192))):
        q = torch.randn(*shape_q, device='cuda').requires_grad_()
        k = torch.randn(*shape_k, device='cuda').requires_grad_()
        v = torch.randn(*shape_k, device='cuda').requires_grad_()
        out = ops.vit_attention_train(q, k, v, 3)
        assert out.shape == shape_q and bool((out == 0).all())
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), torch.ones_like(out))
        assert dq.shape == shape_q and dk.shape == shape_k and dv.shape == shape_k
        assert bool((dq == 0).all()) and bool((dk == 0).all()) and bool((dv == 0).all())
    for shape in ((0, 40, 576), (2, 0, 576)):
        x = torch.randn(*shape, device='cuda').requires_grad_()
        out = ops.vit_attention_train_qkv(x, 3)
        assert out.shape == (shape[0], shape[1], 192)
        (dx,) = torch.autograd.grad(out, x, torch.ones_like(out))
        assert dx.shape == shape and bool((dx == 0).all())
    x = torch.zeros(1, 40, 96, device='cuda', requires_grad=True)             # head dim 32 belongs to K22
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention_train(x, x, x, 3)
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention_train_qkv(torch.zeros(1, 40, 288, device='cuda', requires_grad=True), 3)
    lib = _lib.load()
    y = torch.zeros(1, 40, 96, device='cuda')
    rc = lib.far_vit_attention_bwd_f16s(*[y.data_ptr()] * 6, 1, 40, 40, 3, 32, 40 * 96, 32, 96, 40 * 96, 32, 96, 4, *[y.data_ptr()] * 3,
                                        40 * 96, 32, 96, 40 * 96, 32, 96, y.data_ptr(), None, None)
    assert rc == -22
    q, k, v, g, H = inputs('tails')
    for which in range(3):                                                    # beyond 65504 / 2^4: forward and backward flag it
        t = [q.clone(), k.clone(), v.clone()]
        t[which][1, 17, 70] = 1.0e5
        Q, K, V = (a.requires_grad_() for a in t)
        ops.overflow_flag('cuda').zero_()
        out = ops.vit_attention_train(Q, K, V, H)
        assert ops.activation_overflowed('cuda'), which
        ops.overflow_flag('cuda').zero_()
        out.backward(g)
        assert ops.activation_overflowed('cuda'), which
    ops.overflow_flag('cuda').zero_()
    gn = g.clone()
    gn[0, 3, 5] = float('inf')                                                # a non-finite gradient
    kernel_grads(q, k, v, gn, H)
    assert ops.activation_overflowed('cuda')
    ops.overflow_flag('cuda').zero_()
    with pytest.raises(NotImplementedError, match='far_vit_attention_f16s'):  # the inference front end stays an inference front end
        ops.vit_attention(q.clone().requires_grad_(), k, v, H)
