"""Training through LoFTR's full softmax attention (K22: far_full_attention_train_f16s / far_full_attention_bwd_f16s) on the GPU.

Reference of every gradient: float64 torch autograd of the definition (linear_attention.py:74-86, restated in `attention_def` under
the kernel's mask convention: masked keys at -inf, padded query rows multiplied to zero, an image without a valid key gives zeros).
dev32 is the same definition differentiated in fp32 on the GPU.
Bars: the forward meets K22's own bar (tests/test_full_attention_gpu.py: _bar); each of dq, dk, dv has a relative Frobenius error
of at most max(1e-3, dev32) -- the project's class for backward kernels with 16-bit operands (tests/test_train_kernels_gpu.py,
tests/test_sinkhorn_train_gpu.py); a CPU simulation of the operand rounding (split-fp16 score recompute and dp, plain-fp16 output
contractions) predicts ~3e-4.  On these inputs dev32 is 2e-7 .. 1.4e-6 and every gradient norm is 46 .. 265.
Every measured value is printed ('[train parity] ...'; profiles/full_attention_train_parity.txt records a run)."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import full_attention_inputs as fa_in
from tests.test_full_attention_gpu import _bar

pytestmark = pytest.mark.gpu
H = fa_in.NHEAD
GRAD_BAR = 1e-3
LAYER_BAR = 3e-3          # the bar tests/test_train_kernels_gpu.py holds K1's backward to inside the model

# each shape is the smallest that reaches its code path
CASES = {
    't1': dict(seed=2201, N=2, L=200, S=150, D=32, amp=1.04),      # several 64-key tiles, ragged last tile, 2 query blocks, no split
    't2': dict(seed=2202, N=2, L=200, S=150, D=32, amp=2.94),      # the same, near one-hot rows (|score| ~ 60)
    't3': dict(seed=2203, N=2, L=100, S=500, D=32, amp=1.5),       # forward plan: nsplit = 2 (statistic from k_combine); short query side
    't4': dict(seed=2204, N=2, L=500, S=100, D=32, amp=1.5),       # short key side for the dq kernel
    't5a': dict(seed=2205, N=6, L=25, S=25, D=16, amp=1.2),        # the <= 32-key one-wave form
    't5b': dict(seed=2206, N=6, L=25, S=25, D=16, amp=2.94),
    't5c': dict(seed=2209, N=2, L=40, S=25, D=16, amp=1.2),        # S <= 32 < L: the forward one-wave, the backward tiled
    't5d': dict(seed=2210, N=2, L=25, S=40, D=16, amp=1.2),        # the mirror: only the short side differs
    't6': dict(seed=2207, N=2, L=200, S=150, D=16, amp=1.5),       # D = 16 on the tiled form
    't7': dict(seed=2208, N=2, L=180, S=150, D=32, amp=1.5, q_valid=(130, 180), kv_valid=(150, 70)),
    't7e': dict(seed=2208, N=2, L=180, S=150, D=32, amp=1.5, q_valid=(130, 180), kv_valid=(150, 0)),   # image 1 without a valid key
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (q, k, v, g, q_mask, kv_mask) on the GPU: q, k ~ amp N(0, 1), v, g ~ N(0, 1) from one seeded numpy generator."""
    c = CASES[name]
    rng = np.random.default_rng(c['seed'])
    C = H * c['D']
    q = (c['amp'] * rng.standard_normal((c['N'], c['L'], C))).astype(np.float32)
    k = (c['amp'] * rng.standard_normal((c['N'], c['S'], C))).astype(np.float32)
    v = rng.standard_normal((c['N'], c['S'], C)).astype(np.float32)
    g = rng.standard_normal((c['N'], c['L'], C)).astype(np.float32)
    qm = km = None
    if 'q_valid' in c:
        qm = np.zeros((c['N'], c['L']), bool)
        km = np.zeros((c['N'], c['S']), bool)
        for n in range(c['N']):
            qm[n, :c['q_valid'][n]] = True
            km[n, :c['kv_valid'][n]] = True
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    return t(q), t(k), t(v), t(g), t(qm), t(km)


def attention_def(q, k, v, nhead, q_mask=None, kv_mask=None):
    """linear_attention.py:74-86 in the dtype of its inputs, differentiable: q (N, L, H D), k, v (N, S, H D) -> (N, L, H D)."""
    N, L, C = q.shape
    S, D = k.shape[1], C // nhead
    Q, K, V = q.view(N, L, nhead, D), k.view(N, S, nhead, D), v.view(N, S, nhead, D)
    QK = torch.einsum('nlhd,nshd->nlsh', Q, K) / D ** .5
    if kv_mask is not None:
        km = kv_mask.bool()
        some = km.any(1)[:, None, None, None]                                  # an image without a valid key: zeros, not NaN
        QK = QK + torch.where(km[:, None, :, None] | ~some, 0.0, float('-inf')).to(QK.dtype)
        A = torch.softmax(QK, dim=2) * (km[:, None, :, None] & some).to(QK.dtype)
    else:
        A = torch.softmax(QK, dim=2)
    out = torch.einsum('nlsh,nshd->nlhd', A, V).reshape(N, L, C)
    if q_mask is not None:
        out = out * q_mask.bool()[:, :, None].to(out.dtype)
    return out


def def_grads(q, k, v, g, qm, km, dtype):
    """(out, dq, dk, dv) of the definition in `dtype` by torch autograd."""
    Q, K, V = (t.to(dtype).clone().requires_grad_() for t in (q, k, v))
    out = attention_def(Q, K, V, H, qm, km)
    return (out.detach(),) + torch.autograd.grad(out, (Q, K, V), g.to(dtype))


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 (out, dq, dk, dv) and the fp32 definition's own deviations (dev32 of out: max abs; of each gradient: relative
    Frobenius), computed once per case and left unchanged."""
    q, k, v, g, qm, km = inputs(name)
    r64 = def_grads(q, k, v, g, qm, km, torch.float64)
    r32 = def_grads(q, k, v, g, qm, km, torch.float32)
    dev_out = float((r32[0].double() - r64[0]).abs().max())
    dev = tuple(rel(a, b) for a, b in zip(r32[1:], r64[1:]))
    return r64, dev_out, dev


def rel(got, ref):
    n = float(ref.double().norm())
    d = float((got.double() - ref.double()).norm())
    return d / n if n > 0 else d


def kernel_grads(q, k, v, g, qm=None, km=None):
    from far_amd import ops
    Q, K, V = (t.clone().requires_grad_() for t in (q, k, v))
    out = ops.full_attention_train(Q, K, V, H, qm, km)
    dq, dk, dv = torch.autograd.grad(out, (Q, K, V), g)
    return out.detach(), dq, dk, dv


def compare(name, got, ref, dev):
    """Prints and asserts the gradient bar for (dq, dk, dv); -> the three relative errors."""
    errs = []
    for nm, a, b, d32 in zip(('dq', 'dk', 'dv'), got, ref, dev):
        e = rel(a, b)
        bar = max(GRAD_BAR, d32)
        print(f'[train parity] {name} {nm}: rel Frobenius {e:.3e}  dev32 {d32:.3e}  |ref| {float(b.norm()):.1f}  bar {bar:.1e}')
        errs.append((nm, e, bar))
    for nm, e, bar in errs:
        assert np.isfinite(e) and e <= bar, (name, nm, e, bar)
    return [e for _, e, _ in errs]


# ---- forward and gradients ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_forward_and_gradients(name):
    from far_amd import ops
    q, k, v, g, qm, km = inputs(name)
    r64, dev_out, dev = reference(name)
    ops.overflow_flag('cuda').zero_()
    out, dq, dk, dv = kernel_grads(q, k, v, g, qm, km)
    assert not ops.activation_overflowed('cuda')
    assert torch.equal(out, ops.full_attention(q, k, v, H, qm, km))           # the training forward is the inference kernel's bits
    _bar(f'train forward {name} vs float64', out, r64[0], dev_out, rows=None if qm is None else qm.bool())
    compare(name, (dq, dk, dv), r64[1:], dev)


@pytest.mark.parametrize('name', ['t7', 't7e'])
def test_masks_hold_anything(name):
    from far_amd import ops
    q, k, v, g, qm, km = inputs(name)
    r64, _, dev = reference(name)
    k2, v2, g2 = k.clone(), v.clone(), g.clone()
    k2[~km] = float('nan')
    v2[~km] = float('nan')
    g2[~qm] = float('nan')
    ops.overflow_flag('cuda').zero_()
    out, dq, dk, dv = kernel_grads(q, k2, v2, g2, qm, km)
    assert not ops.activation_overflowed('cuda')
    for nm, t in (('out', out), ('dq', dq), ('dk', dk), ('dv', dv)):
        assert torch.isfinite(t).all(), nm
    assert bool((dk[~km] == 0).all()) and bool((dv[~km] == 0).all())
    assert bool((dq[~qm] == 0).all())
    for n in range(q.shape[0]):
        if not bool(km[n].any()):
            assert bool((dq[n] == 0).all()) and bool((dk[n] == 0).all()) and bool((dv[n] == 0).all()), n
    compare(name + ' (NaN behind the masks)', (dq, dk, dv), r64[1:], dev)


@pytest.mark.parametrize('log2_scale', [-20, 10])
def test_gradient_scale(log2_scale):
    """Upstream gradients scaled by 2^k: the same relative error -- g and ds are normalised by powers of two taken from the
    image's max |g| on the device (the assertion of tests/test_sinkhorn_train_gpu.py: test_gradient_scale)."""
    q, k, v, g, qm, km = inputs('t1')
    r64, _, dev = reference('t1')
    e0 = compare('scale 2^0', kernel_grads(q, k, v, g)[1:], r64[1:], dev)
    sc = 2.0 ** log2_scale
    got = tuple(t / sc for t in kernel_grads(q, k, v, g * sc)[1:])
    ek = compare(f'scale 2^{log2_scale}', got, r64[1:], dev)
    for a, b in zip(e0, ek):
        assert abs(a - b) <= 0.05 * a + 1e-9, (e0, ek)


@pytest.mark.parametrize('name', ['t1', 't3', 't5a'])
def test_determinism_and_batch_independence(name):
    q, k, v, g, qm, km = inputs(name)
    first = kernel_grads(q, k, v, g)
    for _ in range(4):
        for a, b in zip(first, kernel_grads(q, k, v, g)):
            assert torch.equal(a, b)
    for n in range(2):                                                        # an image alone = the image inside the batch
        alone = kernel_grads(q[n:n + 1], k[n:n + 1], v[n:n + 1], g[n:n + 1])
        for a, b in zip(first, alone):
            assert torch.equal(a[n:n + 1], b), (name, n)


def test_memory_stays_below_one_score_tensor():
    from far_amd import ops
    N, L, S, D = 2, 1200, 1200, 32
    gen = torch.Generator(device='cuda').manual_seed(3)
    q, k, v, g = (torch.randn(N, n, H * D, device='cuda', generator=gen) for n in (L, S, S, L))
    q.requires_grad_(); k.requires_grad_(); v.requires_grad_()
    ops.full_attention_train(q, k, v, H).backward(g)                          # warm: the flag, workspaces of the allocator
    q.grad = k.grad = v.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ops.full_attention_train(q, k, v, H).backward(g)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    scores = N * H * L * S * 4
    print(f'[train memory] forward + backward peak {used / 2**20:.1f} MiB; one (N, L, S, H) fp32 score tensor {scores / 2**20:.1f} MiB')
    assert used < scores


def test_edge_cases():
    from far_amd import _lib, ops
    for shape_q, shape_k in (((0, 40, 256), (0, 50, 256)), ((2, 0, 256), (2, 50, 256)), ((2, 40, 256), (2, 0, 256))):
        q = torch.randn(*shape_q, device='cuda').requires_grad_()
        k = torch.randn(*shape_k, device='cuda').requires_grad_()
        v = torch.randn(*shape_k, device='cuda').requires_grad_()
        out = ops.full_attention_train(q, k, v, 8)
        assert out.shape == shape_q and bool((out == 0).all())
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), torch.ones_like(out))
        assert dq.shape == shape_q and dk.shape == shape_k and dv.shape == shape_k
        assert bool((dq == 0).all()) and bool((dk == 0).all()) and bool((dv == 0).all())
    x = torch.zeros(1, 40, 192, device='cuda', requires_grad=True)            # head dim 24
    with pytest.raises(_lib.FarHipError):
        ops.full_attention_train(x, x, x, 8)
    q, k, v, g, _, _ = inputs('t1')
    for which in range(3):                                                    # beyond 65504 / 2^4: the backward flags it too
        t = [q.clone(), k.clone(), v.clone()]
        t[which][1, 17, 40] = 5000.0
        Q, K, V = (a.requires_grad_() for a in t)
        out = ops.full_attention_train(Q, K, V, H)
        assert ops.activation_overflowed('cuda'), which
        ops.overflow_flag('cuda').zero_()
        out.backward(g)
        assert ops.activation_overflowed('cuda'), which
    ops.overflow_flag('cuda').zero_()
    gn = g.clone()
    gn[0, 3, 5] = float('inf')                                                # a non-finite gradient on a row that takes part
    kernel_grads(q, k, v, gn)
    assert ops.activation_overflowed('cuda')
    ops.overflow_flag('cuda').zero_()


# ---- one layer ----------------------------------------------------------------------------------------------------------
def layer_def(w, x, source, nhead, x_mask=None, source_mask=None):
    """LoFTREncoderLayer.forward (transformer.py:44-67) around attention_def, in the dtype of its inputs; w: name -> tensor."""
    lin = lambda t, name: t @ w[name + '.weight'].T
    ln = lambda t, name: torch.nn.functional.layer_norm(t, (t.shape[-1],), w[name + '.weight'], w[name + '.bias'], 1e-5)
    msg = attention_def(lin(x, 'q_proj'), lin(source, 'k_proj'), lin(source, 'v_proj'), nhead, x_mask, source_mask)
    msg = ln(lin(msg, 'merge'), 'norm1')
    msg = lin(torch.relu(lin(torch.cat([x, msg], dim=2), 'mlp.0')), 'mlp.2')
    return x + ln(msg, 'norm2')


@pytest.mark.parametrize('masked', [False, True])
def test_one_layer(masked):
    from far_amd.loftr.transformer import LoFTREncoderLayer
    layer = fa_in.seeded_fill(LoFTREncoderLayer(256, H, 'full'), fa_in.LAYER['seed']).cuda().train()
    rng = np.random.default_rng(2301)
    x, src, gy = (torch.from_numpy(rng.standard_normal((2, n, 256)).astype(np.float32)).cuda() for n in (200, 150, 200))
    xm = sm = None
    if masked:
        xm = torch.arange(200, device='cuda')[None, :] < torch.tensor([130, 200], device='cuda')[:, None]
        sm = torch.arange(150, device='cuda')[None, :] < torch.tensor([150, 70], device='cuda')[:, None]
    X, S_ = x.clone().requires_grad_(), src.clone().requires_grad_()
    with pytest.raises(NotImplementedError, match='full'):                    # opt-in
        layer(X, S_, xm, sm)
    layer.full_training = layer.attention.full_training = True
    y = layer(X, S_, xm, sm)
    names = [n for n, _ in layer.named_parameters()]
    got = torch.autograd.grad(y, [X, S_] + [p for _, p in layer.named_parameters()], gy)
    w = {n: p.detach().double().clone().requires_grad_() for n, p in layer.named_parameters()}
    X64, S64 = x.double().requires_grad_(), src.double().requires_grad_()
    y64 = layer_def(w, X64, S64, H, xm, sm)
    ref = torch.autograd.grad(y64, [X64, S64] + [w[n] for n in names], gy.double())
    tag = 'masked' if masked else 'plain'
    print(f'[train parity] layer {tag} output: max|d| {float((y.detach().double() - y64.detach()).abs().max()):.3e}')
    bad = []
    for nm, a, b in zip(['x', 'source'] + names, got, ref):
        e = rel(a, b)
        print(f'[train parity] layer {tag} d{nm}: rel Frobenius {e:.3e}  |ref| {float(b.norm()):.2f}')
        if not e <= LAYER_BAR:
            bad.append((nm, e))
    assert not bad, bad


# ---- the model ----------------------------------------------------------------------------------------------------------
def _full_model():
    from far_amd import synth
    from far_amd.config import far_train_config
    from far_amd.loftr import LoFTR
    cfg = far_train_config()
    for b in ('coarse', 'fine'):
        cfg['loftr'][b]['attention'] = 'full'
    m = LoFTR(cfg['loftr'])
    synth.load_synthetic(m, seed=0)
    return cfg, m.cuda()


def test_model_train_step():
    from far_amd import synth
    from far_amd.config import RunCfg
    from far_amd.losses import LoFTRLoss
    from far_amd.pipeline import test_step, train_step
    cfg, m = _full_model()
    never = copy.deepcopy(m).eval()                                           # a model that never had the switch on
    loss_fn = LoFTRLoss(cfg).train()
    base = synth.synth_training_batch(1, seed=77, device='cuda')

    def run(model):
        model.zero_grad(set_to_none=True)
        batch = dict(base)
        torch.manual_seed(5)
        train_step(model, batch, loss_fn, RunCfg('prior_ransac', 2), H=256, seed=0)
        batch['loss'].backward()
        return float(batch['loss']), {k: p.grad.clone() for k, p in model.named_parameters()}

    m.train()
    with pytest.raises(NotImplementedError, match='full'):
        run(m)
    assert m.set_full_attention_training() is m
    l0, g0 = run(m)
    l1, g1 = run(m)
    assert l0 == l1 and np.isfinite(l0)
    for k in g0:
        assert torch.isfinite(g0[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k
    for pre in ('loftr_coarse.', 'loftr_fine.'):
        assert all(float(g0[k].abs().sum()) > 0 for k in g0 if k.startswith(pre) and k.endswith('_proj.weight')), pre
        assert sum(float(g0[k].abs().sum()) for k in g0 if k.startswith(pre)) > 0
    name = 'loftr_coarse.layers.0.q_proj.weight'
    wq = dict(m.named_parameters())[name]
    w_before = wq.detach().clone()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.1)
    opt.step()
    assert not torch.equal(wq.detach(), w_before)
    m.load_state_dict(never.state_dict())                                     # back to the state `never` holds
    m.eval()
    keys = ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_f', 'mkpts1_f', 'loftr_rt', 'regressed_rt')
    outs = []
    for model in (m, never):
        im0, im1 = synth.synth_image_pair(1, seed=21)
        K = torch.from_numpy(np.stack([synth.MP3D_K])).cuda()
        d = {'image0': torch.from_numpy(im0).cuda(), 'image1': torch.from_numpy(im1).cuda(), 'K0': K, 'K1': K.clone(),
             'dataset_name': ['mp3d']}
        test_step(model, d, H=256)
        outs.append({k: d[k].clone() for k in keys})
    for k in keys:
        assert torch.equal(outs[0][k], outs[1][k]), k
