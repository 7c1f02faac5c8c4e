"""Training far_amd.vit8pt on the GPU (ViTEss.set_block_training): one Block, the whole model under vit8pt.pose_loss, one optimizer
step, and the refusal without the switch -- on the seeded fill of tests/vit8pt_inputs.py (peaked softmax rows, B = 2).

References: float64 torch autograd of tests/vit8pt_ref.py (_Block; RefViTEss through tests/vit8pt_train_ref.py, which removes the
no_grad wrapper and nothing else).
Bars: one Block's gradients (x and every parameter) have a relative Frobenius error of at most LAYER_BAR = 3e-3, the project's
per-layer bar (tests/test_full_attention_train_gpu.py).  For the whole model nobody has measured how far the existing training
kernels (K9 dgrad, K16 wgrad, K6, K2's backward) sit from float64 through six blocks, so K23's backward is held relative to them: the
same model runs a second time with ONLY the attention core replaced by fp32 torch autograd, and per tensor
err_hip <= err_torch_core + LAYER_BAR.  A tensor whose float64 norm is below 1e-6 of the largest is compared in absolute terms (its
difference over the largest norm).  Both columns are printed ('[vit train parity] ...'; profiles/vit8pt_train_parity.txt)."""
import numpy as np
import pytest
import torch

from tests import vit8pt_inputs as vi
from tests import vit8pt_ref as vr
from tests import vit8pt_train_ref as vtr
from tests.test_vit8pt_gpu import setup

pytestmark = pytest.mark.gpu
LAYER_BAR = 3e-3
W_TR, W_ROT = 1.0, 1.0


def fresh_model(train=True):
    """A new far_amd ViTEss with the seeded fill (the cached one of setup() is never flipped)."""
    from far_amd.vit8pt import ViTEss
    _, ref, inp = setup()
    m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'])
    m.load_state_dict(ref.state_dict(), strict=True)
    m = m.cuda()
    return (m.train().set_block_training() if train else m.eval()), ref, inp


def targets(B):
    g = torch.Generator().manual_seed(77)
    return torch.randn(B, 3, generator=g).cuda(), torch.randn(B, 3, 3, generator=g).cuda()


def rel(got, ref):
    n = float(ref.double().norm())
    d = float((got.double() - ref.double()).norm())
    return d / n if n > 0 else d


def model_grads(m, inp):
    from far_amd.vit8pt import pose_loss
    gt_tran, gt_rot = targets(vi.B)
    m.zero_grad(set_to_none=True)
    out = m.forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
    loss = pose_loss(out, gt_tran, gt_rot, W_TR, W_ROT)
    loss.backward()
    return float(loss.detach()), {k: p.grad.clone() for k, p in m.named_parameters()}


def test_one_block():
    m, ref, inp = fresh_model()
    r64 = ref.as_dtype(torch.float64, 'cuda')
    taps = []
    with torch.no_grad():
        r64.trunk(inp['features'], vi.VIT_INTRINSICS, taps)
    x = taps[1].float()
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(31)).cuda()
    blk, blk64 = m.fusion_transformer.blocks[2], r64.fusion_transformer.blocks[2]
    names = [n for n, _ in blk.named_parameters()]
    assert names == [n for n, _ in blk64.named_parameters()]

    def run():
        X = x.clone().requires_grad_()
        y = blk(X)
        return y.detach(), torch.autograd.grad(y, [X] + [p for _, p in blk.named_parameters()], gy)

    y, got = run()
    X64 = x.double().requires_grad_()
    y64 = blk64(X64)
    want = torch.autograd.grad(y64, [X64] + [p for _, p in blk64.named_parameters()], gy.double())
    print(f'[vit train parity] Block 2 output: max|d| {float((y.double() - y64.detach()).abs().max()):.3e}')
    bad = []
    for nm, a, b in zip(['x'] + names, got, want):
        e = rel(a, b)
        print(f'[vit train parity] Block 2 d{nm}: rel Frobenius {e:.3e}  |ref| {float(b.norm()):.2f}')
        if not e <= LAYER_BAR:
            bad.append((nm, e))
    assert not bad, bad
    y2, got2 = run()
    assert torch.equal(y, y2)
    for nm, a, b in zip(['x'] + names, got, got2):
        assert torch.equal(a, b), nm
    with torch.no_grad():                                                     # the training forward computes the inference path's function
        yi = blk(x)
    assert float((y - yi).abs().max()) <= 1e-4 * float(yi.abs().max())


def test_whole_model_gradients(monkeypatch):
    from far_amd import ops
    from far_amd.vit8pt import pose_loss
    m, ref, inp = fresh_model()
    loss, g_hip = model_grads(m, inp)
    loss2, g_hip2 = model_grads(m, inp)
    assert loss == loss2 and np.isfinite(loss)
    for k in g_hip:
        assert torch.equal(g_hip[k], g_hip2[k]), k
    monkeypatch.setattr(ops, 'vit_attention_train_qkv', vtr.torch_core_qkv)
    loss_t, g_torch = model_grads(m, inp)
    monkeypatch.undo()
    r64 = vtr.from_ref(ref, torch.float64, 'cuda')
    gt_tran, gt_rot = targets(vi.B)
    out64 = r64.forward_features(inp['features'], vi.VIT_INTRINSICS, inp['loftr_num_corr'], inp['loftr_preds'])
    loss64 = pose_loss(out64, gt_tran.double(), gt_rot.double(), W_TR, W_ROT)
    loss64.backward()
    g64 = {k: p.grad for k, p in r64.named_parameters()}
    assert set(g64) == set(g_hip)
    print(f'[vit train parity] model loss: hip {loss:.9g}  torch-core {loss_t:.9g}  float64 {float(loss64.detach()):.9g}')
    top = max(float(g.norm()) for g in g64.values())
    bad = []
    for k in sorted(g64):
        assert torch.isfinite(g_hip[k]).all(), k
        n64 = float(g64[k].norm())
        if n64 < 1e-6 * top:
            e_h, e_t, how = (float((g_hip[k].double() - g64[k]).norm()) / top, float((g_torch[k].double() - g64[k]).norm()) / top, 'abs/top')
        else:
            e_h, e_t, how = rel(g_hip[k], g64[k]), rel(g_torch[k], g64[k]), 'rel'
        print(f'[vit train parity] model d{k}: hip {e_h:.3e}  torch-core {e_t:.3e}  ({how})  |ref| {n64:.3e}')
        if not e_h <= e_t + LAYER_BAR:
            bad.append((k, e_h, e_t))
    assert not bad, bad
    for k, g in g_hip.items():
        if k.startswith('fusion_transformer.'):
            assert float(g.abs().sum()) > 0, k


def test_one_optimisation_step_and_the_inference_bits():
    from far_amd.optim import AdamW
    m, ref, inp = fresh_model()
    never, _, _ = fresh_model(train=False)                                    # a model that never had the switch on
    untouched = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = AdamW(m.parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    model_grads(m, inp)
    name = 'fusion_transformer.blocks.1.attn.qkv.weight'
    w = dict(m.named_parameters())[name]
    before = w.detach().clone()
    opt.step()
    assert not torch.equal(w.detach(), before) and torch.isfinite(w).all()
    m.load_state_dict(untouched)
    m.eval()
    args = (inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
    with torch.no_grad():
        a, b = m.forward_features(*args), never.forward_features(*args)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with torch.no_grad():                                                     # ... and with the switch still on in train mode: the same bits
        for x, y in zip(m.train().forward_features(*args), b):
            assert torch.equal(x, y)


def test_without_the_switch_training_is_refused():
    m, _, inp = fresh_model(train=False)
    m.train()
    for needle in ('far_vit_attention_f16s', 'set_block_training'):
        with pytest.raises(NotImplementedError, match=needle):
            m.forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
    x = torch.zeros(2, 576, 192, device='cuda')
    for needle in ('far_vit_attention_f16s', 'set_block_training'):
        with pytest.raises(NotImplementedError, match=needle):
            m.fusion_transformer.blocks[0](x)
