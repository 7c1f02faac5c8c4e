"""Training the 8-Point-ViT extractor's final block on the GPU (ViTEss.set_extractor_training): the block alone, the whole model from
images under vit8pt.pose_loss, one optimizer step, and what stays as it was -- on the seeded fill of tests/vit8pt_extractor_inputs.py,
images (2, 2, 3, 37, 53): four images, the block sees 4 x 28 x 28 x 128.

Yardstick: tests/vit8pt_extractor_train_ref.py's RefViTEssImagesTrain in float64 (final block in .train(), front in .eval() and frozen,
trunk as tests/vit8pt_train_ref.py; pinned to the reference's ResidualBlock by tests/test_vit8pt_extractor_train_cpu.py).
Bars: the block's training output and the updated running statistics under the project's parity rule (test_full_attention_gpu.py:
_bar: max(3 x dev32, 2^-20 max|r64|), dev32 the fp32 torch module's own deviation in the same run); the block's gradients at
LAYER_BAR = 3e-3 relative Frobenius (tests/test_vit8pt_train_gpu.py), its three convolution bias gradients (~ 0 under batch
statistics) under _bar's absolute rule; the whole model per tensor err_hip <= err_torch_block + LAYER_BAR, where the second leg is
the same model with ONLY the final block on fp32 torch autograd (the form test_vit8pt_train_gpu.py holds the attention core to)."""
import copy

import numpy as np
import pytest
import torch

from tests import vit8pt_extractor_inputs as ei
from tests import vit8pt_extractor_ref as er
from tests import vit8pt_extractor_train_ref as etr
from tests import vit8pt_inputs as vi
from tests.test_full_attention_gpu import _bar
from tests.test_vit8pt_train_gpu import LAYER_BAR, W_ROT, W_TR, rel, targets

pytestmark = pytest.mark.gpu
_CACHE = {}
CONV_BIAS = ('conv1.bias', 'conv2.bias', 'downsample.0.bias')


def seeded():
    """-> (the seeded RefViTEssImagesTrain (fp32, CPU; never modified), inputs on the GPU, the block's input (4, 128, 28, 28) fp32)."""
    if not _CACHE:
        ref = etr.RefViTEssImagesTrain(vi.vit_args())
        inp = ei.filled(ref)
        ref.pose_mean, ref.pose_std = inp['pose_mean'], inp['pose_std']
        gpu = {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in inp.items()}
        x = ref.as_dtype(torch.float32, 'cuda').front(gpu['images'][0])
        _CACHE['v'] = (ref, gpu, x)
    return _CACHE['v']


def fresh(train=True):
    from far_amd.vit8pt import ViTEss
    ref, inp, _ = seeded()
    m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'], extractor=True)
    m.load_state_dict(ref.state_dict(), strict=True)
    m = m.cuda()
    return m.train().set_block_training().set_extractor_training() if train else m.eval()


def torch_block(fc):
    """The final block of a far_amd ViTEss on fp32 torch autograd, NHWC in and out: the comparison leg."""
    def run(x):
        xc = x.permute(0, 3, 1, 2)
        y = torch.relu(fc.norm1(fc.conv1(xc)))
        y = torch.relu(fc.norm2(fc.conv2(y)))
        return torch.relu(fc.downsample(xc) + y).permute(0, 2, 3, 1)
    return run


def block_grads(fn, module, x, gy, nhwc=False):
    """(output NCHW, [dx NCHW] + the gradients of module's parameters in named_parameters order) of one training forward + backward of
    fn; nhwc: fn takes and returns NHWC."""
    X = x.clone().requires_grad_(True)
    y = fn(X.permute(0, 2, 3, 1)).permute(0, 3, 1, 2) if nhwc else fn(X)
    return y.detach(), torch.autograd.grad(y, [X] + [p for _, p in module.named_parameters()], gy.to(y.dtype))


def test_training_forward_and_running_statistics():
    ref, inp, x = seeded()
    m = fresh()
    fc = m.extractor_final_conv
    b64 = ref.as_dtype(torch.float64, 'cuda').extractor_final_conv
    b32 = ref.as_dtype(torch.float32, 'cuda').extractor_final_conv
    before = int(fc.norm1.num_batches_tracked)
    got = m._final_block_train(x.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    assert got.requires_grad and got.shape == (4, 192, 24, 24)
    y64, y32 = b64(x.double()).detach(), b32(x).detach()
    _bar('final block, training forward', got.detach(), y64, float((y32.double() - y64).abs().max()))
    share = float((got > 0).float().mean())
    print(f'[extractor train] positive share of the block output {share:.3f}')
    assert 0.2 < share < 0.8
    for nm in etr.NORMS:
        bn, n64, n32 = getattr(fc, nm), getattr(b64, nm), getattr(b32, nm)
        for stat in ('running_mean', 'running_var'):
            a, r = getattr(bn, stat), getattr(n64, stat)
            assert not torch.equal(a, getattr(getattr(ref.extractor_final_conv, nm), stat).cuda())       # it moved
            _bar(f'final block {nm}.{stat}', a, r, float((getattr(n32, stat).double() - r).abs().max()))
        assert int(bn.num_batches_tracked) == before + 1 == int(n64.num_batches_tracked)


def test_block_gradients():
    ref, inp, x = seeded()
    m = fresh()
    gy = torch.randn(4, 192, 24, 24, generator=torch.Generator().manual_seed(41)).cuda()
    names = ['x'] + [n for n, _ in m.extractor_final_conv.named_parameters()]
    b64 = ref.as_dtype(torch.float64, 'cuda').extractor_final_conv
    b32 = ref.as_dtype(torch.float32, 'cuda').extractor_final_conv
    assert names[1:] == [n for n, _ in b64.named_parameters()]
    y, got = block_grads(m._final_block_train, m.extractor_final_conv, x, gy, nhwc=True)
    _, want = block_grads(b64, b64, x.double(), gy)
    _, t32 = block_grads(b32, b32, x, gy)
    bad = []
    for nm, a, b, c in zip(names, got, want, t32):
        if nm in CONV_BIAS:
            _bar(f'final block d{nm} (~ 0)', a, b, float((c.double() - b).abs().max()))
            continue
        e = rel(a, b)
        print(f'[extractor train parity] final block d{nm}: rel Frobenius {e:.3e}  (fp32 torch {rel(c, b):.3e})  |ref| {float(b.norm()):.3e}')
        if not e <= LAYER_BAR:
            bad.append((nm, e))
    assert not bad, bad
    y2, got2 = block_grads(m._final_block_train, m.extractor_final_conv, x, gy, nhwc=True)                 # (running statistics moved: batch statistics decide)
    assert torch.equal(y, y2)
    for nm, a, b in zip(names, got, got2):
        assert torch.equal(a, b), nm


def model_grads(m, inp):
    from far_amd.vit8pt import pose_loss
    images = inp['images'][0]
    gt_tran, gt_rot = targets(ei.B)
    m.zero_grad(set_to_none=True)
    out = m(images, ei.image_intrinsics(images.shape).cuda(), loftr_num_corr=inp['loftr_num_corr'], loftr_preds=inp['loftr_preds'])
    loss = pose_loss(out, gt_tran, gt_rot, W_TR, W_ROT)
    loss.backward()
    return float(loss.detach()), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


def test_whole_model_gradients(monkeypatch):
    from far_amd.vit8pt import pose_loss, update_intrinsics
    ref, inp, _ = seeded()
    m = fresh()
    loss, g_hip = model_grads(m, inp)
    loss2, g_hip2 = model_grads(m, inp)
    assert loss == loss2 and np.isfinite(loss)
    for k in g_hip:                                                           # two backward passes from the same state
        if k.startswith('resnet.'):
            assert g_hip[k] is None, k
        else:
            assert torch.equal(g_hip[k], g_hip2[k]), k
    monkeypatch.setattr(m, '_final_block_train', torch_block(m.extractor_final_conv))
    loss_t, g_torch = model_grads(m, inp)
    monkeypatch.undo()
    r64 = ref.as_dtype(torch.float64, 'cuda')
    images = inp['images'][0]
    grid = tuple(float(v) for v in update_intrinsics(images.shape, ei.image_intrinsics(images.shape))[0, 0])
    gt_tran, gt_rot = targets(ei.B)
    out64 = r64.forward_images(images, grid, inp['loftr_num_corr'], inp['loftr_preds'])
    loss64 = pose_loss(out64, gt_tran.double(), gt_rot.double(), W_TR, W_ROT)
    loss64.backward()
    g64 = {k: p.grad for k, p in r64.named_parameters() if p.grad is not None}
    trainable = {k for k, g in g_hip.items() if g is not None}
    assert set(g64) == trainable and not any(k.startswith('resnet.') for k in trainable)
    assert any(k.startswith('extractor_final_conv.') for k in trainable)
    print(f'[extractor train parity] model loss: hip {loss:.9g}  torch-block {loss_t:.9g}  float64 {float(loss64.detach()):.9g}')
    top = max(float(g.norm()) for g in g64.values())
    bad = []
    for k in sorted(g64):
        assert torch.isfinite(g_hip[k]).all(), k
        n64 = float(g64[k].norm())
        if n64 < 1e-6 * top:
            e_h, e_t, how = (float((g_hip[k].double() - g64[k]).norm()) / top, float((g_torch[k].double() - g64[k]).norm()) / top, 'abs/top')
        else:
            e_h, e_t, how = rel(g_hip[k], g64[k]), rel(g_torch[k], g64[k]), 'rel'
        print(f'[extractor train parity] model d{k}: hip {e_h:.3e}  torch-block {e_t:.3e}  ({how})  |ref| {n64:.3e}')
        if not e_h <= e_t + LAYER_BAR:
            bad.append((k, e_h, e_t))
    assert not bad, bad


def test_one_optimisation_step_and_the_packs_follow():
    from far_amd.optim import AdamW
    from far_amd.vit8pt import ViTEss
    ref, inp, _ = seeded()
    m = fresh()
    images = inp['images'][0]
    with torch.no_grad():
        m.eval().extract_features(images)                                     # the inference images of the OLD weights exist
    m.train()
    before = {k: p.detach().clone() for k, p in m.extractor_final_conv.named_parameters()}
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    model_grads(m, inp)
    opt.step()
    for k, p in m.extractor_final_conv.named_parameters():
        assert not torch.equal(p.detach(), before[k]) and torch.isfinite(p).all(), k
    model_grads(m, inp)                                                       # a second step's forward + backward: refreshed training images
    other = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'], extractor=True)
    other.load_state_dict(copy.deepcopy(m.state_dict()), strict=True)
    other = other.cuda().eval()
    with torch.no_grad():
        a, b = m.eval().extract_features(images)[0], other.extract_features(images)[0]
    assert torch.equal(a, b)


def test_unchanged_behaviour_and_refusals():
    ref, inp, _ = seeded()
    images = inp['images'][0]
    m = fresh(train=False)
    with torch.no_grad():
        f0 = m.extract_features(images)[0]
    m.train()
    m.extractor_final_conv.conv2.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='set_extractor_training'):  # a default model: the switch is off
        m.extract_features(images)
    m.extractor_final_conv.conv2.weight.requires_grad_(False)
    stats = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.set_extractor_training() is m
    with pytest.raises(NotImplementedError, match='K25'):
        m.set_extractor_training('all')
    with torch.no_grad():                                                     # under no_grad: today's path, today's bits, in either mode
        assert torch.equal(m.extract_features(images)[0], f0)
        assert torch.equal(m.eval().extract_features(images)[0], f0)
    with pytest.raises(NotImplementedError, match='set_extractor_training'):  # .eval() with gradients
        m.extract_features(images)
    m.set_extractor_training(on=False)
    assert torch.equal(m.extract_features(images)[0], f0)                     # .eval() without gradients
    for k, v in m.state_dict().items():
        assert torch.equal(v, stats[k]), k
    m.train().set_extractor_training()
    m.resnet.layer2[1].conv2.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='set_extractor_training'):  # the front stays frozen
        m.extract_features(images)
    m.resnet.layer2[1].conv2.weight.requires_grad_(False)
    feats = m.extract_features(images)[0]                                     # the training path: features with a graph
    assert feats.requires_grad and feats.shape == f0.shape
