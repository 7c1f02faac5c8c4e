"""LoFTR's full softmax attention (attention = 'full') without a GPU: the float64 restatement of the operator (and of the layer and
the stack around it) that the GPU tests measure the kernel against, pinned to the reference's own run (golden G21); the module
and configuration side; the C ABI.

Mask convention of the restatement = the kernel's: a masked key is selected out, a padded query row is exact
zeros, a missing mask is all ones, an image without a valid key gives zeros.  On valid query rows it is the reference's function
(linear_attention.py:74-86); the reference's padded rows are NaN."""
import os

import numpy as np
import pytest
import torch

from far_amd import _lib
from far_amd.config import far_eval_config
from tests import full_attention_inputs as fa_in

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g21_full_attention.npz')


def full_attention_ref(q, k, v, nhead, q_mask=None, kv_mask=None, dtype=torch.float64, chunk=512):
    """out[n, l, h, :] = sum_s softmax_s(q[n,l,h,:] . k[n,s,h,:] / sqrt(D)) v[n,s,h,:] in `dtype`, the operations of
    linear_attention.py:74-86 in their order, `chunk` query rows at a time.  q (N, L, H D), k, v (N, S, H D) -> (N, L, H D)."""
    N, L, C = q.shape
    S = k.shape[1]
    D = C // nhead
    Q, K, V = q.to(dtype).view(N, L, nhead, D), k.to(dtype).view(N, S, nhead, D), v.to(dtype).view(N, S, nhead, D)
    if kv_mask is not None:
        km = kv_mask.bool()
        K = torch.where(km[:, :, None, None], K, torch.zeros_like(K))          # selected out: never multiplied
        V = torch.where(km[:, :, None, None], V, torch.zeros_like(V))
    out = torch.zeros(N, L, nhead, D, dtype=dtype, device=q.device)
    temp = 1. / D ** .5
    for l0 in range(0, L, chunk):
        QK = torch.einsum('nlhd,nshd->nlsh', Q[:, l0:l0 + chunk], K)
        if kv_mask is not None:
            QK = QK.masked_fill(~km[:, None, :, None], float('-inf'))
        A = torch.softmax(temp * QK, dim=2)
        if kv_mask is not None:
            A = torch.nan_to_num(A, nan=0.0)                                   # an image without a valid key: zeros
        out[:, l0:l0 + chunk] = torch.einsum('nlsh,nshd->nlhd', A, V)
    if q_mask is not None:
        out = torch.where(q_mask.bool()[:, :, None, None], out, torch.zeros_like(out))
    return out.reshape(N, L, C)


def encoder_layer_ref(sd, x, source, nhead, x_mask=None, source_mask=None, dtype=torch.float64):
    """LoFTREncoderLayer.forward (transformer.py:44-67) with the full attention core, in `dtype`; sd: the layer's state dict."""
    w = {k: t.to(device=x.device, dtype=dtype) for k, t in sd.items()}
    x, source = x.to(dtype), source.to(dtype)
    lin = lambda t, name: t @ w[name + '.weight'].T
    ln = lambda t, name: torch.nn.functional.layer_norm(t, (t.shape[-1],), w[name + '.weight'], w[name + '.bias'], 1e-5)
    msg = full_attention_ref(lin(x, 'q_proj'), lin(source, 'k_proj'), lin(source, 'v_proj'), nhead, x_mask, source_mask, dtype)
    msg = ln(lin(msg, 'merge'), 'norm1')
    msg = lin(torch.relu(lin(torch.cat([x, msg], dim=2), 'mlp.0')), 'mlp.2')
    return x + ln(msg, 'norm2')


def stack_ref(sd, layer_names, nhead, feat0, feat1, mask0=None, mask1=None, dtype=torch.float64):
    """LocalFeatureTransformer.forward (transformer.py:90-112); sd: the stack's state dict ('layers.<i>.<name>')."""
    feat0, feat1 = feat0.to(dtype), feat1.to(dtype)
    for i, name in enumerate(layer_names):
        lsd = {k[len(f'layers.{i}.'):]: t for k, t in sd.items() if k.startswith(f'layers.{i}.')}
        if name == 'self':
            feat0 = encoder_layer_ref(lsd, feat0, feat0, nhead, mask0, mask0, dtype)
            feat1 = encoder_layer_ref(lsd, feat1, feat1, nhead, mask1, mask1, dtype)
        else:
            feat0 = encoder_layer_ref(lsd, feat0, feat1, nhead, mask0, mask1, dtype)
            feat1 = encoder_layer_ref(lsd, feat1, feat0, nhead, mask1, mask0, dtype)
    return feat0, feat1


def core_tensors(name, device='cpu'):
    inp = fa_in.core_inputs(name)
    t = lambda a: None if a is None else torch.from_numpy(a).to(device)
    return t(inp['q']), t(inp['k']), t(inp['v']), t(inp['q_mask']), t(inp['kv_mask']), inp['H']


def golden():
    return np.load(GOLDEN)


def _rows(t, stride):
    return fa_in.strided_rows(t.detach().cpu().numpy(), stride)


@pytest.mark.parametrize('name', list(fa_in.CASES))
def test_restatement_reproduces_the_reference(name):
    """float64 restatement vs the reference's stored fp32 outputs: within the fp32 run's own distance from float64 (dev32), i.e.
    the restatement IS the reference's float64 evaluation (case d: on valid query rows, the only rows the reference defines)."""
    g = golden()
    q, k, v, qm, km, H = core_tensors(name)
    out = full_attention_ref(q, k, v, H, qm, km)
    got, ref = _rows(out, fa_in.CASES[name]['stride']), g['out_' + name]
    assert got.shape == ref.shape and np.isfinite(got).all()
    d = float(np.abs(got - ref.astype(np.float64)).max())
    dev32 = float(g['dev32_' + name])
    print(f'[g21] {name}: |f64 restatement - reference fp32| = {d:.3e}, dev32 = {dev32:.3e}')
    assert d <= dev32 * (1 + 1e-6) + 1e-12
    assert 0 < dev32 < 1e-4


def test_mask_convention():
    g = golden()
    assert bool(g['ref_masked_stack_nan']) and bool(g['ref_kv_mask_alone_raises'])     # what the deviation is stated against
    q, k, v, qm, km, H = core_tensors('d')
    out = full_attention_ref(q, k, v, H, qm, km)
    assert bool((out[~qm] == 0).all()) and bool(torch.isfinite(out).all())
    # non-finite k / v at masked keys never reach an output
    k2, v2 = k.clone(), v.clone()
    k2[~km], v2[~km] = float('nan'), float('inf')
    assert torch.equal(full_attention_ref(q, k2, v2, H, qm, km), out)
    # masks of ones = no masks; kv_mask alone works; an image without a valid key gives zeros
    ones_q, ones_k = torch.ones_like(qm), torch.ones_like(km)
    assert torch.equal(full_attention_ref(q, k, v, H, ones_q, ones_k), full_attention_ref(q, k, v, H))
    alone = full_attention_ref(q, k, v, H, None, km)
    assert torch.equal(alone[qm], out[qm])
    km0 = km.clone()
    km0[1] = False
    z = full_attention_ref(q, k, v, H, None, km0)
    assert bool((z[1] == 0).all()) and torch.equal(z[0], alone[0])


def test_module_restatements_reproduce_the_reference():
    from far_amd.loftr.transformer import LocalFeatureTransformer, LoFTREncoderLayer
    import copy
    g = golden()
    layer = fa_in.seeded_fill(LoFTREncoderLayer(256, fa_in.NHEAD, 'full'), fa_in.LAYER['seed'])
    x, src = (torch.from_numpy(a) for a in fa_in.layer_inputs())
    y = encoder_layer_ref(layer.state_dict(), x, src, fa_in.NHEAD)
    d = float(np.abs(_rows(y, fa_in.LAYER['stride']) - g['out_layer'].astype(np.float64)).max())
    print(f'[g21] layer: |f64 restatement - reference fp32| = {d:.3e}, dev32 = {float(g["dev32_layer"]):.3e}')
    assert d <= float(g['dev32_layer']) * (1 + 1e-6) + 1e-12
    stack = fa_in.seeded_fill(LocalFeatureTransformer(copy.deepcopy(fa_in.STACK['config'])), fa_in.STACK['seed'])
    f0, f1 = (torch.from_numpy(a) for a in fa_in.stack_inputs())
    a, b = stack_ref(stack.state_dict(), fa_in.STACK['config']['layer_names'], fa_in.NHEAD, f0, f1)
    d = max(float(np.abs(_rows(a, fa_in.STACK['stride']) - g['out_stack0'].astype(np.float64)).max()),
            float(np.abs(_rows(b, fa_in.STACK['stride']) - g['out_stack1'].astype(np.float64)).max()))
    print(f'[g21] stack: |f64 restatement - reference fp32| = {d:.3e}, dev32 = {float(g["dev32_stack"]):.3e}')
    assert d <= float(g['dev32_stack']) * (1 + 1e-6) + 1e-12


def test_full_layer_constructs_with_the_linear_layers_state():
    from far_amd.loftr.transformer import FullAttention, LinearAttention, LoFTREncoderLayer
    full, lin = LoFTREncoderLayer(256, 8, 'full'), LoFTREncoderLayer(256, 8, 'linear')
    assert isinstance(full.attention, FullAttention) and isinstance(lin.attention, LinearAttention)
    assert list(full.state_dict()) == list(lin.state_dict())
    assert not list(FullAttention(use_dropout=False, attention_dropout=0.1, use_num_corres=False).parameters())
    lin.load_state_dict(full.state_dict(), strict=True)
    assert isinstance(LoFTREncoderLayer(128, 8, 'full').attention, FullAttention)
    for bad in ('softmax', 'Full', ''):
        with pytest.raises(NotImplementedError):
            LoFTREncoderLayer(256, 8, bad)


def test_full_attention_refuses_cpu_tensors_and_autograd():
    from far_amd.loftr.transformer import FullAttention, LoFTREncoderLayer
    att = FullAttention()
    q = torch.zeros(1, 4, 8, 32)
    with pytest.raises(_lib.FarHipError):
        att(q, q, q)
    with pytest.raises(NotImplementedError, match='FullAttention'):
        att(q.requires_grad_(), q, q)
    layer = LoFTREncoderLayer(256, 8, 'full').eval()
    with torch.no_grad(), pytest.raises(_lib.FarHipError):
        layer(torch.zeros(1, 4, 256), torch.zeros(1, 4, 256))


@pytest.mark.parametrize('blocks', [('coarse',), ('fine',), ('regress',), ('coarse', 'fine', 'regress')])
def test_config_accepts_full_per_block(blocks):
    from far_amd.loftr import LoFTR
    from far_amd.loftr.transformer import FullAttention, LoFTREncoderLayer
    cfg = far_eval_config()
    for b in blocks:
        cfg[b]['attention'] = 'full'
    m = LoFTR(cfg)
    assert len(m.state_dict()) == 240                     # reference checkpoints load unchanged
    owner = {'coarse': m.loftr_coarse, 'fine': m.loftr_fine, 'regress': m.loftr_regress.loftr}
    for b, mod in owner.items():
        kinds = {isinstance(l.attention, FullAttention) for l in mod.modules() if isinstance(l, LoFTREncoderLayer)}
        assert kinds == {b in blocks}
    m.set_precision('fp16')                               # the stages act on the Linear launches; the core has one precision
    m.set_precision('fp32')


def test_abi_and_workspace_query_without_gpu():
    lib = _lib.load()
    assert _lib.EXPECTED_ABI == lib.far_abi_version()
    assert 'far_full_attention_f16s' in _lib.SIGNATURES and 'far_full_attention_workspace_bytes' in _lib.SIGNATURES
    ws = lib.far_full_attention_workspace_bytes
    assert ws(64, 4800, 4800, 8, 32) == 0                 # enough workgroups per image: no key split, no workspace
    n = ws(2, 300, 1200, 8, 32)                           # short query side: partial (acc, sum, reference) per split
    assert n >= 2 * 8 * 300 * 2 * (32 + 2) * 4
    assert ws(4, 300, 1200, 8, 32) >= 2 * n - 1024        # linear in the batch
    assert ws(2, 300, 1200, 8, 64) == 0 and ws(0, 300, 1200, 8, 32) == 0
