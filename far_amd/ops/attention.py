"""far_amd.ops.attention: K5 linear attention, K22 full attention, K23 head-dim-64 attention and K6 LayerNorm (forward, backward, training wrappers) (one family of the torch-tensor front ends for the C ABI in include/far_hip.h; far_amd/ops/__init__.py
re-exports everything under the flat far_amd.ops namespace the rest of the package uses)."""
import ctypes
import os
import threading

import torch

from .. import _lib, flags
from ._base import _p, _stream, _written, _ws, activation_exponent_value, overflow_flag


def linear_attention(q, k, v, nhead, q_mask=None, kv_mask=None, eps=1e-6):
    """K5.  q: (N, L, C), k, v: (N, S, C) raw projections; returns (N, L, C) (heads concatenated)."""
    lib = _lib.load()
    N, L, C = q.shape
    S = k.shape[1]
    D = C // nhead
    out = torch.empty(N, L, C, dtype=torch.float32, device=q.device)
    if N == 0:
        return out
    ws = _ws(lib.far_linear_attention_workspace_bytes(N, S, nhead, D), q.device)
    rc = lib.far_linear_attention_f32(_p(q, torch.float32), _p(k, torch.float32), _p(v, torch.float32), N, L, S,
                                      nhead, D, _p(q_mask, torch.uint8), _p(kv_mask, torch.uint8), float(eps),
                                      _p(out), _p(ws), _stream())
    _lib.check(rc, 'far_linear_attention_f32')
    return out

def _on_gpu(*ts):
    for t in ts:
        if not t.is_cuda:
            raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')

def _fp32(*ts):
    for t in ts:
        if t.dtype != torch.float32:
            raise _lib.FarHipError(f'expected dtype {torch.float32}, got {t.dtype}')

def _qkv_shape(q, k, v, what, b):
    """GPU tensors q (b, L, C), k, v (b, S, C) -> (b, L, S, C); `b` is the batch axis's letter in the message."""
    _on_gpu(q, k, v)
    if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]:
        raise _lib.FarHipError(f'{what}: q ({b}, L, C), k, v ({b}, S, C); got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}')
    return q.shape[0], q.shape[1], k.shape[1], q.shape[2]

def _full_attention_args(q, k, v, nhead, q_mask, kv_mask):
    """The argument checks K22's front ends share -> (N, L, S, C, D, q_mask, kv_mask) with the masks as contiguous uint8 (or None)."""
    N, L, S, C = _qkv_shape(q, k, v, 'full_attention', 'N')
    if nhead < 1 or C % nhead:
        raise _lib.FarHipError(f'full_attention: {C} channels do not divide into {nhead} heads')
    D = C // nhead
    as_u8 = lambda m, n: None if m is None else m.reshape(N, n).to(torch.uint8).contiguous()
    q_mask, kv_mask = as_u8(q_mask, L), as_u8(kv_mask, S)
    if D not in (16, 32):
        raise _lib.FarHipError(f'full_attention: head dim {D} has no kernel (16 and 32 do)')
    return N, L, S, C, D, q_mask, kv_mask

def full_attention(q, k, v, nhead, q_mask=None, kv_mask=None):
    """K22: LoFTR's full (softmax) attention core, inference (full_attention_train is the form with gradients).  q: (N, L, C), k, v: (N, S, C) raw fp32 projections (heads
    concatenated, head dim C // nhead in {16, 32}); returns (N, L, C) = softmax_s(q . k / sqrt(D)) v per head, on split-fp16 MFMAs
    with an online softmax (the (N, L, S, H) scores never exist).  Masks (N, L) / (N, S), optional (None = all ones): a masked key
    is selected out (non-finite k / v there never reach an output), a padded query row and every row of an image without a valid
    key are exact zeros.  Operands are split around the thread's activation exponent; a value beyond its range ORs
    ops.overflow_flag (check_activation_range raises)."""
    lib = _lib.load()
    N, L, S, C, D, q_mask, kv_mask = _full_attention_args(q, k, v, nhead, q_mask, kv_mask)
    out = torch.empty(N, L, C, dtype=torch.float32, device=q.device)
    if N == 0 or L == 0:
        return out
    if S == 0:
        return out.zero_()
    ws = _ws(lib.far_full_attention_workspace_bytes(N, L, S, nhead, D), q.device)
    rc = lib.far_full_attention_f16s(_p(q, torch.float32), _p(k, torch.float32), _p(v, torch.float32), N, L, S, nhead, D,
                                     _p(q_mask, torch.uint8), _p(kv_mask, torch.uint8), activation_exponent_value(), _p(out), _p(ws),
                                     _p(overflow_flag(q.device)), _stream())
    _lib.check(rc, 'far_full_attention_f16s')
    return out

class _FullAttentionFn(torch.autograd.Function):
    """K22 with its HIP backward (far_full_attention_train_f16s / far_full_attention_bwd_f16s).  Saved: q, k, v, the output, the
    (N, H, L) row statistic and the masks -- nothing of size (L, S)."""

    @staticmethod
    def forward(ctx, q, k, v, nhead, q_mask, kv_mask):
        lib = _lib.load()
        qc, kc, vc = (t.detach().float().contiguous() for t in (q, k, v))
        N, L, C = qc.shape
        S, D = kc.shape[1], C // nhead
        out = torch.empty(N, L, C, dtype=torch.float32, device=qc.device)
        lse = torch.empty(N, nhead, L, dtype=torch.float32, device=qc.device)
        act_exp = activation_exponent_value()
        if N and L and S:
            ws = _ws(lib.far_full_attention_workspace_bytes(N, L, S, nhead, D), qc.device)
            rc = lib.far_full_attention_train_f16s(_p(qc, torch.float32), _p(kc, torch.float32), _p(vc, torch.float32), N, L, S, nhead, D,
                                                   _p(q_mask, torch.uint8), _p(kv_mask, torch.uint8), act_exp, _p(out), _p(lse), _p(ws),
                                                   _p(overflow_flag(qc.device)), _stream())
            _lib.check(rc, 'far_full_attention_train_f16s')
        else:
            out.zero_()                 # S = 0: no key, exact zeros (as full_attention)
        none = torch.empty(0)
        ctx.save_for_backward(qc, kc, vc, out, lse, q_mask if q_mask is not None else none, kv_mask if kv_mask is not None else none)
        ctx.nhead, ctx.act_exp, ctx.has = nhead, act_exp, (q_mask is not None, kv_mask is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        qc, kc, vc, out, lse, qm, km = ctx.saved_tensors
        dq, dk, dv = full_attention_bwd(qc, kc, vc, out, lse, g, ctx.nhead, qm if ctx.has[0] else None, km if ctx.has[1] else None,
                                        act_exp=ctx.act_exp)
        return dq, dk, dv, None, None, None

def full_attention_bwd(qc, kc, vc, out, lse, g, nhead, q_mask=None, kv_mask=None, act_exp=None):
    """K22 backward: (dq, dk, dv) for the output gradient g, from q, k, v (fp32 contiguous), the output and the (N, H, L) row
    statistic of the training forward (same masks, same activation exponent).  No key (S = 0): zeros."""
    lib = _lib.load()
    N, L, C = qc.shape
    S, D = kc.shape[1], C // nhead
    g = g.float().contiguous()
    dq, dk, dv = torch.empty_like(qc), torch.empty_like(kc), torch.empty_like(vc)
    if not (N and L and S):
        return dq.zero_(), dk.zero_(), dv.zero_()
    ws = _ws(lib.far_full_attention_bwd_workspace_bytes(N, L, S, nhead, D), qc.device)
    rc = lib.far_full_attention_bwd_f16s(_p(qc, torch.float32), _p(kc, torch.float32), _p(vc, torch.float32), _p(out, torch.float32),
                                         _p(lse, torch.float32), _p(g, torch.float32), N, L, S, nhead, D, _p(q_mask, torch.uint8),
                                         _p(kv_mask, torch.uint8), activation_exponent_value() if act_exp is None else act_exp,
                                         _p(dq), _p(dk), _p(dv), _p(ws), _p(overflow_flag(qc.device)), _stream())
    _lib.check(rc, 'far_full_attention_bwd_f16s')
    return dq, dk, dv

def full_attention_train(q, k, v, nhead, q_mask=None, kv_mask=None):
    """K22 with gradients: the arguments, checks, edge cases and output bits of full_attention; (dq, dk, dv) come from the HIP
    backward (recomputed score tiles, nothing of size (L, S) is saved or allocated).  Mask convention for gradients: dk = dv = 0
    at a masked key, dq = 0 at a padded query row (the incoming gradient there is ignored), all zero for an image without a valid key."""
    _, _, _, _, _, q_mask, kv_mask = _full_attention_args(q, k, v, nhead, q_mask, kv_mask)
    return _FullAttentionFn.apply(q, k, v, nhead, q_mask, kv_mask)

def _vit_attention_launch(q, k, v, Z, L, S, nhead, q_strides, kv_strides, plain16=False):
    """far_vit_attention_f16s (plain16: far_vit_attention_f16) on operands whose layout the caller has established (strides in
    floats: image, head, row)."""
    lib = _lib.load()
    _on_gpu(q, k, v)
    _fp32(q, k, v)
    entry = 'far_vit_attention_f16' if plain16 else 'far_vit_attention_f16s'
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        raise NotImplementedError(f'vit_attention (K23, {entry}) is the inference front end: run it under torch.no_grad() '
                                  'or on tensors that need no gradient; ops.vit_attention_train / vit_attention_train_qkv are the '
                                  'forms with the HIP backward' + (' (split-fp16 operands only)' if plain16 else ''))
    out = torch.empty(Z, L, nhead * 64, dtype=torch.float32, device=q.device)
    if Z == 0 or L == 0:
        return out
    if S == 0:
        return out.zero_()
    rc = getattr(lib, entry)(ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(v.data_ptr()), Z, L, S,
                             nhead, 64, *q_strides, *kv_strides, activation_exponent_value(), _p(out),
                             _p(overflow_flag(q.device)), _stream())
    _lib.check(rc, entry)
    return out

def vit_attention(q, k, v, nhead, plain16=False):
    """K23: the softmax self-attention core of the 8-Point-ViT's Blocks, head dim 64 only, no masks, inference only.  q: (Z, L, C),
    k, v: (Z, S, C) fp32 GPU tensors with the heads concatenated (C = nhead * 64; any other head dim raises FarHipError);
    returns (Z, L, C) = softmax_s(q . k / 8) v per head, on split-fp16 MFMAs with an online softmax (the (L, S) scores never
    exist).  Operands are split around the thread's activation exponent; a value beyond its range ORs ops.overflow_flag.  Inputs
    that need gradients raise NotImplementedError (vit_attention_train is the form with gradients).  vit_attention_planes is the
    same kernel on the head planes the qkv Linear writes.  plain16=True: far_vit_attention_f16 -- one fp16 value per operand and per
    probability, fp32 softmax; narrower than the reference (ViTEss.set_precision), same checks and edge cases."""
    Z, L, S, C = _vit_views(q, k, v, nhead, 'vit_attention', other='ops.full_attention')
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return _vit_attention_launch(q, k, v, Z, L, S, nhead, (L * C, 64, C), (S * C, 64, C), plain16=plain16)

def vit_attention_planes(planes, nhead, plain16=False):
    """K23 on the head planes ops.linear_f16s(x, qkv, out_planes=3 * nhead) writes: planes (3 nhead, Z, N, 64) fp32 contiguous --
    plane h is q of head h, nhead + h is k, 2 nhead + h is v (the layout K2 reads in place; no copy here either).  Returns
    (Z, N, nhead * 64) with the heads concatenated: what the `proj` Linear reads.  Checks, refusals and plain16 as vit_attention."""
    _on_gpu(planes)
    if planes.dim() != 4 or planes.shape[0] != 3 * nhead or planes.shape[3] != 64 or not planes.is_contiguous():
        raise _lib.FarHipError(f'vit_attention_planes: planes (3 * nhead, Z, N, 64) contiguous, head dim 64 only (K23); got '
                               f'{tuple(planes.shape)} for {nhead} heads')
    _, Z, N, _ = planes.shape
    st = (N * 64, Z * N * 64, 64)
    return _vit_attention_launch(planes[:nhead], planes[nhead:2 * nhead], planes[2 * nhead:], Z, N, N, nhead, st, st, plain16=plain16)

def _vit_views(q, k, v, nhead, what, other='ops.full_attention_train'):
    """The checks K23's front ends share on (Z, L | S, nhead * 64) fp32 GPU tensors -> (Z, L, S, C); `other`: the op the message
    names for head dims 16 and 32."""
    Z, L, S, C = _qkv_shape(q, k, v, what, 'Z')
    if nhead < 1 or C != nhead * 64:
        raise _lib.FarHipError(f'{what}: head dim 64 only (K23), got {C} channels in {nhead} heads '
                               f'(head dims 16 and 32: {other})')
    _fp32(q, k, v)
    return Z, L, S, C

def _row_strides(t):
    """(image, head, row) strides in floats of a (Z, rows, nhead * 64) view with contiguous rows."""
    if t.numel() and t.stride(2) != 1:
        raise _lib.FarHipError('K23 needs rows of contiguous floats')
    return (t.stride(0), 64, t.stride(1))

def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())

def _vit_train_forward(q, k, v, Z, L, S, nhead):
    """far_vit_attention_train_f16s on views with contiguous rows -> (out (Z, L, C), lse (Z, nhead, L), the activation exponent)."""
    lib = _lib.load()
    out = torch.empty(Z, L, nhead * 64, dtype=torch.float32, device=q.device)
    lse = torch.empty(Z, nhead, L, dtype=torch.float32, device=q.device)
    act_exp = activation_exponent_value()
    if Z and L and S:
        if k.stride() != v.stride():
            raise _lib.FarHipError('K23: k and v must share their strides')
        rc = lib.far_vit_attention_train_f16s(_ptr(q), _ptr(k), _ptr(v), Z, L, S, nhead, 64, *_row_strides(q), *_row_strides(k), act_exp,
                                              _p(out), _p(lse), _p(overflow_flag(q.device)), _stream())
        _lib.check(rc, 'far_vit_attention_train_f16s')
    else:
        out.zero_()                     # no key: exact zeros (as vit_attention)
        lse.zero_()
    return out, lse, act_exp

def vit_attention_bwd(q, k, v, out, lse, g, nhead, act_exp=None, into=None):
    """K23 backward (far_vit_attention_bwd_f16s): (dq, dk, dv) for the output gradient g, from q (Z, L, C), k, v (Z, S, C) -- fp32
    GPU tensors with contiguous rows; the three column slices of one (Z, N, 3 C) projection are read in place --, the output and the
    (Z, nhead, L) row statistic of the training forward (same activation exponent).  into: None (three new contiguous tensors) or one
    (Z, N, 3 C) fp32 contiguous tensor (L = S = N) whose column slices [0, C), [C, 2 C), [2 C, 3 C) the kernels write dq, dk, dv
    into, returned as views of it.  Z = 0, L = 0 or S = 0: zeros."""
    lib = _lib.load()
    Z, L, S, C = _vit_views(q, k, v, nhead, 'vit_attention_bwd')
    _on_gpu(g)
    g = g.float().contiguous()
    if tuple(g.shape) != (Z, L, C) or tuple(out.shape) != (Z, L, C) or tuple(lse.shape) != (Z, nhead, L):
        raise _lib.FarHipError(f'vit_attention_bwd: out, g (Z, L, C) and lse (Z, nhead, L); got {tuple(out.shape)}, {tuple(g.shape)}, '
                               f'{tuple(lse.shape)}')
    if into is None:
        dq = torch.empty(Z, L, C, dtype=torch.float32, device=q.device)
        dk, dv = (torch.empty(Z, S, C, dtype=torch.float32, device=q.device) for _ in range(2))
    else:
        if tuple(into.shape) != (Z, L, 3 * C) or L != S or into.dtype != torch.float32 or not into.is_cuda or not into.is_contiguous():
            raise _lib.FarHipError(f'vit_attention_bwd: `into` must be (Z, N, 3 C) fp32 contiguous on the GPU with L = S = N, got '
                                   f'{tuple(into.shape)}')
        dq, dk, dv = into[..., :C], into[..., C:2 * C], into[..., 2 * C:]
    if not (Z and L and S):
        if into is not None:
            into.zero_()
        else:
            dq.zero_(); dk.zero_(); dv.zero_()
        return dq, dk, dv
    if k.stride() != v.stride():
        raise _lib.FarHipError('K23: k and v must share their strides')
    ws = _ws(lib.far_vit_attention_bwd_workspace_bytes(Z, L, S, nhead, 64), q.device)
    rc = lib.far_vit_attention_bwd_f16s(_ptr(q), _ptr(k), _ptr(v), _p(out, torch.float32), _p(lse, torch.float32), _p(g, torch.float32),
                                        Z, L, S, nhead, 64, *_row_strides(q), *_row_strides(k),
                                        activation_exponent_value() if act_exp is None else act_exp, _ptr(dq), _ptr(dk), _ptr(dv),
                                        *_row_strides(dq), *_row_strides(dk), _p(ws), _p(overflow_flag(q.device)), _stream())
    _lib.check(rc, 'far_vit_attention_bwd_f16s')
    if into is not None:
        _written(into)
    return dq, dk, dv

class _VitAttentionFn(torch.autograd.Function):
    """K23 with its HIP backward (far_vit_attention_train_f16s / far_vit_attention_bwd_f16s).  packed: the one tensor is a
    (Z, N, 3 C) qkv projection read in place, its gradient one (Z, N, 3 C) tensor the kernels write in place; else q, k, v.  Saved:
    q, k, v (or the one qkv tensor), the output, the (Z, H, L) row statistic and the activation exponent -- nothing of size (L, S)."""

    @staticmethod
    def forward(ctx, nhead, packed, *ts):
        ts = tuple(t.detach().contiguous() for t in ts)
        C = nhead * 64
        q, k, v = (ts[0][..., :C], ts[0][..., C:2 * C], ts[0][..., 2 * C:]) if packed else ts
        Z, L, S = q.shape[0], q.shape[1], k.shape[1]
        out, lse, act_exp = _vit_train_forward(q, k, v, Z, L, S, nhead)
        ctx.save_for_backward(*ts, out, lse)
        ctx.nhead, ctx.packed, ctx.act_exp = nhead, packed, act_exp
        return out

    @staticmethod
    def backward(ctx, g):
        *ts, out, lse = ctx.saved_tensors
        C = ctx.nhead * 64
        if ctx.packed:
            qkv = ts[0]
            dqkv = torch.empty_like(qkv)
            vit_attention_bwd(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], out, lse, g, ctx.nhead, ctx.act_exp, into=dqkv)
            return None, None, dqkv
        return (None, None) + tuple(vit_attention_bwd(*ts, out, lse, g, ctx.nhead, ctx.act_exp))

def vit_attention_train(q, k, v, nhead):
    """K23 with gradients: the arguments, checks, edge cases and output bits of vit_attention; (dq, dk, dv) come from the HIP
    backward (recomputed score tiles, nothing of size (L, S) is saved or allocated).  Z = 0, L = 0 or S = 0: zeros with zero
    gradients."""
    _vit_views(q, k, v, nhead, 'vit_attention_train')
    return _VitAttentionFn.apply(nhead, False, q, k, v)

def vit_attention_train_qkv(qkv, nhead):
    """K23 with gradients on one (Z, N, 3 nhead 64) qkv projection, columns t C + h 64 + d (t = 0, 1, 2 for q, k, v: the
    reference's reshape(B, N, 3, H, 64), vision_transformer.py:252): q, k, v are read in place, and the backward returns ONE
    (Z, N, 3 C) gradient that the kernels wrote in place -- no chunk, no cat, no copies.  Returns (Z, N, C), heads concatenated:
    the bits of vit_attention_train on the three column slices."""
    _on_gpu(qkv)
    if qkv.dim() != 3 or nhead < 1 or qkv.shape[2] != 3 * nhead * 64:
        raise _lib.FarHipError(f'vit_attention_train_qkv: qkv (Z, N, 3 * nhead * 64), head dim 64 only (K23); got {tuple(qkv.shape)} '
                               f'for {nhead} heads')
    _fp32(qkv)
    return _VitAttentionFn.apply(nhead, True, qkv)

class _LinearAttentionFn(torch.autograd.Function):
    """K5 with its HIP backward (far_linear_attention_f32 / far_linear_attention_bwd_f32)."""

    @staticmethod
    def forward(ctx, q, k, v, nhead, q_mask, kv_mask, eps):
        qc, kc, vc = (t.detach().float().contiguous() for t in (q, k, v))
        out = linear_attention(qc, kc, vc, nhead, q_mask, kv_mask, eps)
        ctx.save_for_backward(qc, kc, vc, q_mask if q_mask is not None else torch.empty(0), kv_mask if kv_mask is not None else torch.empty(0))
        ctx.nhead, ctx.eps, ctx.has = nhead, eps, (q_mask is not None, kv_mask is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        qc, kc, vc, qm, km = ctx.saved_tensors
        dq, dk, dv = linear_attention_bwd(qc, kc, vc, g, ctx.nhead, qm if ctx.has[0] else None, km if ctx.has[1] else None, ctx.eps)
        return dq, dk, dv, None, None, None, None

def linear_attention_bwd(qc, kc, vc, g, nhead, q_mask=None, kv_mask=None, eps=1e-6):
    """K5 backward: (dq, dk, dv) of linear_attention(qc, kc, vc) for the output gradient g; all (N, L | S, C) fp32 contiguous."""
    lib = _lib.load()
    N, L, C = qc.shape
    S = kc.shape[1]
    D = C // nhead
    g = g.float().contiguous()
    dq, dk, dv = torch.empty_like(qc), torch.empty_like(kc), torch.empty_like(vc)
    if N:
        ws = _ws(lib.far_linear_attention_bwd_workspace_bytes(N, L, S, nhead, D), qc.device)
        rc = lib.far_linear_attention_bwd_f32(_p(qc), _p(kc), _p(vc), _p(g, torch.float32), N, L, S, nhead, D,
                                              _p(q_mask, torch.uint8), _p(kv_mask, torch.uint8), float(eps), _p(dq), _p(dk), _p(dv),
                                              _p(ws), _stream())
        _lib.check(rc, 'far_linear_attention_bwd_f32')
    return dq, dk, dv

def linear_attention_train(q, k, v, nhead, q_mask=None, kv_mask=None, eps=1e-6):
    """K5 with gradients: q (N, L, C), k, v (N, S, C) raw projections -> (N, L, C)."""
    as_u8 = lambda m: None if m is None else m.to(torch.uint8).contiguous()
    return _LinearAttentionFn.apply(q, k, v, nhead, as_u8(q_mask), as_u8(kv_mask), eps)

def layernorm(x, weight, bias, eps=1e-5, residual=None, out=None):
    """K6.  LayerNorm over the last dim (+ residual).  x: (..., C) fp32 contiguous GPU tensor; `out`: optional
    contiguous destination of the same shape (e.g. one half of a buffer that a later stage wants concatenated)."""
    lib = _lib.load()
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x) if out is None else out
    if y.shape != x.shape:
        raise _lib.FarHipError('layernorm: `out` must have the shape of x')
    rc = lib.far_layernorm_f32(_p(x, torch.float32), _p(weight, torch.float32), _p(bias, torch.float32),
                               _p(residual, torch.float32), rows, C, float(eps), _p(y), _stream())
    _lib.check(rc, 'far_layernorm_f32')
    return y if out is None else _written(y)

class _LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the last dimension (+ residual) with gradients (transformer.py:61, 65-67 under autograd): K6 forward,
    far_layernorm_bwd_f32 backward (dx; dgamma / dbeta summed in a fixed order).  The residual's gradient is dy itself."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, residual):
        xc = x.detach().float().contiguous()
        r = None if residual is None else residual.detach().float().contiguous()
        y = layernorm(xc, weight.detach(), bias.detach(), eps, residual=r)
        ctx.save_for_backward(xc, weight)
        ctx.eps, ctx.has_res = float(eps), residual is not None
        return y

    @staticmethod
    def backward(ctx, g):
        xc, weight = ctx.saved_tensors
        g = g.float().contiguous()
        dx, dg, db = layernorm_bwd(xc, weight, g, ctx.eps)
        return dx, dg, db, None, (g if ctx.has_res else None)

def layernorm_bwd(xc, weight, g, eps):
    """K6 backward: (dx, dgamma, dbeta) of LayerNorm(xc; eps) * weight + bias over the last dimension for the output gradient g
    (fp32 contiguous, C % 4 == 0, C <= 1024)."""
    lib = _lib.load()
    C = xc.shape[-1]
    rows = xc.numel() // C
    nb = int(lib.far_layernorm_bwd_ws_bytes(rows, C))
    if nb == 0:
        raise _lib.FarHipError(f'layernorm_bwd: {C} channels not covered (C % 4 == 0, C <= 1024)')
    ws = torch.empty(nb, dtype=torch.uint8, device=xc.device)
    dx = torch.empty_like(xc)
    dgb = torch.empty(2, C, dtype=torch.float32, device=xc.device)
    rc = lib.far_layernorm_bwd_f32(_p(xc, torch.float32), _p(weight.detach().contiguous(), torch.float32), _p(g, torch.float32), rows, C,
                                   float(eps), _p(dx), _p(dgb[0]), _p(dgb[1]), _p(ws), nb, _stream())
    _lib.check(rc, 'far_layernorm_bwd_f32')
    return dx, dgb[0], dgb[1]

USE_HIP_LAYERNORM_TRAIN = True      # False: nn.LayerNorm under autograd (comparison leg of bench.py --workload c3 --vendor-train)

def layernorm_train(x, norm, residual=None):
    """K6 with gradients: norm(x) (+ residual) for an nn.LayerNorm over the last dimension of a GPU tensor; shapes the backward
    kernel does not cover (C % 4 != 0 or C > 1024) use the module itself."""
    C = x.shape[-1]
    if not x.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    if (C & 3) or C > 1024 or norm.weight is None or norm.bias is None or x.numel() == 0 or not USE_HIP_LAYERNORM_TRAIN:
        y = norm(x)
        return y if residual is None else y + residual
    return _LayerNormFn.apply(x, norm.weight, norm.bias, norm.eps, residual)

def linear_attention_apply(q, kv, nhead, S, q_mask=None, eps=1e-6):
    """The second half of K5: q (N, L, nhead * 32) raw projection and the state kv (N, nhead * 32, 33) -> (N, L, nhead * 32)."""
    lib = _lib.load()
    N, L, C = q.shape
    if C != nhead * 32 or tuple(kv.shape) != (N, C, 33):
        raise _lib.FarHipError('linear_attention_apply: q (N, L, nhead * 32), kv (N, nhead * 32, 33)')
    out = torch.empty(N, L, C, dtype=torch.float32, device=q.device)
    if N == 0:
        return out
    rc = lib.far_linear_attention_apply_f32(_p(q, torch.float32), _p(kv, torch.float32), N, L, int(S), nhead, _p(q_mask, torch.uint8),
                                            float(eps), _p(out), _stream())
    _lib.check(rc, 'far_linear_attention_apply_f32')
    return out
