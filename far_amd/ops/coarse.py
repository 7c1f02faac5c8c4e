"""far_amd.ops.coarse: K1: statistics, the coarse matcher, conf_matrix, the sparse-position training form (one family of the torch-tensor front ends for the C ABI in include/far_hip.h; far_amd/ops/__init__.py
re-exports everything under the flat far_amd.ops namespace the rest of the package uses)."""
import ctypes
import os
import threading

import torch

from .. import _lib, flags
from ._base import _p, _stream, _written, _ws, overflow_flag


def dual_softmax_stats(f0, f1, feat_div=1.0, sim_div=1.0, sim_mul=1.0, mask0=None, mask1=None):
    """(rowstat [Z,L,2], colstat [Z,S,2]) = (max, sum-exp) of the similarity matrix along each axis."""
    lib = _lib.load()
    Z, L, C = f0.shape
    S = f1.shape[1]
    ws = _ws(lib.far_dual_softmax_workspace_bytes(Z, L, S), f0.device)
    rowstat = torch.empty(Z, L, 2, dtype=torch.float32, device=f0.device)
    colstat = torch.empty(Z, S, 2, dtype=torch.float32, device=f0.device)
    rc = lib.far_dual_softmax_stats_f32(_p(f0, torch.float32), _p(f1, torch.float32), Z, L, S, C,
                                        feat_div, sim_div, sim_mul, _p(mask0, torch.uint8), _p(mask1, torch.uint8),
                                        _p(rowstat), _p(colstat), _p(ws), _stream())
    _lib.check(rc, 'far_dual_softmax_stats_f32')
    return rowstat, colstat

def coarse_match(f0, f1, temperature, thr, border, hw0, hw1, cell_scale, mask0=None, mask1=None,
                 valid_hw=None, scale0=None, scale1=None, want_conf=False, bf16=False, variant=None, overlap=None):
    """K1.  Returns dict(b_ids, i_ids, j_ids, mconf, mkpts0_c, mkpts1_c, counts, conf_matrix|None).
    variant: 'f32' exact-f32 MFMA (default), 'f16s' split-fp16 operands (fp32-grade), 'bf16' bf16 operands.

    One host synchronisation (reading M) is inherent: the reference's outputs have data-dependent shape
    (torch.where, coarse_matching.py:193).  overlap: a callable that enqueues work which does not depend on the matches; it runs
    between the (asynchronous) copy of the counts and the wait for it, so the GPU has that work to do while the host reads M and
    prepares the launches that depend on it.
    """
    lib = _lib.load()
    Z, L, C = f0.shape
    S = f1.shape[1]
    dev = f0.device
    variant = variant or ('bf16' if bf16 else 'f32')
    fn = {'f32': lib.far_coarse_match_f32, 'bf16': lib.far_coarse_match_bf16, 'f16s': lib.far_coarse_match_f16s}[variant]
    ws = _ws({'f32': lambda: lib.far_dual_softmax_workspace_bytes(Z, L, S),
              'bf16': lambda: lib.far_coarse_match_bf16_workspace_bytes(Z, L, S, C),
              'f16s': lambda: lib.far_coarse_match_f16s_workspace_bytes(Z, L, S, C)}[variant](), dev)
    cap = Z * L
    b_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    i_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    j_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    mconf = torch.empty(cap, dtype=torch.float32, device=dev)
    mk0 = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    mk1 = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    counts = torch.empty(Z + 1, dtype=torch.int32, device=dev)
    conf = torch.empty(Z, L, S, dtype=torch.float32, device=dev) if want_conf else None
    rc = fn(
        _p(f0, torch.float32), _p(f1, torch.float32), Z, L, S, C, float(temperature), float(thr), int(border),
        int(hw0[0]), int(hw0[1]), int(hw1[0]), int(hw1[1]), float(cell_scale),
        _p(mask0, torch.uint8), _p(mask1, torch.uint8), _p(valid_hw, torch.int32),
        _p(scale0, torch.float32), _p(scale1, torch.float32), _p(conf),
        _p(b_ids), _p(i_ids), _p(j_ids), _p(mconf), _p(mk0), _p(mk1),
        _p(counts), ctypes.c_void_p(counts.data_ptr() + 4 * Z), _p(ws),
        *([_p(overflow_flag(dev))] if variant == 'f16s' else []), _stream())
    _lib.check(rc, 'far_coarse_match_' + variant)
    if overlap is None:
        counts_h = counts.cpu()
    else:
        counts_h = torch.empty(Z + 1, dtype=torch.int32, pin_memory=True)
        counts_h.copy_(counts, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        overlap()
        done.synchronize()
    M = int(counts_h[Z])
    return {
        'b_ids': b_ids[:M], 'i_ids': i_ids[:M], 'j_ids': j_ids[:M], 'mconf': mconf[:M],
        'mkpts0_c': mk0[:M], 'mkpts1_c': mk1[:M], 'counts': counts_h[:Z], 'conf_matrix': conf,
    }

def coarse_match_sinkhorn(f0, f1, bin_score, iters, thr, border, hw0, hw1, cell_scale, mask0=None, mask1=None, valid_hw=None,
                          scale0=None, scale1=None, prefilter=False, want_conf=False, want_potentials=False, overlap=None):
    """LoFTR's optimal-transport coarse matcher (match_type 'sinkhorn', coarse_matching.py:120-142) on the split-fp16 operands of K1
    (far_coarse_match_sinkhorn_f16s); C must be 256.  bin_score: a one-element fp32 tensor on the GPU (the module's Parameter), read
    by the kernels -- no host copy.  Returns ops.coarse_match's dict plus conf_matrix_with_bin (Z, L+1, S+1), log_u (Z, L+1) and
    log_v (Z, S+1), each None unless asked for (want_conf / want_potentials); conf_matrix is the [:, :L, :S] view of
    conf_matrix_with_bin.  Host synchronisation and `overlap` as ops.coarse_match."""
    lib = _lib.load()
    Z, L, C = f0.shape
    S = f1.shape[1]
    dev = f0.device
    if not f0.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    if C != 256:
        raise NotImplementedError('the Sinkhorn coarse matcher has a kernel for C = 256 only')
    ws = _ws(lib.far_coarse_match_sinkhorn_f16s_workspace_bytes(Z, L, S, C), dev)
    cap = Z * L
    b_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    i_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    j_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    mconf = torch.empty(cap, dtype=torch.float32, device=dev)
    mk0 = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    mk1 = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    counts = torch.empty(Z + 1, dtype=torch.int32, device=dev)
    conf = torch.empty(Z, L + 1, S + 1, dtype=torch.float32, device=dev) if want_conf else None
    log_u = torch.empty(Z, L + 1, dtype=torch.float32, device=dev) if want_potentials else None
    log_v = torch.empty(Z, S + 1, dtype=torch.float32, device=dev) if want_potentials else None
    bin_score = bin_score.detach()
    if bin_score.dtype != torch.float32 or not bin_score.is_contiguous():
        bin_score = bin_score.float().contiguous()
    rc = lib.far_coarse_match_sinkhorn_f16s(
        _p(f0, torch.float32), _p(f1, torch.float32), Z, L, S, C, _p(bin_score, torch.float32), int(iters), int(bool(prefilter)),
        float(thr), int(border), int(hw0[0]), int(hw0[1]), int(hw1[0]), int(hw1[1]), float(cell_scale),
        _p(mask0, torch.uint8), _p(mask1, torch.uint8), _p(valid_hw, torch.int32), _p(scale0, torch.float32), _p(scale1, torch.float32),
        _p(conf), _p(log_u), _p(log_v), _p(b_ids), _p(i_ids), _p(j_ids), _p(mconf), _p(mk0), _p(mk1),
        _p(counts), ctypes.c_void_p(counts.data_ptr() + 4 * Z), _p(ws), _p(overflow_flag(dev)), _stream())
    _lib.check(rc, 'far_coarse_match_sinkhorn_f16s')
    if overlap is None:
        counts_h = counts.cpu()
    else:
        counts_h = torch.empty(Z + 1, dtype=torch.int32, pin_memory=True)
        counts_h.copy_(counts, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        overlap()
        done.synchronize()
    M = int(counts_h[Z])
    return {
        'b_ids': b_ids[:M], 'i_ids': i_ids[:M], 'j_ids': j_ids[:M], 'mconf': mconf[:M],
        'mkpts0_c': mk0[:M], 'mkpts1_c': mk1[:M], 'counts': counts_h[:Z],
        'conf_matrix': None if conf is None else conf[:, :L, :S], 'conf_matrix_with_bin': conf, 'log_u': log_u, 'log_v': log_v,
    }

def conf_matrix(f0, f1, temperature, mask0=None, mask1=None, out=None):
    """K1, materialising mode: data['conf_matrix'] (Z, L, S) alone (coarse_matching.py:108-118) at HBM write speed
    (far_conf_matrix_f16s: fp32-grade statistics, plain-fp16 scores, exact recomputation of every entry above 2^-12).
    Falls back to the fused split-precision matcher's writer if the exact-entry list overflowed; reading that flag is one
    host synchronisation per call.  With `out=` the result is always in `out` (also after the fallback).
    Returns (conf, listed) with listed = number of entries that were recomputed exactly."""
    lib = _lib.load()
    Z, L, C = f0.shape
    S = f1.shape[1]
    dev = f0.device
    ws = _ws(lib.far_coarse_match_f16s_workspace_bytes(Z, L, S, C), dev)
    conf = torch.empty(Z, L, S, dtype=torch.float32, device=dev) if out is None else out
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    rc = lib.far_conf_matrix_f16s(_p(f0, torch.float32), _p(f1, torch.float32), Z, L, S, C, float(temperature),
                                  _p(mask0, torch.uint8), _p(mask1, torch.uint8), 3, _p(conf, torch.float32), _p(info), _p(ws),
                                  _p(overflow_flag(dev)), _stream())
    _lib.check(rc, 'far_conf_matrix_f16s')
    listed, dropped = (int(v) for v in info.cpu())            # one blocking host read per call (the overflow flag)
    if dropped > 0:           # pathological input (a column with more than 8 non-tiny entries): the exact writer
        hw = (1, L), (1, S)
        exact = coarse_match(f0, f1, temperature, 2.0, 0, hw[0], hw[1], 1.0, mask0, mask1, want_conf=True,
                             variant='f16s')['conf_matrix']
        if out is None:
            return exact, listed
        out.copy_(exact)      # the caller's buffer must hold the result it asked for, not the partially exact one
        return _written(out), listed
    return (conf if out is None else _written(conf)), listed

class _CoarsePosConf(torch.autograd.Function):
    """conf_matrix[b, i, j] at M given positions, differentiable w.r.t. both coarse feature maps, without the dense
    matrix (far_coarse_pos_conf_f16s / far_coarse_pos_conf_bwd_f16)."""

    @staticmethod
    def forward(ctx, f0, f1, pb, pi, pj, temperature):
        lib = _lib.load()
        Z, L, C = f0.shape
        S = f1.shape[1]
        f0c, f1c = f0.detach().float().contiguous(), f1.detach().float().contiguous()
        pb, pi, pj = (t.to(torch.int64).contiguous() for t in (pb, pi, pj))
        M = int(pb.numel())
        ws = _ws(lib.far_coarse_train_workspace_bytes(Z, L, S, C), f0.device)
        p = torch.empty(M, dtype=torch.float32, device=f0.device)
        rc = lib.far_coarse_pos_conf_f16s(_p(f0c, torch.float32), _p(f1c, torch.float32), Z, L, S, C, float(temperature),
                                          _p(pb), _p(pi), _p(pj), M, _p(p), _p(ws), _p(overflow_flag(f0.device)), _stream())
        _lib.check(rc, 'far_coarse_pos_conf_f16s')
        ctx.save_for_backward(f0c, f1c, pb, pi, pj, p, ws)
        ctx.temperature = float(temperature)
        return p

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f0c, f1c, pb, pi, pj, p, ws = ctx.saved_tensors
        Z, L, C = f0c.shape
        S = f1c.shape[1]
        w = (g.float() * p).contiguous()                    # dL/dp * p: bounded for the focal loss even where p -> 0
        df0, df1 = torch.empty_like(f0c), torch.empty_like(f1c)
        rc = lib.far_coarse_pos_conf_bwd_f16(_p(f0c), _p(f1c), Z, L, S, C, ctx.temperature, _p(pb), _p(pi), _p(pj),
                                             int(pb.numel()), _p(w, torch.float32), _p(df0), _p(df1), _p(ws), _stream())
        _lib.check(rc, 'far_coarse_pos_conf_bwd_f16')
        return df0, df1, None, None, None, None

class _CoarseDenseFocal(torch.autograd.Function):
    """The dense-supervision focal loss of the dual-softmax matcher (loftr_loss.py:121-127) as ONE scalar, differentiable w.r.t. both
    coarse feature maps, without conf_matrix or any other L x S tensor (far_coarse_dense_focal_f16s / far_coarse_dense_focal_bwd_f16)."""

    @staticmethod
    def forward(ctx, f0, f1, pb, pi, pj, mask0, mask1, temperature, alpha, gamma, pos_weight, neg_weight, no_gt):
        lib = _lib.load()
        Z, L, C = f0.shape
        S = f1.shape[1]
        dev = f0.device
        f0c, f1c = f0.detach().float().contiguous(), f1.detach().float().contiguous()
        pb, pi, pj = (t.to(torch.int64).contiguous() for t in (pb, pi, pj))
        m0 = None if mask0 is None else mask0.reshape(Z, L).to(torch.uint8).contiguous()
        m1 = None if mask1 is None else mask1.reshape(Z, S).to(torch.uint8).contiguous()
        M = int(pb.numel())
        ws = _ws(lib.far_coarse_dense_focal_workspace_bytes(Z, L, S, C, M), dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ctx.args = (Z, L, S, C, float(temperature))
        ctx.focal = (float(alpha), float(gamma), float(pos_weight), float(neg_weight), int(bool(no_gt)))
        rc = lib.far_coarse_dense_focal_f16s(_p(f0c, torch.float32), _p(f1c, torch.float32), *ctx.args, _p(m0), _p(m1), _p(pb), _p(pi),
                                             _p(pj), M, *ctx.focal, _p(loss), _p(ws), _p(overflow_flag(dev)), _stream())
        _lib.check(rc, 'far_coarse_dense_focal_f16s')
        ctx.save_for_backward(f0c, f1c, pb, pi, pj, ws)
        ctx.masks = (m0, m1)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f0c, f1c, pb, pi, pj, ws = ctx.saved_tensors
        m0, m1 = ctx.masks
        gup = g.detach().float().reshape(1).contiguous()                      # stays on the device: no host read
        df0, df1 = torch.empty_like(f0c), torch.empty_like(f1c)
        rc = lib.far_coarse_dense_focal_bwd_f16(_p(f0c), _p(f1c), *ctx.args, _p(m0), _p(m1), _p(pb), _p(pi), _p(pj), int(pb.numel()),
                                                *ctx.focal, _p(gup, torch.float32), int(DENSE_FOCAL_SPLIT_G), _p(df0), _p(df1), _p(ws),
                                                _stream())
        _lib.check(rc, 'far_coarse_dense_focal_bwd_f16')
        return (df0, df1) + (None,) * 11


# The gradient contraction's G = 2 W - u R - v C as an fp16 hi + lo pair (True) or as one fp16 (False); measured errors of both forms:
# profiles/dense_spvs_parity.txt
DENSE_FOCAL_SPLIT_G = True


def coarse_dense_focal_loss(f0, f1, pb, pi, pj, temperature, alpha, gamma, pos_weight, neg_weight, mask0=None, mask1=None, no_gt=False):
    """K1, training with dense coarse supervision (sparse_spvs = False, dual_softmax, focal: loftr_loss.py:56-75, :121-127): the loss
    over EVERY entry of the (Z, L, S) confidence matrix as a 0-dim fp32 tensor with a HIP backward to both feature maps; positives =
    the labels (pb, pi, pj), negatives = every other entry; mask0 (Z, L) / mask1 (Z, S): the loss weight mask0 x mask1 and the masked
    softmaxes of padded batches.  no_gt: not one ground-truth match (the labels are ignored).  Nothing of size L x S is allocated.
    C must be 256."""
    if not (f0.is_cuda and f1.is_cuda):
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    if f0.shape[-1] != 256:
        raise NotImplementedError('the dense coarse supervision has kernels for C = 256 only')
    if f0.shape[0] == 0 or f0.shape[1] == 0 or f1.shape[1] == 0:
        return (f0.sum() + f1.sum()) * 0.0
    return _CoarseDenseFocal.apply(f0, f1, pb, pi, pj, mask0, mask1, temperature, alpha, gamma, pos_weight, neg_weight, no_gt)


SINKHORN_MAX_ITERS = 48          # far_sinkhorn_pos_conf_*: the 2T terms of a column tile are staged in LDS


class _SinkhornPosConf(torch.autograd.Function):
    """The optimal-transport coupling matrix at M given positions and at its dustbin column / row, differentiable w.r.t. both
    coarse feature maps and bin_score, without the dense matrix (far_sinkhorn_pos_conf_f16s / far_sinkhorn_pos_conf_bwd_f16)."""

    @staticmethod
    def forward(ctx, f0, f1, bin_score, pb, pi, pj, mask0, mask1, iters):
        lib = _lib.load()
        Z, L, C = f0.shape
        S = f1.shape[1]
        dev = f0.device
        f0c, f1c = f0.detach().float().contiguous(), f1.detach().float().contiguous()
        bs = bin_score.detach().float().contiguous()
        pb, pi, pj = (t.to(torch.int64).contiguous() for t in (pb, pi, pj))
        m0 = None if mask0 is None else mask0.reshape(Z, L).to(torch.uint8).contiguous()
        m1 = None if mask1 is None else mask1.reshape(Z, S).to(torch.uint8).contiguous()
        M = int(pb.numel())
        ws = _ws(lib.far_sinkhorn_pos_conf_workspace_bytes(Z, L, S, C, iters), dev)
        p = torch.empty(M, dtype=torch.float32, device=dev)
        bin0 = torch.empty(Z, L, dtype=torch.float32, device=dev)
        bin1 = torch.empty(Z, S, dtype=torch.float32, device=dev)
        rc = lib.far_sinkhorn_pos_conf_f16s(_p(f0c, torch.float32), _p(f1c, torch.float32), Z, L, S, C, _p(bs, torch.float32), iters,
                                            _p(m0), _p(m1), _p(pb), _p(pi), _p(pj), M, _p(p), _p(bin0), _p(bin1), _p(ws),
                                            _p(overflow_flag(dev)), _stream())
        _lib.check(rc, 'far_sinkhorn_pos_conf_f16s')
        ctx.save_for_backward(f0c, f1c, bs, pb, pi, pj, p, bin0, bin1, ws)
        ctx.masks = (m0, m1)
        ctx.iters = iters
        ctx.bin_shape = bin_score.shape
        return p, bin0, bin1

    @staticmethod
    def backward(ctx, g_pos, g_bin0, g_bin1):
        lib = _lib.load()
        f0c, f1c, bs, pb, pi, pj, p, bin0, bin1, ws = ctx.saved_tensors
        m0, m1 = ctx.masks
        Z, L, C = f0c.shape
        S = f1c.shape[1]
        # dL/dp * p = dL/dlogP: bounded for the focal loss even where p -> 0
        w = lambda g, q: torch.zeros_like(q) if g is None else (g.float() * q).contiguous()
        wp, w0, w1 = w(g_pos, p), w(g_bin0, bin0), w(g_bin1, bin1)
        df0, df1 = torch.empty_like(f0c), torch.empty_like(f1c)
        dbin = torch.empty(1, dtype=torch.float32, device=f0c.device)
        rc = lib.far_sinkhorn_pos_conf_bwd_f16(_p(f0c), _p(f1c), Z, L, S, C, _p(bs), ctx.iters, _p(m0), _p(m1), _p(pb), _p(pi), _p(pj),
                                               int(pb.numel()), _p(wp, torch.float32), _p(w0, torch.float32), _p(w1, torch.float32),
                                               _p(df0), _p(df1), _p(dbin), _p(ws), _stream())
        _lib.check(rc, 'far_sinkhorn_pos_conf_bwd_f16')
        return df0, df1, dbin.reshape(ctx.bin_shape), None, None, None, None, None, None


def sinkhorn_pos_conf(f0, f1, bin_score, iters, pb, pi, pj, mask0=None, mask1=None):
    """The optimal-transport matcher on the training path: (conf_pos (M,), conf_bin0 (Z, L), conf_bin1 (Z, S)) = the coupling matrix
    exp(log_assign) of ops.coarse_match_sinkhorn (no prefilter) at the positions (pb, pi, pj), its dustbin column [:, :L, S] and its
    dustbin row [:, L, :S] -- what the sparse loss reads (loftr_loss.py:86-119) -- with a HIP backward to f0, f1 and bin_score (the
    gradient of the unrolled iterations).  mask0 (Z, L) / mask1 (Z, S): padded-mask batches.  C must be 256, iters <= 48."""
    if not (f0.is_cuda and f1.is_cuda and bin_score.is_cuda):
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    Z, L, C = f0.shape
    S = f1.shape[1]
    iters = int(iters)
    if C != 256:
        raise NotImplementedError('the Sinkhorn coarse matcher has kernels for C = 256 only')
    if not 0 <= iters <= SINKHORN_MAX_ITERS:
        raise NotImplementedError(f'training through the Sinkhorn matcher is built for 0 <= skh_iters <= {SINKHORN_MAX_ITERS}')
    if Z == 0 or L == 0 or S == 0:         # nothing to launch: empty results that still hang in the graph
        zero = (f0.sum() + f1.sum() + bin_score.sum()) * 0.0
        return (torch.zeros(int(pb.numel()), device=f0.device) + zero, torch.zeros(Z, L, device=f0.device) + zero,
                torch.zeros(Z, S, device=f0.device) + zero)
    return _SinkhornPosConf.apply(f0, f1, bin_score, pb, pi, pj, mask0, mask1, iters)


class _SinkhornDenseFocal(torch.autograd.Function):
    """The dense-supervision focal loss on the optimal-transport coupling matrix (loftr_loss.py:121-127 on conf = P[:, :L, :S]) as ONE
    scalar, differentiable w.r.t. both coarse feature maps and bin_score, without P or any other L x S tensor
    (far_sinkhorn_dense_focal_f16s / far_sinkhorn_dense_focal_bwd_f16)."""

    @staticmethod
    def forward(ctx, f0, f1, bin_score, pb, pi, pj, mask0, mask1, iters, alpha, gamma, pos_weight, neg_weight, no_gt):
        lib = _lib.load()
        Z, L, C = f0.shape
        S = f1.shape[1]
        dev = f0.device
        f0c, f1c = f0.detach().float().contiguous(), f1.detach().float().contiguous()
        bs = bin_score.detach().float().contiguous()
        m0 = None if mask0 is None else mask0.reshape(Z, L).to(torch.uint8).contiguous()
        m1 = None if mask1 is None else mask1.reshape(Z, S).to(torch.uint8).contiguous()
        if no_gt:
            # loftr_loss.py:65-70: the labels are ignored; in the weighted case the dummy entry (0, 0, 0) leaves the negative term too
            pb = pi = pj = torch.zeros(1 if (m0 is not None or m1 is not None) else 0, dtype=torch.int64, device=dev)
        else:
            pb, pi, pj = (t.to(device=dev, dtype=torch.int64).contiguous() for t in (pb, pi, pj))
        M = int(pb.numel())
        ws = _ws(lib.far_sinkhorn_dense_focal_workspace_bytes(Z, L, S, C, iters, M), dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ctx.args = (Z, L, S, C)
        ctx.iters = iters
        ctx.focal = (float(alpha), float(gamma), float(pos_weight), float(neg_weight), int(bool(no_gt)))
        rc = lib.far_sinkhorn_dense_focal_f16s(_p(f0c, torch.float32), _p(f1c, torch.float32), Z, L, S, C, _p(bs, torch.float32), iters,
                                               _p(m0), _p(m1), _p(pb), _p(pi), _p(pj), M, *ctx.focal, _p(loss), _p(ws),
                                               _p(overflow_flag(dev)), _stream())
        _lib.check(rc, 'far_sinkhorn_dense_focal_f16s')
        ctx.save_for_backward(f0c, f1c, bs, pb, pi, pj, ws)
        ctx.masks = (m0, m1)
        ctx.bin_shape = bin_score.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f0c, f1c, bs, pb, pi, pj, ws = ctx.saved_tensors
        m0, m1 = ctx.masks
        gup = g.detach().float().reshape(1).contiguous()                      # stays on the device: no host read
        df0, df1 = torch.empty_like(f0c), torch.empty_like(f1c)
        dbin = torch.empty(1, dtype=torch.float32, device=f0c.device)
        rc = lib.far_sinkhorn_dense_focal_bwd_f16(_p(f0c), _p(f1c), *ctx.args, _p(bs), ctx.iters, _p(m0), _p(m1), _p(pb), _p(pi), _p(pj),
                                                  int(pb.numel()), *ctx.focal, _p(gup, torch.float32), _p(df0), _p(df1), _p(dbin), _p(ws),
                                                  _stream())
        _lib.check(rc, 'far_sinkhorn_dense_focal_bwd_f16')
        return (df0, df1, dbin.reshape(ctx.bin_shape)) + (None,) * 11


def sinkhorn_dense_focal_loss(f0, f1, bin_score, iters, pb, pi, pj, alpha, gamma, pos_weight, neg_weight, mask0=None, mask1=None,
                              no_gt=False):
    """The optimal-transport matcher trained with dense coarse supervision (match_type 'sinkhorn', sparse_spvs = False, focal:
    loftr_loss.py:56-75, :121-127): the loss over EVERY entry of conf = P[:, :L, :S], P the coupling matrix of
    ops.coarse_match_sinkhorn (no prefilter), as a 0-dim fp32 tensor with a HIP backward to f0, f1 and bin_score (the gradient of the
    unrolled iterations under a dense dloss/dlogP).  Positives = the labels (pb, pi, pj), each one positive term; negatives = every
    other entry; mask0 (Z, L) / mask1 (Z, S): padded batches (loss weight mask0 x mask1).  no_gt: not one ground-truth match (the
    labels are ignored).  Nothing of size L x S is allocated.  C must be 256, 0 <= iters <= 48."""
    if not (f0.is_cuda and f1.is_cuda and bin_score.is_cuda):
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    Z, L, C = f0.shape
    S = f1.shape[1]
    iters = int(iters)
    if C != 256:
        raise NotImplementedError('the Sinkhorn coarse matcher has kernels for C = 256 only')
    if not 0 <= iters <= SINKHORN_MAX_ITERS:
        raise NotImplementedError(f'training through the Sinkhorn matcher is built for 0 <= skh_iters <= {SINKHORN_MAX_ITERS}')
    if Z == 0 or L == 0 or S == 0:         # nothing to launch: a zero that still hangs in the graph
        return (f0.sum() + f1.sum() + bin_score.sum()) * 0.0
    return _SinkhornDenseFocal.apply(f0, f1, bin_score, pb, pi, pj, mask0, mask1, iters, alpha, gamma, pos_weight, neg_weight, no_gt)


def coarse_pos_conf(f0, f1, pb, pi, pj, temperature):
    """K1, training: conf_matrix[pb, pi, pj] (M,) fp32 with a HIP backward to both feature maps; C must be 256."""
    if not f0.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    return _CoarsePosConf.apply(f0, f1, pb, pi, pj, temperature)
