"""far_amd.ops.conv: K9 / K17 / K10 convolutions (inference + training forms), the extractor's K24 / K25 / K26, the Map-free encoder's K27 / K28, BatchNorm K19, FPN upsample-add K8, affine epilogues K7 (one family of the torch-tensor front ends for the C ABI in include/far_hip.h; far_amd/ops/__init__.py
re-exports everything under the flat far_amd.ops namespace the rest of the package uses)."""
import ctypes
import os
import threading

import torch

from .. import _lib, flags
from ._base import _ACT, _p, _same_layout, _stream, _written, activation_exponent_value, grad_scale, overflow_flag
from .packs import PackedConv, PackedConvValid, PackedStemRGB, WINO_MIN_ACT_EXP, WINO_MIN_PIXELS


class _ConvF16sFn(torch.autograd.Function):
    """A bias-free 3x3 / 1x1 convolution (stride 1 or 2, 'same' padding) of the ResNet-FPN backbone with gradients
    (resnet_fpn.py:5-12 conv1x1 / conv3x3 under autograd).  Forward: K9.  dgrad: K9 again -- the transposed convolution of a
    'same' stride-1 convolution is a 'same' stride-1 convolution with the spatially flipped, channel-transposed kernel; for
    stride 2 the output gradient is first spread onto the input grid (zeros in between).  wgrad: far_conv_wgrad_f32 when the
    library has it for the shape, else the vendor's backward-weights.  x, y: (N, C, H, W) logical, channels_last memory."""

    @staticmethod
    def forward(ctx, x, weight, stride, pack, pack_d):
        ks = int(weight.shape[-1])
        xn = x.detach().float().contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)      # NHWC view
        xin = xn if (ks == 3 or stride == 1) else xn[:, ::stride, ::stride].contiguous()                # 1x1 stride 2
        y = conv_nhwc(xin, pack())
        ctx.save_for_backward(xn, weight)
        ctx.stride, ctx.pack_d = int(stride), pack_d
        ctx.act_exp = activation_exponent_value()            # the weight gradient splits xn with the forward's exponent
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        xn, weight = ctx.saved_tensors
        ks, st = int(weight.shape[-1]), ctx.stride
        N, H, W, Cin = xn.shape
        gn = g.float().contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)                # (N, Ho, Wo, Cout)
        dx = dw = None
        # gradients sit anywhere in magnitude: a power-of-two scale from the maximum places them in K9's window (as _LinearF16sFn)
        gs = gn.contiguous()
        sc = grad_scale(gs)
        if ctx.needs_input_grad[0]:
            if st == 1:
                dxn = conv_nhwc(gs, ctx.pack_d(), act_scale_dev=sc)
            elif ks == 3:
                up = torch.zeros(N, H, W, gs.shape[-1], dtype=torch.float32, device=g.device)
                up[:, ::st, ::st] = gs
                dxn = conv_nhwc(up, ctx.pack_d(), act_scale_dev=sc)
            else:
                dxn = torch.zeros(N, H, W, Cin, dtype=torch.float32, device=g.device)
                dxn[:, ::st, ::st] = conv_nhwc(gs, ctx.pack_d(), act_scale_dev=sc)
            dx = dxn.permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            dw = conv_wgrad(xn, gs, ks, st, dy_scale=sc, act_exp=ctx.act_exp)
            if dw is None:                                                                              # shape without a kernel: vendor
                dw = torch.ops.aten.convolution_backward(gn.permute(0, 3, 1, 2), xn.permute(0, 3, 1, 2), weight, None, [st, st],
                                                         [ks // 2, ks // 2], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        return dx, dw, None, None, None

def conv_wgrad(xn, gn, ks, stride, dy_scale=None, act_exp=None, keep=None):
    """K16.  dW (Cout, Cin, ks, ks) of a 'same' bias-free convolution from its NHWC input xn (N, H, W, Cin) and NHWC output
    gradient gn (N, Ho, Wo, Cout); split-fp16 operands, deterministic two-stage sum.  dy_scale = grad_scale(gn) if the caller has
    it already; act_exp: the activation exponent xn was consumed with in the forward (default: the current one).  None only on
    the comparison leg (USE_HIP_WGRAD False)."""
    lib = _lib.load()
    N, H, W, Cin = xn.shape
    Cout = gn.shape[-1]
    if not USE_HIP_WGRAD:
        return None
    xn, gn = xn.contiguous(), gn.contiguous()
    dw = torch.empty(Cout, Cin, ks, ks, dtype=torch.float32, device=xn.device)
    nb = int(lib.far_conv_wgrad_ws_bytes(N, H, W, Cin, Cout, ks, stride))
    ws = torch.empty(nb, dtype=torch.uint8, device=xn.device)
    rc = lib.far_conv_wgrad_f16s(_p(xn, torch.float32), _p(gn, torch.float32), N, H, W, Cin, Cout, ks, stride,
                                 activation_exponent_value() if act_exp is None else int(act_exp),
                                 _p(dy_scale) if dy_scale is not None else None, _p(ws), nb, _p(dw),
                                 overflow_flag(xn.device).data_ptr(), _stream())
    _lib.check(rc, 'far_conv_wgrad_f16s')
    if keep is not None:
        keep += [ws, xn, gn]                     # launched on a side stream: alive until the caller's join
    return dw

USE_HIP_WGRAD = True       # False: the vendor's backward-weights / GEMM (comparison leg of bench.py --workload c3 --vendor-train)

def linear_wgrad(x2, g2, dy_scale=None, act_exp=None, keep=None):
    """K16 as a Linear layer's weight gradient: dW (N_out, K) = g2^T x2 for x2 (rows, K), g2 (rows, N_out); None -> caller's GEMM
    (comparison leg only)."""
    rows, K = x2.shape
    if not USE_HIP_WGRAD or rows == 0:
        return None
    h = rows // 32 if rows % 32 == 0 else 1                     # 1x1 kernel: any factoring of the rows into H x W is the same sum
    return conv_wgrad(x2.reshape(1, h, rows // h, K), g2.reshape(1, h, rows // h, g2.shape[1]), 1, 1, dy_scale, act_exp, keep).reshape(g2.shape[1], K)

def conv_train(x, weight, stride, cache, name, split=True):
    """K9 convolution with gradients.  x (N, Cin, H, W) fp32 GPU; weight (Cout, Cin, k, k), k in {1, 3}; cache: a PackCache."""
    if not x.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    ks = int(weight.shape[-1])
    re = lambda pc: pc.refresh(weight)                 # after an optimizer step: same buffers, one launch (the forward image first:
    pack = lambda: cache.get((name, 'fwd', split), [weight], lambda: PackedConv(weight, split=split, stride=stride if ks == 3 else 1), refresh=re)
    pack_d = lambda: cache.get((name, 'dgrad', split), [weight],   # the dgrad image borrows its scale; the forward ran before the backward)
                               lambda: PackedConv(weight, split=split, dgrad=True, pack_scale=pack().pack_scale),
                               refresh=re).follow_scale(pack(), weight)
    return _ConvF16sFn.apply(x, weight, int(stride), pack, pack_d)

def affine_act(x, scale, shift, residual=None, act='relu', slope=0.01, inplace=True):
    """K7.  y = act(x * scale[c] + shift[c] (+ residual)) for x (N, C, H, W) in NCHW or channels_last memory."""
    lib = _lib.load()
    N, C, H, W = x.shape
    lay, ts = _same_layout([x] + ([residual] if residual is not None else []))
    x = ts[0]
    residual = ts[1] if residual is not None else None
    if (lay == 0 and (H * W) % 4) or (lay == 1 and C % 4):
        raise _lib.FarHipError('affine_act needs HW % 4 == 0 (NCHW) or C % 4 == 0 (channels_last)')
    y = x if inplace else torch.empty_like(x)
    code = {'none': 0, 'relu': 1, 'leaky': 2}[act]
    rc = lib.far_affine_act_f32(ctypes.c_void_p(x.data_ptr()), _p(scale, torch.float32), _p(shift, torch.float32),
                                ctypes.c_void_p(residual.data_ptr() if residual is not None else 0),
                                N, C, H * W, lay, code, float(slope), ctypes.c_void_p(y.data_ptr()), _stream())
    _lib.check(rc, 'far_affine_act_f32')
    return _written(y) if inplace else y

def upsample2x_add(lo, hi):
    """K8.  hi + F.interpolate(lo, scale_factor=2, mode='bilinear', align_corners=True)."""
    lib = _lib.load()
    N, C, h, w = lo.shape
    if tuple(hi.shape) != (N, C, 2 * h, 2 * w):
        raise _lib.FarHipError(f'upsample2x_add shape mismatch {tuple(lo.shape)} vs {tuple(hi.shape)}')
    lay, (hi, lo) = _same_layout([hi, lo])
    out = torch.empty_like(hi)
    rc = lib.far_upsample2x_add_f32(ctypes.c_void_p(lo.data_ptr()), ctypes.c_void_p(hi.data_ptr()), N, h, w, C, lay,
                                    ctypes.c_void_p(out.data_ptr()), _stream())
    _lib.check(rc, 'far_upsample2x_add_f32')
    return out

class _BatchNormActFn(torch.autograd.Function):
    """act(bn(x) (+ residual)) with BATCH statistics and gradients (resnet_fpn.py:24-41, 60-62, 75-91 under autograd, nn.BatchNorm2d
    in training mode): K19 statistics + K7 normalise / activate / add forward, far_bn_train_bwd_f32 backward; deterministic.
    Tensors (N, C, H, W) logical, channels_last memory.  The running statistics of `bn` are updated as the module does."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn, act, slope, residual):
        lib = _lib.load()
        cl = torch.channels_last
        xc = x.detach().contiguous(memory_format=cl)
        N, C, H, W = xc.shape
        M = N * H * W
        nb = int(lib.far_bn_train_ws_bytes(M, C))
        buf = torch.empty(4 * C + nb // 4, dtype=torch.float32, device=xc.device)     # { scale, shift, mean, rstd } + partial sums
        y = torch.empty_like(xc)
        track = bn.track_running_stats and bn.running_mean is not None
        r = None if residual is None else residual.detach().contiguous(memory_format=cl)
        vp = buf.data_ptr()
        rc = lib.far_bn_act_train_fwd_f32(xc.data_ptr(), 0 if r is None else r.data_ptr(), M, C,
                                          0 if weight is None else weight.data_ptr(), 0 if bias is None else bias.data_ptr(), float(bn.eps),
                                          float(bn.momentum), bn.running_mean.data_ptr() if track else 0,
                                          bn.running_var.data_ptr() if track else 0, _ACT[act], float(slope), y.data_ptr(), vp,
                                          vp + 16 * C, nb, _stream())
        _lib.check(rc, 'far_bn_act_train_fwd_f32')
        if track:
            bn.num_batches_tracked += 1
            _written(bn.running_mean)                # K19 updated them through raw pointers: the inference image folded from the
            _written(bn.running_var)                 # old statistics (PackCache stamps on their versions) must not be reused
        ctx.save_for_backward(xc, y, buf, weight)
        ctx.act, ctx.slope, ctx.has_res, ctx.nb = _ACT[act], float(slope), residual is not None, nb
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        xc, y, buf, weight = ctx.saved_tensors
        N, C, H, W = xc.shape
        M = N * H * W
        gc = g.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(xc)
        dres = torch.empty_like(xc) if ctx.has_res else None
        dgb = torch.empty(2, C, dtype=torch.float32, device=xc.device)
        vp = buf.data_ptr()
        rc = lib.far_bn_train_bwd_f32(xc.data_ptr(), gc.data_ptr(), y.data_ptr(), vp + 8 * C, vp + 12 * C,
                                      0 if weight is None else weight.data_ptr(), M, C, ctx.act, ctx.slope, dx.data_ptr(), dgb.data_ptr(),
                                      dgb.data_ptr() + 4 * C, 0 if dres is None else dres.data_ptr(), vp + 16 * C, ctx.nb, _stream())
        _lib.check(rc, 'far_bn_train_bwd_f32')
        return (dx, dgb[0] if weight is not None else None, dgb[1] if weight is not None else None, None, None, None, dres)

USE_HIP_BATCHNORM_TRAIN = not flags.off('FAR_NO_BN')      # False: nn.BatchNorm2d + torch activations under autograd (comparison leg, --vendor-train)

USE_HIP_SYNC_BATCHNORM = False       # True: torch.nn.SyncBatchNorm modules in training mode run K19's synchronised form (opt-in:
                                     # LoFTR.set_sync_batchnorm_training; process-wide, and it must be set alike on every rank)

def _cl(t):
    """(N, C, H, W) fp32 GPU tensor in channels_last memory, as [M][C] for the K19 entry points."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise _lib.FarHipError('the BatchNorm kernels need fp32 GPU (N, C, H, W) tensors')
    t = t.detach().contiguous(memory_format=torch.channels_last)
    if t.numel() == 0:
        raise _lib.FarHipError('the synchronised BatchNorm kernels need at least one pixel on every rank')
    return t

def _ws_f32(nbytes, device):
    """K19's partial-sum scratch (far_bn_train_ws_bytes: a multiple of four bytes)."""
    return torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=device)

def sync_bn_moments(x, out=None):
    """K19, synchronised form, stage 1 (no collective): this rank's record { n, sum x, sum x^2 } as a (3, C) float64 tensor (`out`: a
    contiguous (3, C) float64 slot to write it into, e.g. row `rank` of the (W, 3, C) exchange buffer)."""
    lib = _lib.load()
    xc = _cl(x)
    N, C, H, W = xc.shape
    M = N * H * W
    rec = torch.empty(3, C, dtype=torch.float64, device=xc.device) if out is None else out
    nb = int(lib.far_bn_train_ws_bytes(M, C))
    ws = _ws_f32(nb, xc.device)
    _lib.check(lib.far_bn_sync_moments_f32(xc.data_ptr(), M, C, _p(rec, torch.float64), ws.data_ptr(), nb, _stream()), 'far_bn_sync_moments_f32')
    return rec if out is None else _written(rec)

def sync_bn_stats(recs, weight=None, bias=None, eps=1e-5, momentum=0.1, running_mean=None, running_var=None):
    """Stage 2 (no collective): the stacked records (W, 3, C) float64 of all ranks, added in rank order -> a float32 vector of 4 C + 4
    entries { scale, shift, mean, rstd, 1 / total count }; running_mean / running_var are updated in place as the module does
    (momentum, unbiased variance over the total count).  Every rank that passes the same bytes gets the same bits."""
    lib = _lib.load()
    if recs.dim() != 3 or recs.shape[1] != 3:
        raise _lib.FarHipError('sync_bn_stats expects the records as a (W, 3, C) float64 tensor')
    W, _, C = recs.shape
    vec = torch.empty(4 * C + 4, dtype=torch.float32, device=recs.device)
    rc = lib.far_bn_sync_stats_f32(_p(recs, torch.float64), W, C, _p(weight, torch.float32), _p(bias, torch.float32), float(eps), float(momentum),
                                   _p(running_mean, torch.float32), _p(running_var, torch.float32), _p(vec), _stream())
    _lib.check(rc, 'far_bn_sync_stats_f32')
    _written(running_mean)
    _written(running_var)
    return vec

def sync_bn_apply(x, vec, act='none', slope=0.01, residual=None):
    """Stage 3: y = act(x scale + shift (+ residual)) with the vector of sync_bn_stats; channels_last memory."""
    lib = _lib.load()
    xc = _cl(x)
    N, C, H, W = xc.shape
    r = None if residual is None else _cl(residual)
    if vec.numel() != 4 * C + 4 or (r is not None and r.shape != xc.shape):
        raise _lib.FarHipError('sync_bn_apply: the statistics vector or the residual does not fit x')
    y = torch.empty_like(xc)
    rc = lib.far_bn_sync_apply_f32(xc.data_ptr(), 0 if r is None else r.data_ptr(), N * H * W, C, _p(vec, torch.float32), _ACT[act], float(slope),
                                   y.data_ptr(), _stream())
    _lib.check(rc, 'far_bn_sync_apply_f32')
    return y

def sync_bn_bwd_sums(x, dy, y, vec, act='none', slope=0.01, out=None):
    """Backward stage 1 (no collective): this rank's record { sum g, sum g xhat } as (2, C) float64 (g = dy act'(y), xhat from the global
    statistics in vec), and the same sums in fp32 as this rank's (dgamma, dbeta).  Returns (rec, dgamma, dbeta)."""
    lib = _lib.load()
    xc, gc, yc = _cl(x), _cl(dy), _cl(y)
    N, C, H, W = xc.shape
    M = N * H * W
    if vec.numel() != 4 * C + 4 or gc.shape != xc.shape or yc.shape != xc.shape:
        raise _lib.FarHipError('sync_bn_bwd_sums: the statistics vector, dy or y does not fit x')
    rec = torch.empty(2, C, dtype=torch.float64, device=xc.device) if out is None else out
    dgb = torch.empty(2, C, dtype=torch.float32, device=xc.device)
    nb = int(lib.far_bn_train_ws_bytes(M, C))
    ws = _ws_f32(nb, xc.device)
    rc = lib.far_bn_sync_bwd_sums_f32(xc.data_ptr(), gc.data_ptr(), yc.data_ptr(), _p(vec, torch.float32), M, C, _ACT[act], float(slope),
                                      _p(rec, torch.float64), dgb.data_ptr(), dgb.data_ptr() + 4 * C, ws.data_ptr(), nb, _stream())
    _lib.check(rc, 'far_bn_sync_bwd_sums_f32')
    return (rec if out is None else _written(rec)), dgb[0], dgb[1]

def sync_bn_bwd_dx(x, dy, y, vec, weight, recs, act='none', slope=0.01, want_dres=False):
    """Backward stage 2: the stacked records (W, 2, C) float64, added in rank order -> dx = gamma rstd (g - S_g / M - xhat S_gx / M) with
    the global sums and the global count; returns (dx, dres) with dres = g when want_dres, else None."""
    lib = _lib.load()
    xc, gc, yc = _cl(x), _cl(dy), _cl(y)
    N, C, H, W = xc.shape
    if recs.dim() != 3 or tuple(recs.shape[1:]) != (2, C) or vec.numel() != 4 * C + 4 or gc.shape != xc.shape or yc.shape != xc.shape:
        raise _lib.FarHipError('sync_bn_bwd_dx: the records, the statistics vector, dy or y do not fit x')
    dx = torch.empty_like(xc)
    dres = torch.empty_like(xc) if want_dres else None
    sums = torch.empty(2 * C, dtype=torch.float32, device=xc.device)
    rc = lib.far_bn_sync_bwd_dx_f32(xc.data_ptr(), gc.data_ptr(), yc.data_ptr(), _p(vec, torch.float32), _p(weight, torch.float32),
                                    _p(recs, torch.float64), recs.shape[0], N * H * W, C, _ACT[act], float(slope), dx.data_ptr(),
                                    0 if dres is None else dres.data_ptr(), sums.data_ptr(), _stream())
    _lib.check(rc, 'far_bn_sync_bwd_dx_f32')
    return dx, dres

def _exchange(rec_fn, K, C, device, group, world, rank):
    """Every rank's (K, C) float64 record on every rank, as (W, K, C): each rank writes its record into its own slot of a zeroed
    buffer, one all_reduce(SUM) adds the buffers -- adding zeros is exact, so every record arrives unchanged whatever order the
    backend reduces in (RCCL and gloo alike)."""
    buf = torch.zeros(world, K, C, dtype=torch.float64, device=device)
    out = rec_fn(buf[rank])
    torch.distributed.all_reduce(buf, op=torch.distributed.ReduceOp.SUM, group=group)
    return buf, out

class _SyncBatchNormActFn(torch.autograd.Function):
    """act(bn(x) (+ residual)) for a torch.nn.SyncBatchNorm in training mode (mp3d_loftr/train.py:342): K19's synchronised form -- the five
    sync_bn_* stages with one all_reduce in the forward ({ n, sum x, sum x^2 } of every rank) and one in the backward ({ sum g,
    sum g xhat }).  dgamma / dbeta stay per rank (DistributedDataParallel averages them), as with torch's module."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn, act, slope, residual, group, world, rank):
        xc = _cl(x)
        C = xc.shape[1]
        track = bn.track_running_stats and bn.running_mean is not None
        recs, _ = _exchange(lambda slot: sync_bn_moments(xc, out=slot), 3, C, xc.device, group, world, rank)
        vec = sync_bn_stats(recs, weight, bias, bn.eps, bn.momentum, bn.running_mean if track else None, bn.running_var if track else None)
        y = sync_bn_apply(xc, vec, act, slope, residual)
        if track:
            bn.num_batches_tracked += 1
        ctx.save_for_backward(xc, y, vec, weight)
        ctx.act, ctx.slope, ctx.has_res, ctx.pg = act, float(slope), residual is not None, (group, world, rank)
        return y

    @staticmethod
    def backward(ctx, g):
        xc, y, vec, weight = ctx.saved_tensors
        C = xc.shape[1]
        gc = g.contiguous(memory_format=torch.channels_last)
        recs, (_, dgamma, dbeta) = _exchange(lambda slot: sync_bn_bwd_sums(xc, gc, y, vec, ctx.act, ctx.slope, out=slot), 2, C, xc.device, *ctx.pg)
        dx, dres = sync_bn_bwd_dx(xc, gc, y, vec, weight, recs, ctx.act, ctx.slope, want_dres=ctx.has_res)
        return (dx, dgamma if weight is not None else None, dbeta if weight is not None else None, None, None, None, dres, None, None, None)

def _sync_group(bn):
    """(process group, world size, rank) of a SyncBatchNorm module; (None, 1, 0) without an initialised process group."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized()):
        return None, 1, 0
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group, dist.get_world_size(group), dist.get_rank(group)

def bn_act_train(x, bn, act='none', slope=0.01, residual=None, force_exchange=False):
    """K19.  act(bn(x) (+ residual)) for an nn.BatchNorm2d in TRAINING mode (batch statistics) on a GPU tensor, with gradients;
    what the kernels do not cover (eval-mode modules, momentum None, C % 4 != 0, C > 1024) runs the module and torch activations.
    With USE_HIP_SYNC_BATCHNORM a torch.nn.SyncBatchNorm takes the synchronised form: statistics over all ranks of the module's
    process_group, one all_reduce forward and one backward; at world size 1 (or without a process group) no collective is issued
    and the call is the plain one, as with torch's module.  Whether such a module runs here depends only on what is equal on every
    rank (the switch, the module's configuration, C, dtype): a rank-local obstacle (an empty shard) raises instead of leaving the
    other ranks alone in the collective.  force_exchange: run the exchange at world size 1 too (a test aid)."""
    if not x.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    C = x.shape[1]
    sync = USE_HIP_SYNC_BATCHNORM and type(bn) is torch.nn.SyncBatchNorm
    if (not USE_HIP_BATCHNORM_TRAIN or not (type(bn) is torch.nn.BatchNorm2d or sync) or not bn.training or bn.momentum is None or (C & 3) or C > 1024
            or x.dtype != torch.float32 or x.dim() != 4 or (x.numel() == 0 and not sync) or (bn.weight is None) != (bn.bias is None)):
        y = bn(x)
        if residual is not None:
            y = y + residual
        return torch.relu(y) if act == 'relu' else (torch.nn.functional.leaky_relu(y, slope) if act == 'leaky' else y)
    if sync:
        if x.numel() == 0:
            raise _lib.FarHipError('SyncBatchNorm on the HIP kernels needs at least one pixel on every rank (an empty shard cannot fall '
                                   'back to the module: the other ranks are already in the collective)')
        group, world, rank = _sync_group(bn)
        if world > 1 or (force_exchange and group is not None):
            return _SyncBatchNormActFn.apply(x, bn.weight, bn.bias, bn, act, slope, residual, group, world, rank)
    return _BatchNormActFn.apply(x, bn.weight, bn.bias, bn, act, slope, residual)

class _Upsample2xAddFn(torch.autograd.Function):
    """hi + F.interpolate(lo, scale_factor=2, mode='bilinear', align_corners=True) with gradients (resnet_fpn.py:108-109,
    :113-114 under autograd): forward K8, backward far_upsample2x_bwd_f32 -- a gather in a fixed order, where the node torch
    records for F.interpolate scatters with atomics (the one source of run-to-run differences in the backbone gradients)."""

    @staticmethod
    def forward(ctx, lo, hi):
        cl = torch.channels_last
        return upsample2x_add(lo.detach().contiguous(memory_format=cl), hi.detach().contiguous(memory_format=cl))

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        N, C, H, W = g.shape
        dlo = None
        if ctx.needs_input_grad[0]:
            gn = g.float().contiguous(memory_format=torch.channels_last)
            dlo = torch.empty(N, C, H // 2, W // 2, dtype=torch.float32, device=g.device, memory_format=torch.channels_last)
            rc = lib.far_upsample2x_bwd_f32(ctypes.c_void_p(gn.data_ptr()), N, H // 2, W // 2, C, ctypes.c_void_p(dlo.data_ptr()),
                                            _stream())
            _lib.check(rc, 'far_upsample2x_bwd_f32')
        return dlo, (g if ctx.needs_input_grad[1] else None)

def upsample2x_add_train(lo, hi):
    """K8 with gradients; lo (N, C, h, w), hi (N, C, 2h, 2w) fp32 GPU, C % 4 == 0."""
    return _Upsample2xAddFn.apply(lo, hi)

USE_WINO = not flags.off('FAR_NO_WINO')      # inference 3x3 stride-1 layers on K17 (conv_nhwc dispatches); False: K9 everywhere

def conv3x3_wino(x, pw, residual=None, act='none', slope=0.01, out=None):
    """K17.  x (N, H, W, Cin) fp32 contiguous -> act(conv3x3(x) * scale + shift (+ residual)) as (N, H, W, Cout): conv_nhwc's
    result for a stride-1 3x3 layer, on the Winograd kernel."""
    lib = _lib.load()
    N, H, W, Cin = x.shape
    if Cin != pw.Cin:
        raise _lib.FarHipError(f'conv3x3_wino: input has {Cin} channels, weights expect {pw.Cin}')
    shape = (N, H, W, pw.Cout)
    if out is None:
        y = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        y = out
        if y.numel() != N * H * W * pw.Cout or not y.is_contiguous() or y.dtype != torch.float32:
            raise _lib.FarHipError('conv3x3_wino: `out` must be a contiguous fp32 tensor of the output size')
    if residual is not None and (residual.numel() != y.numel() or not residual.is_contiguous()):
        raise _lib.FarHipError('conv3x3_wino: `residual` must be a contiguous tensor of the output size')
    ptr = lambda t: _p(t, torch.float32).value
    d = _lib.ConvDesc(x=ptr(x), x2=None, packed=_p(pw.packed).value, scale=ptr(pw.scale), shift=ptr(pw.shift), res=ptr(residual),
                      ln_gamma=None, ln_beta=None, post_res=None, up=None, y=ptr(y), N=N, H=H, W=W, Cin=Cin, Cin1=Cin, Cout=pw.Cout,
                      ksize=3, stride=1, act=_ACT[act], split=1, out_planes=1, res_group=1, slope=float(slope), ln_eps=0.0,
                      act_exp=max(activation_exponent_value(), 0), overflow=overflow_flag(x.device).data_ptr(), act_scale_dev=None)
    _lib.check(lib.far_conv3x3_wino_f32(ctypes.byref(d), _stream()), 'far_conv3x3_wino_f32')
    return y if out is None else _written(y)

def conv_nhwc(x, pc, residual=None, act='none', slope=0.01, x2=None, out_planes=1, res_group=1, ln=None,
              post_residual=None, out=None, up=None, act_scale_dev=None, in_stride=1):
    """K9.  x (N, H, W, Cin) fp32 contiguous -> act(conv(x) * scale + shift (+ residual)) as (N, H, W, Cout).
    With x2 (N, H, W, C2) the convolution input is cat([x, x2], -1), read in place.  out_planes = P > 1 returns
    (P, N, H, W, Cout / P): the output channels split into P separate contiguous tensors.
    up (N, H/2, W/2, Cout), 1x1 convolutions: + F.interpolate(up, scale_factor=2, bilinear, align_corners=True)
    in the epilogue (the FPN merge).  in_stride = 2 (1x1 weights): the convolution of x[:, ::2, ::2] read in place -- the
    down-sampling shortcut of a BasicBlock (resnet_fpn.py:26-29) without the subsampled copy."""
    lib = _lib.load()
    N, H, W, Cin1 = x.shape
    if in_stride not in (1, 2) or (in_stride == 2 and (pc.ksize != 1 or pc.stride != 1 or x2 is not None or up is not None or res_group != 1)):
        raise _lib.FarHipError('conv_nhwc: in_stride = 2 is the in-place subsampling of a plain 1x1 convolution')
    if (USE_WINO and pc.ksize == 3 and pc.stride == 1 and pc.split and x2 is None and out_planes == 1 and res_group == 1 and ln is None
            and post_residual is None and up is None and act_scale_dev is None and not torch.is_grad_enabled()
            and activation_exponent_value() >= WINO_MIN_ACT_EXP and H * W >= WINO_MIN_PIXELS and H * W * pc.Cout < 2 ** 31):
        pw = pc.wino()
        if pw is not None:
            # K17 (Winograd F(2x2, 3x3)): 1.03-1.26x K9 on the backbone's stride-1 3x3 layers at one third of its error
            return conv3x3_wino(x, pw, residual=residual, act=act, slope=slope, out=out)
    if up is not None and (tuple(up.shape) != (N, H // 2, W // 2, pc.Cout) or not up.is_contiguous()):
        raise _lib.FarHipError(f'conv_nhwc: `up` must be a contiguous ({N}, {H // 2}, {W // 2}, {pc.Cout}) tensor')
    Cin = Cin1 + (x2.shape[-1] if x2 is not None else 0)
    if Cin != pc.Cin or (x2 is not None and tuple(x2.shape[:3]) != (N, H, W)):
        raise _lib.FarHipError(f'conv_nhwc: input has {Cin} channels, weights expect {pc.Cin}')
    st = pc.stride * in_stride
    if pc.Cout % out_planes:
        raise _lib.FarHipError('conv_nhwc: out_planes must divide the output channel count')
    shape = (N, (H - 1) // st + 1, (W - 1) // st + 1, pc.Cout // out_planes)
    full = (out_planes,) + shape if out_planes > 1 else shape
    if out is None:
        y = torch.empty(full, dtype=torch.float32, device=x.device)
    else:
        y = out
        n_out = 1
        for d in full:
            n_out *= d
        if y.numel() != n_out or not y.is_contiguous() or y.dtype != torch.float32:
            raise _lib.FarHipError('conv_nhwc: `out` must be a contiguous fp32 tensor of the output size')
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    ptr = lambda t: _p(t, torch.float32).value
    d = _lib.ConvDesc(x=ptr(x), x2=ptr(x2), packed=_p(pc.packed).value, scale=ptr(pc.scale), shift=ptr(pc.shift),
                      res=ptr(residual), ln_gamma=ptr(g), ln_beta=ptr(b), post_res=ptr(post_residual), up=ptr(up), y=ptr(y),
                      N=N, H=H, W=W, Cin=Cin, Cin1=Cin1, Cout=pc.Cout, ksize=pc.ksize, stride=st, act=_ACT[act],
                      split=int(pc.split), out_planes=int(out_planes), res_group=int(res_group), slope=float(slope),
                      ln_eps=float(eps), act_exp=activation_exponent_value(), overflow=overflow_flag(x.device).data_ptr(),
                      act_scale_dev=None if act_scale_dev is None else act_scale_dev.data_ptr())
    rc = lib.far_conv_nhwc_f32(ctypes.byref(d), _stream())
    _lib.check(rc, 'far_conv_nhwc_f32')
    return y if out is None else _written(y)

def stem7x7(img, weight, scale=None, shift=None):
    """K10.  img (N, 1, H, W) fp32 -> relu(bn(conv7x7 stride 2)) as NHWC (N, H/2, W/2, Cout); without scale / shift the bare
    convolution (training: BatchNorm follows with batch statistics)."""
    lib = _lib.load()
    N, one, H, W = img.shape
    Cout = weight.shape[0]
    if one != 1 or tuple(weight.shape[1:]) != (1, 7, 7):
        raise _lib.FarHipError('stem7x7 expects a 1-channel image and a (Cout, 1, 7, 7) weight')
    y = torch.empty(N, (H + 1) // 2, (W + 1) // 2, Cout, dtype=torch.float32, device=img.device)
    rc = lib.far_stem7x7_nhwc_f32(_p(img.contiguous(), torch.float32), _p(weight.detach().contiguous(), torch.float32),
                                  _p(scale, torch.float32) if scale is not None else None,
                                  _p(shift, torch.float32) if shift is not None else None, N, H, W, Cout, _p(y), _stream())
    _lib.check(rc, 'far_stem7x7_nhwc_f32')
    return y

class _StemFn(torch.autograd.Function):
    """The stem convolution with its weight gradient (resnet_fpn.py:60 under autograd; the image needs no gradient): K10 forward
    without the BatchNorm fold, far_stem7x7_wgrad_f32 backward.  Returns (N, Cout, H/2, W/2) logical, channels_last memory."""

    @staticmethod
    def forward(ctx, img, weight):
        img = img.detach().float().contiguous()
        ctx.save_for_backward(img)
        return stem7x7(img, weight).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        img, = ctx.saved_tensors
        lib = _lib.load()
        N, _, H, W = img.shape
        gn = g.float().contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).contiguous()
        Cout = gn.shape[-1]
        nb = int(lib.far_stem7x7_wgrad_ws_bytes(N, H, W, Cout))
        ws = torch.empty(nb, dtype=torch.uint8, device=img.device)
        dw = torch.empty(Cout, 1, 7, 7, dtype=torch.float32, device=img.device)
        rc = lib.far_stem7x7_wgrad_f32(_p(img, torch.float32), _p(gn, torch.float32), N, H, W, Cout, _p(ws), nb, _p(dw), _stream())
        _lib.check(rc, 'far_stem7x7_wgrad_f32')
        return None, dw

def stem_train(img, weight):
    """K10 with the weight gradient: img (N, 1, H, W) fp32 GPU, weight (Cout, 1, 7, 7) -> conv7x7 stride 2 (no BN, no ReLU)."""
    if not img.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    return _StemFn.apply(img, weight)

def conv_valid(x, pack, residual=None, act='none'):
    """K24.  x (N, H, W, Cin) fp32 contiguous -> act(conv5x5_valid(x) * scale + shift (+ residual)) as (N, H - 4, W - 4, Cout) for a
    PackedConvValid; act 'none' or 'relu'; residual in the output's layout.  Takes part in the activation-range guard as K9 does.
    A pack built with split=False runs far_conv_valid_f16 (plain fp16 operands, narrower than the reference) -- the same contract."""
    lib = _lib.load()
    if not isinstance(pack, PackedConvValid):
        raise _lib.FarHipError('conv_valid takes a PackedConvValid')
    if x.dim() != 4 or x.shape[-1] != pack.Cin:
        raise _lib.FarHipError(f'conv_valid: input of shape {tuple(x.shape)}, weights expect (N, H, W, {pack.Cin})')
    N, H, W, Cin = x.shape
    k = pack.ksize
    if H < k or W < k:
        raise _lib.FarHipError(f'conv_valid: a {H} x {W} input is smaller than the {k} x {k} kernel')
    if act not in ('none', 'relu'):
        raise _lib.FarHipError("conv_valid: act is 'none' or 'relu'")
    y = torch.empty(N, H - k + 1, W - k + 1, pack.Cout, dtype=torch.float32, device=x.device)
    if residual is not None and (tuple(residual.shape) != tuple(y.shape) or not residual.is_contiguous()):
        raise _lib.FarHipError(f'conv_valid: `residual` must be a contiguous {tuple(y.shape)} tensor')
    entry = 'far_conv_valid_f16s' if pack.split else 'far_conv_valid_f16'          # a PackedConvValid(split=False): plain fp16 operands
    rc = getattr(lib, entry)(_p(x, torch.float32), _p(pack.packed), _p(pack.scale), _p(pack.shift, torch.float32), _p(residual, torch.float32),
                             _p(y), N, H, W, Cin, pack.Cout, k, _ACT[act], activation_exponent_value(), overflow_flag(x.device).data_ptr(),
                             _stream())
    _lib.check(rc, entry)
    return y

def _valid_bwd_shapes(what, x_shape, dy, Cin, Cout):
    """(N, H, W) of a K24 backward launch; FarHipError for anything far_conv_valid_f16s would not have produced dy from."""
    if not dy.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    if len(x_shape) != 4 or dy.dim() != 4:
        raise _lib.FarHipError(f'{what}: NHWC tensors expected, got x {tuple(x_shape)} and dy {tuple(dy.shape)}')
    N, H, W, _ = x_shape
    if Cin % 32 or Cout % 32 or Cin <= 0 or Cout <= 0:
        raise _lib.FarHipError(f'{what}: K24 covers Cin and Cout multiples of 32, got {Cin} -> {Cout}')
    if H < 5 or W < 5:
        raise _lib.FarHipError(f'{what}: a {H} x {W} input is smaller than the 5 x 5 kernel')
    if tuple(dy.shape) != (N, H - 4, W - 4, Cout):
        raise _lib.FarHipError(f'{what}: dy of shape {tuple(dy.shape)}, expected {(N, H - 4, W - 4, Cout)}')
    return N, H, W

def conv_valid_dgrad(dy, weight_or_pack, dy_scale=None):
    """K24 dgrad.  dy (N, H - 4, W - 4, Cout) fp32 NHWC -> dx (N, H, W, Cin), the input gradient of conv5x5_valid with the weight
    (Cout, Cin, 5, 5) or its PackedConvValid(dgrad=True) image; dy_scale = grad_scale(dy) if the caller has it already."""
    lib = _lib.load()
    if isinstance(weight_or_pack, PackedConvValid):
        pack = weight_or_pack
        if not pack.dgrad:
            raise _lib.FarHipError('conv_valid_dgrad takes a PackedConvValid built with dgrad=True')
    else:
        w = weight_or_pack
        if w.dim() != 4 or tuple(w.shape[2:]) != (5, 5):
            raise _lib.FarHipError(f'conv_valid_dgrad takes a (Cout, Cin, 5, 5) weight, got {tuple(w.shape)}')
        pack = PackedConvValid(w, dgrad=True, pack_scale=PackedConvValid(w).pack_scale)
    if dy.dim() != 4:
        raise _lib.FarHipError(f'conv_valid_dgrad: NHWC dy expected, got {tuple(dy.shape)}')
    N, H, W = _valid_bwd_shapes('conv_valid_dgrad', (dy.shape[0], dy.shape[1] + 4, dy.shape[2] + 4, pack.Cin), dy, pack.Cin, pack.Cout)
    dy = dy.contiguous()
    sc = grad_scale(dy) if dy_scale is None else dy_scale
    dx = torch.empty(N, H, W, pack.Cin, dtype=torch.float32, device=dy.device)
    rc = lib.far_conv_valid_dgrad_f16s(_p(dy, torch.float32), _p(pack.packed), _p(pack.pack_scale), _p(sc, torch.float32), _p(dx), N, H, W,
                                       pack.Cin, pack.Cout, pack.ksize, overflow_flag(dy.device).data_ptr(), _stream())
    _lib.check(rc, 'far_conv_valid_dgrad_f16s')
    return dx

def conv_valid_wgrad(x, dy, dy_scale=None, act_exp=None):
    """K24 wgrad.  dW (Cout, Cin, 5, 5) of conv5x5_valid from its NHWC input x (N, H, W, Cin) and output gradient dy (N, H - 4, W - 4,
    Cout); deterministic two-stage sum.  act_exp: the activation exponent x was consumed with in the forward (default: the current
    one); takes part in the activation-range guard."""
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    Cin, Cout = int(x.shape[-1]), int(dy.shape[-1])
    N, H, W = _valid_bwd_shapes('conv_valid_wgrad', tuple(x.shape), dy, Cin, Cout)
    x, dy = x.contiguous(), dy.contiguous()
    dw = torch.empty(Cout, Cin, 5, 5, dtype=torch.float32, device=x.device)
    if N == 0:
        return dw.zero_()
    nb = int(lib.far_conv_valid_wgrad_ws_bytes(N, H, W, Cin, Cout, 5))
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    rc = lib.far_conv_valid_wgrad_f16s(_p(x, torch.float32), _p(dy, torch.float32), N, H, W, Cin, Cout, 5,
                                       activation_exponent_value() if act_exp is None else int(act_exp),
                                       _p(dy_scale, torch.float32) if dy_scale is not None else None, _p(ws), nb, _p(dw),
                                       overflow_flag(x.device).data_ptr(), _stream())
    _lib.check(rc, 'far_conv_valid_wgrad_f16s')
    return dw

class _ConvValidFn(torch.autograd.Function):
    """The bare 5x5 unpadded convolution of the extractor's final block with gradients (extractor.py:11, :46-47 under autograd, without
    the bias): forward K24, backward far_conv_valid_dgrad_f16s / far_conv_valid_wgrad_f16s.  NHWC in and out."""

    @staticmethod
    def forward(ctx, x, weight, pack, pack_d):
        xn = x.detach().float().contiguous()
        y = conv_valid(xn, pack())
        ctx.save_for_backward(xn, weight)
        ctx.pack_d = pack_d
        ctx.act_exp = activation_exponent_value()            # the weight gradient splits xn with the forward's exponent
        return y

    @staticmethod
    def backward(ctx, g):
        xn, weight = ctx.saved_tensors
        gs = g.float().contiguous()
        sc = grad_scale(gs)
        dx = conv_valid_dgrad(gs, ctx.pack_d(), dy_scale=sc) if ctx.needs_input_grad[0] else None
        dw = conv_valid_wgrad(xn, gs, dy_scale=sc, act_exp=ctx.act_exp) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None

def conv_valid_train(x, weight, cache, name):
    """K24 with gradients.  x (N, H, W, Cin) fp32 GPU, NHWC; weight (Cout, Cin, 5, 5); cache: a PackCache.  Returns the bare
    convolution (N, H - 4, W - 4, Cout), NHWC.  The images are re-packed in place after an optimizer step, as conv_train's."""
    if not x.is_cuda or not weight.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (5, 5) or x.dim() != 4 or x.shape[-1] != weight.shape[1]:
        raise _lib.FarHipError(f'conv_valid_train: x {tuple(x.shape)} (NHWC) and weight {tuple(weight.shape)} are no 5x5 convolution')
    if x.shape[1] < 5 or x.shape[2] < 5:
        raise _lib.FarHipError(f'conv_valid_train: a {x.shape[1]} x {x.shape[2]} input is smaller than the 5 x 5 kernel')
    re = lambda pc: pc.refresh(weight)                 # the forward image first: the dgrad image borrows its (refreshed) scale
    pack = lambda: cache.get((name, 'valid'), [weight], lambda: PackedConvValid(weight), refresh=re)
    pack_d = lambda: cache.get((name, 'valid', 'dgrad'), [weight], lambda: PackedConvValid(weight, dgrad=True, pack_scale=pack().pack_scale),
                               refresh=re).follow_scale(pack(), weight)
    return _ConvValidFn.apply(x, weight, pack, pack_d)

_RESIZE_TABLES = {}

def resize_tables(H, W, device, size=224):
    """The source row / column of every destination row / column of F.interpolate(x, size=size) (nearest) for an (H, W) fp32 image on
    `device`, as two int32 device vectors -- taken from torch's own interpolate of two index images, once per (H, W, device), so that
    K25 reads exactly the pixels torch would."""
    device = torch.device(device)
    key = (int(H), int(W), str(device), int(size))
    t = _RESIZE_TABLES.get(key)
    if t is None:
        F = torch.nn.functional
        rows = F.interpolate(torch.arange(H, dtype=torch.float32, device=device).view(1, 1, H, 1).expand(1, 1, H, W).contiguous(), size=size)[0, 0]
        cols = F.interpolate(torch.arange(W, dtype=torch.float32, device=device).view(1, 1, 1, W).expand(1, 1, H, W).contiguous(), size=size)[0, 0]
        r, c = rows[:, 0].to(torch.int32).contiguous(), cols[0, :].to(torch.int32).contiguous()
        ok = (bool((rows == rows[:, :1]).all()) and bool((cols == cols[:1, :]).all()) and 0 <= int(r.min()) and int(r.max()) < H
              and 0 <= int(c.min()) and int(c.max()) < W)
        if not ok:
            raise _lib.FarHipError(f'resize_tables: the nearest-neighbour resize of a {H} x {W} image is not a row / column gather')
        t = _RESIZE_TABLES[key] = (r, c)
    return t

def stem_rgb(images, pack):
    """K25.  images (N, 3, H, W) fp32 contiguous on the GPU, values 0 .. 255 in the channel order the reference takes -> relu(bn1(conv1(
    F.interpolate(normalise(flip(images)), size=224)))) as NHWC (N, 112, 112, 64) for a PackedStemRGB; `images` is only read."""
    lib = _lib.load()
    if not isinstance(pack, PackedStemRGB):
        raise _lib.FarHipError('stem_rgb takes a PackedStemRGB')
    if not images.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] < 1 or images.shape[3] < 1:
        raise _lib.FarHipError(f'stem_rgb expects (N, 3, H, W) images, got {tuple(images.shape)}')
    N, _, H, W = images.shape
    rows, cols = resize_tables(H, W, images.device)
    y = torch.empty(N, 112, 112, 64, dtype=torch.float32, device=images.device)
    rc = lib.far_stem_rgb_f16s(_p(images, torch.float32), N, H, W, _p(rows, torch.int32), _p(cols, torch.int32), _p(pack.packed), _p(pack.scale),
                               _p(pack.shift), _p(y), _stream())
    _lib.check(rc, 'far_stem_rgb_f16s')
    return y

def maxpool3x3s2(x):
    """K26.  F.max_pool2d(x, 3, stride=2, padding=1) for NHWC x (N, H, W, C) fp32 contiguous, C % 4 == 0 -> (N, (H - 1) // 2 + 1,
    (W - 1) // 2 + 1, C); exact."""
    lib = _lib.load()
    if x.dim() != 4 or x.shape[-1] % 4 or x.shape[1] < 1 or x.shape[2] < 1:
        raise _lib.FarHipError(f'maxpool3x3s2 expects NHWC (N, H, W, C) with C % 4 == 0, got {tuple(x.shape)}')
    N, H, W, C = x.shape
    y = torch.empty(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=torch.float32, device=x.device)
    _lib.check(lib.far_maxpool3x3s2_nhwc_f32(_p(x, torch.float32), N, H, W, C, _p(y), _stream()), 'far_maxpool3x3s2_nhwc_f32')
    return y

def stem_conv_rgb(images, pack):
    """K27.  images (N, 3, H, W) fp32 contiguous on the GPU, as the network consumes them (no flip, no normalisation, no resize) ->
    relu(bn(conv7x7 stride 2 pad 3)) as NHWC (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64) for a PackedStemRGB (K25's weight image);
    `images` is only read.  Takes part in the activation-range guard as K9 does: the pixels are split around the thread's activation
    exponent, one beyond its range ORs ops.overflow_flag."""
    lib = _lib.load()
    if not isinstance(pack, PackedStemRGB):
        raise _lib.FarHipError('stem_conv_rgb takes a PackedStemRGB')
    if not images.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] < 1 or images.shape[3] < 1:
        raise _lib.FarHipError(f'stem_conv_rgb expects (N, 3, H, W) images, got {tuple(images.shape)}')
    N, _, H, W = images.shape
    y = torch.empty(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64, dtype=torch.float32, device=images.device)
    rc = lib.far_stem_conv_rgb_f16s(_p(images, torch.float32), N, H, W, _p(pack.packed), _p(pack.scale), _p(pack.shift), _p(y),
                                    activation_exponent_value(), overflow_flag(images.device).data_ptr(), _stream())
    _lib.check(rc, 'far_stem_conv_rgb_f16s')
    return y

def upsample2x_pad(lo=None, skip=None, size=None):
    """K28, one launch.  lo (N, h, w, C) fp32 NHWC -> F.interpolate(lo, scale_factor=2, mode='bilinear', align_corners=True) as
    (N, 2h, 2w, C); skip (N, hs, ws, Cs) -> the skip map zero-padded to (N, 2h, 2w, Cs), diff // 2 before and the rest after
    (resunet.py:90-95).  Returns (up, padded); an absent input gives None (size = (2h, 2w) is then needed for the pad alone); a skip
    map that already has the size is returned as it is."""
    lib = _lib.load()
    if lo is None and skip is None:
        raise _lib.FarHipError('upsample2x_pad: nothing to do')
    for t in (lo, skip):
        if t is not None and not t.is_cuda:
            raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
        if t is not None and (t.dim() != 4 or t.shape[-1] % 4 or t.dtype != torch.float32):
            raise _lib.FarHipError(f'upsample2x_pad expects fp32 NHWC (N, H, W, C) with C % 4 == 0, got {tuple(t.shape)} {t.dtype}')
    if lo is not None:
        N, h, w, C = lo.shape
        if size is not None and tuple(size) != (2 * h, 2 * w):
            raise _lib.FarHipError(f'upsample2x_pad: size {tuple(size)} is not twice {(h, w)}')
    else:
        if size is None or size[0] % 2 or size[1] % 2:
            raise _lib.FarHipError('upsample2x_pad: the pad alone needs an even size = (H, W)')
        N, h, w, C = skip.shape[0], size[0] // 2, size[1] // 2, 0
    H, W = 2 * h, 2 * w
    up = None if lo is None else torch.empty(N, H, W, C, dtype=torch.float32, device=lo.device)
    padded = None
    if skip is not None:
        if skip.shape[0] != N or skip.shape[1] > H or skip.shape[2] > W or skip.shape[1] < 1 or skip.shape[2] < 1:
            raise _lib.FarHipError(f'upsample2x_pad: a skip map {tuple(skip.shape)} does not fit into ({N}, {H}, {W}, .)')
        if tuple(skip.shape[1:3]) == (H, W):
            padded, skip = skip, None                         # nothing to pad: K9 reads the skip map itself
        else:
            padded = torch.empty(N, H, W, skip.shape[3], dtype=torch.float32, device=skip.device)
    if lo is None and skip is None:
        return up, padded
    rc = lib.far_upsample2x_pad_f32(_p(lo, torch.float32), N, h, w, C, _p(up), _p(skip, torch.float32),
                                    0 if skip is None else skip.shape[1], 0 if skip is None else skip.shape[2],
                                    0 if skip is None else skip.shape[3], _p(padded) if skip is not None else None, _stream())
    _lib.check(rc, 'far_upsample2x_pad_f32')
    return up, padded

def elu(x, inplace=False):
    """K28.  F.elu(x) (alpha 1) for a contiguous fp32 GPU tensor of any shape; exact fp32 (expm1)."""
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
    y = x if inplace else torch.empty_like(x)
    _lib.check(lib.far_elu_f32(_p(x, torch.float32), x.numel(), _p(y), _stream()), 'far_elu_f32')
    return _written(y) if inplace else y
