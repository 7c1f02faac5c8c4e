"""The optimal-transport coarse matcher (far_coarse_match_sinkhorn_f16s, T = 3 as in the loftr_ot configurations) against the dual-softmax
K1 (far_coarse_match_f16s) on the same inputs, in one process: HIP events around the C calls (no host synchronisation inside the timed
region), warm-up, then REPS alternating repetitions; the median of each.  Shapes: 32 pairs at 60 x 80 (the bench) and 16 pairs at
68 x 90 (Map-free).  Prints one JSON line.  Usage: python tools/sinkhorn_time.py [--reps N] [--prefilter]
--train: the training path instead -- far_sinkhorn_pos_conf_f16s + far_sinkhorn_pos_conf_bwd_f16 (forward + backward, T = 3) against
far_coarse_pos_conf_f16s + far_coarse_pos_conf_bwd_f16 on the same features and positions, at 1 and 2 pairs of 60 x 80 with 1500
positions per pair; forward and backward also timed apart.  --pairs N [N ...]: other batch sizes for the --train leg (32: the bench's
batch, where the position grouping of the backward scans 48 000 positions).
--dense: the optimal-transport matcher with dense supervision -- far_sinkhorn_dense_focal_f16s + far_sinkhorn_dense_focal_bwd_f16
(forward + backward, T = 3, 1500 labels per pair) against, in the same run, the sparse optimal-transport pair above and the fp32 torch
autograd of the materialising definition + losses.coarse_focal_loss_dense_torch (its L x S tensors included)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from far_amd import _lib, ops


def shape_case(lib, Z, hw, reps, prefilter):
    L = hw[0] * hw[1]
    g = torch.Generator(device='cuda').manual_seed(7)
    f0 = 3.75 * torch.randn(Z, L, 256, device='cuda', generator=g)
    f1 = f0[:, torch.randperm(L, device='cuda', generator=g)] + 0.1 * torch.randn(Z, L, 256, device='cuda', generator=g)
    bs = torch.tensor(1.0, device='cuda')
    cap = Z * L
    outs = [torch.empty(cap, dtype=torch.int64, device='cuda') for _ in range(3)] + [torch.empty(cap, device='cuda'),
                                                                                      torch.empty(cap, 2, device='cuda'),
                                                                                      torch.empty(cap, 2, device='cuda')]
    counts_s = torch.empty(Z + 1, dtype=torch.int32, device='cuda')      # each matcher its own counts: both report their match count
    counts_d = torch.empty(Z + 1, dtype=torch.int32, device='cuda')
    ws_s = torch.empty(lib.far_coarse_match_sinkhorn_f16s_workspace_bytes(Z, L, L, 256), dtype=torch.uint8, device='cuda')
    ws_d = torch.empty(lib.far_coarse_match_f16s_workspace_bytes(Z, L, L, 256), dtype=torch.uint8, device='cuda')
    flag = ops.overflow_flag(torch.device('cuda'))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = [ctypes.c_void_p(t.data_ptr()) for t in outs]
    cnt_s, tot_s = ctypes.c_void_p(counts_s.data_ptr()), ctypes.c_void_p(counts_s.data_ptr() + 4 * Z)
    cnt_d, tot_d = ctypes.c_void_p(counts_d.data_ptr()), ctypes.c_void_p(counts_d.data_ptr() + 4 * Z)
    null = ctypes.c_void_p(0)

    def sinkhorn():
        return lib.far_coarse_match_sinkhorn_f16s(f0.data_ptr(), f1.data_ptr(), Z, L, L, 256, bs.data_ptr(), 3, int(prefilter), 0.2, 2,
                                                  hw[0], hw[1], hw[0], hw[1], 8.0, null, null, null, null, null, null, null, null,
                                                  *p, cnt_s, tot_s, ws_s.data_ptr(), flag.data_ptr(), st)

    def dual_softmax():
        return lib.far_coarse_match_f16s(f0.data_ptr(), f1.data_ptr(), Z, L, L, 256, 0.1, 0.2, 2, hw[0], hw[1], hw[0], hw[1], 8.0,
                                         null, null, null, null, null, null, *p, cnt_d, tot_d, ws_d.data_ptr(), flag.data_ptr(), st)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn()
        b.record()
        b.synchronize()
        _lib.check(rc, fn.__name__)
        return a.elapsed_time(b)

    for _ in range(3):                                  # warm-up (kernel attributes, caches, clocks)
        timed(sinkhorn), timed(dual_softmax)
    m_skh, m_ds = int(counts_s[Z]), int(counts_d[Z])
    ts, td = [], []
    for _ in range(reps):
        ts.append(timed(sinkhorn))
        td.append(timed(dual_softmax))
    return {'pairs': Z, 'grid': list(hw), 'sinkhorn_ms': round(statistics.median(ts), 4), 'dual_softmax_ms': round(statistics.median(td), 4),
            'ratio': round(statistics.median(ts) / statistics.median(td), 3), 'sinkhorn_matches': m_skh, 'dual_softmax_matches': m_ds, 'reps': reps}


def train_case(lib, Z, hw, reps, per_pair=1500):
    L = hw[0] * hw[1]
    g = torch.Generator(device='cuda').manual_seed(7)
    f0 = 3.75 * torch.randn(Z, L, 256, device='cuda', generator=g)
    perm = torch.randperm(L, device='cuda', generator=g)
    f1 = f0[:, perm] + 0.1 * torch.randn(Z, L, 256, device='cuda', generator=g)
    k = torch.randperm(L, device='cuda', generator=g)[:per_pair]
    pb = torch.arange(Z, device='cuda').repeat_interleave(per_pair)
    pi, pj = perm[k].repeat(Z).contiguous(), k.repeat(Z).contiguous()        # f1[:, k] = f0[:, perm[k]]
    M = Z * per_pair
    bs = torch.tensor(1.0, device='cuda')
    w_pos, w0, w1 = (1e-4 * torch.randn(n, device='cuda', generator=g) for n in (M, Z * L, Z * L))
    conf, b0, b1 = torch.empty(M, device='cuda'), torch.empty(Z, L, device='cuda'), torch.empty(Z, L, device='cuda')
    df0, df1, dbin = torch.empty_like(f0), torch.empty_like(f1), torch.empty(1, device='cuda')
    ws_s = torch.empty(lib.far_sinkhorn_pos_conf_workspace_bytes(Z, L, L, 256, 3), dtype=torch.uint8, device='cuda')
    ws_d = torch.empty(lib.far_coarse_train_workspace_bytes(Z, L, L, 256), dtype=torch.uint8, device='cuda')
    flag = ops.overflow_flag(torch.device('cuda'))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def skh_fwd():
        return lib.far_sinkhorn_pos_conf_f16s(P(f0), P(f1), Z, L, L, 256, P(bs), 3, null, null, P(pb), P(pi), P(pj), M, P(conf), P(b0), P(b1),
                                              P(ws_s), P(flag), st)

    def skh_bwd():
        return lib.far_sinkhorn_pos_conf_bwd_f16(P(f0), P(f1), Z, L, L, 256, P(bs), 3, null, null, P(pb), P(pi), P(pj), M, P(w_pos), P(w0),
                                                 P(w1), P(df0), P(df1), P(dbin), P(ws_s), st)

    def ds_fwd():
        return lib.far_coarse_pos_conf_f16s(P(f0), P(f1), Z, L, L, 256, 0.1, P(pb), P(pi), P(pj), M, P(conf), P(ws_d), P(flag), st)

    def ds_bwd():
        return lib.far_coarse_pos_conf_bwd_f16(P(f0), P(f1), Z, L, L, 256, 0.1, P(pb), P(pi), P(pj), M, P(w_pos), P(df0), P(df1), P(ws_d), st)

    def timed(*fns):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rcs = [fn() for fn in fns]
        b.record()
        b.synchronize()
        for rc, fn in zip(rcs, fns):
            _lib.check(rc, fn.__name__)
        return a.elapsed_time(b)

    for _ in range(3):
        timed(skh_fwd, skh_bwd), timed(ds_fwd, ds_bwd)
    t = {k: [] for k in ('skh', 'skh_f', 'skh_b', 'ds', 'ds_f', 'ds_b')}
    for _ in range(reps):
        t['skh'].append(timed(skh_fwd, skh_bwd)); t['ds'].append(timed(ds_fwd, ds_bwd))
        t['skh_f'].append(timed(skh_fwd)); t['skh_b'].append(timed(skh_bwd))
        t['ds_f'].append(timed(ds_fwd)); t['ds_b'].append(timed(ds_bwd))
    md = {k: statistics.median(v) for k, v in t.items()}
    return {'pairs': Z, 'grid': list(hw), 'positions': M, 'sinkhorn_fwd_bwd_ms': round(md['skh'], 4), 'dual_softmax_fwd_bwd_ms': round(md['ds'], 4),
            'ratio': round(md['skh'] / md['ds'], 3), 'sinkhorn_fwd_ms': round(md['skh_f'], 4), 'sinkhorn_bwd_ms': round(md['skh_b'], 4),
            'dual_softmax_fwd_ms': round(md['ds_f'], 4), 'dual_softmax_bwd_ms': round(md['ds_b'], 4),
            'bwd_ratio': round(md['skh_b'] / md['ds_b'], 3), 'reps': reps}


def dense_case(lib, Z, hw, reps, per_pair=1500):
    from far_amd import losses
    L = hw[0] * hw[1]
    g = torch.Generator(device='cuda').manual_seed(7)
    f0 = 3.75 * torch.randn(Z, L, 256, device='cuda', generator=g)
    perm = torch.randperm(L, device='cuda', generator=g)
    f1 = f0[:, perm] + 0.1 * torch.randn(Z, L, 256, device='cuda', generator=g)
    k = torch.randperm(L, device='cuda', generator=g)[:per_pair]
    pb = torch.arange(Z, device='cuda').repeat_interleave(per_pair)
    pi, pj = perm[k].repeat(Z).contiguous(), k.repeat(Z).contiguous()
    M = Z * per_pair
    bs = torch.tensor(1.0, device='cuda')
    w_pos, w0, w1 = (1e-4 * torch.randn(n, device='cuda', generator=g) for n in (M, Z * L, Z * L))
    conf, b0, b1 = torch.empty(M, device='cuda'), torch.empty(Z, L, device='cuda'), torch.empty(Z, L, device='cuda')
    df0, df1, dbin = torch.empty_like(f0), torch.empty_like(f1), torch.empty(1, device='cuda')
    loss, gup = torch.empty((), device='cuda'), torch.ones(1, device='cuda')
    ws_s = torch.empty(lib.far_sinkhorn_pos_conf_workspace_bytes(Z, L, L, 256, 3), dtype=torch.uint8, device='cuda')
    ws_d = torch.empty(lib.far_sinkhorn_dense_focal_workspace_bytes(Z, L, L, 256, 3, M), dtype=torch.uint8, device='cuda')
    flag = ops.overflow_flag(torch.device('cuda'))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    focal = (0.25, 2.0, 1.0, 1.0, 0)

    def skh_fwd():
        return lib.far_sinkhorn_pos_conf_f16s(P(f0), P(f1), Z, L, L, 256, P(bs), 3, null, null, P(pb), P(pi), P(pj), M, P(conf), P(b0), P(b1),
                                              P(ws_s), P(flag), st)

    def skh_bwd():
        return lib.far_sinkhorn_pos_conf_bwd_f16(P(f0), P(f1), Z, L, L, 256, P(bs), 3, null, null, P(pb), P(pi), P(pj), M, P(w_pos), P(w0),
                                                 P(w1), P(df0), P(df1), P(dbin), P(ws_s), st)

    def dense_fwd():
        return lib.far_sinkhorn_dense_focal_f16s(P(f0), P(f1), Z, L, L, 256, P(bs), 3, null, null, P(pb), P(pi), P(pj), M, *focal, P(loss),
                                                 P(ws_d), P(flag), st)

    def dense_bwd():
        return lib.far_sinkhorn_dense_focal_bwd_f16(P(f0), P(f1), Z, L, L, 256, P(bs), 3, null, null, P(pb), P(pi), P(pj), M, *focal, P(gup),
                                                    P(df0), P(df1), P(dbin), P(ws_d), st)

    def definition(a0, a1, alpha, T=3):                       # the materialising definition, fp32
        s = torch.einsum('nlc,nsc->nls', a0, a1) / 256
        a = alpha.reshape(1, 1, 1)
        Zc = torch.cat([torch.cat([s, a.expand(Z, L, 1)], 2), a.expand(Z, 1, L + 1)], 1)
        norm = -torch.log(torch.tensor(2.0 * L, device='cuda'))
        lmu = torch.cat([norm.expand(L), torch.log(torch.tensor(float(L), device='cuda'))[None] + norm])
        u = torch.zeros(Z, L + 1, device='cuda')
        v = torch.zeros(Z, L + 1, device='cuda')
        for _ in range(T):
            u = lmu - torch.logsumexp(Zc + v[:, None, :], 2)
            v = lmu - torch.logsumexp(Zc + u[:, :, None], 1)
        return (Zc + u[:, :, None] + v[:, None, :] - norm).exp()

    def torch_leg():
        a0, a1, al = f0.clone().requires_grad_(True), f1.clone().requires_grad_(True), bs.clone().requires_grad_(True)
        losses.coarse_focal_loss_dense_torch(definition(a0, a1, al)[:, :-1, :-1], (pb, pi, pj), False).backward()
        return 0

    def timed(*fns):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rcs = [fn() for fn in fns]
        b.record()
        b.synchronize()
        for rc, fn in zip(rcs, fns):
            _lib.check(rc, fn.__name__)
        return a.elapsed_time(b)

    for _ in range(3):
        timed(skh_fwd, skh_bwd), timed(dense_fwd, dense_bwd), timed(torch_leg)
    t = {k: [] for k in ('skh', 'dense', 'dense_f', 'dense_b', 'torch')}
    for _ in range(reps):
        t['skh'].append(timed(skh_fwd, skh_bwd)); t['dense'].append(timed(dense_fwd, dense_bwd))
        t['dense_f'].append(timed(dense_fwd)); t['dense_b'].append(timed(dense_bwd))
        t['torch'].append(timed(torch_leg))
    md = {k: statistics.median(v) for k, v in t.items()}
    return {'pairs': Z, 'grid': list(hw), 'labels': M, 'dense_fwd_bwd_ms': round(md['dense'], 4), 'sparse_fwd_bwd_ms': round(md['skh'], 4),
            'torch_fp32_fwd_bwd_ms': round(md['torch'], 4), 'ratio_to_sparse': round(md['dense'] / md['skh'], 3),
            'ratio_to_torch': round(md['dense'] / md['torch'], 3), 'dense_fwd_ms': round(md['dense_f'], 4),
            'dense_bwd_ms': round(md['dense_b'], 4), 'loss': float(loss), 'reps': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--prefilter', action='store_true')
    ap.add_argument('--train', action='store_true')
    ap.add_argument('--dense', action='store_true')
    ap.add_argument('--pairs', type=int, nargs='+', default=[1, 2])
    a = ap.parse_args()
    lib = _lib.load()
    if a.dense:
        res = [dense_case(lib, z, (60, 80), a.reps) for z in a.pairs]
        print(json.dumps({'tool': 'sinkhorn_time', 'leg': 'dense', 'iters': 3, 'device': torch.cuda.get_device_name(),
                          'overflow': bool(ops.overflow_flag(torch.device('cuda')).item()), 'cases': res}), flush=True)
        return
    if a.train:
        res = [train_case(lib, z, (60, 80), a.reps) for z in a.pairs]
        print(json.dumps({'tool': 'sinkhorn_time', 'leg': 'train', 'iters': 3, 'device': torch.cuda.get_device_name(),
                          'overflow': bool(ops.overflow_flag(torch.device('cuda')).item()), 'cases': res}), flush=True)
        return
    res = [shape_case(lib, 32, (60, 80), a.reps, a.prefilter), shape_case(lib, 16, (68, 90), a.reps, a.prefilter)]
    print(json.dumps({'tool': 'sinkhorn_time', 'iters': 3, 'prefilter': a.prefilter, 'device': torch.cuda.get_device_name(),
                      'overflow': bool(ops.overflow_flag(torch.device('cuda')).item()), 'cases': res}), flush=True)


if __name__ == '__main__':
    main()
