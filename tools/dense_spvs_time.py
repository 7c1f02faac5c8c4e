"""Dense coarse supervision (far_coarse_dense_focal_f16s + far_coarse_dense_focal_bwd_f16: sparse_spvs = False, dual_softmax, focal)
timed in one process against (a) K1's sparse training pair far_coarse_pos_conf_f16s + far_coarse_pos_conf_bwd_f16 on the same features
and positions and (b) the fp32 torch dense composition -- conf_matrix = softmax(sim, 1) * softmax(sim, 2) (coarse_matching.py:104-118),
the loss of far_amd.losses.coarse_focal_loss_dense_torch, autograd -- at 1 and 2 pairs of 60 x 80 with 1500 positives per pair.
HIP events around the C calls (no host synchronisation inside the timed region), warm-up, then REPS alternating repetitions; the
median of each; forward and backward also timed apart, and the backward in both forms of G (fp16 hi + lo pair / one fp16).
Prints one JSON line.  Usage: python tools/dense_spvs_time.py [--reps N] [--pairs N [N ...]]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from far_amd import _lib, losses, ops

ALPHA, GAMMA, POS_W, NEG_W, T = 0.25, 2.0, 1.0, 1.0, 0.1


def case(lib, Z, hw, reps, per_pair=1500):
    L = hw[0] * hw[1]
    g = torch.Generator(device='cuda').manual_seed(7)
    f0 = 3.75 * torch.randn(Z, L, 256, device='cuda', generator=g)
    perm = torch.randperm(L, device='cuda', generator=g)
    f1 = f0[:, perm] + 0.1 * torch.randn(Z, L, 256, device='cuda', generator=g)
    k = torch.randperm(L, device='cuda', generator=g)[:per_pair]
    pb = torch.arange(Z, device='cuda').repeat_interleave(per_pair)
    pi, pj = perm[k].repeat(Z).contiguous(), k.repeat(Z).contiguous()        # f1[:, k] = f0[:, perm[k]]
    M = Z * per_pair
    w_pos = 1e-4 * torch.randn(M, device='cuda', generator=g)
    conf, loss, gup = torch.empty(M, device='cuda'), torch.empty((), device='cuda'), torch.ones(1, device='cuda')
    df0, df1 = torch.empty_like(f0), torch.empty_like(f1)
    ws_n = torch.empty(lib.far_coarse_dense_focal_workspace_bytes(Z, L, L, 256, M), dtype=torch.uint8, device='cuda')
    ws_d = torch.empty(lib.far_coarse_train_workspace_bytes(Z, L, L, 256), dtype=torch.uint8, device='cuda')
    flag = ops.overflow_flag(torch.device('cuda'))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def dense_fwd():
        return lib.far_coarse_dense_focal_f16s(P(f0), P(f1), Z, L, L, 256, T, null, null, P(pb), P(pi), P(pj), M, ALPHA, GAMMA, POS_W, NEG_W,
                                               0, P(loss), P(ws_n), P(flag), st)

    def dense_bwd(split=1):
        return lib.far_coarse_dense_focal_bwd_f16(P(f0), P(f1), Z, L, L, 256, T, null, null, P(pb), P(pi), P(pj), M, ALPHA, GAMMA, POS_W,
                                                  NEG_W, 0, P(gup), split, P(df0), P(df1), P(ws_n), st)

    def dense_bwd_plain():
        return dense_bwd(0)

    def sparse_fwd():
        return lib.far_coarse_pos_conf_f16s(P(f0), P(f1), Z, L, L, 256, T, P(pb), P(pi), P(pj), M, P(conf), P(ws_d), P(flag), st)

    def sparse_bwd():
        return lib.far_coarse_pos_conf_bwd_f16(P(f0), P(f1), Z, L, L, 256, T, P(pb), P(pi), P(pj), M, P(w_pos), P(df0), P(df1), P(ws_d), st)

    def torch_dense():
        a0, a1 = f0.detach().requires_grad_(True), f1.detach().requires_grad_(True)
        sim = torch.einsum('nlc,nsc->nls', a0 / 16.0, a1 / 16.0) / T
        c = torch.softmax(sim, 1) * torch.softmax(sim, 2)
        losses.coarse_focal_loss_dense_torch(c, (pb, pi, pj), False, ALPHA, GAMMA, POS_W, NEG_W).backward()
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

    for _ in range(3):                                  # warm-up (kernel attributes, caches, clocks, the allocator's blocks)
        timed(dense_fwd, dense_bwd), timed(dense_fwd, dense_bwd_plain), timed(sparse_fwd, sparse_bwd), timed(torch_dense)
    loss_value = float(loss)
    t = {k: [] for k in ('dense', 'dense_f', 'dense_b', 'dense_b_plain', 'sparse', 'sparse_f', 'sparse_b', 'torch')}
    for _ in range(reps):
        t['dense'].append(timed(dense_fwd, dense_bwd)); t['sparse'].append(timed(sparse_fwd, sparse_bwd))
        t['torch'].append(timed(torch_dense))
        t['dense_f'].append(timed(dense_fwd)); t['dense_b'].append(timed(dense_bwd)); t['dense_b_plain'].append(timed(dense_bwd_plain))
        t['sparse_f'].append(timed(sparse_fwd)); t['sparse_b'].append(timed(sparse_bwd))
    md = {k: statistics.median(v) for k, v in t.items()}
    return {'pairs': Z, 'grid': list(hw), 'positives': M, 'loss': loss_value,
            'dense_fwd_bwd_ms': round(md['dense'], 4), 'sparse_fwd_bwd_ms': round(md['sparse'], 4), 'torch_dense_fwd_bwd_ms': round(md['torch'], 4),
            'ratio_to_sparse': round(md['dense'] / md['sparse'], 3), 'torch_over_dense': round(md['torch'] / md['dense'], 3),
            'dense_fwd_ms': round(md['dense_f'], 4), 'dense_bwd_ms': round(md['dense_b'], 4), 'dense_bwd_fp16_g_ms': round(md['dense_b_plain'], 4),
            'sparse_fwd_ms': round(md['sparse_f'], 4), 'sparse_bwd_ms': round(md['sparse_b'], 4), 'reps': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--pairs', type=int, nargs='+', default=[1, 2])
    a = ap.parse_args()
    lib = _lib.load()
    res = [case(lib, z, (60, 80), a.reps) for z in a.pairs]
    print(json.dumps({'tool': 'dense_spvs_time', 'device': torch.cuda.get_device_name(),
                      'overflow': bool(ops.overflow_flag(torch.device('cuda')).item()), 'cases': res}), flush=True)


if __name__ == '__main__':
    main()
