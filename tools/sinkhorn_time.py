"""The optimal-transport coarse matcher (far_coarse_match_sinkhorn_f16s, T = 3 as in the loftr_ot configurations) against the dual-softmax
K1 (far_coarse_match_f16s) on the same inputs, in one process: HIP events around the C calls (no host synchronisation inside the timed
region), warm-up, then REPS alternating repetitions; the median of each.  Shapes: 32 pairs at 60 x 80 (the bench) and 16 pairs at
68 x 90 (Map-free).  Prints one JSON line.  Usage: python tools/sinkhorn_time.py [--reps N] [--prefilter]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--prefilter', action='store_true')
    a = ap.parse_args()
    lib = _lib.load()
    res = [shape_case(lib, 32, (60, 80), a.reps, a.prefilter), shape_case(lib, 16, (68, 90), a.reps, a.prefilter)]
    print(json.dumps({'tool': 'sinkhorn_time', 'iters': 3, 'prefilter': a.prefilter, 'device': torch.cuda.get_device_name(),
                      'overflow': bool(ops.overflow_flag(torch.device('cuda')).item()), 'cases': res}), flush=True)


if __name__ == '__main__':
    main()
