"""K12 training (ops.corr_volume_warp_train: far_corr_volume_warp_train_f32 + far_corr_volume_warp_bwd_f32) timed in one process on one
GPU at the model's 92 x 68 grid, B = 1 and B = 32 pairs (bench.py measures the LoFTR regressor and is not touched):

  * forward alone (the training forward, which also saves the row statistics) and forward + backward with both gradients, next to fp32
    torch autograd of the materialising composition the reference runs (aggregator.py:42-116: a (B, HW, HW) softmax) on the same inputs.
    If the torch leg runs out of memory at a batch size it is timed at the largest B that fits (halving), and the table says which;
  * the peak device memory of one forward + backward of either leg (torch.cuda.max_memory_allocated over the call, inputs excluded);
  * backward / forward: the arithmetic ratio is 3.5 (112 against 32 MFMAs per 32 x 32 tile).

Timing as tools/mapfree_reg_time.py: HIP events around groups of calls, every leg warmed up, the legs ALTERNATED round by round, medians
over the rounds with the min .. max spread.  Prints a table and one JSON line.  --trace B: one forward + backward at batch size B and
nothing else (for a kernel trace of that one call, in a run of its own).
Usage: python tools/cvw_train_time.py [--rounds N] [--batches 1,32] [--trace B]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from far_amd import ops
from tools.vit8pt_time import alternate

GRID = (92, 68)


def composition(vol0, vol1):
    """aggregator.py:42-116 in FAR's configuration, as the reference writes it."""
    B, D, H, W = vol0.shape
    a, b = vol0.view(B, D, H * W), vol1.view(B, D, H * W)
    cvolume = torch.softmax(torch.bmm(a.transpose(1, 2), b), dim=2)
    vol1w = torch.bmm(b, cvolume.transpose(1, 2))
    uu, vv = torch.meshgrid(torch.linspace(-1, 1, H, device=a.device), torch.linspace(-1, 1, W, device=a.device), indexing='ij')
    grid = torch.stack([uu, vv], dim=0).view(2, H * W).unsqueeze(0).repeat(B, 1, 1)
    pos = torch.bmm(grid, cvolume.transpose(1, 2))
    max_score = torch.max(cvolume, dim=2, keepdim=True)[0].transpose(1, 2)
    return torch.cat([a, vol1w, pos, max_score], dim=1).view(B, -1, H, W)


def inputs(B):
    g = torch.Generator(device='cuda').manual_seed(B)
    v0 = (0.5 * torch.randn(B, 32, *GRID, device='cuda', generator=g)).requires_grad_(True)
    v1 = (0.5 * torch.randn(B, 32, *GRID, device='cuda', generator=g)).requires_grad_(True)
    dagg = torch.randn(B, 67, *GRID, device='cuda', generator=g)
    return v0, v1, dagg


def fwd_bwd(fn, v0, v1, dagg):
    return torch.autograd.grad(fn(v0, v1), (v0, v1), dagg)


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def torch_batch(B):
    """The largest batch size <= B (halving) at which the torch leg's forward + backward fits."""
    while B >= 1:
        try:
            v0, v1, dagg = inputs(B)
            fwd_bwd(composition, v0, v1, dagg)
            torch.cuda.synchronize()
            return B
        except torch.cuda.OutOfMemoryError:
            del v0, v1, dagg
            torch.cuda.empty_cache()
            B //= 2
    raise SystemExit('the torch composition does not fit at B = 1')


def case(B, rounds):
    v0, v1, dagg = inputs(B)
    Bt = torch_batch(B)
    t0, t1, tg = (v0, v1, dagg) if Bt == B else inputs(Bt)
    with torch.no_grad():
        dev = float((ops.corr_volume_warp(t0[:1], t1[:1]) - composition(t0[:1], t1[:1])).abs().max())
    legs = {'k12_forward': lambda: ops.corr_volume_warp_train(v0, v1),
            'k12_forward_backward': lambda: fwd_bwd(ops.corr_volume_warp_train, v0, v1, dagg),
            'torch_fp32_forward': lambda: composition(t0, t1),
            'torch_fp32_forward_backward': lambda: fwd_bwd(composition, t0, t1, tg)}
    mem = {'k12_peak_mb': peak_mb(legs['k12_forward_backward']), 'torch_fp32_peak_mb': peak_mb(legs['torch_fp32_forward_backward'])}
    r = alternate(legs, rounds, target_ms=40.0)
    out = {'B': B, 'torch_B': Bt, 'grid': list(GRID), 'max_abs_diff_agg_vs_torch_fp32': dev, **mem,
           **{name: {'median_ms': m, 'min_ms': lo, 'max_ms': hi} for name, (m, lo, hi) in r.items()}}
    f, fb = out['k12_forward']['median_ms'], out['k12_forward_backward']['median_ms']
    out['k12_backward_over_forward'] = (fb - f) / f
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--batches', default='1,32')
    ap.add_argument('--trace', type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cvw_train_time needs a GPU: nothing is timed without one')
    if a.trace:
        v0, v1, dagg = inputs(a.trace)
        fwd_bwd(ops.corr_volume_warp_train, v0, v1, dagg)
        torch.cuda.synchronize()
        return
    res = {'tool': 'cvw_train_time', 'device': torch.cuda.get_device_name(), 'rounds': a.rounds, 'cases': []}
    fmt = lambda d: f'{d["median_ms"]:9.4f} ms  ({d["min_ms"]:.4f} .. {d["max_ms"]:.4f})'
    for B in (int(b) for b in a.batches.split(',')):
        c = case(B, a.rounds)
        res['cases'].append(c)
        note = '' if c['torch_B'] == B else f'; the torch legs ran out of memory at B = {B} and are timed at B = {c["torch_B"]} (per-pair figures in brackets)'
        print(f'# K12 training at {GRID[0]} x {GRID[1]}, B = {B}{note}; max |agg - torch fp32| {c["max_abs_diff_agg_vs_torch_fp32"]:.2e}')
        for leg, other in (('k12_forward', 'torch_fp32_forward'), ('k12_forward_backward', 'torch_fp32_forward_backward')):
            ratio = (c[other]['median_ms'] / c['torch_B']) / (c[leg]['median_ms'] / B)
            print(f'  {leg:28s} {fmt(c[leg])}')
            print(f'  {other:28s} {fmt(c[other])}   [{c[other]["median_ms"] / c["torch_B"]:.4f} ms per pair]   x{ratio:.2f} of {leg}'
                  + ('   SLOWER THAN TORCH' if ratio < 1 else ''))
        print(f'  backward / forward           {c["k12_backward_over_forward"]:.2f}   (arithmetic: 3.5)')
        print(f'  peak memory of one forward + backward: K12 {c["k12_peak_mb"]:.1f} MB, torch fp32 {c["torch_fp32_peak_mb"]:.1f} MB (B = {c["torch_B"]})')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
