"""The 8-Point-ViT path timed in one process on one GPU (bench.py measures the LoFTR regressor and is not touched):

  * K23 (far_vit_attention_f16s through ops.vit_attention_planes) at the production shape L = S = 576, 3 heads x 64, for B = 1 and
    B = 32 pairs (Z = 2 and 64 images), next to the fp32 torch composition of the same operator (scores materialised, softmax,
    P V) and torch's fused scaled_dot_product_attention on fp32 inputs;
  * one ViTEss.forward_features call (5 Blocks, CrossBlock, LayerNorm, head) at B = 1 and B = 32, next to the fp32 torch
    restatement of the same model (tests/vit8pt_ref.py) on the same weights.

Timing: HIP events around groups of launches (a group is long enough that the event resolution and the launch gaps do not decide),
every leg warmed up first, the legs ALTERNATED round by round, medians over the rounds with the min .. max spread.  The MFMA floor
of K23 is 3 (split products) x 4 L S H 64 Z flop at the 1.71 PFLOP/s that far_mfma_probe_f16 sustains.
Prints a table and one JSON line.  Usage: python tools/vit8pt_time.py [--rounds N]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from far_amd import ops

MFMA_RATE = 1.71e15


def group_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(legs, rounds, target_ms=30.0):
    """legs: {name: fn}.  -> {name: (median, min, max) ms per call}; every round times each leg once, in turn."""
    per = {}
    for name, fn in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        per[name] = max(1, min(200, int(target_ms / max(group_ms(fn, 3), 1e-3))))
    ts = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            ts[name].append(group_ms(fn, per[name]))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ts.items()}


def attention_case(B, rounds):
    H, N, Z = 3, 576, 2 * B
    g = torch.Generator(device='cuda').manual_seed(B)
    planes = torch.randn(3 * H, Z, N, 64, device='cuda', generator=g) * 1.5
    q, k, v = (planes[t * H:(t + 1) * H].permute(1, 0, 2, 3).contiguous() for t in range(3))       # (Z, H, N, 64)

    def composition():
        a = (q @ k.transpose(-2, -1)) * 0.125
        return (a.softmax(dim=-1) @ v).transpose(1, 2).reshape(Z, N, H * 64)

    def sdpa():
        return torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(Z, N, H * 64)
    legs = {'k23': lambda: ops.vit_attention_planes(planes, H), 'torch_fp32_composition': composition}
    try:                                     # a torch build without an fp32 fused path: the leg is left out, and the table says so
        sdpa()
        legs['torch_fp32_sdpa'] = sdpa
    except RuntimeError as e:
        print(f'# torch_fp32_sdpa not timed: {str(e).splitlines()[0]}')
    r = alternate(legs, rounds)
    dev = float((ops.vit_attention_planes(planes, H) - composition()).abs().max())
    floor = 3 * 4.0 * N * N * H * 64 * Z / MFMA_RATE * 1e3
    return {'B': B, 'Z': Z, 'workgroups': Z * H * ((N + 127) // 128), 'mfma_floor_ms': floor, 'max_abs_diff_vs_composition': dev,
            **{name: {'median_ms': m, 'min_ms': lo, 'max_ms': hi} for name, (m, lo, hi) in r.items()}}


def model_case(B, rounds):
    from far_amd.vit8pt import ViTEss
    from tests import vit8pt_inputs as vi
    from tests import vit8pt_ref as vr
    ref = vr.RefViTEss(vi.vit_args())
    inp = vi.seeded_inputs(vi.seeded_fill(ref), 1)
    ref.pose_mean, ref.pose_std = inp['pose_mean'], inp['pose_std']
    m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'])
    m.load_state_dict(ref.state_dict(), strict=True)
    m, ref = m.eval().cuda(), ref.as_dtype(torch.float32, 'cuda')
    g = torch.Generator(device='cuda').manual_seed(100 + B)
    feats = torch.randn(2 * B, 576, 192, device='cuda', generator=g)
    intr = inp['intrinsics'].cuda().expand(B, 2, 4).contiguous()
    ncorr, preds = inp['loftr_num_corr'].cuda().expand(B).contiguous(), inp['loftr_preds'].cuda().expand(B, 4, 4).contiguous()

    def ours():
        with torch.no_grad():
            return m.forward_features(feats, intr, ncorr, preds)

    def theirs():
        return ref.forward_features(feats, vi.VIT_INTRINSICS, ncorr, preds)
    r = alternate({'far_amd': ours, 'torch_fp32_restatement': theirs}, rounds, target_ms=60.0)
    dev = max(float((a - b).abs().max()) for a, b in zip(ours(), theirs()))
    return {'B': B, 'max_abs_diff_of_the_outputs': dev, **{name: {'median_ms': md, 'min_ms': lo, 'max_ms': hi} for name, (md, lo, hi) in r.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vit8pt_time needs a GPU: nothing is timed without one')
    res = {'tool': 'vit8pt_time', 'device': torch.cuda.get_device_name(), 'rounds': a.rounds, 'attention': [], 'forward_features': []}
    fmt = lambda d: f'{d["median_ms"]:9.4f} ms  ({d["min_ms"]:.4f} .. {d["max_ms"]:.4f})'
    for B in (1, 32):
        c = attention_case(B, a.rounds)
        res['attention'].append(c)
        print(f'# attention L = S = 576, H = 3, D = 64, B = {B} (Z = {c["Z"]}, {c["workgroups"]} workgroups), MFMA floor {c["mfma_floor_ms"]:.4f} ms')
        for leg in (n for n in ('k23', 'torch_fp32_composition', 'torch_fp32_sdpa') if n in c):
            print(f'  {leg:26s} {fmt(c[leg])}' + (f'   x{c[leg]["median_ms"] / c["k23"]["median_ms"]:.2f} of K23' if leg != 'k23' else
                                                f'   {c["mfma_floor_ms"] / c[leg]["median_ms"]:.1%} of the MFMA floor'))
    for B in (1, 32):
        c = model_case(B, a.rounds)
        res['forward_features'].append(c)
        print(f'# forward_features B = {B} (depth 6, gating, normalized 6d); max |output difference| {c["max_abs_diff_of_the_outputs"]:.2e}')
        for leg in ('far_amd', 'torch_fp32_restatement'):
            print(f'  {leg:26s} {fmt(c[leg])}' + (f'   x{c[leg]["median_ms"] / c["far_amd"]["median_ms"]:.2f} of far_amd' if leg != 'far_amd' else ''))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
