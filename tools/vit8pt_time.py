"""The 8-Point-ViT path timed in one process on one GPU (bench.py measures the LoFTR regressor and is not touched):

  * K23 (far_vit_attention_f16s through ops.vit_attention_planes) at the production shape L = S = 576, 3 heads x 64, for B = 1 and
    B = 32 pairs (Z = 2 and 64 images), next to the fp32 torch composition of the same operator (scores materialised, softmax,
    P V) and torch's fused scaled_dot_product_attention on fp32 inputs;
  * one ViTEss.forward_features call (5 Blocks, CrossBlock, LayerNorm, head) at B = 1 and B = 32, next to the fp32 torch
    restatement of the same model (tests/vit8pt_ref.py) on the same weights;
  * training (--legs train): K23's training forward + HIP backward (ops.vit_attention_train_qkv on one (Z, N, 3 C) projection) at
    the same shape for Z = 2 and Z = 64, its raw forward and raw backward launches on their own (the backward / forward ratio),
    next to fp32 torch autograd of the materialising composition and of scaled_dot_product_attention;
  * one training iteration without the optimizer -- forward_features + pose_loss + backward with set_block_training() -- at B = 1
    and B = 32, next to the fp32 torch restatement under autograd (tests/vit8pt_train_ref.py).

Timing: HIP events around groups of launches (a group is long enough that the event resolution and the launch gaps do not decide),
every leg warmed up first, the legs ALTERNATED round by round, medians over the rounds with the min .. max spread.  The MFMA floor
of K23 is 3 (split products) x 4 L S H 64 Z flop at the 1.71 PFLOP/s that far_mfma_probe_f16 sustains.
--precision fp16 (inference legs): the 16-bit-operand mode of ViTEss.set_precision next to the default one IN THE SAME PROCESS on the
same inputs -- K23 on plain fp16 operands (far_vit_attention_f16, leg k23_f16) alternating with K23, and forward_features of a second
model on the same weights with every trunk stage on 16-bit operands (leg far_amd_fp16) alternating with the fp32-grade model; the
deviation of each from the fp32 torch computation is printed next to the gain (the mode is narrower than the reference).
Prints a table and one JSON line.  Usage: python tools/vit8pt_time.py [--rounds N] [--legs inference,train] [--precision fp32|fp16]"""
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


def attention_case(B, rounds, fp16=False):
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
    if fp16:
        legs = {'k23': legs['k23'], 'k23_f16': lambda: ops.vit_attention_planes(planes, H, plain16=True), 'torch_fp32_composition': composition}
    try:                                     # a torch build without an fp32 fused path: the leg is left out, and the table says so
        sdpa()
        legs['torch_fp32_sdpa'] = sdpa
    except RuntimeError as e:
        print(f'# torch_fp32_sdpa not timed: {str(e).splitlines()[0]}')
    r = alternate(legs, rounds)
    dev = float((ops.vit_attention_planes(planes, H) - composition()).abs().max())
    floor = 3 * 4.0 * N * N * H * 64 * Z / MFMA_RATE * 1e3
    extra = {'max_abs_diff_vs_composition_f16': float((ops.vit_attention_planes(planes, H, plain16=True) - composition()).abs().max())} if fp16 else {}
    return {'B': B, 'Z': Z, 'workgroups': Z * H * ((N + 127) // 128), 'mfma_floor_ms': floor, 'max_abs_diff_vs_composition': dev, **extra,
            **{name: {'median_ms': m, 'min_ms': lo, 'max_ms': hi} for name, (m, lo, hi) in r.items()}}


def model_case(B, rounds, fp16=False):
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
    legs, extra = {'far_amd': ours, 'torch_fp32_restatement': theirs}, {}
    if fp16:
        m16 = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'])
        m16.load_state_dict(m.state_dict(), strict=True)
        m16 = m16.eval().cuda().set_precision(ViTEss.STAGES[1:])              # every stage of the trunk (this model has no extractor)

        def ours16():
            with torch.no_grad():
                return m16.forward_features(feats, intr, ncorr, preds)
        legs = {'far_amd': ours, 'far_amd_fp16': ours16, 'torch_fp32_restatement': theirs}
    r = alternate(legs, rounds, target_ms=60.0)
    dev = max(float((a - b).abs().max()) for a, b in zip(ours(), theirs()))
    if fp16:
        extra = {'max_abs_diff_of_the_outputs_fp16': max(float((a - b).abs().max()) for a, b in zip(ours16(), theirs()))}
    return {'B': B, 'max_abs_diff_of_the_outputs': dev, **extra, **{name: {'median_ms': md, 'min_ms': lo, 'max_ms': hi} for name, (md, lo, hi) in r.items()}}


def attention_train_case(B, rounds):
    H, N, Z = 3, 576, 2 * B
    C = H * 64
    g = torch.Generator(device='cuda').manual_seed(B)
    qkv = (torch.randn(Z, N, 3 * C, device='cuda', generator=g) * 1.5).requires_grad_()
    go = torch.randn(Z, N, C, device='cuda', generator=g)
    q4, k4, v4 = (qkv.detach()[..., t * C:(t + 1) * C].reshape(Z, N, H, 64).transpose(1, 2).contiguous().requires_grad_() for t in range(3))
    g4 = go.reshape(Z, N, H, 64).transpose(1, 2).contiguous()
    from far_amd.ops import attention as at
    raw = qkv.detach()
    views = (raw[..., :C], raw[..., C:2 * C], raw[..., 2 * C:])
    out, lse, act_exp = at._vit_train_forward(*views, Z, N, N, H)
    into = torch.empty_like(raw)

    def through(fn, leaves):
        def run():
            for t in leaves:
                t.grad = None
            fn().backward(go if leaves[0] is qkv else g4)
        return run

    def composition():
        a = (q4 @ k4.transpose(-2, -1)) * 0.125
        return a.softmax(dim=-1) @ v4

    def sdpa():
        return torch.nn.functional.scaled_dot_product_attention(q4, k4, v4)
    legs = {'k23_train_forward': lambda: at._vit_train_forward(*views, Z, N, N, H),
            'k23_backward': lambda: ops.vit_attention_bwd(*views, out, lse, go, H, act_exp, into=into),
            'k23_forward_backward': through(lambda: ops.vit_attention_train_qkv(qkv, H), (qkv,)),
            'torch_fp32_composition_autograd': through(composition, (q4, k4, v4))}
    try:                                     # a torch build without an fp32 fused path with a backward: the leg is left out
        through(sdpa, (q4, k4, v4))()
        legs['torch_fp32_sdpa_autograd'] = through(sdpa, (q4, k4, v4))
    except RuntimeError as e:
        print(f'# torch_fp32_sdpa_autograd not timed: {str(e).splitlines()[0]}')
    r = alternate(legs, rounds)
    legs['k23_forward_backward']()
    legs['torch_fp32_composition_autograd']()
    ref = torch.cat([t.grad.transpose(1, 2).reshape(Z, N, C) for t in (q4, k4, v4)], dim=-1)
    dev = float((qkv.grad - ref).norm() / ref.norm())
    return {'B': B, 'Z': Z, 'rel_frobenius_diff_of_dqkv_vs_composition': dev,
            'backward_over_forward': r['k23_backward'][0] / r['k23_train_forward'][0],
            **{name: {'median_ms': m, 'min_ms': lo, 'max_ms': hi} for name, (m, lo, hi) in r.items()}}


def model_train_case(B, rounds):
    from far_amd.vit8pt import ViTEss, pose_loss
    from tests import vit8pt_inputs as vi
    from tests import vit8pt_ref as vr
    from tests import vit8pt_train_ref as vtr
    ref = vr.RefViTEss(vi.vit_args())
    inp = vi.seeded_inputs(vi.seeded_fill(ref), 1)
    ref.pose_mean, ref.pose_std = inp['pose_mean'], inp['pose_std']
    m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'])
    m.load_state_dict(ref.state_dict(), strict=True)
    m, ref = m.cuda().train().set_block_training(), vtr.from_ref(ref, torch.float32, 'cuda').train()
    g = torch.Generator(device='cuda').manual_seed(100 + B)
    feats = torch.randn(2 * B, 576, 192, device='cuda', generator=g)
    gt_tran, gt_rot = torch.randn(B, 3, device='cuda', generator=g), torch.randn(B, 3, 3, device='cuda', generator=g)
    intr = inp['intrinsics'].cuda().expand(B, 2, 4).contiguous()
    ncorr, preds = inp['loftr_num_corr'].cuda().expand(B).contiguous(), inp['loftr_preds'].cuda().expand(B, 4, 4).contiguous()

    def step(model, k):
        def run():
            model.zero_grad(set_to_none=True)
            loss = pose_loss(model.forward_features(feats, k, ncorr, preds), gt_tran, gt_rot, 1.0, 1.0)
            loss.backward()
            return loss
        return run
    ours, theirs = step(m, intr), step(ref, vi.VIT_INTRINSICS)
    r = alternate({'far_amd': ours, 'torch_fp32_restatement': theirs}, rounds, target_ms=60.0)
    dl = abs(float(ours().detach()) - float(theirs().detach()))
    name = 'fusion_transformer.blocks.0.attn.qkv.weight'
    ga, gb = dict(m.named_parameters())[name].grad, dict(ref.named_parameters())[name].grad
    return {'B': B, 'abs_diff_of_the_loss': dl, 'rel_frobenius_diff_of_block0_dqkv_weight': float((ga - gb).norm() / gb.norm()),
            **{nm: {'median_ms': md, 'min_ms': lo, 'max_ms': hi} for nm, (md, lo, hi) in r.items()}}


def main_train(a, res, fmt):
    res['attention_train'], res['train_iteration'] = [], []
    for B in (1, 32):
        c = attention_train_case(B, a.rounds)
        res['attention_train'].append(c)
        print(f'# attention training L = S = 576, H = 3, D = 64, Z = {c["Z"]}; backward / forward = {c["backward_over_forward"]:.2f} '
              f'(K22: 2.4-3.0); rel Frobenius difference of dqkv against the fp32 composition {c["rel_frobenius_diff_of_dqkv_vs_composition"]:.2e}')
        for leg in (n for n in ('k23_train_forward', 'k23_backward', 'k23_forward_backward', 'torch_fp32_composition_autograd',
                                'torch_fp32_sdpa_autograd') if n in c):
            print(f'  {leg:34s} {fmt(c[leg])}' + (f'   x{c[leg]["median_ms"] / c["k23_forward_backward"]["median_ms"]:.2f} of K23 forward + backward'
                                                if leg.startswith('torch') else ''))
    for B in (1, 32):
        c = model_train_case(B, a.rounds)
        res['train_iteration'].append(c)
        print(f'# forward_features + pose_loss + backward B = {B} (depth 6, gating, normalized 6d); |loss difference| {c["abs_diff_of_the_loss"]:.2e}, '
              f'block 0 dqkv.weight rel Frobenius difference {c["rel_frobenius_diff_of_block0_dqkv_weight"]:.2e}')
        for leg in ('far_amd', 'torch_fp32_restatement'):
            print(f'  {leg:34s} {fmt(c[leg])}' + (f'   x{c[leg]["median_ms"] / c["far_amd"]["median_ms"]:.2f} of far_amd' if leg != 'far_amd' else ''))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--legs', default='inference,train', help='comma-separated: inference, train')
    ap.add_argument('--precision', choices=('fp32', 'fp16'), default='fp32',
                    help='fp16: the 16-bit-operand kernels / mode next to the default ones, in the same process (inference legs)')
    a = ap.parse_args()
    which = set(a.legs.split(','))
    if not torch.cuda.is_available():
        raise SystemExit('vit8pt_time needs a GPU: nothing is timed without one')
    fp16 = a.precision == 'fp16'
    res = {'tool': 'vit8pt_time', 'device': torch.cuda.get_device_name(), 'rounds': a.rounds, 'precision': a.precision, 'attention': [],
           'forward_features': []}
    fmt = lambda d: f'{d["median_ms"]:9.4f} ms  ({d["min_ms"]:.4f} .. {d["max_ms"]:.4f})'
    for B in (1, 32) if 'inference' in which else ():
        c = attention_case(B, a.rounds, fp16)
        res['attention'].append(c)
        print(f'# attention L = S = 576, H = 3, D = 64, B = {B} (Z = {c["Z"]}, {c["workgroups"]} workgroups), MFMA floor {c["mfma_floor_ms"]:.4f} ms')
        for leg in (n for n in ('k23', 'k23_f16', 'torch_fp32_composition', 'torch_fp32_sdpa') if n in c):
            print(f'  {leg:26s} {fmt(c[leg])}' + (f'   x{c[leg]["median_ms"] / c["k23"]["median_ms"]:.2f} of K23' if leg != 'k23' else
                                                f'   {c["mfma_floor_ms"] / c[leg]["median_ms"]:.1%} of the MFMA floor'))
        if fp16:
            print(f'  max |out - fp32 composition|: K23 {c["max_abs_diff_vs_composition"]:.2e}, plain fp16 {c["max_abs_diff_vs_composition_f16"]:.2e}')
    for B in (1, 32) if 'inference' in which else ():
        c = model_case(B, a.rounds, fp16)
        res['forward_features'].append(c)
        print(f'# forward_features B = {B} (depth 6, gating, normalized 6d); max |output difference| {c["max_abs_diff_of_the_outputs"]:.2e}')
        for leg in (n for n in ('far_amd', 'far_amd_fp16', 'torch_fp32_restatement') if n in c):
            print(f'  {leg:26s} {fmt(c[leg])}' + (f'   x{c[leg]["median_ms"] / c["far_amd"]["median_ms"]:.2f} of far_amd' if leg != 'far_amd' else ''))
        if fp16:
            print(f'  max |output - fp32 restatement|: fp32 mode {c["max_abs_diff_of_the_outputs"]:.2e}, 16-bit trunk stages {c["max_abs_diff_of_the_outputs_fp16"]:.2e}')
    if 'train' in which:
        main_train(a, res, fmt)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
