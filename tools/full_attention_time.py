"""The full softmax attention core (far_full_attention_f16s, K22) timed in one process: HIP events around each launch (no host
synchronisation inside the timed region), warm-up, then REPS repetitions; the median of each.
  * kernel time at the coarse shape (N = 64 image-calls = batch 32, L = S = 4800, H = 8, D = 32) and at the fine-window shape
    (N windows of 25 tokens, D = 16), next to two arithmetic floors: the MFMA floor 3 x 4 L S H D N flop at the probed sustained
    f16 MFMA rate of this repository (1.71 PFLOP/s) and the exponential floor, one exp per score at the transcendental rate
    (256 CUs x 4 SIMDs x 16 lanes / 4 per cycle at 2.4 GHz);
  * N = 4, L = S = 4800 against the materialising fp32 torch composition of linear_attention.py:74-86 on the same GPU (the one hard
    condition: the kernel is faster);
  * far_amd.pipeline.test_step with coarse.attention = 'full' against 'linear' at the bench shape (32 pairs of 480 x 640).
  * --train: forward + backward of ops.full_attention_train (K22's training forward, then the backward kernels of
    full_attention_bwd_f16s.hip) at the coarse shape (N = 4 and 64) and at the fine-window shape, the backward / forward ratio, and at
    N = 4 fp32 torch autograd of the materialising composition on the same GPU (the hard condition of the training path: forward +
    backward of the kernels is faster).  Only these legs run.
Prints one JSON line.  Usage: python tools/full_attention_time.py [--reps N] [--no-step] [--train]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from far_amd import ops

MFMA_RATE = 1.71e15                     # flop/s, f16 MFMA sustained: the rate far_mfma_probe_f16 measured
EXP_RATE = 256 * 4 * 16 / 4 * 2.4e9     # exponentials/s: quarter-rate transcendental unit


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def kernel_case(N, L, S, H, D, reps, seed=1):
    g = torch.Generator(device='cuda').manual_seed(seed)
    q, k, v = (torch.randn(N, n, H * D, device='cuda', generator=g) for n in (L, S, S))
    med, lo, hi = timed(lambda: ops.full_attention(q, k, v, H), reps)
    mfma = 3 * 4.0 * L * S * H * D * N / MFMA_RATE * 1e3
    exps = 1.0 * L * S * H * N / EXP_RATE * 1e3
    return {'N': N, 'L': L, 'S': S, 'H': H, 'D': D, 'kernel_ms': round(med, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
            'mfma_floor_ms': round(mfma, 4), 'exp_floor_ms': round(exps, 4), 'fraction_of_mfma_floor': round(mfma / med, 3),
            'fraction_of_max_floor': round(max(mfma, exps) / med, 3), 'reps': reps}


def against_torch(reps):
    N, L, H, D = 4, 4800, 8, 32
    g = torch.Generator(device='cuda').manual_seed(2)
    q, k, v = (torch.randn(N, L, H * D, device='cuda', generator=g) for _ in range(3))

    def composition():
        Q, K, V = (t.view(N, L, H, D) for t in (q, k, v))
        QK = torch.einsum('nlhd,nshd->nlsh', Q, K)                       # the (N, L, S, H) score tensor: 2.9 GB
        A = torch.softmax(QK / D ** .5, dim=2)
        return torch.einsum('nlsh,nshd->nlhd', A, V).contiguous()
    tk = timed(lambda: ops.full_attention(q, k, v, H), reps)[0]
    tt = timed(composition, max(reps // 4, 5), warm=2)[0]
    return {'N': N, 'L': L, 'kernel_ms': round(tk, 4), 'torch_fp32_materialising_ms': round(tt, 4), 'torch_over_kernel': round(tt / tk, 2),
            'kernel_is_faster': tk < tt}


def train_case(N, L, S, H, D, reps, seed=3, torch_leg=False):
    """Forward alone, forward + backward and (their difference) the backward of ops.full_attention_train; torch_leg: fp32 autograd
    of the materialising composition next to it."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    q, k, v, go = (torch.randn(N, n, H * D, device='cuda', generator=g) for n in (L, S, S, L))
    q.requires_grad_(); k.requires_grad_(); v.requires_grad_()

    def fwd_bwd():
        torch.autograd.grad(ops.full_attention_train(q, k, v, H), (q, k, v), go)
    tf = timed(lambda: ops.full_attention_train(q, k, v, H), reps)[0]
    tfb = timed(fwd_bwd, reps)[0]
    mfma = (3 * 4.0 + (3 + 3 + 1) * 2.0 + (3 + 3 + 2) * 2.0) * L * S * H * D * N / MFMA_RATE * 1e3   # forward; dq kernel; dk/dv kernel
    out = {'N': N, 'L': L, 'S': S, 'H': H, 'D': D, 'forward_ms': round(tf, 4), 'forward_backward_ms': round(tfb, 4),
           'backward_ms': round(tfb - tf, 4), 'backward_over_forward': round((tfb - tf) / tf, 2), 'mfma_floor_ms': round(mfma, 4),
           'fraction_of_mfma_floor': round(mfma / tfb, 3), 'reps': reps}
    if torch_leg:
        def composition():
            Q, K, V = (t.view(N, n, H, D) for t, n in ((q, L), (k, S), (v, S)))
            QK = torch.einsum('nlhd,nshd->nlsh', Q, K)
            A = torch.softmax(QK / D ** .5, dim=2)
            out = torch.einsum('nlsh,nshd->nlhd', A, V).reshape(N, L, H * D)
            torch.autograd.grad(out, (q, k, v), go)
        tt = timed(composition, max(reps // 4, 5), warm=2)[0]
        out.update(torch_fp32_autograd_ms=round(tt, 4), torch_over_kernel=round(tt / tfb, 2), kernel_is_faster=tfb < tt)
    return out


def step_times(reps):
    from far_amd import synth
    from far_amd.config import far_eval_config
    from far_amd.loftr import LoFTR
    from far_amd.pipeline import test_step
    im0, im1 = synth.synth_image_pair(32, seed=0)
    K = torch.from_numpy(np.stack([synth.MP3D_K] * 32)).cuda()
    out = {}
    for att in ('linear', 'full'):
        cfg = far_eval_config()
        cfg['coarse']['attention'] = att
        m = LoFTR(cfg).eval()
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synthetic_state_dict(shapes, 0).items()})
        m = m.cuda()

        def step():
            d = {'image0': torch.from_numpy(im0).cuda(), 'image1': torch.from_numpy(im1).cuda(), 'K0': K, 'K1': K.clone(), 'dataset_name': ['mp3d']}
            test_step(m, d, H=480)
        out[att + '_step_ms'] = round(timed(step, reps, warm=3)[0], 3)
    out['full_over_linear'] = round(out['full_step_ms'] / out['linear_step_ms'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--train', action='store_true')
    a = ap.parse_args()
    if a.train:
        res = {'tool': 'full_attention_time --train', 'device': torch.cuda.get_device_name(),
               'coarse_n4': train_case(4, 4800, 4800, 8, 32, a.reps, torch_leg=True), 'coarse_n64': train_case(64, 4800, 4800, 8, 32, a.reps),
               'fine_windows': train_case(16384, 25, 25, 8, 16, a.reps)}
        res['overflow'] = bool(ops.overflow_flag(torch.device('cuda')).item())
        print(json.dumps(res), flush=True)
        return
    res = {'tool': 'full_attention_time', 'device': torch.cuda.get_device_name(),
           'coarse': kernel_case(64, 4800, 4800, 8, 32, a.reps), 'mapfree_c5': kernel_case(32, 6120, 6120, 8, 32, a.reps),
           'batch1': kernel_case(2, 4800, 4800, 8, 32, a.reps), 'fine_windows': kernel_case(16384, 25, 25, 8, 16, a.reps),
           'against_torch': against_torch(a.reps)}
    if not a.no_step:
        res['test_step_32_pairs'] = step_times(max(a.reps // 2, 5))
    res['overflow'] = bool(ops.overflow_flag(torch.device('cuda')).item())
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
