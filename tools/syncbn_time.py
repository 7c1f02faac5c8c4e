"""Cost of K19's synchronised form (torch.nn.SyncBatchNorm on the HIP kernels) at the 17 BatchNorm layers of one training pair (two
480 x 640 images through ResNetFPN_8_2): forward + backward of
  (i)   K19 plain (ops.bn_act_train on nn.BatchNorm2d), as before the synchronised form existed;
  (ii)  the synchronised operator with the exchange forced, in a world-size-1 RCCL group (two float64 slot all-reduces per layer);
  (iii) torch.nn.SyncBatchNorm + torch activation / add in the same group (at world size 1 torch's module skips its collectives and
        runs the local batch_norm kernels: the figure is its floor).
One process, interleaved rounds, device events, medians.  Needs a GPU; writes the table to --out (default profiles/syncbn_time.txt).

    python tools/syncbn_time.py [--rounds 11] [--iters 40] [--out profiles/syncbn_time.txt]
"""
import argparse
import os
import statistics
import sys
from datetime import timedelta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist
import torch.nn.functional as F

from far_amd import ops, parallel

# (name, C, H, W, activation, residual, how many of the 17 layers have this shape) for N = 2 images of 480 x 640
LAYERS = [('stem / layer1 bn1', 128, 240, 320, 'relu', False, 3), ('layer1 bn2 + shortcut', 128, 240, 320, 'relu', True, 2),
          ('layer2 bn1', 196, 120, 160, 'relu', False, 2), ('layer2 bn2 + shortcut', 196, 120, 160, 'relu', True, 2),
          ('layer2 downsample', 196, 120, 160, 'none', False, 1),
          ('layer3 bn1', 256, 60, 80, 'relu', False, 2), ('layer3 bn2 + shortcut', 256, 60, 80, 'relu', True, 2),
          ('layer3 downsample', 256, 60, 80, 'none', False, 1),
          ('layer2_outconv2', 256, 120, 160, 'leaky', False, 1), ('layer1_outconv2', 196, 240, 320, 'leaky', False, 1)]
SLOPE = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'syncbn_time.txt'))
    a = ap.parse_args()
    assert sum(l[-1] for l in LAYERS) == 17
    if not torch.cuda.is_available():
        sys.exit('syncbn_time.py measures on the GPU: none found')
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{parallel.free_port()}', rank=0, world_size=1, device_id=dev,
                            timeout=timedelta(seconds=60))
    ops.USE_HIP_SYNC_BATCHNORM = True
    N = 2
    lines = [f'BatchNorm + activation (+ shortcut add), forward + backward, at the 17 layer shapes of one training pair (N = 2, 480 x 640), '
             f'{torch.cuda.get_device_name(0)}',
             f'{a.rounds} interleaved rounds of {a.iters} calls per leg after one warm-up round, device events; median microseconds per call '
             f'(spread = (max - min) / median over the rounds)',
             '(i) K19 plain   (ii) K19 synchronised, exchange forced, world-size-1 RCCL group   (iii) torch.nn.SyncBatchNorm + torch act / add, same group',
             f'{"layer":<24}{"C":>5}{"H x W":>11}{"x":>3}{"(i)":>10}{"(ii)":>10}{"(iii)":>10}{"(ii)/(i)":>10}{"(ii)/(iii)":>11}{"spread i / ii / iii":>24}']
    tot = [0.0, 0.0, 0.0]
    for name, C, H, W, act, res, count in LAYERS:
        g = torch.Generator(device='cuda').manual_seed(C + H)
        cl = torch.channels_last
        x = (torch.randn(N, C, H, W, device=dev, generator=g) * 1.7 + 30.0).contiguous(memory_format=cl).requires_grad_()
        r = torch.randn(N, C, H, W, device=dev, generator=g).contiguous(memory_format=cl).requires_grad_() if res else None
        up = torch.randn(N, C, H, W, device=dev, generator=g).contiguous(memory_format=cl)
        plain = torch.nn.BatchNorm2d(C).to(dev).train()
        sync = torch.nn.SyncBatchNorm(C).to(dev).train()
        vend = torch.nn.SyncBatchNorm(C).to(dev).train()

        def torch_leg():
            y = vend(x)
            if r is not None:
                y = y + r
            return torch.relu(y) if act == 'relu' else (F.leaky_relu(y, SLOPE) if act == 'leaky' else y)
        legs = [lambda: ops.bn_act_train(x, plain, act, SLOPE, residual=r),
                lambda: ops.bn_act_train(x, sync, act, SLOPE, residual=r, force_exchange=True),
                torch_leg]

        def run(leg):
            x.grad = None
            if r is not None:
                r.grad = None
            leg().backward(up)
        times = [[], [], []]
        for rnd in range(a.rounds + 1):
            for i, leg in enumerate(legs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    run(leg)
                e1.record()
                e1.synchronize()
                if rnd:                                        # round 0 warms every shape of every leg up
                    times[i].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med = [statistics.median(t) for t in times]
        spr = [(max(t) - min(t)) / m for t, m in zip(times, med)]
        for i in range(3):
            tot[i] += med[i] * count
        lines.append(f'{name:<24}{C:>5}{f"{H} x {W}":>11}{count:>3}{med[0]:>10.1f}{med[1]:>10.1f}{med[2]:>10.1f}{med[1] / med[0]:>10.3f}{med[1] / med[2]:>11.3f}'
                     f'{f"{spr[0]:.1%} / {spr[1]:.1%} / {spr[2]:.1%}":>24}')
    lines.append(f'{"all 17 layers":<24}{"":>5}{"":>11}{17:>3}{tot[0]:>10.1f}{tot[1]:>10.1f}{tot[2]:>10.1f}{tot[1] / tot[0]:>10.3f}{tot[1] / tot[2]:>11.3f}')
    lines.append(f'(ii) - (i) per layer: {(tot[1] - tot[0]) / 17:.1f} microseconds (two all-reduces of a zeroed float64 buffer and two more launch boundaries)')
    dist.destroy_process_group()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
