"""Training the 8-Point-ViT extractor's final block, timed in one process on one GPU (bench.py measures the LoFTR regressor and is not
touched):

  * K24's backward kernels alone at 28 x 28 -> 24 x 24, 128 -> 192 and 192 -> 192, at 64 images and at 2: ops.conv_valid_dgrad and
    ops.conv_valid_wgrad (gradient scale included, as a training step pays it) next to fp32 torch's convolution backward for the input
    and for the weight (aten.convolution_backward, NCHW and channels_last), and to their MFMA floor: 3 (split products) x
    2 x 576 x 25 Cin Cout flop per image at the 1.71 PFLOP/s that far_mfma_probe_f16 sustains;
  * one training step from images -- ViTEss.forward(images) + pose_loss + backward, 480 x 640 images -- at B = 1 and B = 32 pairs with
    the final block on the HIP kernels (set_extractor_training), with ONLY the final block on fp32 torch autograd, and with the
    extractor frozen (set_block_training alone: the step as it was before the final block trained).

Timing as tools/vit8pt_time.py: HIP events around groups of launches, every leg warmed up, the legs ALTERNATED round by round, medians
over the rounds with the min .. max spread.  Prints a table and one JSON line.  Usage: python tools/vit8pt_extractor_train_time.py [--rounds N]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from far_amd import ops
from tools.vit8pt_extractor_time import SIZE, stats
from tools.vit8pt_time import MFMA_RATE, alternate


def kernel_case(cin, N, rounds):
    cout = 192
    g = torch.Generator(device='cuda').manual_seed(cin + N)
    x = torch.randn(N, 28, 28, cin, device='cuda', generator=g)
    w = torch.randn(cout, cin, 5, 5, device='cuda', generator=g) * (2.0 / (25 * cin)) ** 0.5
    dy = 1e-3 * torch.randn(N, 24, 24, cout, device='cuda', generator=g)
    fwd = ops.PackedConvValid(w)
    pd = ops.PackedConvValid(w, dgrad=True, pack_scale=fwd.pack_scale)
    xn, gn = x.permute(0, 3, 1, 2).contiguous(), dy.permute(0, 3, 1, 2).contiguous()
    xcl, gcl, wcl = (t.contiguous(memory_format=torch.channels_last) for t in (xn, gn, w))

    def torch_bwd(xx, gg, ww, mask):
        return lambda: torch.ops.aten.convolution_backward(gg, xx, ww, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, mask)
    legs = {'k24_dgrad': lambda: ops.conv_valid_dgrad(dy, pd), 'k24_wgrad': lambda: ops.conv_valid_wgrad(x, dy),
            'torch_fp32_dgrad_nchw': torch_bwd(xn, gn, w, [True, False, False]),
            'torch_fp32_dgrad_channels_last': torch_bwd(xcl, gcl, wcl, [True, False, False]),
            'torch_fp32_wgrad_nchw': torch_bwd(xn, gn, w, [False, True, False]),
            'torch_fp32_wgrad_channels_last': torch_bwd(xcl, gcl, wcl, [False, True, False])}
    with torch.no_grad():
        r = alternate(legs, rounds)
        dx, dw = torch.ops.aten.convolution_backward(gn, xn, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [True, True, False])[:2]
        dev_d = float((ops.conv_valid_dgrad(dy, pd) - dx.permute(0, 2, 3, 1)).abs().max())
        dev_w = float((ops.conv_valid_wgrad(x, dy) - dw).abs().max())
    floor = 3 * 2.0 * N * 576 * 25 * cin * cout / MFMA_RATE * 1e3
    return {'images': N, 'Cin': cin, 'Cout': cout, 'mfma_floor_ms': floor, 'max_abs_diff_dgrad_vs_torch': dev_d, 'max_abs_diff_wgrad_vs_torch': dev_w,
            **stats(r)}


def torch_block(fc):
    """The final block on fp32 torch autograd, NHWC in and out (the comparison leg of tests/test_vit8pt_extractor_train_gpu.py)."""
    def run(x):
        xc = x.permute(0, 3, 1, 2)
        y = torch.relu(fc.norm1(fc.conv1(xc)))
        y = torch.relu(fc.norm2(fc.conv2(y)))
        return torch.relu(fc.downsample(xc) + y).permute(0, 2, 3, 1)
    return run


def step_case(B, rounds):
    from far_amd.vit8pt import ViTEss, pose_loss
    from tests import vit8pt_extractor_inputs as ei
    from tests import vit8pt_extractor_ref as er
    from tests import vit8pt_inputs as vi
    ref = er.RefViTEssImages(vi.vit_args())
    inp = ei.filled(ref, 1)

    def model():
        m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'], extractor=True)
        m.load_state_dict(ref.state_dict(), strict=True)
        return m.cuda().train().set_block_training()
    hip, tor, frozen = model().set_extractor_training(), model().set_extractor_training(), model()
    tor._final_block_train = torch_block(tor.extractor_final_conv)
    g = torch.Generator(device='cuda').manual_seed(B)
    images = torch.randint(0, 256, (B, 2, 3, *SIZE), device='cuda', generator=g).float()
    intr = ei.image_intrinsics(images.shape, B).cuda()
    ncorr, preds = inp['loftr_num_corr'].cuda().expand(B).contiguous(), inp['loftr_preds'].cuda().expand(B, 4, 4).contiguous()
    gt_tran, gt_rot = torch.randn(B, 3, device='cuda', generator=g), torch.randn(B, 3, 3, device='cuda', generator=g)

    def step(m):
        def run():
            m.zero_grad(set_to_none=True)
            loss = pose_loss(m(images, intr, loftr_num_corr=ncorr, loftr_preds=preds), gt_tran, gt_rot, 1.0, 1.0)
            loss.backward()
            return loss
        return run
    r = alternate({'final_block_on_hip': step(hip), 'final_block_on_torch_fp32': step(tor), 'extractor_frozen': step(frozen)}, rounds, target_ms=60.0)
    dl = abs(float(step(hip)().detach()) - float(step(tor)().detach()))
    return {'B': B, 'images': 2 * B, 'image_size': list(SIZE), 'abs_diff_of_the_loss_hip_vs_torch_block': dl, **stats(r)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vit8pt_extractor_train_time needs a GPU: nothing is timed without one')
    res = {'tool': 'vit8pt_extractor_train_time', 'device': torch.cuda.get_device_name(), 'rounds': a.rounds, 'kernels': [], 'step': []}
    fmt = lambda d: f'{d["median_ms"]:9.4f} ms  ({d["min_ms"]:.4f} .. {d["max_ms"]:.4f})'
    for N in (64, 2):
        for cin in (128, 192):
            c = kernel_case(cin, N, a.rounds)
            res['kernels'].append(c)
            print(f'# 5x5 valid convolution backward {cin} -> 192, 28 x 28 -> 24 x 24, {N} images, MFMA floor {c["mfma_floor_ms"]:.4f} ms each; '
                  f'max |dgrad - torch| {c["max_abs_diff_dgrad_vs_torch"]:.2e}, max |wgrad - torch| {c["max_abs_diff_wgrad_vs_torch"]:.2e}')
            for kind in ('dgrad', 'wgrad'):
                ours = c[f'k24_{kind}']
                print(f'  {"k24_" + kind:34s} {fmt(ours)}   {c["mfma_floor_ms"] / ours["median_ms"]:.1%} of the MFMA floor')
                for leg in (f'torch_fp32_{kind}_nchw', f'torch_fp32_{kind}_channels_last'):
                    print(f'  {leg:34s} {fmt(c[leg])}   x{c[leg]["median_ms"] / ours["median_ms"]:.2f} of k24_{kind}')
    for B in (1, 32):
        c = step_case(B, a.rounds)
        res['step'].append(c)
        print(f'# forward(images) + pose_loss + backward, B = {B} ({c["images"]} images of {SIZE[0]} x {SIZE[1]}); |loss hip - loss torch-block| '
              f'{c["abs_diff_of_the_loss_hip_vs_torch_block"]:.2e}')
        for leg in ('final_block_on_hip', 'final_block_on_torch_fp32', 'extractor_frozen'):
            print(f'  {leg:34s} {fmt(c[leg])}' + ('' if leg == 'final_block_on_hip' else f'   x{c[leg]["median_ms"] / c["final_block_on_hip"]["median_ms"]:.2f} of final_block_on_hip'))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
