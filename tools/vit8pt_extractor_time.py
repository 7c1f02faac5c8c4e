"""The 8-Point-ViT's extractor timed in one process on one GPU (bench.py measures the LoFTR regressor and is not touched), at B = 1 and
B = 32 pairs (2 and 64 images of 480 x 640):

  * ViTEss.extract_features (14 launches) and its kernels on their own -- K25 (ops.stem_rgb), K26 (ops.maxpool3x3s2), the K9 / K17
    layers (layer1, layer2, extractor_final_conv.conv1), K24 (ops.conv_valid) for the 192 -> 192 and the 128 -> 192 convolution --
    next to the fp32 torch composition of the same layers (tests/vit8pt_extractor_ref.py on the same weights);
  * the 5x5 kernel alone at 28 x 28 -> 24 x 24 next to torch.nn.functional.conv2d in fp32 (NCHW and channels_last), to the route the
    repository could already take (F.unfold + a K9 Linear over 25 Cin columns), and to its MFMA floor: 3 (split products) x
    2 x 576 x 25 Cin Cout flop per image at the 1.71 PFLOP/s that far_mfma_probe_f16 sustains;
  * end to end: ViTEss.forward(images) next to the torch extractor followed by today's forward_features.

Timing as tools/vit8pt_time.py: HIP events around groups of launches, every leg warmed up, the legs ALTERNATED round by round, medians
over the rounds with the min .. max spread.
--precision fp16: the 16-bit-operand mode of ViTEss.set_precision next to the default one IN THE SAME PROCESS on the same inputs -- K24 on
plain fp16 operands (far_conv_valid_f16, leg k24_f16) alternating with K24, and extract_features / forward(images) of a second model on
the same weights in mode 'fp16' (legs *_fp16) alternating with the fp32-grade model; deviations are printed next to the gains (the mode
is narrower than the reference).
Prints a table and one JSON line.  Usage: python tools/vit8pt_extractor_time.py [--rounds N] [--precision fp32|fp16]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from far_amd import ops
from tools.vit8pt_time import MFMA_RATE, alternate

SIZE = (480, 640)


def models():
    from far_amd.vit8pt import ViTEss
    from tests import vit8pt_extractor_inputs as ei
    from tests import vit8pt_extractor_ref as er
    from tests import vit8pt_inputs as vi
    ref = er.RefViTEssImages(vi.vit_args())
    inp = ei.filled(ref, 1)
    ref.pose_mean, ref.pose_std = inp['pose_mean'], inp['pose_std']
    m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'], extractor=True)
    m.load_state_dict(ref.state_dict(), strict=True)
    return m.eval().cuda(), ref.as_dtype(torch.float32, 'cuda'), inp


def stats(r):
    return {name: {'median_ms': m, 'min_ms': lo, 'max_ms': hi} for name, (m, lo, hi) in r.items()}


def extractor_case(m, ref, inp, B, rounds, m16=None):
    from tests import vit8pt_extractor_inputs as ei
    g = torch.Generator(device='cuda').manual_seed(B)
    images = torch.randint(0, 256, (B, 2, 3, *SIZE), device='cuda', generator=g).float()
    flat = images.flatten(0, 1)
    intr = ei.image_intrinsics(images.shape, B).cuda()
    ncorr, preds = inp['loftr_num_corr'].cuda().expand(B).contiguous(), inp['loftr_preds'].cuda().expand(B, 4, 4).contiguous()
    with torch.no_grad():
        feats = m.extract_features(images)[0]                                  # builds the packs
        pk, rn, fc = m._extractor_packs._store, m.resnet, m.extractor_final_conv
        get = lambda k: pk[k if k == 'stem' else (k, m.extractor_split)][1]
        s = ops.stem_rgb(flat, get('stem'))
        p = ops.maxpool3x3s2(s)
        x = p
        for lname, layer in (('layer1', rn.layer1), ('layer2', rn.layer2)):
            for i, blk in enumerate(layer):
                x = m._block(m._extractor_packs, f'{lname}.{i}', blk, x)
        y1 = ops.conv_nhwc(x, get('final.conv1'), act='relu')
        y2 = ops.conv_valid(y1, get('final.conv2'), act='relu')

    def k9_layers():
        z = p
        for lname, layer in (('layer1', rn.layer1), ('layer2', rn.layer2)):
            for i, blk in enumerate(layer):
                z = m._block(m._extractor_packs, f'{lname}.{i}', blk, z)
        return ops.conv_nhwc(z, get('final.conv1'), act='relu')

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    grid = m.update_intrinsics(images.shape, intr)
    legs = {'extract_features': lambda: m.extract_features(images),
            'k25_stem_rgb': lambda: ops.stem_rgb(flat, get('stem')),
            'k26_maxpool': lambda: ops.maxpool3x3s2(s),
            'k9_k17_layers': k9_layers,
            'k24_conv2_192_192': lambda: ops.conv_valid(y1, get('final.conv2'), act='relu'),
            'k24_downsample_128_192': lambda: ops.conv_valid(x, get('final.downsample'), residual=y2, act='relu'),
            'torch_fp32_extractor': lambda: ref.extract_features(images),
            'forward_images': lambda: m(images, intr, loftr_num_corr=ncorr, loftr_preds=preds),
            'torch_extractor_then_forward_features': lambda: m.forward_features(ref.extract_features(images).contiguous(), grid, ncorr, preds)}
    extra = {}
    if m16 is not None:
        legs['extract_features_fp16'] = lambda: m16.extract_features(images)
        legs['forward_images_fp16'] = lambda: m16(images, intr, loftr_num_corr=ncorr, loftr_preds=preds)
    r = alternate({k: nograd(v) for k, v in legs.items()}, rounds, target_ms=40.0)
    dev = float((feats - ref.extract_features(images)).abs().max())
    if m16 is not None:
        with torch.no_grad():
            extra = {'max_abs_diff_of_the_features_vs_torch_fp32_fp16': float((m16.extract_features(images)[0] - ref.extract_features(images)).abs().max()),
                     'max_abs_features': float(feats.abs().max())}
    return {'B': B, 'images': 2 * B, 'image_size': list(SIZE), 'max_abs_diff_of_the_features_vs_torch_fp32': dev, **extra, **stats(r)}


def conv5_case(cin, B, rounds, fp16=False):
    N, cout = 2 * B, 192
    g = torch.Generator(device='cuda').manual_seed(cin + B)
    x = torch.randn(N, 28, 28, cin, device='cuda', generator=g)
    w = torch.randn(cout, cin, 5, 5, device='cuda', generator=g) * (2.0 / (25 * cin)) ** 0.5
    pack = ops.PackedConvValid(w)
    lin = ops.PackedConv(w.reshape(cout, cin * 25).contiguous())
    xn = x.permute(0, 3, 1, 2).contiguous()
    xcl = xn.contiguous(memory_format=torch.channels_last)
    wcl = w.contiguous(memory_format=torch.channels_last)

    def unfold_k9():
        cols = F.unfold(xn, 5).transpose(1, 2).reshape(N * 576, cin * 25).contiguous()
        return ops.linear_f16s(cols, lin)
    legs = {'k24': lambda: ops.conv_valid(x, pack), 'torch_fp32_conv2d_nchw': lambda: F.conv2d(xn, w),
            'torch_fp32_conv2d_channels_last': lambda: F.conv2d(xcl, wcl), 'unfold_plus_k9_linear': unfold_k9}
    extra = {}
    if fp16:
        pack16 = ops.PackedConvValid(w, split=False)
        legs = {'k24': legs['k24'], 'k24_f16': lambda: ops.conv_valid(x, pack16), **legs}
    with torch.no_grad():
        r = alternate(legs, rounds)
        if fp16:
            extra = {'max_abs_diff_vs_conv2d_f16': float((ops.conv_valid(x, pack16) - F.conv2d(xn, w).permute(0, 2, 3, 1)).abs().max())}
        dev = float((ops.conv_valid(x, pack) - F.conv2d(xn, w).permute(0, 2, 3, 1)).abs().max())
        dev_u = float((unfold_k9().reshape(N, 24, 24, cout) - F.conv2d(xn, w).permute(0, 2, 3, 1)).abs().max())
    floor = 3 * 2.0 * N * 576 * 25 * cin * cout / MFMA_RATE * 1e3
    return {'B': B, 'images': N, 'Cin': cin, 'Cout': cout, 'workgroups': N * 3 * (3 if N * 3 < 128 else 1), 'mfma_floor_ms': floor, 'max_abs_diff_vs_conv2d': dev,
            'max_abs_diff_of_unfold_route_vs_conv2d': dev_u, **extra, **stats(r)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--precision', choices=('fp32', 'fp16'), default='fp32',
                    help='fp16: the 16-bit-operand kernels / mode next to the default ones, in the same process')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vit8pt_extractor_time needs a GPU: nothing is timed without one')
    fp16 = a.precision == 'fp16'
    res = {'tool': 'vit8pt_extractor_time', 'device': torch.cuda.get_device_name(), 'rounds': a.rounds, 'precision': a.precision, 'conv5x5': [],
           'extractor': []}
    fmt = lambda d: f'{d["median_ms"]:9.4f} ms  ({d["min_ms"]:.4f} .. {d["max_ms"]:.4f})'
    for B in (1, 32):
        for cin in (128, 192):
            c = conv5_case(cin, B, a.rounds, fp16)
            res['conv5x5'].append(c)
            print(f'# 5x5 valid convolution {cin} -> 192, 28 x 28 -> 24 x 24, B = {B} ({c["images"]} images, {c["workgroups"]} workgroups), MFMA floor '
                  f'{c["mfma_floor_ms"]:.4f} ms; max |K24 - conv2d| {c["max_abs_diff_vs_conv2d"]:.2e}')
            for leg in (n for n in ('k24', 'k24_f16', 'torch_fp32_conv2d_nchw', 'torch_fp32_conv2d_channels_last', 'unfold_plus_k9_linear') if n in c):
                print(f'  {leg:34s} {fmt(c[leg])}' + (f'   x{c[leg]["median_ms"] / c["k24"]["median_ms"]:.2f} of K24' if leg != 'k24' else
                                                    f'   {c["mfma_floor_ms"] / c[leg]["median_ms"]:.1%} of the MFMA floor'))
            if fp16:
                print(f'  max |out - fp32 conv2d|: K24 {c["max_abs_diff_vs_conv2d"]:.2e}, plain fp16 {c["max_abs_diff_vs_conv2d_f16"]:.2e}')
    m, ref, inp = models()
    m16 = None
    if fp16:
        m16 = models()[0].set_precision('fp16')
    for B in (1, 32):
        c = extractor_case(m, ref, inp, B, a.rounds, m16)
        res['extractor'].append(c)
        print(f'# extractor B = {B} ({c["images"]} images of {SIZE[0]} x {SIZE[1]}); max |features - torch fp32| {c["max_abs_diff_of_the_features_vs_torch_fp32"]:.2e}')
        if fp16:
            print(f'  max |features - torch fp32| in mode fp16: {c["max_abs_diff_of_the_features_vs_torch_fp32_fp16"]:.2e} (max |features| {c["max_abs_features"]:.2f})')
        for leg in (n for n in ('extract_features', 'extract_features_fp16', 'k25_stem_rgb', 'k26_maxpool', 'k9_k17_layers', 'k24_conv2_192_192',
                                'k24_downsample_128_192', 'torch_fp32_extractor', 'forward_images', 'forward_images_fp16',
                                'torch_extractor_then_forward_features') if n in c):
            ratio = ''
            if leg == 'extract_features_fp16':
                ratio = f'   x{c[leg]["median_ms"] / c["extract_features"]["median_ms"]:.2f} of extract_features'
            if leg == 'forward_images_fp16':
                ratio = f'   x{c[leg]["median_ms"] / c["forward_images"]["median_ms"]:.2f} of forward(images)'
            if leg == 'torch_fp32_extractor':
                ratio = f'   x{c[leg]["median_ms"] / c["extract_features"]["median_ms"]:.2f} of extract_features'
            if leg == 'torch_extractor_then_forward_features':
                ratio = f'   x{c[leg]["median_ms"] / c["forward_images"]["median_ms"]:.2f} of forward(images)'
            print(f'  {leg:40s} {fmt(c[leg])}{ratio}')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
