"""The Map-free regressor (far_amd.mapfree.RegressionModel) timed in one process on one GPU (bench.py measures the LoFTR regressor and is
not touched), at B = 1 and B = 32 pairs of 360 x 270 images:

  * K27 (ops.stem_conv_rgb) next to fp32 torch conv2d + BatchNorm + ReLU; encode (both images of every pair), regress and forward
    with supplied solver outputs next to the fp32 torch restatement of the same layers on the same weights
    (tests/mapfree_reg_ref.py) -- nothing is compared with the code under test;
  * the four 3x3 decoder convolutions (upconv4 1024 -> 512 and iconv4 1024 -> 512 at 46 x 34, upconv3 512 -> 256 and iconv3 512 -> 256
    at 92 x 68), one launch each, next to their MFMA floors in the manner of tools/step_floors.py: 3 (split products) x 2 x pixels x
    9 Cin Cout flop at the 1.71 PFLOP/s far_mfma_probe_f16 sustains -- and next to torch's fp32 conv2d of the same layer;
  * the five ELU passes (K28) on their own: what the elementwise form costs over an epilogue form.

Timing as tools/vit8pt_time.py: HIP events around groups of launches, every leg warmed up, the legs ALTERNATED round by round, medians
over the rounds with the min .. max spread.  Prints a table and one JSON line.
Usage: python tools/mapfree_reg_time.py [--rounds N] [--batches 1,32]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from far_amd import ops
from tools.vit8pt_time import MFMA_RATE, alternate

SIZE = (360, 270)
KW = dict(use_loftr_preds=True, use_vanilla_transformer=True)
DECODER = (('upconv4', 1024, 512, (46, 34), False), ('iconv4', 1024, 512, (46, 34), True), ('upconv3', 512, 256, (92, 68), False),
           ('iconv3', 512, 256, (92, 68), True))


def models():
    from far_amd.mapfree import RegressionModel
    from tests import mapfree_reg_inputs as mi
    from tests import mapfree_reg_ref as rr
    ref = mi.seeded_fill(rr.RefRegressionModel())
    m = RegressionModel(mi.config(), **KW)
    m.load_state_dict(ref.state_dict(), strict=True)
    return m.cuda(), ref.cuda()


def stats(r):
    return {name: {'median_ms': m, 'min_ms': lo, 'max_ms': hi} for name, (m, lo, hi) in r.items()}


def model_case(m, ref, B, rounds):
    from tests import mapfree_reg_inputs as mi
    im0, im1 = (t.cuda() for t in mi.seeded_images(batch=B))
    rt, inl = (t.cuda() for t in mi.seeded_solver_outputs(B))
    both = torch.cat([im0, im1]).contiguous()
    enc = ref.encoder
    with torch.no_grad():
        vols = m.encode(both)                                                      # builds the packs
        v0, v1 = vols[:B].contiguous(), vols[B:].contiguous()
        R, t = m.regress(v0, v1, rt, inl)
        R32, t32 = ref.regress(ref.encode(im0), ref.encode(im1), rt, inl)
        stem = m._pack_cache._store['firstconv'][1]
    data = lambda: {'image0_reg': im0, 'image1_reg': im1, 'loftr_rt': rt, 'inliers': inl}

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    legs = {'k27_stem': lambda: ops.stem_conv_rgb(both, stem),
            'torch_fp32_stem': lambda: F.relu(enc.firstbn(enc.firstconv(both))),
            'encode': lambda: m.encode(both),
            'torch_fp32_encode': lambda: ref.encode(both),
            'regress': lambda: m.regress(v0, v1, rt, inl),
            'torch_fp32_regress': lambda: ref.regress(v0, v1, rt, inl),
            'forward': lambda: m(data()),
            'torch_fp32_forward': lambda: ref(data())}
    r = alternate({k: nograd(v) for k, v in legs.items()}, rounds, target_ms=40.0)
    dev = {'max_abs_diff_R_vs_torch_fp32': float((R - R32).abs().max()), 'max_abs_diff_t_vs_torch_fp32': float((t - t32).abs().max())}
    return {'B': B, 'images': 2 * B, 'image_size': list(SIZE), **dev, **stats(r)}


def decoder_case(m, ref, B, rounds):
    """One launch of each 3x3 decoder convolution (the model's own weight images, bias + BatchNorm folded, no ELU) and the ELU pass
    behind it, next to torch's fp32 conv2d (channels_last) of the same layer and the layer's MFMA floor."""
    N = 2 * B
    out = []
    enc = ref.encoder
    mods = {'upconv4': enc.upconv4.conv1, 'iconv4': enc.iconv4, 'upconv3': enc.upconv3.conv1, 'iconv3': enc.iconv3}
    g = torch.Generator(device='cuda').manual_seed(B)
    for name, cin, cout, (h, w), cat in DECODER:
        pc = m._pack_cache._store[name][1]
        x = torch.randn(N, h, w, cin // 2 if cat else cin, device='cuda', generator=g)
        x2 = torch.randn(N, h, w, cin // 2, device='cuda', generator=g) if cat else None
        full = x if x2 is None else torch.cat([x, x2], -1)
        xcl = full.permute(0, 3, 1, 2)                                           # NCHW logical, channels_last memory
        conv = mods[name].conv
        wcl = conv.weight.detach().contiguous(memory_format=torch.channels_last)
        y = ops.conv_nhwc(x, pc, x2=x2)
        legs = {'conv': lambda: ops.conv_nhwc(x, pc, x2=x2), 'elu': lambda: ops.elu(y),
                'torch_fp32_conv2d': lambda: F.conv2d(xcl, wcl, conv.bias, 1, 1)}
        with torch.no_grad():
            r = alternate(legs, rounds)
        floor = 3 * 2.0 * N * h * w * 9 * cin * cout / MFMA_RATE * 1e3
        kernel = 'K9' if (cat or not ops.USE_WINO or h * w < ops.WINO_MIN_PIXELS) else 'K17'
        out.append({'layer': name, 'kernel': kernel, 'B': B, 'images': N, 'Cin': cin, 'Cout': cout, 'grid': [h, w], 'mfma_floor_ms': floor,
                    'gflop': 2.0 * N * h * w * 9 * cin * cout / 1e9, **stats(r)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--batches', default='1,32')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mapfree_reg_time needs a GPU: nothing is timed without one')
    res = {'tool': 'mapfree_reg_time', 'device': torch.cuda.get_device_name(), 'rounds': a.rounds, 'model': [], 'decoder': []}
    fmt = lambda d: f'{d["median_ms"]:9.4f} ms  ({d["min_ms"]:.4f} .. {d["max_ms"]:.4f})'
    m, ref = models()
    for B in (int(b) for b in a.batches.split(',')):
        c = model_case(m, ref, B, a.rounds)
        res['model'].append(c)
        print(f'# Map-free regressor B = {B} ({c["images"]} images of {SIZE[0]} x {SIZE[1]}); max |R - torch fp32| {c["max_abs_diff_R_vs_torch_fp32"]:.2e}, '
              f'max |t - torch fp32| {c["max_abs_diff_t_vs_torch_fp32"]:.2e}')
        for leg, other in (('k27_stem', 'torch_fp32_stem'), ('encode', 'torch_fp32_encode'), ('regress', 'torch_fp32_regress'),
                           ('forward', 'torch_fp32_forward')):
            ratio = c[other]['median_ms'] / c[leg]['median_ms']
            print(f'  {leg:22s} {fmt(c[leg])}')
            print(f'  {other:22s} {fmt(c[other])}   x{ratio:.2f} of {leg}' + ('   SLOWER THAN TORCH' if ratio < 1 else ''))
        d = decoder_case(m, ref, B, a.rounds)
        res['decoder'] += d
        print(f'# decoder 3x3 convolutions, one launch each, B = {B} ({2 * B} images)')
        for e in d:
            print(f'  {e["layer"]:8s} {e["kernel"]:3s} {e["Cin"]:4d} -> {e["Cout"]:3d} at {e["grid"][0]} x {e["grid"][1]}: {fmt(e["conv"])}   MFMA floor '
                  f'{e["mfma_floor_ms"]:.4f} ms ({e["mfma_floor_ms"] / e["conv"]["median_ms"]:.1%})   torch fp32 conv2d {fmt(e["torch_fp32_conv2d"])} '
                  f'(x{e["torch_fp32_conv2d"]["median_ms"] / e["conv"]["median_ms"]:.2f})   ELU pass {fmt(e["elu"])}')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
