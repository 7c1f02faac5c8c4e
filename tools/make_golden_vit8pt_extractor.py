"""Container-only: golden G26 -- the 8-Point-ViT from images, produced by the reference's own model:

    interiornetStreetlearn_8ptVit/src/model.py: ViTEss.__init__ (:56-60), extract_features (:131-163), forward (:165-217) and
    src/modules/extractor.py: ResidualBlock, all unmodified; args of eval_interiornet_t.sh / eval_streetlearn_t.sh
    (tests/vit8pt_inputs.py: vit_args)

torchvision is absent; a stub module stands in whose models.resnet18() returns this project's own torch.nn restatement of the front
(tests/vit8pt_extractor_ref.py: ResNet18Front), and Tensor.cuda is the identity as in tools/make_golden_vit8pt.py.  Weights and images
come from the seeded CPU generators of tests/vit8pt_inputs.py (trunk, head) and tests/vit8pt_extractor_inputs.py (extractor, images);
the fixture holds outputs only: strided taps of the extractor's (2B, 576, 192) output and the four outputs of forward, per image size.
Usage: python tools/make_golden_vit8pt_extractor.py"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference/interiornetStreetlearn_8ptVit'


def reference_model():
    from tests import vit8pt_extractor_ref as er
    from tests import vit8pt_inputs as vi
    torch.Tensor.cuda = lambda self, *a, **k: self            # positional table and tools.py:23
    tv, tvm = types.ModuleType('torchvision'), types.ModuleType('torchvision.models')
    tvm.resnet18 = er.resnet18
    tv.models = tvm
    sys.modules['torchvision'] = tv
    sys.modules['torchvision.models'] = tvm
    sys.path.insert(0, REF)
    from src.model import ViTEss
    return ViTEss(vi.vit_args()).eval()


def main():
    from tests import vit8pt_extractor_inputs as ei
    from tests import vit8pt_extractor_ref as er
    from tests import vit8pt_inputs as vi
    from tests import vit8pt_ref as vr
    from far_amd.vit8pt import update_intrinsics
    ref = reference_model()
    inp = ei.filled(ref)
    ref.global_pose_mean, ref.global_pose_std = inp['pose_mean'], inp['pose_std']
    # the restatement in float64 on the same weights: the conditions the fill promises, and the reference's own fp32 deviation
    r64 = er.RefViTEssImages(vi.vit_args(), inp['pose_mean'], inp['pose_std'])
    r64.load_state_dict(ref.state_dict(), strict=True)
    r64 = r64.as_dtype(torch.float64)
    store = {}
    for (h, w), images in zip(ei.SIZES, inp['images']):
        tag = f'{h}x{w}'
        intr = ei.image_intrinsics(images.shape)
        keep = images.clone()
        with torch.no_grad():
            feats, _ = ref.extract_features(images, None)
            out = ref(images, intrinsics=intr.clone(), loftr_num_corr=inp['loftr_num_corr'], loftr_preds=inp['loftr_preds'])
        assert torch.equal(images, keep)
        taps = []
        f64 = r64.extract_features(images, taps)
        for i, (share, amax) in enumerate(taps):
            print(f'{tag} ReLU {i:2d}: positive share {share:.3f}  max |.| {amax:.1f}')
        print(f'{tag} features: reference fp32 vs float64 restatement {float((feats.double() - f64).abs().max()):.3e}  (max |.| {float(f64.abs().max()):.3f})')
        grid = tuple(float(v) for v in update_intrinsics(images.shape, intr)[0, 0])
        cond = vr.fill_conditions(r64, f64, grid)
        for i, c in enumerate(cond['blocks']):
            print(f'{tag} block {i}: ' + '  '.join(f'{k} {v:.3f}' for k, v in c.items()))
        print(f'{tag} CrossBlock output max {cond["cross_absmax"]:.1f}')
        out64 = r64.forward_features(f64, grid, inp['loftr_num_corr'], inp['loftr_preds'])
        for nm, a, b in zip(ei.OUTPUTS, out, out64):
            print(f'{tag} {nm}: reference fp32 vs float64 restatement {float((a.double() - b).abs().max()):.3e}  (max |.| {float(b.abs().max()):.3f})')
            store[f'{nm}_{tag}'] = a.numpy()
        store[f'features_{tag}'] = ei.tap(feats).contiguous().numpy()
    path = os.path.join(OUT, 'g26_vit8pt_extractor.npz')
    np.savez_compressed(path, seed=ei.SEED, **store,
                        note='reference: interiornetStreetlearn_8ptVit src/model.py ViTEss from images, B = 2, depth 6, gating + normalized 6d; '
                             f'features: every {ei.TAP_TOKENS}th token, every {ei.TAP_CHANNELS}th channel')
    print(f'g26_vit8pt_extractor: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
