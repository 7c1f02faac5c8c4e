"""Container-only: golden G25 -- the 8-Point-ViT regressor behind its extractor, produced by the reference's own model:

    interiornetStreetlearn_8ptVit/src/model.py: ViTEss (forward :165-217 with extract_features replaced by the seeded features),
    args of eval_interiornet_t.sh / eval_streetlearn_t.sh (tests/vit8pt_inputs.py: vit_args)

The reference imports torchvision for its extractor only; a stub module stands in (resnet18() -> an empty module with an `fc`
attribute), and Tensor.cuda is the identity as in tools/make_golden_vit.py.  Weights and inputs come from the seeded CPU generator of
tests/vit8pt_inputs.py; the fixture holds outputs, the state dict's names and shapes, and no weights.
Usage: python tools/make_golden_vit8pt.py"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference/interiornetStreetlearn_8ptVit'


class _NoResNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Identity()


def reference_model():
    from tests import vit8pt_inputs as vi
    torch.Tensor.cuda = lambda self, *a, **k: self            # positional table (:192) and tools.py:23
    tv, tvm = types.ModuleType('torchvision'), types.ModuleType('torchvision.models')
    tvm.resnet18 = lambda *a, **k: _NoResNet()
    tv.models = tvm
    sys.modules.setdefault('torchvision', tv)
    sys.modules.setdefault('torchvision.models', tvm)
    sys.path.insert(0, REF)
    from src.model import ViTEss
    return ViTEss(vi.vit_args()).eval()


def main():
    from tests import vit8pt_inputs as vi
    from tests import vit8pt_ref as vr
    ref = reference_model()
    g = vi.seeded_fill(ref)
    inp = vi.seeded_inputs(g)
    ref.global_pose_mean, ref.global_pose_std = inp['pose_mean'], inp['pose_std']
    feats = inp['features']
    ref.extract_features = lambda images, intrinsics=None: (feats, intrinsics)
    taps = {}
    for i in vi.TAP_BLOCKS:
        ref.fusion_transformer.blocks[i].register_forward_hook(lambda mod, a, out, i=i: taps.__setitem__(i, out.detach().clone()))
    norm_out = {}
    ref.fusion_transformer.norm.register_forward_hook(lambda mod, a, out: norm_out.__setitem__('f', out.detach().clone()))
    images = torch.zeros(vi.B, 2, 3, 8, 8)                     # only its batch size is read (model.py:169)
    with torch.no_grad():
        tran, rot, mtx, r6 = ref(images, intrinsics=inp['intrinsics'].clone(), loftr_num_corr=inp['loftr_num_corr'],
                                 loftr_preds=inp['loftr_preds'])
    sd = {k: v for k, v in ref.state_dict().items() if not k.startswith(vi.SKIP)}
    names = sorted(sd)
    # the restatement in float64 on the same weights: the conditions the fill promises, and the reference's own fp32 deviation
    r64 = vr.RefViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'])
    r64.load_state_dict(sd, strict=True)
    r64 = r64.as_dtype(torch.float64)
    cond = vr.fill_conditions(r64, feats, vi.VIT_INTRINSICS)
    for i, c in enumerate(cond['blocks']):
        print(f'block {i}: ' + '  '.join(f'{k} {v:.3f}' for k, v in c.items()))
    print(f'CrossBlock output max {cond["cross_absmax"]:.1f}')
    out64 = r64.forward_features(feats, vi.VIT_INTRINSICS, inp['loftr_num_corr'], inp['loftr_preds'])
    for nm, a, b in zip(('tran', 'rot', 'mtx', 'rot6d'), (tran, rot, mtx, r6), out64):
        print(f'{nm}: reference fp32 vs float64 restatement {float((a.double() - b).abs().max()):.3e}  (max |.| {float(b.abs().max()):.3f})')
    tap = lambda t: t[list(vi.TAP_ROWS), ::vi.TAP_STRIDE].numpy()
    path = os.path.join(OUT, 'g25_vit8pt.npz')
    np.savez_compressed(path, seed=vi.SEED, tran_preds_unnorm=tran.numpy(), rot_preds=rot.numpy(), rot_preds_mtx=mtx.numpy(),
                        rot_preds_6d=r6.numpy(), features=norm_out['f'].numpy(),
                        **{f'block{i}_out': tap(taps[i]) for i in vi.TAP_BLOCKS},
                        sd_names=np.array(names), sd_shapes=np.array([','.join(map(str, sd[k].shape)) for k in names]),
                        note='reference: interiornetStreetlearn_8ptVit src/model.py ViTEss, B = 2, depth 6, gating + normalized 6d; '
                             f'block taps: images {vi.TAP_ROWS}, every {vi.TAP_STRIDE}th token')
    print(f'g25_vit8pt: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
