"""Container-only: golden G28 -- the Map-free regressor, produced by the reference's own classes:

    mapfree_6dreg/lib/models/regression/model.py: RegressionModel.__init__ (:36-165), regression_mlp (:198-233), forward (:235-308);
    encoder/resunet.py: ResUNet; aggregator.py: CorrelationVolumeWarping; head.py: DirectDeepResBlockMLP -- all unmodified, in FAR's
    configuration (config/regression/mapfree/rot6d_trans_with_loftr.yaml, --use_loftr_preds --use_vanilla_transformer, with and
    without --use_prior; tests/mapfree_reg_inputs.py: config)

pytorch_lightning, yacs, kornia, cv2 and the two matcher submodules are absent; stubs stand in, as tools/ref_shim.py and
tools/make_golden_vit8pt_extractor.py stub theirs: pl.LightningModule = nn.Module, a parameter-free stand-in for LoFTR (and its
checkpoint load), Tensor.cuda as the identity, and match_no_load / estimate_pose replaced by functions that return the seeded
loftr_rt / inliers of tests/mapfree_reg_inputs.py.  Weights, running statistics, images and the solver's outputs come from the seeded
CPU generators there; the fixture holds outputs only: strided taps of the encoder volumes and of x3, R and t for use_prior False and
True, and the reference's state-dict names and shapes.

The fill's conditions (tests/mapfree_reg_inputs.py) are asserted here on the reference's own CPU run and printed.
Usage: python tools/make_golden_mapfree_reg.py"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference/mapfree_6dreg'


class _AnyName(types.ModuleType):
    """A stub module: a name nobody defined imports as None (it is imported by the reference, never called on this path)."""

    def __getattr__(self, k):
        if k.startswith('__'):
            raise AttributeError(k)
        return None


def _mk(name, **attrs):
    m = _AnyName(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _StandInLoFTR(nn.Module):
    """Parameter-free stand-in for upstream LoFTR: the regressor's state dict then holds no matcher.* entry of ours."""

    def __init__(self, config=None):
        super().__init__()

    def load_state_dict(self, *a, **k):
        return None


def install_stubs():
    pl = _mk('pytorch_lightning', LightningModule=nn.Module)
    _mk('pytorch_lightning.utilities', rank_zero_only=lambda fn: fn)
    del pl

    class CfgNode(dict):
        pass
    _mk('yacs')
    _mk('yacs.config', CfgNode=CfgNode)
    _mk('cv2')
    _mk('kornia')
    _mk('kornia.geometry')
    _mk('kornia.geometry.conversions', quaternion_to_rotation_matrix=None)
    for name in ('etc', 'etc.feature_matching_baselines', 'etc.feature_matching_baselines.LoFTR', 'etc.feature_matching_baselines.LoFTR.src',
                 'etc.feature_matching_baselines.SuperGlue', 'etc.feature_matching_baselines.SuperGlue.models'):
        _mk(name)
    _mk('etc.feature_matching_baselines.LoFTR.src.loftr', LoFTR=_StandInLoFTR, default_cfg={})
    _mk('etc.feature_matching_baselines.SuperGlue.models.matching', Matching=None)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.load = lambda *a, **k: {'state_dict': {}}               # model.py:105 reads the matcher's checkpoint (the stand-in ignores it)
    sys.path.insert(0, REF)


def reference_model(use_prior, rt, inl):
    """The reference's RegressionModel on the seeded fill, its matcher + solver replaced by the seeded outputs."""
    from tests import mapfree_reg_inputs as mi
    from lib.models.regression.model import RegressionModel
    m = RegressionModel(mi.config(), use_loftr_preds=True, use_vanilla_transformer=True, use_prior=use_prior, inference=True).eval()
    mi.seeded_fill(m)
    state = {'i': 0}

    def match_no_load(inp0, inp1):
        return np.zeros((8, 2)), np.zeros((8, 2))

    def estimate_pose(k0, k1, data, prior=None):
        i = state['i'] % rt.shape[0]
        state['i'] += 1
        R, t = rt[i, :, :3].double().numpy(), rt[i, :, 3].double().numpy()
        n = [int(v) for v in inl[i]]
        return (R, t, n[0]), (n[1] if use_prior else 0), (n[2] if use_prior else 0)
    m.match_no_load = match_no_load
    m.pose_solver.estimate_pose = estimate_pose
    return m


def main():
    install_stubs()
    from tests import mapfree_reg_inputs as mi
    from tests import mapfree_reg_ref as rr
    im0, im1 = mi.seeded_images()
    store, manifest = {}, None
    for use_prior in (False, True):
        tag = 'prior' if use_prior else 'noprior'
        rt, inl = mi.seeded_solver_outputs(prior=use_prior)
        ref = reference_model(use_prior, rt, inl)
        if manifest is None:
            manifest = {k: list(v.shape) for k, v in ref.state_dict().items()}
        data = {'image0': torch.zeros(mi.B, 1, 8, 8), 'image1': torch.zeros(mi.B, 1, 8, 8), 'K_color0': torch.eye(3).expand(mi.B, 3, 3),
                'K_color1': torch.eye(3).expand(mi.B, 3, 3), 'image0_reg': im0.clone(), 'image1_reg': im1.clone()}
        with torch.no_grad():
            R, t = ref(data)
            vol0, vol1 = ref.encoder(im0), ref.encoder(im1)
            agg = ref.aggregator(vol0, vol1)
            _, _, x3 = ref.head(agg, data)
        assert torch.equal(data['image0_reg'], im0) and torch.equal(data['loftr_rt'], rt) and torch.equal(data['inliers'].float(), inl)
        R, t = R.detach(), t.detach()                                  # model.py:278 re-enables gradients for the last loop
        store[f'R_{tag}'], store[f't_{tag}'] = R.numpy(), t.numpy()
        if not use_prior:
            store['vol'] = mi.tap_volume(torch.cat([vol0, vol1])).contiguous().numpy()
            store['x3'] = mi.tap_x3(x3).contiguous().numpy()
        # the conditions of the fill, on the reference's weights through the restatement (float64: also the reference's own fp32 error)
        r64 = rr.RefRegressionModel(use_prior)
        r64.load_state_dict({k: v for k, v in ref.state_dict().items() if not k.startswith('matcher.')}, strict=True)
        r64 = r64.double()
        taps, out, bad = [], {}, []
        with torch.no_grad():
            v0 = r64.encode(im0.double(), taps)
            v1 = r64.encode(im1.double())
            agg64 = rr.corr_volume_warp(v0, v1)
            r64.head(agg64, taps)
            R64, t64 = r64.regress(v0, v1, rt, inl, out)
        for i, (share, amax) in enumerate(taps):
            print(f'{tag} activation {i:2d}: positive share {share:.3f}  max |.| {amax:.1f}')
            bad += [(tag, i, share, amax)] if not (mi.RELU_SHARE[0] <= share <= mi.RELU_SHARE[1] and amax < mi.ACT_MAX) else []
        assert not bad, bad
        for nm in ('agg', 'x3', 'transformer'):
            assert float(out[nm].abs().max()) < mi.ACT_MAX
            print(f'{tag} {nm}: max |.| {float(out[nm].abs().max()):.2f}')
        med = float(out['agg'][:, -1].median())
        print(f'{tag} K12 max-score channel: median {med:.3f}')
        assert mi.MAX_SCORE[0] <= med <= mi.MAX_SCORE[1]
        print(f'{tag} gate weights: {out["gate"].tolist()}')
        assert bool(((out['gate'] > mi.GATE[0]) & (out['gate'] < mi.GATE[1])).all())
        ratio = out['ratio']
        inside = (ratio > mi.CLAMP[0]) & (ratio < mi.CLAMP[1])
        print(f'{tag} translation-norm ratio: {ratio.tolist()}')
        assert bool(inside.any()) and bool((~inside).any())
        for nm, a, b in (('vol0', vol0, v0), ('x3', x3, out['x3']), ('R', R, R64), ('t', t, t64)):
            print(f'{tag} {nm}: reference fp32 vs float64 restatement {float((a.double() - b).abs().max()):.3e}  (max |.| {float(b.abs().max()):.3f})')
    path = os.path.join(OUT, 'g28_mapfree_regressor.npz')
    np.savez_compressed(path, seed=mi.SEED, manifest=json.dumps(manifest), **store,
                        note='reference: mapfree_6dreg RegressionModel (rot6d_trans_with_loftr.yaml, use_loftr_preds, use_vanilla_transformer), '
                             f'B = {mi.B}, {mi.SIZE[0]} x {mi.SIZE[1]}; vol: cat[vol0, vol1] every {mi.TAP_VOL[0]}th row / {mi.TAP_VOL[1]}th column; '
                             f'x3: every {mi.TAP_X3_CH}th channel')
    print(f'g28_mapfree_regressor: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
