"""The 8-Point-ViT regressor (far_amd.vit8pt) on the CPU: the float64 / fp32 restatement of tests/vit8pt_ref.py pinned to the
reference's own fp32 run (golden G25, tools/make_golden_vit8pt.py), state-dict compatibility, the pair-order conversion, the pure
helpers, the refusals and the C ABI of K23.  Nothing here launches a kernel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import vit8pt_inputs as vi
from tests import vit8pt_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g25_vit8pt.npz')
OUTPUTS = ('tran_preds_unnorm', 'rot_preds', 'rot_preds_mtx', 'rot_preds_6d')


def golden():
    return np.load(GOLDEN)


_CACHE = {}


def restated():
    """The seeded RefViTEss (fp32) and its inputs, and what the fp32 and float64 restatements compute: built once per process."""
    if not _CACHE:
        inp_model = vr.RefViTEss(vi.vit_args())
        gen = vi.seeded_fill(inp_model)
        inp = vi.seeded_inputs(gen)
        inp_model.pose_mean, inp_model.pose_std = inp['pose_mean'], inp['pose_std']
        res = {}
        for dt in (torch.float32, torch.float64):
            m = inp_model.as_dtype(dt)
            taps = []
            with torch.no_grad():
                feats = m.trunk(inp['features'], vi.VIT_INTRINSICS, taps)
            out = m.forward_features(inp['features'], vi.VIT_INTRINSICS, inp['loftr_num_corr'], inp['loftr_preds'])
            res[dt] = dict(zip(OUTPUTS, out), features=feats,
                           **{f'block{i}_out': taps[i][list(vi.TAP_ROWS), ::vi.TAP_STRIDE] for i in vi.TAP_BLOCKS})
        _CACHE.update(model=inp_model, inp=inp, res=res)
    return _CACHE


def test_restatement_is_pinned_to_the_reference_run():
    """Per stored tensor: dev = max|reference fp32 - float64 restatement| is the reference's own fp32 deviation; the fp32 restatement
    stays within 4 x dev of the reference's stored output (the triangle rule of tests/test_full_attention_gpu.py), and dev itself is
    within the project's bar for regression outputs, 1e-3 max|reference|."""
    g = golden()
    assert int(g['seed']) == vi.SEED
    r = restated()['res']
    for key in OUTPUTS + ('features',) + tuple(f'block{i}_out' for i in vi.TAP_BLOCKS):
        want = torch.from_numpy(g[key])
        r64, r32 = r[torch.float64][key], r[torch.float32][key]
        assert tuple(want.shape) == tuple(r64.shape), key
        dev = float((want.double() - r64).abs().max())
        d32 = float((r32.double() - want.double()).abs().max())
        print(f'[golden pin] {key}: reference-vs-float64 {dev:.3e}  fp32 restatement-vs-reference {d32:.3e}  max|ref| {float(want.abs().max()):.3f}')
        assert dev <= 1e-3 * float(want.abs().max()), key
        assert d32 <= 4.0 * dev, key


def test_fill_conditions():
    """The regime tests/vit8pt_inputs.py promises: a peaked softmax with rescaling rows, everything inside the default range."""
    c = restated()
    cond = vr.fill_conditions(c['model'].as_dtype(torch.float64), c['inp']['features'], vi.VIT_INTRINSICS)
    assert len(cond['blocks']) == vi.DEPTH - 1
    for b in cond['blocks']:
        assert -60 < b['score_min'] < -45 and 45 < b['score_max'] < 60, b
        assert 0.77 <= round(b['pmax_median'], 2) <= 0.81, b
        assert 0.12 < b['pmax_min'] < 0.2, b
        assert b['qkv_absmax'] <= 16.5 and b['out_absmax'] <= 30, b
    assert cond['cross_absmax'] <= 3.5


def test_state_dict_names_and_shapes_match_the_reference():
    from far_amd.vit8pt import ViTEss
    g = golden()
    want = dict(zip((str(s) for s in g['sd_names']), (tuple(int(x) for x in str(s).split(',')) for s in g['sd_shapes'])))
    m = ViTEss(vi.vit_args())
    have = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert have == want
    # ... and the restatement module of the tests carries the same names: its state dict loads strictly
    ref = restated()['model']
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == want
    m.load_state_dict(ref.state_dict(), strict=True)
    assert 'fusion_transformer.blocks.0.attn.qkv.weight' in want and 'fusion_transformer.blocks.5.cross_attn.proj_fundamental.bias' in want
    assert want['moe_predictor.0.weight'] == (512, 26880 + 19) and want['pose_regressor.0.weight'] == (512, 26880)
    # without the gate there is no moe_predictor (model.py:93-116)
    assert not any(k.startswith('moe_predictor') for k in ViTEss(vi.vit_args(use_loftr_gating=False)).state_dict())


def test_pair_order_conversion_at_batch_two():
    from far_amd.vit8pt import concatenated_to_interleaved, interleaved_to_concatenated
    x = torch.arange(4.)[:, None, None] + torch.zeros(4, 3, 2)               # row r holds the value r: pair b = rows 2b, 2b + 1
    c = interleaved_to_concatenated(x)
    assert c[:, 0, 0].tolist() == [0., 2., 1., 3.]                            # img0 of pairs 0, 1, then img1 of pairs 0, 1
    assert torch.equal(concatenated_to_interleaved(c), x)
    y = torch.randn(6, 5, 7)
    assert torch.equal(interleaved_to_concatenated(y), torch.cat([y[0::2], y[1::2]], 0))
    assert torch.equal(concatenated_to_interleaved(interleaved_to_concatenated(y)), y)


def test_update_intrinsics_is_pure():
    from far_amd.vit8pt import ViTEss, update_intrinsics
    k = torch.tensor([[[400., 410., 320., 240.]] * 2, [[380., 390., 300., 250.]] * 2])
    before = k.clone()
    out = update_intrinsics((2, 2, 3, 480, 640), k)
    assert torch.equal(k, before) and out.data_ptr() != k.data_ptr()
    want = before.clone()
    want[:, :, [0, 2]] *= 24 / 640                                            # model.py:122-127
    want[:, :, [1, 3]] *= 24 / 480
    torch.testing.assert_close(out, want, rtol=1e-6, atol=0)
    assert torch.equal(ViTEss.update_intrinsics((480, 640), k), out)


def test_rotation_and_gate_helpers():
    from far_amd.vit8pt import loftr_gate_inputs, pose_from_rotation_matrix, rotation_matrix_from_ortho6d
    o6 = torch.randn(5, 6, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    o6[4] = 0                                                                 # the 1e-8 floor: finite, no division by zero
    m = rotation_matrix_from_ortho6d(o6)
    assert torch.isfinite(m).all() and torch.equal(m, vr.rotation_from_6d(o6))
    eye = torch.eye(3, dtype=torch.float64)
    assert float((m[:4].transpose(1, 2) @ m[:4] - eye).abs().max()) < 1e-12
    assert torch.equal(pose_from_rotation_matrix(torch.eye(3), m), m.transpose(1, 2))      # rest pose e_j -> column j
    rt = torch.arange(24.).reshape(2, 3, 4)
    preds, n = loftr_gate_inputs({'loftr_rt': rt, 'num_correspondences_after_ransac': torch.tensor([7, 9])})
    assert preds.shape == (2, 4, 4) and torch.equal(preds[:, :3], rt) and preds[:, 3].tolist() == [[0., 0., 0., 1.]] * 2
    assert n.dtype == torch.float32 and n.tolist() == [7., 9.]
    preds, n = loftr_gate_inputs({'loftr_rt': rt[0], 'num_correspondences_after_ransac': 0})   # one pair, the (3, 4) form
    assert preds.shape == (1, 4, 4) and n.tolist() == [0.]


def test_refusals():
    from far_amd import vit8pt
    m = vit8pt.ViTEss(vi.vit_args())
    with pytest.raises(NotImplementedError, match='forward_features'):
        m(torch.zeros(1, 2, 3, 8, 8))
    with pytest.raises(NotImplementedError, match='pooled-conv'):
        vit8pt.ViTEss(vi.vit_args(fusion_transformer=False))
    for make in (lambda: vit8pt.Block(192, 3, drop=0.1), lambda: vit8pt.Block(192, 3, drop_path=0.1),
                 lambda: vit8pt.Attention(192, 3, attn_drop=0.1), lambda: vit8pt.FusionTransformer(drop_rate=0.1)):
        with pytest.raises(NotImplementedError, match='drop'):
            make()
    with pytest.raises(NotImplementedError, match='64'):
        vit8pt.Attention(192, 6)
    feats = torch.zeros(4, 576, 192)
    k = torch.tensor(vi.VIT_INTRINSICS).expand(2, 2, 4).clone()
    other = k.clone()
    other[1] *= 1.5                                                           # pair 1 has another camera
    with pytest.raises(NotImplementedError, match='per-sample intrinsics'):
        m.forward_features(feats, other)
    frames = k.clone()
    frames[0, 1, 0] += 1.0                                                    # the two frames of pair 0 differ
    with pytest.raises(ValueError, match='frames'):
        m.forward_features(feats, frames)
    with pytest.raises(ValueError):
        m.forward_features(torch.zeros(3, 576, 192))
    from far_amd import _lib
    with pytest.raises(_lib.FarHipError):                                     # CPU tensors: no eager fallback
        with torch.no_grad():
            m.forward_features(feats, k)


def test_abi_of_k23():
    from far_amd import _lib, ops
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'far_hip.h')).read()
    name = 'far_vit_attention_f16s'
    assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in far_hip.h'
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    c_p, c_i, c_l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib.SIGNATURES[name] == (c_i, [c_p] * 3 + [c_i] * 5 + [c_l] * 6 + [c_i] + [c_p] * 3)
    assert lib.far_abi_version() == _lib.EXPECTED_ABI == 8                    # a pure addition
    assert callable(ops.vit_attention) and callable(ops.vit_attention_planes)
    # K22's entry point keeps its own list of head dims
    assert lib.far_full_attention_workspace_bytes(1, 40, 40, 3, 64) == 0
    x = torch.zeros(1, 4, 192)
    for fn in (lambda: ops.vit_attention(x, x, x, 3), lambda: ops.vit_attention_planes(torch.zeros(9, 1, 4, 64), 3)):
        with pytest.raises(_lib.FarHipError):                                 # CPU tensors
            fn()
