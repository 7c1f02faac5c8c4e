"""far_amd.vit8pt on the GPU: one Block, the trunk and forward_features on the seeded fill of tests/vit8pt_inputs.py, against the
float64 restatement (tests/vit8pt_ref.py, pinned to the reference's run by tests/test_vit8pt_cpu.py) and against golden G25.

Bars: Block outputs and the final features under the project's parity rule (tests/test_full_attention_gpu.py: _bar), at most
max(3 x dev32, 2^-20 max|out|) from float64 with dev32 the fp32 restatement's own deviation on the same GPU in the same run; the four
regression outputs at the project's bar for regression outputs, 1e-3 max|reference| (the form of tests/test_vit_shape_gpu.py)."""
import os

import numpy as np
import pytest
import torch

from tests import vit8pt_inputs as vi
from tests import vit8pt_ref as vr
from tests.test_full_attention_gpu import _bar

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g25_vit8pt.npz')
OUTPUTS = ('tran_preds_unnorm', 'rot_preds', 'rot_preds_mtx', 'rot_preds_6d')
_CACHE = {}


def setup(batch=vi.B, **over):
    """-> (far_amd ViTEss on the GPU, the seeded RefViTEss (fp32, CPU), inputs on the GPU); the default configuration is built once."""
    key = (batch, tuple(sorted(over.items())))
    if key not in _CACHE:
        from far_amd.vit8pt import ViTEss
        ref = vr.RefViTEss(vi.vit_args(**over))
        inp = vi.seeded_inputs(vi.seeded_fill(ref), batch)
        ref.pose_mean, ref.pose_std = inp['pose_mean'], inp['pose_std']
        m = ViTEss(vi.vit_args(**over), inp['pose_mean'], inp['pose_std'])
        m.load_state_dict(ref.state_dict(), strict=True)
        _CACHE[key] = (m.eval().cuda(), ref, {k: v.cuda() for k, v in inp.items()})
    return _CACHE[key]


def test_block_and_trunk_against_float64():
    m, ref, inp = setup()
    got = []
    with torch.no_grad():
        feats = m.trunk(inp['features'], inp['intrinsics'], got)
    r64, r32 = ref.as_dtype(torch.float64, 'cuda'), ref.as_dtype(torch.float32, 'cuda')
    t64, t32 = [], []
    with torch.no_grad():
        f64 = r64.trunk(inp['features'], vi.VIT_INTRINSICS, t64)
        f32 = r32.trunk(inp['features'], vi.VIT_INTRINSICS, t32)
    assert len(got) == vi.DEPTH
    for i in range(vi.DEPTH):
        what = f'Block {i}' if i < vi.DEPTH - 1 else 'CrossBlock'
        _bar(f'vit8pt {what} output', got[i], t64[i], float((t32[i].double() - t64[i]).abs().max()))
    _bar('vit8pt final features', feats, f64, float((f32.double() - f64).abs().max()))
    # one Block on its own, from the float64 input of Block 2 (its own input rounded to fp32): the per-layer figure
    x = t64[1].float()
    with torch.no_grad():
        y = m.fusion_transformer.blocks[2](x)
        y64 = r64.fusion_transformer.blocks[2](x.double())
        y32 = r32.fusion_transformer.blocks[2](x)
    _bar('vit8pt Block 2 alone', y, y64, float((y32.double() - y64).abs().max()))
    # the stored Block taps of the reference's run, at the triangle rule's 4 x dev32
    g = np.load(GOLDEN)
    for i in vi.TAP_BLOCKS:
        want = torch.from_numpy(g[f'block{i}_out']).cuda()
        rows = lambda t: t[list(vi.TAP_ROWS), ::vi.TAP_STRIDE]
        _bar(f'vit8pt Block {i} vs the reference fp32 taps', rows(got[i]), want, float((want.double() - rows(t64[i])).abs().max()), 4.0)


def test_forward_features_against_the_golden():
    m, ref, inp = setup()
    g = np.load(GOLDEN)
    from far_amd import ops
    ops.overflow_flag('cuda').zero_()
    with torch.no_grad():
        out = m.forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
    assert not ops.activation_overflowed('cuda')
    for name, t in zip(OUTPUTS, out):
        want = g[name]
        sc = float(np.abs(want).max())
        d = float(np.abs(t.cpu().numpy() - want).max())
        print(f'[vit8pt] {name}: max |got - reference| / max|reference| = {d / sc:.3e}')
        assert t.shape == want.shape and d <= 1e-3 * sc, name
    mtx = out[2].double()
    eye = torch.eye(3, dtype=torch.float64, device='cuda')
    assert float((mtx.transpose(1, 2) @ mtx - eye).abs().max()) <= 1e-5
    assert float((torch.linalg.det(mtx) - 1).abs().max()) <= 1e-5
    # the same through loftr_gate_inputs from a pipeline-shaped data dict: the same bits
    from far_amd.vit8pt import loftr_gate_inputs
    data = {'loftr_rt': inp['loftr_preds'][:, :3].contiguous(), 'num_correspondences_after_ransac': inp['loftr_num_corr'].to(torch.int32)}
    preds, ncorr = loftr_gate_inputs(data)
    with torch.no_grad():
        out2 = m.forward_features(inp['features'], inp['intrinsics'], ncorr, preds)
    for a, b in zip(out, out2):
        assert torch.equal(a, b)
    # the gate takes part: another solver pose gives another answer
    with torch.no_grad():
        out3 = m.forward_features(inp['features'], inp['intrinsics'], ncorr, preds.flip(0))
    assert not torch.equal(out[0], out3[0])


@pytest.mark.parametrize('over', [dict(use_loftr_gating=False), dict(use_normalized_6d=False), dict(transformer_depth=2)])
def test_other_configurations_against_float64(over):
    m, ref, inp = setup(**over)
    with torch.no_grad():
        out = m.forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
        want = ref.as_dtype(torch.float64, 'cuda').forward_features(inp['features'], vi.VIT_INTRINSICS, inp['loftr_num_corr'], inp['loftr_preds'])
    for name, a, b in zip(OUTPUTS, out, want):
        sc = float(b.abs().max())
        d = float((a.double() - b).abs().max())
        print(f'[vit8pt {over}] {name}: max |got - float64| / max = {d / sc:.3e}')
        assert d <= 1e-3 * sc, name


def test_no_intrinsics_uses_the_plain_table():
    m, ref, inp = setup()
    with torch.no_grad():
        f = m.trunk(inp['features'], None)
        f64 = ref.as_dtype(torch.float64, 'cuda').trunk(inp['features'], None)
        fk = m.trunk(inp['features'], inp['intrinsics'])
    assert float((f.double() - f64).abs().max()) <= 1e-3 * float(f64.abs().max())
    assert not torch.equal(f, fk)
    assert len(m.fusion_transformer._tables) == 2                         # one table per distinct value, kept


def test_pairs_have_the_same_bits_alone_and_in_a_batch_of_three():
    m, _, inp = setup(batch=3)
    args = lambda s: (inp['features'][2 * s.start:2 * s.stop], inp['intrinsics'][s], inp['loftr_num_corr'][s], inp['loftr_preds'][s])
    with torch.no_grad():
        out3 = m.forward_features(*args(slice(0, 3)))
        for b in range(3):
            out1 = m.forward_features(*args(slice(b, b + 1)))
            for name, a3, a1 in zip(OUTPUTS, out3, out1):
                assert torch.equal(a3[b:b + 1], a1), (b, name)
    # pair order: swapping the two pairs of a batch swaps the outputs (B = 1 cannot tell interleaved from concatenated)
    perm = torch.tensor([2, 3, 0, 1], device='cuda')
    with torch.no_grad():
        a = m.forward_features(inp['features'][:4], inp['intrinsics'][:2], inp['loftr_num_corr'][:2], inp['loftr_preds'][:2])
        b = m.forward_features(inp['features'][:4][perm], inp['intrinsics'][:2], inp['loftr_num_corr'][:2].flip(0), inp['loftr_preds'][:2].flip(0))
    for x, y in zip(a, b):
        assert torch.equal(x, y.flip(0))


def test_a_saved_reference_shaped_state_dict_loads_strictly(tmp_path):
    from far_amd.vit8pt import ViTEss
    _, ref, inp = setup()
    path = tmp_path / 'vit8pt.pt'
    ckpt = {'resnet.conv1.weight': torch.zeros(64, 3, 7, 7), 'extractor_final_conv.conv1.weight': torch.zeros(192, 128, 5, 5)}
    ckpt.update(ref.state_dict())                                        # what a released checkpoint holds: extractor entries too
    torch.save(ckpt, path)
    sd = {k: v for k, v in torch.load(path).items() if not k.startswith(vi.SKIP)}
    m = ViTEss(vi.vit_args(), inp['pose_mean'], inp['pose_std'])
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m0 = setup()[0]
    with torch.no_grad():
        a = m.eval().cuda().forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
        b = m0.forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_training_is_refused():
    m, _, inp = setup()
    with pytest.raises(NotImplementedError, match='far_vit_attention_f16s'):
        m.forward_features(inp['features'], inp['intrinsics'], inp['loftr_num_corr'], inp['loftr_preds'])     # parameters need gradients
