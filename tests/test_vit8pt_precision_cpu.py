"""ViTEss.set_precision and the plain-fp16 siblings of K23 / K24 on the CPU: the setter's arguments, what it sets and restores, the
size queries of the plain weight image, and the refusals that need no GPU.  Nothing here launches a kernel."""
import pytest
import torch

from tests import vit8pt_inputs as vi


def _model(extractor=False):
    from far_amd.vit8pt import ViTEss
    return ViTEss(vi.vit_args(), extractor=extractor)


def _switches(m):
    """Every attribute set_precision writes, by module path."""
    from far_amd.vit8pt import Block
    out = {'precision_stages': m.precision_stages, 'extractor_split': m.extractor_split}
    for i, blk in enumerate(m.fusion_transformer.blocks):
        if isinstance(blk, Block):
            out[f'{i}.attn.split_operands'], out[f'{i}.attn.plain16'] = blk.attn.split_operands, blk.attn.plain16
        else:
            out[f'{i}.cross_attn.plain16'] = blk.cross_attn.plain16
        out[f'{i}.mlp.split_operands'] = blk.mlp.split_operands
    return out


def test_modes_and_stage_iterables():
    from far_amd.vit8pt import ViTEss
    assert ViTEss.STAGES == ('extractor', 'blocks_dense', 'blocks_attn', 'cross')
    assert ViTEss.MODES == {'fp32': (), 'fp16': ViTEss.STAGES}
    m = _model(extractor=True)
    keys = list(m.state_dict())
    assert m.precision_stages == ()
    assert m.set_precision('fp16') is m and m.precision_stages == ViTEss.STAGES
    assert m.set_precision('fp32') is m and m.precision_stages == ()
    assert m.set_precision(['cross', 'extractor']).precision_stages == ('extractor', 'cross')          # STAGES order, a tuple
    assert m.set_precision(s for s in ('blocks_attn', 'blocks_dense')).precision_stages == ('blocks_dense', 'blocks_attn')
    assert m.set_precision(()).precision_stages == ()
    assert list(m.state_dict()) == keys
    for bad in ('fp64', 'mixed16', ['blocks'], ['cross', 'k1'], 3, [3], None):
        with pytest.raises(ValueError, match='blocks_dense'):
            m.set_precision(bad)
    assert m.precision_stages == ()                                          # a refused call changes nothing


def test_extractor_stage_needs_an_extractor():
    m = _model()
    for mode in ('fp16', ['extractor'], ('cross', 'extractor')):
        with pytest.raises(ValueError, match='extractor'):
            m.set_precision(mode)
    assert m.precision_stages == ()
    assert m.set_precision(('blocks_dense', 'blocks_attn', 'cross')).precision_stages == ('blocks_dense', 'blocks_attn', 'cross')


def test_each_stage_sets_its_own_switches_and_fp32_restores_all():
    from far_amd.vit8pt import Block
    m = _model(extractor=True)
    base = _switches(m)
    assert all(v is True for k, v in base.items() if k.endswith(('split_operands', 'extractor_split')))
    assert all(v is False for k, v in base.items() if k.endswith('plain16'))
    changed = {}
    for stage in m.STAGES:
        now = _switches(m.set_precision([stage]))
        changed[stage] = {k for k in base if k != 'precision_stages' and now[k] != base[k]}
        assert changed[stage], stage
    nblk = sum(isinstance(b, Block) for b in m.fusion_transformer.blocks)
    last = len(m.fusion_transformer.blocks) - 1
    assert changed['extractor'] == {'extractor_split'}
    assert changed['blocks_dense'] == {f'{i}.{x}.split_operands' for i in range(nblk) for x in ('attn', 'mlp')}
    assert changed['blocks_attn'] == {f'{i}.attn.plain16' for i in range(nblk)}
    assert changed['cross'] == {f'{last}.cross_attn.plain16', f'{last}.mlp.split_operands'}
    m.set_precision('fp16')
    assert {k for k in base if k != 'precision_stages' and _switches(m)[k] != base[k]} == set().union(*changed.values())
    assert _switches(m.set_precision('fp32')) == base
    # another model of the process is untouched: instance attributes, not class attributes
    assert _switches(_model(extractor=True)) == base


def test_plain_image_size_query():
    from far_amd import _lib
    lib = _lib.load()
    assert lib.far_conv_valid_f16_packed_bytes(128, 192, 5) == lib.far_conv_valid_packed_bytes(128, 192, 5) // 2 == 128 * 192 * 25 * 2
    assert lib.far_conv_valid_f16_packed_bytes(192, 192, 5) == lib.far_conv_valid_packed_bytes(192, 192, 5) // 2
    for cin, cout, k in ((128, 192, 3), (100, 192, 5), (128, 48, 5)):
        assert lib.far_conv_valid_f16_packed_bytes(cin, cout, k) == 0


def test_refusals_without_a_gpu():
    from far_amd import _lib, ops
    x = torch.zeros(1, 40, 192)
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention(x, x, x, 3, plain16=True)
    with pytest.raises(_lib.FarHipError):
        ops.vit_attention_planes(torch.zeros(9, 1, 40, 64), 3, plain16=True)
    w = torch.zeros(192, 128, 5, 5)
    with pytest.raises(_lib.FarHipError, match='forward only'):
        ops.PackedConvValid(w, split=False, dgrad=True, pack_scale=torch.zeros(2))
    with pytest.raises(_lib.FarHipError):
        ops.PackedConvValid(w, split=False)                                   # a CPU weight: no eager fallback


def test_gradients_with_a_stage_on_are_refused_before_any_launch():
    m = _model().set_precision(['blocks_attn'])
    feats = torch.zeros(2, 576, 192)
    for training in (False, True):
        m.set_block_training(training)
        with pytest.raises(NotImplementedError, match='set_precision'):
            m.forward_features(feats)                                         # parameters need gradients
    m.set_precision('fp32').set_block_training(False)
    with pytest.raises(NotImplementedError, match='far_vit_attention_f16s'):  # as before the switch existed
        m.forward_features(feats)
