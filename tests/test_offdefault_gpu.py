"""far_amd.loftr.LoFTR in evaluation mode OFF its default launch sequence: images of unequal size, padded coarse masks with scales,
one image under 64 coarse tokens (inputs: tests/util.py:offdefault_inputs; golden G20 = the reference's own run on them).

The model picks its launches by the shape of its inputs (model.py:_feature_extraction, transformer.py:LocalFeatureTransformer /
LoFTREncoderLayer, stages.py:CoarseMatching / FinePreprocess / FineMatching); every other end-to-end parity test takes the default
branch of each.  Per case here:
  (a) against the reference (G20) with G7's protocol and G7's bars for the same quantity (tests/test_pipeline_gpu.py:33-59);
  (b) against oracle.model.matcher_forward in float64 on the FULL coarse tokens and mconf;
  (c) the branch ran, with the right arguments (the far_amd.ops entry points wrapped by recorders);
  (d) masks of ones == no masks (two branches, one function);
  (e) run-to-run bits and batch independence;
  (f) the Sinkhorn model on the same inputs against the direct ops call and the float64 definition;
  (h) the masked d256 sequence at the bench grid next to a busy stream.
((g), K5's masked forward on its own, is in tests/test_fine_attn_gpu.py.)

Would the tests notice?  One-line mutations of the glue, each run once against this file on MI355X (none changes an index, length
or size handed to a kernel), and the tests they turned red ((a) = test_matcher_vs_reference_golden, (b) =
test_full_tokens_and_mconf_vs_float64_oracle, (c) = test_the_branch_ran_with_the_right_arguments, (d) =
test_masks_of_ones_equal_no_masks, (h) = test_masked_bench_grid_next_to_a_busy_stream):
  1. transformer.py cross layer, second call: `mask1, mask0` -> `mask0, mask1` (equal-canvas cases only)
         -> (a), (b), (c) [masked]
  2. stages.py CoarseMatching valid_hw: height / width of image 1 swapped
         -> (a), (b), (c) [masked, masked_unequal, masked_all_true], (d)
  3. stages.py FineMatching: `s1 = None` always
         -> (a), (c) [masked, masked_unequal, masked_all_true]
  4. transformer.py self layers: `None, None` for the masks
         -> (a), (b) [masked, masked_unequal], (c) [all three masked cases], (d), (h) (their launch-sequence assertions)
  5. stages.py CoarseMatching: `None` for s1 into ops.coarse_match
         -> (a), (c) [masked, masked_unequal, masked_all_true]
A wrong width (`hw1_c[1]` -> `hw0_c[1]` in FinePreprocess) is not run on the GPU -- the gather would read outside its map --; it is
caught by the argument assertions of (c): test_recording_stubs_catch_a_wrong_gather_width applies it with every ops entry point
replaced by a stub that launches nothing.
"""
import inspect
import os

import numpy as np
import pytest
import torch

from far_amd import synth
from far_amd.config import far_eval_config
from tests.util import (OFFDEFAULT, OFFDEFAULT_MASKED, deviation, g20_common, g20_input_conditions, ids_protocol, margin_rows,
                        offdefault_data, offdefault_inputs)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = list(OFFDEFAULT)

# G7's bars (tests/test_pipeline_gpu.py:40-59), by quantity: (atol, rtol)
BAR_FEATS_C, BAR_FMAP_F, BAR_TOKENS = (6e-5, 1e-4), (1.2e-4, 1e-4), (7e-5, 1e-4)
BAR_MCONF, BAR_MKPTS1_F, BAR_EXPEC_F = 1.5e-4, 4e-3, 1.5e-3
OUT_KEYS = ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c', 'mkpts0_f', 'mkpts1_f', 'expec_f', 'featmap0', 'featmap1')


@pytest.fixture(scope='module')
def model():
    from far_amd.loftr import LoFTR
    m = LoFTR(far_eval_config()).eval()
    synth.load_synthetic(m, seed=0)
    return m.cuda()


@pytest.fixture(scope='module')
def g20():
    return np.load(os.path.join(G, 'g20_matcher_offdefault.npz'))


def _forward(model, inp, masks=True):
    data = offdefault_data(inp, 'cuda', masks=masks)
    with torch.no_grad():
        model(data)
    torch.cuda.synchronize()
    return data


def _ids(data):
    return tuple(data[k].cpu().numpy() for k in ('b_ids', 'i_ids', 'j_ids'))


def _max_scale1(inp):
    return float(inp['scale1'].max()) if 'scale1' in inp else 1.0


def _values_within_g7_bars(what, got, ref, a, b, inp):
    """mconf / mkpts1_f / expec_f of the common matches (a into got, b into ref) at G7's bars; mkpts1_f's bar in pixels of the
    original image: scaled by the largest scale1 entry."""
    deviation(f'{what} mconf', got['mconf'][a], ref['mconf'][b], atol=BAR_MCONF)
    deviation(f'{what} mkpts1_f', got['mkpts1_f'][a], ref['mkpts1_f'][b], atol=BAR_MKPTS1_F * _max_scale1(inp))
    deviation(f'{what} expec_f', got['expec_f'][a], ref['expec_f'][b], atol=BAR_EXPEC_F)


# ---------------------------------------------------------------------------------------------------------------------
# (a) against the reference's own run
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_matcher_vs_reference_golden(model, g20, case):
    g = g20
    g20_input_conditions(g, case)
    inp = offdefault_inputs(case)
    data = _forward(model, inp)
    ref = {k: g[f'{case}__{k}'] for k in ('mconf', 'mkpts0_c', 'mkpts1_c', 'mkpts1_f', 'expec_f')}
    assert tuple(data['hw0_c']) == tuple(g[f'{case}__hw0_c']) and tuple(data['hw1_c']) == tuple(g[f'{case}__hw1_c'])
    # the coarse backbone maps (replaced by the tokens in `data`): from the public feature-extraction call
    d2 = offdefault_data(inp, 'cuda')
    with torch.no_grad():
        model.forward_feature_extraction(d2)
    for k in ('0', '1'):
        deviation(f'g20 {case} coarse map {k}', d2['featmap' + k][:, ::16, ::3, ::5], g[f'{case}__featc{k}_sample'],
                  atol=BAR_FEATS_C[0], rtol=BAR_FEATS_C[1])
        deviation(f'g20 {case} featmap_f{k}', data['featmap_f' + k][:, ::16, ::7, ::9], g[f'{case}__featmap_f{k}_sample'],
                  atol=BAR_FMAP_F[0], rtol=BAR_FMAP_F[1])
        st = int(g[f'{case}__token_stride'])
        deviation(f'g20 {case} featmap{k} (tokens)', data['featmap' + k][:, ::st], g[f'{case}__featmap{k}'],
                  atol=BAR_TOKENS[0], rtol=BAR_TOKENS[1])
    a, b = g20_common(g, case, _ids(data), 1e-4, 0.99)
    got = {k: data[k].cpu().numpy() for k in ref}
    for k in ('mkpts0_c', 'mkpts1_c'):           # exact without scales, rtol 1e-6 with them (tests/test_coarse_gpu.py)
        np.testing.assert_allclose(got[k][a], ref[k][b], rtol=1e-6 if 'scale0' in inp else 0, atol=0, err_msg=k)
    _values_within_g7_bars(f'g20 {case}', got, ref, a, b, inp)


# ---------------------------------------------------------------------------------------------------------------------
# (b) against the float64 oracle on the full tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_full_tokens_and_mconf_vs_float64_oracle(model, g20, case):
    """Bar per quantity: max(G7's bar, 3 x dev32_*): dev32_* (stored in G20) is what the reference's fp32 arithmetic loses against
    the float64 oracle on the same input.  Both parts are printed."""
    import json
    from oracle import model as om
    man = json.load(open(os.path.join(G, 'g8_state_dict_manifest.json')))
    w = om.Weights(synth.synthetic_state_dict({k: tuple(v) for k, v in man.items()}))
    inp = offdefault_inputs(case)
    o = om.matcher_forward(w, far_eval_config(), inp['image0'], inp['image1'], mask0=inp.get('mask0'), mask1=inp.get('mask1'),
                           scale0=inp.get('scale0'), scale1=inp.get('scale1'), dtype=np.float64)
    data = _forward(model, inp)
    d32 = float(g20[f'{case}__dev32_tokens'])
    bar = max(BAR_TOKENS[0], 3 * d32)
    print(f'[float64 {case}] tokens bar {bar:.2e} = max(G7 {BAR_TOKENS[0]:g}, 3 x dev32 {d32:.2e})')
    for k in ('featmap0', 'featmap1'):
        assert tuple(data[k].shape) == o[k].shape
        deviation(f'float64 {case} {k} (all tokens)', data[k], o[k], atol=bar, rtol=BAR_TOKENS[1])
    safe = margin_rows(g20, case, margin=1e-4)
    a, b = ids_protocol(f'float64 {case}', _ids(data), (o['b_ids'], o['i_ids'], o['j_ids']), safe, 0.99)
    d32 = float(g20[f'{case}__dev32_mconf'])
    bar = max(BAR_MCONF, 3 * d32)
    print(f'[float64 {case}] mconf bar {bar:.2e} = max(G7 {BAR_MCONF:g}, 3 x dev32 {d32:.2e})')
    deviation(f'float64 {case} mconf', data['mconf'][a], o['mconf'][b], atol=bar)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the branch ran, with the right arguments
# ---------------------------------------------------------------------------------------------------------------------
RECORDED = ('fine_gather', 'linear_gather_f16s', 'linear_kv_state', 'linear_q_apply', 'linear_attention', 'linear_attention_apply',
            'coarse_match', 'fine_expect')


def _record(monkeypatch, stub=None):
    """Wraps the far_amd.ops entry points of RECORDED: -> {name: [bound arguments per call]}.  stub(name, arguments) replaces the
    launch when given."""
    from far_amd import ops
    calls = {n: [] for n in RECORDED}
    for name in RECORDED:
        orig = getattr(ops, name)
        sig = inspect.signature(orig)

        def wrapper(*a, _orig=orig, _sig=sig, _name=name, **kw):
            bound = _sig.bind(*a, **kw)
            bound.apply_defaults()
            calls[_name].append(bound.arguments)
            return _orig(*a, **kw) if stub is None else stub(_name, bound.arguments)
        monkeypatch.setattr(ops, name, wrapper)
    return calls


def _check_gather_widths(calls, data):
    """FinePreprocess off the fused gather: ops.fine_gather once per image, each with ITS image's coarse width and fine map."""
    fg = calls['fine_gather']
    assert len(fg) == 2 and not calls['linear_gather_f16s']
    stride = data['hw0_f'][0] // data['hw0_c'][0]
    for c, hw_c, hw_f, ids in ((fg[0], data['hw0_c'], data['hw0_f'], data['i_ids']), (fg[1], data['hw1_c'], data['hw1_f'], data['j_ids'])):
        assert c['wc'] == hw_c[1] and c['stride'] == stride
        assert tuple(c['feat_f'].shape[2:]) == tuple(hw_f) and hw_f[1] == hw_c[1] * stride
        assert torch.equal(c['cell_ids'], ids) and int(c['cell_ids'].max()) < hw_c[0] * hw_c[1]


def _check_unequal(calls, data, inp):
    N = inp['image0'].shape[0]
    L0, L1 = data['hw0_c'][0] * data['hw0_c'][1], data['hw1_c'][0] * data['hw1_c'][1]
    assert L0 != L1 and data['hw0_c'][1] != data['hw1_c'][1] and data['feats_c'] is None
    _check_gather_widths(calls, data)
    kv = [c for c in calls['linear_kv_state'] if c['x'].shape[-1] == 256]
    assert kv and all(c['x'].shape[0] == N and c['S'] == c['x'].shape[1] for c in kv)          # per image: no stacked self layers
    qa = [c for c in calls['linear_q_apply'] if c['x'].shape[-1] == 256]
    assert {(c['x'].shape[1], c['S']) for c in qa} == {(L0, L0), (L1, L1), (L0, L1), (L1, L0)}   # L != S in the cross launches
    assert not calls['linear_attention']


def _check_short_side(calls, data, inp):
    L0, L1 = data['hw0_c'][0] * data['hw0_c'][1], data['hw1_c'][0] * data['hw1_c'][1]
    assert L0 < 64 <= L1
    plain = calls['linear_attention']
    assert plain and all(c['q_mask'] is None and c['kv_mask'] is None and c['k'].shape[1] == L0 for c in plain)
    assert {c['q'].shape[1] for c in plain} == {L0, L1}                 # image 0's self layers, and image 1 reading image 0
    ap = calls['linear_attention_apply']
    assert ap and all(c['q'].shape[1] == L0 and c['S'] == L1 for c in ap)   # image 0 reading image 1: k|v-state + apply
    assert all(c['S'] == L1 for c in calls['linear_kv_state'])
    _check_gather_widths(calls, data)


def _check_masked(calls, data, inp, model):
    N = inp['image0'].shape[0]
    m = {0: torch.from_numpy(inp['mask0'].reshape(N, -1).astype(np.uint8)).cuda(),
         1: torch.from_numpy(inp['mask1'].reshape(N, -1).astype(np.uint8)).cuda()}
    assert not calls['linear_q_apply'] and not calls['linear_kv_state'] and not calls['linear_attention_apply']
    la = calls['linear_attention']
    names = model.loftr_coarse.layer_names
    assert len(la) == 2 * len(names)
    # the reference's order (loftr_module/transformer.py:101-108): self (m0, m0), (m1, m1); cross (m0, m1), (m1, m0)
    want = [p for n in names for p in (((0, 0), (1, 1)) if n == 'self' else ((0, 1), (1, 0)))]
    for k, (c, (qi, ki)) in enumerate(zip(la, want)):
        assert c['q_mask'] is not None and c['kv_mask'] is not None, k
        assert c['q_mask'].dtype == torch.uint8 and c['kv_mask'].dtype == torch.uint8
        assert tuple(c['q_mask'].shape) == tuple(c['q'].shape[:2]) and tuple(c['kv_mask'].shape) == tuple(c['k'].shape[:2]), k
        assert torch.equal(c['q_mask'], m[qi]) and torch.equal(c['kv_mask'], m[ki]), f'coarse attention call {k}: masks of images {(qi, ki)} expected'
    cm, = calls['coarse_match']
    assert torch.equal(cm['mask0'], m[0]) and torch.equal(cm['mask1'], m[1])
    assert cm['valid_hw'].dtype == torch.int32 and np.array_equal(cm['valid_hw'].cpu().numpy(), inp['extents'])
    assert np.array_equal(cm['scale0'].cpu().numpy(), inp['scale0']) and np.array_equal(cm['scale1'].cpu().numpy(), inp['scale1'])
    assert tuple(cm['hw0']) == tuple(data['hw0_c']) and tuple(cm['hw1']) == tuple(data['hw1_c'])
    fe, = calls['fine_expect']
    assert fe['scale1'] is not None and np.array_equal(fe['scale1'].cpu().numpy(), inp['scale1']) and torch.equal(fe['b_ids'], data['b_ids'])
    if data['hw0_c'] != data['hw1_c']:
        _check_gather_widths(calls, data)


def _check_case(case, calls, data, inp, model):
    if case == 'unequal':
        _check_unequal(calls, data, inp)
    elif case == 'short_side':
        _check_short_side(calls, data, inp)
    else:
        _check_masked(calls, data, inp, model)


@pytest.mark.parametrize('case', CASES)
def test_the_branch_ran_with_the_right_arguments(model, monkeypatch, case):
    inp = offdefault_inputs(case)
    calls = _record(monkeypatch)
    data = _forward(model, inp)
    assert data['b_ids'].numel() >= OFFDEFAULT[case]['min_matches']
    _check_case(case, calls, data, inp, model)


def test_recording_stubs_catch_a_wrong_gather_width(model, monkeypatch):
    """The guard against a wrong width handed to the gather (never run on the GPU with real launches: it would read outside the
    map).  Every recorded ops entry point is replaced by a stub that launches nothing and returns zeros of the right shape (K1's
    stub returns a few in-range matches); FinePreprocess is then run with image 0's coarse width for both images, as a mutation
    of stages.py would, and the argument assertions of (c) must refuse it -- and accept the unmutated module."""
    from far_amd.loftr import stages
    inp = offdefault_inputs('unequal')
    dev = 'cuda'

    def stub(name, a):
        if name == 'coarse_match':
            N, M = a['f0'].shape[0], 6
            L1 = a['hw1'][0] * a['hw1'][1]
            b = torch.arange(N, device=dev).repeat_interleave(M)
            i = torch.arange(M, device=dev).repeat(N) * 7
            return {'b_ids': b, 'i_ids': i, 'j_ids': L1 - 1 - i, 'mconf': torch.full((N * M,), 0.5, device=dev),
                    'mkpts0_c': torch.zeros(N * M, 2, device=dev), 'mkpts1_c': torch.zeros(N * M, 2, device=dev),
                    'counts': [M] * N, 'conf_matrix': None}
        if name == 'fine_gather':
            out = a['out'] if a['out'] is not None else torch.zeros(a['b_ids'].numel(), a['W'] ** 2, a['feat_f'].shape[1], device=dev)
            return out.zero_()
        if name == 'fine_expect':
            M = a['feat0'].shape[0]
            return torch.zeros(M, 3, device=dev), torch.zeros(M, 2, device=dev)
        if name in ('linear_q_apply', 'linear_attention_apply', 'linear_attention'):
            q = a['x'] if name == 'linear_q_apply' else a['q']
            return torch.zeros(q.shape[0], q.shape[1], 256 if name == 'linear_q_apply' else q.shape[2], device=dev)
        if name == 'linear_kv_state':
            n = a['x'].shape[0]
            kv = torch.zeros(n, 256, 33, device=dev)
            return (kv, torch.zeros(1, device=dev)) if a['want_image'] else kv
        raise AssertionError(name)
    calls = _record(monkeypatch, stub)
    data = _forward(model, inp)
    _check_gather_widths(calls, data)                       # the module as it is: accepted

    class WrongWidth(dict):                                 # hw1_c read as hw0_c inside FinePreprocess only
        def __getitem__(self, k):
            return dict.__getitem__(self, 'hw0_c' if k == 'hw1_c' else k)
    orig = stages.FinePreprocess.forward

    def mutated(self, f0, f1, c0, c1, d):
        wd = WrongWidth(d)
        out = orig(self, f0, f1, c0, c1, wd)
        d['W'] = dict.__getitem__(wd, 'W')
        return out
    monkeypatch.setattr(stages.FinePreprocess, 'forward', mutated)
    for v in calls.values():
        v.clear()
    data = _forward(model, inp)
    with pytest.raises(AssertionError):
        _check_gather_widths(calls, data)


# ---------------------------------------------------------------------------------------------------------------------
# (d) two branches, one function
# ---------------------------------------------------------------------------------------------------------------------
def test_masks_of_ones_equal_no_masks(model, g20, monkeypatch):
    """mask_border_with_padding with full extents is mask_border, a mask of ones multiplies by one (coarse_matching.py:8-43,
    linear_attention.py:38-42): the masked sequence (q|k|v planes + K5, K1 with masks and extents) and the default fused one
    compute the same function.  Ids identical on the reference's margin rows, values within the bars of (a)."""
    case = 'masked_all_true'
    inp = offdefault_inputs(case)
    calls = _record(monkeypatch)
    masked = _forward(model, inp)
    assert calls['linear_attention'] and not calls['linear_q_apply']
    for v in calls.values():
        v.clear()
    plain = _forward(model, inp, masks=False)
    assert calls['linear_q_apply'] and not calls['linear_attention'] and calls['linear_gather_f16s']     # the default sequence
    a, b = ids_protocol('ones vs none', _ids(masked), _ids(plain), margin_rows(g20, case, margin=1e-4), 0.99)
    for k in ('featmap0', 'featmap1'):
        deviation(f'ones vs none {k}', masked[k], plain[k], atol=BAR_TOKENS[0], rtol=BAR_TOKENS[1])
    got, ref = ({k: d[k].cpu().numpy() for k in ('mconf', 'mkpts0_c', 'mkpts1_c', 'mkpts1_f', 'expec_f')} for d in (masked, plain))
    for k in ('mkpts0_c', 'mkpts1_c'):
        np.testing.assert_array_equal(got[k][a], ref[k][b])
    _values_within_g7_bars('ones vs none', got, ref, a, b, inp)


# ---------------------------------------------------------------------------------------------------------------------
# (e) determinism and batch independence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_twice_identical_and_pair0_alone(model, g20, case):
    inp = offdefault_inputs(case)
    first, second = _forward(model, inp), _forward(model, inp)
    for k in OUT_KEYS:
        assert torch.equal(first[k], second[k]), k
    one = _forward(model, {k: v[:1] for k, v in inp.items()})
    sel = first['b_ids'] == 0
    for k in ('i_ids', 'j_ids'):
        assert torch.equal(one[k], first[k][sel]), k
    same = {k: torch.equal(one[k], first[k][sel]) for k in ('mconf', 'mkpts0_c', 'mkpts1_c', 'mkpts1_f', 'expec_f')}
    same.update({k: torch.equal(one[k][0], first[k][0]) for k in ('featmap0', 'featmap1')})
    print(f'[pair 0 alone, {case}] bit-identical to the batch of two:', same)
    n = int(sel.sum())
    idx = np.arange(n)
    got, ref = ({k: d[k].cpu().numpy() for k in ('mconf', 'mkpts1_f', 'expec_f')} for d in (one, first))
    _values_within_g7_bars(f'pair 0 alone {case}', got, ref, idx, np.nonzero(sel.cpu().numpy())[0], inp)
    for k in ('featmap0', 'featmap1'):
        deviation(f'pair 0 alone {case} {k}', one[k][0], first[k][0], atol=BAR_TOKENS[0], rtol=BAR_TOKENS[1])
    assert all(same.values()), same          # measured on MI355X: every case is bit-identical, like the default path


# ---------------------------------------------------------------------------------------------------------------------
# (f) the Sinkhorn model on the same inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['unequal', 'masked'])
def test_sinkhorn_model_offdefault(case):
    """match_type 'sinkhorn' with skh_prefilter on the unequal / masked inputs: the model's coarse outputs equal
    ops.coarse_match_sinkhorn called directly on the captured tokens with the masks, extents and scales restated here from the
    data dict, and that call agrees with the float64 definition (tests/test_sinkhorn_gpu.py:oracle) and the reference's selection
    (oracle.coarse.get_coarse_match, pinned to G20 with masks on the CPU): ids bit-exact, mconf at that file's bar.  The reference
    cannot run this match type (it imports a module its tree does not have), so this leg is pinned to the float64 definition only."""
    from far_amd import ops
    from oracle import coarse as oc
    from tests import test_sinkhorn_gpu as sk
    m, cap = sk._ot_model()
    inp = offdefault_inputs(case)
    data = _forward(m, inp)
    N = inp['image0'].shape[0]
    cmod = m.coarse_matching
    hw0, hw1, hw_i = tuple(data['hw0_c']), tuple(data['hw1_c']), tuple(data['hw0_i'])
    m0 = m1 = vh = s0 = s1 = None
    if 'mask0' in inp:
        b0, b1 = data['mask0'].cpu().numpy(), data['mask1'].cpu().numpy()
        m0, m1 = (torch.from_numpy(b.reshape(N, -1).astype(np.uint8)).cuda() for b in (b0, b1))
        # rows / columns that hold a valid cell (rectangular padding masks): (h0, w0, h1, w1) per pair
        ext = np.stack([b0.any(2).sum(1), b0.any(1).sum(1), b1.any(2).sum(1), b1.any(1).sum(1)], 1)
        assert np.array_equal(ext, inp['extents'])
        vh = torch.from_numpy(ext.astype(np.int32)).cuda()
        s0, s1 = data['scale0'].float().contiguous(), data['scale1'].float().contiguous()
    ref = ops.coarse_match_sinkhorn(cap['f0'], cap['f1'], cmod.bin_score, cmod.skh_iters, cmod.thr, cmod.border_rm, hw0, hw1,
                                    hw_i[0] / hw0[0], m0, m1, vh, s0, s1, prefilter=True)
    print(f'[sinkhorn model {case}] coarse matches: {ref["b_ids"].numel()}')
    assert ref['b_ids'].numel() > 0
    for k in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c'):
        assert torch.equal(data[k], ref[k]), k
    f0, f1 = cap['f0'].cpu().numpy(), cap['f1'].cpu().numpy()
    L, S = f0.shape[1], f1.shape[1]
    bm0, bm1 = (None, None) if m0 is None else (inp['mask0'].reshape(N, -1), inp['mask1'].reshape(N, -1))
    A, _, _ = sk.oracle(f0, f1, 1.0, cmod.skh_iters, bm0, bm1, prefilter=True)
    conf = A[:, :L, :S]
    sk._margin_ok(conf)
    want = oc.get_coarse_match(conf, cmod.thr, cmod.border_rm, hw0, hw1, hw_i, inp.get('scale0'), inp.get('scale1'),
                               inp.get('mask0'), inp.get('mask1'))
    for k in ('b_ids', 'i_ids', 'j_ids'):
        np.testing.assert_array_equal(ref[k].cpu().numpy(), want[k], err_msg=k)
    for k in ('mkpts0_c', 'mkpts1_c'):
        np.testing.assert_allclose(ref[k].cpu().numpy(), want[k], rtol=1e-6 if s0 is not None else 0, atol=0)
    A32, _, _ = sk.restatement32(f0, f1, 1.0, cmod.skh_iters, bm0, bm1, prefilter=True)
    idx = (want['b_ids'], want['i_ids'], want['j_ids'])
    sk._bar(f'sinkhorn model {case} mconf', sk._dev(ref['mconf'].cpu().numpy(), conf[idx]), sk.ATOL_CONF, sk._dev(A32[idx], conf[idx]))


# ---------------------------------------------------------------------------------------------------------------------
# (h) the masked d256 sequence at the bench grid next to a busy stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_masked_bench_grid_next_to_a_busy_stream(model, monkeypatch):
    """The `masked` inputs at the bench grid (480 x 640 canvas, 60 x 80 cells, 8 pairs: q|k|v planes + K5 with masks at d256, K1
    with masks, extents and scales) next to tests/test_determinism_gpu.py's busy stream: every output bit-identical over its
    launches."""
    from tests.test_determinism_gpu import _repeat
    inp = offdefault_inputs('masked', N=8, canvas=(480, 640))
    assert inp['mask0'].shape == (8, 60, 80) and not inp['mask0'].all() and not inp['mask1'].all()
    calls = _record(monkeypatch)
    first = _forward(model, inp)
    assert first['b_ids'].numel() > 8 * 100 and calls['linear_attention'] and not calls['linear_q_apply']
    monkeypatch.undo()

    def fn():
        d = _forward(model, inp)
        return tuple(d[k] for k in OUT_KEYS)
    _repeat(fn, 'masked matcher 8 x 4800')
