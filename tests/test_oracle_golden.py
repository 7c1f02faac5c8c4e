"""Pins the oracle (oracle/*.py) to the REFERENCE: every check compares against tests/golden/*.npz, which
tools/make_goldens.py produced by running crockwell/far's own Python on CPU in the build container.
CPU only; a few seconds each.  Also pins the host-side mirror (far_amd modules that carry no kernel)."""
import json
import os

import numpy as np
import pytest
import torch

from far_amd import synth
from far_amd.config import far_eval_config
from tests.util import correlated_features

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name):
    return np.load(os.path.join(G, name + '.npz'), allow_pickle=False)


# ------------------------------------------------------------------------------------------------ G1
def test_g1_coarse_small_full_tensors():
    from oracle import coarse as oc
    g = load('g1_coarse_small')
    f0, f1, _ = correlated_features(2, (12, 16), 64, seed=1, amp=2.0)
    cfg = far_eval_config()['match_coarse']
    out = oc.coarse_matching(f0, f1, cfg, (12, 16), (12, 16), (96, 128))
    np.testing.assert_allclose(out['conf_matrix'], g['conf_matrix'], atol=2e-6, rtol=0)
    for k in ['b_ids', 'i_ids', 'j_ids']:
        np.testing.assert_array_equal(out[k], g[k])
    np.testing.assert_allclose(out['mconf'], g['mconf'], atol=2e-6, rtol=0)
    np.testing.assert_array_equal(out['mkpts0_c'], g['mkpts0_c'])
    np.testing.assert_array_equal(out['mkpts1_c'], g['mkpts1_c'])


def test_g1_coarse_full_grid_and_fp32_swamping():
    from oracle import coarse as oc
    g = load('g1_coarse_full')
    f0, f1, _ = correlated_features(1, (60, 80), 256, seed=3, amp=1.2, frac=0.8)
    cfg = far_eval_config()['match_coarse']
    out = oc.coarse_matching(f0, f1, cfg, (60, 80), (60, 80), (480, 640))
    for k in ['b_ids', 'i_ids', 'j_ids']:
        np.testing.assert_array_equal(out[k], g[k])
    # two fp32 evaluations (numpy here, torch/oneDNN in the reference) agree to ~5e-6 ...
    np.testing.assert_allclose(out['mconf'], g['mconf'], atol=2e-5, rtol=0)
    np.testing.assert_allclose(out['conf_matrix'][0].max(1), g['rowmax'], atol=2e-5, rtol=0)
    # ... but BOTH are ~7e-5 away from the exact value (softmax swamping): this is why the kernels are held
    # to the float64 evaluation at 1e-5 and to the fp32 restatement only at 2e-4
    c64 = oc.conf_matrix(f0, f1, 0.1, dtype=np.float64)
    dev = np.abs(c64[0].max(1) - g['rowmax']).max()
    assert 1e-5 < dev < 2e-4, dev


# ------------------------------------------------------------------------------------------------ G2
def test_g2_fine_windows_and_expectation():
    from oracle import fine as of
    g = load('g2_fine')
    M = len(g['i_ids'])
    b = np.zeros(M, np.int64)
    w0 = of.unfold_windows(g['ff0'], b, g['i_ids'], 8, 5, 4)
    w1 = of.unfold_windows(g['ff1'], b, g['j_ids'], 8, 5, 4)
    # the reference output went through down_proj / merge_feat: redo those two Linear layers with the same weights
    sd = synth.synthetic_state_dict({'fine_preprocess.down_proj.weight': (128, 256), 'fine_preprocess.down_proj.bias': (128,),
                                     'fine_preprocess.merge_feat.weight': (128, 256), 'fine_preprocess.merge_feat.bias': (128,)})
    t = lambda k: torch.from_numpy(sd['fine_preprocess.' + k])
    F = torch.nn.functional
    cw = F.linear(torch.from_numpy(np.concatenate([g['fc0'][0][g['i_ids']], g['fc1'][0][g['j_ids']]], 0)),
                  t('down_proj.weight'), t('down_proj.bias'))
    both = torch.cat([torch.from_numpy(np.concatenate([w0, w1], 0)), cw.unsqueeze(1).expand(-1, 25, -1)], -1)
    both = F.linear(both, t('merge_feat.weight'), t('merge_feat.bias')).numpy()
    np.testing.assert_allclose(both[:M], g['win0'], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(both[M:], g['win1'], atol=2e-5, rtol=1e-5)
    expec, mk1 = of.fine_matching(g['f0'], g['f1'], g['mk'], 4.0)
    np.testing.assert_allclose(expec, g['expec_f'], atol=2e-6, rtol=0)
    np.testing.assert_allclose(mk1, g['mkpts1_f'], atol=1e-4, rtol=0)


# ------------------------------------------------------------------------------------------------ G3
def _weights(prefixes):
    man = json.load(open(os.path.join(G, 'g8_state_dict_manifest.json')))
    shapes = {k: tuple(v) for k, v in man.items() if any(k.startswith(p) for p in prefixes)}
    from oracle.model import Weights
    return Weights(synth.synthetic_state_dict(shapes))


def test_g3_linear_attention_and_encoder():
    from oracle import attention as oa
    from oracle import model as om
    g = load('g3_encoder')
    q, k, v = (g[n].reshape(g[n].shape[0], g[n].shape[1], 256) for n in 'qkv')
    out = oa.linear_attention(q, k, v, 8)
    np.testing.assert_allclose(out, g['attn_out'].reshape(out.shape), atol=2e-5, rtol=1e-5)
    w = _weights(['loftr_coarse.'])
    y = om.encoder_layer(w, 'loftr_coarse.layers.1', g['x'], g['src'], 8)
    np.testing.assert_allclose(y, g['layer1_out'], atol=1e-4, rtol=1e-4)
    a, b = om.feature_transformer(w, 'loftr_coarse', g['x'], g['src'], ['self', 'cross'] * 3, 8)
    np.testing.assert_allclose(a, g['stack_out0'], atol=3e-4, rtol=1e-4)
    np.testing.assert_allclose(b, g['stack_out1'], atol=3e-4, rtol=1e-4)


# ------------------------------------------------------------------------------------------------ G4
def _g4_inputs():
    rng = np.random.default_rng(14)
    f0 = rng.standard_normal((1, 4800, 256)).astype(np.float32)
    f1 = (0.5 * f0 + rng.standard_normal((1, 4800, 256))).astype(np.float32)
    return f0, f1


def test_g4_positional_table():
    from far_amd.loftr.transformer import positional_table
    from oracle import head as oh
    g = load('g4_head')
    np.testing.assert_array_equal(oh.positional_encodings(), g['pos6'])       # oracle: literal loop, bit exact
    np.testing.assert_array_equal(positional_table().numpy(), g['pos6'])      # product: vectorised, bit exact


@pytest.mark.timeout(600)
def test_g4_head_block_and_regression():
    from oracle import model as om
    g = load('g4_head')
    f0, f1 = _g4_inputs()
    w = _weights(['loftr_regress.'])
    cfg = far_eval_config()
    e = 'loftr_regress.emm.'
    C = 256
    F = torch.nn.functional
    ln = lambda a: F.layer_norm(torch.from_numpy(a + w.sd[e + 'pos_embed']), (C,), w.t(e + 'norm1.weight'),
                                w.t(e + 'norm1.bias')).numpy()
    fa, fb = om.cross_attention(w, ln(f0), ln(f1), g['pos6'])
    scale = np.abs(g['xattn_a']).max()
    np.testing.assert_allclose(fa, g['xattn_a'], atol=2e-4 * scale, rtol=1e-3)
    np.testing.assert_allclose(fb, g['xattn_b'], atol=2e-4 * scale, rtol=1e-3)
    n = g['counts']
    lp, ilp = om.preprocess_helper(cfg, g['loftr_rt'], n[0], n[1], n[2], n[3])
    np.testing.assert_allclose(lp, g['loftr_preds_6d'], atol=1e-6, rtol=1e-6)
    np.testing.assert_allclose(ilp, g['inv_loftr_preds_6d'], atol=1e-5, rtol=1e-5)
    reg, gate, _ = om.head_forward(w, cfg, f0, f1, lp, ilp, g['pos6'])
    # north_star tolerance on the regression output: 1e-3 relative (fp32)
    np.testing.assert_allclose(reg, g['regressed_rt'], atol=1e-3 * np.abs(g['regressed_rt']).max(), rtol=1e-3)
    np.testing.assert_allclose(om.prior_from_regressed(reg), g['priorRT'], atol=2e-3, rtol=1e-3)


# ------------------------------------------------------------------------------------------------ G5
def test_g5_eight_point_decomposition_and_scores():
    from oracle import solver as osv
    g = load('g5_solver')
    K = g['K']
    kn0, kn1 = osv.normalize_keypoints(g['kpts0'], g['kpts1'], K, K)
    kp1 = kn0.astype(np.float32).astype(np.float64)
    kp2 = kn1.astype(np.float32).astype(np.float64)
    s = g['samples']
    F = osv.run_8point(kp1[s], kp2[s])
    # the float32 reference (torch.linalg.svd of a 9x9 Gram matrix) vs the float64 oracle: equal up to the
    # reference's own round-off, which grows with the conditioning of the sample
    rel = np.abs(F - g['F']).reshape(len(F), -1).max(1) / np.abs(g['F']).reshape(len(F), -1).max(1)
    assert np.median(rel) < 2e-3 and (rel < 5e-2).mean() > 0.9, (np.median(rel), (rel < 5e-2).mean())
    # decomposition of the SAME matrices: compare as sets {R1, R2} and t up to sign (LAPACK sign freedom)
    R1, R2, t = osv.decompose_essential(g['F'].astype(np.float64))
    a = np.minimum(np.abs(R1 - g['R1']).reshape(len(F), -1).max(1) + np.abs(R2 - g['R2']).reshape(len(F), -1).max(1),
                   np.abs(R1 - g['R2']).reshape(len(F), -1).max(1) + np.abs(R2 - g['R1']).reshape(len(F), -1).max(1))
    tt = g['T'][..., 0]
    dt = np.minimum(np.abs(t - tt).max(1), np.abs(t + tt).max(1))
    assert np.median(a) < 1e-4 and (a < 1e-2).mean() > 0.95, (np.median(a), (a < 1e-2).mean())
    assert np.median(dt) < 1e-4 and (dt < 1e-2).mean() > 0.95
    # Sampson distances of the SAME models on the same points (kornia restatement in the shim)
    samp = osv.sampson_distance(kp1, kp2, g['F'].astype(np.float64))
    ok = np.isfinite(g['sampson']) & (g['sampson'] < 1e-2)
    np.testing.assert_allclose(samp[ok], g['sampson'][ok], rtol=5e-3, atol=1e-9)
    cnt = (samp <= 3e-7).sum(1)
    assert (np.abs(cnt - g['count']) <= np.maximum(2, 0.02 * g['count'])).mean() > 0.98
    # prior error: min over the two candidates the reference happened to test vs. this build's convention
    # agree whenever the sign conventions coincide; check the convention-free lower envelope instead
    _, RTn = osv.prior_E(g['prior'])
    pcl = g['pcl'].astype(np.float64)
    tgt = pcl @ RTn[:, :3].T + RTn[:, 3]
    def err(R, tv):
        x = np.einsum('hij,pj->hpi', R, pcl) + tv[:, None, :]
        return np.abs(x - tgt[None]).reshape(len(R), -1).mean(1)
    cands = np.stack([err(R1, t), err(R2, t), err(R1, -t), err(R2, -t)], 1)
    ref = g['prior_err']
    d = np.abs(cands - ref[:, None]).min(1) / np.maximum(ref, 1e-6)
    assert np.median(d) < 1e-3 and (d < 5e-2).mean() > 0.9, (np.median(d), (d < 5e-2).mean())


def test_g5_oracle_solver_recovers_pose():
    from oracle import solver as osv
    g = load('g5_solver')
    ret, na, ti, ul, dbg = osv.estimate_pose(g['kpts0'], g['kpts1'], g['K'], g['K'], 0.5, solver='prior_ransac',
                                             priorRT=g['prior'], H=512, pcl=g['pcl'])
    R, t, mask, E = ret
    assert np.linalg.norm(R - g['R_gt']) < 0.03 and np.linalg.norm(t - g['t_gt']) < 0.1
    assert 300 < na <= mask.size and ti <= dbg['count'][dbg['best']]


# ------------------------------------------------------------------------------------------------ G6
def test_g6_pose6d_oracle_and_product():
    from far_amd import pose6d
    from oracle import model as om
    g = load('g6_pose6d')
    np.testing.assert_array_equal(pose6d.pose_mean_6d.numpy(), g['mean'])
    np.testing.assert_array_equal(pose6d.pose_std_6d.numpy(), g['std'])
    np.testing.assert_allclose(pose6d.rotation_6d_to_matrix(torch.from_numpy(g['d6'])).numpy(), g['R'], atol=1e-6)
    np.testing.assert_allclose(pose6d.compute_normalized_6d(torch.from_numpy(g['rt'])).numpy(), g['n6'], atol=1e-6)
    for i in range(len(g['d6'])):
        np.testing.assert_allclose(om.rotation_6d_to_matrix(g['d6'][i]), g['R'][i], atol=1e-6)
        np.testing.assert_allclose(om.normalized_6d(g['rt'][i]), g['n6'][i], atol=1e-5)


# ------------------------------------------------------------------------------------------------ G7
@pytest.mark.timeout(900)
def test_g7_full_matcher_forward():
    from oracle import model as om
    g = load('g7_full')
    man = json.load(open(os.path.join(G, 'g8_state_dict_manifest.json')))
    w = om.Weights(synth.synthetic_state_dict({k: tuple(v) for k, v in man.items()}))
    im0, im1 = synth.synth_image_pair(1, seed=0)
    data = om.matcher_forward(w, far_eval_config(), im0, im1)
    np.testing.assert_allclose(data['featmap0'][0, ::97], g['featmap0_sample'], atol=2e-3, rtol=1e-3)
    # ids: exact on the rows that have margin in the reference's own conf matrix
    safe = (np.abs(g['rowmax'] - 0.2) > 1e-3) & (g['rowgap'] > 1e-3)
    ref_rows = set(g['i_ids'].tolist())
    got = dict(zip(data['i_ids'].tolist(), data['j_ids'].tolist()))
    ref = dict(zip(g['i_ids'].tolist(), g['j_ids'].tolist()))
    for i in np.nonzero(safe)[0]:
        assert (i in got) == (i in ref_rows), i
        if i in got:
            assert got[i] == ref[i]
    common = [i for i in ref if i in got]
    assert len(common) > 0.98 * len(ref) > 1000
    gi = {i: n for n, i in enumerate(data['i_ids'].tolist())}
    ri = {i: n for n, i in enumerate(g['i_ids'].tolist())}
    a = np.array([gi[i] for i in common])
    b = np.array([ri[i] for i in common])
    np.testing.assert_allclose(data['mconf'][a], g['mconf'][b], atol=5e-3, rtol=0)
    np.testing.assert_allclose(data['mkpts1_f'][a], g['mkpts1_f'][b], atol=2e-2, rtol=0)
    np.testing.assert_allclose(data['expec_f'][a], g['expec_f'][b], atol=5e-3, rtol=0)


# ------------------------------------------------------------------------------------------------ G20
@pytest.mark.timeout(900)
@pytest.mark.parametrize('case', ['unequal', 'short_side', 'masked', 'masked_unequal', 'masked_all_true'])
def test_g20_matcher_forward_offdefault(case):
    """The extended oracle (unequal sizes, padded masks, scales) in fp32 against the reference's own run (G20), at the bars
    test_g7_full_matcher_forward uses: this pins the extension to the reference before a GPU test leans on it."""
    from oracle import model as om
    from tests.util import g20_common, g20_input_conditions, offdefault_inputs
    g = load('g20_matcher_offdefault')
    g20_input_conditions(g, case)
    man = json.load(open(os.path.join(G, 'g8_state_dict_manifest.json')))
    w = om.Weights(synth.synthetic_state_dict({k: tuple(v) for k, v in man.items()}))
    inp = offdefault_inputs(case)
    data = om.matcher_forward(w, far_eval_config(), inp['image0'], inp['image1'], mask0=inp.get('mask0'), mask1=inp.get('mask1'),
                              scale0=inp.get('scale0'), scale1=inp.get('scale1'))
    assert tuple(data['hw0_c']) == tuple(g[f'{case}__hw0_c']) and tuple(data['hw1_c']) == tuple(g[f'{case}__hw1_c'])
    st = int(g[f'{case}__token_stride'])
    for k in ('featmap0', 'featmap1'):
        np.testing.assert_allclose(data[k][:, ::st], g[f'{case}__{k}'], atol=2e-3, rtol=1e-3)
    a, b = g20_common(g, case, (data['b_ids'], data['i_ids'], data['j_ids']), 1e-3, 0.98)
    for k in ('mkpts0_c', 'mkpts1_c'):
        np.testing.assert_allclose(data[k][a], g[f'{case}__{k}'][b], rtol=1e-6, atol=0)
    np.testing.assert_allclose(data['mconf'][a], g[f'{case}__mconf'][b], atol=5e-3, rtol=0)
    np.testing.assert_allclose(data['mkpts1_f'][a], g[f'{case}__mkpts1_f'][b], atol=2e-2, rtol=0)
    np.testing.assert_allclose(data['expec_f'][a], g[f'{case}__expec_f'][b], atol=5e-3, rtol=0)


def test_oracle_padding_border_equals_plain_border_on_full_extents():
    """mask_border_with_padding with full extents is mask_border (coarse_matching.py:8-43)."""
    from oracle import coarse as oc
    rng = np.random.default_rng(3)
    a = rng.random((2, 6, 8, 5, 7)) > 0.3
    b = a.copy()
    oc.mask_border(a, 2, False)
    oc.mask_border_with_padding(b, 2, False, np.ones((2, 6, 8), bool), np.ones((2, 5, 7), bool))
    np.testing.assert_array_equal(a, b)
    m0 = np.zeros((2, 6, 8), bool); m0[0, :5, :7] = True; m0[1, :6, :4] = True
    m1 = np.zeros((2, 5, 7), bool); m1[0, :3, :7] = True; m1[1, :5, :6] = True
    np.testing.assert_array_equal(oc.valid_extents(m0, m1), [[5, 7, 3, 7], [6, 4, 5, 6]])


# ------------------------------------------------------------------------------------------------ G11
@pytest.mark.timeout(900)
def test_g11_matcher_forward_544x720():
    """The oracle's matcher at BASELINE configs[4]'s resolution (coarse 68x90, L = S = 6120) against the reference's run."""
    from oracle import model as om
    g = load('g11_matcher_544x720')
    man = json.load(open(os.path.join(G, 'g8_state_dict_manifest.json')))
    w = om.Weights(synth.synthetic_state_dict({k: tuple(v) for k, v in man.items()}))
    im0, im1 = synth.synth_image_pair(1, seed=5, hw=(544, 720))
    data = om.matcher_forward(w, far_eval_config(), im0, im1)
    assert data['featmap0'].shape == (1, 6120, 256)
    np.testing.assert_allclose(data['featmap0'][0, ::97], g['featmap0_sample'], atol=2e-3, rtol=1e-3)
    safe = (np.abs(g['rowmax'] - 0.2) > 1e-3) & (g['rowgap'] > 1e-3)
    got = dict(zip(data['i_ids'].tolist(), data['j_ids'].tolist()))
    ref = dict(zip(g['i_ids'].tolist(), g['j_ids'].tolist()))
    for i in np.nonzero(safe)[0]:
        assert (i in got) == (i in ref), i
        if i in got:
            assert got[i] == ref[i]
    common = [i for i in ref if i in got]
    assert len(common) > 0.98 * len(ref) > 2000
    gi = {i: n for n, i in enumerate(data['i_ids'].tolist())}
    ri = {i: n for n, i in enumerate(g['i_ids'].tolist())}
    a = np.array([gi[i] for i in common])
    b = np.array([ri[i] for i in common])
    np.testing.assert_allclose(data['mconf'][a], g['mconf'][b], atol=5e-3, rtol=0)
    np.testing.assert_allclose(data['mkpts1_f'][a], g['mkpts1_f'][b], atol=2e-2, rtol=0)


# ------------------------------------------------------------------------------------------------ G12
def g12_expectations(tag, got_valid, got_count, got_score, got_best, got_wq, got_counts3, got_mask, g):
    """Shared by the oracle (CPU) and kernel (GPU) tests against the reference's whole RANSAC loop (G12).
    The reference ran in float32 (torch.linalg.svd of a 9x9 Gram matrix per hypothesis: the winning E itself is
    0.9 % off its float64 value on the prior case), the oracle / kernel in float64; measured agreement is quoted next
    to each bar.  What the LAPACK sign freedom decides in the reference (which two of the four (R, t) candidates enter
    the prior score) is excluded by construction: scores are compared on the models
    whose prior term agrees, the selected model on all."""
    from oracle import solver as osv
    keep = g[f'{tag}_keep']
    np.testing.assert_array_equal(got_valid, keep)                       # remove_bad_models :303-308 (measured: all 512)
    assert got_best == int(g[f'{tag}_best'])                              # argmax of count + prior score :279-281
    cnt, rc = got_count[keep], g[f'{tag}_count']
    assert (cnt == rc).mean() > 0.93                                      # measured 0.957 / 0.959
    assert (np.abs(cnt - rc) <= 2).mean() > 0.97
    if tag == 'p':
        ps, rps = got_score[keep] - cnt, g['p_prior_score']
        rel = np.abs(ps - rps) / np.maximum(np.abs(rps), 1e-6)
        assert np.median(rel) < 1e-3 and (rel < 1e-3).mean() > 0.6        # measured 2.4e-5 / 0.69 (rest: sign convention)
        same = rel < 1e-3
        d = np.abs(got_score[keep][same] - g['p_score'][same])
        assert (d <= 2.01).all() and np.median(d) < 1e-3
        wq = osv.quantize_weights(g['p_bias_weight'])                     # bias weights :358-371
        assert np.abs(wq.astype(np.int64) - got_wq.astype(np.int64)).max() <= 1 and (wq == got_wq).mean() > 0.99
    else:
        assert np.median(np.abs(got_score[keep] - g['n_score'])) == 0
    # the three inlier sets of the winning model :284-287 (ours after cheirality, which can only remove)
    na, ti, ul = got_counts3
    ref3 = (int(g[f'{tag}_inliers'].sum()), int(g[f'{tag}_tight'].sum()), int(g[f'{tag}_ultra'].sum()))
    assert abs(na - ref3[0]) <= 0.03 * ref3[0] and abs(ti - ref3[1]) <= 4 and abs(ul - ref3[2]) <= 3, ((na, ti, ul), ref3)
    sym = int((got_mask ^ g[f'{tag}_inliers']).sum())
    assert sym <= 0.02 * got_mask.size, sym                               # measured 8 / 500 and 1 / 500
    # off the decision margin (the reference's own error of the winning model outside [thr / 3, 3 thr]; measured
    # disagreements lie within [0.73, 1.84] thr) the masks must agree exactly: cheirality removed nothing there
    eb = g[f'{tag}_err_best']
    safe = (eb < 1e-7) | (eb > 9e-7)
    np.testing.assert_array_equal(got_mask[safe], g[f'{tag}_inliers'][safe])


@pytest.mark.parametrize('tag,solver', [('p', 'prior_ransac'), ('n', 'prior_ransac_noprior')])
def test_g12_whole_ransac_loop(tag, solver):
    """oracle.solver.estimate_pose on the committed sample indices against the reference's own RANSAC.forward
    (ransac.py:340-442) run on the same indices (tools/make_goldens.py:g12_ransac_loop)."""
    from oracle import solver as osv
    g = load('g12_ransac_loop')
    prior = g['p_prior'] if tag == 'p' else None
    pcl = g['p_pcl'] if tag == 'p' else None
    ret, na, ti, ul, dbg = osv.estimate_pose(g[f'{tag}_kpts0'], g[f'{tag}_kpts1'], g[f'{tag}_K'], g[f'{tag}_K'], 0.5,
                                             solver=solver, priorRT=prior, pcl=pcl,
                                             samples=g[f'{tag}_samples'].astype(np.int32))
    R, t, mask, E = ret
    g12_expectations(tag, dbg['valid'], dbg['count'], dbg['score'], dbg['best'], dbg['wq'], (na, ti, ul), mask, g)
    assert np.abs(E - g[f'{tag}_E']).max() / np.abs(E).max() < 2e-2      # measured 9.1e-3 / 7.9e-5 (float32 reference)
    assert np.linalg.norm(R - g[f'{tag}_R_gt']) < 0.03


# ------------------------------------------------------------------------------------------------ G17
def _essential_residual(E):
    """max |2 E E^T E - tr(E E^T) E| and |det E|: zero exactly for an essential matrix (the ten cubic constraints)."""
    EEt = E @ np.swapaxes(E, -1, -2)
    c = np.abs(2 * EEt @ E - np.trace(EEt, axis1=-2, axis2=-1)[..., None, None] * E).max((-1, -2))
    return np.maximum(c, np.abs(np.linalg.det(E)))


def _model_dist(A, B):
    """(n, a, 3, 3) x (n, b, 3, 3) unit-norm models -> (n, a, b) max-abs distance up to sign."""
    return np.minimum(np.abs(A[:, :, None] - B[:, None]).max((-1, -2)), np.abs(A[:, :, None] + B[:, None]).max((-1, -2)))


def g17_model_agreement(kind, E, valid, g, tol=1e-6, drop_small_diagonal=False):
    """Shared by the oracle (CPU) and kernel (GPU) tests: five-point models of committed samples against the reference's own
    run_5point_our_kornia (cv_geometry.py:861-1043) in float64.  The reference returns ten models per sample -- the real parts
    of ALL ten roots (:994) --, the oracle / kernel the real roots only (documented deviation); so the comparison is set-wise
    on the models that ARE essential matrices (cubic residual < 1e-10).  On well-conditioned samples (every model of both
    sides either an essential matrix to 1e-10 or clearly not one, models of a sample > 0.05 apart: no near-double root) the
    two sets must agree one to one within 1e-6; near-double roots and coplanar samples whose degree-10 polynomial is
    ill-conditioned lose digits on BOTH sides (whichever side has the larger residual is the one that is off), so over all
    samples the bar is the fraction of models reproduced.  Returns the measured numbers.
    drop_small_diagonal: the kernel applies remove_bad_models (ransac.py:303-308: min |diagonal| > 1e-4) where it forms the models;
    the same filter is then applied to the reference's."""
    ref = g[f'{kind}_models64']
    n = len(ref)
    cr = _essential_residual(ref)
    co = np.where(valid, _essential_residual(E), 0.0)
    d = _model_dist(E, ref)                                            # (n, 10, 10)
    doo = _model_dist(E, E)
    doo = np.where(valid[:, :, None] & valid[:, None, :] & ~np.eye(10, dtype=bool)[None], doo, np.inf)
    well = (co.max(1) < 1e-10) & ((cr < 1e-10) | (cr > 1e-6)).all(1) & (doo.min((1, 2)) > 0.05)
    realref = cr < 1e-10
    if drop_small_diagonal:
        realref &= np.abs(np.stack([ref[..., 0, 0], ref[..., 1, 1], ref[..., 2, 2]], -1)).min(-1) > 2e-4
    o2r = np.where(valid, d.min(2), 0.0)                               # every model of ours -> nearest reference model
    r2o = np.where(realref, np.where(valid[:, :, None], d, np.inf).min(1), 0.0)      # every reference essential matrix -> ours
    assert (o2r[well] < tol).all() and (r2o[well] < tol).all(), (kind, o2r[well].max(), r2o[well].max())
    if not drop_small_diagonal:
        np.testing.assert_array_equal(valid.sum(1)[well], realref.sum(1)[well])
    frac = float((np.where(valid, d.min(2), np.inf) < tol).sum() / max(valid.sum(), 1))
    return {'samples': n, 'well': int(well.sum()), 'worst_well': float(max(o2r[well].max(), r2o[well].max())), 'models': int(valid.sum()),
            'frac_1e-6': frac}


G17_BARS = {'general': (30, 0.97), 'two_planes': (10, 0.93), 'plane': (5, 0.80)}       # (well-conditioned samples, fraction within 1e-6)


def test_g17_five_point_models_match_the_reference_solver():
    """oracle/fivepoint.py against the reference's torch Nister solver on committed samples (golden G17a).  Measured: general
    32 / 40 well-conditioned samples, worst 2.9e-10, 176 / 178 models within 1e-6; two planes 12 / 20, 1.4e-10, 88 / 92;
    coplanar 6 / 20, 1.5e-7, 84 / 98."""
    from oracle import fivepoint as fp
    g = load('g17_fivepoint')
    for kind, (min_well, min_frac) in G17_BARS.items():
        E, valid = fp.five_point(g[f'{kind}_p1'], g[f'{kind}_p2'])
        m = g17_model_agreement(kind, E, valid, g)
        print(f'[g17] {kind}: {m}')
        assert m['well'] >= min_well and m['frac_1e-6'] >= min_frac, m
        # the truth is among the reference's models too (the fixture is what it claims to be)
        dt = _model_dist(g[f'{kind}_models64'], g[f'{kind}_E_true'][:, None])[..., 0].min(1)
        assert (dt < 1e-6).mean() >= 0.9


def g17_loop_expectations(tag, best, valid, count, counts3, mask, E, g):
    """The five-point loop against the reference's RANSAC(model_type='essential').forward (ransac.py:146-150, :340-442) on
    committed samples (golden G17b; the reference in float32, ours in float64).  Models are numbered 10 s + k on both sides
    (k: root order, which differs), so: the same winning SAMPLE, the winning model itself within 5e-4 (measured 1.1e-4 /
    2.1e-5), the inlier sets equal off the decision margin and within 2 % overall (measured 4 and 1 of 400), the three
    counts within 3 % / 4 / 4."""
    assert best // 10 == int(g[f'{tag}_best']) // 10, (best, int(g[f'{tag}_best']))
    Er = g[f'{tag}_E'].astype(np.float64)
    Er, En = Er / np.linalg.norm(Er), E / np.linalg.norm(E)
    dE = min(np.abs(En - Er).max(), np.abs(En + Er).max())
    assert dE < 5e-4, dE
    ref3 = (int(g[f'{tag}_inliers'].sum()), int(g[f'{tag}_tight'].sum()), int(g[f'{tag}_ultra'].sum()))
    na, ti, ul = counts3
    assert abs(na - ref3[0]) <= 0.03 * ref3[0] and abs(ti - ref3[1]) <= 4 and abs(ul - ref3[2]) <= 4, (counts3, ref3)
    sym = int((mask ^ g[f'{tag}_inliers'].astype(bool)).sum())
    assert sym <= 0.02 * mask.size, sym
    eb = g[f'{tag}_err_best']
    safe = (eb < 1e-7) | (eb > 9e-7)
    refm = g[f'{tag}_inliers'].astype(bool)
    # off the decision margin: nothing of ours outside the reference's set, and nothing missing but what the cheirality test
    # removed afterwards (ours is the mask after recoverPose, metrics.py:164-165; the reference's is RANSAC's own)
    removed = int(count[best]) - int(mask.sum())
    assert not (mask & ~refm)[safe].any() and int((refm & ~mask)[safe].sum()) <= removed, (removed, int((refm & ~mask)[safe].sum()))
    # per sample, the best inlier count over its models: float32 five-point models are individually much less accurate than
    # float64 ones (the reference's own float32 / float64 runs of G17a differ more than this), so this is a sanity bar only
    keep = g[f'{tag}_keep']
    cnt = np.zeros(len(keep), np.int64)
    cnt[keep] = g[f'{tag}_count']
    rc = cnt.reshape(-1, 10).max(1)
    oc = np.where(valid, count, 0).reshape(-1, 10).max(1)
    assert (np.abs(rc - oc) <= 2).mean() > 0.7                             # measured 0.82 / 0.86
    return dE, sym


@pytest.mark.parametrize('tag,solver', [('p', 'prior_ransac'), ('n', 'prior_ransac_noprior')])
def test_g17_five_point_ransac_loop(tag, solver):
    from oracle import solver as osv
    g = load('g17_fivepoint')
    prior = g['p_prior'] if tag == 'p' else None
    pcl = g['p_pcl'] if tag == 'p' else None
    ret, na, ti, ul, dbg = osv.estimate_pose(g[f'{tag}_kpts0'], g[f'{tag}_kpts1'], g[f'{tag}_K'], g[f'{tag}_K'], 0.5, solver=solver,
                                             priorRT=prior, pcl=pcl, samples=g[f'{tag}_samples'].astype(np.int32))
    R, t, mask, E = ret
    dE, sym = g17_loop_expectations(tag, dbg['best'], dbg['valid'], dbg['count'], (na, ti, ul), mask, E, g)
    print(f'[g17 loop] {tag}: winning model {dE:.2e} from the reference\'s, {sym} of {mask.size} mask entries differ')
    assert np.linalg.norm(R - g[f'{tag}_R_gt']) < 0.05            # sanity only (96 five-point samples on 0.3 px noise: measured 0.034)


# ------------------------------------------------------------------------------------------------ G8
def test_g8_state_dict_manifest_matches_reference():
    from far_amd.loftr import LoFTR
    man = json.load(open(os.path.join(G, 'g8_state_dict_manifest.json')))
    m = LoFTR(far_eval_config())
    sd = m.state_dict()
    assert list(sd.keys()) == list(man.keys())          # same names, same order
    for k, v in sd.items():
        assert list(v.shape) == man[k], k
    assert sum(p.numel() for p in m.parameters()) == 51092731
    # checkpoints are stored under 'matcher.' (lightning_loftr.py:58-75): the prefix strip must work
    m.load_state_dict({'matcher.' + k: v for k, v in sd.items()})


# ------------------------------------------------------------------------------------------------ G9
def test_g9_pose_metrics_oracle_and_product():
    from far_amd import metrics as fm
    from oracle import metrics as omx
    g = load('g9_metrics')
    for b in range(len(g['T'])):
        np.testing.assert_allclose(omx.relative_pose_error(g['T'][b], g['R'][b], g['t'][b]), g['errs'][b], rtol=1e-12, atol=1e-10)
    te, Re, ta = fm.relative_pose_error_batch(torch.from_numpy(g['T']), torch.from_numpy(g['R']), torch.from_numpy(g['t']))
    np.testing.assert_allclose(np.stack([te.numpy(), Re.numpy(), ta.numpy()], 1), g['errs'], rtol=1e-7, atol=2e-5)   # acos near 0 deg amplifies 1-ulp differences of the trace
    auc = fm.error_auc(np.maximum(g['errs'][:, 0], g['errs'][:, 1]))
    np.testing.assert_allclose([auc['auc@5'], auc['auc@10'], auc['auc@20']], g['auc'], rtol=1e-12)
    agg = fm.aggregate_pose_metrics(g['errs'][:, 0], g['errs'][:, 1], g['errs'][:, 2], np.ones(len(g['T'])))
    assert agg['dset size'] == len(g['T']) and agg['rot median err'] == np.round(np.median(g['errs'][:, 1]), 2)


# ------------------------------------------------------------------------------------------------ G13
def test_g13_mapfree_corr_volume_warp_oracle():
    """oracle.mapfree.corr_volume_warp against the reference's CorrelationVolumeWarping (golden G13)."""
    from oracle import mapfree as omf
    g = load('g13_mapfree_cvw')
    agg = omf.corr_volume_warp(g['s_vol0'], g['s_vol1'])
    np.testing.assert_allclose(agg, g['s_agg'], rtol=2e-5, atol=2e-6)
    B, H, W = (int(v) for v in g['f_shape'])
    rng = np.random.default_rng(33)                      # the generator's draw order: small case first, then the full grid
    for (b, h, w, amp) in ((2, 12, 9, 0.6),):
        rng.standard_normal((b, 32, h, w)); rng.standard_normal((b, 32, h, w))
    amp = float(g['f_amp'])
    v0 = (amp * rng.standard_normal((B, 32, H, W))).astype(np.float32)
    v1 = (amp * rng.standard_normal((B, 32, H, W))).astype(np.float32)
    v1[:, :, : H // 2] = 2.0 * v0[:, :, : H // 2][:, :, ::-1] + 0.3 * v1[:, :, : H // 2]
    agg = omf.corr_volume_warp(v0, v1)
    np.testing.assert_allclose(agg[:, :, ::7, ::5], g['f_agg_sample'], rtol=5e-5, atol=5e-6)
    np.testing.assert_allclose(agg[:, 66], g['f_max_score'], rtol=5e-5, atol=1e-7)
    np.testing.assert_allclose(agg.sum((2, 3)), g['f_agg_sum'], rtol=1e-5, atol=1e-3)


# ------------------------------------------------------------------------------------------------ G14
def test_g14_spvs_coarse_matches_reference():
    """far_amd.supervision.spvs_coarse (batched, no conf_matrix_gt) against the reference's spvs_coarse run on the same
    synthetic planar scenes (golden G14): identical ground-truth match ids, warped points, and -- with dense_gt -- the
    same 0/1 matrix."""
    from far_amd.supervision import spvs_coarse
    from tests import util as mod
    d0, d1, T01, T10, K = mod.spvs_scene()
    g = load('g14_spvs_coarse')
    N = len(d0)
    data = {'image0': torch.zeros(N, 1, 480, 640), 'image1': torch.zeros(N, 1, 480, 640), 'depth0': torch.from_numpy(d0),
            'depth1': torch.from_numpy(d1), 'T_0to1': torch.from_numpy(T01), 'T_1to0': torch.from_numpy(T10),
            'K0': torch.from_numpy(K), 'K1': torch.from_numpy(K), 'dataset_name': ['mp3d']}
    spvs_coarse(data, {'LOFTR': {'RESOLUTION': (8, 2)}}, dense_gt=True)
    for k, gk in (('spv_b_ids', 'b_ids'), ('spv_i_ids', 'i_ids'), ('spv_j_ids', 'j_ids')):
        np.testing.assert_array_equal(data[k].numpy(), g[gk])
    assert len(g['b_ids']) > 5000
    np.testing.assert_allclose(data['spv_w_pt0_i'][:, ::37].numpy(), g['w_pt0_i_sample'], rtol=1e-5, atol=1e-3)
    np.testing.assert_array_equal(data['spv_pt1_i'][:, ::37].numpy(), g['pt1_i_sample'])
    assert float(data['conf_matrix_gt'].sum()) == float(g['gt_sum'])
    np.testing.assert_array_equal(data['conf_matrix_gt'].sum(2).numpy().astype(np.int8), g['gt_rowsum'])
    d2 = dict(data)
    d2.pop('conf_matrix_gt')
    spvs_coarse(d2, 8)
    assert 'conf_matrix_gt' not in d2 and torch.equal(d2['spv_j_ids'], data['spv_j_ids'])


# ------------------------------------------------------------------------------------------------ G15
def test_g15_losses_and_fine_supervision_match_reference():
    """far_amd.losses.LoFTRLoss (coarse focal on the ground-truth positions + fine l2-with-std + 6D pose L1/L2) and
    far_amd.supervision.spvs_fine against the reference's LoFTRLoss.forward / spvs_fine on the same tensors (golden G15).
    The coarse term is evaluated three ways: gathered from conf_matrix_gt, from spv ids, and from data['conf_pos'] (the form
    the GPU training path provides) -- all must give the reference's number."""
    from far_amd.config import far_train_config, RunCfg
    from far_amd.losses import LoFTRLoss
    from far_amd.supervision import spvs_fine, compute_supervision_fine
    from tests import util as mod
    x = mod.loss_inputs()
    g = load('g15_losses')
    b, i, j = np.nonzero(x['gt'])
    for tag, l1, shift in (('l1', True, 0.0), ('l2', False, 0.0), ('nocorrect', True, 5.0)):
        cfg = far_train_config()
        cfg['loftr']['loss']['use_l1_rt_loss'] = l1
        lf = LoFTRLoss(cfg).train()
        common = {'expec_f': torch.from_numpy(x['expec_f']), 'expec_f_gt': torch.from_numpy(x['expec_f_gt'] + np.float32(shift)),
                  'expec_rt': torch.from_numpy(x['expec_rt']), 'T_0to1': torch.from_numpy(x['T']),
                  'num_correspondences_after_ransac': 0, 'num_correspondences_before_ransac': 0}
        conf = torch.from_numpy(x['conf'])
        ids = {'spv_b_ids': torch.from_numpy(b), 'spv_i_ids': torch.from_numpy(i), 'spv_j_ids': torch.from_numpy(j)}
        variants = [dict(common, conf_matrix=conf, conf_matrix_gt=torch.from_numpy(x['gt'])),
                    dict(common, conf_matrix=conf, **ids),
                    dict(common, conf_matrix=None, conf_pos=conf[ids['spv_b_ids'], ids['spv_i_ids'], ids['spv_j_ids']], **ids)]
        for data in variants:
            lf(data)
            np.testing.assert_allclose(data['loss'].numpy(), g[f'loss_{tag}'], rtol=2e-6)
            for k in ('loss_c', 'loss_f', 'loss_rot', 'loss_tr'):
                np.testing.assert_allclose(data['loss_scalars'][k].item(), g[f'{k}_{tag}'], rtol=2e-6, atol=1e-9, err_msg=f'{k} {tag}')
    # no ground-truth coarse match at all (loftr_loss.py:65-70): the dummy (0, 0, 0) entry that spvs_coarse leaves
    # (supervision.py:122-128) carries zero weight -- dense form, far_amd's sparse form with spv_gt_count, and the bare
    # dummy ids (a lone entry at cell 0 can only be the dummy)
    lf = LoFTRLoss(far_train_config()).train()
    zero = torch.zeros(1, dtype=torch.int64)
    dummy = {'spv_b_ids': zero, 'spv_i_ids': zero, 'spv_j_ids': zero}
    conf_g = conf.clone().requires_grad_(True)
    forms = [dict(common, conf_matrix=conf, conf_matrix_gt=torch.zeros_like(conf)),
             dict(common, conf_matrix=None, conf_pos=conf_g[zero, zero, zero], spv_gt_count=0, **dummy),
             dict(common, conf_matrix=conf, **dummy)]
    for data in forms:
        data['expec_f_gt'] = torch.from_numpy(x['expec_f_gt'])
        lf(data)
        assert float(data['loss_scalars']['loss_c']) == float(g['loss_c_nogt']) == 0.0
        np.testing.assert_allclose(data['loss'].detach().numpy(), g['loss_nogt'], rtol=2e-6)
    forms[1]['loss'].backward()
    assert float(conf_g.grad.abs().max()) == 0.0              # and no gradient flows into the dummy position
    # eval mode without a correct coarse match: no fine term, scalar 1 (loftr_loss.py:171-172, :322-324)
    lf = LoFTRLoss(far_train_config()).eval()
    data = dict(variants[1], expec_f_gt=torch.from_numpy(x['expec_f_gt'] + np.float32(5.0)))
    lf(data)
    assert float(data['loss_scalars']['loss_f']) == 1.0
    data = {'spv_w_pt0_i': torch.from_numpy(x['w_pt0']), 'spv_pt1_i': torch.from_numpy(x['pt1']), 'b_ids': torch.from_numpy(x['b_ids']),
            'i_ids': torch.from_numpy(x['i_ids']), 'j_ids': torch.from_numpy(x['j_ids']), 'dataset_name': ['mp3d']}
    spvs_fine(data, {'LOFTR': {'RESOLUTION': (8, 2), 'FINE_WINDOW_SIZE': 5}})
    np.testing.assert_array_equal(data['expec_f_gt'].numpy(), g['expec_f_gt'])
    d2 = dict(data)
    compute_supervision_fine(d2, RunCfg())               # the config object the pipeline hands over
    np.testing.assert_array_equal(d2['expec_f_gt'].numpy(), g['expec_f_gt'])


# ------------------------------------------------------------------------------------------------ G16
def _g16_stub(x):
    calls = []

    def stub(k0, k1, K0, K1, thr, conf=None, translation_scale=None, solver=None, priorRT=None):
        b = len(calls)
        calls.append(len(k0))
        if x['fit_ok'][b] == 0:
            return None, 0, 0, 0
        mask = x['fit_mask'][x['m_bids'] == b] > 0
        return (torch.from_numpy(x['fit_R'][b]), torch.from_numpy(x['fit_t'][b]), mask, torch.eye(3)), torch.tensor(int(mask.sum())), 0, 0
    return stub


def test_g16_eval_metrics_match_reference():
    """The evaluation step after the path (lightning_loftr.py:227-264): far_amd.metrics.compute_symmetrical_epipolar_errors,
    compute_pose_errors (head branch, solver branch with committed fits incl. a failed one, no-match branch),
    epidist_prec and aggregate_metrics -- and the float64 oracle -- against the reference's own functions (golden G16)."""
    from far_amd import metrics as fm
    from far_amd.config import RunCfg
    from oracle import metrics as om
    from tests.util import eval_batch, eval_metrics_table
    g = load('g16_eval_metrics')
    x = eval_batch()
    B = len(x['T'])
    t = torch.from_numpy
    # epipolar errors: fp32 in the reference; the oracle is float64
    ref64 = om.compute_symmetrical_epipolar_errors(x['T'].astype(np.float64), x['m_bids'], x['mk0'].astype(np.float64),
                                                   x['mk1'].astype(np.float64), x['K0'].astype(np.float64), x['K1'].astype(np.float64))
    np.testing.assert_allclose(ref64, g['epi_errs'], rtol=2e-4, atol=1e-9)
    data = {'T_0to1': t(x['T']), 'K0': t(x['K0']), 'K1': t(x['K1']), 'm_bids': t(x['m_bids']), 'mkpts0_f': t(x['mk0']), 'mkpts1_f': t(x['mk1'])}
    fm.compute_symmetrical_epipolar_errors(data)
    assert data['epi_errs'].shape == (len(x['m_bids']),)
    np.testing.assert_allclose(data['epi_errs'].numpy(), g['epi_errs'], rtol=2e-4, atol=1e-9)
    d64 = {k: (v.double() if v.is_floating_point() else v) for k, v in data.items() if k != 'epi_errs'}
    fm.compute_symmetrical_epipolar_errors(d64)
    np.testing.assert_allclose(d64['epi_errs'].numpy(), ref64, rtol=1e-10)
    # an unsorted m_bids (training order) gives the reference's pair-after-pair concatenation
    perm = np.random.default_rng(0).permutation(len(x['m_bids']))
    dp = dict(d64, m_bids=d64['m_bids'][perm], mkpts0_f=d64['mkpts0_f'][perm], mkpts1_f=d64['mkpts1_f'][perm])
    fm.compute_symmetrical_epipolar_errors(dp)
    np.testing.assert_allclose(np.sort(dp['epi_errs'].numpy()), np.sort(ref64), rtol=1e-10)
    for b in range(B):
        np.testing.assert_allclose(np.sort(dp['epi_errs'].numpy()[np.sort(x['m_bids']) == b]), np.sort(ref64[x['m_bids'] == b]), rtol=1e-10)
    cfg = RunCfg('prior_ransac')
    # (1) head branch: per pair (the reference's batch size 1) and all pairs in one call
    d = {'T_0to1': t(x['T']), 'K0': t(x['K0']), 'K1': t(x['K1']), 'regressed_rt': t(x['regressed_rt'])}
    fm.compute_pose_errors(d, cfg)
    got = np.array([d['R_errs'], d['t_errs'], d['t_errs_abs'], d['successful_fits']]).T
    np.testing.assert_allclose(got, g['head_errs'], rtol=1e-5, atol=2e-3)       # the reference evaluates acos in fp32
    o = om.compute_pose_errors(x['T'], regressed_rt=x['regressed_rt'])
    np.testing.assert_allclose(got[:, :3], np.array([o['R_errs'], o['t_errs'], o['t_errs_abs']]).T, rtol=1e-5, atol=2e-4)
    np.testing.assert_allclose(d['pred_R'], g['head_pred_R'], atol=1e-6)
    np.testing.assert_allclose(d['pred_t'], g['head_pred_t'], atol=1e-6)
    assert d['inliers'] == [0] * B and isinstance(d['pred_R'], np.ndarray)
    # (2) solver branch with the committed fits the generator's stub returned
    d = dict(data, translation_scale=None, priorRT=x['priorRT'])
    fm.compute_pose_errors(d, cfg, estimate_pose_fn=_g16_stub(x))
    got = np.array([d['R_errs'], d['t_errs'], d['t_errs_abs'], d['successful_fits']], np.float64).T
    # (angles: the reference takes the norm of its float32 ground-truth translation in float32 (metrics.py:20); acos turns
    # that 6e-8 into up to 0.02 degrees near zero error -- pair 0's fit IS the truth and reads 0.015 there, 9e-7 here)
    np.testing.assert_allclose(got, g['fit_errs'], rtol=1e-6, atol=2e-2)
    np.testing.assert_allclose(got[:, 2:], g['fit_errs'][:, 2:], rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal([np.asarray(i).sum() for i in d['inliers']], g['fit_inlier_sums'])
    np.testing.assert_array_equal([len(i) for i in d['inliers']], g['fit_inlier_lens'])
    np.testing.assert_array_equal(d['num_correspondences_before_ransac'], g['fit_before'])
    np.testing.assert_array_equal([int(v) for v in d['num_correspondences_after_ransac']], g['fit_after'])
    np.testing.assert_allclose(d['pred_R'], g['fit_pred_R'], atol=1e-12)
    np.testing.assert_allclose(d['pred_t'], g['fit_pred_t'], atol=1e-12)
    assert bool(g['stub_saw_prior'].all())
    fits = [None if not x['fit_ok'][b] else (x['fit_R'][b], x['fit_t'][b], None) for b in range(B)]
    o = om.compute_pose_errors(x['T'], fits=fits)
    np.testing.assert_allclose(np.array([o['R_errs'], o['t_errs'], o['t_errs_abs'], o['successful_fits']]).T, g['fit_errs'], rtol=1e-6, atol=2e-2)
    np.testing.assert_allclose(np.array([o['R_errs'], o['t_errs'], o['t_errs_abs'], o['successful_fits']]).T, got, rtol=1e-9, atol=1e-5)
    # (3) nothing to fit on
    d = {'T_0to1': t(x['T'][:1]), 'K0': t(x['K0'][:1]), 'K1': t(x['K1'][:1])}
    fm.compute_pose_errors(d, cfg)
    np.testing.assert_allclose([d['R_errs'][0], d['t_errs'][0], d['t_errs_abs'][0], d['successful_fits'][0]], g['none_errs'], rtol=1e-6, atol=2e-2)
    # (4) aggregation
    m = eval_metrics_table()
    for agg in (fm.aggregate_metrics(dict(m), 5e-4), om.aggregate_metrics(dict(m), 5e-4)):
        assert list(agg.keys()) == g['agg_keys'].tolist()
        np.testing.assert_allclose([float(v) for v in agg.values()], g['agg_vals'], rtol=1e-12)
    pr = fm.epidist_prec(m['epi_errs'], [1e-4, 5e-4, 1e-3], True)
    assert list(pr.keys()) == g['prec_keys'].tolist()
    np.testing.assert_allclose(list(pr.values()), g['prec_vals'], rtol=1e-12)
    np.testing.assert_allclose(list(om.epidist_prec(m['epi_errs'], [1e-4, 5e-4, 1e-3]).values()), g['prec_vals'], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ G19
def test_g19_vit_shape_cross_attention_oracle():
    """The 8-Point-ViT shape of K2 (N = 576, 3 heads x 64, positional index k*w + j: SURVEY.md section 2.5) -- golden produced by
    the reference's own vision_transformer.CrossBlock (tools/make_golden_vit.py): the oracle's positional tables bit for bit, its
    CrossAttention within fp32 round-off, and the product's table builder (host code, no GPU needed)."""
    import torch
    from far_amd.loftr.transformer import CrossBlock, positional_table_vit
    from oracle import head as oh
    from oracle import model as om
    from tests.util import VIT_INTRINSICS, vit_seeded_fill
    g = load('g19_vit_crossblock')
    assert tuple(np.round(g['intrinsics'], 4)) == tuple(np.round(np.float32(VIT_INTRINSICS), 4))
    for intr, key in ((VIT_INTRINSICS, 'pos_intr'), (None, 'pos_none')):
        np.testing.assert_array_equal(oh.positional_encodings_vit(24, 24, intr), g[key])
        np.testing.assert_array_equal(positional_table_vit(24, 24, intr).numpy(), g[key])
    assert not np.array_equal(g['pos_intr'][:, 3].reshape(24, 24), g['pos_intr'][:, 3].reshape(24, 24).T)      # k*w + j is not j*w + k
    blk = CrossBlock(192, 3, qkv_bias=True, pos=positional_table_vit(24, 24, VIT_INTRINSICS)).eval()
    x = vit_seeded_fill(blk, seed=19)
    w = om.Weights({k: v.detach() for k, v in blk.state_dict().items()})
    ln = lambda a: torch.nn.functional.layer_norm(a, (192,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps).detach().numpy()
    fa, fb = om.cross_attention(w, ln(x[0:1]), ln(x[1:2]), g['pos_intr'], num_heads=3, prefix='cross_attn.')
    sc = np.abs(g['xattn_a']).max()
    assert np.abs(fa - g['xattn_a']).max() < 2e-5 * sc and np.abs(fb - g['xattn_b']).max() < 2e-5 * sc
    with pytest.raises(Exception, match='no CPU fallback'):    # the product module has no CPU inference path: loud, not a fallback
        with torch.no_grad():
            blk(x)
