"""The optimal-transport coarse matcher (match_type 'sinkhorn', far_coarse_match_sinkhorn_f16s) on the GPU against a float64
restatement of its definition (sinkhorn_f16s.hip).  The reference cannot run this branch (it imports a
superglue.py its tree does not have), so nothing here is pinned to a reference run: the oracle below is the definition in
numpy float64, and the selection is oracle.coarse.get_coarse_match on its conf_matrix.

Bars: ids bit-exact; mconf and conf_matrix within 2e-5, log_u / log_v within 5e-5 of float64.  These are derived, not measured;
where the fp32 restatement (what the reference computes) deviates more on a test's inputs, its deviation is the bar (printed)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 256
THR, BORDER = 0.2, 2
ATOL_CONF, ATOL_POT = 2e-5, 5e-5


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def oracle(f0, f1, alpha, T, m0=None, m1=None, prefilter=False, dt=np.float64):
    """SuperGlue's log-domain Sinkhorn with a dustbin row and column, as LoFTR's coarse_matching.py:120-139 applies it.
    -> (assign (N, L+1, S+1) with the prefilter's zeros in its [:, :L, :S] block, u (N, L+1), v (N, S+1))."""
    N, L, _ = f0.shape
    S = f1.shape[1]
    a = f0.astype(dt) / np.sqrt(dt(C))
    b = f1.astype(dt) / np.sqrt(dt(C))
    s = np.einsum('nlc,nsc->nls', a, b)
    if m0 is not None:
        s[~(m0[:, :, None] & m1[:, None, :])] = dt(-1e9)
    Zc = np.full((N, L + 1, S + 1), dt(alpha), dt)
    Zc[:, :L, :S] = s
    del s
    norm = -np.log(dt(L + S))
    lmu = np.full(L + 1, norm, dt)
    lmu[L] = np.log(dt(S)) + norm
    lnu = np.full(S + 1, norm, dt)
    lnu[S] = np.log(dt(L)) + norm
    u = np.zeros((N, L + 1), dt)
    v = np.zeros((N, S + 1), dt)
    for _ in range(T):
        u = lmu - _lse(Zc + v[:, None, :], 2)
        v = lnu - _lse(Zc + u[:, :, None], 1)
    Zc += u[:, :, None]
    Zc += v[:, None, :]
    Zc -= norm
    assign = np.exp(Zc, out=Zc)
    if prefilter:
        rows = assign.argmax(2)[:, :L] == S          # ties -> the first index: a real entry
        cols = assign.argmax(1)[:, :S] == L
        blk = assign[:, :L, :S]
        blk[rows] = 0
        blk[np.broadcast_to(cols[:, None, :], blk.shape)] = 0
    return assign, u, v


def restatement32(f0, f1, alpha, T, m0=None, m1=None, prefilter=False):
    """What the reference computes: the same definition in fp32 torch on the GPU (einsum, logsumexp, exp) -> float64 numpy."""
    N, L, _ = f0.shape
    S = f1.shape[1]
    s = torch.einsum('nlc,nsc->nls', torch.from_numpy(f0).cuda() / C ** .5, torch.from_numpy(f1).cuda() / C ** .5)
    if m0 is not None:
        valid = torch.from_numpy(m0).cuda()[:, :, None] & torch.from_numpy(m1).cuda()[:, None, :]
        s = s.masked_fill(~valid, -1e9)
    a = torch.tensor(float(alpha), device='cuda')
    Zc = torch.cat([torch.cat([s, a.expand(N, L, 1)], 2), a.expand(N, 1, S + 1)], 1)
    norm = -torch.tensor(float(L + S), device='cuda').log()
    lmu = torch.cat([norm.expand(L), torch.tensor(float(S), device='cuda').log()[None] + norm])
    lnu = torch.cat([norm.expand(S), torch.tensor(float(L), device='cuda').log()[None] + norm])
    u = torch.zeros(N, L + 1, device='cuda')
    v = torch.zeros(N, S + 1, device='cuda')
    for _ in range(T):
        u = lmu - torch.logsumexp(Zc + v[:, None, :], 2)
        v = lnu - torch.logsumexp(Zc + u[:, :, None], 1)
    assign = (Zc + u[:, :, None] + v[:, None, :] - norm).exp()
    if prefilter:
        rows = assign.max(2)[1][:, :L] == S
        cols = assign.max(1)[1][:, :S] == L
        blk = assign[:, :L, :S]
        blk[rows[..., None].expand(N, L, S)] = 0
        blk[cols[:, None].expand(N, L, S)] = 0
    return assign.double().cpu().numpy(), u.double().cpu().numpy(), v.double().cpu().numpy()


def _dev(got, ref):
    """max |got - ref| / max(1, |ref|): absolute for probabilities; relative for the entries above 1 (the dustbin corner
    assign[L, S], which holds about as much mass as there are matches, and every entry at T = 0, where nothing is normalised)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


def _abs(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max())


def features(N, L, S, amp=3.75, noise=0.1, seed=0, weak=0.0, weak_scale=0.5, share=1.0):
    """f1 holds a permuted, noisy copy of part of f0 (`share` of min(L, S) rows; `weak` of those only weakly correlated):
    -> f0 (N, L, C), f1 (N, S, C), [(rows of f0, their rows in f1)] per pair."""
    rng = np.random.default_rng(seed)
    f0 = (amp * rng.standard_normal((N, L, C))).astype(np.float32)
    f1 = (amp * rng.standard_normal((N, S, C))).astype(np.float32)
    pairs = []
    for n in range(N):
        k = int(min(L, S) * share)
        src = rng.permutation(L)[:k]
        dst = rng.permutation(S)[:k]
        sc = np.ones(k, np.float32)
        if weak:
            sc[rng.random(k) < weak] = weak_scale
        f1[n, dst] = f0[n, src] * sc[:, None] + np.sqrt(1 - sc[:, None] ** 2) * f1[n, dst]
        pairs.append((src, dst))
    f1 = (f1 + noise * rng.standard_normal(f1.shape)).astype(np.float32)
    return f0, f1, pairs


def _bar(name, got_dev, derived, dev32):
    bar = max(derived, dev32)
    print(f'[{name}] |kernel - float64| = {got_dev:.3e}   bar {bar:.1e} (derived {derived:.0e}, fp32 restatement {dev32:.3e})')
    assert got_dev <= bar, f'{name}: {got_dev:.3e} > {bar:.1e}'


def _run(f0, f1, alpha, T, hw0, hw1, prefilter=False, want_conf=False, masks=None, valid_hw=None, scales=None, thr=THR,
         border=BORDER):
    from far_amd import ops
    bs = torch.tensor(alpha, dtype=torch.float32, device='cuda') if not torch.is_tensor(alpha) else alpha
    m0, m1 = (None, None) if masks is None else (torch.from_numpy(masks[0].astype(np.uint8)).cuda(),
                                                  torch.from_numpy(masks[1].astype(np.uint8)).cuda())
    s0, s1 = (None, None) if scales is None else (torch.from_numpy(scales[0]).cuda(), torch.from_numpy(scales[1]).cuda())
    out = ops.coarse_match_sinkhorn(torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda(), bs, T, thr, border, hw0, hw1, 8.0,
                                    m0, m1, valid_hw, s0, s1, prefilter=prefilter, want_conf=want_conf, want_potentials=True)
    torch.cuda.synchronize()
    return out


def _margin_ok(conf, thr=THR):
    """ids are only well defined away from the selection's discontinuities: margins on the float64 side."""
    from oracle import coarse as oc
    rg, cg, tg = oc.margins(conf, thr)
    sel = conf.max(axis=2) > 0.05
    if sel.any():
        assert rg[sel].min() > 1e-5 and tg[sel].min() > 1e-5, 'test input lacks margin'
    csel = conf.max(axis=1) > 0.05
    if csel.any():
        assert cg[csel].min() > 1e-5, 'test input lacks margin'


def _check(f0, f1, alpha, T, hw0, hw1, prefilter=False, want_conf=False, name='', min_matches=1):
    """Kernel vs oracle: ids bit-exact, mconf / conf_matrix / potentials within their bars.  -> (kernel output, oracle matches)"""
    from oracle import coarse as oc
    L, S = f0.shape[1], f1.shape[1]
    A, u, v = oracle(f0, f1, alpha, T, prefilter=prefilter)
    conf = A[:, :L, :S]
    _margin_ok(conf)
    ref = oc.get_coarse_match(conf, THR, BORDER, hw0, hw1, (hw0[0] * 8, hw0[1] * 8))
    got = _run(f0, f1, alpha, T, hw0, hw1, prefilter=prefilter, want_conf=want_conf)
    assert len(ref['i_ids']) >= min_matches, f'{name}: the input gives {len(ref["i_ids"])} matches'
    for k in ('b_ids', 'i_ids', 'j_ids'):
        assert got[k].dtype == torch.int64
        np.testing.assert_array_equal(got[k].cpu().numpy(), ref[k], err_msg=f'{name} {k}')
    np.testing.assert_array_equal(got['mkpts0_c'].cpu().numpy(), ref['mkpts0_c'])
    np.testing.assert_array_equal(got['mkpts1_c'].cpu().numpy(), ref['mkpts1_c'])
    A32, u32, v32 = restatement32(f0, f1, alpha, T, prefilter=prefilter)
    idx = (ref['b_ids'], ref['i_ids'], ref['j_ids'])
    _bar(f'{name} mconf', _dev(got['mconf'].cpu().numpy(), conf[idx]), ATOL_CONF, _dev(A32[idx], conf[idx]))
    _bar(f'{name} log_u', _abs(got['log_u'].cpu().numpy(), u), ATOL_POT, _abs(u32, u))
    _bar(f'{name} log_v', _abs(got['log_v'].cpu().numpy(), v), ATOL_POT, _abs(v32, v))
    if want_conf:
        _check_conf(name, got, A, A32, L, S, prefilter)
    return got, ref


def _check_conf(name, got, A, A32, L, S, prefilter=False):
    """conf_matrix (the real block) within the conf bar; the dustbin row and column within 2 x the potentials' bar relatively
    (assign = exp(alpha + u + v - norm): its relative error is that of u + v)."""
    cw = got['conf_matrix_with_bin']
    assert cw.shape == (A.shape[0], L + 1, S + 1)
    assert got['conf_matrix'].data_ptr() == cw.data_ptr() and got['conf_matrix'].shape == (A.shape[0], L, S)
    g = cw.cpu().numpy()
    _bar(f'{name} conf_matrix', _dev(g[:, :L, :S], A[:, :L, :S]), ATOL_CONF, _dev(A32[:, :L, :S], A[:, :L, :S]))
    rel = lambda x, y: float((np.abs(np.asarray(x, np.float64) - y) / np.abs(y)).max())
    bins = lambda t: np.concatenate([t[:, :, S].ravel(), t[:, L, :S].ravel()])
    _bar(f'{name} dustbin entries (relative)', rel(bins(g), bins(A)), 2 * ATOL_POT, rel(bins(A32), bins(A)))
    if prefilter:       # the prefilter's zeros are exact zeros
        np.testing.assert_array_equal(g[:, :L, :S][A[:, :L, :S] == 0], 0)


def test_ragged_shapes():
    """L != S in both directions, not multiples of the 128-row block or the 64-column tile."""
    for (hw0, hw1), seed in ((((12, 16), (10, 14)), 1), (((9, 13), (15, 17)), 2)):
        L, S = hw0[0] * hw0[1], hw1[0] * hw1[1]
        f0, f1, _ = features(2, L, S, seed=seed)
        _check(f0, f1, 1.0, 3, hw0, hw1, want_conf=True, name=f'ragged {hw0} {hw1}', min_matches=20)


@pytest.mark.parametrize('hw', [(60, 80), (68, 90)])
def test_bench_and_mapfree_grids(hw):
    """The 640x480 coarse grid (L = S = 4800) and Map-free's 544x720 (68 x 90 = 6120, not a multiple of 128)."""
    L = hw[0] * hw[1]
    f0, f1, _ = features(1, L, L, seed=11, share=0.9)
    got, ref = _check(f0, f1, 1.0, 3, hw, hw, name=f'grid {hw}', min_matches=1000)


def test_batch_of_four_recovers_each_permutation():
    hw = (16, 20)
    L = hw[0] * hw[1]
    f0, f1, pairs = features(4, L, L, seed=5)
    got, ref = _check(f0, f1, 1.0, 3, hw, hw, name='batch 4', min_matches=4 * 100)
    b, i, j = (got[k].cpu().numpy() for k in ('b_ids', 'i_ids', 'j_ids'))
    for n, (src, dst) in enumerate(pairs):
        truth = dict(zip(src.tolist(), dst.tolist()))
        sel = b == n
        assert sel.sum() > 80, n
        assert all(truth[ii] == jj for ii, jj in zip(i[sel].tolist(), j[sel].tolist())), n


def test_no_match_input_goes_to_the_dustbin():
    """Unrelated features: every row's mass goes to the dustbin, no match above thr (with and without the prefilter)."""
    hw = (12, 16)
    L = hw[0] * hw[1]
    f0, f1, _ = features(2, L, L, amp=1.0, seed=8, share=0.0)
    for pf in (False, True):
        got, ref = _check(f0, f1, 1.0, 3, hw, hw, prefilter=pf, want_conf=True, name=f'no match pf={pf}', min_matches=0)
        assert len(ref['i_ids']) == 0 and got['b_ids'].numel() == 0
    A, _, _ = oracle(f0, f1, 1.0, 3)
    assert (A.argmax(2)[:, :L] == L).all()          # every row's largest entry is its dustbin entry


@pytest.mark.parametrize('prefilter, alpha, weak', [(False, 1.0, 0.0), (True, 2.5, 0.4)])
def test_masks_valid_hw_and_scales(prefilter, alpha, weak):
    """mask_c0 / mask_c1 (-1e9 fill of the real block, coarse_matching.py:123-126), mask_border_with_padding (:28-43) and
    scale0 / scale1 (:247-254), the selection restated in torch as tests/test_coarse_gpu.py does.  With the prefilter (and weakly
    correlated rows under a high dustbin score, so that it filters unmasked rows and columns too): masked entries stay out of the
    filters' maxima."""
    rng = np.random.default_rng(9)
    N, hw = 2, (12, 16)
    L = hw[0] * hw[1]
    f0, f1, _ = features(N, L, L, seed=4, weak=weak, weak_scale=0.6)
    m0 = np.zeros((N, hw[0], hw[1]), bool)
    m1 = np.zeros((N, hw[0], hw[1]), bool)
    ext = [(10, 13, 12, 16), (12, 16, 9, 14)]
    for n, (h0, w0, h1, w1) in enumerate(ext):
        m0[n, :h0, :w0] = True
        m1[n, :h1, :w1] = True
    sc0 = rng.uniform(0.8, 1.3, (N, 2)).astype(np.float32)
    sc1 = rng.uniform(0.8, 1.3, (N, 2)).astype(np.float32)
    mm0, mm1 = m0.reshape(N, L), m1.reshape(N, L)
    A, u, v = oracle(f0, f1, alpha, 3, mm0, mm1, prefilter=prefilter)
    if prefilter:
        A0, _, _ = oracle(f0, f1, alpha, 3, mm0, mm1)
        rows = (A0.argmax(2)[:, :L] == L) & mm0
        cols = (A0.argmax(1)[:, :L] == L) & mm1
        print(f'[masks + prefilter] unmasked rows / columns filtered: {int(rows.sum())} / {int(cols.sum())}')
        assert rows.any() and cols.any(), 'the input does not exercise the prefilter'
    conf = torch.from_numpy(A[:, :L, :L].copy())
    _margin_ok(A[:, :L, :L])
    mask = (conf > THR).reshape(N, *hw, *hw).clone()
    bd = BORDER
    mask[:, :bd] = False; mask[:, :, :bd] = False; mask[:, :, :, :bd] = False; mask[:, :, :, :, :bd] = False
    for n, (h0, w0, h1, w1) in enumerate(ext):
        mask[n, h0 - bd:] = False; mask[n, :, w0 - bd:] = False
        mask[n, :, :, h1 - bd:] = False; mask[n, :, :, :, w1 - bd:] = False
    mask = mask.reshape(N, L, L) & (conf == conf.max(2, keepdim=True)[0]) & (conf == conf.max(1, keepdim=True)[0])
    mv, aj = mask.max(2)
    bi, ii = torch.where(mv)
    jj = aj[bi, ii]
    vh = torch.tensor(ext, dtype=torch.int32).cuda()
    got = _run(f0, f1, alpha, 3, hw, hw, prefilter=prefilter, masks=(mm0, mm1), valid_hw=vh, scales=(sc0, sc1), want_conf=True)
    assert len(bi) > 20
    np.testing.assert_array_equal(got['b_ids'].cpu().numpy(), bi.numpy())
    np.testing.assert_array_equal(got['i_ids'].cpu().numpy(), ii.numpy())
    np.testing.assert_array_equal(got['j_ids'].cpu().numpy(), jj.numpy())
    mk0 = torch.stack([ii % hw[1], ii // hw[1]], 1) * (8.0 * torch.from_numpy(sc0)[bi])
    mk1 = torch.stack([jj % hw[1], jj // hw[1]], 1) * (8.0 * torch.from_numpy(sc1)[bi])
    np.testing.assert_allclose(got['mkpts0_c'].cpu().numpy(), mk0.numpy(), rtol=1e-6)
    np.testing.assert_allclose(got['mkpts1_c'].cpu().numpy(), mk1.numpy(), rtol=1e-6)
    A32, u32, v32 = restatement32(f0, f1, alpha, 3, mm0, mm1, prefilter=prefilter)
    _check_conf('masks', got, A, A32, L, L, prefilter)
    _bar('masks log_u', _abs(got['log_u'].cpu().numpy(), u), ATOL_POT, _abs(u32, u))
    _bar('masks log_v', _abs(got['log_v'].cpu().numpy(), v), ATOL_POT, _abs(v32, v))
    # a masked entry is exactly 0
    cw = got['conf_matrix_with_bin'][:, :L, :L].cpu().numpy()
    assert (cw[~(mm0[:, :, None] & mm1[:, None, :])] == 0).all()


@pytest.mark.parametrize('T, prefilter', [(0, False), (1, False), (3, False), (5, False), (0, True)])
def test_iterations(T, prefilter):
    hw0, hw1 = (12, 16), (10, 16)
    L, S = hw0[0] * hw0[1], hw1[0] * hw1[1]
    alpha = 1.0
    if prefilter:
        # T = 0 with the prefilter: no column pass has run, the column maxima come from a max-only column pass.  Rows and columns
        # without a partner, under a dustbin score above their best score, make both filters fire.
        f0, f1, _ = features(2, L, S, seed=20, share=0.7)
        alpha = 2.5
        A0, _, _ = oracle(f0, f1, alpha, T)
        assert (A0.argmax(2)[:, :L] == S).any() and (A0.argmax(1)[:, :S] == L).any(), 'the input does not exercise the prefilter'
    else:
        f0, f1, _ = features(2, L, S, seed=20 + T)
    _check(f0, f1, alpha, T, hw0, hw1, prefilter=prefilter, want_conf=True, name=f'T={T} prefilter={prefilter}',
           min_matches=0 if T == 0 else 20)


@pytest.mark.parametrize('alpha', [1.0, -0.5, 2.5])
def test_bin_scores(alpha):
    hw0, hw1 = (12, 16), (10, 16)
    f0, f1, _ = features(2, hw0[0] * hw0[1], hw1[0] * hw1[1], seed=30, weak=0.3)
    _check(f0, f1, alpha, 3, hw0, hw1, want_conf=True, name=f'alpha={alpha}', min_matches=10)


def test_bin_score_is_read_on_the_device():
    """Changing the parameter in place on the device (no host copy anywhere) changes the result to that of the new value."""
    hw = (12, 16)
    L = hw[0] * hw[1]
    f0, f1, _ = features(2, L, L, seed=31, weak=0.3)
    bs = torch.tensor(1.0, device='cuda')
    a = _run(f0, f1, bs, 3, hw, hw)
    with torch.no_grad():
        bs.fill_(2.5)
    b = _run(f0, f1, bs, 3, hw, hw)
    c = _run(f0, f1, 2.5, 3, hw, hw)
    assert not torch.equal(a['log_u'], b['log_u'])
    for k in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'log_u', 'log_v'):
        assert torch.equal(b[k], c[k]), k


def test_prefilter_changes_the_match_set():
    """skh_prefilter (coarse_matching.py:134-139): rows / columns whose largest assignment is the dustbin entry are zeroed.
    Weakly correlated rows under a high dustbin score: matches above thr that the prefilter removes."""
    from oracle import coarse as oc
    hw = (16, 20)
    L = hw[0] * hw[1]
    f0, f1, _ = features(2, L, L, seed=40, weak=0.4, weak_scale=0.6)
    alpha = 2.5
    A, _, _ = oracle(f0, f1, alpha, 3)
    plain = oc.get_coarse_match(A[:, :L, :L], THR, BORDER, hw, hw, (hw[0] * 8, hw[1] * 8))
    got, ref = _check(f0, f1, alpha, 3, hw, hw, prefilter=True, want_conf=True, name='prefilter', min_matches=20)
    print(f'[prefilter] matches without / with the prefilter: {len(plain["i_ids"])} / {len(ref["i_ids"])}')
    assert len(ref['i_ids']) < len(plain['i_ids']), 'the input does not exercise the prefilter'
    nopf = _run(f0, f1, alpha, 3, hw, hw, prefilter=False)
    np.testing.assert_array_equal(nopf['i_ids'].cpu().numpy(), plain['i_ids'])


def test_determinism_next_to_a_busy_stream():
    """32 pairs at 60 x 80, >= 20 launches next to tests/test_determinism_gpu.py's busy stream: every output bit-identical."""
    from far_amd import ops
    from tests.test_determinism_gpu import _repeat
    hw = (60, 80)
    L = hw[0] * hw[1]
    g = torch.Generator(device='cuda').manual_seed(5)
    f0 = 3.75 * torch.randn(32, L, C, device='cuda', generator=g)
    perm = torch.randperm(L, device='cuda', generator=g)
    f1 = f0[:, perm] + 0.1 * torch.randn(32, L, C, device='cuda', generator=g)
    bs = torch.tensor(1.0, device='cuda')

    def fn():
        o = ops.coarse_match_sinkhorn(f0, f1, bs, 3, THR, BORDER, hw, hw, 8.0, prefilter=True, want_potentials=True)
        return o['b_ids'], o['i_ids'], o['j_ids'], o['mconf'], o['mkpts0_c'], o['mkpts1_c'], o['log_u'], o['log_v']
    first = fn()
    assert first[0].numel() > 32 * 3000
    _repeat(fn, 'sinkhorn 32 x 4800')


# ---- the drop-in module ------------------------------------------------------------------------------------------------
FEAT_GAIN = 4.0        # the synthetic checkpoint's coarse features are ~unit scale; scaled so that the matcher is confident


def _ot_model():
    from far_amd import synth
    from far_amd.config import far_eval_config
    from far_amd.loftr import LoFTR
    cfg = far_eval_config()
    cfg['match_coarse'].update(match_type='sinkhorn', skh_prefilter=True)
    m = LoFTR(cfg).eval()
    # the synthetic checkpoint of the dual-softmax model (the same weights as tests/test_pipeline_gpu.py's), bin_score = 1
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if k != 'coarse_matching.bin_score'}
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synthetic_state_dict(shapes, 0).items()}, strict=False)
    assert res.missing_keys == ['coarse_matching.bin_score'] and not res.unexpected_keys
    with torch.no_grad():
        m.coarse_matching.bin_score.fill_(1.0)
    m = m.cuda()
    captured = {}

    def hook(mod, args):
        a0, a1 = args[0] * FEAT_GAIN, args[1] * FEAT_GAIN
        captured['f0'], captured['f1'] = a0.detach().clone(), a1.detach().clone()
        return (a0, a1) + tuple(args[2:])
    m.coarse_matching.register_forward_pre_hook(hook)
    return m, captured


def _batch(N, seed):
    from far_amd import synth
    im0, im1 = synth.synth_image_pair(N, seed=seed)
    K = torch.from_numpy(np.stack([synth.MP3D_K] * N)).cuda()
    return {'image0': torch.from_numpy(im0).cuda(), 'image1': torch.from_numpy(im1).cuda(), 'K0': K, 'K1': K.clone(),
            'dataset_name': ['mp3d']}


def test_model_coarse_outputs_equal_the_ops_call():
    from far_amd import ops
    m, cap = _ot_model()
    data = _batch(2, 3)
    with torch.no_grad():
        m(data)
    ref = ops.coarse_match_sinkhorn(cap['f0'], cap['f1'], m.coarse_matching.bin_score, m.coarse_matching.skh_iters, m.coarse_matching.thr,
                                    m.coarse_matching.border_rm, data['hw0_c'], data['hw1_c'], data['hw0_i'][0] / data['hw0_c'][0],
                                    prefilter=True)
    print(f'[model] coarse matches: {ref["b_ids"].numel()}')
    assert ref['b_ids'].numel() > 0
    for k in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c'):
        assert torch.equal(data[k], ref[k]), k
    assert data['conf_matrix'] is None and 'conf_pos' not in data
    m.coarse_matching.materialize_conf = True
    d2 = _batch(2, 3)
    with torch.no_grad():
        m(d2)
    cw = d2['conf_matrix_with_bin']
    L, S = cw.shape[1] - 1, cw.shape[2] - 1
    assert d2['conf_matrix'].shape == (2, L, S) and d2['conf_matrix'].data_ptr() == cw.data_ptr()
    for k in ('b_ids', 'i_ids', 'j_ids', 'mconf'):
        assert torch.equal(d2[k], ref[k]), k


def test_model_test_step_twice_bit_identical_and_precision_refused():
    """far_amd.pipeline.test_step (match + solve + regress) on an optimal-transport model, with the head's feature stage on its
    side stream next to the Sinkhorn launches: two runs, the same bits."""
    from far_amd.loftr import LoFTR
    from far_amd.pipeline import test_step
    m, _ = _ot_model()
    assert LoFTR.head_side_stream
    keys = ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_f', 'mkpts1_f', 'loftr_rt', 'regressed_rt', 'solver_inlier_mask')
    outs = []
    for _ in range(2):
        d = _batch(4, 21)
        torch.cuda.synchronize()
        test_step(m, d, H=256)
        torch.cuda.synchronize()
        outs.append({k: d[k].clone() for k in keys})
    assert outs[0]['b_ids'].numel() > 0
    for k in keys:
        assert torch.equal(outs[0][k], outs[1][k]), k
    with pytest.raises(NotImplementedError, match='Sinkhorn'):
        m.set_precision('fp16')
    assert m.precision_stages == ()


def test_activation_range_guard_covers_the_sinkhorn_model():
    """LoFTR's activation-range guard (model.py: _guarded) on an optimal-transport model.  An overflow outside the coarse features
    (the FPN's fine branch scaled by 2^13: the fine level's inputs leave the split-fp16 range) is widened and re-run like on the
    dual-softmax model, and the Sinkhorn matcher runs in the widened state.  Coarse features themselves beyond the range (the stem's
    BatchNorm scaled by 2^13, as tests/test_pipeline_gpu.py does) have no exact-f32 Sinkhorn form: ActivationOverflow, and the
    module is left as it was -- the same model on clean weights runs at the default range again."""
    import warnings
    from far_amd import ops
    from far_amd.loftr.transformer import LoFTREncoderLayer
    m, _ = _ot_model()
    with torch.no_grad():
        m.backbone.layer1_outconv2[3].weight.mul_(2.0 ** 13)
    data = _batch(1, 5)
    ops.overflow_flag('cuda').zero_()
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        m(data)
    print('[sinkhorn range recovery] activation exponent after the re-run(s):', m.act_exp, ' matches:', data['b_ids'].numel())
    assert m.act_exp < 4 and any('activation' in str(w.message) for w in rec)
    assert float(data['featmap_f0'].abs().max()) > 4094.0            # the test does exercise the range
    for key in ('expec_f', 'mkpts1_f', 'mconf'):
        assert torch.isfinite(data[key]).all(), key
    assert data['b_ids'].numel() > 100
    assert not ops.activation_overflowed('cuda')
    d2 = _batch(1, 6)                                                   # the widened setting sticks: no further re-run
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec2:
        warnings.simplefilter('always')
        m(d2)
    assert not [w for w in rec2 if 'activation' in str(w.message)] and d2['b_ids'].numel() > 100

    m, _ = _ot_model()
    layers = [l for l in m.modules() if isinstance(l, LoFTREncoderLayer)]
    before = (m.act_exp, m.coarse_matching.variant, [(l.fused_attn, l.fused_mlp) for l in layers])
    with torch.no_grad():
        m.backbone.bn1.weight.mul_(2.0 ** 13)
        m.backbone.bn1.bias.mul_(2.0 ** 13)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(ops.ActivationOverflow):
            m(_batch(1, 5))
    assert (m.act_exp, m.coarse_matching.variant, [(l.fused_attn, l.fused_mlp) for l in layers]) == before
    with torch.no_grad():
        m.backbone.bn1.weight.div_(2.0 ** 13)                          # powers of two: the original weights exactly
        m.backbone.bn1.bias.div_(2.0 ** 13)
    d3 = _batch(1, 5)
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec3:
        warnings.simplefilter('always')
        m(d3)
    assert not [w for w in rec3 if 'activation' in str(w.message)] and m.act_exp == 4 and d3['b_ids'].numel() > 100
