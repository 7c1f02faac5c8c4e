"""K12 training (far_corr_volume_warp_train_f32 / far_corr_volume_warp_bwd_f32, ops.corr_volume_warp_train,
mapfree.CorrelationVolumeWarping) on the GPU against the float64 restatement of tests/cvw_train_ref.py.

The bar is the project's rule (tests/test_full_attention_gpu.py: _bar), per gradient tensor:
    |got - r64| <= max(3 dev32, 2^-20 max |r64|),   dev32 = the same restatement in fp32 on the same GPU in the same run.
Every parity case first asserts its input condition in float64 (each row's two largest scores at least cvw_train_ref.MIN_GAP apart:
the arg-max channel's gradient is discontinuous); no row is excluded from any comparison.  The measured ratios are printed
(profiles/cvw_train_parity.txt holds a copy)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import cvw_train_ref as cr

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FLOOR = 2.0 ** -20


def _bar(name, got, r64, r32, factor=3.0):
    """Asserts max |got - r64| <= max(factor dev32, 2^-20 max |r64|), printing the figures first."""
    r64 = r64.double()
    dev32 = float((r32.double() - r64).abs().max())
    floor = FLOOR * float(r64.abs().max())
    bar = max(factor * dev32, floor)
    d = float((got.double() - r64).abs().max())
    ratio = f'{d / dev32:.2f}' if dev32 > 0 else 'n/a'
    print(f'[parity] {name}: kernel-vs-ref {d:.3e}  dev32 {dev32:.3e}  ratio {ratio}  bar {bar:.3e} '
          f'({"floor 2^-20 max|ref| decides" if floor > factor * dev32 else f"{factor:g} x dev32"})')
    assert torch.isfinite(got).all(), name
    assert d <= bar, f'{name}: {d:.3e} > {bar:.3e}'
    return d


def _refs(v0, v1, dagg, rows=None):
    """The input condition, then (r64, r32): (agg, dvol0, dvol1) of the restatement in float64 and in fp32 on the GPU."""
    t0, t1 = torch.from_numpy(v0).cuda(), torch.from_numpy(v1).cuda()
    gap = cr.min_gap(t0, t1, rows)
    print(f'[condition] smallest top-2 score gap {gap:.3e} (>= {cr.MIN_GAP:g})')
    assert gap >= cr.MIN_GAP
    return cr.grads(v0, v1, dagg, torch.float64, 'cuda'), cr.grads(v0, v1, dagg, torch.float32, 'cuda')


@functools.lru_cache(maxsize=None)
def _case(name):
    v0, v1, dagg = cr.case_inputs(name)
    r64, r32 = _refs(v0, v1, dagg)
    return v0, v1, dagg, r64, r32


def _run(v0, v1, dagg, need=(True, True)):
    """ops.corr_volume_warp_train + backward -> (agg, dvol0 | None, dvol1 | None)."""
    from far_amd import ops
    a = torch.from_numpy(v0).cuda().requires_grad_(need[0])
    b = torch.from_numpy(v1).cuda().requires_grad_(need[1])
    agg = ops.corr_volume_warp_train(a, b)
    agg.backward(dagg if torch.is_tensor(dagg) else torch.from_numpy(dagg).cuda())
    return agg.detach(), a.grad, b.grad


@pytest.mark.parametrize('name', list(cr.CASES))
def test_parity_against_float64(name):
    v0, v1, dagg, r64, r32 = _case(name)
    agg, d0, d1 = _run(v0, v1, dagg)
    _bar(f'{name} agg', agg, r64[0], r32[0])
    _bar(f'{name} dvol0', d0, r64[1], r32[1])
    _bar(f'{name} dvol1', d1, r64[2], r32[2])


@pytest.mark.parametrize('name', ['flat', 'tiny'])
def test_forward_bits_are_the_inference_launch(name):
    from far_amd import ops
    v0, v1, dagg = cr.case_inputs(name)
    a, b = torch.from_numpy(v0).cuda(), torch.from_numpy(v1).cuda()
    want = ops.corr_volume_warp(a, b)
    got = ops.corr_volume_warp_train(a.clone().requires_grad_(True), b.clone().requires_grad_(True))
    assert got.grad_fn is not None
    assert torch.equal(got.detach(), want)


GROUPS = {'ga': slice(0, 32), 'gw': slice(32, 64), 'ge': slice(64, 66), 'gm': slice(66, 67)}


def _only(dagg, group):
    out = np.zeros_like(dagg)
    out[:, GROUPS[group]] = dagg[:, GROUPS[group]]
    return out


def test_ga_only_and_zero_gradient_are_exact():
    v0, v1, dagg = cr.case_inputs('two-block')
    ga = _only(dagg, 'ga')
    _, d0, d1 = _run(v0, v1, ga)
    assert torch.equal(d0.cpu(), torch.from_numpy(ga[:, :32]))
    assert torch.equal(d1, torch.zeros_like(d1))
    _, d0, d1 = _run(v0, v1, np.zeros_like(dagg))
    assert torch.equal(d0, torch.zeros_like(d0)) and torch.equal(d1, torch.zeros_like(d1))


@pytest.mark.parametrize('group', ['gw', 'ge', 'gm'])
def test_one_channel_group_at_a_time(group):
    """A wrong small term cannot hide behind the warp term: each group of dagg alone is held to the bar."""
    v0, v1, dagg = cr.case_inputs('two-block')
    g = _only(dagg, group)
    r64, r32 = _refs(v0, v1, g)
    _, d0, d1 = _run(v0, v1, g)
    assert float(r64[1].abs().max()) > 0 and float(r64[2].abs().max()) > 0
    _bar(f'two-block {group}-only dvol0', d0, r64[1], r32[1])
    _bar(f'two-block {group}-only dvol1', d1, r64[2], r32[2])


def test_ties_follow_the_first_index():
    """vol1 columns 40, 32, 131 are copies of columns 3, 31, 100 and six vol0 rows are 5 x those columns: their maxima (and those of
    the few rows that peak at one of these columns anyway) are tied between a column and its copy -- inside one lane's registers, across the two half-waves, across tiles.  The max-score gradient
    goes to the lower index alone, as in the float64 restatement; dvol1 at the tied columns tells the two apart."""
    v0, v1, dagg = cr.case_inputs('two-block')
    v0, v1 = v0.copy(), v1.copy()
    B, D, H, W = v0.shape
    f0, f1 = v0.reshape(B, D, H * W), v1.reshape(B, D, H * W)
    first, copy = (3, 31, 100), (40, 32, 131)
    for c, k in zip(first, copy):
        f1[:, :, k] = f1[:, :, c]
    tied_rows = (0, 17, 50, 64, 129, 131)
    for i, c in zip(tied_rows, first + first):
        f0[:, :, i] = 5.0 * f1[:, :, c]
    js = cr.argmax_first(torch.from_numpy(v0).double(), torch.from_numpy(v1).double())
    assert [int(js[0, i]) for i in tied_rows] == list(first + first)
    # every row whose best column is one of the copied ones is tied (the six made so, and those that happen to peak there): the
    # input condition is asked of all the others
    rows = ~torch.isin(js, torch.tensor(first))
    assert not rows[0, list(tied_rows)].any()
    print(f'[ties] {int((~rows).sum())} tied rows of {rows.numel()}')
    g = _only(dagg, 'gm')
    r64, r32 = _refs(v0, v1, g, rows)
    _, d0, d1 = _run(v0, v1, g)
    _bar('ties gm-only dvol0', d0, r64[1], r32[1])
    _bar('ties gm-only dvol1', d1, r64[2], r32[2])
    # the yardstick does tell the rule: at the tied columns the two choices differ by far more than the bar
    r1 = r64[2].reshape(B, D, H * W)
    assert float((r1[:, :, list(first)] - r1[:, :, list(copy)]).abs().max()) > 1e-2


def test_needs_input_grad_double_backward_and_no_grad():
    from far_amd import ops
    v0, v1, dagg = cr.case_inputs('two-block')
    _, d0, d1 = _run(v0, v1, dagg)
    _, e0, none1 = _run(v0, v1, dagg, need=(True, False))
    none0, e1, = _run(v0, v1, dagg, need=(False, True))[1:]
    assert none1 is None and none0 is None
    assert torch.equal(e0, d0) and torch.equal(e1, d1)
    a = torch.from_numpy(v0).cuda().requires_grad_(True)
    b = torch.from_numpy(v1).cuda().requires_grad_(True)
    agg = ops.corr_volume_warp_train(a, b)
    (g0,) = torch.autograd.grad(agg, (a,), torch.from_numpy(dagg).cuda(), create_graph=True)
    with pytest.raises(RuntimeError):
        g0.sum().backward()
    with torch.no_grad():
        assert ops.corr_volume_warp_train(a, b).grad_fn is None
    assert ops.corr_volume_warp_train(a.detach(), b.detach()).grad_fn is None
    with pytest.raises(Exception):
        ops.corr_volume_warp_train(torch.zeros(1, 16, 4, 4).cuda().requires_grad_(True), torch.zeros(1, 16, 4, 4).cuda())     # D must be 32


def test_nhwc_upstream_gradient_gives_the_same_bits():
    v0, v1, dagg = cr.case_inputs('tiny')
    _, d0, d1 = _run(v0, v1, dagg)
    g = torch.from_numpy(dagg).cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)          # NCHW view of NHWC memory
    assert not g.is_contiguous()
    _, e0, e1 = _run(v0, v1, g)
    assert torch.equal(e0, d0) and torch.equal(e1, d1)


def test_batch_independence_and_repeatability():
    v0, v1, dagg = cr.case_inputs('flat')
    agg, d0, d1 = _run(v0, v1, dagg)
    a1, s0, s1 = _run(v0[1:2], v1[1:2], dagg[1:2])
    assert torch.equal(a1, agg[1:2]) and torch.equal(s0, d0[1:2]) and torch.equal(s1, d1[1:2])
    side = torch.cuda.Stream()
    m = torch.randn(1024, 1024, device='cuda')
    for rep in range(5):
        if rep >= 2:                                    # neighbours on the CUs: a second stream busy with matmuls
            with torch.cuda.stream(side):
                for _ in range(20):
                    m @ m
        again = _run(v0, v1, dagg)
        assert torch.equal(again[0], agg) and torch.equal(again[1], d0) and torch.equal(again[2], d1), rep
    torch.cuda.synchronize()


def test_golden_g29():
    g = np.load(os.path.join(G, 'g29_cvw_train.npz'))
    agg, d0, d1 = _run(g['vol0'], g['vol1'], g['dagg'])
    gap = cr.min_gap(torch.from_numpy(g['vol0']), torch.from_numpy(g['vol1']))
    assert gap >= cr.MIN_GAP
    np.testing.assert_allclose(agg.cpu().numpy(), g['agg32'], rtol=2e-5, atol=2e-6)
    t = lambda k: torch.from_numpy(g[k]).cuda()
    _bar('g29 agg', agg, t('agg64'), t('agg32'))
    _bar('g29 dvol0', d0, t('dvol0_64'), t('dvol0_32'))
    _bar('g29 dvol1', d1, t('dvol1_64'), t('dvol1_32'))


def test_module_in_a_composition():
    """mapfree.CorrelationVolumeWarping, a torch 3 x 3 convolution 67 -> 8 and a sum of squares: the gradients of both volumes and of the
    convolution weight against the same composition in float64."""
    import torch.nn.functional as F
    from far_amd import mapfree
    from tests import mapfree_reg_inputs as mi
    m = mapfree.CorrelationVolumeWarping(mi.config().AGGREGATOR, 32)
    assert m.num_out_layers == 67 and len(m.state_dict()) == 0 and not list(m.parameters())
    v0, v1, _ = cr.case_inputs('two-block')
    w = (np.random.default_rng(19).standard_normal((8, 67, 3, 3)) / np.sqrt(67 * 9)).astype(np.float32)
    gap = cr.min_gap(torch.from_numpy(v0), torch.from_numpy(v1))
    assert gap >= cr.MIN_GAP

    def compose(agg_fn, dtype, device='cuda'):
        a, b, k = (torch.from_numpy(x).to(device=device, dtype=dtype).requires_grad_(True) for x in (v0, v1, w))
        loss = F.conv2d(agg_fn(a, b), k, padding=1).pow(2).sum()
        return [t.cuda() for t in [loss.detach()] + list(torch.autograd.grad(loss, (a, b, k)))]

    r64 = compose(cr.aggregate, torch.float64, 'cpu')                    # (float64 convolutions: on the CPU)
    r32, got = compose(cr.aggregate, torch.float32), compose(m, torch.float32)
    for name, x, y, z in zip(('loss', 'dvol0', 'dvol1', 'dweight'), got, r64, r32):
        _bar(f'module {name}', x, y, z)
    with torch.no_grad():
        assert m(torch.from_numpy(v0).cuda(), torch.from_numpy(v1).cuda()).grad_fn is None
