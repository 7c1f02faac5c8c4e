"""Gradient clipping by the global norm, Adam and the non-finite guard in K20's optimizer step (far_amd/optim.py,
far_amd/csrc/adamw_f32.hip) on the GPU.

Shapes: the K20 test's odd sizes, an exact chunk (4096) and one tensor of 1100 * 4096 + 3 elements, so that the finalize kernel sums
more partials (1108) than it has lanes (1024); the last tensor never gets a gradient.

Measured on an MI355X (test_fused_step_against_float64_reference; worst tensor's fraction of the K20 bar, ours / torch's own fp32
two-call form; the full list is profiles/grad_clip_parity.txt): AdamW wd 0.1 parameters 0.226 / 0.226, exp_avg 0.413 / 0.488, exp_avg_sq
0.160 / 0.203; Adam wd 0 0.131 / 0.131, 0.413 / 0.488, 0.160 / 0.203; Adam wd 0.1 0.258 / 0.256, 0.091 / 0.086, 0.164 / 0.159."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(5000,), (64, 33, 3, 3), (1,), (4097,), (256, 256), (4096,), (1100 * 4096 + 3,), (7,)]
NOGRAD = len(SHAPES) - 1                       # this tensor never gets a gradient
HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8)
# randn gradients of these shapes have a 2-norm of about 2460 x their scale: with this base the five steps scaled 10^(it - 2) have norms
# of about 0.025, 0.25, 2.5, 25, 250 -- two steps below max_grad_norm = 0.5 (coefficient exactly 1), three above it
BASE = 1e-3
P_RTOL, P_ATOL = 2e-6, 1e-7                    # the project's K20 bars (test_adamw_one_launch_matches_torch_adamw)
M_RTOL, M_ATOL = 2e-6, 2e-7                    # the moments' atol is relative to max |moment|


def _params(seed=3):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device='cuda')) for s in SHAPES]


def _clone(ps):
    return [torch.nn.Parameter(p.detach().clone()) for p in ps]


def _grads(it, seed=11, base=BASE):
    g = torch.Generator(device='cuda').manual_seed(seed * 100 + it)
    return [None if i == NOGRAD else torch.randn(s, device='cuda', generator=g) * (base * 10.0 ** (it - 2)) for i, s in enumerate(SHAPES)]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.clone()


def _norm64(gs, norm_type=2.0):
    gs = [g for g in gs if g is not None]
    if norm_type == math.inf:
        return torch.stack([g.double().abs().max() for g in gs]).max()
    return torch.stack([(g.double() ** 2).sum() for g in gs]).sum().sqrt()


def _within_one_ulp(got, ref64):
    ref = ref64.float()                           # the float64 norm rounded to fp32
    ulp = torch.nextafter(ref.abs(), torch.tensor(math.inf, device=ref.device)) - ref.abs()
    return bool((got.double() - ref.double()).abs() <= ulp.double())


def _bits_equal(a, b):
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _state_equal(oa, pa, ob, pb):
    for i, (a, b) in enumerate(zip(pa, pb)):
        if not _bits_equal(a, b):
            return False
        if i != NOGRAD and not all(_bits_equal(oa.state[a][k], ob.state[b][k]) for k in ('exp_avg', 'exp_avg_sq')):
            return False
    return True


def _case_grads(case):
    if case == 'ordinary':
        return _grads(2, base=1.0)
    if case == 'zero':
        return [None if g is None else torch.zeros_like(g) for g in _grads(2)]
    # 'wide': 1e-20 ... 1e15 across the tensors of one table, and the large tensor at 1e18: its squares sum to 4.5e42, past fp32
    gs = _grads(2, base=1.0)
    for i, e in zip(range(NOGRAD), (-20, -15, -10, -5, 5, 15, 18)):
        gs[i] = gs[i] * (10.0 ** e)
    return gs


@pytest.mark.parametrize('norm_type', [2.0, math.inf])
@pytest.mark.parametrize('case', ['ordinary', 'wide', 'zero'])
def test_norm_matches_float64(case, norm_type):
    """optimizer.grad_norm and clip_grad_norm_'s return value: the float64 norm of the concatenated gradients rounded to fp32, within
    1 fp32 ulp (exact squares, a float64 sum of < 1e8 terms, one rounding); inf: exactly max |g|; repeated launches give the same bits."""
    from far_amd import optim
    ps = _params()
    gs = _case_grads(case)
    ref = _norm64(gs, norm_type)
    _set(ps, gs)
    got = [optim.clip_grad_norm_(ps, 1e30, norm_type) for _ in range(3)]          # the coefficient is 1: the gradients stay as they are
    assert got[0].shape == () and got[0].dtype == torch.float32 and got[0].is_cuda
    print(f'[grad_norm] {case} norm_type {norm_type}: ours {float(got[0])!r} float64 {float(ref)!r}')
    assert _bits_equal(got[0], got[1]) and _bits_equal(got[0], got[2])
    assert all(g is None or _bits_equal(p.grad, g) for p, g in zip(ps, gs))
    opt = optim.AdamW(ps, max_grad_norm=1e30, norm_type=norm_type, **HYPER)
    opt.step()
    assert _bits_equal(opt.grad_norm, got[0])
    assert opt.grad_norm.shape == () and opt.skipped_steps.dtype == torch.int32 and int(opt.skipped_steps) == 0
    if norm_type == math.inf:
        assert float(got[0]) == float(ref)
    else:
        assert _within_one_ulp(got[0], ref), (float(got[0]), float(ref))
    assert math.isfinite(float(got[0]))
    if case == 'zero':
        assert float(got[0]) == 0.0 and float(opt._ws['coef']) == 1.0
    assert all(bool(torch.isfinite(p).all()) for p in ps)


def test_coefficient_of_one_changes_no_bits():
    """Five steps of AdamW(max_grad_norm=1e30) against today's AdamW(): with a coefficient of exactly 1 the CLIP path is the plain one."""
    from far_amd.optim import AdamW
    pa = _params()
    pb = _clone(pa)
    oa = AdamW(pa, weight_decay=0.1, max_grad_norm=1e30, **HYPER)
    ob = AdamW(pb, weight_decay=0.1, **HYPER)
    for it in range(5):
        gs = _grads(it, base=1.0)
        _set(pa, gs); _set(pb, gs)
        oa.step(); ob.step()
    assert ob.grad_norm is None
    assert _state_equal(oa, pa, ob, pb)


@pytest.mark.parametrize('cls_name,wd', [('AdamW', 0.1), ('Adam', 0.1)])
def test_fused_step_is_the_two_step_form_bit_for_bit(cls_name, wd):
    """AdamW(max_grad_norm=0.5).step() against far_amd.optim.clip_grad_norm_(params, 0.5) + AdamW().step(): parameters and both moments
    bit for bit over five steps of which some clip and some do not (a g * coef contracted into the following g - m would differ);
    the fused step leaves p.grad alone, clip_grad_norm_ leaves g * coef behind."""
    import numpy as np
    from far_amd import optim
    cls = getattr(optim, cls_name)
    pa = _params()
    pb = _clone(pa)
    oa = cls(pa, weight_decay=wd, max_grad_norm=0.5, **HYPER)
    ob = cls(pb, weight_decay=wd, **HYPER)
    clipped = []
    for it in range(5):
        gs = _grads(it)
        _set(pa, gs); _set(pb, gs)
        oa.step()
        norm = optim.clip_grad_norm_(pb, 0.5)
        ob.step()
        assert _bits_equal(oa.grad_norm, norm)
        assert all(g is None or _bits_equal(p.grad, g) for p, g in zip(pa, gs)), 'the fused step modified p.grad'
        # the coefficient in IEEE fp32 on the host, as torch forms it: reciprocal, times max_norm, clamp
        n32 = np.float32(float(norm))
        coef = min(np.float32(np.float32(1.0) / np.float32(n32 + np.float32(1e-6))) * np.float32(0.5), np.float32(1.0))
        clipped.append(bool(coef < 1.0))
        for p, g in zip(pb, gs):
            assert (p.grad is None) if g is None else _bits_equal(p.grad, g * float(coef)), f'step {it}: clip_grad_norm_ is not g * coef'
        assert _state_equal(oa, pa, ob, pb), f'step {it}'
    assert clipped == [False, False, True, True, True], clipped
    assert pb[NOGRAD].grad is None and _bits_equal(pa[NOGRAD], _params()[NOGRAD])


def _ref64_steps(p0, steps, coupled, wd, max_norm, lr, betas, eps):
    """clip_grad_norm_ + AdamW / Adam restated in float64 on the same fp32 inputs."""
    b1, b2 = betas
    p = [x.detach().double() for x in p0]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    for k, gs in enumerate(steps, 1):
        coef = torch.clamp(max_norm / (_norm64(gs) + 1e-6), max=1.0)
        for i, g in enumerate(gs):
            if g is None:
                continue
            g = g.double() * coef
            if coupled:
                if wd != 0:
                    g = g + wd * p[i]
            else:
                p[i] = p[i] * (1 - lr * wd)
            m[i] = m[i] + (1 - b1) * (g - m[i])
            v[i] = b2 * v[i] + (1 - b2) * g * g
            p[i] = p[i] - (lr / (1 - b1 ** k)) * (m[i] / (v[i].sqrt() / math.sqrt(1 - b2 ** k) + eps))
    return p, m, v


def _bar_fraction(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 passes assert_close(rtol, atol)."""
    return float(((got.detach().double() - want).abs() / (atol + rtol * want.abs())).max())


@pytest.mark.parametrize('cls_name,wd', [('AdamW', 0.1), ('Adam', 0.0), ('Adam', 0.1)])
def test_fused_step_against_float64_reference(cls_name, wd):
    """Five fused steps at max_grad_norm = 0.5 against the float64 restatement, at the K20 bars (parameters rtol 2e-6 atol 1e-7, moments
    rtol 2e-6 atol 2e-7 max |moment|).  torch.nn.utils.clip_grad_norm_ + torch.optim in fp32 runs next to it on copies; where torch's
    own deviation exceeds a bar, the bar for that tensor is twice torch's deviation."""
    from far_amd import optim
    pa = _params()
    pb = _clone(pa)
    oa = getattr(optim, cls_name)(pa, weight_decay=wd, max_grad_norm=0.5, **HYPER)
    ob = getattr(torch.optim, cls_name)(pb, weight_decay=wd, **HYPER)
    steps = [_grads(it) for it in range(5)]
    p64, m64, v64 = _ref64_steps(pa, steps, cls_name == 'Adam', wd, 0.5, **HYPER)
    for gs in steps:
        _set(pa, gs); _set(pb, gs)
        oa.step()
        torch.nn.utils.clip_grad_norm_(pb, 0.5)
        ob.step()
    worst = {}
    fails = []
    for i, (a, b) in enumerate(zip(pa, pb)):
        rows = [('param', a, b, p64[i], P_RTOL, P_ATOL)]
        if i != NOGRAD:
            rows += [(k, oa.state[a][k], ob.state[b][k], w, M_RTOL, M_ATOL * float(w.abs().max()))
                     for k, w in (('exp_avg', m64[i]), ('exp_avg_sq', v64[i]))]
        for name, ours, theirs, want, rtol, atol in rows:
            if atol == 0.0:
                atol = 1e-300
            fo, ft = _bar_fraction(ours, want, rtol, atol), _bar_fraction(theirs, want, rtol, atol)
            print(f'[grad_clip_parity] {cls_name} wd={wd} tensor {i} {tuple(SHAPES[i])} {name}: ours {fo:.3f} torch {ft:.3f} of the bar')
            w = worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], fo), max(w[1], ft)
            if fo > max(1.0, 2.0 * ft):
                fails.append((i, name, fo, ft))
    for name, (fo, ft) in worst.items():
        print(f'[grad_clip_parity] {cls_name} wd={wd} worst {name}: ours {fo:.3f} torch {ft:.3f} of the bar')
    assert not fails, fails
    assert _bits_equal(pa[NOGRAD], pb[NOGRAD])


def test_adam_state_dict_round_trips_with_torch_adam():
    """A state dict written by torch.optim.Adam loads into far_amd.optim.Adam and the next (clipped) step agrees; and the reverse."""
    from far_amd import optim
    pa = _params()
    pb = _clone(pa)
    kw = dict(weight_decay=0.1, **HYPER)
    oa = optim.Adam(pa, max_grad_norm=0.5, **kw)
    ob = torch.optim.Adam(pb, **kw)

    def both(it, ours, theirs):
        gs = _grads(it)
        _set(pa, gs); _set(pb, gs)
        ours.step()
        torch.nn.utils.clip_grad_norm_(pb, 0.5)
        theirs.step()

    def check():
        for i, (a, b) in enumerate(zip(pa, pb)):
            torch.testing.assert_close(a, b, rtol=P_RTOL, atol=P_ATOL)

    for it in (1, 3):
        both(it, oa, ob)
    check()
    oa.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert oa.max_grad_norm == 0.5 and oa._coupled
    for a, b in zip(pa, pb):
        with torch.no_grad():
            a.copy_(b)
    both(2, oa, ob)
    check()
    assert [int(oa.state[a]['step']) for a in pa[:NOGRAD]] == [3] * NOGRAD
    oc = torch.optim.Adam(pb, **kw)
    oc.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert all(torch.is_tensor(oa.state[a]['step']) for a in pa[:NOGRAD])
    for a, b in zip(pa, pb):
        with torch.no_grad():
            b.copy_(a)
    both(3, oa, oc)
    check()
    for i, (a, b) in enumerate(zip(pa[:NOGRAD], pb[:NOGRAD])):
        for k in ('exp_avg', 'exp_avg_sq'):
            want = oc.state[b][k]
            torch.testing.assert_close(oa.state[a][k], want, rtol=M_RTOL, atol=M_ATOL * float(want.abs().max()))


@pytest.mark.parametrize('norm_type', [2.0, math.inf])
@pytest.mark.parametrize('bad', ['nan', 'inf'])
def test_nonfinite_gradient_default_mode_matches_torch(bad, norm_type):
    """One NaN (or +inf) in one gradient, default mode: the outcome of the fused step equals torch's two-call form on a copy.  NaN:
    every updated parameter is NaN.  inf: the norm is inf, the coefficient 0, the entry that held inf becomes NaN (inf * 0) and every
    other update is torch's result for g * 0.  The tensor without a gradient is untouched."""
    from far_amd import optim
    pa = _params()
    pb = _clone(pa)
    p0 = [p.detach().clone() for p in pa]
    oa = optim.AdamW(pa, weight_decay=0.1, max_grad_norm=0.5, norm_type=norm_type, **HYPER)
    ob = torch.optim.AdamW(pb, weight_decay=0.1, **HYPER)
    gs = _grads(2, base=1.0)
    gs[3][17] = math.nan if bad == 'nan' else math.inf
    _set(pa, gs); _set(pb, gs)
    oa.step()
    tn = torch.nn.utils.clip_grad_norm_(pb, 0.5, norm_type=norm_type)
    ob.step()
    torch.testing.assert_close(oa.grad_norm, tn, rtol=0, atol=0, equal_nan=True)
    assert int(oa.skipped_steps) == 0
    for i, (a, b) in enumerate(zip(pa, pb)):
        torch.testing.assert_close(a, b, rtol=P_RTOL, atol=P_ATOL, equal_nan=True)
        if i != NOGRAD:
            for k in ('exp_avg', 'exp_avg_sq'):
                torch.testing.assert_close(oa.state[a][k], ob.state[b][k], rtol=M_RTOL, atol=1e-30, equal_nan=True)
    assert _bits_equal(pa[NOGRAD], p0[NOGRAD])
    if bad == 'nan':
        assert math.isnan(float(oa.grad_norm))
        assert all(bool(torch.isnan(a).all()) for a in pa[:NOGRAD])
    else:
        assert float(oa.grad_norm) == math.inf and float(oa._ws['coef']) == 0.0
        nan = [torch.isnan(a) for a in pa[:NOGRAD]]
        assert int(sum(x.sum() for x in nan)) == 1 and bool(nan[3][17])


@pytest.mark.parametrize('cls_name', ['AdamW', 'Adam'])
def test_skip_nonfinite(cls_name):
    """skip_nonfinite=True: a step with a NaN gradient leaves parameters and both moments bit-identical and counts in skipped_steps; the
    next finite step updates normally (as a plain optimizer whose step count advanced too) and leaves the counter; with finite
    gradients the flag changes no bits."""
    from far_amd import optim
    cls = getattr(optim, cls_name)
    pa = _params()
    pb = _clone(pa)
    oa = cls(pa, weight_decay=0.1, skip_nonfinite=True, **HYPER)
    ob = cls(pb, weight_decay=0.1, **HYPER)
    for it in (2, 3):
        gs = _grads(it)
        _set(pa, gs); _set(pb, gs)
        oa.step(); ob.step()
    assert _state_equal(oa, pa, ob, pb)                       # finite gradients: the flag changes no bits
    assert int(oa.skipped_steps) == 0
    gs = _grads(4)
    gs[1][5, 7, 1, 2] = math.nan
    _set(pa, gs)
    oa.step()
    assert math.isnan(float(oa.grad_norm))
    assert int(oa.skipped_steps) == 1
    assert _state_equal(oa, pa, ob, pb)                       # untouched: still the twin's bits
    assert [int(oa.state[a]['step']) for a in pa[:NOGRAD]] == [3] * NOGRAD          # the host count advanced (documented)
    for b in pb[:NOGRAD]:
        ob.state[b]['step'] += 1
    gs = _grads(1)
    _set(pa, gs); _set(pb, gs)
    oa.step(); ob.step()
    assert int(oa.skipped_steps) == 1
    assert _state_equal(oa, pa, ob, pb)
    assert not _bits_equal(pa[0], _params()[0])
    # with max_grad_norm as well: an inf gradient is skipped too (its norm is inf)
    pc = _clone(pa)
    oc = cls(pc, weight_decay=0.1, max_grad_norm=0.5, skip_nonfinite=True, **HYPER)
    gs = _grads(2)
    gs[0][4999] = -math.inf
    _set(pc, gs)
    oc.step()
    assert int(oc.skipped_steps) == 1 and float(oc.grad_norm) == math.inf
    assert all(_bits_equal(c, a) for c, a in zip(pc, pa))
    assert all(float(oc.state[c][k].abs().max()) == 0.0 for c in pc[:NOGRAD] for k in ('exp_avg', 'exp_avg_sq'))


def test_error_if_nonfinite_raises_before_scaling():
    from far_amd import optim
    ps = _params()
    gs = _grads(2)
    gs[2][0] = math.nan
    _set(ps, gs)
    with pytest.raises(RuntimeError, match='non-finite'):
        optim.clip_grad_norm_(ps, 0.5, error_if_nonfinite=True)
    assert all(g is None or _bits_equal(p.grad, g) for p, g in zip(ps, gs))
    _set(ps, _grads(2))
    assert math.isfinite(float(optim.clip_grad_norm_(ps, 0.5, error_if_nonfinite=True)))


def test_two_parameter_groups_share_one_norm():
    """The norm is global over the parameter groups, as torch.nn.utils.clip_grad_norm_(all parameters) is."""
    from far_amd import optim
    pa = _params()
    pb = _clone(pa)
    oa = optim.AdamW([{'params': pa[:3]}, {'params': pa[3:], 'lr': 1e-3}], weight_decay=0.1, max_grad_norm=0.5, **HYPER)
    ob = optim.AdamW([{'params': pb[:3]}, {'params': pb[3:], 'lr': 1e-3}], weight_decay=0.1, **HYPER)
    for it in (1, 3):
        gs = _grads(it)
        _set(pa, gs); _set(pb, gs)
        oa.step()
        norm = optim.clip_grad_norm_(pb, 0.5)
        ob.step()
        assert _bits_equal(oa.grad_norm, norm) and _within_one_ulp(norm, _norm64(gs))
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert _bits_equal(a, b)
        if i != NOGRAD:
            assert all(_bits_equal(oa.state[a][k], ob.state[b][k]) for k in ('exp_avg', 'exp_avg_sq'))


def test_model_parameter_table():
    """The parameter list of LoFTR(far_train_config()['loftr']) (189 tensors, about 12 500 partials): one fused step at max_grad_norm = 0.5
    is bit-identical to clip_grad_norm_ + AdamW().step(), and the norm is within 1 ulp of float64."""
    from far_amd import optim
    from far_amd.config import far_train_config
    from far_amd.loftr import LoFTR
    shapes = [tuple(p.shape) for p in LoFTR(far_train_config()['loftr']).parameters()]
    assert len(shapes) > 100
    torch.manual_seed(5)
    pa = [torch.nn.Parameter(torch.randn(s, device='cuda') * 0.05) for s in shapes]
    pb = _clone(pa)
    skip = len(shapes) // 2
    gs = [None if i == skip else torch.randn(s, device='cuda') * 1e-3 for i, s in enumerate(shapes)]
    _set(pa, gs); _set(pb, gs)
    oa = optim.AdamW(pa, lr=1e-3, weight_decay=0.1, max_grad_norm=0.5)
    ob = optim.AdamW(pb, lr=1e-3, weight_decay=0.1)
    oa.step()
    norm = optim.clip_grad_norm_(pb, 0.5)
    ob.step()
    assert oa._tables[0]['nblocks'] == sum((math.prod(s) + 4095) // 4096 for s in shapes) > 12000
    ref = _norm64(gs)
    print(f'[grad_norm] model table: ours {float(norm)!r} float64 {float(ref)!r}, {oa._tables[0]["nblocks"]} partials')
    assert float(norm) > 0.5                                   # the step clipped
    assert _bits_equal(oa.grad_norm, norm) and _within_one_ulp(norm, ref)
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert _bits_equal(a, b), i
        if i != skip:
            assert all(_bits_equal(oa.state[a][k], ob.state[b][k]) for k in ('exp_avg', 'exp_avg_sq')), i
    assert float(oa.state[pa[skip]]['exp_avg'].abs().max()) == 0.0
