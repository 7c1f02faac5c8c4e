"""K9 in Linear mode (ops.linear_f16s: conv_igemm_f16s.hip and linear_small_f16s.hip), its training pair (K9's transposed-weight dgrad,
K16 linear_wgrad) and K6 LayerNorm at the 8-Point-ViT trunk's layer shapes, against float64, in every launch form the host code picks.

The layers (far_amd/vit8pt.py: Attention.forward, Mlp, Block):

    layer   K -> Cout   call                          cfg_for: pad128 / pad256 -> tile            column blocks (nblkY)
    qkv     192 -> 576  out_planes = 9 (planes of 64) 640 < 768 -> 4 x 1 waves, 128 columns       5; the last is half real (512..575), and
                                                                                                  every block spans two planes
    proj    192 -> 192  residual=                     256 = 256 -> 2 x 2 waves, 256 columns       1, with 64 padded columns
    fc1     192 -> 768  plain                         768 = 768 -> 2 x 2 waves, 256 columns       3
    fc2     768 -> 192  residual=, input gelu(.)      as proj                                     1

Launch forms (conv_nhwc_impl).  nbx = ceil(rows / (64 mw)) full-height row tiles, mw = 4 (qkv) or 2:
  * few-row kernel: split operands, nbx nblkY < 512, and far_linear_small_covers: K <= 256 and ceil(rows / 128) ceil(Cout / 64) <= 320;
  * K9 on half-height tiles (32 mw rows): nbx nblkY < 192;
  * K9 on full-height tiles (64 mw rows) otherwise, and always under tuning knob 7.
Where the forms change, for split operands:
    qkv   few-row: ceil(rows / 128) 9 <= 320 -> 35 blocks -> rows <= 4480 (nbx 5 < 512 holds up to 26 112 rows)
          half:    ceil(rows / 256) 5 < 192 -> nbx <= 38 -> rows <= 9728;            full: rows >= 9729
    fc1   few-row: ceil(rows / 128) 12 <= 320 -> 26 blocks -> rows <= 3328
          half:    ceil(rows / 128) 3 < 192 -> nbx <= 63 -> rows <= 8064;            full: rows >= 8065
    proj  few-row: ceil(rows / 128) 3 <= 320 -> 106 blocks -> rows <= 13 568 (nbx < 512 holds beyond that)
          half:    ceil(rows / 128) < 192 -> nbx <= 191 -> rows <= 24 448;           full: rows >= 24 449
    fc2   few-row: never (K = 768 > 256);  half / full as proj
Plain fp16 operands (split=False) have no few-row form; their half / full boundaries are the same.  _form() restates this arithmetic and
test_row_counts_reach_every_form pins the table above to it.

Row counts (ROWS), for every layer and both operand classes: 1 and 37; 2304 (the model tests' count); the last count of each form and the
first of the next; one count inside each form that is no multiple of 32 (37 in the first form, then 7001 / 5001 / 19 001 and the largest).
The inputs of a count are the first rows of the layer's largest case, so the float64 and fp32 references are computed once per layer and
the bits of every count can be compared with the largest launch's (the batch-invariance the model promises).

Bars.  Split operands: the project's parity rule (tests/test_full_attention_gpu.py: _bar), max(3 x dev32, 2^-20 max|ref|), dev32 being the
fp32 torch composition's deviation from float64 in the same run -- applied to every output plane, to the real channels of the last column
block and to the rows of the last (partial) row tile separately, each with its own dev32 and its own floor, so that a quiet block or tail
cannot hide under the global maximum.  Plain fp16 operands: the sharp bar of tests/test_conv_valid_f16_gpu.py (float64 of the operands
rounded as the kernel rounds them, the same rule) and the class bar es < e < 3e-3.  Training: the same rule for dx, dW, db against float64
autograd, dev32 from fp32 autograd.  K6 at C = 192: the bars of test_layernorm and test_layernorm_train_matches_float64.

What a slip would meet.  Plane co / 128 instead of co / Csub sends every qkv channel from 64 up to the wrong plane: eight of the
nine planes of test_split_matches_float64 are off by O(1).  Without the co < Cout guard the last block's padded columns go to 'plane 9' of qkv
(behind the result, inside the guard of one whole plane) and, for proj / fc2, to the next row -- for the last row behind the result:
test_nothing_outside_the_result_is_written.  A row tail one too long writes row `rows` of the last plane behind the result (the same
test); one too short leaves the last row's sentinel in place (the same test) and fails the last-row-tile bar.  A form that orders its
products differently fails the two bit comparisons.

Every measured figure is printed ('[parity] ...'; profiles/linear_vit_shapes_parity.txt records a run)."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_full_attention_gpu import _bar

pytestmark = pytest.mark.gpu

LAYERS = {            # K, Cout, output planes, residual, gelu input
    'qkv': (192, 576, 9, False, False),
    'proj': (192, 192, 1, True, False),
    'fc1': (192, 768, 1, False, False),
    'fc2': (768, 192, 1, True, True),
}
ROWS = {
    'qkv': (1, 37, 2304, 4480, 4481, 7001, 9728, 9729, 10007),
    'fc1': (1, 37, 2304, 3328, 3329, 5001, 8064, 8065, 8231),
    'proj': (1, 37, 2304, 13568, 13569, 19001, 24448, 24449, 24503),
    'fc2': (1, 37, 2304, 19001, 24448, 24449, 24503),
}
CASES = [(layer, rows) for layer in LAYERS for rows in ROWS[layer]]
IDS = [f'{layer}-{rows}' for layer, rows in CASES]
ACT_EXP = 4
LN_EPS = 1e-6                                                             # vit8pt.NORM
_CACHE = {}


def _cdiv(a, b):
    return (a + b - 1) // b


def _tile(Cout):
    """cfg_for at stride 1: (mw, nt)."""
    return (4, 128) if _cdiv(Cout, 128) * 128 < _cdiv(Cout, 256) * 256 else (2, 256)


def _form(K, Cout, rows, split):
    """(launch form, rows per row tile) as conv_nhwc_impl decides for a plain Linear launch with tuning knob 7 clear."""
    mw, nt = _tile(Cout)
    nblk, nbx = _cdiv(Cout, nt), _cdiv(rows, 64 * mw)
    if split and nbx * nblk < 512 and 32 <= K <= 256 and K % 32 == 0 and _cdiv(rows, 128) * _cdiv(Cout, 64) <= 320:
        return 'few', 128
    if nbx * nblk < 192:
        return 'half', 32 * mw
    return 'full', 64 * mw


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _rounded(x, act_exp=ACT_EXP):
    return (x * 2.0 ** act_exp).half().float() * 2.0 ** -act_exp


def _case(layer):
    """Seeded operands of a layer at its largest row count, both packs and the float64 / fp32 compositions every check shares (never
    modified; one layer's tensors at a time)."""
    if layer not in _CACHE:
        from far_amd import ops
        K, Cout, P, has_res, gelu = LAYERS[layer]
        R = max(ROWS[layer])
        g = _gen(1000 * K + Cout)
        x = torch.randn(R, K, device='cuda', generator=g)                            # LayerNorm-output scale, signed
        if gelu:
            x = F.gelu(x)
        w = torch.randn(Cout, K, device='cuda', generator=g) * K ** -0.5
        b = 0.5 * torch.randn(Cout, device='cuda', generator=g)
        res = torch.randn(R, Cout, device='cuda', generator=g) if has_res else None
        c = dict(x=x, w=w, b=b, res=res)
        c['pack', True], c['pack', False] = ops.PackedConv(w, None, b), ops.PackedConv(w, None, b, split=False)
        c['r64'], c['r32'] = _compose(x, w, b, res, torch.float64), _compose(x, w, b, res, torch.float32)
        _CACHE.clear()
        _CACHE[layer] = c
    return _CACHE[layer]


def _compose(x, w, b, res, dtype):
    y = F.linear(x.to(dtype), w.to(dtype), b.to(dtype))
    return y if res is None else y + res.to(dtype)


def _rounded_refs(c):
    """float64 and fp32 compositions of the operands rounded as the plain-fp16 kernel rounds them (lazily: the plain tests only)."""
    if 'p64' not in c:
        s = c['pack', False].pack_scale[0]
        xr, wr = _rounded(c['x']), (c['w'] * s).half().float() / s
        c['p64'], c['p32'] = _compose(xr, wr, c['b'], c['res'], torch.float64), _compose(xr, wr, c['b'], c['res'], torch.float32)
    return c['p64'], c['p32']


def _run(c, layer, rows, split, out=None):
    """The launch the model issues for this layer on the first `rows` rows."""
    from far_amd import ops
    P, has_res = LAYERS[layer][2], LAYERS[layer][3]
    return ops.linear_f16s(c['x'][:rows], c['pack', split], residual=c['res'][:rows] if has_res else None, out_planes=P, out=out)


def _flat(y):
    """(P, rows, Csub) planes -> (rows, Cout)."""
    return y if y.dim() == 2 else y.permute(1, 0, 2).reshape(y.shape[1], -1)


def _hold(name, y, r64, r32, layer, rows, split):
    """The parity rule on every output plane, on the real channels of the last column block and on the rows of the last row tile, each
    with the fp32 composition's deviation on the same elements."""
    K, Cout, P, _, _ = LAYERS[layer]
    Csub = Cout // P
    yf = _flat(y)
    assert yf.shape == (rows, Cout)
    r64, r32 = r64[:rows], r32[:rows]
    dev = lambda sl: float((r32[sl].double() - r64[sl]).abs().max())
    for p in range(P):
        sl = (slice(None), slice(p * Csub, (p + 1) * Csub))
        got = y[p] if P > 1 else y
        _bar(f'{name} plane {p}', got, r64[sl], dev(sl))
    nt = _tile(Cout)[1]
    c0 = (_cdiv(Cout, nt) - 1) * nt
    if c0 > 0:
        sl = (slice(None), slice(c0, Cout))
        _bar(f'{name} last column block {c0}..{Cout - 1}', yf[sl], r64[sl], dev(sl))
    T = _form(K, Cout, rows, split)[1]
    t0 = (rows - 1) // T * T
    sl = (slice(t0, rows), slice(None))
    _bar(f'{name} last row tile {t0}..{rows - 1}', yf[sl], r64[sl], dev(sl))


def test_row_counts_reach_every_form():
    """The table of the docstring, restated by _form: the last count of each form, the first of the next, and what ROWS covers."""
    bounds = {'qkv': (4480, 9728), 'fc1': (3328, 8064), 'proj': (13568, 24448), 'fc2': (None, 24448)}
    for layer, (few, half) in bounds.items():
        K, Cout = LAYERS[layer][:2]
        for split in (True, False):
            if few is not None and split:
                assert _form(K, Cout, few, True)[0] == 'few' and _form(K, Cout, few + 1, True)[0] == 'half'
                assert _form(K, Cout, 1, True)[0] == 'few'
            else:
                assert _form(K, Cout, 1, split)[0] == 'half'
            assert _form(K, Cout, half, split)[0] == 'half' and _form(K, Cout, half + 1, split)[0] == 'full'
            forms = {}
            for rows in ROWS[layer]:
                forms.setdefault(_form(K, Cout, rows, split)[0], []).append(rows)
            assert set(forms) == ({'few', 'half', 'full'} if few is not None and split else {'half', 'full'}), (layer, split, forms)
            for f, rr in forms.items():                                   # inside every form a count that is no multiple of 32
                assert any(r % 32 for r in rr), (layer, split, f, rr)
        assert 2304 in ROWS[layer] and {1, 37} <= set(ROWS[layer])
    assert _tile(576) == (4, 128) and _tile(192) == (2, 256) and _tile(768) == (2, 256)


# ---- split operands against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize('layer,rows', CASES, ids=IDS)
def test_split_matches_float64(layer, rows):
    from far_amd import ops
    assert ops.activation_exponent_value() == ACT_EXP
    c = _case(layer)
    K, Cout, P, _, _ = LAYERS[layer]
    ops.overflow_flag('cuda').zero_()
    y = _run(c, layer, rows, True)
    assert not ops.activation_overflowed('cuda')
    assert y.shape == ((P, rows, Cout // P) if P > 1 else (rows, Cout)) and y.is_contiguous() and y.dtype == torch.float32
    form = _form(K, Cout, rows, True)[0]
    _hold(f'linear {layer} {K}->{Cout} @ {rows} rows split ({form})', y, c['r64'], c['r32'], layer, rows, True)


def test_qkv_planes_are_what_attention_consumes():
    """Attention.forward hands (Z, N, C) tokens to the qkv launch and its (3 h, Z, N, 64) planes straight to K23."""
    from far_amd import ops
    c = _case('qkv')
    x = c['x'][:2304].view(4, 576, 192)
    planes = ops.linear_f16s(x, c['pack', True], out_planes=9)
    assert planes.shape == (9, 4, 576, 64) and planes.is_contiguous()
    assert torch.equal(planes.view(9, 2304, 64), _run(c, 'qkv', 2304, True))
    assert ops.vit_attention_planes(planes, 3).shape == (4, 576, 192)


# ---- nothing outside the result is written ------------------------------------------------------------------------------
@pytest.mark.parametrize('layer,rows', CASES, ids=IDS)
def test_nothing_outside_the_result_is_written(layer, rows):
    """out= is a view into a larger buffer of sentinels: the guards in front of and behind it (one whole plane, or 256 rows, whichever
    is more: where a padded column 576..639 / 192..255 or a row past the last one would land) keep every byte, in both operand classes."""
    c = _case(layer)
    K, Cout, P, _, _ = LAYERS[layer]
    n = rows * Cout
    G = max(rows * (Cout // P), 256 * Cout) + 4096
    S = 7.25e11
    for split in (True, False):
        buf = torch.full((G + n + G,), S, device='cuda')
        out = buf[G:G + n].view((P, rows, Cout // P) if P > 1 else (rows, Cout))
        y = _run(c, layer, rows, split, out=out)
        assert y.data_ptr() == out.data_ptr()
        assert bool((buf[:G] == S).all()), f'{layer} @ {rows} rows split={split}: written in front of the result'
        assert bool((buf[G + n:] == S).all()), f'{layer} @ {rows} rows split={split}: written behind the result'
        assert not bool((out == S).any()), f'{layer} @ {rows} rows split={split}: an element of the result was not written'
        assert torch.equal(out, _run(c, layer, rows, split)), (layer, rows, split)
        del buf, out, y


# ---- the three forms give the same bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize('layer,rows', CASES, ids=IDS)
def test_default_launch_equals_full_height_launch(layer, rows):
    from far_amd import _lib
    lib = _lib.load()
    c = _case(layer)
    for split in (True, False):
        y = _run(c, layer, rows, split)
        lib.far_set_tuning(7, 1)
        try:
            full = _run(c, layer, rows, split)
        finally:
            lib.far_set_tuning(7, 0)
        assert torch.equal(y, full), (layer, rows, split, _form(*LAYERS[layer][:2], rows, split)[0])


@pytest.mark.parametrize('layer', list(LAYERS))
def test_rows_do_not_depend_on_the_launch_they_are_in(layer):
    """The first 2304 rows computed alone -- and the first rows of every other count, whatever form it takes -- have the bits of the same
    rows in the largest launch."""
    c = _case(layer)
    R = max(ROWS[layer])
    for split in (True, False):
        big = _run(c, layer, R, split)
        for rows in (2304,) + tuple(r for r in ROWS[layer] if r not in (2304, R)):
            assert torch.equal(_run(c, layer, rows, split), big[..., :rows, :]), (layer, rows, split)


# ---- plain fp16 operands ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layer,rows', CASES, ids=IDS)
def test_plain_fp16_sharp_and_class_bars(layer, rows):
    from far_amd import ops
    assert ops.activation_exponent_value() == ACT_EXP
    c = _case(layer)
    K, Cout, P, _, _ = LAYERS[layer]
    p64, p32 = _rounded_refs(c)
    ops.overflow_flag('cuda').zero_()
    got = _run(c, layer, rows, False)
    assert not ops.activation_overflowed('cuda')
    assert got.shape == ((P, rows, Cout // P) if P > 1 else (rows, Cout)) and got.is_contiguous()
    form = _form(K, Cout, rows, False)[0]
    name = f'linear {layer} {K}->{Cout} @ {rows} rows plain fp16 ({form})'
    _hold(name, got, p64, p32, layer, rows, False)
    gots = _run(c, layer, rows, True)
    u64 = c['r64'][:rows]
    sc = float(u64.abs().max())
    e = float((_flat(got).double() - u64).abs().max()) / sc
    es = float((_flat(gots).double() - u64).abs().max()) / sc
    print(f'[parity] {name} class: plain vs float64 {e:.3e}  split {es:.3e}  bar 3e-3')
    assert es < e < 3e-3, name
    assert not torch.equal(got, gots), name


# ---- the training pair --------------------------------------------------------------------------------------------------
TRAIN_ROWS = (2304, 1237, 24576)       # the model tests' count; ragged: linear_wgrad's h = 1 path; forward and dgrad (Cout = 192: >= 24 449) full-height


def _autograd(x, w, b, dy, dtype):
    xd, wd, bd = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    y = F.linear(xd, wd, bd)
    return (y.detach(),) + torch.autograd.grad(y, (xd, wd, bd), dy.to(dtype))


def _train_case(layer, rows):
    K, Cout, _, _, gelu = LAYERS[layer]
    g = _gen(7 * rows + Cout + K)
    x = torch.randn(rows, K, device='cuda', generator=g)
    if gelu:
        x = F.gelu(x)
    w = torch.randn(Cout, K, device='cuda', generator=g) * K ** -0.5
    b = 0.5 * torch.randn(Cout, device='cuda', generator=g)
    dy = 1e-3 * torch.randn(rows, Cout, device='cuda', generator=g)
    return x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True), dy


@pytest.mark.parametrize('rows', TRAIN_ROWS)
@pytest.mark.parametrize('layer', list(LAYERS))
def test_linear_train_against_float64_autograd(layer, rows):
    from far_amd import ops
    from far_amd.ops import conv as ops_conv
    K, Cout = LAYERS[layer][:2]
    x, w, b, dy = _train_case(layer, rows)
    r64, r32 = _autograd(x, w, b, dy, torch.float64), _autograd(x, w, b, dy, torch.float32)
    ops.overflow_flag('cuda').zero_()
    y = ops.linear_train(x, w, b, ops.PackCache(), ('train', layer))
    grads = [torch.autograd.grad(y, (x, w, b), dy, retain_graph=True) for _ in range(3)]
    assert not ops.activation_overflowed('cuda')
    name = f'linear_train {layer} {K}->{Cout} @ {rows} rows'
    for what, got, a64, a32 in zip(('y', 'dx', 'dW', 'db'), (y.detach(),) + grads[0], r64, r32):
        assert got.shape == a64.shape
        _bar(f'{name} {what}', got, a64, float((a32.double() - a64).abs().max()))
    for again in grads[1:]:                                               # three backward passes: the same bits
        for a, bb in zip(grads[0], again):
            assert torch.equal(a, bb), name
    # the weight gradient came from K16, not from the comparison leg's GEMM
    assert ops_conv.USE_HIP_WGRAD
    dw = ops.linear_wgrad(x.detach(), dy, ops.grad_scale(dy), ACT_EXP)
    assert torch.is_tensor(dw) and dw.shape == (Cout, K) and torch.equal(dw, grads[0][1]), name


@pytest.mark.parametrize('layer', ['qkv', 'fc1'])                         # dgrad at K = 576 and K = 768
def test_linear_train_scale_invariance(layer):
    """dy times 2^-20 and times 2^10: the same relative error within a factor of 2 (the rule of tests/test_conv_valid_bwd_gpu.py:
    test_scale_invariance) -- the device-side gradient scale places any magnitude in the split's window."""
    from far_amd import ops
    K, Cout = LAYERS[layer][:2]
    x, w, b, dy = _train_case(layer, 1237)
    _, dx64, dw64, _ = _autograd(x, w, b, dy, torch.float64)
    y = ops.linear_train(x, w, b, ops.PackCache(), ('train', layer))
    errs = {'dx': [], 'dW': []}
    for e in (0, -20, 10):
        s = 2.0 ** e
        dx, dw, _ = torch.autograd.grad(y, (x, w, b), dy * s, retain_graph=True)
        for what, got, ref in (('dx', dx, dx64 * s), ('dW', dw, dw64 * s)):
            errs[what].append(float((got.double() - ref).abs().max()) / float(ref.abs().max()))
            print(f'[parity] linear_train {layer} {K}->{Cout} @ 1237 rows {what}, dy x 2^{e}: relative error {errs[what][-1]:.3e}')
    for what, ee in errs.items():
        assert all(torch.isfinite(torch.tensor(ee))) and ee[0] > 0, (what, ee)
        for v in ee[1:]:
            assert ee[0] / 2 <= v <= ee[0] * 2, (what, ee)


# ---- K6 LayerNorm at C = 192 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('rows', [1, 37, 2304])
def test_layernorm_c192(rows, res):
    """ops.layernorm with the model's eps, at the bar of tests/test_fine_attn_gpu.py: test_layernorm."""
    from far_amd import ops
    C = 192
    g = _gen(C + rows + int(res))
    x = 3 * torch.randn(rows, C, device='cuda', generator=g) + 0.5
    gamma, beta = torch.rand(C, device='cuda', generator=g) + 0.5, torch.randn(C, device='cuda', generator=g)
    r = torch.randn(rows, C, device='cuda', generator=g) if res else None
    got = ops.layernorm(x, gamma, beta, LN_EPS, r)
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), LN_EPS)
    if res:
        ref = ref + r.double()
    d = (got.double() - ref).abs()
    bar = 2e-6 * float(ref.abs().max()) + 1e-5 * ref.abs()
    print(f'[parity] layernorm C=192 @ {rows} rows res={res}: max|d| {float(d.max()):.3e}  max d / bar {float((d / bar).max()):.3f}')
    assert got.shape == x.shape and bool((d <= bar).all())


@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('rows', [1, 37, 2304])
def test_layernorm_train_c192(rows, res):
    """ops.layernorm_train with the model's eps, at the bar of tests/test_train_kernels_gpu.py: test_layernorm_train_matches_float64."""
    from far_amd import ops
    C = 192
    g = _gen(2 * C + rows + int(res))
    x = (torch.randn(rows, C, device='cuda', generator=g) * 2 + 0.3).requires_grad_(True)
    r = torch.randn(rows, C, device='cuda', generator=g).requires_grad_(True) if res else None
    norm = torch.nn.LayerNorm(C, eps=LN_EPS).cuda()
    with torch.no_grad():
        norm.weight.copy_(torch.rand(C, device='cuda', generator=g) + 0.5)
        norm.bias.copy_(torch.randn(C, device='cuda', generator=g) * 0.2)
    y = ops.layernorm_train(x, norm, residual=r)
    dy = torch.randn(rows, C, device='cuda', generator=g) * 1e-3
    y.backward(dy)
    x64 = x.detach().double().requires_grad_(True)
    w64, b64 = norm.weight.detach().double().requires_grad_(True), norm.bias.detach().double().requires_grad_(True)
    y64 = F.layer_norm(x64, (C,), w64, b64, norm.eps)
    if res:
        y64 = y64 + r.detach().double()
    y64.backward(dy.double())
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    e = (rel(y.detach(), y64.detach()), rel(x.grad, x64.grad), rel(norm.weight.grad, w64.grad), rel(norm.bias.grad, b64.grad))
    print(f'[parity] layernorm_train C=192 @ {rows} rows res={res}: y {e[0]:.1e}  dx {e[1]:.1e}  dgamma {e[2]:.1e}  dbeta {e[3]:.1e}  bar 5e-6')
    assert max(e) < 5e-6
    if res:
        assert torch.equal(r.grad, dy)
    gw = norm.weight.grad.clone()
    norm.weight.grad = None
    x.grad = None
    ops.layernorm_train(x, norm, residual=r).backward(dy)
    assert torch.equal(gw, norm.weight.grad)


# ---- next to a busy stream ----------------------------------------------------------------------------------------------
def test_ten_launches_are_bit_identical_next_to_a_busy_stream():
    """qkv (nine planes) and fc2 (residual) at 36 864 rows (B = 32: full-height K9), both operand classes: 10 launches bit-identical to the
    first while a second stream runs a loop of large K9 Linear launches (the construction of tests/test_vit_attention_f16_gpu.py)."""
    from far_amd import ops
    rows = 36864
    g = _gen(6)
    big = torch.randn(1 << 17, 256, device='cuda', generator=g)
    pc = ops.PackedConv(torch.randn(256, 256, device='cuda', generator=g) / 16)
    side = torch.cuda.Stream()
    for layer in ('qkv', 'fc2'):
        K, Cout, P, has_res, gelu = LAYERS[layer]
        assert _form(K, Cout, rows, True)[0] == 'full'
        x = torch.randn(rows, K, device='cuda', generator=g)
        x = F.gelu(x) if gelu else x
        w = torch.randn(Cout, K, device='cuda', generator=g) * K ** -0.5
        b = 0.5 * torch.randn(Cout, device='cuda', generator=g)
        res = torch.randn(rows, Cout, device='cuda', generator=g) if has_res else None
        for split in (True, False):
            pack = ops.PackedConv(w, None, b, split=split)
            launch = lambda: ops.linear_f16s(x, pack, residual=res, out_planes=P)
            first = launch().clone()
            torch.cuda.synchronize()
            keep = []
            for it in range(10):
                with torch.cuda.stream(side):
                    for _ in range(4):
                        keep.append(ops.linear_f16s(big, pc))
                    del keep[:-4]
                assert torch.equal(launch(), first), f'{layer} split={split}: next to the busy stream, launch {it}'
            side.synchronize()
            torch.cuda.synchronize()
