"""float64 reference of LoFTREncoderLayer under training, and the inputs it is compared on -- TEST INFRASTRUCTURE (no test in here;
tests/test_encoder_layer_train_cpu.py pins it against tests/vendor_ops.py, tests/test_encoder_layer_train_gpu.py holds the HIP
training path to it).

`layer_forward` restates mp3d_loftr/src/loftr/loftr_module/transformer.py:44-67 on explicit tensors (no module): three F.linear
projections, tests.vendor_ops.linear_attention (with optional masks), merge + F.layer_norm, cat([x, n1]) -> F.linear -> ReLU ->
F.linear -> F.layer_norm, x + message.  It also returns the hidden PRE-activation, because the inputs are chosen by it:

ReLU margin.  A hidden unit whose pre-activation lies within rounding of zero gets a different ReLU mask in two evaluations of
the same layer, and one such unit moves every gradient behind it by far more than either evaluation's own error.  At the small
shapes used here (1k - 34k hidden units) inputs without such a unit exist: `draw_layer` / `draw_stack` return the first draw d
in range(32) (seed base + d) whose float64 pre-activations all satisfy  min|pre| > 2^-18 max|pre|  (3.8e-6 relative: over ten
times the 3e-7 by which a kernel call of the path deviates from float64), and raise if there is none.  The margin is a condition
on the inputs, not a tolerance on the result.

All draws come from numpy.random.default_rng(seed) on the CPU: N(0, 1) activations, Xavier-uniform weights, LayerNorm weights
1 + 0.1 N(0, 1) and biases 0.1 N(0, 1) (so that dgamma / dbeta are not trivial), upstream gradients 1e-3 N(0, 1); every tensor is
rounded to fp32 once, and the reference reads exactly those fp32 values as float64.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import vendor_ops

# state_dict names of a LoFTREncoderLayer's parameters, in Module.parameters() order
PARAMS = ('q_proj.weight', 'k_proj.weight', 'v_proj.weight', 'merge.weight', 'mlp.0.weight', 'mlp.2.weight',
          'norm1.weight', 'norm1.bias', 'norm2.weight', 'norm2.bias')
LN_EPS, ATTN_EPS = 1e-5, 1e-6            # nn.LayerNorm's and LinearAttention's defaults
MARGIN = 2.0 ** -18
DRAWS = 32


def layer_forward(x, source, w, nhead, x_mask=None, source_mask=None):
    """transformer.py:44-67 on explicit tensors of one dtype; w: {PARAMS name: tensor}.  -> (y, pre) with pre the hidden
    pre-activation mlp[0](cat[x, norm1(merge(message))]) (before the ReLU)."""
    C = x.shape[-1]
    q, k, v = F.linear(x, w['q_proj.weight']), F.linear(source, w['k_proj.weight']), F.linear(source, w['v_proj.weight'])
    msg = vendor_ops.linear_attention(q, k, v, nhead, x_mask, source_mask, ATTN_EPS)
    n1 = F.layer_norm(F.linear(msg, w['merge.weight']), (C,), w['norm1.weight'], w['norm1.bias'], LN_EPS)
    pre = F.linear(torch.cat([x, n1], dim=2), w['mlp.0.weight'])
    m2 = F.layer_norm(F.linear(torch.relu(pre), w['mlp.2.weight']), (C,), w['norm2.weight'], w['norm2.bias'], LN_EPS)
    return x + m2, pre


def _f64_leaf(t):
    return t.detach().double().clone().requires_grad_(True)


def layer_reference(x, source, w, nhead, g, x_mask=None, source_mask=None):
    """float64 forward + autograd of one layer call; source None = self-attention (source is x).
    -> {'y', 'pre', 'dx', 'dsource' (absent for self-attention), 'd' + name for the ten parameters}, all float64."""
    xd = _f64_leaf(x)
    sd = None if source is None else _f64_leaf(source)
    wd = {k: _f64_leaf(w[k]) for k in PARAMS}
    y, pre = layer_forward(xd, xd if sd is None else sd, wd, nhead, x_mask, source_mask)
    y.backward(g.double())
    out = {'y': y.detach(), 'pre': pre.detach(), 'dx': xd.grad}
    if sd is not None:
        out['dsource'] = sd.grad
    out.update({'d' + k: wd[k].grad for k in PARAMS})
    return out


def stack_forward(feat0, feat1, ws, names, nhead, mask0=None, mask1=None):
    """LocalFeatureTransformer.forward in the reference's order (transformer.py:99-110): 'self' = the layer on each image;
    'cross' = feat0 from feat1, then feat1 from the UPDATED feat0; one weight set per layer, shared by its two calls.
    -> (feat0, feat1, [pre of every layer call])."""
    pres = []
    for w, name in zip(ws, names):
        if name == 'self':
            feat0, p0 = layer_forward(feat0, feat0, w, nhead, mask0, mask0)
            feat1, p1 = layer_forward(feat1, feat1, w, nhead, mask1, mask1)
        elif name == 'cross':
            feat0, p0 = layer_forward(feat0, feat1, w, nhead, mask0, mask1)
            feat1, p1 = layer_forward(feat1, feat0, w, nhead, mask1, mask0)
        else:
            raise KeyError(name)
        pres += [p0, p1]
    return feat0, feat1, pres


def stack_reference(feat0, feat1, ws, names, nhead, g0, g1, mask0=None, mask1=None):
    """float64 forward + autograd of the stack with upstream gradients on both outputs.
    -> {'feat0', 'feat1', 'dfeat0', 'dfeat1', 'dlayers.<i>.<name>' for every parameter, 'pres'}."""
    f0, f1 = _f64_leaf(feat0), _f64_leaf(feat1)
    wd = [{k: _f64_leaf(w[k]) for k in PARAMS} for w in ws]
    y0, y1, pres = stack_forward(f0, f1, wd, names, nhead, mask0, mask1)
    torch.autograd.backward([y0, y1], [g0.double(), g1.double()])
    out = {'feat0': y0.detach(), 'feat1': y1.detach(), 'dfeat0': f0.grad, 'dfeat1': f1.grad, 'pres': [p.detach() for p in pres]}
    for i, w in enumerate(wd):
        out.update({f'dlayers.{i}.{k}': w[k].grad for k in PARAMS})
    return out


def relu_margin_ok(pres):
    """min|pre| > 2^-18 max|pre| over every given pre-activation tensor (each layer call on its own scale)."""
    return all(float(p.abs().min()) > MARGIN * float(p.abs().max()) for p in pres)


def prefix_mask(lengths, L):
    """(len(lengths), L) bool, row i valid on [0, lengths[i]): padding as the data loader produces it."""
    return torch.arange(L)[None, :] < torch.tensor(lengths)[:, None]


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _draw_weights(rng, C):
    def xavier(o, i):
        b = (6.0 / (i + o)) ** 0.5
        return _f32(rng.uniform(-b, b, size=(o, i)))
    w = {'q_proj.weight': xavier(C, C), 'k_proj.weight': xavier(C, C), 'v_proj.weight': xavier(C, C), 'merge.weight': xavier(C, C),
         'mlp.0.weight': xavier(2 * C, 2 * C), 'mlp.2.weight': xavier(C, 2 * C)}
    for n in ('norm1', 'norm2'):
        w[n + '.weight'] = _f32(1.0 + 0.1 * rng.standard_normal(C))
        w[n + '.bias'] = _f32(0.1 * rng.standard_normal(C))
    return w


def _one_layer_draw(seed, bs, L, S, C, self_attn):
    rng = np.random.default_rng(seed)
    x = _f32(rng.standard_normal((bs, L, C)))
    source = None if self_attn else _f32(rng.standard_normal((bs, S, C)))
    w = _draw_weights(rng, C)
    g = _f32(1e-3 * rng.standard_normal((bs, L, C)))
    return {'x': x, 'source': source, 'w': w, 'g': g}


def draw_layer(case, base, x_mask=None, source_mask=None):
    """case = (bs, L, S, C, nhead, self_attn).  -> ({'x', 'source' (None for self-attention), 'w', 'g'} as fp32 CPU tensors, d):
    the first draw d (seed base + d) that keeps the ReLU margin under the given masks."""
    bs, L, S, C, nhead, self_attn = case
    assert not self_attn or L == S
    for d in range(DRAWS):
        inp = _one_layer_draw(base + d, bs, L, S, C, self_attn)
        with torch.no_grad():
            xd = inp['x'].double()
            sd = xd if self_attn else inp['source'].double()
            _, pre = layer_forward(xd, sd, {k: t.double() for k, t in inp['w'].items()}, nhead, x_mask, source_mask)
        if relu_margin_ok([pre]):
            return inp, d
    raise RuntimeError(f'no draw in range({DRAWS}) from seed {base} keeps the ReLU margin for {case}')


def draw_stack(n, L0, L1, C, nhead, names, base, mask0=None, mask1=None):
    """-> ({'feat0', 'feat1', 'ws' (one weight dict per layer), 'g0', 'g1'}, d): the first draw whose EVERY layer call keeps the
    ReLU margin."""
    for d in range(DRAWS):
        rng = np.random.default_rng(base + d)
        inp = {'feat0': _f32(rng.standard_normal((n, L0, C))), 'feat1': _f32(rng.standard_normal((n, L1, C))),
               'ws': [_draw_weights(rng, C) for _ in names]}
        inp['g0'] = _f32(1e-3 * rng.standard_normal((n, L0, C)))
        inp['g1'] = _f32(1e-3 * rng.standard_normal((n, L1, C)))
        with torch.no_grad():
            _, _, pres = stack_forward(inp['feat0'].double(), inp['feat1'].double(),
                                       [{k: t.double() for k, t in w.items()} for w in inp['ws']], names, nhead, mask0, mask1)
        if relu_margin_ok(pres):
            return inp, d
    raise RuntimeError(f'no draw in range({DRAWS}) from seed {base} keeps the ReLU margin for the stack {(n, L0, L1, C, nhead, names)}')


def rel_fro(a, ref):
    """relative Frobenius error of a against the float64 tensor ref."""
    return float((a.detach().double().cpu() - ref).norm() / ref.norm())
