"""K19's synchronised form (torch.nn.SyncBatchNorm on the HIP kernels) in ONE process: shards of a batch stand in for ranks and the five
collective-free stages (ops.sync_bn_moments / _stats / _apply / _bwd_sums / _bwd_dx) are chained by hand, the stacked float64 records
taking the place of the all-reduce.  Reference: float64 autograd of nn.BatchNorm2d (training mode) + activation + residual over the
CONCATENATED batch -- what SyncBatchNorm is by definition.  The bars are K19's own
(test_train_kernels_gpu.py::test_batchnorm_train_matches_float64_autograd_and_the_module): the arithmetic is K19's with one more level
of float64 addition.

Inputs as in K19's test (mean ~ 30, sigma ~ 1.7: a careless variance cancels), and shard r is offset by 5 r: averaging per-rank
variances instead of combining the moments fails visibly."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SLOPE = 0.01
# (shard shapes, activation, residual): the smallest shapes at which each piece can go wrong
CASES = {
    'c4_unequal': ([(1, 4, 1, 3), (1, 4, 1, 2)], 'relu', False),                # one vector column, fewer pixels than side-by-side rows
    'c196_res': ([(1, 196, 15, 20), (2, 196, 15, 20)], 'relu', True),           # 49 vector columns: idle lanes; channel tail of the finalize grid
    'c256_ranges': ([(1, 256, 29, 37), (2, 256, 8, 10)], 'leaky', False),       # 1073 pixels: three ranges with a short last one; 160: one range
    'three_ranks': ([(1, 128, 12, 16)] * 3, 'none', False),                     # odd W
    'eight_ranks': ([(1, 64, 6, 8)] * 8, 'relu', False),                        # the reference's rank count
}
_ACTS = {'relu': torch.relu, 'leaky': lambda t: F.leaky_relu(t, SLOPE), 'none': lambda t: t}
_cache = {}


def _rows(t):
    """(N, C, H, W) -> [M][C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _case(name):
    """Inputs and the float64 reference of one case, computed once and shared (never modified) by the tests below."""
    if name in _cache:
        return _cache[name]
    shapes, act, res = CASES[name]
    C = shapes[0][1]
    g = torch.Generator(device='cuda').manual_seed(C + 7 * len(shapes))
    cl = torch.channels_last
    xs = [(torch.randn(*s, device='cuda', generator=g) * 1.7 + 30.0 + 5.0 * r).contiguous(memory_format=cl) for r, s in enumerate(shapes)]
    rs = [torch.randn(*s, device='cuda', generator=g).contiguous(memory_format=cl) for s in shapes] if res else [None] * len(shapes)
    ups = [(torch.randn(*s, device='cuda', generator=g) * 1e-3).contiguous(memory_format=cl) for s in shapes]
    weight = torch.empty(C, device='cuda').uniform_(0.5, 1.5, generator=g)
    bias = torch.empty(C, device='cuda').normal_(generator=g)
    # the concatenated batch as (1, C, M, 1): the shards of one case may differ in H x W, BatchNorm2d only sees pixels
    cat = lambda ts: torch.cat([_rows(t) for t in ts]).double().t().reshape(1, C, -1, 1)
    ref_bn = torch.nn.BatchNorm2d(C).cuda().train().double()
    with torch.no_grad():
        ref_bn.weight.copy_(weight); ref_bn.bias.copy_(bias)
    xd = cat(xs).requires_grad_()
    rd = cat(rs).requires_grad_() if res else None
    z = ref_bn(xd) + (rd if res else 0)
    z.retain_grad()
    yd = _ACTS[act](z)
    yd.backward(cat(ups))
    # per-shard dgamma / dbeta: float64 sums over the shard's own pixels with the GLOBAL statistics
    mean = xd.detach().mean(dim=(0, 2, 3), keepdim=True)
    var = xd.detach().var(dim=(0, 2, 3), unbiased=False, keepdim=True)
    xhat = (xd.detach() - mean) / torch.sqrt(var + ref_bn.eps)
    counts = [s[0] * s[2] * s[3] for s in shapes]
    offs = [sum(counts[:r]) for r in range(len(shapes) + 1)]
    sl = lambda t, r: t[0, :, offs[r]:offs[r + 1], 0].t()                      # the rows of shard r, [M_r][C]
    ref = dict(y=[sl(yd.detach(), r) for r in range(len(shapes))], dx=[sl(xd.grad, r) for r in range(len(shapes))],
               dres=[sl(rd.grad, r) for r in range(len(shapes))] if res else None,
               dgamma=[(sl(z.grad, r) * sl(xhat, r)).sum(0) for r in range(len(shapes))], dbeta=[sl(z.grad, r).sum(0) for r in range(len(shapes))],
               rm=ref_bn.running_mean.clone(), rv=ref_bn.running_var.clone(), yscale=float(yd.detach().abs().max()), dxscale=float(xd.grad.abs().max()))
    _cache[name] = dict(xs=xs, rs=rs, ups=ups, weight=weight, bias=bias, act=act, res=res, C=C, ref=ref, eps=ref_bn.eps, momentum=ref_bn.momentum)
    return _cache[name]


def _chain(c, stack=None):
    """The five stages by hand.  stack(records) -> (W, K, C): how the exchange buffer is assembled (default: every rank writes its slot)."""
    from far_amd import ops
    W, C, act = len(c['xs']), c['C'], c['act']
    dev = c['xs'][0].device
    if stack is None:
        recs = torch.zeros(W, 3, C, dtype=torch.float64, device=dev)
        for r, x in enumerate(c['xs']):
            ops.sync_bn_moments(x, out=recs[r])
    else:
        recs = stack([ops.sync_bn_moments(x) for x in c['xs']])
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    vec = ops.sync_bn_stats(recs, c['weight'], c['bias'], c['eps'], c['momentum'], rm, rv)
    ys = [ops.sync_bn_apply(x, vec, act, SLOPE, r) for x, r in zip(c['xs'], c['rs'])]
    if stack is None:
        recb = torch.zeros(W, 2, C, dtype=torch.float64, device=dev)
        sums = [ops.sync_bn_bwd_sums(x, up, y, vec, act, SLOPE, out=recb[r]) for r, (x, up, y) in enumerate(zip(c['xs'], c['ups'], ys))]
    else:
        sums = [ops.sync_bn_bwd_sums(x, up, y, vec, act, SLOPE) for x, up, y in zip(c['xs'], c['ups'], ys)]
        recb = stack([s[0] for s in sums])
    back = [ops.sync_bn_bwd_dx(x, up, y, vec, c['weight'], recb, act, SLOPE, want_dres=c['res']) for x, up, y in zip(c['xs'], c['ups'], ys)]
    out = dict(y=ys, dx=[b[0] for b in back], dgamma=[s[1] for s in sums], dbeta=[s[2] for s in sums], rm=rm, rv=rv, vec=vec, recs=recs, recb=recb)
    if c['res']:
        out['dres'] = [b[1] for b in back]
    return out


def _flat(o):
    return [t for k in sorted(o) for t in (o[k] if isinstance(o[k], list) else [o[k]])]


@pytest.mark.parametrize('name', list(CASES))
def test_shards_as_ranks_match_float64_batchnorm_over_the_concatenated_batch(name):
    c = _case(name)
    ref = c['ref']
    outs = [_chain(c) for _ in range(3)]
    o = outs[0]
    tag = f'[deviation] sync_bn {name}'
    for r in range(len(c['xs'])):
        ey = float((_rows(o['y'][r]).double() - ref['y'][r]).abs().max())
        edx = float((_rows(o['dx'][r]).double() - ref['dx'][r]).abs().max()) / max(ref['dxscale'], 1e-30)
        edg = float((o['dgamma'][r].double() - ref['dgamma'][r]).abs().max() / ref['dgamma'][r].abs().max().clamp_min(1e-30))
        edb = float((o['dbeta'][r].double() - ref['dbeta'][r]).abs().max() / ref['dbeta'][r].abs().max().clamp_min(1e-30))
        print(f'{tag} shard {r}: y {ey:.2e} (bar {3e-6 * max(ref["yscale"], 1.0):.2e}) dx {edx:.2e} dgamma {edg:.2e} dbeta {edb:.2e}')
        assert ey < 3e-6 * max(ref['yscale'], 1.0), (r, ey)
        assert edx < 2e-5, (r, edx)
        assert edg < 2e-5, (r, edg)
        assert edb < 2e-5, (r, edb)
        if c['res']:
            assert float((_rows(o['dres'][r]).double() - ref['dres'][r]).abs().max()) < 1e-9
    torch.testing.assert_close(o['rm'].double(), ref['rm'], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(o['rv'].double(), ref['rv'], rtol=1e-5, atol=1e-6)
    for other in outs[1:]:                                     # three repeats: bit-identical
        assert all(torch.equal(a, b) for a, b in zip(_flat(other), _flat(o)))


@pytest.mark.parametrize('name', ['c256_ranges', 'three_ranks'])
def test_the_stacked_records_are_the_only_input_whatever_assembled_them(name):
    """The exchange is a sum of W zeroed buffers in which each rank filled its slot.  Whatever order they are added in (every rank's own
    buffer comes first on that rank), the stacked records carry the same bytes, and so does everything computed from them."""
    c = _case(name)
    base = _chain(c)
    W = len(c['xs'])

    def reduce_in(order):
        def stack(records):
            bufs = []
            for r, rec in enumerate(records):
                b = torch.zeros(W, *rec.shape, dtype=torch.float64, device=rec.device)
                b[r] = rec
                bufs.append(b)
            acc = bufs[order[0]].clone()
            for r in order[1:]:
                acc += bufs[r]
            return acc
        return stack

    for order in (list(range(W)), list(range(W))[::-1], [(r + 1) % W for r in range(W)]):
        o = _chain(c, stack=reduce_in(order))
        assert all(torch.equal(a, b) for a, b in zip(_flat(o), _flat(base))), order


@pytest.mark.parametrize('shape,act,res', [((2, 196, 15, 20), 'relu', True), ((1, 256, 29, 37), 'leaky', False), ((1, 4, 1, 3), 'relu', False)])
def test_one_rank_through_the_sync_stages_is_plain_k19_bit_for_bit(shape, act, res):
    from far_amd import ops
    N, C, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(C + H)
    cl = torch.channels_last
    x = (torch.randn(*shape, device='cuda', generator=g) * 1.7 + 30.0).contiguous(memory_format=cl).requires_grad_()
    r = torch.randn(*shape, device='cuda', generator=g).contiguous(memory_format=cl).requires_grad_() if res else None
    up = (torch.randn(*shape, device='cuda', generator=g) * 1e-3).contiguous(memory_format=cl)
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=g); bn.bias.normal_(generator=g)
        bn.running_mean.normal_(generator=g); bn.running_var.uniform_(0.5, 2.0, generator=g)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    y = ops.bn_act_train(x, bn, act, SLOPE, residual=r)
    y.backward(up)
    rec = ops.sync_bn_moments(x)[None]
    assert float(rec[0, 0, 0]) == N * H * W
    vec = ops.sync_bn_stats(rec, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum, rm, rv)
    ys = ops.sync_bn_apply(x, vec, act, SLOPE, r)
    recb, dg, db = ops.sync_bn_bwd_sums(x, up, ys, vec, act, SLOPE)
    dx, dres = ops.sync_bn_bwd_dx(x, up, ys, vec, bn.weight.detach(), recb[None], act, SLOPE, want_dres=res)
    assert torch.equal(ys, y.detach()) and torch.equal(dx, x.grad)
    assert torch.equal(dg, bn.weight.grad) and torch.equal(db, bn.bias.grad)
    assert torch.equal(rm, bn.running_mean) and torch.equal(rv, bn.running_var)
    if res:
        assert torch.equal(dres, r.grad)


def test_sync_module_at_world_size_1_takes_the_plain_path_and_empty_shards_raise():
    """Without a process group the switched-on SyncBatchNorm call issues no collective and is the plain call: the bits of a BatchNorm2d
    with the same state; num_batches_tracked advances; an empty shard raises instead of falling back to the module."""
    from far_amd import _lib, ops
    g = torch.Generator(device='cuda').manual_seed(5)
    x = (torch.randn(2, 64, 6, 8, device='cuda', generator=g) + 3.0).requires_grad_()
    up = torch.randn(2, 64, 6, 8, device='cuda', generator=g)
    plain = torch.nn.BatchNorm2d(64).cuda().train()
    sync = torch.nn.SyncBatchNorm.convert_sync_batchnorm(torch.nn.Sequential(torch.nn.BatchNorm2d(64))).cuda().train()[0]
    assert type(sync) is torch.nn.SyncBatchNorm and ops.USE_HIP_SYNC_BATCHNORM is False
    ops.USE_HIP_SYNC_BATCHNORM = True
    try:
        ya = ops.bn_act_train(x, plain, 'relu')
        ya.backward(up)
        dxa, x.grad = x.grad, None
        yb = ops.bn_act_train(x, sync, 'relu')
        assert type(yb.grad_fn).__name__.startswith('_BatchNormActFn')
        yb.backward(up)
        assert torch.equal(ya, yb) and torch.equal(dxa, x.grad) and torch.equal(plain.weight.grad, sync.weight.grad)
        assert torch.equal(plain.running_var, sync.running_var) and int(sync.num_batches_tracked) == 1
        with pytest.raises(_lib.FarHipError):
            ops.bn_act_train(x[:0], sync, 'relu')
    finally:
        ops.USE_HIP_SYNC_BATCHNORM = False
