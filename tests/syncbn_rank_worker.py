"""Child rank of tests/test_sync_batchnorm_ranks_gpu.py (not collected by pytest): torch.nn.SyncBatchNorm on K19's synchronised form across
REAL ranks.  `--mode ranks`: W ranks share cuda:0 over gloo -- (a) the operator against float64 BatchNorm over the concatenated shards,
(b) a converted ResNetFPN_8_2 against the plain-BatchNorm model on the concatenated batch.  `--mode rccl1`: one rank in an RCCL group,
the exchange forced: the float64 slot all-reduce on the real collective library must return the bits of the skipped-exchange path.
Every check asserts; the measured deviations are printed."""
import argparse
import copy
import os
import sys
from datetime import timedelta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist
import torch.nn.functional as F

from far_amd import ops
from far_amd.config import far_train_config
from far_amd.loftr.backbone import ResNetFPN_8_2

SLOPE = 0.01
OP_SHAPES = [(1, 196, 15, 20), (2, 196, 9, 11), (1, 196, 29, 37)]          # rank r's shard: unequal pixel counts (300, 198, 1073)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _say(line):
    """One write per line: the ranks share the launcher's stdout, and a newline written on its own can land behind another rank's text."""
    sys.stdout.write(line + '\n')
    sys.stdout.flush()


def _relmax(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max().clamp_min(1e-30))


def _same_bits_on_every_rank(t, rank, world, what):
    """The slot all-reduce of the operator itself: every rank's copy of `t` on every rank, then compared bit for bit."""
    buf = torch.zeros(world, t.numel(), dtype=torch.float64, device=t.device)
    buf[rank] = t.double().flatten()
    dist.all_reduce(buf, op=dist.ReduceOp.SUM)
    for r in range(world):
        assert torch.equal(buf[r], buf[rank]), f'{what}: rank {r} and rank {rank} hold different bits'


def operator_level(rank, world):
    shapes = OP_SHAPES[:world]
    C = shapes[0][1]
    cl = torch.channels_last
    xs, rs, ups = [], [], []
    for r, s in enumerate(shapes):                            # every rank can regenerate every shard: shard r comes from seed r
        g = torch.Generator(device='cuda').manual_seed(r)
        xs.append((torch.randn(*s, device='cuda', generator=g) * 1.7 + 30.0 + 5.0 * r).contiguous(memory_format=cl))
        rs.append(torch.randn(*s, device='cuda', generator=g).contiguous(memory_format=cl))
        ups.append((torch.randn(*s, device='cuda', generator=g) * 1e-3).contiguous(memory_format=cl))
    g = torch.Generator(device='cuda').manual_seed(100)
    bn = torch.nn.SyncBatchNorm(C).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=g); bn.bias.normal_(generator=g)
    # float64 reference over the concatenated batch, as (1, C, M, 1)
    cat = lambda ts: torch.cat([_rows(t) for t in ts]).double().t().reshape(1, C, -1, 1)
    ref_bn = torch.nn.BatchNorm2d(C).cuda().train().double()
    with torch.no_grad():
        ref_bn.weight.copy_(bn.weight); ref_bn.bias.copy_(bn.bias)
    xd, rd = cat(xs).requires_grad_(), cat(rs).requires_grad_()
    z = ref_bn(xd) + rd
    z.retain_grad()
    yd = torch.relu(z)
    yd.backward(cat(ups))
    xhat = (xd.detach() - xd.detach().mean(dim=(0, 2, 3), keepdim=True)) / torch.sqrt(xd.detach().var(dim=(0, 2, 3), unbiased=False, keepdim=True) + ref_bn.eps)
    counts = [s[0] * s[2] * s[3] for s in shapes]
    lo, hi = sum(counts[:rank]), sum(counts[:rank + 1])
    mine = lambda t: t[0, :, lo:hi, 0].t()
    # this rank's call
    x, res = xs[rank].clone().requires_grad_(), rs[rank].clone().requires_grad_()
    y = ops.bn_act_train(x, bn, 'relu', SLOPE, residual=res)
    assert type(y.grad_fn).__name__.startswith('_SyncBatchNormActFn'), type(y.grad_fn).__name__
    y.backward(ups[rank])
    ey = float((_rows(y.detach()).double() - mine(yd.detach())).abs().max())
    edx = float((_rows(x.grad).double() - mine(xd.grad)).abs().max() / xd.grad.abs().max())
    edg = _relmax(bn.weight.grad, (mine(z.grad) * mine(xhat)).sum(0))
    edb = _relmax(bn.bias.grad, mine(z.grad).sum(0))
    eres = float((_rows(res.grad).double() - mine(rd.grad)).abs().max())
    ybar = 3e-6 * max(float(yd.detach().abs().max()), 1.0)
    _say(f'[deviation] sync_bn ranks W={world} rank {rank} operator: y {ey:.2e} (bar {ybar:.2e}) dx {edx:.2e} dgamma {edg:.2e} dbeta {edb:.2e} dres {eres:.2e}')
    assert ey < ybar and edx < 2e-5 and edg < 2e-5 and edb < 2e-5 and eres < 1e-9
    torch.testing.assert_close(bn.running_mean.double(), ref_bn.running_mean, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(bn.running_var.double(), ref_bn.running_var, rtol=1e-5, atol=1e-6)
    assert int(bn.num_batches_tracked) == 1
    _same_bits_on_every_rank(bn.running_mean, rank, world, 'running_mean')
    _same_bits_on_every_rank(bn.running_var, rank, world, 'running_var')


def backbone_level(rank, world):
    cfg = far_train_config()['loftr']['resnetfpn']
    torch.manual_seed(0)
    plain = ResNetFPN_8_2(cfg)
    with torch.no_grad():
        for m in plain.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0.0, 0.1)
    sync = torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(plain)).cuda().train()
    plain = plain.cuda().train()
    g = torch.Generator(device='cuda').manual_seed(1)
    imgs = torch.rand(world, 1, 32, 48, device='cuda', generator=g)
    # the plain-BatchNorm model (K19 as it is) on the concatenated batch, in this process
    c_ref, f_ref = plain(imgs)
    wc, wf = torch.randn(c_ref.shape, device='cuda', generator=g), torch.randn(f_ref.shape, device='cuda', generator=g)
    ((c_ref * wc).sum() + (f_ref * wf).sum()).backward()
    # this rank's image through the converted model
    c, f = sync(imgs[rank:rank + 1])
    ((c * wc[rank:rank + 1]).sum() + (f * wf[rank:rank + 1]).sum()).backward()
    bns = [(n, m) for n, m in sync.named_modules() if isinstance(m, torch.nn.SyncBatchNorm)]
    assert len(bns) == 17
    ec, ef = _relmax(c.detach(), c_ref.detach()[rank:rank + 1]), _relmax(f.detach(), f_ref.detach()[rank:rank + 1])
    worst, worst_name = 0.0, ''
    ref_params = dict(plain.named_parameters())
    for n, p in sync.named_parameters():
        tot = p.grad.detach().clone()
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)            # the sum over ranks of each weight gradient
        e = _relmax(tot, ref_params[n].grad)
        if e > worst:
            worst, worst_name = e, n
        assert e < 1e-3, (n, e)
    ref_mods = dict(plain.named_modules())
    worst_rs = 0.0
    for i, (n, m) in enumerate(bns):
        assert int(m.num_batches_tracked) == 1 and int(ref_mods[n].num_batches_tracked) == 1, n
        if i == 0:                                             # the stem's layer: its input is the same numbers in both runs
            torch.testing.assert_close(m.running_mean, ref_mods[n].running_mean, rtol=1e-6, atol=1e-6)
            torch.testing.assert_close(m.running_var, ref_mods[n].running_var, rtol=1e-5, atol=1e-6)
        e = max(_relmax(m.running_mean, ref_mods[n].running_mean), _relmax(m.running_var, ref_mods[n].running_var))
        worst_rs = max(worst_rs, e)
        assert e < 1e-4, (n, e)
        _same_bits_on_every_rank(m.running_mean, rank, world, n + '.running_mean')
        _same_bits_on_every_rank(m.running_var, rank, world, n + '.running_var')
    _say(f'[deviation] sync_bn ranks W={world} rank {rank} backbone: coarse {ec:.2e} fine {ef:.2e} worst summed weight gradient {worst:.2e} '
          f'({worst_name}) worst running statistic {worst_rs:.2e}')
    assert ec < 1e-3 and ef < 1e-3


def rccl_world_1():
    """One rank over RCCL: the forced exchange runs the float64 slot all-reduce on the collective library; same bits as without it."""
    g = torch.Generator(device='cuda').manual_seed(3)
    cl = torch.channels_last
    shape = (2, 196, 15, 20)
    x0 = (torch.randn(*shape, device='cuda', generator=g) * 1.7 + 30.0).contiguous(memory_format=cl)
    r0 = torch.randn(*shape, device='cuda', generator=g).contiguous(memory_format=cl)
    up = (torch.randn(*shape, device='cuda', generator=g) * 1e-3).contiguous(memory_format=cl)
    base = torch.nn.SyncBatchNorm(shape[1]).cuda().train()
    with torch.no_grad():
        base.weight.uniform_(0.5, 1.5, generator=g); base.bias.normal_(generator=g)
    outs = []
    for force in (False, True):
        bn = copy.deepcopy(base)
        x, r = x0.clone().requires_grad_(), r0.clone().requires_grad_()
        y = ops.bn_act_train(x, bn, 'leaky', SLOPE, residual=r, force_exchange=force)
        assert type(y.grad_fn).__name__.startswith('_SyncBatchNormActFn' if force else '_BatchNormActFn'), type(y.grad_fn).__name__
        y.backward(up)
        outs.append((y.detach(), x.grad, r.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var, bn.num_batches_tracked))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    _say(f'[deviation] sync_bn rccl world 1: forced exchange over {dist.get_backend()} is bit-identical to the skipped one')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('ranks', 'rccl1'), required=True)
    a = ap.parse_args()
    torch.cuda.set_device(0)                                   # every rank shares cuda:0 (gloo; RCCL refuses two ranks on one device)
    dev = torch.device('cuda', 0)
    if a.mode == 'rccl1':
        dist.init_process_group('nccl', device_id=dev, timeout=timedelta(seconds=60))
    else:
        dist.init_process_group('gloo', timeout=timedelta(seconds=60))
    rank, world = dist.get_rank(), dist.get_world_size()
    ops.USE_HIP_SYNC_BATCHNORM = True
    try:
        if a.mode == 'rccl1':
            assert world == 1
            rccl_world_1()
        else:
            assert 2 <= world <= len(OP_SHAPES)
            operator_level(rank, world)
            backbone_level(rank, world)
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
