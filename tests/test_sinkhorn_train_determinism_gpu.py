"""Run-to-run determinism of the optimal-transport matcher's training kernels (sinkhorn_train_f16s.hip), in the manner of
tests/test_determinism_gpu.py: every reduction has a fixed order and no float atomic exists in them, so the forward outputs and
all three gradients are bit-identical over LAUNCHES + 1 calls next to a busy neighbour stream, and a pair's results do not depend
on what else is in the batch."""
import pytest
import torch

from tests.test_determinism_gpu import LAUNCHES, _repeat

pytestmark = pytest.mark.gpu

C = 256
HW = (60, 80)
L = HW[0] * HW[1]


def _inputs(N, seed=5, per_pair=1500):
    g = torch.Generator(device='cuda').manual_seed(seed)
    f0 = 3.75 * torch.randn(N, L, C, device='cuda', generator=g)
    perm = torch.stack([torch.randperm(L, device='cuda', generator=g) for _ in range(N)])
    f1 = torch.gather(f0, 1, perm[:, :, None].expand(N, L, C)) + 0.1 * torch.randn(N, L, C, device='cuda', generator=g)
    # f1[n, k] = f0[n, perm[n, k]]: ground truth (i = perm[n, k], j = k); plus off-pairs that share rows with it, in mixed order
    k = torch.stack([torch.randperm(L, device='cuda', generator=g)[:per_pair] for _ in range(N)])
    b = torch.arange(N, device='cuda')[:, None].expand(N, per_pair)
    i = torch.gather(perm, 1, k)
    j = k.clone()
    j[:, ::10] = torch.randint(0, L, j[:, ::10].shape, device='cuda', generator=g)
    order = torch.randperm(N * per_pair, device='cuda', generator=g)
    ids = tuple(x.reshape(-1)[order].contiguous() for x in (b, i, j))
    w = [1e-4 * torch.randn(s, device='cuda', generator=g) for s in ((N * per_pair,), (N, L), (N, L))]
    return f0, f1, ids, w


def _step(f0, f1, bs, ids, w, masks=(None, None)):
    from far_amd import ops
    f0 = f0.detach().requires_grad_(True)
    f1 = f1.detach().requires_grad_(True)
    bs = bs.detach().requires_grad_(True)
    pos, bin0, bin1 = ops.sinkhorn_pos_conf(f0, f1, bs, 3, *ids, *masks)
    ((pos * w[0]).sum() + (bin0 * w[1]).sum() + (bin1 * w[2]).sum()).backward()
    return pos.detach(), bin0.detach(), bin1.detach(), f0.grad, f1.grad, bs.grad.reshape(1)


def test_forward_and_gradients_bit_identical_next_to_a_busy_stream():
    assert LAUNCHES >= 20
    f0, f1, ids, w = _inputs(2)
    bs = torch.tensor(1.0, device='cuda')
    first = _step(f0, f1, bs, ids, w)
    assert float(first[3].abs().max()) > 0 and float(first[4].abs().max()) > 0 and float(first[5].abs()) > 0
    _repeat(lambda: _step(f0, f1, bs, ids, w), 'sinkhorn training 2 x 4800')


def test_masked_batch_bit_identical():
    f0, f1, ids, w = _inputs(2, seed=6)
    m0 = torch.zeros(2, *HW, dtype=torch.bool, device='cuda')
    m1 = torch.zeros(2, *HW, dtype=torch.bool, device='cuda')
    m0[0, :52, :80] = True; m0[1, :60, :64] = True
    m1[0, :60, :70] = True; m1[1, :48, :80] = True
    masks = (m0.reshape(2, L), m1.reshape(2, L))
    bs = torch.tensor(0.5, device='cuda')
    _repeat(lambda: _step(f0, f1, bs, ids, w, masks), 'sinkhorn training 2 x 4800, padded masks')


def test_a_pair_does_not_depend_on_the_rest_of_the_batch():
    """Pair 0 alone, and pair 0 in a batch of three with its positions interleaved with the others': the same bits for everything
    that belongs to pair 0 (d bin_score is a sum over the batch: compared on the single-pair calls)."""
    f0, f1, ids, w = _inputs(3, seed=7, per_pair=700)
    bs = torch.tensor(1.0, device='cuda')
    full = _step(f0, f1, bs, ids, w)
    sel = ids[0] == 0
    alone = _step(f0[:1].contiguous(), f1[:1].contiguous(), bs, tuple(x[sel].contiguous() for x in ids),
                  [w[0][sel].contiguous(), w[1][:1].contiguous(), w[2][:1].contiguous()])
    assert torch.equal(full[0][sel], alone[0])
    for k in (1, 2, 3, 4):
        assert torch.equal(full[k][:1], alone[k]), k
