"""Run-to-run determinism of the dense-supervision kernels of the optimal-transport matcher (sinkhorn_train_f16s.hip:
far_sinkhorn_dense_focal_*), in the manner of tests/test_sinkhorn_train_determinism_gpu.py: every reduction has a fixed order and no
float atomic exists in them, so the loss and all three gradients are bit-identical over LAUNCHES + 1 calls next to a busy neighbour
stream -- at 2 x 4800 with 1500 labels per pair, unmasked and with padded masks."""
import pytest
import torch

from tests.test_determinism_gpu import LAUNCHES, _repeat
from tests.test_sinkhorn_train_determinism_gpu import HW, L, _inputs

pytestmark = pytest.mark.gpu

FOCAL = dict(alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=300.0)


def _step(f0, f1, bs, ids, masks=(None, None)):
    from far_amd import ops
    f0 = f0.detach().requires_grad_(True)
    f1 = f1.detach().requires_grad_(True)
    bs = bs.detach().requires_grad_(True)
    loss = ops.sinkhorn_dense_focal_loss(f0, f1, bs, 3, *ids, mask0=masks[0], mask1=masks[1], **FOCAL)
    loss.backward()
    return loss.detach().reshape(1), f0.grad, f1.grad, bs.grad.reshape(1)


def test_loss_and_gradients_bit_identical_next_to_a_busy_stream():
    assert LAUNCHES >= 20
    f0, f1, ids, _ = _inputs(2)
    bs = torch.tensor(1.0, device='cuda')
    first = _step(f0, f1, bs, ids)
    assert torch.isfinite(first[0]).all() and float(first[0]) > 0
    assert float(first[1].abs().max()) > 0 and float(first[2].abs().max()) > 0 and float(first[3].abs()) > 0
    _repeat(lambda: _step(f0, f1, bs, ids), 'sinkhorn dense supervision 2 x 4800')


def test_masked_batch_bit_identical():
    f0, f1, ids, _ = _inputs(2, seed=6)
    m0 = torch.zeros(2, *HW, dtype=torch.bool, device='cuda')
    m1 = torch.zeros(2, *HW, dtype=torch.bool, device='cuda')
    m0[0, :52, :80] = True; m0[1, :60, :64] = True
    m1[0, :60, :70] = True; m1[1, :48, :80] = True
    masks = (m0.reshape(2, L), m1.reshape(2, L))
    bs = torch.tensor(0.5, device='cuda')
    first = _step(f0, f1, bs, ids, masks)
    assert float(first[1][~masks[0]].abs().max()) == 0 and float(first[2][~masks[1]].abs().max()) == 0
    _repeat(lambda: _step(f0, f1, bs, ids, masks), 'sinkhorn dense supervision 2 x 4800, padded masks')
