"""The yardstick of K12's training tests: a materialising torch restatement of the Map-free aggregator in FAR's configuration
(mapfree_6dreg/lib/models/regression/aggregator.py:42-116: POSITION_ENCODER, MAX_SCORE_CHANNEL, nothing else), differentiated by
autograd in the dtype of its inputs (float64: the reference of every bar; fp32 on the same device: dev32).  Outside far_amd on purpose.

The max-score channel is taken at an EXPLICIT arg-max, the lowest column index among equal maxima, found on the CPU: the scores that
decide it are accumulated channel by channel with elementwise operations, so two identical vol1 columns give identical bits whatever
the BLAS does with its tiles.  With that index the channel is gather(softmax, j*), whose gradient flows to j* alone."""
import numpy as np
import torch

MIN_GAP = 1e-4        # the input condition of the parity cases: each row's two largest float64 scores differ by at least this


def grid(H, W, dtype, device):
    u = torch.linspace(-1, 1, H, dtype=dtype, device=device)
    v = torch.linspace(-1, 1, W, dtype=dtype, device=device)
    uu, vv = torch.meshgrid(u, v, indexing='ij')
    return torch.stack([uu, vv], dim=0).view(2, H * W)


def scores_elementwise(vol0, vol1):
    """x[b, i, j] = sum_c vol0[b, c, i] vol1[b, c, j], channel after channel: every element by the same sequence of operations."""
    B, D, H, W = vol0.shape
    a, b = vol0.detach().reshape(B, D, H * W), vol1.detach().reshape(B, D, H * W)
    x = torch.zeros(B, H * W, H * W, dtype=a.dtype, device=a.device)
    for c in range(D):
        x.addcmul_(a[:, c, :, None], b[:, c, None, :])
    return x


def argmax_first(vol0, vol1):
    """(B, HW) int64 on the CPU: the lowest index among each row's equal maxima, written out."""
    x = scores_elementwise(vol0, vol1).cpu()
    HW = x.shape[-1]
    top = x.max(dim=-1, keepdim=True).values
    idx = torch.arange(HW).expand_as(x)
    return torch.where(x == top, idx, torch.full_like(idx, HW)).min(dim=-1).values


def min_gap(vol0, vol1, rows=None):
    """The smallest difference between a row's two largest float64 scores (over `rows`: a (B, HW) boolean mask)."""
    x = scores_elementwise(vol0.double(), vol1.double())
    top2 = torch.topk(x, 2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]
    if rows is not None:
        gap = gap[rows.to(gap.device)]
    return float(gap.min())


def aggregate(vol0, vol1, jstar=None):
    """CorrelationVolumeWarping.forward, materialising the (B, HW, HW) softmax as the reference does."""
    B, D, H, W = vol0.shape
    a, b = vol0.reshape(B, D, H * W), vol1.reshape(B, D, H * W)
    cvolume = torch.softmax(torch.bmm(a.transpose(1, 2), b), dim=2)
    vol1w = torch.bmm(b, cvolume.transpose(1, 2))
    g = grid(H, W, a.dtype, a.device).unsqueeze(0).repeat(B, 1, 1)
    pos_encoder = torch.bmm(g, cvolume.transpose(1, 2))
    if jstar is None:
        jstar = argmax_first(vol0, vol1)
    max_score = torch.gather(cvolume, 2, jstar.to(a.device)[..., None]).transpose(1, 2)
    return torch.cat([a, vol1w, pos_encoder, max_score], dim=1).view(B, -1, H, W)


def grads(vol0, vol1, dagg, dtype, device='cpu', jstar=None):
    """numpy or torch inputs -> (agg, dvol0, dvol1) of the restatement in `dtype` on `device` (detached)."""
    t = lambda x: torch.as_tensor(x).to(device=device, dtype=dtype)
    v0, v1 = t(vol0).requires_grad_(True), t(vol1).requires_grad_(True)
    agg = aggregate(v0, v1, jstar)
    d0, d1 = torch.autograd.grad(agg, (v0, v1), t(dagg))
    return agg.detach(), d0, d1


# ---- the parity cases: inputs amp * default_rng(seed).standard_normal(shape), vol0 then vol1, then dagg from the same generator with the
# max-score channel scaled by 4 (its term would otherwise be lost under the others)
CASES = {
    'flat': ((3, 32, 23, 17), 0.5, 5),          # HW = 391: four row blocks, 13 column tiles with a tail of 7, three pairs
    'peaked': ((3, 32, 23, 17), 2.0, 6),        # score range ~ 240: near-one-hot rows, p underflowing off the peak
    'tiny': ((2, 32, 7, 5), 0.5, 7),            # HW = 35: one partial row block, a 3-column tail
    'two-block': ((1, 32, 12, 11), 1.0, 8),     # HW = 132: a 4-row second block
    'full': ((1, 32, 92, 68), 0.5, 9),          # the model's own grid, once
}


def case_inputs(name):
    shape, amp, seed = CASES[name]
    rng = np.random.default_rng(seed)
    v0 = (amp * rng.standard_normal(shape)).astype(np.float32)
    v1 = (amp * rng.standard_normal(shape)).astype(np.float32)
    dagg = rng.standard_normal((shape[0], 67) + shape[2:]).astype(np.float32)
    dagg[:, 66] *= 4
    return v0, v1, dagg
