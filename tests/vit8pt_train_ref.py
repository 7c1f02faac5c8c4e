"""The differentiable form of tests/vit8pt_ref.py's RefViTEss: forward_features there runs under torch.no_grad() (it is the yardstick of
the inference tests); training tests need the same function with a graph.  Nothing is restated: the decorated function's body is
called without its no_grad wrapper, so the two cannot drift apart."""
import torch

from tests.vit8pt_ref import RefViTEss, attention_ref


class RefViTEssTrain(RefViTEss):
    """RefViTEss whose forward_features records a graph: float64 (or fp32) torch autograd of the whole regressor."""

    def forward_features(self, features, intrinsics=None, loftr_num_corr=None, loftr_preds=None):
        return RefViTEss.forward_features.__wrapped__(self, features, intrinsics, loftr_num_corr, loftr_preds)


def from_ref(ref, dtype, device):
    """A RefViTEssTrain with the parameters and pose statistics of the RefViTEss `ref`, in `dtype` on `device`."""
    m = RefViTEssTrain(ref.args, ref.pose_mean, ref.pose_std)
    m.load_state_dict(ref.state_dict(), strict=True)
    return m.to(dtype=dtype, device=device)


def torch_core_qkv(qkv, nhead):
    """ops.vit_attention_train_qkv's function as fp32 torch autograd of the materialising composition (the comparison leg)."""
    q, k, v = qkv.chunk(3, dim=-1)
    return attention_ref(q, k, v, nhead, torch.float32)
