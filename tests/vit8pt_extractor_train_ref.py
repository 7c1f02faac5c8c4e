"""The yardstick of training the 8-Point-ViT extractor's final block, and the seeded case of golden G27.

RefViTEssImagesTrain is tests/vit8pt_extractor_ref.py's RefViTEssImages as far_amd.vit8pt trains it after set_extractor_training(): the
ResNet front in .eval() (running statistics) and frozen, under no_grad; the final block (FinalConv: the reference's ResidualBlock(128,
192, 'batch', kernel_size=5)) in .train() with a graph; the trunk and the head as tests/vit8pt_train_ref.py has them (forward_features
without its no_grad wrapper).  Nothing is restated: the same modules, other modes.

G27 pins FinalConv in .train() to the reference's own ResidualBlock: block_fill / block_case below are the ONE definition of its seeded
weights, input and output gradient that tools/make_golden_vit8pt_extractor_train.py (the reference's class) and
tests/test_vit8pt_extractor_train_cpu.py (FinalConv in float64) both replay; block_run is the run both make."""
import torch

from tests import vit8pt_extractor_ref as er
from tests.vit8pt_ref import RefViTEss

SEED = 27
CASE_SHAPE = (4, 128, 9, 11)            # NCHW: four images, 5 x 7 output pixels (partial tiles of K24 in both directions)
WGRAD_SLICE = (slice(None, None, 4), slice(None, None, 8))      # of every (Cout, Cin, k, k) weight gradient kept in the fixture
CONVS = ('conv1', 'conv2', 'downsample.0')
NORMS = ('norm1', 'norm2', 'norm3')


class RefViTEssImagesTrain(er.RefViTEssImages):
    def modes(self):
        """Front in .eval(), final block in .train(); only the front is frozen."""
        self.eval()
        self.extractor_final_conv.train()
        self.resnet.requires_grad_(False)
        return self

    def as_dtype(self, dtype, device=None):
        return RefViTEss.as_dtype(self, dtype, device).modes()

    def front(self, images):
        """-> the final block's input (2B, 128, 28, 28) in the parameters' dtype, no graph."""
        rn = self.resnet
        with torch.no_grad():
            x = er.normalised_input(images.to(rn.conv1.weight.device), rn.conv1.weight.dtype)
            x = rn.maxpool(torch.relu(rn.bn1(rn.conv1(x))))
            for layer in (rn.layer1, rn.layer2):
                for blk in layer:
                    x = blk(x)
        return x

    def extract_features(self, images, taps=None):
        x = self.extractor_final_conv(self.front(images), taps)
        return x.reshape(x.shape[0], 192, 576).permute(0, 2, 1)

    def forward_features(self, features, intrinsics=None, loftr_num_corr=None, loftr_preds=None):
        return RefViTEss.forward_features.__wrapped__(self, features, intrinsics, loftr_num_corr, loftr_preds)

    def forward_images(self, images, grid_intrinsics=None, loftr_num_corr=None, loftr_preds=None):
        return self.forward_features(self.extract_features(images), grid_intrinsics, loftr_num_corr, loftr_preds)


def block_entries(block):
    """(name, tensor) of a ResidualBlock-shaped module in sorted-name order; the shared norm3 once (under its own name)."""
    return [(k, v) for k, v in sorted(block.state_dict().items()) if not k.startswith('downsample.1.') and not k.endswith('num_batches_tracked')]


def block_fill(block, seed=SEED):
    """Fills the block in place and returns the generator: convolutions randn sqrt(2 / fan_in), BatchNorm weights 1 + 0.1 randn, other
    1-D parameters 0.1 randn, running_mean 0.1 randn, running_var 0.5 + rand (tests/vit8pt_extractor_inputs.py's rule)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in block_entries(block):
            leaf = name.rsplit('.', 1)[-1]
            if t.dim() == 4:
                v = torch.randn(t.shape, generator=g) * (2.0 / (t.shape[1] * t.shape[2] * t.shape[3])) ** 0.5
            elif leaf == 'running_mean':
                v = 0.1 * torch.randn(t.shape, generator=g)
            elif leaf == 'running_var':
                v = 0.5 + torch.rand(t.shape, generator=g)
            elif leaf == 'weight':
                v = 1.0 + 0.1 * torch.randn(t.shape, generator=g)
            else:
                v = 0.1 * torch.randn(t.shape, generator=g)
            t.copy_(v)
    return g


def block_case(g):
    """Continues block_fill's generator: the input (a ReLU output, as layer2's) and the output gradient, fp32 NCHW."""
    n, c, h, w = CASE_SHAPE
    x = torch.relu(torch.randn(CASE_SHAPE, generator=g)) * 1.5
    gy = torch.randn(n, 192, h - 4, w - 4, generator=g)
    return x, gy


def block_run(block, x, gy):
    """One training forward + backward of `block` (in .train(), any dtype) -> dict of recorded results, float64 numpy-ready tensors:
    the output, the input gradient, the BatchNorm and bias gradients, the updated running statistics, the slice of every weight
    gradient."""
    block.train()
    block.zero_grad(set_to_none=True)
    dt = block.conv1.weight.dtype
    X = x.to(dt).clone().requires_grad_(True)
    y = block(X)
    y.backward(gy.to(dt))
    mods = dict(block.named_modules())
    out = {'y': y.detach(), 'dx': X.grad}
    for c in CONVS:
        out[f'd_{c}.bias'] = mods[c].bias.grad
        out[f'd_{c}.weight_slice'] = mods[c].weight.grad[WGRAD_SLICE].contiguous()
    for nm in NORMS:
        out[f'd_{nm}.weight'], out[f'd_{nm}.bias'] = mods[nm].weight.grad, mods[nm].bias.grad
        out[f'{nm}.running_mean'], out[f'{nm}.running_var'] = mods[nm].running_mean.detach().clone(), mods[nm].running_var.detach().clone()
    return {k: v.detach().double().cpu() for k, v in out.items()}
