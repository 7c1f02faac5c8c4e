"""Seeded inputs of golden G26 (the 8-Point-ViT from images: extractor + trunk + head): ONE definition that
tools/make_golden_vit8pt_extractor.py (the reference's own ViTEss) and the tests (far_amd.vit8pt, tests/vit8pt_extractor_ref.py) both
replay.  The trunk and the head are filled by tests/vit8pt_inputs.py: seeded_fill (seed 25, G25's fill); the extractor's parameters and
buffers by extractor_fill below from a CPU generator seeded 26, in sorted-name order; the images continue that generator.

The fill keeps the extractor in a working regime (measured in float64 on tests/vit8pt_extractor_ref.py; the tool prints the figures,
tests/test_vit8pt_extractor_cpu.py asserts the bounds): every ReLU has between 0.30 and 0.85 of its outputs positive and no
activation exceeds 256 -- far inside the split-fp16 range (4094)."""
import torch

from tests import vit8pt_inputs as vi

SEED = 26
B = 2
SIZES = ((37, 53), (300, 260))          # (H, W): smaller than 224 in both directions and odd; larger and non-square
TAP_TOKENS = 6                          # the fixture keeps every 6th token ...
TAP_CHANNELS = 4                        # ... and every 4th channel of the extractor's (2B, 576, 192) output
EXTRACTOR = ('resnet.', 'extractor_final_conv.')
FINAL_NORMS = ('extractor_final_conv.norm2.', 'extractor_final_conv.norm3.')
FINAL_SCALE = 1.0 / 32                  # on their weights and biases: the block's output (max 164 without it) comes out near unit scale, where
                                        # the trunk behind it stays in the regime G25 documents (tests/vit8pt_inputs.py)
RELU_SHARE = (0.30, 0.85)
ACT_MAX = 256.0
OUTPUTS = ('tran_preds_unnorm', 'rot_preds', 'rot_preds_mtx', 'rot_preds_6d')


def extractor_entries(module):
    """(name, tensor) of the extractor's parameters and buffers in sorted-name order; the shared norm3 once (under its own name)."""
    return [(k, v) for k, v in sorted(module.state_dict().items())
            if k.startswith(EXTRACTOR) and not k.startswith('extractor_final_conv.downsample.1.') and not k.endswith('num_batches_tracked')]


def extractor_fill(module, seed=SEED):
    """Fills the extractor of a ViTEss-shaped module (the reference's or this package's) in place and returns the generator:
    convolutions randn sqrt(2 / fan_in), BatchNorm weights 1 + 0.1 randn, other 1-D parameters 0.1 randn, running_mean 0.1 randn,
    running_var 0.5 + rand; the weights and biases of extractor_final_conv.norm2 / norm3 then times FINAL_SCALE."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in extractor_entries(module):
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
            if name.startswith(FINAL_NORMS) and leaf in ('weight', 'bias'):
                v = v * FINAL_SCALE
            t.copy_(v)
    return g


def seeded_images(g, batch=B):
    """Continues extractor_fill's generator: one (batch, 2, 3, H, W) fp32 tensor of integer values 0 .. 255 per entry of SIZES."""
    return [torch.randint(0, 256, (batch, 2, 3, h, w), generator=g).float() for h, w in SIZES]


def image_intrinsics(shape, batch=B):
    """(batch, 2, 4) [fx, fy, cx, cy] AT THE IMAGE SIZE shape[-2:], chosen so that the feature grid sees about tests/util.py's
    VIT_INTRINSICS."""
    h, w = shape[-2:]
    fx, fy, cx, cy = vi.VIT_INTRINSICS
    k = torch.tensor([fx * w / 24, fy * h / 24, cx * w / 24, cy * h / 24], dtype=torch.float32)
    return k.expand(batch, 2, 4).contiguous()


def filled(model, batch=B):
    """Fills `model` (trunk: G25's fill; extractor: seed 26) -> dict(images=[per size], loftr_preds, loftr_num_corr, pose_mean,
    pose_std)."""
    inp = vi.seeded_inputs(vi.seeded_fill(model), batch)
    images = seeded_images(extractor_fill(model), batch)
    return dict(images=images, loftr_preds=inp['loftr_preds'], loftr_num_corr=inp['loftr_num_corr'], pose_mean=inp['pose_mean'],
                pose_std=inp['pose_std'])


def tap(features):
    return features[:, ::TAP_TOKENS, ::TAP_CHANNELS]
