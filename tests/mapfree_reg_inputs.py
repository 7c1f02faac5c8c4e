"""Seeded inputs of golden G28 (the Map-free regressor: ResUNet encoder, K12 aggregator, DeepResBlock head, TransformerEncoder, gate): ONE
definition that tools/make_golden_mapfree_reg.py (the reference's own classes) and the tests (far_amd.mapfree.RegressionModel,
tests/mapfree_reg_ref.py) both replay.  Everything comes from CPU generators: the parameters and buffers from one seeded 28, in
sorted-name order; the images, loftr_rt and inliers from one seeded 2028.

The fill keeps the model in a working regime (conditions, asserted by the tool on the reference's own CPU run and printed):
  * after every ReLU and ELU the positive share is within RELU_SHARE;
  * every activation is inside the split-fp16 range at the default activation exponent (ACT_MAX);
  * K12's max-score channel has its median within MAX_SCORE (the softmax is neither uniform nor one-hot);
  * both gate weights are within GATE for every pair (both experts reach R and t);
  * the translation-norm ratio lies inside its clamps for at least one pair and outside for at least one.
"""
import types

import torch

SEED, INPUT_SEED = 28, 2028
B = 2
SIZE = (360, 270)                       # DATASET.HEIGHT x WIDTH: the smallest class of sizes the hard-wired 12 x 9 grid admits
VOLUME = (92, 68)
TAP_VOL = (7, 5)                        # the fixture keeps every 7th row / 5th column of the (2B, 32, 92, 68) encoder volumes ...
TAP_X3_CH = 4                           # ... and every 4th channel of x3 (B, 256, 12, 9)
RELU_SHARE = (0.2, 0.8)
ACT_MAX = 65504.0 / 16
MAX_SCORE = (0.02, 0.9)
GATE = (0.05, 0.95)
CLAMP = (1e-2, 1e2)

# fill scales (chosen so that the conditions above hold; the tool prints the figures)
OUTCONV_GAIN = 0.35                     # on outconv.normalize's weight and bias: K12's scores ~ |vol|^2 stay off the one-hot regime
FIRST_BN_MEAN = 1.5                     # added to encoder1.0.bn1's running_mean: its input is a max-pooled ReLU output (all >= 0)
CONV3_GAIN = 0.5                        # on the bottlenecks' conv3: the un-normalised residual stream grows 2x slower
LAST_LINEAR_GAIN = {'pose_regressor.4.': 1.0, 'moe_predictor.4.': 0.5}


def ns(**kw):
    return types.SimpleNamespace(**kw)


def config(**over):
    """config/regression/mapfree/rot6d_trans_with_loftr.yaml over config/default.py, as a plain namespace tree; `over`: dotted
    overrides, e.g. config(**{'ENCODER.BLOCK_TYPE': 0})."""
    cfg = ns(
        MODEL='Regression',
        ENCODER=ns(TYPE='ResUNet', BLOCK_TYPE=1, NUM_BLOCKS='3-3-3', NOT_CONCAT=False, NUM_OUT_LAYERS=32),
        AGGREGATOR=ns(TYPE='CorrelationVolumeWarping', POSITION_ENCODER=True, POSITION_ENCODER_IM1=False, MAX_SCORE_CHANNEL=True,
                      NORMALISE_DOT=False, RESIDUAL_ATT=False, CV_OUTLAYERS=0, CV_HALF_CHANNELS=False, UPSAMPLE_POS_ENC=0, DUSTBIN=False),
        HEAD=ns(TYPE='DirectDeepResBlockMLP', ADD_BASIS=True, NUM_PTS=6, AVG_POOL=True, BATCH_NORM=True, SEPARATE_SCALE=True),
        TRAINING=ns(ROT_LOSS='rot_6d_loss', TRANS_LOSS='trans_unnormalized_loss', LAMBDA=1.),
        DATASET=ns(HEIGHT=360, WIDTH=270),
        SOLVER=ns(EMAT_RANSAC=ns(PIX_THRESHOLD=2.0, SCALE_THRESHOLD=0.1, CONFIDENCE=0.9999)))
    for k, v in over.items():
        node = cfg
        *path, leaf = k.split('.')
        for p in path:
            node = getattr(node, p)
        setattr(node, leaf, v)
    return cfg


def entries(module):
    """(name, tensor) of the regressor's parameters and buffers in sorted-name order (no matcher, no counters)."""
    return [(k, v) for k, v in sorted(module.state_dict().items()) if not k.startswith('matcher.') and not k.endswith('num_batches_tracked')]


def seeded_fill(module, seed=SEED):
    """Fills a RegressionModel-shaped module (the reference's, this package's or the restatement) in place: convolutions and Linear
    weights randn sqrt(2 / fan_in) (the attention projections and the last Linear layers sqrt(1 / fan_in)), BatchNorm / LayerNorm
    weights 1 + 0.1 randn, biases 0.1 randn, running_mean 0.1 randn, running_var 0.5 + rand; then the gains above."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in entries(module):
            leaf = name.rsplit('.', 1)[-1]
            if t.dim() >= 2:
                fan_in = t[0].numel()
                gain = 1.0 if ('self_attn' in name or name.startswith(tuple(LAST_LINEAR_GAIN))) else 2.0
                v = torch.randn(t.shape, generator=g) * (gain / fan_in) ** 0.5
            elif leaf == 'running_mean':
                v = 0.1 * torch.randn(t.shape, generator=g)
            elif leaf == 'running_var':
                v = 0.5 + torch.rand(t.shape, generator=g)
            elif leaf == 'weight':
                v = 1.0 + 0.1 * torch.randn(t.shape, generator=g)
            else:
                v = 0.1 * torch.randn(t.shape, generator=g)
            if name.startswith('encoder.outconv.normalize.') and leaf in ('weight', 'bias'):
                v = v * OUTCONV_GAIN
            if name == 'encoder.encoder1.0.bn1.running_mean':
                v = v + FIRST_BN_MEAN
            if name.startswith('encoder.encoder') and name.endswith('.conv3.weight'):
                v = v * CONV3_GAIN
            for prefix, gn in LAST_LINEAR_GAIN.items():
                if name.startswith(prefix):
                    v = v * gn
            t.copy_(v)
    return module


def seeded_images(size=SIZE, batch=B, seed=INPUT_SEED):
    """(image0_reg, image1_reg), each (batch, 3, H, W): smooth structure plus noise, normalised as the reference's dataset delivers
    them (zero mean, unit scale); image1 is image0 shifted plus fresh noise, so the correlation volume has structure to find."""
    g = torch.Generator().manual_seed(seed + 7 * size[0] + size[1])
    h, w = size
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing='ij')
    out = []
    base = torch.randn(batch, 3, h + 8, w + 8, generator=g)
    for k, (dy, dx) in enumerate(((0, 0), (5, 3))):
        img = base[:, :, dy:dy + h, dx:dx + w] * 0.8
        img = img + torch.sin(6.3 * (2 + k) * yy + 1.3 * k) * torch.cos(6.3 * 3 * xx) + 0.3 * torch.randn(batch, 3, h, w, generator=g)
        out.append(img.contiguous())
    return out[0], out[1]


def seeded_solver_outputs(batch=B, seed=INPUT_SEED, prior=False):
    """(loftr_rt (batch, 3, 4), inliers (batch, 3) with prior else (batch, 1)): a rotation near the identity per pair and translations
    whose norms straddle the clamps of the translation-norm transfer (pair 0 ordinary, pair 1 tiny: its ratio is clamped)."""
    g = torch.Generator().manual_seed(seed + 1)
    w = 0.2 * torch.randn(batch, 3, generator=g)
    K = torch.zeros(batch, 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    K = K - K.transpose(1, 2)
    R = torch.linalg.matrix_exp(K)
    t = torch.randn(batch, 3, generator=g)
    t = t / t.norm(dim=1, keepdim=True)
    scale = torch.tensor([1.0, 1e-4, 3.0, 0.5])[torch.arange(batch) % 4]
    rt = torch.cat([R, (t * scale[:, None])[:, :, None]], dim=2).float().contiguous()
    n = torch.randint(40, 400, (batch, 1), generator=g).float()
    if prior:
        inl = torch.cat([n, torch.floor(n * 0.6), torch.floor(n * 0.3)], dim=1)
    else:
        inl = n
    return rt, inl.contiguous()


def seeded_volumes(batch=B, seed=INPUT_SEED, scale=0.5):
    """Two (batch, 32, 92, 68) volumes for regress alone: smooth + noise, the second a shifted copy of the first plus noise."""
    g = torch.Generator().manual_seed(seed + 2)
    h, w = VOLUME
    base = torch.randn(batch, 32, h + 4, w + 4, generator=g)
    v0 = base[:, :, :h, :w]
    v1 = base[:, :, 2:h + 2, 1:w + 1] + 0.3 * torch.randn(batch, 32, h, w, generator=g)
    return (scale * v0).contiguous(), (scale * v1).contiguous()


def tap_volume(vol):
    return vol[:, :, ::TAP_VOL[0], ::TAP_VOL[1]]


def tap_x3(x3):
    return x3[:, ::TAP_X3_CH]
