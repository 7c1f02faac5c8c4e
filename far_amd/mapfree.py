"""Map-free (mapfree_6dreg) counterparts of the pieces of FAR's hot path that live outside mp3d_loftr (SURVEY.md section
8 f4): the essential-matrix pose solver the regression model calls per sample, the per-sample matcher + solver loop of
RegressionModel.forward, the correlation-volume warp of its aggregator (kernel K12, far_amd.ops.corr_volume_warp), and -- second half
of this file -- the regressor itself: RegressionModel (ResUNet encoder, DeepResBlock head, TransformerEncoder, pose_regressor /
moe_predictor gate; inference) on K27 / K28 and the kernels the package already had.

Reference:
  lib/models/matching/pose_solver.py:20-97     EssentialMatrixSolver.estimate_pose
  lib/models/regression/model.py:167-188       match_no_load (matcher on one pair -> mkpts0_f / mkpts1_f)
  lib/models/regression/model.py:236-273       the loop `for i in range(len(data['image0']))`: match, solve, pack
                                               loftr_rt (B, 3, 4) / inliers (B, 3 | 1), identity fallback
  lib/models/regression/aggregator.py:44-115   CorrelationVolumeWarping.forward

The matcher of the reference is upstream LoFTR (an un-vendored submodule, absent from /root/reference); its arithmetic is
the mp3d_loftr fork's, so far_amd.loftr.LoFTR with regress_rt = False stands in.  The minimal
solver is the GPU 8-point in every branch, batched over the pairs instead of looped.
"""
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .solver import _branch, prior_point_cloud


class EssentialMatrixSolver:
    """pose_solver.py:20-97.  cfg: an object with EMAT_RANSAC.PIX_THRESHOLD / .CONFIDENCE (or None: the values of
    config/matching/mapfree/loftr_emat_*.yaml: 2.0 px, 0.9999)."""

    def __init__(self, cfg=None, use_prior_ransac=False, H=2048, seed=0, minimal=8):
        er = getattr(cfg, 'EMAT_RANSAC', None) if cfg is not None else None
        self.ransac_pix_threshold = float(er.PIX_THRESHOLD) if er is not None else 2.0
        self.ransac_confidence = float(er.CONFIDENCE) if er is not None else 0.9999
        self.use_prior_ransac = use_prior_ransac
        self.H, self.seed = H, seed
        self.minimal = minimal        # 8: normalized 8-point hypotheses; 5: Nister five-point (what Map-free executes through cv2, :81)
        self.mask = None

    def solve_batch(self, kpts0, kpts1, counts, K0, K1, priorRT=None):
        """kpts0 / kpts1: (Mtot, 2) fp32 GPU, pairs concatenated in order; counts: per-pair M (host); K0, K1 (B, 3, 3);
        priorRT: None or (B, 3, 4).  Returns far_amd.ops.solve_pose_batch's dict of device tensors."""
        dev = kpts0.device
        counts = [int(c) for c in counts]
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        K0d, K1d = K0.to(device=dev, dtype=torch.float64), K1.to(device=dev, dtype=torch.float64)
        mode = _branch('prior_ransac' if self.use_prior_ransac else 'ransac', priorRT is not None)
        if mode == 'prior':
            inl_th = torch.full((len(counts),), 3e-7, dtype=torch.float64, device=dev)                    # :63
            prior = torch.as_tensor(np.asarray(priorRT), dtype=torch.float32).reshape(-1, 3, 4).to(dev).contiguous()
            pcl = prior_point_cloud(dev)
        else:
            f = (K0d[:, 0, 0] + K1d[:, 1, 1] + K0d[:, 1, 1] + K1d[:, 0, 0]) / 4                          # :44
            inl_th = (self.ransac_pix_threshold / f) ** 2
            prior = pcl = None
        return ops.solve_pose_batch(kpts0.float().contiguous(), kpts1.float().contiguous(), offs, K0d, K1d,
                                    inl_th.contiguous(), mode == 'prior', priorRT=prior, pcl=pcl, prior_lambda=0.3,
                                    H=self.H, seed=self.seed, minimal=self.minimal)

    def estimate_pose(self, kpts0, kpts1, data, priorRT=None):
        """Single pair, the reference's contract: ((R (3,3), t (3,), n_inliers), inliers_best_tight, inliers_best_ultra_tight)
        as numpy / python numbers; identity + zeros when there are too few correspondences or no model (:31-34, :85-86)."""
        R, t = np.eye(3), np.zeros(3)
        if len(kpts0) < 5:
            return (R, t, 0), 0, 0
        dev = data['K_color0'].device if data['K_color0'].is_cuda else torch.device('cuda')
        k0 = torch.as_tensor(kpts0, dtype=torch.float32, device=dev)
        k1 = torch.as_tensor(kpts1, dtype=torch.float32, device=dev)
        out = self.solve_batch(k0, k1, [len(k0)], data['K_color0'].reshape(1, 3, 3), data['K_color1'].reshape(1, 3, 3),
                               None if priorRT is None else np.asarray(torch.as_tensor(priorRT).cpu())[None])
        self.mask = out['mask'].cpu().numpy()[:, None]
        if not int(out['status'][0]):
            return (R, t, 0), 0, 0
        return ((out['R'][0].cpu().numpy(), out['t'][0].cpu().numpy(), int(out['n_cheir'][0])),
                int(out['tight'][0]), int(out['ultra'][0]))


@torch.no_grad()
def match_and_solve(matcher, data, solver, priorRT=None, use_prior=True):
    """model.py:245-273 without the per-sample loop: the matcher runs on the whole batch, the solver on all pairs at once.
    data: image0 / image1 (B, 1, H, W) grayscale as the matcher takes them, K_color0 / K_color1 (B, 3, 3).
    Writes data['loftr_rt'] (B, 3, 4) float32 (identity where the solver found nothing, :268-269) and data['inliers']
    ((B, 3) [n, tight, ultra] with a prior-capable model, (B, 1) otherwise, :259-266), plus mkpts0_f / mkpts1_f / m_bids."""
    batch = {'image0': data['image0'], 'image1': data['image1']}
    matcher(batch)                                                                                   # :167-172
    B = data['image0'].shape[0]
    dev = data['image0'].device
    bids = batch['m_bids']
    order = torch.argsort(bids, stable=True)
    mk0, mk1 = batch['mkpts0_f'][order], batch['mkpts1_f'][order]
    counts = torch.bincount(bids, minlength=B).cpu()
    out = solver.solve_batch(mk0, mk1, counts.tolist(), data['K_color0'], data['K_color1'], priorRT)
    ok = out['status'].bool()
    eye = torch.eye(3, 4, dtype=torch.float32, device=dev).expand(B, 3, 4)
    rt = torch.cat([out['R'].float(), out['t'].float()[:, :, None]], dim=2)
    data['loftr_rt'] = torch.where(ok[:, None, None], rt, eye)
    n = torch.where(ok, out['n_cheir'], torch.zeros_like(out['n_cheir'])).float()
    if use_prior:
        z = torch.zeros_like(n)
        data['inliers'] = torch.stack([n, torch.where(ok, out['tight'].float(), z), torch.where(ok, out['ultra'].float(), z)], 1)
    else:
        data['inliers'] = n[:, None]
    data.update(mkpts0_f=mk0, mkpts1_f=mk1, m_bids=bids[order], match_counts=counts, solver_status=out['status'])
    return data


# ---------------------------------------------------------------------------------------------------------------------
# The matcher Map-free instantiates: upstream LoFTR (zju3dv/LoFTR, an un-vendored submodule: etc/feature_matching_baselines/LoFTR,
# .gitmodules) built from its `default_cfg` and loaded from a released checkpoint with strict=False
# (lib/models/regression/model.py:103-106).  The mp3d_loftr fork this build mirrors keeps upstream's module tree for the
# matcher (backbone / pos_encoding / loftr_coarse / coarse_matching / fine_preprocess / loftr_fine / fine_matching: same
# parameter names and shapes per layer), so an upstream state dict loads into far_amd.loftr.LoFTR once the config says what
# upstream's says: four (self, cross) coarse layer pairs, the pre-fix position encoding, no regression head.
# ---------------------------------------------------------------------------------------------------------------------
def upstream_loftr_config():
    """Upstream LoFTR's `default_cfg` (src/loftr/utils/cvpr_ds_config.py, lower-cased) as the dict far_amd.loftr.LoFTR takes."""
    from .config import far_eval_config
    cfg = far_eval_config()
    cfg['coarse'].update(layer_names=['self', 'cross'] * 4, temp_bug_fix=False)     # released checkpoints predate the fix
    cfg['match_coarse'].update(train_coarse_percent=0.4, skh_prefilter=True)
    cfg.update(regress_rt=False, solver='ransac', use_many_ransac_thr=False, regress_loftr_layers=0)
    return cfg


def load_upstream_loftr(state_dict, device='cuda'):
    """far_amd.loftr.LoFTR with upstream LoFTR's released weights: `state_dict` is the checkpoint's ['state_dict'] (keys
    'matcher.*', as torch.load(weights_path)['state_dict'] in model.py:105).  Loaded the way the reference does, strict=False:
    the optimal-transport checkpoints ('outdoor_ot.ckpt', the file Map-free names) carry `coarse_matching.bin_score`, which
    the dual-softmax matcher of `default_cfg` does not have.  Anything ELSE missing or unexpected is an error here -- a
    silent partial load would give a matcher that runs and matches nothing."""
    from .loftr import LoFTR
    m = LoFTR(upstream_loftr_config()).eval()
    sd = state_dict.get('state_dict', state_dict)
    res = m.load_state_dict(dict(sd), strict=False)
    unexpected = [k for k in res.unexpected_keys if not k.endswith('coarse_matching.bin_score')]
    if res.missing_keys or unexpected:
        raise KeyError(f'upstream LoFTR checkpoint does not fit: missing {res.missing_keys[:5]}{"..." if len(res.missing_keys) > 5 else ""}, '
                       f'unexpected {unexpected[:5]}{"..." if len(unexpected) > 5 else ""}')
    return m.to(device)


# ---------------------------------------------------------------------------------------------------------------------
# The regressor itself (lib/models/regression/model.py: RegressionModel) in FAR's configuration
# (config/regression/mapfree/rot6d_trans_with_loftr.yaml, --use_loftr_preds --use_vanilla_transformer, with and without --use_prior):
# ResUNet encoder -> CorrelationVolumeWarping (K12) -> DeepResBlock head -> nn.TransformerEncoder -> pose_regressor / moe_predictor
# gate that blends the regressed pose with the solver's.  Inference only.  The modules below are PARAMETER CONTAINERS under the
# reference's names and shapes (as far_amd/vit8pt.py does it): they are never called; RegressionModel runs their tensors on the kernels.
# ---------------------------------------------------------------------------------------------------------------------
GRID = (12, 9)             # the head's output grid the reference hard-codes in self.H = 256 * 12 * 9 (model.py:97)
D_MODEL, NHEAD, NLAYERS = 256, 8, 6                          # model.py:58-61
H_FEATS, H2, POSE_SIZE, NUM_CORR = 256 * 12 * 9, 512, 9, 3   # model.py:96-98, :133


class _PreActBottleneck(nn.Module):
    """encoder/preact.py:39-64 under its names."""
    expansion = 4

    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.conv1 = nn.Conv2d(in_planes, planes, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, bias=False)
        if stride != 1 or in_planes != 4 * planes:
            self.shortcut = nn.Sequential(nn.Conv2d(in_planes, 4 * planes, 1, stride, bias=False))


class _PreActBlock(nn.Module):
    """encoder/preact.py:13-36 under its names (bn=True)."""

    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.conv1 = nn.Conv2d(in_planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        if stride != 1 or in_planes != planes:
            self.shortcut = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride, bias=False))


class _ConvBNELU(nn.Module):
    """encoder/resunet.py:15-26 (`conv`): Conv2d with bias + BatchNorm2d (+ ELU)."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, 1, (k - 1) // 2)
        self.normalize = nn.BatchNorm2d(cout)


class _UpConv(nn.Module):
    """encoder/resunet.py:29-39 (`upconv`)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = _ConvBNELU(cin, cout, 3)


class _ResUNet(nn.Module):
    """encoder/resunet.py:42-81 for BLOCK_TYPE 1, NUM_BLOCKS '3-3-3', NOT_CONCAT False."""

    def __init__(self, num_out_layers=32):
        super().__init__()
        self.firstconv = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.firstbn = nn.BatchNorm2d(64)
        self.in_planes = 64
        self.encoder1 = self._make_layer(64, 3, 1)
        self.encoder2 = self._make_layer(128, 3, 2)
        self.encoder3 = self._make_layer(256, 3, 2)
        self.upconv4 = _UpConv(1024, 512)
        self.iconv4 = _ConvBNELU(512 + 512, 512, 3)
        self.upconv3 = _UpConv(512, 256)
        self.iconv3 = _ConvBNELU(256 + 256, 256, 3)
        self.outconv = _ConvBNELU(256, num_out_layers, 1)
        self.num_out_layers = num_out_layers

    def _make_layer(self, planes, n, stride):
        layers = []
        for st in [stride] + [1] * (n - 1):
            layers.append(_PreActBottleneck(self.in_planes, planes, st))
            self.in_planes = 4 * planes
        return nn.Sequential(*layers)


class _DeepResBlock(nn.Module):
    """head.py:27-55, 248-281: DirectDeepResBlockMLP(full_forward_pass=False) -- three PreActBlocks, no MLP."""

    def __init__(self, in_channels):
        super().__init__()
        self.resblock1 = _PreActBlock(in_channels, 64, 2)
        self.resblock2 = _PreActBlock(64, 128, 2)
        self.resblock3 = _PreActBlock(128, 256, 2)


def reference_state_dict(sd):
    """A FAR Map-free checkpoint's state dict (or the checkpoint: its ['state_dict']) -> the entries a RegressionModel of this package
    loads with strict=True: everything but `matcher.*` (upstream LoFTR, which load_upstream_loftr loads into its own module)."""
    sd = sd.get('state_dict', sd)
    return {k: v for k, v in sd.items() if not k.startswith('matcher.')}


def rotation_6d_to_matrix(d6):
    """model.py:25-31: (..., 6) -> (..., 3, 3), rows b1, b2, b3 (F.normalize: the norms floored at 1e-12)."""
    F = torch.nn.functional
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = F.normalize(b2, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def _bn_affine(bn):
    """An inference BatchNorm as a per-channel affine map (running statistics), folded in float64."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    return scale.float(), shift.float()


def _bn_tensors(bn):
    return [bn.weight, bn.bias, bn.running_mean, bn.running_var]


def _get(node, name, default=None):
    return getattr(node, name, default) if node is not None else default


def _check_aggregator_options(agg, who):
    """K12 is the aggregator of the FAR configuration only: every other option of aggregator.py:10-17 is refused by name."""
    on = [k for k in ('POSITION_ENCODER_IM1', 'NORMALISE_DOT', 'RESIDUAL_ATT', 'CV_OUTLAYERS', 'CV_HALF_CHANNELS', 'UPSAMPLE_POS_ENC',
                      'DUSTBIN') if _get(agg, k)]
    off = [k for k in ('POSITION_ENCODER', 'MAX_SCORE_CHANNEL') if not _get(agg, k)]
    if on or off:
        raise NotImplementedError(f'{who}: K12 (far_corr_volume_warp_f32) is CorrelationVolumeWarping with POSITION_ENCODER and '
                                  f'MAX_SCORE_CHANNEL and nothing else; not built: {[k + " on" for k in on] + [k + " off" for k in off]}')


class CorrelationVolumeWarping(nn.Module):
    """lib/models/regression/aggregator.py:6-116 in the FAR configuration, trainable: cfg is the reference's AGGREGATOR node
    (POSITION_ENCODER and MAX_SCORE_CHANNEL on, everything else off), volume_channels must be 32.  No parameters, an empty state
    dict, num_out_layers = 67.  forward(vol0, vol1): (B, 32, H, W) x 2 on the GPU -> (B, 67, H, W); K12's training forward with its
    HIP backward (ops.corr_volume_warp_train) when a gradient is needed, the inference launch otherwise -- the same bits either way."""

    def __init__(self, cfg, volume_channels):
        super().__init__()
        _check_aggregator_options(cfg, 'CorrelationVolumeWarping')
        if volume_channels != 32:
            raise NotImplementedError(f'CorrelationVolumeWarping: K12 is built for 32 volume channels, got {volume_channels!r}')
        self.position_encoder, self.max_score_channel = True, True
        self.num_out_layers = 2 * volume_channels + 2 + 1

    def forward(self, vol0, vol1):
        return ops.corr_volume_warp_train(vol0, vol1)


class RegressionModel(nn.Module):
    """lib/models/regression/model.py:33-308, inference.  cfg: the reference's configuration as any attribute tree (a yacs node, the
    namespace of tests/mapfree_reg_inputs.py: ENCODER / AGGREGATOR / HEAD / TRAINING / SOLVER); matcher: a far_amd.loftr.LoFTR
    (load_upstream_loftr) or None when every call supplies data['loftr_rt'] / data['inliers'] -- it is NOT part of the state dict.

    State dict: encoder.*, head.resblock{1,2,3}.*, transformer.layers.{0..5}.*, pose_regressor.{0,2,4}.*, moe_predictor.{0,2,4}.* under
    the reference's names and shapes; a FAR checkpoint loads with strict=True after reference_state_dict(sd).  Construction and
    load_state_dict work on the CPU; the weight images are packed at the first GPU call (and re-packed when a tensor changes).

    Kernels: K27 (stem), K26 (max-pool), K7 (bn1 + ReLU of every pre-activation block), K9 / K17 (every 1x1 / 3x3 convolution, bn2 / bn3
    + ReLU and the decoder's bias + BatchNorm folded into the epilogues, the shortcut add in the last convolution's, the strided 1x1
    shortcuts through in_stride = 2, the decoder's concatenations read in place through x2), K28 (bilinear x2, skip pad, ELU), K12
    (aggregator), K9 + K22 + K6 (the six post-norm encoder layers), K15 (the five dense layers of the gate: a pair's pose has the
    same bits alone and in a batch).  BatchNorm uses its running statistics whatever .train() says.

    The loop (model.py:235-308): without a prior, match_and_solve once, then regress; with use_prior, solve, regress, priorRT =
    [rotation_6d_to_matrix(R) | t], solve again with the prior, regress again.  The encoder, the aggregator, the head and the
    transformer do not depend on the loop index (the reference recomputes them per loop, without gradients in the first): they run ONCE
    and only the solver and the gate repeat.

    Not built (NotImplementedError): other encoder / aggregator / head types or options, use_superglue_preds,
    use_vanilla_transformer=False, use_loftr_preds=False, LAMBDA == 0 (the learnable loss weights), training (a call that needs
    gradients, or .train() with gradients enabled).  CPU tensors raise FarHipError."""

    def __init__(self, cfg, use_loftr_preds=False, use_superglue_preds=False, ckpt_path=None, not_strict=False, inference=False,
                 use_vanilla_transformer=False, d_model=32, max_steps=200_000, use_prior=False, matcher=None):
        super().__init__()
        self._check_config(cfg, use_loftr_preds, use_superglue_preds, use_vanilla_transformer)
        self.cfg = cfg
        self.max_steps = max_steps
        self.use_prior = bool(use_prior)
        self.use_loftr_preds, self.use_superglue_preds, self.use_vanilla_transformer = True, False, True
        self.LAMBDA = cfg.TRAINING.LAMBDA
        self.encoder = _ResUNet(int(cfg.ENCODER.NUM_OUT_LAYERS))
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=D_MODEL, nhead=NHEAD), num_layers=NLAYERS,
                                                 enable_nested_tensor=False)
        self.head = _DeepResBlock(2 * self.encoder.num_out_layers + 3)
        self.H2, self.H, self.pose_size, self.num_corr_size = H2, H_FEATS, POSE_SIZE, NUM_CORR
        self.moe_predictor = nn.Sequential(nn.Linear(self.H + 2 * self.pose_size + self.num_corr_size, self.H2), nn.ReLU(),
                                           nn.Linear(self.H2, self.H2), nn.ReLU(), nn.Linear(self.H2, 2), nn.Sigmoid())
        self.pose_regressor = nn.Sequential(nn.Linear(self.H, self.H2), nn.ReLU(), nn.Linear(self.H2, self.H2), nn.ReLU(),
                                            nn.Linear(self.H2, self.pose_size))
        self.pose_solver = EssentialMatrixSolver(_get(cfg, 'SOLVER'), self.use_prior)
        self.__dict__['matcher'] = matcher                  # not a submodule: the state dict holds the regressor alone
        self.act_exp = ops._CONV_ACT_EXP
        self.requires_grad_(False)
        self.eval()
        if ckpt_path is not None:
            sd = reference_state_dict(torch.load(ckpt_path, map_location='cpu'))
            self.load_state_dict(sd, strict=not not_strict)

    @staticmethod
    def _check_config(cfg, use_loftr_preds, use_superglue_preds, use_vanilla_transformer):
        no = NotImplementedError
        enc, agg, head, tr = _get(cfg, 'ENCODER'), _get(cfg, 'AGGREGATOR'), _get(cfg, 'HEAD'), _get(cfg, 'TRAINING')
        if _get(enc, 'TYPE') != 'ResUNet':
            raise no(f"RegressionModel: encoder {_get(enc, 'TYPE')!r} is not built (only 'ResUNet')")
        if (_get(enc, 'BLOCK_TYPE') != 1 or str(_get(enc, 'NUM_BLOCKS')).strip() != '3-3-3' or _get(enc, 'NOT_CONCAT', False)
                or _get(enc, 'NUM_OUT_LAYERS') != 32):
            raise no("RegressionModel: the ResUNet is built for BLOCK_TYPE 1 (PreActBottleneck), NUM_BLOCKS '3-3-3', NOT_CONCAT False, "
                     f"NUM_OUT_LAYERS 32; got BLOCK_TYPE {_get(enc, 'BLOCK_TYPE')!r}, NUM_BLOCKS {_get(enc, 'NUM_BLOCKS')!r}, NOT_CONCAT "
                     f"{_get(enc, 'NOT_CONCAT')!r}, NUM_OUT_LAYERS {_get(enc, 'NUM_OUT_LAYERS')!r}")
        if _get(agg, 'TYPE') != 'CorrelationVolumeWarping':
            raise no(f"RegressionModel: aggregator {_get(agg, 'TYPE')!r} is not built (only 'CorrelationVolumeWarping', K12)")
        _check_aggregator_options(agg, 'RegressionModel')
        if _get(head, 'TYPE') != 'DirectDeepResBlockMLP':
            raise no(f"RegressionModel: head {_get(head, 'TYPE')!r} is not built (only 'DirectDeepResBlockMLP')")
        if not _get(head, 'BATCH_NORM', True):
            raise no('RegressionModel: HEAD.BATCH_NORM False is not built')
        if use_superglue_preds:
            raise no('RegressionModel: use_superglue_preds -- SuperPoint / SuperGlue are not part of this package')
        if not use_vanilla_transformer:
            raise no('RegressionModel: use_vanilla_transformer=False (the head without the TransformerEncoder) is not built')
        if not use_loftr_preds:
            raise no('RegressionModel: use_loftr_preds=False (the transformer_head without the gate) is not built')
        if _get(tr, 'LAMBDA') is None or float(tr.LAMBDA) == 0.:
            raise no('RegressionModel: TRAINING.LAMBDA == 0 (the learnable loss weights s_r / s_t of training) is not built')

    # ---- the activation-range guard (as far_amd.loftr.LoFTR._guarded, for a module without fused fixed-exponent kernels): the
    # split-fp16 launches (K27, K9, K17, K22) OR the per-device flag when an operand left the range 65504 / 2^e; it is read once
    # behind the call, and an overflow lowers e by 4 (16x the range) and runs the call again.  The setting sticks to the module.
    def _guarded(self, fn, device, inputs=()):
        ops.overflow_flag(device).zero_()
        start = self.act_exp
        while True:
            with ops.activation_exponent(self.act_exp):
                out = fn()
            if not ops.activation_overflowed(device):
                return out
            bad = [t for t in inputs if torch.is_tensor(t) and t.is_floating_point() and not bool(torch.isfinite(t).all())]
            if bad or self.act_exp - 4 < ops.ACT_EXP_MIN:
                self.act_exp = start                          # nothing that did not yield finite outputs is kept
                raise ops.ActivationOverflow('RegressionModel: non-finite values in the inputs, or activations beyond the widest '
                                             'split-fp16 range (|a| > 1e12): the outputs of this call contain inf / NaN')
            self.act_exp -= 4
            warnings.warn(f'far_amd: an activation exceeded the split-fp16 range; re-running with activation exponent {self.act_exp} '
                          f'(|a| <= {65504.0 / 2.0 ** self.act_exp:.3g})')

    def _enter(self, *tensors):
        """The checks every public call makes: no training, GPU tensors."""
        if torch.is_grad_enabled() and (self.training or any(p.requires_grad for p in self.parameters())
                                         or any(torch.is_tensor(t) and t.requires_grad for t in tensors)):
            raise NotImplementedError('RegressionModel: training is not built (no backward kernels for K27 / K28 / K12, BatchNorm on '
                                      'running statistics): call it in .eval() mode with requires_grad False on its parameters and '
                                      'inputs, or under torch.no_grad()')
        for t in tensors:
            if torch.is_tensor(t) and not t.is_cuda:
                raise ops._lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
        if any(p.device.type != 'cuda' for p in self.parameters()):
            raise ops._lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists): move the model with .cuda()')

    def _packs(self):
        return self.__dict__.setdefault('_pack_cache', ops.PackCache())

    def _conv(self, name, conv, bn=None, stride=1, pad_cin=0):
        """The K9 image of `conv` with `bn` (the BatchNorm BEHIND it) and its bias folded into the epilogue vectors."""
        def build():
            w = conv.weight.detach()
            if pad_cin:
                w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, pad_cin))
            scale = shift = None
            if bn is not None:
                scale, shift = _bn_affine(bn)
                if conv.bias is not None:
                    shift = (shift.double() + scale.double() * conv.bias.detach().double()).float()
            elif conv.bias is not None:
                shift = conv.bias.detach().float()
            return ops.PackedConv(w, scale, shift, stride=stride)
        tensors = [t for t in (conv.weight, conv.bias) if t is not None] + (_bn_tensors(bn) if bn is not None else [])
        return self._packs().get(name, tensors, build)

    def _bn_relu(self, name, bn, x, pad=0):
        """relu(bn(x)) for NHWC x on K7 (a new tensor: x also feeds the identity shortcut)."""
        def build():
            s, b = _bn_affine(bn)
            if pad:
                s, b = torch.cat([s, s.new_ones(pad)]), torch.cat([b, b.new_zeros(pad)])
            return s.contiguous(), b.contiguous()
        s, b = self._packs().get(name, _bn_tensors(bn), build)
        return ops.affine_act(x.permute(0, 3, 1, 2), s, b, act='relu', inplace=False).permute(0, 2, 3, 1)

    def _bottleneck(self, name, blk, x):
        st = blk.conv2.stride[0]
        a = self._bn_relu(name + '.bn1', blk.bn1, x)
        y = ops.conv_nhwc(a, self._conv(name + '.conv1', blk.conv1, blk.bn2), act='relu')
        y = ops.conv_nhwc(y, self._conv(name + '.conv2', blk.conv2, blk.bn3, stride=st), act='relu')
        sc = ops.conv_nhwc(a, self._conv(name + '.shortcut', blk.shortcut[0]), in_stride=st) if hasattr(blk, 'shortcut') else x
        return ops.conv_nhwc(y, self._conv(name + '.conv3', blk.conv3), residual=sc)

    def _preact_block(self, name, blk, x, pad=0):
        st = blk.conv1.stride[0]
        a = self._bn_relu(name + '.bn1', blk.bn1, x, pad)
        sc = ops.conv_nhwc(a, self._conv(name + '.shortcut', blk.shortcut[0], pad_cin=pad), in_stride=st)
        y = ops.conv_nhwc(a, self._conv(name + '.conv1', blk.conv1, blk.bn2, stride=st, pad_cin=pad), act='relu')
        return ops.conv_nhwc(y, self._conv(name + '.conv2', blk.conv2), residual=sc)

    def _conv_elu(self, name, m, x, x2=None):
        return ops.elu(ops.conv_nhwc(x, self._conv(name, m.conv, m.normalize), x2=x2), inplace=True)

    def _encode(self, images, taps=None):
        enc = self.encoder
        pk = self._packs()
        stem = pk.get('firstconv', [enc.firstconv.weight] + _bn_tensors(enc.firstbn),
                      lambda: ops.PackedStemRGB(enc.firstconv.weight, *_bn_affine(enc.firstbn)))
        x = ops.maxpool3x3s2(ops.stem_conv_rgb(images.detach().float().contiguous(), stem))
        skips = []
        for lname in ('encoder1', 'encoder2', 'encoder3'):
            for i, blk in enumerate(getattr(enc, lname)):
                x = self._bottleneck(f'{lname}.{i}', blk, x)
            skips.append(x)
        x2, x3, x4 = skips
        up, x3p = ops.upsample2x_pad(x4, x3)                              # resunet.py:117-119
        x = self._conv_elu('upconv4', enc.upconv4.conv1, up)
        x = self._conv_elu('iconv4', enc.iconv4, x, x2=x3p)
        up, x2p = ops.upsample2x_pad(x, x2)                               # :122-124
        x = self._conv_elu('upconv3', enc.upconv3.conv1, up)
        x = self._conv_elu('iconv3', enc.iconv3, x, x2=x2p)
        x = self._conv_elu('outconv', enc.outconv, x)                     # :127
        if taps is not None:
            taps.update(x2=x2, x3=x3, x4=x4)
        return x.permute(0, 3, 1, 2)                                      # (N, 32, h, w) logical, NHWC memory

    def encode(self, images):
        """resunet.py:105-128: images (N, 3, H, W) fp32 on the GPU, normalised as the reference's dataset delivers them, at any size
        -> the (N, 32, h, w) volume, h = 4 ceil(H / 16), w = 4 ceil(W / 16) (360 x 270 -> 92 x 68).  Image n's volume does not depend
        on N.  `images` is only read."""
        self._enter(images)
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f'images: (N, 3, H, W), got {tuple(images.shape)}')
        with torch.no_grad():
            return self._guarded(lambda: self._encode(images), images.device, (images,))

    def _features(self, vol0, vol1, taps=None):
        """Aggregator, head, transformer: (B, 32, h, w) x 2 -> the (B, 27648) features the gate reads."""
        agg = ops.corr_volume_warp(vol0, vol1)                            # (B, 67, h, w) NCHW
        B, C, h, w = agg.shape
        pad = -C % 4
        x = agg.new_zeros(B, h, w, C + pad)
        x[..., :C] = agg.permute(0, 2, 3, 1)                              # NHWC with a zero channel: K7 / K9 take C % 4 == 0
        hd = self.head
        x = self._preact_block('head.resblock1', hd.resblock1, x, pad)
        x = self._preact_block('head.resblock2', hd.resblock2, x)
        x3 = self._preact_block('head.resblock3', hd.resblock3, x)        # (B, 12, 9, 256) NHWC (_check_volumes saw to the grid)
        x = x3.reshape(B, GRID[0] * GRID[1], D_MODEL)                     # model.py:289-291: sequence = positions, batch = pairs
        pk = self._packs()
        lin = lambda name, w, b: pk.get(name, [w, b], lambda: ops.PackedConv(w, None, b))
        for i, layer in enumerate(self.transformer.layers):
            at = layer.self_attn
            qkv = ops.linear_f16s(x, lin(f'tr{i}.in', at.in_proj_weight, at.in_proj_bias), out_planes=3)
            a = ops.full_attention(qkv[0], qkv[1], qkv[2], NHEAD)
            y = ops.linear_f16s(a, lin(f'tr{i}.out', at.out_proj.weight, at.out_proj.bias), residual=x)
            x = ops.layernorm(y, layer.norm1.weight, layer.norm1.bias, layer.norm1.eps)
            hid = ops.linear_f16s(x, lin(f'tr{i}.l1', layer.linear1.weight, layer.linear1.bias), act='relu')
            y = ops.linear_f16s(hid, lin(f'tr{i}.l2', layer.linear2.weight, layer.linear2.bias), residual=x)
            x = ops.layernorm(y, layer.norm2.weight, layer.norm2.bias, layer.norm2.eps)
        if taps is not None:
            taps.update(x3=x3.permute(0, 3, 1, 2), transformer=x)
        return x.transpose(1, 2).reshape(B, self.H)                       # (B, 256, 108) flattened: channel-major as model.py:291

    def _gate(self, feats, pre, loftr_rt, inliers):
        """regression_mlp, model.py:198-233, behind the two 27648-wide first layers (pre = their one K15 launch)."""
        B = feats.shape[0]
        pk = self._packs()
        reg, moe = self.pose_regressor, self.moe_predictor
        lin = lambda name, m, **kw: pk.get(name, [m.weight, m.bias], lambda: ops.PackedRows(m.weight, m.bias, **kw))
        h = torch.relu(pre[:, :self.H2] + reg[0].bias)
        h = ops.rows_linear(h, lin('reg2', reg[2]), act='relu')
        pred_reg_6d = ops.rows_linear(h, lin('reg4', reg[4]))                                       # (B, 9) [t | R 6d]
        rt = loftr_rt.to(feats.device).float()
        loftr_6d = torch.cat([rt[..., 3], rt[..., :2, :3].reshape(B, 6)], dim=-1)                   # :203-204
        n = inliers.detach().to(feats.device).float().reshape(B, -1) / 500
        if self.use_prior:
            if n.shape[1] != 3:
                raise ValueError(f'use_prior: inliers must be (B, 3) [n, tight, ultra], got {tuple(inliers.shape)}')
        else:
            if n.shape[1] != 1:
                raise ValueError(f'inliers must be (B, 1) without a prior, got {tuple(inliers.shape)}')
            n = torch.cat([n, n / 10, n / 100], dim=-1)                                             # :211
        norm = torch.linalg.norm
        ratio = torch.clamp((norm(pred_reg_6d[..., :3], dim=-1) / torch.clamp(norm(loftr_6d[..., :3], dim=-1), 1e-2, 1e2)).unsqueeze(1),
                            1e-2, 1e2)
        out = torch.cat([loftr_6d[..., :3] * ratio, loftr_6d[..., 3:], n], dim=-1)                  # :221-224, (B, 12)
        tail = torch.cat([pred_reg_6d, out], dim=-1).contiguous()                                   # (B, 21)
        g = ops.rows_linear(tail, lin('moe0-tail', moe[0], cols=(self.H, moe[0].weight.shape[1])), act='relu', add=pre[:, self.H2:])
        g = ops.rows_linear(g, lin('moe2', moe[2]), act='relu')
        wt = ops.rows_linear(g, lin('moe4', moe[4]), act='sigmoid')                                 # (B, 2)
        t = wt[..., :1] * pred_reg_6d[..., :3] + (1 - wt[..., :1]) * out[..., :3]
        R = wt[..., 1:] * pred_reg_6d[..., 3:] + (1 - wt[..., 1:]) * out[..., 3:-self.num_corr_size]
        return R, t, wt

    def _first_layers(self, feats):
        """The two 27648-wide first layers read the features only: one K15 launch for both -> (B, 2 H2)."""
        reg, moe = self.pose_regressor, self.moe_predictor
        both = self._packs().get('reg0|moe0', [reg[0].weight, moe[0].weight],
                                 lambda: ops.PackedRows(torch.cat([reg[0].weight, moe[0].weight[:, :self.H]], 0)))
        return ops.rows_linear(feats, both)               # no bias yet: reg0's goes in with its ReLU, moe0's with its 21-wide tail (_gate)

    def _prepare(self, vol0, vol1, taps=None):
        """Everything that does not depend on the solver's output: -> (feats (B, 27648), pre (B, 1024))."""
        feats = self._features(vol0, vol1, taps)
        return feats, self._first_layers(feats)

    @staticmethod
    def _check_volumes(vol0, vol1):
        if vol0.dim() != 4 or vol0.shape != vol1.shape or vol0.shape[1] != 32:
            raise ValueError(f'vol0 / vol1: two (B, 32, h, w) volumes, got {tuple(vol0.shape)} and {tuple(vol1.shape)}')
        h, w = vol0.shape[2:]
        red = lambda s: (((s - 1) // 2) // 2) // 2 + 1           # three 3x3 stride-2 pad-1 convolutions
        if (red(h), red(w)) != GRID:
            raise ValueError(f'RegressionModel.regress: a {h} x {w} volume reaches the gate as {red(h)} x {red(w)}; it needs the '
                             f'{GRID[0]} x {GRID[1]} grid the reference hard-codes (H = 256 * 12 * 9): volumes of 89..96 x 65..72')

    def regress(self, vol0, vol1, loftr_rt, inliers, taps=None):
        """Aggregator, head, transformer and gate (model.py:285-294): vol0 / vol1 (B, 32, h, w) from encode, loftr_rt (B, 3, 4) the
        solver's pose, inliers (B, 1) -- (B, 3) [n, tight, ultra] with use_prior -- -> (R (B, 6), t (B, 3)).  The volumes must reach the
        gate on the 12 x 9 grid (ValueError otherwise).  taps (tests): a dict that receives x3, the transformer output, the gate weights."""
        self._enter(vol0, vol1, loftr_rt, inliers)
        self._check_volumes(vol0, vol1)
        with torch.no_grad():
            feats, pre = self._guarded(lambda: self._prepare(vol0, vol1, taps), vol0.device, (vol0, vol1))
            R, t, wt = self._gate(feats, pre, loftr_rt, inliers)
        if taps is not None:
            taps['gate'] = wt
        return R, t

    def forward(self, data):
        """model.py:235-308.  data: image0_reg / image1_reg (B, 3, H, W) normalised as the reference's dataset delivers them; and either
        loftr_rt (B, 3, 4) + inliers (cached predictions: the matcher and the solver are skipped, in every loop) or the matcher's
        image0 / image1 (B, 1, H, W) + K_color0 / K_color1 (B, 3, 3).  Returns (R (B, 6), t (B, 3)), also written to data['R'] / data['t'].
        The same bits as regress(encode(image0_reg), encode(image1_reg), ...).  The encoder, aggregator, head and transformer run once;
        with use_prior only the solver and the gate run twice (class docstring).  Inputs are only read."""
        im0, im1 = data['image0_reg'], data['image1_reg']
        cached = 'loftr_rt' in data and 'inliers' in data
        if not cached and self.matcher is None:
            raise ValueError("RegressionModel.forward: data holds no 'loftr_rt' / 'inliers' and the model was built without a matcher")
        self._enter(im0, im1, *((data['loftr_rt'], data['inliers']) if cached else (data['image0'], data['image1'])))
        if im0.dim() != 4 or im0.shape != im1.shape or im0.shape[1] != 3:
            raise ValueError(f'image0_reg / image1_reg: two (B, 3, H, W) tensors, got {tuple(im0.shape)} and {tuple(im1.shape)}')
        B = im0.shape[0]

        def run():
            vols = self._encode(torch.cat([im0, im1], 0))                 # one pass over both images of every pair
            self._check_volumes(vols[:B], vols[B:])
            return self._prepare(vols[:B], vols[B:])
        with torch.no_grad():
            feats, pre = self._guarded(run, im0.device, (im0, im1))
            # the solver and the gate alone repeat (the matcher guards its own activation range; K15 is exact fp32)
            R = t = None
            for loop in range(2 if self.use_prior else 1):
                if not cached:
                    prior = None
                    if loop > 0:
                        prior = torch.cat([rotation_6d_to_matrix(R), t.unsqueeze(2)], dim=-1).cpu().numpy()     # model.py:298-299
                    match_and_solve(self.matcher, data, self.pose_solver, prior, use_prior=self.use_prior)
                R, t, _ = self._gate(feats, pre, data['loftr_rt'], data['inliers'])
        data['R'], data['t'] = R, t
        return R, t
