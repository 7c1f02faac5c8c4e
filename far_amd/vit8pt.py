"""The 8-Point-ViT regressor of FAR (interiornetStreetlearn_8ptVit/src/model.py: ViTEss): inference from extractor features or -- opt-in --
from images, and -- opt-in -- training of the trunk and the head.

Mirrors the module / parameter structure of the reference so that a released checkpoint loads with strict=True after
reference_state_dict(sd) dropped its `resnet.*` / `extractor_final_conv.*` entries:
    fusion_transformer.pos_embed, fusion_transformer.blocks.{i}.{norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2},
    fusion_transformer.blocks.{depth-1}.{norm1, cross_attn.qkv, cross_attn.proj_fundamental, norm2, mlp.*}, fusion_transformer.norm,
    pose_regressor.{0, 2, 4}, moe_predictor.{0, 2, 4}
Reference lines: Attention / Block vision_transformer.py:236-283, CrossBlock :210-234 (far_amd.loftr.transformer.CrossBlock, K2),
the trunk and the head model.py:171-217, 6D -> matrix tools.py:20-60.

Kernels: K6 (LayerNorm), K9 (qkv into head planes, proj / fc2 with the residual in the epilogue, fc1), K23 (the head-dim-64 softmax
self-attention, ops.vit_attention_planes), K2 (the CrossBlock), K15 (every Linear of the head).  No eager fallback: CPU tensors raise.

The extractor (model.py:56-60, :131-163; modules/extractor.py:5-65) is opt-in: `ViTEss(args, mean, std, extractor=True)` adds
    resnet.{conv1, bn1, layer1.{0, 1}, layer2.{0, 1}} (torchvision's ResNet18 front under its names; layer2.0 with downsample.{0, 1}),
    extractor_final_conv.{conv1, conv2, norm1, norm2, norm3, downsample.{0, 1}} (downsample.1 IS norm3, as in the reference)
as nn.Conv2d / nn.BatchNorm2d modules -- reference_state_dict(sd, extractor=True) then drops only resnet.layer3.* / layer4.* -- and
`forward(images)` / `extract_features(images)` run it in 14 launches: K25 (ops.stem_rgb: channel flip, / 255, normalisation, nearest
resize to 224, conv1, bn1, relu), K26 (ops.maxpool3x3s2), K9 / K17 (ops.conv_nhwc: layer1, layer2, extractor_final_conv.conv1) and
K24 (ops.conv_valid: the two 5x5 unpadded convolutions with the block's add and ReLUs).  By default it is inference-only and FROZEN,
which the reference's is not (it fine-tunes these layers): requires_grad False on its parameters, running statistics in every
BatchNorm whatever .train() says, detached features under set_block_training(); an extractor parameter with requires_grad=True
raises when gradients are enabled.  Without the keyword nothing changes: no such submodules, and forward(images) raises as before.
`ViTEss.set_extractor_training()` opts in to fine-tuning extractor_final_conv (the reference's ResidualBlock(128, 192, 'batch',
kernel_size=5), half of the extractor's arithmetic) with the trunk: in .train() mode under enabled gradients the block runs on
K9 + K16 (conv1), K24 forward + its HIP backward (ops.conv_valid_train: conv2, downsample.0) and K19 (the three BatchNorm layers with
batch statistics, running statistics updated as nn.BatchNorm2d does), and the features carry gradients.  The ResNet front stays
frozen on its running statistics (a deviation: the reference's whole model is in .train()); gradients into resnet.* raise.

Training (the reference's train.py: MSE on the translation plus MSE on the rotation output, clip_grad_norm_, AdamW) is opt-in,
modelled on LoFTR.set_full_attention_training(): `ViTEss.set_block_training()` sets `block_training` on the trunk, its Blocks and
their Attention modules; without it a call that needs gradients raises NotImplementedError as before.  With it a Block runs K6
forward + backward (ops.layernorm_train), K9 forward + dgrad and K16 wgrad for qkv, proj, fc1 and fc2 (ops.linear_train, one PackCache
per module), and K23's training forward + HIP backward on the qkv projection in place (ops.vit_attention_train_qkv: no chunk, no cat);
GELU and the residual adds are elementwise torch ops.  The CrossBlock trains on K2's kernels; the head's two small parameter
containers run under autograd (the package's convention for them, far_amd/_vendor.py).  `pose_loss` is the reference's loss;
far_amd.optim (K20) is the optimizer side.  The no-grad path is the same code and the same bits whatever the switch says.

16-bit operands are opt-in and inference only, modelled on LoFTR.set_precision: `ViTEss.set_precision('fp16')` (or a set of
ViTEss.STAGES names) runs the extractor's K9 / K24 launches, the Blocks' Linear layers, K23 (far_vit_attention_f16) and the CrossBlock
on plain fp16 operands.  Narrower than the reference; 'fp32' stays the default and the only mode held to the reference's bars.

Not built (each raises NotImplementedError): 16-bit training (a call that needs gradients with a precision stage on), training the extractor's ResNet front (K25 / K26 have no backward), dropout and drop-path (0 in every script), per-sample intrinsics, and
the pooled-conv ablation (fusion_transformer=False).

Pair order: the reference keeps the two images of pair b in rows 2b, 2b + 1 of a (2B, N, C) tensor; this package's CrossBlock takes
cat([img0s, img1s]).  forward_features takes and returns the reference's order and converts once, in front of the trunk (the
Blocks work per image, the CrossBlock's output is per pair in either convention).
"""
from functools import partial

import torch
import torch.nn as nn

from . import _vendor as ag
from . import ops
from .loftr.transformer import CrossBlock, Mlp, _init_vit, positional_table_vit

GRID = (24, 24)            # feature_resolution of the reference (model.py:44)
DIM, HEADS = 192, 3        # total_num_features, num_heads (:43, :64)
NORM = partial(nn.LayerNorm, eps=1e-6)


def update_intrinsics(input_shape, intrinsics):
    """model.py:120-129 as a pure function: (B, 2, 4) [fx, fy, cx, cy] at the image size input_shape[-2:] -> the same on the 24 x 24
    feature grid.  Returns a new tensor; the argument is left as it is (the reference scales it in place)."""
    sizey, sizex = GRID
    scale = torch.tensor([sizex / input_shape[-1], sizey / input_shape[-2]] * 2, dtype=intrinsics.dtype, device=intrinsics.device)
    return intrinsics * scale


def interleaved_to_concatenated(x):
    """(2B, ...) with rows (2b, 2b + 1) = pair b  ->  cat([img0s, img1s])."""
    B = x.shape[0] // 2
    return x.reshape(B, 2, *x.shape[1:]).transpose(0, 1).reshape(x.shape)


def concatenated_to_interleaved(x):
    """cat([img0s, img1s])  ->  (2B, ...) with rows (2b, 2b + 1) = pair b."""
    B = x.shape[0] // 2
    return x.reshape(2, B, *x.shape[1:]).transpose(0, 1).reshape(x.shape)


def rotation_matrix_from_ortho6d(o6):
    """tools.py:47-60 (Gram-Schmidt, the norms floored at 1e-8 as normalize_vector :20-29): (B, 6) -> (B, 3, 3), columns x, y, z."""
    floor = torch.tensor(1e-8, dtype=o6.dtype, device=o6.device)
    unit = lambda v: v / torch.max(torch.sqrt(v.pow(2).sum(1)), floor).unsqueeze(1)
    x = unit(o6[:, 0:3])
    z = unit(torch.cross(x, o6[:, 3:6], dim=1))
    y = torch.cross(z, x, dim=1)
    return torch.stack([x, y, z], dim=2)


def pose_from_rotation_matrix(T_pose, r):
    """tools.py:9-17: (J, 3) rest poses under the (B, 3, 3) rotations -> (B, J, 3)."""
    return torch.matmul(r.unsqueeze(1), T_pose.to(r).reshape(1, -1, 3, 1)).squeeze(-1)


def loftr_gate_inputs(data):
    """The gate's inputs from the data dict far_amd.pipeline / supervision.spvs_RT fill: -> (loftr_preds (B, 4, 4) fp32,
    loftr_num_corr (B,) fp32) from data['loftr_rt'] ((3, 4) for one pair, else (B, 3, 4)) and
    data['num_correspondences_after_ransac'] -- what the reference reads from cached prediction files."""
    rt = data['loftr_rt']
    rt = (rt.unsqueeze(0) if rt.dim() == 2 else rt).detach().float()
    B = rt.shape[0]
    bottom = torch.tensor([0., 0., 0., 1.], device=rt.device).expand(B, 1, 4)
    n = data['num_correspondences_after_ransac']
    n = n if torch.is_tensor(n) else torch.as_tensor(n)
    return torch.cat([rt, bottom], dim=1), n.detach().to(rt.device).float().reshape(-1).expand(B).contiguous()


def _no_drop(**rates):
    for name, r in rates.items():
        if r:
            raise NotImplementedError(f'{name}={r}: dropout / drop-path are 0 in every 8-Point-ViT script; this package does not build '
                                      'them')


def pose_loss(outputs, gt_tran, gt_rot, w_tr, w_rot, losson6d=False):
    """The reference's training loss (interiornetStreetlearn_8ptVit/train.py:308-344) on what forward_features returns:
    w_tr mean((tran_preds - gt_tran)^2) + w_rot mean((rot_preds - gt_rot)^2); with losson6d the rotation term is on rot_preds_6d
    and gt_rot is the (B, 6) ground truth in the same (normalised or not) units.  gt_tran: (B, 3) in the units of tran_preds;
    gt_rot: (B, J, 3) rest poses under the ground-truth rotation.  Pure torch on the four returned tensors."""
    tran_preds, rot_preds, _, rot_preds_6d = outputs
    loss_tr = torch.pow(tran_preds - gt_tran, 2).mean()
    loss_rot = torch.pow((rot_preds_6d if losson6d else rot_preds) - gt_rot, 2).mean()
    return w_tr * loss_tr + w_rot * loss_rot


class Attention(nn.Module):
    """vision_transformer.py:236-262: the qkv Linear on K9 straight into head planes, K23, `proj` on K9 (the Block adds the residual
    in its epilogue).  Head dim 64 only.  forward_train is the form with gradients (block_training)."""

    block_training = False       # True: gradients run K23's training forward + HIP backward; False: a call that needs them raises
    split_operands = True        # inference: K9 operand precision of qkv / proj (False: plain fp16, ViTEss.set_precision 'blocks_dense')
    plain16 = False              # inference: K23 on plain fp16 operands (far_vit_attention_f16; ViTEss.set_precision 'blocks_attn')

    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        _no_drop(attn_drop=attn_drop, proj_drop=proj_drop)
        if dim != num_heads * 64:
            raise NotImplementedError(f'Attention: head dim {dim // num_heads} -- K23 (far_vit_attention_f16s) is a head-dim-64 kernel')
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, residual=None):
        pk = self.__dict__.setdefault('_packs', ops.PackCache())
        qkv_t = [self.qkv.weight] + ([self.qkv.bias] if self.qkv.bias is not None else [])
        sp = self.split_operands
        pq = pk.get(('qkv', sp), qkv_t, lambda: ops.PackedConv(self.qkv.weight, None, self.qkv.bias, split=sp))
        pp = pk.get(('proj', sp), [self.proj.weight, self.proj.bias], lambda: ops.PackedConv(self.proj.weight, None, self.proj.bias, split=sp))
        planes = ops.linear_f16s(x.contiguous(), pq, out_planes=3 * self.num_heads)          # (3h, Z, N, 64)
        a = ops.vit_attention_planes(planes, self.num_heads, plain16=self.plain16)          # (Z, N, C), heads concatenated
        return ops.linear_f16s(a, pp, residual=None if residual is None else residual.contiguous())

    def forward_train(self, x):
        """proj(attention(qkv(x))) with gradients: K9 forward + dgrad and K16 wgrad for both Linear layers, K23's training forward and
        HIP backward on the (Z, N, 3 C) projection in place."""
        if not self.block_training:
            raise NotImplementedError('vit8pt.Attention: gradients through K23 (far_vit_attention_f16s) are off for this module; '
                                      'ViTEss.set_block_training() / block_training = True turns the HIP backward on')
        pk = self.__dict__.setdefault('_packs', ops.PackCache())
        qkv = ops.linear_train(x, self.qkv.weight, self.qkv.bias, pk, ('train', 'qkv'))
        a = ops.vit_attention_train_qkv(qkv, self.num_heads)
        return ops.linear_train(a, self.proj.weight, self.proj.bias, pk, ('train', 'proj'))


class Block(nn.Module):
    """vision_transformer.py:265-283: x + attn(norm1(x)), then x + mlp(norm2(x)); K6, K9, K23, K9, K6, K9, K9.  With block_training
    a call that needs gradients runs the same operators with their backward kernels (K6, K9 + K16, K23 backward)."""

    block_training = False

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., drop_path=0., act_layer=nn.GELU,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        _no_drop(drop=drop, attn_drop=attn_drop, drop_path=drop_path)
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer)

    def forward(self, x, intrinsics=None):
        if ag.needs_grad(x, self.norm1.weight):
            if not self.block_training:
                raise NotImplementedError('vit8pt.Block: training / gradients through the ViT blocks are off (K23, '
                                          'far_vit_attention_f16s, runs as an inference kernel); ViTEss.set_block_training() turns the '
                                          'HIP backward on, or call it under torch.no_grad()')
            if not x.is_cuda:
                raise ops._lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
            pk = self.__dict__.setdefault('_packs', ops.PackCache())
            x = x + self.attn.forward_train(ops.layernorm_train(x.contiguous(), self.norm1))
            hid = self.mlp.act(ops.linear_train(ops.layernorm_train(x.contiguous(), self.norm2), self.mlp.fc1.weight, self.mlp.fc1.bias,
                                                pk, ('train', 'fc1')))
            return x + ops.linear_train(hid, self.mlp.fc2.weight, self.mlp.fc2.bias, pk, ('train', 'fc2'))
        x = x.contiguous()
        x = self.attn(ops.layernorm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps), residual=x)
        return self.mlp(ops.layernorm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps), residual=x)


class FusionTransformer(nn.Module):
    """The reference's trimmed VisionTransformer (model.py:63-79, :171-180): x + pos_embed, depth - 1 Blocks, the CrossBlock, the
    final LayerNorm.  forward takes cat([img0s, img1s]) (2B, 576, 192) and returns (2B, 70, 192), rows (2b, 2b + 1) = pair b.

    intrinsics: None (the plain table) or one camera's (fx, fy, cx, cy) on the 24 x 24 grid; one positional table is built per
    distinct value and kept (both datasets have one camera).  With block_training gradients pass through (pos_embed included)."""

    block_training = False

    def __init__(self, embed_dim=DIM, depth=6, num_heads=HEADS, mlp_ratio=4., qkv_bias=True, drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0.):
        super().__init__()
        _no_drop(drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate)
        if depth < 1:
            raise ValueError('transformer_depth >= 1: the last block is the CrossBlock')
        self.num_patches = GRID[0] * GRID[1]
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches, embed_dim))
        blocks = [Block(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer=NORM) for _ in range(depth - 1)]
        blocks.append(CrossBlock(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer=NORM, pos=positional_table_vit(*GRID, None)))
        self.blocks = nn.Sequential(*blocks)
        self.norm = NORM(embed_dim)
        self.apply(_init_vit)
        nn.init.xavier_uniform_(self.pos_embed)                    # model.py:77-79
        self._tables = {}

    def _table(self, key, device):
        t = self._tables.get((key, str(device)))
        if t is None:
            t = self._tables[(key, str(device))] = positional_table_vit(*GRID, key).to(device)
        return t

    def forward(self, x, intrinsics=None, taps=None):
        """taps: optional list that receives every block's output (tests)."""
        train = ag.needs_grad(x, self.pos_embed)
        if train and not self.block_training:
            raise NotImplementedError('vit8pt.FusionTransformer: training / gradients are off (K23, far_vit_attention_f16s, runs as an '
                                      'inference kernel); ViTEss.set_block_training() turns the HIP backward on, or call it under '
                                      'torch.no_grad()')
        if not x.is_cuda:
            raise ops._lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
        cross = self.blocks[-1]
        cross.cross_attn.pos6 = self._table(None if intrinsics is None else tuple(float(v) for v in intrinsics), x.device)
        x = x + self.pos_embed
        for blk in self.blocks:
            x = blk(x)
            if taps is not None:
                taps.append(x)
        if train:
            return ops.layernorm_train(x.contiguous(), self.norm)
        return ops.layernorm(x.contiguous(), self.norm.weight, self.norm.bias, self.norm.eps)


def reference_state_dict(sd, extractor=False):
    """A released checkpoint's state dict -> the entries a ViTEss of this package loads with strict=True.  extractor=True (a model
    built with the keyword): only `resnet.layer3.*` / `resnet.layer4.*` go -- the layers model.py:147-152 never runs (`resnet.fc` is an
    Identity: it has no entries); otherwise every `resnet.*` / `extractor_final_conv.*` entry goes."""
    drop = ('resnet.layer3.', 'resnet.layer4.') if extractor else ('resnet.', 'extractor_final_conv.')
    return {k: v for k, v in sd.items() if not k.startswith(drop)}


class _BasicBlock(nn.Module):
    """torchvision's BasicBlock under its parameter names (conv1, bn1, conv2, bn2, downsample.{0, 1}); run by Extractor on K9 / K17."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))


class _ResNetFront(nn.Module):
    """The layers of torchvision's ResNet18 that model.py:147-152 runs: conv1, bn1, (relu, maxpool), layer1, layer2."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.layer1 = nn.Sequential(_BasicBlock(64, 64, 1), _BasicBlock(64, 64, 1))
        self.layer2 = nn.Sequential(_BasicBlock(64, 128, 2), _BasicBlock(128, 128, 1))


class _FinalConv(nn.Module):
    """extractor.py:5-65 as model.py:60 builds it: ResidualBlock(128, 192, 'batch', kernel_size=5); downsample.1 IS norm3."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(128, DIM, 3, padding=1)
        self.conv2 = nn.Conv2d(DIM, DIM, 5)
        self.norm1 = nn.BatchNorm2d(DIM)
        self.norm2 = nn.BatchNorm2d(DIM)
        self.norm3 = nn.BatchNorm2d(DIM)
        self.downsample = nn.Sequential(nn.Conv2d(128, DIM, 5), self.norm3)


def _fold(conv, bn):
    """(scale, shift) of bn(conv(.)) with the RUNNING statistics as a per-channel affine map behind the bias-free convolution:
    scale = gamma / sqrt(var + eps), shift = beta - mean scale + scale bias; folded in float64, returned in fp32."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    if conv.bias is not None:
        shift = shift + scale * conv.bias.detach().double()
    return scale.float(), shift.float()


def _fold_tensors(conv, bn):
    return [t for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]


def _one_camera(intrinsics):
    """(B, 2, 4) -> the (fx, fy, cx, cy) every frame of the batch shares (host floats)."""
    k = intrinsics.detach().float().cpu()
    if k.dim() != 3 or tuple(k.shape[1:]) != (2, 4):
        raise ValueError(f'intrinsics: (B, 2, 4) [fx, fy, cx, cy] per frame on the feature grid, got {tuple(k.shape)}')
    if not bool(torch.all(k[:, 0] == k[:, 1])):
        raise ValueError('intrinsics differ between the two frames of a pair (the reference asserts they are equal, '
                         'vision_transformer.py:117)')
    if not bool(torch.all(k[:, 0] == k[0, 0])):
        raise NotImplementedError('per-sample intrinsics: the pairs of this batch have different cameras; one positional table per '
                                  'call is built (both datasets have one camera) -- split the batch by camera')
    return tuple(float(v) for v in k[0, 0])


class ViTEss(nn.Module):
    """model.py:38-217; the extractor only with extractor=True (module docstring).  args: fusion_transformer (must be True), transformer_depth, fc_hidden_size, pool_size
    (read, unused on this path), use_loftr_gating, use_normalized_6d, T_pose (J, 3).  global_pose_mean / global_pose_std: (9,)
    tensors, needed with use_normalized_6d (plain attributes as in the reference: not part of the state dict)."""

    def __init__(self, args, global_pose_mean=None, global_pose_std=None, extractor=False):
        super().__init__()
        self.has_extractor = bool(extractor)
        if self.has_extractor:
            # model.py:58-60 under the reference's names; frozen here (the reference fine-tunes them) until set_extractor_training()
            self.resnet = _ResNetFront()
            self.extractor_final_conv = _FinalConv()
            self.resnet.requires_grad_(False)
            self.extractor_final_conv.requires_grad_(False)
        self.total_num_features = DIM
        self.feature_resolution = GRID
        self.pose_size = 9
        self.num_patches = GRID[0] * GRID[1]
        self.H2 = args.fc_hidden_size
        self.use_loftr_gating = args.use_loftr_gating
        self.use_normalized_6d = args.use_normalized_6d
        self.global_pose_mean = global_pose_mean
        self.global_pose_std = global_pose_std
        if not args.fusion_transformer:
            raise NotImplementedError('fusion_transformer=False (the pooled-conv ablation, model.py:83-91) is not built')
        self.num_heads = HEADS
        self.transformer_depth = args.transformer_depth
        self.fusion_transformer = FusionTransformer(DIM, args.transformer_depth, HEADS)
        self.H = int(HEADS * 2 * (DIM // HEADS + 6) * (DIM // HEADS))                       # 26880
        H, H2 = self.H, self.H2
        if self.use_loftr_gating:
            self.moe_predictor = nn.Sequential(nn.Linear(H + 2 * self.pose_size + 1, H2), nn.ReLU(), nn.Linear(H2, H2), nn.ReLU(),
                                               nn.Linear(H2, 2), nn.Sigmoid())
        self.pose_regressor = nn.Sequential(nn.Linear(H, H2), nn.ReLU(), nn.Linear(H2, H2), nn.ReLU(), nn.Linear(H2, self.pose_size))
        self.T_pose = args.T_pose

    update_intrinsics = staticmethod(update_intrinsics)

    # Operand precision of the inference path, as LoFTR.set_precision: the stages that run on plain fp16 operands (one fp16 value per
    # operand, fp32 accumulation) instead of split-fp16 pairs.  NARROWER THAN THE REFERENCE: 'fp32' (no stage) is the only mode held
    # to the reference's bars and the default; the 16-bit stages exist for users who have accepted 16-bit operands, and cost
    # deviation (README, 8-Point-ViT section).  The LayerNorms (K6), the head's Linear layers (K15), K25 and K26 stay exact.
    STAGES = ('extractor',     # resnet.layer1 / layer2 and extractor_final_conv.conv1 on K9 plain fp16 (PackedConv(split=False);
                               # conv_nhwc then never takes K17), conv2 / downsample.0 on far_conv_valid_f16.  K25 (stem) and K26 unchanged.
              'blocks_dense',  # qkv, proj, fc1, fc2 of the five Blocks: K9 plain fp16
              'blocks_attn',   # K23 -> far_vit_attention_f16
              'cross')         # the CrossBlock: CrossAttention.plain16 (qkv projection + far_emm_pv_f16) and its Mlp
    MODES = {'fp32': (), 'fp16': STAGES}
    PRECISIONS = tuple(MODES)
    precision_stages = ()      # stages on 16-bit operands (set_precision); () = fp32-grade everywhere = the parity configuration
    extractor_split = True     # False: the extractor's K9 / K24 launches on plain fp16 operands ('extractor')

    def set_precision(self, mode):
        """mode: a name of MODES ('fp32': every product on split-fp16 operand pairs, fp32-grade, the parity configuration and the
        default; 'fp16': every stage on plain fp16 operands) or an iterable of STAGES names (the stages that run on 16-bit operands).
        Inference only: a call that needs gradients while a stage is on raises NotImplementedError (training stays fp32-grade);
        under torch.no_grad(), or in .eval() without gradients, the stages apply whatever the training switches say.  Sets
        `precision_stages` (a tuple in STAGES order) and plain attributes on the submodules; the state dict does not change, and
        every weight image is cached under its operand class, so going back to 'fp32' gives the bits from before.  Returns self."""
        if isinstance(mode, str):
            if mode not in self.MODES:
                raise ValueError(f'precision must be one of {self.PRECISIONS} or an iterable of {self.STAGES}')
            st = set(self.MODES[mode])
        else:
            try:
                st = set(mode)
            except TypeError:
                raise ValueError(f'precision must be one of {self.PRECISIONS} or an iterable of {self.STAGES}') from None
            if not all(isinstance(s, str) for s in st) or not st <= set(self.STAGES):
                raise ValueError(f'unknown precision stages {sorted(map(str, st - set(self.STAGES)))}; known: {self.STAGES} '
                                 f'(or a mode: {self.PRECISIONS})')
        if 'extractor' in st and not self.has_extractor:
            raise ValueError("precision stage 'extractor': this model was built without extractor=True -- it has no extractor to "
                             f'switch; the stages of the trunk are {self.STAGES[1:]}')
        self.precision_stages = tuple(s for s in self.STAGES if s in st)
        self.extractor_split = 'extractor' not in st
        for blk in self.fusion_transformer.blocks:
            if isinstance(blk, Block):
                blk.attn.split_operands = blk.mlp.split_operands = 'blocks_dense' not in st
                blk.attn.plain16 = 'blocks_attn' in st
            else:                                                   # the CrossBlock
                blk.cross_attn.plain16 = 'cross' in st
                blk.mlp.split_operands = 'cross' not in st
        return self

    def _precision_no_grad(self, what):
        return NotImplementedError(f'ViTEss.{what}: gradients are wanted while the precision stages {self.precision_stages} are on -- '
                                   "the 16-bit-operand stages are inference only (no 16-bit backward kernels exist; training stays "
                                   "fp32-grade): call set_precision('fp32') before training, or run under torch.no_grad()")

    def set_block_training(self, on=True):
        """Opt in to (or out of) gradients through the trunk: sets `block_training` on the FusionTransformer, its Blocks and their
        Attention modules -- plain instance attributes, the state dict's keys do not change.  Returns self."""
        on = bool(on)
        ft = self.fusion_transformer
        ft.block_training = on
        for blk in ft.blocks:
            if isinstance(blk, Block):
                blk.block_training = blk.attn.block_training = on
        return self

    def set_extractor_training(self, part='final', on=True):
        """Opt in to (or out of) fine-tuning the extractor's final block (extractor_final_conv, half of the extractor's arithmetic)
        with the trunk: sets the plain attribute `extractor_training` and requires_grad on the extractor_final_conv.* parameters; the
        state dict's keys do not change.  In .train() mode under enabled gradients extract_features then runs the block on the
        training kernels (batch statistics, K9 + K16, K24 forward + backward, K19) and its output carries gradients; the ResNet front
        stays frozen on its running statistics.  Returns self."""
        if not self.has_extractor:
            raise self._no_extractor()
        if part != 'final':
            raise NotImplementedError(f"ViTEss.set_extractor_training(part={part!r}): only part='final' (extractor_final_conv) trains; "
                                      'gradients into resnet.* need backward kernels for K25 (far_stem_rgb_f16s) and K26 '
                                      '(far_maxpool3x3s2_nhwc_f32), which do not exist')
        self.extractor_training = bool(on)
        self.extractor_final_conv.requires_grad_(bool(on))
        return self

    def _final_block_train(self, x):
        """extractor.py:51-65 in training mode with gradients: x (N, H, W, 128) NHWC fp32 -> (N, H - 4, W - 4, 192) NHWC.  conv1 on K9 +
        K16 (ops.conv_train), conv2 / downsample.0 on K24 forward + backward (ops.conv_valid_train), the three BatchNorm layers with
        batch statistics on K19 (ops.bn_act_train: norm3 takes the block's add and final ReLU); the convolution biases are torch
        elementwise adds in front of the BatchNorm (running_mean then equals the module's; their gradients come from autograd)."""
        fc = self.extractor_final_conv
        pk = self.__dict__.setdefault('_extractor_train_packs', ops.PackCache())
        nchw = lambda t: t.permute(0, 3, 1, 2)                       # NHWC tensor -> (N, C, H, W) logical, channels_last memory
        y = ops.conv_train(nchw(x), fc.conv1.weight, 1, pk, 'final.conv1') + fc.conv1.bias.view(1, -1, 1, 1)
        y = ops.bn_act_train(y, fc.norm1, act='relu')                                                    # extractor.py:53
        y = ops.conv_valid_train(y.permute(0, 2, 3, 1), fc.conv2.weight, pk, 'final.conv2') + fc.conv2.bias
        y = ops.bn_act_train(nchw(y), fc.norm2, act='relu')                                              # :54
        d = ops.conv_valid_train(x, fc.downsample[0].weight, pk, 'final.downsample') + fc.downsample[0].bias
        return ops.bn_act_train(nchw(d), fc.norm3, act='relu', residual=y).permute(0, 2, 3, 1)           # :56-57, :65

    def _no_extractor(self):
        return NotImplementedError('ViTEss.forward(images): the extractor (torchvision ResNet18 conv1 .. layer2 + ResidualBlock, '
                                   'model.py:131-163) is not built -- torchvision is not a dependency of this package.  Run it '
                                   'elsewhere and call forward_features(features, intrinsics, loftr_num_corr, loftr_preds) with its '
                                   '(2B, 576, 192) output and update_intrinsics(images.shape, intrinsics)')

    def forward(self, images, intrinsics=None, inference=False, loftr_num_corr=None, loftr_preds=None):
        """model.py:165-217 from images (a model built with extractor=True): images (B, 2, 3, H, W) fp32 on the GPU, values 0 .. 255
        in the channel order the reference takes, left unmodified; intrinsics: None or (B, 2, 4) [fx, fy, cx, cy] AT THE IMAGE SIZE.
        The same bits as forward_features(*extract_features(images, intrinsics), loftr_num_corr, loftr_preds)."""
        if not self.has_extractor:
            raise self._no_extractor()
        return self.forward_features(*self.extract_features(images, intrinsics), loftr_num_corr, loftr_preds)

    def _block(self, pk, name, blk, x):
        """One BasicBlock on K9 / K17: relu(bn1(conv1(x))), then relu(bn2(conv2(.)) + shortcut) with the add and the ReLU in conv2's
        epilogue; the 1x1 stride-2 shortcut reads x[:, ::2, ::2] in place (in_stride = 2)."""
        st = blk.conv1.stride[0]
        sp = self.extractor_split                                   # False: plain fp16 operands (conv_nhwc then never takes K17)
        fold = lambda conv, bn, **kw: (lambda: ops.PackedConv(conv.weight, *_fold(conv, bn), split=sp, **kw))
        p1 = pk.get((name + '.conv1', sp), _fold_tensors(blk.conv1, blk.bn1), fold(blk.conv1, blk.bn1, stride=st))
        p2 = pk.get((name + '.conv2', sp), _fold_tensors(blk.conv2, blk.bn2), fold(blk.conv2, blk.bn2))
        y = ops.conv_nhwc(x, p1, act='relu')
        if blk.downsample is not None:
            pd = pk.get((name + '.downsample', sp), _fold_tensors(blk.downsample[0], blk.downsample[1]),
                        fold(blk.downsample[0], blk.downsample[1]))
            x = ops.conv_nhwc(x, pd, in_stride=st)
        return ops.conv_nhwc(y, p2, residual=x, act='relu')

    def extract_features(self, images, intrinsics=None):
        """model.py:131-163: images (B, 2, 3, H, W) fp32 on the GPU, 0 .. 255 -> (features (2B, 576, 192) with rows (2b, 2b + 1) = pair
        b, intrinsics on the 24 x 24 grid (update_intrinsics with the ORIGINAL image size; None stays None)).  14 launches: K25 (flip,
        normalisation, resize to 224, conv1, bn1, relu), K26 (maxpool), K9 / K17 (layer1, layer2, extractor_final_conv.conv1), K24
        (the two 5x5 convolutions with the block's add and ReLUs).  BatchNorm uses its running statistics whatever .train() says;
        the extractor is frozen: the features carry no gradient.  `images` is only read.
        After set_extractor_training(), in .train() mode under enabled gradients, the ResNet front runs exactly as above and the final
        block runs _final_block_train: batch statistics, gradients into extractor_final_conv.* and through the features.  One
        deviation from the reference remains there: the frozen front keeps its running statistics in .train(), where the reference's
        whole model uses batch statistics.  Under torch.no_grad(), or in .eval() without gradients, the switch changes nothing."""
        if not self.has_extractor:
            raise self._no_extractor()
        if not torch.is_tensor(images) or images.dim() != 5 or tuple(images.shape[1:3]) != (2, 3):
            raise ValueError(f'images: (B, 2, 3, H, W), got {tuple(images.shape) if torch.is_tensor(images) else type(images)}')
        train_final = False
        if torch.is_grad_enabled():
            switch = bool(getattr(self, 'extractor_training', False))
            if any(p.requires_grad for p in self.resnet.parameters()):
                raise NotImplementedError('ViTEss: training the extractor front (resnet.*) is not built -- K25 / K26 have no backward '
                                          'kernels and its BatchNorm layers use running statistics; keep its parameters at '
                                          'requires_grad=False (set_extractor_training() trains extractor_final_conv only) or call it '
                                          'under torch.no_grad()')
            wanted = any(p.requires_grad for p in self.extractor_final_conv.parameters())
            if wanted and not switch:
                raise NotImplementedError('ViTEss: an extractor_final_conv.* parameter has requires_grad=True but training the extractor '
                                          'is off: ViTEss.set_extractor_training() turns the HIP backward of the final block on; or keep '
                                          'the parameters at requires_grad=False / call it under torch.no_grad()')
            if wanted and not self.extractor_final_conv.training:
                raise NotImplementedError('ViTEss: gradients into extractor_final_conv.* are wanted (set_extractor_training()) with the '
                                          'block in .eval() mode: its training kernels use batch statistics -- call .train(), '
                                          'set_extractor_training(on=False), or run under torch.no_grad()')
            if wanted and self.precision_stages:
                raise self._precision_no_grad('extract_features')
            train_final = wanted
        if not images.is_cuda:
            raise ops._lib.FarHipError('far_amd ops need tensors on the GPU (no CPU fallback exists)')
        grid_intrinsics = None if intrinsics is None else update_intrinsics(images.shape, intrinsics)
        pk = self.__dict__.setdefault('_extractor_packs', ops.PackCache())
        rn, fc = self.resnet, self.extractor_final_conv
        with torch.no_grad():
            stem = pk.get('stem', _fold_tensors(rn.conv1, rn.bn1), lambda: ops.PackedStemRGB(rn.conv1.weight, *_fold(rn.conv1, rn.bn1)))
            x = ops.maxpool3x3s2(ops.stem_rgb(images.detach().flatten(0, 1).contiguous(), stem))          # (2B, 56, 56, 64) NHWC
            for lname, layer in (('layer1', rn.layer1), ('layer2', rn.layer2)):
                for i, blk in enumerate(layer):
                    x = self._block(pk, f'{lname}.{i}', blk, x)                                          # -> (2B, 28, 28, 128)
        if train_final:
            # the final block on the training kernels: its output carries gradients into the trunk (set_extractor_training)
            x = self._final_block_train(x)
            return x.reshape(x.shape[0], self.num_patches, DIM), grid_intrinsics
        with torch.no_grad():
            sp = self.extractor_split                               # False: K9 / K24 on plain fp16 operands (set_precision 'extractor')
            p1 = pk.get(('final.conv1', sp), _fold_tensors(fc.conv1, fc.norm1),
                        lambda: ops.PackedConv(fc.conv1.weight, *_fold(fc.conv1, fc.norm1), split=sp))
            p2 = pk.get(('final.conv2', sp), _fold_tensors(fc.conv2, fc.norm2),
                        lambda: ops.PackedConvValid(fc.conv2.weight, *_fold(fc.conv2, fc.norm2), split=sp))
            pd = pk.get(('final.downsample', sp), _fold_tensors(fc.downsample[0], fc.norm3),
                        lambda: ops.PackedConvValid(fc.downsample[0].weight, *_fold(fc.downsample[0], fc.norm3), split=sp))
            y = ops.conv_valid(ops.conv_nhwc(x, p1, act='relu'), p2, act='relu')                        # extractor.py:53-54
            x = ops.conv_valid(x, pd, residual=y, act='relu')                                            # :56-57, :65 -> (2B, 24, 24, 192)
        # model.py:156-161: (2B, 192, 576) permuted to (2B, 576, 192) is the NHWC tensor itself; the channel cut [:, :192] is a no-op
        return x.reshape(x.shape[0], self.num_patches, DIM), grid_intrinsics

    def trunk(self, features, intrinsics=None, taps=None):
        """(2B, 576, 192) extractor output in the reference's pair order -> the (2B, 70, 192) normalised features (model.py:171-180).
        taps (tests): receives each block's output, Blocks in the reference's pair order."""
        if features.dim() != 3 or features.shape[0] % 2 or tuple(features.shape[1:]) != (self.num_patches, DIM):
            raise ValueError(f'features: (2B, {self.num_patches}, {DIM}) with rows (2b, 2b + 1) = pair b, got {tuple(features.shape)}')
        if self.precision_stages and ag.needs_grad(features, self.fusion_transformer.pos_embed):
            raise self._precision_no_grad('trunk')
        cam = None if intrinsics is None else _one_camera(intrinsics)
        got = None if taps is None else []
        out = self.fusion_transformer(interleaved_to_concatenated(features.float()), cam, got)
        if taps is not None:
            taps.extend([concatenated_to_interleaved(t) for t in got[:-1]] + got[-1:])
        return out

    def forward_features(self, features, intrinsics=None, loftr_num_corr=None, loftr_preds=None):
        """model.py:171-217 from the extractor's output.  features: (2B, 576, 192) fp32 on the GPU, rows (2b, 2b + 1) = the two images
        of pair b; intrinsics: None or (B, 2, 4) [fx, fy, cx, cy] ON THE FEATURE GRID (update_intrinsics), equal in both frames
        (ValueError otherwise) and, in this package, equal for every pair of the batch -- differing cameras raise
        NotImplementedError; loftr_preds (B, 4, 4), loftr_num_corr (B,): the solver's pose and inlier count (loftr_gate_inputs),
        needed with use_loftr_gating.  Returns the reference's (tran_preds_unnorm (B, 3), rot_preds (B, J, 3), rot_preds_mtx
        (B, 3, 3), rot_preds_6d (B, 6)).  Pair b's outputs do not depend on the batch it is computed in."""
        feats = self.trunk(features, intrinsics)
        B = feats.shape[0] // 2
        feats = feats.reshape(B, -1)                                                       # (B, 26880)
        dev = feats.device
        pk = self.__dict__.setdefault('_packs', ops.PackCache())
        lin = lambda name, m, **kw: pk.get(name, [m.weight, m.bias], lambda: ops.PackedRows(m.weight, m.bias, **kw))
        reg = self.pose_regressor
        mean = std = None
        if self.use_normalized_6d:
            if self.global_pose_mean is None or self.global_pose_std is None:
                raise ValueError('use_normalized_6d needs global_pose_mean and global_pose_std')
            mean, std = self.global_pose_mean.to(dev).float(), self.global_pose_std.to(dev).float()
        if self.use_loftr_gating and (loftr_preds is None or loftr_num_corr is None):
            raise ValueError('use_loftr_gating needs loftr_preds (B, 4, 4) and loftr_num_corr (B,)')
        if ag.needs_grad(feats, reg[0].weight, self.moe_predictor[0].weight if self.use_loftr_gating else None):
            # training: the two small parameter containers under autograd (far_amd/_vendor.py; the mp3d head's forward_emm does the
            # same) -- the same function as below, model.py:181-205; the reg0 | moe0 merge is an inference optimisation only
            pred_reg_6d = reg(feats)
            if self.use_loftr_gating:
                rt = loftr_preds.to(dev).float()
                solver_6d = torch.cat([rt[..., :3, 3], rt[..., :2, :3].reshape(B, 6)], dim=-1)
                if self.use_normalized_6d:
                    solver_6d = (solver_6d - mean) / std
                ncorr = loftr_num_corr.detach().to(dev).float().reshape(B, 1) / 500
                solver_6d = torch.cat([solver_6d, ncorr], dim=-1)
                wt = self.moe_predictor(torch.cat([feats, pred_reg_6d, solver_6d], dim=-1))
                pred_T = wt[..., :1] * pred_reg_6d[..., :3] + (1 - wt[..., :1]) * solver_6d[..., :3]
                pred_R = wt[..., 1:] * pred_reg_6d[..., 3:] + (1 - wt[..., 1:]) * solver_6d[..., 3:-1]
                pose = torch.cat([pred_T, pred_R], dim=-1)
            else:
                pose = pred_reg_6d
            return self._pose_outputs(pose, mean, std)
        if self.use_loftr_gating:
            moe = self.moe_predictor
            # the two 26880-wide first layers read the features only: one K15 launch for both (no bias yet)
            both = pk.get('reg0|moe0', [reg[0].weight, moe[0].weight],
                          lambda: ops.PackedRows(torch.cat([reg[0].weight, moe[0].weight[:, :self.H]], 0)))
            pre = ops.rows_linear(feats, both)                                             # (B, 2 H2)
            h = torch.relu(pre[:, :self.H2] + reg[0].bias)
        else:
            h = ops.rows_linear(feats, lin('reg0', reg[0]), act='relu')
        h = ops.rows_linear(h, lin('reg2', reg[2]), act='relu')
        pred_reg_6d = ops.rows_linear(h, lin('reg4', reg[4]))                              # (B, 9)
        if self.use_loftr_gating:
            rt = loftr_preds.to(dev).float()
            solver_6d = torch.cat([rt[..., :3, 3], rt[..., :2, :3].reshape(B, 6)], dim=-1)      # compute_6d, model.py:11-30
            if self.use_normalized_6d:
                solver_6d = (solver_6d - mean) / std
            ncorr = loftr_num_corr.detach().to(dev).float().reshape(B, 1) / 500
            solver_6d = torch.cat([solver_6d, ncorr], dim=-1)                              # (B, 10)
            tail = torch.cat([pred_reg_6d, solver_6d], dim=-1).contiguous()                # (B, 19)
            g = ops.rows_linear(tail, lin('moe0-tail', moe[0], cols=(self.H, moe[0].weight.shape[1])), act='relu',
                                add=pre[:, self.H2:])
            g = ops.rows_linear(g, lin('moe2', moe[2]), act='relu')
            wt = ops.rows_linear(g, lin('moe4', moe[4]), act='sigmoid')                    # (B, 2)
            pred_T = wt[..., :1] * pred_reg_6d[..., :3] + (1 - wt[..., :1]) * solver_6d[..., :3]
            pred_R = wt[..., 1:] * pred_reg_6d[..., 3:] + (1 - wt[..., 1:]) * solver_6d[..., 3:-1]
            pose = torch.cat([pred_T, pred_R], dim=-1)
        else:
            pose = pred_reg_6d
        return self._pose_outputs(pose, mean, std)

    def _pose_outputs(self, pose, mean, std):
        """model.py:206-217: the (B, 9) pose -> the four returned tensors."""
        rot_6d, tran = pose[:, 3:], pose[:, :3]
        if self.use_normalized_6d:
            rot_unnorm = rot_6d * std[3:] + mean[3:]
            tran_unnorm = tran * std[:3] + mean[:3]
        else:
            rot_unnorm, tran_unnorm = rot_6d, tran
        mtx = rotation_matrix_from_ortho6d(rot_unnorm)
        return tran_unnorm, pose_from_rotation_matrix(self.T_pose, mtx), mtx, rot_6d
