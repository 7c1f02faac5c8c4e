"""A dtype-generic torch restatement (fp32 / float64, CPU or GPU) of the 8-Point-ViT regressor behind its extractor: Attention and
Block (vision_transformer.py:236-283), CrossAttention / CrossBlock (:160-234), the trunk and the head (model.py:171-217), the 6D ->
matrix map (tools.py:20-60).  Plain dense tensor algebra, the (N, N) score tensors materialised: the yardstick of the GPU tests
(float64) and the source of their dev32 (fp32, same device, same run).  RefViTEss carries the reference's parameter names, so its
state dict is what a released checkpoint looks like without `resnet.*` / `extractor_final_conv.*`.

tests/test_vit8pt_cpu.py pins it to the reference's own fp32 run (golden G25, tools/make_golden_vit8pt.py)."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

DIM, HEADS, GRID = 192, 3, 24


def attention_ref(q, k, v, nhead, dtype=torch.float64, chunk=256):
    """softmax_s(q . k / sqrt(D)) v per head.  q (Z, L, C), k, v (Z, S, C), heads concatenated -> (Z, L, C) in `dtype`."""
    Z, L, C = q.shape
    S, D = k.shape[1], C // nhead
    qh = q.to(dtype).view(Z, L, nhead, D).permute(0, 2, 1, 3)
    kh = k.to(dtype).view(Z, S, nhead, D).permute(0, 2, 1, 3)
    vh = v.to(dtype).view(Z, S, nhead, D).permute(0, 2, 1, 3)
    out = torch.empty(Z, nhead, L, D, dtype=dtype, device=q.device)
    for z in range(0, Z, chunk):
        a = (qh[z:z + chunk] @ kh[z:z + chunk].transpose(-2, -1)) * D ** -0.5
        out[z:z + chunk] = a.softmax(dim=-1) @ vh[z:z + chunk]
    return out.permute(0, 2, 1, 3).reshape(Z, L, C)


def positional(intrinsics, dtype, device):
    """The (576, 6) table of vision_transformer.py:90-158, computed in fp32 as the reference does, then cast.  intrinsics: None or
    (fx, fy, cx, cy)."""
    from far_amd.loftr.transformer import positional_table_vit
    return positional_table_vit(GRID, GRID, intrinsics).to(device=device, dtype=dtype)


class _Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(dim, 4 * dim), nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class _Attention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)

    def forward(self, x):
        q, k, v = self.qkv(x).chunk(3, dim=-1)                     # channel = t h d + head d + c (:252)
        return self.proj(attention_ref(q, k, v, self.heads, x.dtype))


class _Block(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.norm1, self.attn = nn.LayerNorm(dim, eps=1e-6), _Attention(dim, heads)
        self.norm2, self.mlp = nn.LayerNorm(dim, eps=1e-6), _Mlp(dim)

    def forward(self, x, pos=None):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class _CrossAttention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.qkv, self.proj_fundamental = nn.Linear(dim, 3 * dim), nn.Linear(dim + 6 * heads, dim)

    def forward(self, x1, x2, pos):
        B, N, C = x1.shape
        h, d = self.heads, C // self.heads
        split = lambda x: self.qkv(x).reshape(B, N, 3, h, d).permute(2, 0, 3, 1, 4)
        (q1, k1, v1), (q2, k2, v2) = split(x1), split(x2)
        out = []
        for q, k, v in ((q2, k1, v1), (q1, k2, v2)):
            a = (q @ k.transpose(-2, -1)) * d ** -0.5
            a = a.softmax(dim=-1) * a.softmax(dim=-2)
            vp = torch.cat([v, pos.expand(B, h, N, 6)], dim=3)
            f = (vp.transpose(-2, -1) @ a) @ vp                                         # (B, h, 70, 70)
            out.append(self.proj_fundamental(f.reshape(B, C + 6 * h, (C + 6 * h) // h).transpose(-2, -1)))
        return out[1], out[0]                                                            # flipped (:206-208)


class _CrossBlock(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.norm1, self.cross_attn = nn.LayerNorm(dim, eps=1e-6), _CrossAttention(dim, heads)
        self.norm2, self.mlp = nn.LayerNorm(dim, eps=1e-6), _Mlp(dim)

    def forward(self, x, pos):
        b_s, h_w, nf = x.shape
        x = x.reshape(-1, 2, h_w, nf)                                                    # rows (2b, 2b + 1) = pair b (:226-228)
        f1, f2 = self.cross_attn(self.norm1(x[:, 0]), self.norm1(x[:, 1]), pos)
        f = torch.cat([f1.unsqueeze(1), f2.unsqueeze(1)], dim=1).reshape(b_s, -1, nf)
        return f + self.mlp(self.norm2(f))


class _Trunk(nn.Module):
    def __init__(self, depth):
        super().__init__()
        self.pos_embed = nn.Parameter(torch.zeros(1, GRID * GRID, DIM))
        self.blocks = nn.Sequential(*[_Block(DIM, HEADS) for _ in range(depth - 1)], _CrossBlock(DIM, HEADS))
        self.norm = nn.LayerNorm(DIM, eps=1e-6)


def rotation_from_6d(o6):
    floor = torch.tensor(1e-8, dtype=o6.dtype, device=o6.device)
    unit = lambda v: v / torch.maximum(v.pow(2).sum(1).sqrt(), floor)[:, None]
    x = unit(o6[:, :3])
    z = unit(torch.linalg.cross(x, o6[:, 3:6]))
    y = torch.linalg.cross(z, x)
    return torch.stack([x, y, z], dim=2)


class RefViTEss(nn.Module):
    """forward_features of the reference model (fusion_transformer=True), every tensor in the parameters' dtype."""

    def __init__(self, args, pose_mean=None, pose_std=None):
        super().__init__()
        self.args, self.pose_mean, self.pose_std = args, pose_mean, pose_std
        self.fusion_transformer = _Trunk(args.transformer_depth)
        H, H2 = HEADS * 2 * (DIM // HEADS + 6) * (DIM // HEADS), args.fc_hidden_size
        if args.use_loftr_gating:
            self.moe_predictor = nn.Sequential(nn.Linear(H + 19, H2), nn.ReLU(), nn.Linear(H2, H2), nn.ReLU(), nn.Linear(H2, 2), nn.Sigmoid())
        self.pose_regressor = nn.Sequential(nn.Linear(H, H2), nn.ReLU(), nn.Linear(H2, H2), nn.ReLU(), nn.Linear(H2, 9))

    def as_dtype(self, dtype, device=None):
        m = copy.deepcopy(self).to(dtype=dtype)
        return m if device is None else m.to(device)

    def trunk(self, features, intrinsics=None, taps=None):
        """features (2B, 576, 192), rows (2b, 2b + 1) = pair b; intrinsics None or (fx, fy, cx, cy).  taps: receives block outputs."""
        ft = self.fusion_transformer
        dt, dev = ft.pos_embed.dtype, ft.pos_embed.device
        pos = positional(intrinsics, dt, dev)
        x = features.to(device=dev, dtype=dt) + ft.pos_embed
        for blk in ft.blocks:
            x = blk(x, pos)
            if taps is not None:
                taps.append(x)
        return ft.norm(x)

    @torch.no_grad()
    def forward_features(self, features, intrinsics=None, loftr_num_corr=None, loftr_preds=None):
        a = self.args
        feats = self.trunk(features, intrinsics)
        dt, dev = feats.dtype, feats.device
        B = feats.shape[0] // 2
        feats = feats.reshape(B, -1)
        pred = self.pose_regressor(feats)
        if a.use_normalized_6d:
            mean, std = self.pose_mean.to(device=dev, dtype=dt), self.pose_std.to(device=dev, dtype=dt)
        if a.use_loftr_gating:
            rt = loftr_preds.to(device=dev, dtype=dt)
            s6 = torch.cat([rt[:, :3, 3], rt[:, :2, :3].reshape(B, 6)], dim=-1)
            if a.use_normalized_6d:
                s6 = (s6 - mean) / std
            s6 = torch.cat([s6, loftr_num_corr.to(device=dev, dtype=dt).reshape(B, 1) / 500], dim=-1)
            wt = self.moe_predictor(torch.cat([feats, pred, s6], dim=-1))
            pose = torch.cat([wt[:, :1] * pred[:, :3] + (1 - wt[:, :1]) * s6[:, :3],
                              wt[:, 1:] * pred[:, 3:] + (1 - wt[:, 1:]) * s6[:, 3:-1]], dim=-1)
        else:
            pose = pred
        r6, t = pose[:, 3:], pose[:, :3]
        r6u, tu = (r6 * std[3:] + mean[3:], t * std[:3] + mean[:3]) if a.use_normalized_6d else (r6, t)
        mtx = rotation_from_6d(r6u)
        rot = (mtx[:, None] @ a.T_pose.to(device=dev, dtype=dt).reshape(1, -1, 3, 1)).squeeze(-1)
        return tu, rot, mtx, r6


def fill_conditions(model64, features, intrinsics):
    """The figures tests/vit8pt_inputs.py promises, measured on a float64 RefViTEss: per Block the score span, the median / minimum
    over rows of the largest attention probability and max|q, k, v|; the largest Block and CrossBlock outputs."""
    ft = model64.fusion_transformer
    out = {'blocks': []}
    taps = []
    with torch.no_grad():
        model64.trunk(features, intrinsics, taps)
        x = features.to(ft.pos_embed.dtype) + ft.pos_embed
        for i, blk in enumerate(ft.blocks[:-1]):
            qkv = blk.attn.qkv(blk.norm1(x))
            q, k, _ = (t.view(*t.shape[:2], HEADS, 64).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
            s = (q @ k.transpose(-2, -1)) / 8
            pmax = s.softmax(-1).amax(-1)
            out['blocks'].append(dict(score_min=float(s.min()), score_max=float(s.max()), pmax_median=float(pmax.median()),
                                      pmax_min=float(pmax.min()), qkv_absmax=float(qkv.abs().max()), out_absmax=float(taps[i].abs().max())))
            x = taps[i]
    out['cross_absmax'] = float(taps[-1].abs().max())
    return out
