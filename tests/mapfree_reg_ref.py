"""A plain torch.nn restatement of the Map-free regressor (mapfree_6dreg/lib/models/regression: encoder/resunet.py:105-128,
encoder/preact.py:13-64, aggregator.py:44-115, head.py:27-55, model.py:57-61, 198-233, 235-308) under the reference's parameter names,
usable in fp32 and float64 on either device: the comparison leg of the GPU tests (float64) and of tools/mapfree_reg_time.py (fp32).
tests/test_mapfree_regressor_cpu.py pins it to golden G28, which the reference's own classes produced."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class PreActBlock(nn.Module):
    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.conv1 = nn.Conv2d(in_planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        if stride != 1 or in_planes != planes:
            self.shortcut = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride, bias=False))

    def forward(self, x, taps=None):
        out = F.relu(self.bn1(x))
        _note(taps, out)
        shortcut = self.shortcut(out) if hasattr(self, 'shortcut') else x
        out = F.relu(self.bn2(self.conv1(out)))
        _note(taps, out)
        return self.conv2(out) + shortcut


class PreActBottleneck(nn.Module):
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

    def forward(self, x, taps=None):
        out = F.relu(self.bn1(x))
        _note(taps, out)
        shortcut = self.shortcut(out) if hasattr(self, 'shortcut') else x
        out = F.relu(self.bn2(self.conv1(out)))
        _note(taps, out)
        out = F.relu(self.bn3(self.conv2(out)))
        _note(taps, out)
        return self.conv3(out) + shortcut


def _note(taps, act):
    """taps: None or a list that receives (positive share, max |.|) of an activation's output."""
    if taps is not None:
        taps.append((float((act > 0).double().mean()), float(act.abs().max())))


class ConvBNELU(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, 1, (k - 1) // 2)
        self.normalize = nn.BatchNorm2d(cout)

    def forward(self, x, taps=None):
        x = F.elu(self.normalize(self.conv(x)))
        _note(taps, x)
        return x


class UpConv(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = ConvBNELU(cin, cout, 3)

    def forward(self, x, taps=None):
        return self.conv1(F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True), taps)


def skipconnect(x1, x2):
    dy, dx = x2.shape[2] - x1.shape[2], x2.shape[3] - x1.shape[3]
    return torch.cat([x2, F.pad(x1, (dx // 2, dx - dx // 2, dy // 2, dy - dy // 2))], dim=1)


class ResUNet(nn.Module):
    def __init__(self, num_out_layers=32):
        super().__init__()
        self.firstconv = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.firstbn = nn.BatchNorm2d(64)
        planes_in = [64]

        def layer(planes, stride):
            blocks = []
            for st in (stride, 1, 1):
                blocks.append(PreActBottleneck(planes_in[0], planes, st))
                planes_in[0] = 4 * planes
            return nn.Sequential(*blocks)
        self.encoder1, self.encoder2, self.encoder3 = layer(64, 1), layer(128, 2), layer(256, 2)
        self.upconv4 = UpConv(1024, 512)
        self.iconv4 = ConvBNELU(1024, 512, 3)
        self.upconv3 = UpConv(512, 256)
        self.iconv3 = ConvBNELU(512, 256, 3)
        self.outconv = ConvBNELU(256, num_out_layers, 1)

    def forward(self, x, taps=None):
        x1 = F.relu(self.firstbn(self.firstconv(x)))
        _note(taps, x1)
        x = F.max_pool2d(x1, 3, 2, 1)
        skips = []
        for enc in (self.encoder1, self.encoder2, self.encoder3):
            for blk in enc:
                x = blk(x, taps)
            skips.append(x)
        x2, x3, x4 = skips
        x = self.iconv4(skipconnect(x3, self.upconv4(x4, taps)), taps)
        x = self.iconv3(skipconnect(x2, self.upconv3(x, taps)), taps)
        return self.outconv(x, taps)


def corr_volume_warp(vol0, vol1):
    """aggregator.py:44-115 with POSITION_ENCODER and MAX_SCORE_CHANNEL: (B, D, H, W) x 2 -> (B, 2 D + 3, H, W)."""
    B, D, H, W = vol0.shape
    a, b = vol0.reshape(B, D, H * W), vol1.reshape(B, D, H * W)
    cv = torch.softmax(torch.bmm(a.transpose(1, 2), b), dim=2)
    warped = torch.bmm(b, cv.transpose(1, 2))
    u = torch.linspace(-1, 1, H).to(device=vol0.device, dtype=vol0.dtype)        # fp32 linspace, as the reference forms it
    v = torch.linspace(-1, 1, W).to(device=vol0.device, dtype=vol0.dtype)
    uu, vv = torch.meshgrid(u, v, indexing='ij')
    grid = torch.stack([uu, vv], dim=0).reshape(1, 2, H * W).expand(B, 2, H * W)
    pos = torch.bmm(grid, cv.transpose(1, 2))
    mx = cv.max(dim=2, keepdim=True)[0].transpose(1, 2)
    return torch.cat([a, warped, pos, mx], dim=1).reshape(B, -1, H, W)


class DeepResBlock(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.resblock1 = PreActBlock(in_channels, 64, 2)
        self.resblock2 = PreActBlock(64, 128, 2)
        self.resblock3 = PreActBlock(128, 256, 2)

    def forward(self, x, taps=None):
        return self.resblock3(self.resblock2(self.resblock1(x, taps), taps), taps)


def encoder_layer(layer, x, nhead):
    """One post-norm nn.TransformerEncoderLayer (ReLU, dropout inactive) on x (S, N, E), written out."""
    S, N, E = x.shape
    at = layer.self_attn
    q, k, v = F.linear(x, at.in_proj_weight, at.in_proj_bias).chunk(3, dim=-1)
    heads = lambda t: t.reshape(S, N * nhead, E // nhead).transpose(0, 1)                   # (N h, S, d)
    p = torch.softmax(torch.bmm(heads(q), heads(k).transpose(1, 2)) / (E // nhead) ** 0.5, dim=-1)
    a = torch.bmm(p, heads(v)).transpose(0, 1).reshape(S, N, E)
    x = F.layer_norm(x + F.linear(a, at.out_proj.weight, at.out_proj.bias), (E,), layer.norm1.weight, layer.norm1.bias, layer.norm1.eps)
    y = F.linear(F.relu(F.linear(x, layer.linear1.weight, layer.linear1.bias)), layer.linear2.weight, layer.linear2.bias)
    return F.layer_norm(x + y, (E,), layer.norm2.weight, layer.norm2.bias, layer.norm2.eps)


def rotation_6d_to_matrix(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


class RefRegressionModel(nn.Module):
    """The reference's RegressionModel(use_loftr_preds, use_vanilla_transformer, use_prior) without its matcher and solver: the state
    dict has the reference's names and shapes (minus matcher.*)."""

    def __init__(self, use_prior=False):
        super().__init__()
        self.use_prior = use_prior
        self.encoder = ResUNet(32)
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=256, nhead=8), num_layers=6, enable_nested_tensor=False)
        self.head = DeepResBlock(67)
        H, H2 = 256 * 12 * 9, 512
        self.moe_predictor = nn.Sequential(nn.Linear(H + 21, H2), nn.ReLU(), nn.Linear(H2, H2), nn.ReLU(), nn.Linear(H2, 2), nn.Sigmoid())
        self.pose_regressor = nn.Sequential(nn.Linear(H, H2), nn.ReLU(), nn.Linear(H2, H2), nn.ReLU(), nn.Linear(H2, 9))
        self.eval()

    def encode(self, images, taps=None):
        return self.encoder(images, taps)

    def features(self, vol0, vol1, taps=None, out=None):
        agg = corr_volume_warp(vol0, vol1)
        x3 = self.head(agg, taps)
        B, C, H, W = x3.shape
        x = x3.reshape(B, C, H * W).permute(2, 0, 1)
        for layer in self.transformer.layers:
            x = encoder_layer(layer, x, 8)
        if out is not None:
            out.update(agg=agg, x3=x3, transformer=x.permute(1, 0, 2))                      # (B, 108, 256)
        return x.permute(1, 2, 0).reshape(B, -1)

    def gate(self, feats, loftr_rt, inliers, out=None):
        """regression_mlp, model.py:198-233."""
        B = feats.shape[0]
        rt = loftr_rt.to(feats)
        l6 = torch.cat([rt[..., 3], rt[..., :2, :3].reshape(B, 6)], dim=-1)
        n = inliers.to(feats).reshape(B, -1) / 500
        if not self.use_prior:
            n = torch.cat([n, n / 10, n / 100], dim=-1)
        l6 = torch.cat([l6, n], dim=-1)
        reg = self.pose_regressor(feats)
        ratio = torch.linalg.norm(reg[..., :3], dim=-1) / torch.clamp(torch.linalg.norm(l6[..., :3], dim=-1), 1e-2, 1e2)
        l6o = torch.cat([l6[..., :3] * torch.clamp(ratio.unsqueeze(1), 1e-2, 1e2), l6[..., 3:]], dim=-1)
        wt = self.moe_predictor(torch.cat([feats, reg, l6o], dim=-1))
        if out is not None:
            out.update(gate=wt, ratio=ratio)
        t = wt[..., :1] * reg[..., :3] + (1 - wt[..., :1]) * l6o[..., :3]
        R = wt[..., 1:] * reg[..., 3:] + (1 - wt[..., 1:]) * l6o[..., 3:-3]
        return R, t

    def regress(self, vol0, vol1, loftr_rt, inliers, out=None):
        return self.gate(self.features(vol0, vol1, out=out), loftr_rt, inliers, out)

    @torch.no_grad()
    def forward(self, data, out=None):
        """With data['loftr_rt'] / data['inliers'] supplied (every loop then sees the same solver output, as the tool's stubs give)."""
        vol0, vol1 = self.encode(data['image0_reg']), self.encode(data['image1_reg'])
        if out is not None:
            out.update(vol0=vol0, vol1=vol1)
        return self.regress(vol0, vol1, data['loftr_rt'], data['inliers'], out)
