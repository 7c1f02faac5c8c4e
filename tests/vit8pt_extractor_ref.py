"""The 8-Point-ViT's extractor restated in plain torch.nn, in any dtype: the ResNet18 front (conv1, bn1, relu, maxpool, layer1, layer2
under torchvision's parameter names) and the kernel-size-5 ResidualBlock behind it, as interiornetStreetlearn_8ptVit/src/model.py
:131-163 runs them.  Two users:

  * tools/make_golden_vit8pt_extractor.py installs `resnet18` below as the stub `torchvision.models.resnet18` (torchvision is absent),
    so that the reference's own ViTEss.__init__, extract_features, ResidualBlock and forward run unmodified and write golden G26;
  * the tests: RefViTEssImages (the float64 / fp32 yardstick of the GPU tests), pinned to the reference's run by
    tests/test_vit8pt_extractor_cpu.py through G26's taps.

BatchNorm always uses its running statistics (the reference runs in eval mode)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import vit8pt_ref as vr

SIZE = 224


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x, taps=None):
        y = self.relu(self.bn1(self.conv1(x)))
        _tap(taps, y)
        y = self.bn2(self.conv2(y))
        if self.downsample is not None:
            x = self.downsample(x)
        y = self.relu(y + x)
        _tap(taps, y)
        return y


class ResNet18Front(nn.Module):
    """What the reference uses of torchvision.models.resnet18(): conv1, bn1, relu, maxpool, layer1, layer2, and an `fc` attribute
    it overwrites with an Identity."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = nn.Sequential(BasicBlock(64, 64), BasicBlock(64, 64))
        self.layer2 = nn.Sequential(BasicBlock(64, 128, 2), BasicBlock(128, 128))
        self.fc = nn.Identity()


def resnet18(*args, **kwargs):
    return ResNet18Front()


class FinalConv(nn.Module):
    """ResidualBlock(128, 192, 'batch', kernel_size=5): conv1 3x3 pad 1, conv2 5x5 unpadded, the 5x5 unpadded shortcut whose norm
    is norm3 itself."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(128, 192, 3, padding=1)
        self.conv2 = nn.Conv2d(192, 192, 5)
        self.norm1 = nn.BatchNorm2d(192)
        self.norm2 = nn.BatchNorm2d(192)
        self.norm3 = nn.BatchNorm2d(192)
        self.downsample = nn.Sequential(nn.Conv2d(128, 192, 5), self.norm3)

    def forward(self, x, taps=None):
        y = torch.relu(self.norm1(self.conv1(x)))
        _tap(taps, y)
        y = torch.relu(self.norm2(self.conv2(y)))
        _tap(taps, y)
        y = torch.relu(self.downsample(x) + y)
        _tap(taps, y)
        return y


def _tap(taps, y):
    """One ReLU output: (share of positive outputs, largest magnitude)."""
    if taps is not None:
        taps.append((float((y > 0).double().mean()), float(y.abs().max())))


def normalised_input(images, dtype):
    """(B, 2, 3, H, W) fp32 0 .. 255 -> (2B, 3, 224, 224) in `dtype`: model.py:135-145.  The nearest-neighbour resize is a gather and
    commutes with the elementwise normalisation: it is taken on the fp32 image (exact on integers, the index arithmetic of the
    reference's fp32 call), the normalisation then runs in `dtype` with the reference's fp32 constants."""
    x = F.interpolate(images.float().flatten(0, 1)[:, [2, 1, 0]], size=SIZE).to(dtype) / 255.0
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32, device=x.device).to(dtype)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32, device=x.device).to(dtype)
    return (x - mean[:, None, None]) / std[:, None, None]


class RefViTEssImages(vr.RefViTEss):
    """tests/vit8pt_ref.py's RefViTEss with the extractor in front: the state dict of far_amd.vit8pt.ViTEss(..., extractor=True)."""

    def __init__(self, args, pose_mean=None, pose_std=None):
        super().__init__(args, pose_mean, pose_std)
        self.resnet = ResNet18Front()
        del self.resnet.fc                                          # (an Identity in the reference: no entries either way)
        self.extractor_final_conv = FinalConv()
        self.eval()

    def as_dtype(self, dtype, device=None):
        return super().as_dtype(dtype, device).eval()

    @torch.no_grad()
    def extract_features(self, images, taps=None):
        """-> (2B, 576, 192) in the parameters' dtype; taps: receives (positive share, max |.|) of every ReLU's output, in order."""
        rn = self.resnet
        x = normalised_input(images.to(rn.conv1.weight.device), rn.conv1.weight.dtype)
        x = torch.relu(rn.bn1(rn.conv1(x)))
        _tap(taps, x)
        x = rn.maxpool(x)
        for layer in (rn.layer1, rn.layer2):
            for blk in layer:
                x = blk(x, taps)
        x = self.extractor_final_conv(x, taps)
        return x.reshape(x.shape[0], 192, 576).permute(0, 2, 1)

    @torch.no_grad()
    def forward_images(self, images, grid_intrinsics=None, loftr_num_corr=None, loftr_preds=None):
        """grid_intrinsics: None or the (fx, fy, cx, cy) tuple ON THE FEATURE GRID."""
        return self.forward_features(self.extract_features(images), grid_intrinsics, loftr_num_corr, loftr_preds)
