"""PyTorch restatement of the published LPIPS v0.1 forward pass with the VGG16 backbone (lpips.LPIPS(net='vgg',
spatial=False) in eval mode, called with normalize=False on (x / 255 - 0.5) * 2, as the reference does): scaling layer,
torchvision's VGG16 `features` up to relu5_3, unit-normalisation over channels with the guard 1e-10 added outside the square
root, squared difference, the bias-free 1 x 1 `lin` layers, spatial mean, sum over the five taps.  Written from the published
description, in any floating dtype.  Neither the lpips package nor torchvision is installed here and the published weights cannot
be fetched: parity with the package itself is unpinned at that boundary (as skimage's is for SSIM in tests/test_metrics.py).
Not a test module: shared by tests/test_lpips_host.py and tests/test_lpips_gpu.py."""
import numpy as np
import torch
import torch.nn.functional as F

CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
TAPS = (2, 7, 14, 21, 28)          # the tap is the ReLU of these convolutions
POOLS = (5, 10, 17, 24)            # a 2 x 2 max-pool precedes these convolutions
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
NOISE_STD = (2.0, 8.0, 32.0)       # grey levels


def features(state, u8, dtype):
    x = (u8.to(dtype) / 255.0 - 0.5) * 2.0
    x = (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    taps = []
    for k in CONVS:
        if k in POOLS:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, state[f"features.{k}.weight"].to(dtype), state[f"features.{k}.bias"].to(dtype), padding=1))
        if k in TAPS:
            taps.append(x)
    return taps


def lpips_layers(state, a_u8, b_u8, dtype=torch.float64):
    """[N, 5] per-tap values; the metric is their sum over dim 1"""
    out = []
    for t, (fa, fb) in enumerate(zip(features(state, a_u8, dtype), features(state, b_u8, dtype))):
        na = fa / (torch.sqrt(torch.sum(fa ** 2, dim=1, keepdim=True)) + 1e-10)
        nb = fb / (torch.sqrt(torch.sum(fb ** 2, dim=1, keepdim=True)) + 1e-10)
        w = state[f"lin{t}.model.1.weight"].to(dtype)
        out.append(F.conv2d((na - nb) ** 2, w).mean(dim=(2, 3)).reshape(-1))
    return torch.stack(out, dim=1)


def tap_value(feat, lin, dtype=torch.float64):
    """one tap on a raw convolution output [2N, H, W, C] (NHWC, ReLU still to be applied) -> [N]"""
    f = F.relu(feat.to(dtype))
    n = f.shape[0] // 2
    fa, fb = f[:n], f[n:]
    na = fa / (torch.sqrt(torch.sum(fa ** 2, dim=3, keepdim=True)) + 1e-10)
    nb = fb / (torch.sqrt(torch.sum(fb ** 2, dim=3, keepdim=True)) + 1e-10)
    return (((na - nb) ** 2) * lin.to(dtype)).sum(dim=3).mean(dim=(1, 2))


def noisy(imgs, std, seed=3):
    """uint8 images + seeded Gaussian noise of `std` grey levels, rounded and clipped back to uint8"""
    g = np.random.default_rng(seed)
    x = imgs.numpy().astype(np.float64) + std * g.standard_normal(tuple(imgs.shape))
    return torch.from_numpy(np.rint(x).clip(0, 255).astype(np.uint8))
