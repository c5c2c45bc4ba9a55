"""LPIPS v0.1 with the VGG16 backbone on the device (reference: generate_conditional.py:499-583, `lpips.LPIPS(net='vgg')` on
`(x / 255 - 0.5) * 2`; Zhang et al., "The Unreasonable Effectiveness of Deep Features as a Perceptual Metric", 2018).

The thirteen 3 x 3 convolutions are the UNet's own entry points (`fh_conv2d_x6_nhwc`, the exact 3-way bf16 split, where
`unet_hip._use_x6` chooses it; `fh_conv2d_nhwc` for the 64-channel outputs), always in precision mode 0 (with
`FH_CONV_MODE=f32|wino` no split planes exist and every layer runs `fh_conv2d_nhwc` on the fp32 matrix cores: the accuracy
figures and tests are those of the default mode); the scaling layer,
ReLU, max-pool and the per-tap reduction are the kernels of csrc/fh_lpips.hip.  Both images of a pair go through the network
in ONE batch of 2N.  Only the weights need files: torchvision's `vgg16-397923af.pth` and the lpips package's
`weights/v0.1/vgg.pth`, taken by path (`load_weights`); `seeded_weights` gives the same structure with random values.

The `lpips` package and torchvision are absent from this image and the published weights cannot be fetched, so the metric
is pinned to a PyTorch restatement of the published forward pass (tests/test_lpips_gpu.py), not to the package itself:
parity unpinned at that boundary.  There is no CPU fallback."""
from __future__ import annotations

import os

import torch

from . import _lib
from . import unet_hip

# VGG16 `features`: index of every convolution, the convolutions whose ReLU output is a tap (relu1_2 ... relu5_3) and the
# convolutions that a 2 x 2 max-pool precedes
VGG_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
VGG_TAPS = (2, 7, 14, 21, 28)
VGG_POOLS = (5, 10, 17, 24)
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-0.030, -0.088, -0.188)  # the scaling layer of LPIPS v0.1
SCALE = (0.458, 0.448, 0.450)
MAX_PAIRS = 8  # pairs per pass: bounds the workspace (16 x H x W x 64 floats for the first block)


def _conv_shapes():
    cin = 3
    for k, co in zip(VGG_CONVS, VGG_CHANNELS):
        yield k, co, cin
        cin = co


def _lin_key(t):
    return f"lin{t}.model.1.weight"


def _check(state, key, shape, where):
    if key not in state:
        raise ValueError(f"{where}: key '{key}' is missing")
    v = state[key]
    if not torch.is_tensor(v) or tuple(v.shape) != tuple(shape):
        got = tuple(v.shape) if torch.is_tensor(v) else type(v).__name__
        raise ValueError(f"{where}: key '{key}' has shape {got}, expected {tuple(shape)}")
    return v.detach().to(torch.float32).contiguous()


def load_weights(vgg_path, lin_path):
    """The two published files -> one flat state: `features.K.weight|bias` of torchvision's VGG16 (`classifier.*` ignored)
    and `linT.model.1.weight` [1, C, 1, 1] of the LPIPS linear layers (`lins.T.model.1.weight` is accepted as well).  A missing
    key or a wrong shape is a ValueError that names it."""
    for p in (vgg_path, lin_path):
        if not os.path.isfile(p):
            raise FileNotFoundError(f"LPIPS weight file '{p}' does not exist")
    vgg = torch.load(vgg_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True)
    if not isinstance(vgg, dict) or not isinstance(lin, dict):
        raise ValueError("LPIPS weight files must hold state dicts")
    state = {}
    for k, co, ci in _conv_shapes():
        state[f"features.{k}.weight"] = _check(vgg, f"features.{k}.weight", (co, ci, 3, 3), vgg_path)
        state[f"features.{k}.bias"] = _check(vgg, f"features.{k}.bias", (co,), vgg_path)
    for t, c in enumerate(TAP_CHANNELS):
        alt = f"lins.{t}.model.1.weight"
        key = alt if (_lin_key(t) not in lin and alt in lin) else _lin_key(t)
        state[_lin_key(t)] = _check(lin, key, (1, c, 1, 1), lin_path)
    return state


def seeded_weights(seed):
    """The structure of `load_weights` with seeded random values: He-scaled convolution weights, biases 0.05 x normal, linear
    weights uniform in [0, 2 / C) - for tests and for machines without the published files."""
    g = torch.Generator().manual_seed(int(seed))
    state = {}
    for k, co, ci in _conv_shapes():
        state[f"features.{k}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (ci * 9)) ** 0.5
        state[f"features.{k}.bias"] = 0.05 * torch.randn(co, generator=g)
    for t, c in enumerate(TAP_CHANNELS):
        state[_lin_key(t)] = torch.rand(1, c, 1, 1, generator=g) * (2.0 / c)
    return state


def save_weights(state, vgg_path, lin_path):
    """Write a state in the two published key layouts."""
    torch.save({k: v.clone() for k, v in state.items() if k.startswith("features.")}, vgg_path)
    torch.save({k: v.clone() for k, v in state.items() if k.startswith("lin")}, lin_path)


def prep_table():
    """[3, 256] float32: ((v / 255 - 0.5) * 2 - shift_c) / scale_c evaluated in float64 and rounded once."""
    v = torch.arange(256, dtype=torch.float64)
    x = (v / 255.0 - 0.5) * 2.0
    rows = [(x - torch.tensor(s, dtype=torch.float64)) / torch.tensor(d, dtype=torch.float64) for s, d in zip(SHIFT, SCALE)]
    return torch.stack(rows).to(torch.float32).contiguous()


def pack_conv(w, b):
    """`unet_hip._Conv` of one VGG convolution, forward copies only (the metric has no backward pass)."""
    return unet_hip._Conv(w, b, forward_only=True)


class LPIPS:
    """`LPIPS(state, device)(a_u8, b_u8)` -> float64 [N]: the distance of every uint8 image pair [N, 3, H, W] on the device."""

    def __init__(self, state, device):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.FhError("LPIPS runs on the device (libfh_hip.so); there is no CPU fallback")
        self.convs = []
        for k, co, ci in _conv_shapes():
            w = _check(state, f"features.{k}.weight", (co, ci, 3, 3), "LPIPS state")
            b = _check(state, f"features.{k}.bias", (co,), "LPIPS state")
            self.convs.append((k, pack_conv(w.to(self.device), b.to(self.device))))
        self.lins = [_check(state, _lin_key(t), (1, c, 1, 1), "LPIPS state").reshape(c).to(self.device).contiguous()
                     for t, c in enumerate(TAP_CHANNELS)]
        self.table = prep_table().to(self.device)

    # ---------------------------------------------------------------- kernel wrappers
    def _prep(self, a, b):
        n, _, H, W = a.shape
        x = torch.empty(2 * n, H, W, 32, dtype=torch.float32, device=a.device)
        _lib.check(self.lib.fh_lpips_prep_u8(a.data_ptr(), b.data_ptr(), self.table.data_ptr(), x.data_ptr(), n, H, W,
                                             _lib.stream()), "fh_lpips_prep_u8")
        return x

    def _conv(self, c, x):
        assert x.shape[-1] == c.ci_p, (x.shape, c.ci_p)
        return unet_hip.conv_launch(self.lib, c, True, x, None, c.b)[0]

    def _relu(self, x):
        _lib.check(self.lib.fh_relu_f32(x.data_ptr(), x.numel(), _lib.stream()), "fh_relu_f32")
        return x

    def _relu_pool(self, x):
        N, H, W, C = x.shape
        out = torch.empty(N, H // 2, W // 2, C, dtype=torch.float32, device=x.device)
        _lib.check(self.lib.fh_relu_maxpool2_nhwc(x.data_ptr(), out.data_ptr(), N, H, W, C, _lib.stream()),
                   "fh_relu_maxpool2_nhwc")
        return out

    def tap(self, feat, lin, out=None):
        """One tap on a raw convolution output [2N, H, W, C] (ReLU applied on read) -> float64 [N] (or into `out`, any
        stride)."""
        if not (feat.is_cuda and lin.is_cuda):
            raise _lib.FhError("LPIPS runs on the device (libfh_hip.so); there is no CPU fallback")
        if not (feat.dim() == 4 and feat.shape[0] % 2 == 0 and feat.dtype == torch.float32 and feat.is_contiguous()
                and lin.dtype == torch.float32 and lin.is_contiguous() and lin.numel() == feat.shape[-1]):
            raise ValueError(f"LPIPS tap takes contiguous float32 features [2N, H, W, C] and C float32 weights, got "
                             f"{feat.dtype} {tuple(feat.shape)} and {lin.dtype} {tuple(lin.shape)}")
        N2, H, W, C = feat.shape
        n = N2 // 2
        out = torch.empty(n, dtype=torch.float64, device=feat.device) if out is None else out
        scratch = torch.empty(int(self.lib.fh_lpips_tap_scratch_doubles(n)), dtype=torch.float64, device=feat.device)
        _lib.check(self.lib.fh_lpips_tap(feat.data_ptr(), lin.data_ptr(), n, H, W, C, scratch.data_ptr(), out.data_ptr(),
                                         out.stride(0), _lib.stream()), "fh_lpips_tap")
        return out

    # ---------------------------------------------------------------- the metric
    def _pass(self, a, b, layers):
        x = self._prep(a, b)
        t = 0
        for j, (k, c) in enumerate(self.convs):
            y = self._conv(c, x)
            if k in VGG_TAPS:
                self.tap(y, self.lins[t], out=layers[:, t])
                t += 1
            if j + 1 == len(self.convs):
                break
            x = self._relu_pool(y) if self.convs[j + 1][0] in VGG_POOLS else self._relu(y)

    def __call__(self, a_u8, b_u8, per_layer=False):
        if not (torch.is_tensor(a_u8) and torch.is_tensor(b_u8) and a_u8.is_cuda and b_u8.is_cuda):
            raise _lib.FhError("LPIPS runs on the device (libfh_hip.so); there is no CPU fallback")
        if not (a_u8.dtype == torch.uint8 and b_u8.dtype == torch.uint8 and a_u8.shape == b_u8.shape and a_u8.dim() == 4
                and a_u8.shape[0] >= 1 and a_u8.shape[1] == 3 and a_u8.shape[2] >= 16 and a_u8.shape[3] >= 16):
            raise ValueError(f"LPIPS takes two uint8 image batches [N, 3, H, W] of one shape with H, W >= 16, got "
                             f"{a_u8.dtype} {tuple(a_u8.shape)} and {b_u8.dtype} {tuple(b_u8.shape)}")
        N, C, H, W = a_u8.shape
        a, b = a_u8.contiguous(), b_u8.contiguous()
        layers = torch.empty(N, len(VGG_TAPS), dtype=torch.float64, device=a.device)
        # the convolution precision switch is per host thread: the metric always runs the exact split (mode 0) and puts
        # back what the sampler left
        mode = self.lib.fh_unet_get_precision()
        _lib.check(self.lib.fh_unet_set_precision(0), "fh_unet_set_precision")
        try:
            for s in range(0, N, MAX_PAIRS):
                self._pass(a[s: s + MAX_PAIRS], b[s: s + MAX_PAIRS], layers[s: s + MAX_PAIRS])
        finally:
            _lib.check(self.lib.fh_unet_set_precision(mode), "fh_unet_set_precision")
        if per_layer:
            return layers
        total = layers[:, 0].clone()
        for t in range(1, len(VGG_TAPS)):  # the plain sum of the five tap values, in tap order
            total += layers[:, t]
        return total
