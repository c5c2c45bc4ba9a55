"""Split-K launches of the split-bf16 convolution on the row-reuse kernel (k_conv_x6r with a K range): every case is one
fh_conv2d_x6_nhwc call with an explicit split-K factor and its own workspace, held to
  - the last bit (torch.equal) against the same call in a child process started with FH_CONV_SPLITK_REUSE=0 (the generic
    kernel; the switch is read once per process), and
  - rel < 2e-6 against F.conv2d in float64 (the bar of test_conv_split_bf16_splitk);
and one reduced network whose 32^2 and 16^2 levels run split-K: forward and input-VJP equal the child process bit for bit."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inputs
import nets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, REUSE_SPLIT = 0, 2

# name: (N, H, W, Cin, Cout, ksplit, bias + residual, input-gradient weights, kernel family with the switch on)
CASES = {
    "w64_27chunks_unaligned": (1, 64, 64, 96, 128, 8, False, False, REUSE_SPLIT),  # ranges start / end mid-row and mid-chunk
    "w32_two_images_two_ntiles": (2, 32, 32, 64, 256, 8, False, False, REUSE_SPLIT),
    "w16_segw16_unaligned": (4, 16, 16, 160, 512, 8, False, False, REUSE_SPLIT),
    "w128_one_chunk_per_row": (1, 128, 128, 32, 128, 2, False, False, REUSE_SPLIT),
    "w32_masked_ntile_bias_res": (2, 32, 32, 64, 192, 8, True, False, REUSE_SPLIT),
    "w16_input_gradient": (4, 16, 16, 160, 512, 8, False, True, REUSE_SPLIT),
    "w8_ineligible": (3, 8, 8, 512, 96, 4, False, False, GENERIC),
}


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _lib():
    from free_hunch_amd import _lib as L
    return L, L.load()


def family(case):
    _L, lib = _lib()
    N, H, W, Ci, Co, ks = CASES[case][:6]
    buf = (ctypes.c_int32 * 8)()
    assert lib.fh_conv2d_x6_plan(ks, N, H, W, Ci, Co, 3, 3, 1, 1, buf) == 0
    return buf[0]


def _case_inputs(case):
    """(x [N][Ci][H][W], conv weight [Co][Ci][3][3] in F.conv2d's layout, bias, residual) on the CPU, seeded per case"""
    N, H, W, Ci, Co, _ks, full, dgrad, _fam = CASES[case]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(case))
    x = torch.randn(N, Ci, H, W, generator=g)
    if dgrad:  # the input gradient of a [Ci][Co] layer: flipped taps, channels exchanged (HipOps packs wd the same way)
        w4 = torch.randn(Ci, Co, 3, 3, generator=g) / math.sqrt(Ci * 9)
        w = w4.flip(2, 3).transpose(0, 1).contiguous()
    else:
        w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(Ci * 9)
    b = torch.randn(Co, generator=g) if full else None
    res = torch.randn(N, Co, H, W, generator=g) if full else None
    return x, w, b, res


def conv_case(case, dev):
    """the split-K launch of one case -> output [N][H][W][Co]"""
    from free_hunch_amd.unet_hip import _split3
    L, lib = _lib()
    N, H, W, Ci, Co, ks = CASES[case][:6]
    x, w, b, res = _case_inputs(case)
    xn = x.to(dev).permute(0, 2, 3, 1).contiguous()
    wx = _split3(w.to(dev).permute(0, 2, 3, 1).reshape(Co, 9, Ci).contiguous())
    bn = b.to(dev) if b is not None else None
    rn = res.to(dev).permute(0, 2, 3, 1).contiguous() if res is not None else None
    out = torch.full((N, H, W, Co), float("nan"), device=dev)
    ws = torch.full((ks, N * H * W, Co), float("nan"), device=dev)
    L.check(lib.fh_conv2d_x6_nhwc(xn.data_ptr(), wx.data_ptr(), bn.data_ptr() if bn is not None else None,
                                  rn.data_ptr() if rn is not None else None, out.data_ptr(), ws.data_ptr(), ks, N, H, W,
                                  Ci, Co, 3, 3, 1, 1, L.stream()), case)
    torch.cuda.synchronize()
    return out


# ---- network level: 128 channels at 32^2, 256 at 16^2 (with attention), batch 8: both levels' 3 x 3 layers run split-K on
# 128 x 128 tiles (32^2: ksplit 4, grid (64, 1, 4); 16^2: ksplit 8, grid (16, 2, 8))
NET_BATCH = 8


def _net_cfg():
    from oracle.unet_oracle import UNetConfig
    return UNetConfig(image_size=32, num_channels=128, num_res_blocks=1, channel_mult=(1, 2), learn_sigma=True,
                      attention_resolutions="2", num_heads=4, num_head_channels=64, use_scale_shift_norm=True,
                      resblock_updown=True, use_new_attention_order=False)


def net_layers_rerouted():
    """the (H, W, Cin, Cout) of the network's 3 x 3 layers (forward and input-gradient) that the plan reroutes at NET_BATCH"""
    import make_conv_plan
    from free_hunch_amd import unet as hu
    _L, lib = _lib()
    buf = (ctypes.c_int32 * 8)()
    out = []
    for H, W, Ci, Co, k, stride in make_conv_plan.unet_layers(nets._hip_cfg(_net_cfg()), hu._plan):
        ks = lib.fh_conv2d_splitk(NET_BATCH, H, W, Ci, Co, k, k)
        assert lib.fh_conv2d_x6_plan(ks, NET_BATCH, H, W, Ci, Co, k, k, k // 2, stride, buf) == 0
        if buf[0] == REUSE_SPLIT:
            out.append((H, W, Ci, Co))
    return out


def net_case(dev):
    net = nets.damped_hip_net(_net_cfg(), 17, dev)
    x = (inputs.randn((NET_BATCH, 3, 32, 32), 31) * 0.7).to(dev).requires_grad_()
    sigma = torch.tensor(1.5, dtype=torch.float64, device=dev)
    cot = inputs.randn((NET_BATCH, 3, 32, 32), 32).to(dev)
    D, _ = net(x, sigma)
    (gx,) = torch.autograd.grad((D * cot).sum(), x)
    torch.cuda.synchronize()
    return D.detach(), gx


_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}, {gold!r}]
import test_splitk_reuse_gpu as t
assert all(t.family(c) == t.GENERIC for c in t.CASES) and not t.net_layers_rerouted()  # FH_CONV_SPLITK_REUSE=0
dev = torch.device("cuda:0")
res = {{c: t.conv_case(c, dev).cpu().numpy() for c in t.CASES}}
res["net_D"], res["net_gx"] = (v.cpu().numpy() for v in t.net_case(dev))
np.savez(sys.argv[1], **res)
"""


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def generic(dev, tmp_path_factory):
    """every case and the network from a child process with the switch off"""
    assert os.environ.get("FH_CONV_SPLITK_REUSE") is None, "the switch is read once per process: run the tests without it"
    path = str(tmp_path_factory.mktemp("splitk") / "generic.npz")
    src = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), gold=os.path.join(ROOT, "tests", "golden"))
    subprocess.run([sys.executable, "-c", src, path], check=True, env=dict(os.environ, FH_CONV_SPLITK_REUSE="0"), timeout=300)
    return np.load(path)


@pytest.mark.parametrize("case", list(CASES))
def test_split_conv_equals_generic_bitwise_and_float64(dev, generic, case):
    assert family(case) == CASES[case][8], (case, family(case))
    out = conv_case(case, dev)
    x, w, b, res = _case_inputs(case)
    ref = F.conv2d(x.double(), w.double(), b.double() if b is not None else None, padding=1)
    if res is not None:
        ref = ref + res.double()
    want = torch.from_numpy(generic[case])
    r = rel(out.cpu().permute(0, 3, 1, 2), ref)
    print(case, "rel to float64 %.3e" % r, "differing elements", int((out.cpu() != want).sum()), flush=True)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out.cpu(), want), case
    assert r < 2e-6, (case, r)


def test_network_forward_and_vjp_equal_generic_bitwise(dev, generic):
    layers = net_layers_rerouted()
    print("rerouted layers (H, W, Cin, Cout):", layers, flush=True)
    assert {h for h, _w, _ci, _co in layers} == {32, 16}, layers  # both small levels run the new kernel
    D, gx = net_case(dev)
    assert bool(torch.isfinite(D).all()) and bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    assert torch.equal(D.cpu(), torch.from_numpy(generic["net_D"]))
    assert torch.equal(gx.cpu(), torch.from_numpy(generic["net_gx"]))
