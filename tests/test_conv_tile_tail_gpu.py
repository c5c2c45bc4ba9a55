"""The tile-tail form of the exact-split 256-pixel convolution tiles (k_conv_x6r with TT: the epilogue moves 16 bytes per
lane after a 4 x 4 transpose in every lane quad) against the kernel with the 4-byte epilogue, which a child process started
with FH_CONV_TILE_TAIL=0 runs (the switch is read once per process): outputs AND group-sum partial buffers equal bit for bit
(compared as SHA-256 of the buffers' bytes), for the smallest shapes that still plan a 256-pixel tile - more tiles than CUs,
a tile count that is no multiple of 8, an odd chunk count, a ragged last column tile, a Cout the 16-byte form does not take -
in every epilogue mode; and one reduced network, forward and input-VJP."""
import ctypes
import hashlib
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import inputs
import nets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (N, H, W, Cin, Cout), tiles of the planned grid
SHAPES = {
    "w64_288_tiles": ((9, 64, 64, 32, 256), 288),              # 256 + 32: a second, partial wave of workgroups
    "w64_273_tiles_27_chunks": ((13, 28, 64, 96, 384), 273),   # not a multiple of 8 (no XCD remap); 27 chunks
    "w128_320_tiles": ((5, 128, 128, 64, 128), 320),
    "w256_512_tiles_ragged_ntile": ((1, 256, 256, 32, 192), 512),  # the second column tile has 64 masked columns
    "w256_cout_130_scalar_epilogue": ((1, 256, 256, 32, 130), 512),  # Cout % 4 != 0: the 4-byte epilogue (no group sums)
}
MODES = ("plain", "bias_res", "gn0", "gn1", "norm_gn_act0", "norm_gn_act1")


def modes_of(shape):
    return MODES if SHAPES[shape][0][4] % 32 == 0 else MODES[:2]


def _lib():
    from free_hunch_amd import _lib as L
    return L, L.load()


def planned(shape):
    _L, lib = _lib()
    N, H, W, Ci, Co = SHAPES[shape][0]
    buf = (ctypes.c_int32 * 8)()
    assert lib.fh_conv2d_x6_plan(1, N, H, W, Ci, Co, 3, 3, 1, 1, buf) == 0
    return list(buf)


def _decades(shape, g, lo=-3.0, hi=2.0):
    """normal values with magnitudes spread over several decades"""
    return torch.randn(shape, generator=g) * 10.0 ** (lo + (hi - lo) * torch.rand(shape, generator=g))


def conv_case(shape, mode, dev):
    """one launch -> (output, group-sum partials or None)"""
    from free_hunch_amd.unet_hip import _split3
    L, lib = _lib()
    N, H, W, Ci, Co = SHAPES[shape][0]
    g = torch.Generator().manual_seed(7000 + 10 * sorted(SHAPES).index(shape) + MODES.index(mode))
    x = _decades((N, H, W, Ci), g).to(dev)
    wx = _split3((_decades((Co, 9, Ci), g, -2.0, 0.0) / math.sqrt(Ci * 9)).to(dev).contiguous())
    b = _decades((Co,), g, -2.0, 1.0).to(dev) if mode != "plain" else None
    res = _decades((N, H, W, Co), g).to(dev) if mode != "plain" else None
    bp, rp = (b.data_ptr() if b is not None else None), (res.data_ptr() if res is not None else None)
    out = torch.full((N, H, W, Co), float("nan"), device=dev)
    partial = None
    if mode in ("plain", "bias_res"):
        L.check(lib.fh_conv2d_x6_nhwc(x.data_ptr(), wx.data_ptr(), bp, rp, out.data_ptr(), None, 1, N, H, W, Ci, Co, 3, 3, 1, 1,
                                      L.stream()), shape)
    else:
        chunks = lib.fh_conv2d_x6_gn_chunks(1, N, H, W, Ci, Co, 3, 3, 1, 1)
        assert chunks == (H * W // 256) * -(-Co // 128)
        partial = torch.full((N * chunks * 64,), float("nan"), dtype=torch.float64, device=dev)
        e = L.FhGnEpilogue()
        e.partial, e.mode, e.act = partial.data_ptr(), int(mode == "gn1"), 1
        if mode == "gn1":
            xin = _decades((N, H, W, Co), g, -2.0, 1.0).to(dev)
            tab = torch.randn(N, 5, Co, generator=g).to(dev)  # A, Bc, mean, rstd, gamma (1 + scale): any finite numbers
            e.x, e.tab = xin.data_ptr(), tab.data_ptr()
        if mode.startswith("norm"):
            assert lib.fh_conv2d_x6_norm_supported(N, H, W, Ci, Co) == 1
            table = torch.cat([1 + 0.1 * torch.randn(N, 1, Ci, generator=g), 0.1 * torch.randn(N, 1, Ci, generator=g)], 1).to(dev)
            L.check(lib.fh_conv2d_x6_norm_nhwc_gn(x.data_ptr(), table.contiguous().data_ptr(), int(mode.endswith("1")), wx.data_ptr(),
                                                  bp, rp, out.data_ptr(), N, H, W, Ci, Co, ctypes.byref(e), L.stream()), shape)
        else:
            L.check(lib.fh_conv2d_x6_nhwc_gn(x.data_ptr(), wx.data_ptr(), bp, rp, out.data_ptr(), None, 1, N, H, W, Ci, Co, 3, 3,
                                             1, 1, ctypes.byref(e), L.stream()), shape)
    torch.cuda.synchronize()
    return out, partial


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def case_digests(shape, mode, dev):
    out, partial = conv_case(shape, mode, dev)
    assert bool(torch.isfinite(out).all()) and (partial is None or bool(torch.isfinite(partial).all())), (shape, mode)
    return [digest(out), digest(partial) if partial is not None else None]


# ---- network level: 128 channels at 64^2, batch 16: the 3 x 3 layers of the first level plan 256 tiles of 256 pixels
NET_BATCH = 16


def _net_cfg():
    from oracle.unet_oracle import UNetConfig
    return UNetConfig(image_size=64, num_channels=128, num_res_blocks=1, channel_mult=(1, 2), learn_sigma=True,
                      attention_resolutions="8", num_heads=4, num_head_channels=64, use_scale_shift_norm=True,
                      resblock_updown=True, use_new_attention_order=False)


def net_layers_256():
    """the (H, W, Cin, Cout) of the network's 3 x 3 layers (forward and input-gradient) that plan 256-pixel tiles"""
    import make_conv_plan
    from free_hunch_amd import unet as hu
    _L, lib = _lib()
    buf, out = (ctypes.c_int32 * 8)(), []
    for H, W, Ci, Co, k, stride in make_conv_plan.unet_layers(nets._hip_cfg(_net_cfg()), hu._plan):
        ks = lib.fh_conv2d_splitk(NET_BATCH, H, W, Ci, Co, k, k)
        assert lib.fh_conv2d_x6_plan(ks, NET_BATCH, H, W, Ci, Co, k, k, k // 2, stride, buf) == 0
        if buf[1] == 256:
            out.append((H, W, Ci, Co))
    return out


def net_case(dev):
    net = nets.damped_hip_net(_net_cfg(), 19, dev)
    x = (inputs.randn((NET_BATCH, 3, 64, 64), 41) * 0.7).to(dev).requires_grad_()
    sigma = torch.tensor(1.5, dtype=torch.float64, device=dev)
    cot = inputs.randn((NET_BATCH, 3, 64, 64), 42).to(dev)
    D, _ = net(x, sigma)
    (gx,) = torch.autograd.grad((D * cot).sum(), x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(D).all()) and bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    return [digest(D), digest(gx)]


_CHILD = r"""
import sys, json, torch
sys.path[:0] = [{root!r}, {tests!r}, {gold!r}]
import test_conv_tile_tail_gpu as t
dev = torch.device("cuda:0")
res = {{s + "/" + m: t.case_digests(s, m, dev) for s in t.SHAPES for m in t.modes_of(s)}}
res["net"] = t.net_case(dev)
json.dump(res, open(sys.argv[1], "w"))
"""


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def flat(dev, tmp_path_factory):
    """every case and the network from a child process with the switch off"""
    assert os.environ.get("FH_CONV_TILE_TAIL") is None, "the switch is read once per process: run the tests without it"
    path = str(tmp_path_factory.mktemp("tile_tail") / "flat.json")
    src = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), gold=os.path.join(ROOT, "tests", "golden"))
    subprocess.run([sys.executable, "-c", src, path], check=True, env=dict(os.environ, FH_CONV_TILE_TAIL="0"), timeout=300)
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile_tail_equals_flat_launch_bitwise(dev, flat, shape):
    plan = planned(shape)
    assert plan[0] == 1 and plan[1] == 256 and plan[4] == 1 and plan[5] * plan[6] == SHAPES[shape][1], plan
    for mode in modes_of(shape):
        got = case_digests(shape, mode, dev)
        print(shape, mode, "output", got[0] == flat[shape + "/" + mode][0], "partials", got[1] == flat[shape + "/" + mode][1],
              flush=True)
        assert got == flat[shape + "/" + mode], (shape, mode)


def test_network_forward_and_vjp_equal_flat_launch_bitwise(dev, flat):
    layers = net_layers_256()
    print("layers on 256-pixel tiles (H, W, Cin, Cout):", layers, flush=True)
    assert layers and {h for h, _w, _ci, _co in layers} == {64}, layers
    assert net_case(dev) == flat["net"]
