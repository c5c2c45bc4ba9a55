"""Writes tests/golden/conv_plan.json: what the built library answers, per layer, to the three host-side questions the
split-bf16 convolution launch is planned from - fh_conv2d_splitk, fh_conv2d_x6_gn_chunks (at that split-K factor and at
ksplit = 1) and fh_conv2d_x6_norm_supported.  No device is needed.  The committed table was written by the library as it
stood before the launch code was folded into one plan function; tests/test_conv_plan.py holds every later build to it.

    python tests/golden/make_conv_plan.py [--root CHECKOUT] [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = (1, 2, 3, 4, 8, 9, 16)
# (N, H, W, Cin, Cout, k, stride) of the convolution cases tests/test_hip_unet.py parametrises
TEST_SHAPES = [
    (1, 64, 64, 128, 128, 3, 1), (1, 16, 16, 256, 96, 3, 1), (2, 8, 8, 64, 256, 3, 1), (1, 32, 32, 160, 64, 1, 1),
    (1, 256, 256, 32, 128, 3, 1), (1, 9, 13, 32, 6, 3, 1), (2, 16, 32, 64, 96, 3, 1), (1, 9, 14, 32, 6, 3, 1),
    (3, 8, 8, 160, 64, 3, 1), (2, 32, 32, 256, 320, 1, 1), (1, 33, 31, 64, 130, 3, 2), (8, 64, 64, 128, 256, 3, 1),
    (2, 128, 128, 64, 160, 3, 1), (4, 128, 256, 96, 128, 3, 1), (16, 32, 32, 64, 384, 3, 1), (9, 64, 64, 32, 256, 3, 1),
    (1, 256, 256, 64, 128, 3, 1), (8, 64, 64, 96, 256, 3, 1), (2, 128, 128, 64, 128, 3, 1), (8, 64, 64, 128, 128, 3, 1),
    (2, 128, 128, 64, 384, 3, 1), (8, 32, 32, 256, 256, 3, 1), (8, 64, 64, 128, 256, 1, 1), (2, 64, 64, 96, 160, 3, 1),
]


def _pad32(n):
    return (n + 31) // 32 * 32


def unet_layers(cfg, plan):
    """(H, W, Cin, Cout, k, stride) of every convolution of the step list, forward and input-gradient (the input-gradient
    of a [Cout][Cin] layer is a stride-1 convolution from Cout, padded to 32, to Cin)"""
    out = set()

    def conv(h, ci, co, k):
        out.add((h, h, _pad32(ci), co, k, 1))
        out.add((h, h, _pad32(co), ci, k, 1))

    steps, ch0 = plan(cfg)
    h = cfg.image_size
    for op, _p, ci, co, _heads in steps:
        if op == "conv_in":
            conv(h, ci, co, 3)
        elif op in ("res", "res_down", "res_up"):
            h = h // 2 if op == "res_down" else (h * 2 if op == "res_up" else h)
            conv(h, ci, co, 3)
            conv(h, co, co, 3)
            if ci != co:
                conv(h, ci, co, 1)
        elif op == "attn":
            conv(h, ci, 3 * ci, 1)
            conv(h, ci, ci, 1)
    conv(h, ch0, cfg.out_channels, 3)
    return sorted(out)


def vgg_layers(lpips, size=256):
    out, h = [], size
    for k, co, ci in lpips._conv_shapes():
        if k in lpips.VGG_POOLS:
            h //= 2
        out.append((h, h, _pad32(ci), co, 3, 1))
    return out


def rows(lib, unet, lpips):
    keys = []
    for cfg in (unet.FFHQ256, unet.IMAGENET256):
        keys += [(n,) + s for s in unet_layers(cfg, unet._plan) for n in BATCHES]
    keys += [(n,) + s[1:] for s in TEST_SHAPES for n in sorted(set(BATCHES) | {s[0]})]
    keys += [(n,) + s for s in vgg_layers(lpips) for n in (2, 16)]
    table = []
    for N, H, W, Ci, Co, k, stride in sorted(set(keys)):
        pad = k // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        ks = lib.fh_conv2d_splitk(N, Ho, Wo, Ci, Co, k, k)
        table.append([N, H, W, Ci, Co, k, stride, ks,
                      lib.fh_conv2d_x6_gn_chunks(ks, N, H, W, Ci, Co, k, k, pad, stride),
                      lib.fh_conv2d_x6_gn_chunks(1, N, H, W, Ci, Co, k, k, pad, stride),
                      lib.fh_conv2d_x6_norm_supported(N, H, W, Ci, Co)])
    return table


COLUMNS = ["N", "H", "W", "Cin", "Cout", "k", "stride", "ksplit", "gn_chunks", "gn_chunks_ksplit1", "norm_supported"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)))
    ap.add_argument("--out", default=os.path.join(HERE, "conv_plan.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from free_hunch_amd import _lib, lpips, unet
    table = rows(_lib.load(), unet, lpips)
    with open(a.out, "w") as f:
        f.write('{"columns": %s,\n "rows": [\n' % json.dumps(COLUMNS))
        f.write(",\n".join("  " + json.dumps(r) for r in table))
        f.write("\n ]}\n")
    print(f"{len(table)} rows -> {a.out}")


if __name__ == "__main__":
    main()
