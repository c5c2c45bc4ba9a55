"""Timings of the dense-window convolution (profiles/custom_psf.md), 256 x 256:
  conv: fh_conv_window next to fh_conv_circ on a full 31 x 31 window (961 taps, the largest both run), 24 planes, forward and
        adjoint, and fh_conv_window alone at 41 x 41 (the radius-20 disk), 61 x 61 and 65 x 65.  Each figure is the median of
        REPS device-event windows of CALLS back-to-back launches after a warm-up, the kernels alternating window by window.
  cg:   one batched CG iteration (B images, m factor columns) with the disk PSF (op = 4) next to the shipped motion PSF
        (op = 1, tap list), by the two-cap difference of profiles/tools/channel_ops_time.py.
    python profiles/tools/custom_psf_time.py [--part conv,cg] [--batch 8] [--m 0,32]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "profiles", "tools")]
F64 = torch.float64
S, PLANES = 256, 24
CALLS, REPS = 40, 9


def disk_psf(radius=20.3, size=61):
    yy, xx = np.mgrid[-(size // 2): size - size // 2, -(size // 2): size - size // 2]
    k = (yy ** 2 + xx ** 2 <= radius ** 2).astype(np.float64)
    return k / k.sum()


def window_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def conv_part(dev):
    from free_hunch_amd import _lib
    from free_hunch_amd.measurements import _TapList
    ctx = _lib.Context.get(S, PLANES, 0)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((PLANES, S, S))).to(dev)
    out_w, out_c = torch.empty_like(x), torch.empty_like(x)
    for side in (31, 41, 61, 65):
        h = side // 2
        k = disk_psf(20.3, 41) if side == 41 else rng.standard_normal((side, side))
        win = torch.from_numpy(np.ascontiguousarray(k)).to(dev)
        taps = _TapList(k, dev) if side == 31 else None
        for adjoint in (False, True):
            runs = {"window": lambda: ctx.conv_window(x, out_w, (win, h, h), PLANES, adjoint)}
            if taps is not None:
                runs["tap_list"] = lambda: ctx.conv(x, out_c, taps, PLANES, 1, adjoint)
            for fn in runs.values():  # warm-up: code objects, clocks
                for _ in range(10):
                    fn()
            ts = {name: [] for name in runs}
            for _ in range(REPS):
                for name, fn in runs.items():
                    ts[name].append(window_us(fn))
            if taps is not None:  # the same sums in two orders
                err = float((out_w - out_c).abs().max() / out_c.abs().max())
                assert err < 1e-12, err
            for name, t in ts.items():
                t = sorted(t)
                madds = PLANES * S * S * side * side  # every window entry is multiplied, zeros included
                print(json.dumps(dict(part="conv", kernel=name, window=f"{side}x{side}", adjoint=int(adjoint),
                                      us=round(t[len(t) // 2], 2), us_min=round(t[0], 2), us_max=round(t[-1], 2),
                                      gmadd_per_s=round(madds / t[len(t) // 2] * 1e-3, 1))), flush=True)


def cg_part(dev, batch, ms):
    import channel_ops_time as cot
    from free_hunch_amd.measurements import get_operator

    def operator(name, dev):
        kw = dict(device=dev, sigma_s=0.05, in_shape=(1, 3, S, S))
        if name == "custom_blur":
            return get_operator(name=name, kernel=disk_psf(), **kw)
        return get_operator(name=name, kernel_size=61, intensity=0.5, **kw)

    cot.operator = operator  # Solve builds its fh_problem from this
    with torch.cuda.stream(torch.cuda.Stream()):  # a capturable stream: the iterations replay as graphs, as in the sampler
        for m in ms:
            covs = cot.covariances(batch, m, dev)
            for name in ("custom_blur", "motion_blur"):
                s = cot.Solve(name, covs, dev)
                s.run(cot.LO)
                torch.cuda.synchronize()
                lo, hi = s.timed(cot.LO), s.timed(cot.HI)
                print(json.dumps(dict(part="cg", operator=name, op=int(s.prob.op), ntaps=int(s.prob.ntaps), B=batch, m=m,
                                      ms_lo=round(lo, 4), ms_hi=round(hi, 4),
                                      us_per_iteration=round((hi - lo) / (cot.HI - cot.LO) * 1e3, 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="conv,cg")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--m", default="0,32")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    try:  # the clocks the figures were taken at (read only)
        print(subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout, flush=True)
    except (OSError, subprocess.SubprocessError) as e:
        print(f"clocks not read: {e}", flush=True)
    if "conv" in a.part:
        conv_part(dev)
    if "cg" in a.part:
        cg_part(dev, a.batch, [int(v) for v in a.m.split(",")])


if __name__ == "__main__":
    main()
