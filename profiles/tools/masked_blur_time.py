"""Time per batched CG iteration of `masked_blur` next to its `custom_blur` twin (profiles/masked_blur.md): 256 x 256, B images,
m factor columns, the shipped Gaussian (folded symmetric DCT route), the shipped motion PSF (k_conv_tile8) and the radius-20
disk (k_conv_window).  The masks are the PSF's own border (mask_border = -1) times 5 % random zeros, one mask per image.
Both operators live in one process and are timed alternately after a warm-up: per repetition one device-event window around
SOLVES solves capped at LO iterations and one around SOLVES solves capped at HI (rtol far below reach), the difference divided by
the SOLVES * (HI - LO) = 224 iterations between them - the solves' fixed part (masking b, first apply, initialisation, final
copy) drops out.  (One long solve would not do at m = 32: these systems reach the pAp <= 1e-16 stop after 60 .. 200 iterations.)
    python profiles/tools/masked_blur_time.py [--batch 8] [--m 0,32] [--psf gaussian,motion,disk] [--reps 7]
    python profiles/tools/masked_blur_time.py --once --m 0
        (--once: warm-up + ONE 16-iteration solve of every operator, for a rocprofv3 --kernel-trace --stats run)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "profiles", "tools")]
F64 = torch.float64
S = 256
LO, HI, SOLVES = 16, 48, 7


def psf(kind):
    from custom_psf_time import disk_psf
    from free_hunch_amd.measurements import KERNEL_DIR
    if kind == "disk":
        return disk_psf()
    return np.load(os.path.join(KERNEL_DIR, {"gaussian": "gaussian_ks61_std3.0.npy", "motion": "motion_ks61_std0.5.npy"}[kind]))


class Solve:
    """fh_cg_solve_batched of one operator over the covariances `covs` (channel_ops_time.Solve with per-image masks)."""

    def __init__(self, name, kind, covs, dev):
        import inputs
        from free_hunch_amd import _lib
        from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
        from free_hunch_amd.measurements import get_operator
        B = len(covs)
        self.lib, self.B = _lib, B
        self.ctx = _lib.Context.get(S, 3 * B, 0, slot=6100 + B)
        self.ctx.set_exclusive(True)
        kw = dict(device=dev, sigma_s=0.05, in_shape=(1, 3, S, S), kernel=psf(kind))
        if name == "masked_blur":
            self.ops = [get_operator(name=name, mask_border=-1,
                                     mask=(np.random.default_rng(900 + b).random((3, S, S)) >= 0.05).astype(np.float64), **kw)
                        for b in range(B)]
        else:
            self.ops = [get_operator(name=name, **kw)]
        self.prob, self.keep = _problem(self.ops[0], covs[0], _sigma_y2(self.ops[0]))
        self.per = _lib.FhBatch()
        self.per.nimg = B
        for b, cov in enumerate(covs):
            self.per.D[b], self.per.r[b], self.per.B[b], self.per.M[b] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(),
                                                                         cov.famC.B.data_ptr(), cov.C.M_dev.data_ptr())
            if name == "masked_blur":
                mk = self.ops[b].mask.to(device=dev, dtype=F64).contiguous()
                self.keep.append(mk)
                self.per.mask[b] = mk.data_ptr()
        self.kept = float(torch.stack([o.mask for o in self.ops]).mean()) if name == "masked_blur" else 1.0
        self.b = inputs.randn((B, 3, S, S), 77).to(dev).contiguous()
        self.x = torch.empty_like(self.b)
        self.rtols = (C.c_double * B)(*([1e-300] * B))
        self.infos = (_lib.FhCgInfo * B)()
        self.short = False

    def run(self, iters):
        self.lib.check(self.ctx.lib.fh_cg_solve_batched(self.ctx.h, C.byref(self.prob), C.byref(self.per), self.b.data_ptr(),
                                                        self.x.data_ptr(), self.rtols, 0.0, iters, self.infos,
                                                        self.lib.stream()), "fh_cg_solve_batched")
        return [self.infos[b].niter for b in range(self.B)]

    def window_ms(self, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        ns = [self.run(iters) for _ in range(SOLVES)]
        e1.record()
        torch.cuda.synchronize()
        self.short = self.short or ns != [[iters] * self.B] * SOLVES  # an image stopped below the cap: not a per-iteration figure
        return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--m", default="0,32")
    ap.add_argument("--psf", default="gaussian,motion,disk")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import channel_ops_time as cot
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = ("masked_blur", "custom_blur")
    with torch.cuda.stream(torch.cuda.Stream()):  # a capturable stream: the iterations replay as graphs, as in the sampler
        for m in [int(v) for v in a.m.split(",")]:
            covs = cot.covariances(a.batch, m, dev)
            for kind in a.psf.split(","):
                solves = {name: Solve(name, kind, covs, dev) for name in names}
                for s in solves.values():  # warm-up: graph capture, lazy kernel loading
                    s.run(LO)
                torch.cuda.synchronize()
                if a.once:
                    for s in solves.values():
                        s.run(LO)
                    torch.cuda.synchronize()
                    continue
                for s in solves.values():
                    s.window_ms(HI)
                us = {name: [] for name in names}
                for _ in range(a.reps):  # alternating: both operators see the same clocks and neighbours
                    for name, s in solves.items():
                        lo, hi = s.window_ms(LO), s.window_ms(HI)
                        us[name].append((hi - lo) / (SOLVES * (HI - LO)) * 1e3)
                row = dict(psf=kind, B=a.batch, m=m, op_masked=int(solves["masked_blur"].prob.op),
                           op_twin=int(solves["custom_blur"].prob.op), fold_sym=int(solves["masked_blur"].prob.fold_sym),
                           kept=round(solves["masked_blur"].kept, 4), stopped_below_cap=any(s.short for s in solves.values()))
                for name in names:
                    t = sorted(us[name])
                    row[name] = dict(us_per_iteration=round(t[len(t) // 2], 2), min=round(t[0], 2), max=round(t[-1], 2))
                row["masked_minus_twin_us"] = round(row["masked_blur"]["us_per_iteration"] - row["custom_blur"]["us_per_iteration"], 2)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
