"""Time per batched CG iteration of `custom_sr` on its two routes (profiles/custom_sr.md): 256 x 256, B images, factor s,
m factor columns, a rank-1 binomial PSF - fh_problem.op = 7 (rectangular folded DCT passes) against op = 2 (the same operator
built under FH_NO_FOLD=1: k_conv_up, the symmetric DCT passes, k_conv_dec).
Both problems live in one process and are timed alternately after a warm-up, by the scheme of masked_blur_time.py: per
repetition one device-event window around SOLVES solves capped at LO iterations and one around SOLVES solves capped at HI
(rtol far below reach), the difference divided by the SOLVES * (HI - LO) iterations between them, so the solves' fixed part drops
out.  Each row gives, per route, the median, minimum and maximum over the repetitions (the same-route spread) and the
difference of the medians.
    python profiles/tools/custom_sr_time.py [--batch 8] [--m 0,16] [--scale 4] [--taps 13] [--reps 7] [--lo 16] [--hi 48]
        (a system that stops below --hi - `stopped_below_cap`, with the fewest iterations seen - needs smaller caps: with factor
        columns these low-resolution systems reach the pAp <= 1e-16 stop early)
    python profiles/tools/custom_sr_time.py --once --m 0
        (--once: warm-up + ONE 16-iteration solve of either route, for a rocprofv3 --kernel-trace --stats run)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "profiles", "tools")]
S = 256
LO, HI, SOLVES = 16, 48, 7


def binomial_psf(n):
    v = np.array([1.0])
    for _ in range(n - 1):
        v = np.convolve(v, [0.5, 0.5])
    return np.outer(v, v)


class Solve:
    """fh_cg_solve_batched of one custom_sr problem over the covariances `covs`; fold = False builds it under FH_NO_FOLD=1"""

    def __init__(self, fold, scale, taps, covs, dev):
        import inputs
        from free_hunch_amd import _lib
        from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
        from free_hunch_amd.measurements import get_operator
        B, So = len(covs), S // scale
        self.lib, self.B = _lib, B
        self.ctx = _lib.Context.get(S, 3 * B, 0, slot=6200 + 2 * B + int(fold))
        self.ctx.set_exclusive(True)
        op = get_operator(name="custom_sr", device=dev, sigma_s=0.05, in_shape=(1, 3, S, S), scale_factor=scale,
                          kernel=binomial_psf(taps))
        before = os.environ.pop("FH_NO_FOLD", None)
        if not fold:
            os.environ["FH_NO_FOLD"] = "1"
        try:
            self.prob, self.keep = _problem(op, covs[0], _sigma_y2(op))
        finally:
            os.environ.pop("FH_NO_FOLD", None)
            if before is not None:
                os.environ["FH_NO_FOLD"] = before
        assert self.prob.op == (7 if fold else 2), self.prob.op
        self.per = _lib.FhBatch()
        self.per.nimg = B
        for b, cov in enumerate(covs):
            self.per.D[b], self.per.r[b], self.per.B[b], self.per.M[b] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(),
                                                                         cov.famC.B.data_ptr(), cov.C.M_dev.data_ptr())
        self.b = inputs.randn((B, 3, So, So), 77).to(dev).contiguous()
        self.x = torch.empty_like(self.b)
        self.rtols = (C.c_double * B)(*([1e-300] * B))
        self.infos = (_lib.FhCgInfo * B)()
        self.short, self.fewest = False, 1 << 30

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
        self.fewest = min(self.fewest, min(min(n) for n in ns))
        return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--m", default="0,16")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--taps", type=int, default=13)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lo", type=int, default=LO)
    ap.add_argument("--hi", type=int, default=HI)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    lo_cap, hi_cap = a.lo, a.hi
    import channel_ops_time as cot
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = ("op7", "op2")
    with torch.cuda.stream(torch.cuda.Stream()):  # a capturable stream: the iterations replay as graphs, as in the sampler
        for m in [int(v) for v in a.m.split(",")]:
            covs = cot.covariances(a.batch, m, dev)
            solves = {"op7": Solve(True, a.scale, a.taps, covs, dev), "op2": Solve(False, a.scale, a.taps, covs, dev)}
            for s in solves.values():  # warm-up: graph capture, lazy kernel loading
                s.run(lo_cap)
            torch.cuda.synchronize()
            agree = float((solves["op7"].x - solves["op2"].x).abs().max() / solves["op2"].x.abs().max())
            if a.once:
                for s in solves.values():
                    s.run(lo_cap)
                torch.cuda.synchronize()
                continue
            for s in solves.values():
                s.window_ms(hi_cap)
            us = {name: [] for name in names}
            for _ in range(a.reps):  # alternating: both routes see the same clocks and neighbours
                for name, s in solves.items():
                    lo, hi = s.window_ms(lo_cap), s.window_ms(hi_cap)
                    us[name].append((hi - lo) / (SOLVES * (hi_cap - lo_cap)) * 1e3)
            row = dict(B=a.batch, m=m, scale=a.scale, psf=f"binomial {a.taps}x{a.taps}", caps=[lo_cap, hi_cap],
                       solutions_after_lo_rel_diff=agree, stopped_below_cap=any(s.short for s in solves.values()),
                       fewest_iterations=min(s.fewest for s in solves.values()))
            for name in names:
                t = sorted(us[name])
                row[name] = dict(us_per_iteration=round(t[len(t) // 2], 2), min=round(t[0], 2), max=round(t[-1], 2))
            row["op2_minus_op7_us"] = round(row["op2"]["us_per_iteration"] - row["op7"]["us_per_iteration"], 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
