"""Time per batched CG iteration of `varying_blur` (fh_problem.op = 14) on its two routes (profiles/varying_blur.md): 256 x 256, B
images, K PSFs on a grid (2 x 2, 3 x 3, ...) blended by `grid_blend_weights`, m factor columns - the fused kernel (k_conv_blend:
one launch per direction and iteration) against the chain (FH_BLEND_FUSED=0: per PSF one convolution launch and one streaming
multiply, kernels the library had before op 14), and `custom_blur` with ONE PSF of the family on its tap list (op 1,
FH_NO_FOLD=1) as the per-PSF yardstick.  The family: 13 x 13 windows of an elongated Gaussian (sigma 3 along, 0.9 across) turned
by another angle per grid node, entries below 2 % of the peak dropped - non-separable, 50 .. 70 taps, ragged lists.
All problems live in one process and are timed alternately after a warm-up, by the scheme of burst_sr_time.py: per repetition
one device-event window around SOLVES solves capped at LO iterations and one around SOLVES solves capped at HI (rtol far below
reach), the difference divided by the SOLVES * (HI - LO) iterations between them, so the solves' fixed part drops out.  Each row
gives, per route, the median, minimum and maximum over the repetitions (the same-route spread).
    python profiles/tools/varying_blur_time.py [--batch 8] [--m 0,16] [--psfs 4,9] [--taps 13] [--reps 7] [--lo 8] [--hi 24]
        (a system that stops below --hi - `stopped_below_cap`, with the fewest iterations seen - needs smaller caps)
    python profiles/tools/varying_blur_time.py --once --m 0 --psfs 9
        (--once: warm-up + ONE LO-iteration solve of every route, for a rocprofv3 --kernel-trace --stats run)"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "profiles", "tools")]
S = 256
LO, HI, SOLVES = 8, 24, 5


def streak_psf(size, k, K):
    """PSF k of K: an elongated Gaussian turned by pi (k + 0.5) / K (never along an axis), thresholded and normalised"""
    h = size // 2
    yy, xx = np.mgrid[-h:h + 1, -h:h + 1].astype(np.float64)
    th = math.pi * (k + 0.5) / K
    u, v = xx * math.cos(th) + yy * math.sin(th), -xx * math.sin(th) + yy * math.cos(th)
    g = np.exp(-0.5 * ((u / 3.0) ** 2 + (v / 0.9) ** 2))
    g[g < 0.02 * g.max()] = 0.0
    return g / g.sum()


def grid_of(K):
    r = int(round(math.sqrt(K)))
    return (r, r) if r * r == K else (1, K)


class Solve:
    """fh_cg_solve_batched of one problem over the covariances `covs`: route "fused" / "chain" (varying_blur under FH_BLEND_FUSED
    = 1 / 0, read by the library at every call) or "op1" (custom_blur with PSF K // 2 of the family, built under FH_NO_FOLD=1)"""

    def __init__(self, route, taps, K, covs, dev):
        import inputs
        from free_hunch_amd import _lib
        from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
        from free_hunch_amd.measurements import get_operator
        B = len(covs)
        self.lib, self.B, self.route = _lib, B, route
        self.ctx = _lib.Context.get(S, 3 * B, 0, slot=6800 + 4 * B + ("fused", "chain", "op1").index(route))
        self.ctx.set_exclusive(True)
        kw = dict(device=dev, sigma_s=0.05, in_shape=(1, 3, S, S))
        if route == "op1":
            op = get_operator(name="custom_blur", kernel=streak_psf(taps, K // 2, K), **kw)  # (near 45 degrees: the flattest PSFs fill half of their window and would take the dense-window kernel)
            before, os.environ["FH_NO_FOLD"] = os.environ.get("FH_NO_FOLD"), "1"
            try:
                self.prob, self.keep = _problem(op, covs[0], _sigma_y2(op))
            finally:
                os.environ.pop("FH_NO_FOLD", None)
                if before is not None:
                    os.environ["FH_NO_FOLD"] = before
            assert self.prob.op == 1 and self.prob.ntaps2 == 0 and not self.prob.fold_fwd_w, "the yardstick must run on its tap list"
            self.taps = [int(self.prob.ntaps)]
        else:
            op = get_operator(name="varying_blur", kernels=[streak_psf(taps, k, K) for k in range(K)], psf_grid=grid_of(K), **kw)
            self.prob, self.keep = _problem(op, covs[0], _sigma_y2(op))
            assert self.prob.op == 14, self.prob.op
            self.taps = [t.n for t in op.frames]
        self.per = _lib.FhBatch()
        self.per.nimg = B
        for b, cov in enumerate(covs):
            self.per.D[b], self.per.r[b], self.per.B[b], self.per.M[b] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(),
                                                                         cov.famC.B.data_ptr(), cov.C.M_dev.data_ptr())
        self.b = inputs.randn((B, 3, S, S), 77).to(dev).contiguous()
        self.x = torch.empty_like(self.b)
        self.rtols = (C.c_double * B)(*([1e-300] * B))
        self.infos = (_lib.FhCgInfo * B)()
        self.short, self.fewest = False, 1 << 30

    def run(self, iters):
        if self.route != "op1":
            os.environ["FH_BLEND_FUSED"] = "0" if self.route == "chain" else "1"
        try:
            self.lib.check(self.ctx.lib.fh_cg_solve_batched(self.ctx.h, C.byref(self.prob), C.byref(self.per), self.b.data_ptr(),
                                                            self.x.data_ptr(), self.rtols, 0.0, iters, self.infos,
                                                            self.lib.stream()), "fh_cg_solve_batched")
        finally:
            os.environ.pop("FH_BLEND_FUSED", None)
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
    ap.add_argument("--psfs", default="4,9")
    ap.add_argument("--taps", type=int, default=13)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lo", type=int, default=LO)
    ap.add_argument("--hi", type=int, default=HI)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    lo_cap, hi_cap = a.lo, a.hi
    os.environ.pop("FH_BLEND_FUSED", None)
    import channel_ops_time as cot
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = ("fused", "chain", "op1")
    with torch.cuda.stream(torch.cuda.Stream()):  # a capturable stream: the iterations replay as graphs, as in the sampler
        for m in [int(v) for v in a.m.split(",")]:
            covs = cot.covariances(a.batch, m, dev)
            for K in [int(v) for v in a.psfs.split(",")]:
                solves = {name: Solve(name, a.taps, K, covs, dev) for name in names}
                for s in solves.values():  # warm-up: graph capture, lazy kernel loading
                    s.run(lo_cap)
                torch.cuda.synchronize()
                same_bits = bool(torch.equal(solves["fused"].x, solves["chain"].x))
                if a.once:
                    for s in solves.values():
                        s.run(lo_cap)
                    torch.cuda.synchronize()
                    continue
                for s in solves.values():
                    s.window_ms(hi_cap)
                us = {name: [] for name in names}
                for _ in range(a.reps):  # alternating: all routes see the same clocks and neighbours
                    for name, s in solves.items():
                        lo, hi = s.window_ms(lo_cap), s.window_ms(hi_cap)
                        us[name].append((hi - lo) / (SOLVES * (hi_cap - lo_cap)) * 1e3)
                row = dict(B=a.batch, m=m, K=K, psf=f"streak {a.taps}x{a.taps}", taps=solves["fused"].taps,
                           op1_taps=solves["op1"].taps[0], caps=[lo_cap, hi_cap], fused_equals_chain_after_lo=same_bits,
                           stopped_below_cap=any(s.short for s in solves.values()),
                           fewest_iterations=min(s.fewest for s in solves.values()))
                for name in names:
                    t = sorted(us[name])
                    row[name] = dict(us_per_iteration=round(t[len(t) // 2], 2), min=round(t[0], 2), max=round(t[-1], 2))
                row["chain_minus_fused_us"] = round(row["chain"]["us_per_iteration"] - row["fused"]["us_per_iteration"], 2)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
