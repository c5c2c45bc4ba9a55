"""Time per batched CG iteration of `burst_sr` (fh_problem.op = 12) on its two routes (profiles/burst_sr.md): 256 x 256, B images,
factor s, K frames of a binomial PSF under `shifted_psf`, m factor columns - the fused frame kernels (k_conv_up_frames,
k_conv_dec_frames: one launch each per iteration) against the chain (FH_FRAMES_FUSED=0: k_conv_up / k_conv_dec per frame and
image), and `custom_sr` on its tap list (op 2, K = 1, FH_NO_FOLD=1) at the same PSF as the per-frame yardstick.
All problems live in one process and are timed alternately after a warm-up, by the scheme of custom_sr_time.py: per repetition
one device-event window around SOLVES solves capped at LO iterations and one around SOLVES solves capped at HI (rtol far below
reach), the difference divided by the SOLVES * (HI - LO) iterations between them, so the solves' fixed part drops out.  Each row
gives, per route, the median, minimum and maximum over the repetitions (the same-route spread).
    python profiles/tools/burst_sr_time.py [--batch 8] [--m 0,16] [--frames 4,16] [--scale 4] [--taps 13] [--reps 7] [--lo 8] [--hi 24]
        (a system that stops below --hi - `stopped_below_cap`, with the fewest iterations seen - needs smaller caps)
    python profiles/tools/burst_sr_time.py --once --m 0 --frames 16
        (--once: warm-up + ONE LO-iteration solve of every route, for a rocprofv3 --kernel-trace --stats run)"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "profiles", "tools")]
S = 256
LO, HI, SOLVES = 8, 24, 5


def frame_shifts(scale, K):
    """K = 4: the half-sampling lattice (0, 0), (0, s/2), (s/2, 0), (s/2, s/2); else the first K of all s^2 integer shifts"""
    h = scale // 2
    if K == 4 and scale > 2:
        return [(0, 0), (0, h), (h, 0), (h, h)]
    return [(a, b) for a in range(scale) for b in range(scale)][:K]


class Solve:
    """fh_cg_solve_batched of one problem over the covariances `covs`: route "fused" / "chain" (burst_sr under FH_FRAMES_FUSED
    unset / 0, read by the library at every call) or "op2" (custom_sr built under FH_NO_FOLD=1)"""

    def __init__(self, route, scale, taps, K, covs, dev):
        import inputs
        from custom_sr_time import binomial_psf
        from free_hunch_amd import _lib
        from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
        from free_hunch_amd.measurements import get_operator
        B, So = len(covs), S // scale
        self.lib, self.B, self.route = _lib, B, route
        self.ctx = _lib.Context.get(S, 3 * B, 0, slot=6400 + 4 * B + ("fused", "chain", "op2").index(route))
        self.ctx.set_exclusive(True)
        kw = dict(device=dev, sigma_s=0.05, in_shape=(1, 3, S, S), scale_factor=scale)
        if route == "op2":
            op = get_operator(name="custom_sr", kernel=binomial_psf(taps), **kw)
            before, os.environ["FH_NO_FOLD"] = os.environ.get("FH_NO_FOLD"), "1"
            try:
                self.prob, self.keep = _problem(op, covs[0], _sigma_y2(op))
            finally:
                os.environ.pop("FH_NO_FOLD", None)
                if before is not None:
                    os.environ["FH_NO_FOLD"] = before
            K = 1
        else:
            op = get_operator(name="burst_sr", kernels=[binomial_psf(taps)], frame_shifts=frame_shifts(scale, K), **kw)
            self.prob, self.keep = _problem(op, covs[0], _sigma_y2(op))
        assert self.prob.op == (2 if route == "op2" else 12), self.prob.op
        self.per = _lib.FhBatch()
        self.per.nimg = B
        for b, cov in enumerate(covs):
            self.per.D[b], self.per.r[b], self.per.B[b], self.per.M[b] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(),
                                                                         cov.famC.B.data_ptr(), cov.C.M_dev.data_ptr())
        self.b = inputs.randn((B, 3 * K, So, So), 77).to(dev).contiguous()
        self.x = torch.empty_like(self.b)
        self.rtols = (C.c_double * B)(*([1e-300] * B))
        self.infos = (_lib.FhCgInfo * B)()
        self.short, self.fewest = False, 1 << 30

    def run(self, iters):
        if self.route == "chain":
            os.environ["FH_FRAMES_FUSED"] = "0"
        try:
            self.lib.check(self.ctx.lib.fh_cg_solve_batched(self.ctx.h, C.byref(self.prob), C.byref(self.per), self.b.data_ptr(),
                                                            self.x.data_ptr(), self.rtols, 0.0, iters, self.infos,
                                                            self.lib.stream()), "fh_cg_solve_batched")
        finally:
            os.environ.pop("FH_FRAMES_FUSED", None)
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
    ap.add_argument("--frames", default="4,16")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--taps", type=int, default=13)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lo", type=int, default=LO)
    ap.add_argument("--hi", type=int, default=HI)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    lo_cap, hi_cap = a.lo, a.hi
    os.environ.pop("FH_FRAMES_FUSED", None)
    import channel_ops_time as cot
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = ("fused", "chain", "op2")
    with torch.cuda.stream(torch.cuda.Stream()):  # a capturable stream: the iterations replay as graphs, as in the sampler
        for m in [int(v) for v in a.m.split(",")]:
            covs = cot.covariances(a.batch, m, dev)
            for K in [int(v) for v in a.frames.split(",")]:
                solves = {name: Solve(name, a.scale, a.taps, K, covs, dev) for name in names}
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
                row = dict(B=a.batch, m=m, K=K, scale=a.scale, psf=f"binomial {a.taps}x{a.taps}", caps=[lo_cap, hi_cap],
                           fused_equals_chain_after_lo=same_bits, stopped_below_cap=any(s.short for s in solves.values()),
                           fewest_iterations=min(s.fewest for s in solves.values()))
                for name in names:
                    t = sorted(us[name])
                    row[name] = dict(us_per_iteration=round(t[len(t) // 2], 2), min=round(t[0], 2), max=round(t[-1], 2))
                row["chain_minus_fused_us"] = round(row["chain"]["us_per_iteration"] - row["fused"]["us_per_iteration"], 2)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
