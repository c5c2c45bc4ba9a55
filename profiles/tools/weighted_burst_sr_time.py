"""Time per batched CG iteration of `weighted_burst_sr` (fh_problem.op = 13) against its `burst_sr` twin (op = 12) on the same
frames (profiles/weighted_burst_sr.md): 256 x 256, B images, factor s, K frames of a binomial PSF under `shifted_psf`, m factor
columns.  Op 13 differs from op 12 in the WEIGHTED epilogue of k_conv_dec_frames (fused) or one k_mask pass per frame and image
(chain), and in the CG's weighted direction update (k_cg_step2_w, which also writes W p).  Every image of the batch brings its
own map: frame k = a smooth sigma field in 0.03 .. 0.21 times (1 + 0.5 k), channel c times (1, 1.5, 2)[c], a tenth of the
entries inf, a different seed per image.
Both problems live in one process and are timed alternately after a warm-up, by the scheme of burst_sr_time.py: per repetition
one device-event window around SOLVES solves capped at LO iterations and one around SOLVES solves capped at HI, the difference
divided by the SOLVES * (HI - LO) iterations between them.  Each row gives, per problem, the median, minimum and maximum over the
repetitions (the same-route spread).
    python profiles/tools/weighted_burst_sr_time.py [--batch 8] [--m 0,16] [--frames 4,16] [--scale 4] [--taps 13] [--reps 7]
                                                    [--lo 8] [--hi 24] [--chain]
        (--chain: both ops on the chain, FH_FRAMES_FUSED=0, instead of the fused kernels)
    python profiles/tools/weighted_burst_sr_time.py --once --m 0 --frames 16
        (--once: warm-up + ONE LO-iteration solve of both ops, for a rocprofv3 --kernel-trace --stats run)"""
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
LO, HI, SOLVES = 8, 24, 5


def burst_map(n, K, seed):
    yy, xx = np.mgrid[0:n, 0:n]
    g = 0.5 + 0.5 * np.sin(2 * np.pi * yy / n) * np.cos(2 * np.pi * xx / n)
    sig = np.sqrt(0.03 ** 2 + 0.1 ** 2 * g)
    sig[np.random.default_rng(seed).random((n, n)) < 0.1] = np.inf
    return np.stack([np.stack([sig * f for f in (1.0, 1.5, 2.0)]) * (1 + 0.5 * k) for k in range(K)])


class Solve:
    """fh_cg_solve_batched of op 12 (`weighted` false) or op 13 over the covariances `covs`, on the fused route or the chain"""

    def __init__(self, weighted, chain, scale, taps, K, covs, dev):
        import inputs
        from burst_sr_time import frame_shifts
        from custom_sr_time import binomial_psf
        from free_hunch_amd import _lib
        from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
        from free_hunch_amd.measurements import get_operator
        B, So = len(covs), S // scale
        self.lib, self.B, self.chain = _lib, B, chain
        self.ctx = _lib.Context.get(S, 3 * B, 0, slot=6600 + 4 * B + 2 * int(chain) + int(weighted))
        self.ctx.set_exclusive(True)
        kw = dict(device=dev, sigma_s=0.05, in_shape=(1, 3, S, S), scale_factor=scale, kernels=[binomial_psf(taps)],
                  frame_shifts=frame_shifts(scale, K))
        self.ops = [get_operator(name="weighted_burst_sr", noise_map=burst_map(So, K, 5 + b), **kw) for b in range(B)] if weighted \
            else [get_operator(name="burst_sr", **kw)]
        self.prob, self.keep = _problem(self.ops[0], covs[0], _solver_sigma_y2(self.ops[0]))
        assert self.prob.op == (13 if weighted else 12), self.prob.op
        self.per = _lib.FhBatch()
        self.per.nimg = B
        for b, cov in enumerate(covs):
            self.per.D[b], self.per.r[b], self.per.B[b], self.per.M[b] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(),
                                                                         cov.famC.B.data_ptr(), cov.C.M_dev.data_ptr())
            if weighted:
                self.per.mask[b] = self.ops[b].weights.data_ptr()
        self.b = inputs.randn((B, 3 * K, So, So), 77).to(dev).contiguous()
        self.x = torch.empty_like(self.b)
        self.rtols = (C.c_double * B)(*([1e-300] * B))
        self.infos = (_lib.FhCgInfo * B)()
        self.short, self.fewest = False, 1 << 30

    def run(self, iters):
        if self.chain:
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
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    lo_cap, hi_cap = a.lo, a.hi
    os.environ.pop("FH_FRAMES_FUSED", None)
    import channel_ops_time as cot
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = ("op12", "op13")
    with torch.cuda.stream(torch.cuda.Stream()):  # a capturable stream: the iterations replay as graphs, as in the sampler
        for m in [int(v) for v in a.m.split(",")]:
            covs = cot.covariances(a.batch, m, dev)
            for K in [int(v) for v in a.frames.split(",")]:
                solves = {name: Solve(name == "op13", a.chain, a.scale, a.taps, K, covs, dev) for name in names}
                for s in solves.values():  # warm-up: graph capture, lazy kernel loading, the W p vector of op 13
                    s.run(lo_cap)
                torch.cuda.synchronize()
                if a.once:
                    for s in solves.values():
                        s.run(lo_cap)
                    torch.cuda.synchronize()
                    continue
                for s in solves.values():
                    s.window_ms(hi_cap)
                us = {name: [] for name in names}
                for _ in range(a.reps):  # alternating: both ops see the same clocks and neighbours
                    for name, s in solves.items():
                        lo, hi = s.window_ms(lo_cap), s.window_ms(hi_cap)
                        us[name].append((hi - lo) / (SOLVES * (hi_cap - lo_cap)) * 1e3)
                row = dict(B=a.batch, m=m, K=K, scale=a.scale, psf=f"binomial {a.taps}x{a.taps}", caps=[lo_cap, hi_cap],
                           route="chain" if a.chain else "fused", stopped_below_cap=any(s.short for s in solves.values()),
                           fewest_iterations=min(s.fewest for s in solves.values()),
                           doubles_per_vector=a.batch * 3 * K * (S // a.scale) ** 2)
                for name in names:
                    t = sorted(us[name])
                    row[name] = dict(us_per_iteration=round(t[len(t) // 2], 2), min=round(t[0], 2), max=round(t[-1], 2))
                row["op13_minus_op12_us"] = round(row["op13"]["us_per_iteration"] - row["op12"]["us_per_iteration"], 2)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
