"""Time per batched CG iteration of `fourier_sampling` (fh_problem.op = 15, profiles/fourier_sampling.md): 256 x 256, B images,
a cartesian mask at acceleration R, m factor columns - next to the two nearest existing routes with the same dense-pass count:
`noise` (op 0: k_mask, the symmetric DCT pair, k_mask) and `custom_blur` with a rank-1 PSF that is NOT mirror symmetric, so that
its fold takes the dense bases (op 1, fold_sym = 0: four k_gemm_f64 passes).  Op 15 runs four k_dct_rect passes between its two
butterfly launches (k_hartley_fix).
All problems live in one process and are timed alternately after a warm-up, by the scheme of varying_blur_time.py: per
repetition one device-event window around SOLVES solves capped at LO iterations and one around SOLVES solves capped at HI (rtol
far below reach), the difference divided by the SOLVES * (HI - LO) iterations between them, so the solves' fixed part drops
out.  Each row gives, per route, the median, minimum and maximum over the repetitions (the same-route spread).
    python profiles/tools/fourier_sampling_time.py [--batch 8] [--m 0,16] [--acceleration 4] [--reps 7] [--lo 8] [--hi 24]
    python profiles/tools/fourier_sampling_time.py --once --m 0
        (--once: warm-up + ONE LO-iteration solve of the op-15 route alone, for a rocprofv3 --kernel-trace --stats run)"""
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
NAMES = ("fourier", "noise", "op1_dense_fold")


class Solve:
    """fh_cg_solve_batched of one problem over the covariances `covs`"""

    def __init__(self, route, acceleration, covs, dev):
        import inputs
        from free_hunch_amd import _lib
        from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
        from free_hunch_amd.measurements import get_operator
        B = len(covs)
        self.lib, self.B, self.route = _lib, B, route
        self.ctx = _lib.Context.get(S, 3 * B, 0, slot=6900 + 4 * B + NAMES.index(route))
        self.ctx.set_exclusive(True)
        kw = dict(device=dev, sigma_s=0.05, in_shape=(1, 3, S, S))
        if route == "fourier":
            op = get_operator(name="fourier_sampling", pattern="cartesian", acceleration=acceleration, **kw)
            want = 15
        elif route == "noise":
            op = get_operator(name="noise", **kw)
            want = 0
        else:  # a 9 x 9 outer product of two skewed 1-D profiles: rank 1, no mirror symmetry
            prof = np.array([0.02, 0.05, 0.10, 0.16, 0.25, 0.20, 0.12, 0.07, 0.03])
            op = get_operator(name="custom_blur", kernel=np.outer(prof, prof[::-1] ** 1.5 / (prof ** 1.5).sum()), **kw)
            want = 1
        self.prob, self.keep = _problem(op, covs[0], _solver_sigma_y2(op))
        assert self.prob.op == want, (route, self.prob.op)
        if route == "op1_dense_fold":
            assert self.prob.fold_fwd_w and self.prob.fold_sym == 0, "the yardstick must run on dense folded bases"
        self.per = _lib.FhBatch()
        self.per.nimg = B
        mask = self.keep[-1] if route in ("fourier", "noise") else None
        for b, cov in enumerate(covs):
            self.per.D[b], self.per.r[b], self.per.B[b], self.per.M[b] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(),
                                                                         cov.famC.B.data_ptr(), cov.C.M_dev.data_ptr())
            if mask is not None:
                self.per.mask[b] = mask.data_ptr()
        self.b = inputs.randn((B, 3, S, S), 77).to(dev).contiguous()
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
    ap.add_argument("--acceleration", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lo", type=int, default=LO)
    ap.add_argument("--hi", type=int, default=HI)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    lo_cap, hi_cap = a.lo, a.hi
    import channel_ops_time as cot
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = NAMES[:1] if a.once else NAMES
    with torch.cuda.stream(torch.cuda.Stream()):  # a capturable stream: the iterations replay as graphs, as in the sampler
        for m in [int(v) for v in a.m.split(",")]:
            covs = cot.covariances(a.batch, m, dev)
            solves = {name: Solve(name, a.acceleration, covs, dev) for name in names}
            for s in solves.values():  # warm-up: graph capture, lazy kernel loading
                s.run(lo_cap)
            torch.cuda.synchronize()
            if a.once:
                solves["fourier"].run(lo_cap)
                torch.cuda.synchronize()
                continue
            for s in solves.values():
                s.window_ms(hi_cap)
            us = {name: [] for name in names}
            for _ in range(a.reps):  # alternating: all routes see the same clocks and neighbours
                for name, s in solves.items():
                    lo, hi = s.window_ms(lo_cap), s.window_ms(hi_cap)
                    us[name].append((hi - lo) / (SOLVES * (hi_cap - lo_cap)) * 1e3)
            row = dict(B=a.batch, m=m, acceleration=a.acceleration, caps=[lo_cap, hi_cap],
                       stopped_below_cap=any(s.short for s in solves.values()),
                       fewest_iterations=min(s.fewest for s in solves.values()))
            for name in names:
                t = sorted(us[name])
                row[name] = dict(us_per_iteration=round(t[len(t) // 2], 2), min=round(t[0], 2), max=round(t[-1], 2))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
