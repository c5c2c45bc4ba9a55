"""Time per batched CG iteration of the colorization, denoising and inpainting operators at 256 x 256, B images, m factor
columns (profiles/channel_ops.md).  The same fh_cg_solve_batched call is run with two iteration caps (rtol far below reach,
so every solve runs to its cap); the difference of the two device-event times divided by the difference of the caps is
the time of one iteration without the solve's fixed part (first apply, initialisation, final copy).
    python profiles/tools/channel_ops_time.py [--batch 4] [--m 0,32]
    python profiles/tools/channel_ops_time.py --once colorization --m 32
        (--once: warm-up solve + ONE 16-iteration solve of that operator, for a rocprofv3 --kernel-trace --stats run)"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
F64 = torch.float64
S = 256
LO, HI = 16, 48  # iteration caps (multiples of the 8-iteration chunk; at m = 32 the systems reach pAp <= 1e-16 after ~74)


def operator(name, dev):
    from free_hunch_amd.measurements import get_operator
    return get_operator(name=name, device=dev, sigma_s=0.05, in_shape=(1, 3, S, S), channel_weights=(0.299, 0.587, 0.114),
                        mask=torch.ones(1, 3, S, S),  # inpainting with everything observed: the same A as denoising
                        mask_opt={"mask_type": "random", "mask_prob_range": (0.1, 0.3), "image_size": S})


def covariances(B, m, dev):
    import inputs
    from free_hunch_amd import covariance as hc
    data = os.path.join(ROOT, "free-hunch_amd", "data")
    covs = []
    for b in range(B):
        cov = hc.CovarianceHessianBFGSDCT(data, 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=b)
        for what, a in inputs.script(4242 + b, (1, 3, S, S), m // 2, 80.0):
            if what == "time":
                cov.update_time_step(a["x"].to(dev), a["sigma"], a["sigma_next"], a["score"].to(dev))
            else:
                cov.update_space_step(a["m0"].to(dev), a["m1"].to(dev), a["sigma"], a["x"].to(dev), a["xn"].to(dev))
        assert cov.famC.m == m
        covs.append(cov)
    return covs


class Solve:
    def __init__(self, name, covs, dev):
        import inputs
        from free_hunch_amd import _lib
        from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
        B = len(covs)
        self.lib, self.B = _lib, B
        self.ctx = _lib.Context.get(S, 3 * B, 0, slot=6000 + B)
        self.ctx.set_exclusive(True)
        op = operator(name, dev)
        self.prob, self.keep = _problem(op, covs[0], _sigma_y2(op))
        self.per = _lib.FhBatch()
        self.per.nimg = B
        mask = torch.ones(3 * S * S, dtype=F64, device=dev)
        for b, cov in enumerate(covs):
            self.per.D[b], self.per.r[b], self.per.B[b], self.per.M[b] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(),
                                                                         cov.famC.B.data_ptr(), cov.C.M_dev.data_ptr())
            self.per.mask[b] = mask.data_ptr()
        self.keep.append(mask)
        planes = 1 if name == "colorization" else 3
        self.b = inputs.randn((B, planes, S, S), 77).to(dev).contiguous()
        self.x = torch.empty_like(self.b)
        self.rtols = (C.c_double * B)(*([1e-300] * B))
        self.infos = (_lib.FhCgInfo * B)()

    def run(self, iters):
        self.lib.check(self.ctx.lib.fh_cg_solve_batched(self.ctx.h, C.byref(self.prob), C.byref(self.per), self.b.data_ptr(),
                                                        self.x.data_ptr(), self.rtols, 0.0, iters, self.infos,
                                                        self.lib.stream()), "fh_cg_solve_batched")
        return [self.infos[b].niter for b in range(self.B)]

    def timed(self, iters, reps=9):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            n = self.run(iters)
            e1.record()
            torch.cuda.synchronize()
            assert n == [iters] * self.B, n  # every image ran to the cap
            ts.append(e0.elapsed_time(e1))
        return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--m", default="0,32")
    ap.add_argument("--once", default="")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []
    with torch.cuda.stream(torch.cuda.Stream()):  # a capturable stream: the iterations replay as graphs, as in the sampler
        for m in [int(v) for v in a.m.split(",")]:
            covs = covariances(a.batch, m, dev)
            for name in ([a.once] if a.once else ["colorization", "noise", "inpainting"]):
                s = Solve(name, covs, dev)
                s.run(LO)  # warm-up: graph capture, lazy kernel loading
                torch.cuda.synchronize()
                if a.once:
                    s.run(LO)
                    torch.cuda.synchronize()
                    continue
                lo, hi = s.timed(LO), s.timed(HI)
                rows.append(dict(operator=name, B=a.batch, m=m, ms_lo=round(lo, 4), ms_hi=round(hi, 4),
                                 us_per_iteration=round((hi - lo) / (HI - LO) * 1e3, 2)))
                print(json.dumps(rows[-1]), flush=True)


if __name__ == "__main__":
    main()
