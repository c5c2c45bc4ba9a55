"""Time per batched CG iteration of `weighted_blur` / `weighted_sr` next to their twins without a noise map
(profiles/noise_map.md): 256 x 256, B images, m factor columns.
    gaussian   op 8 on the folded symmetric DCT route      against masked_blur, op 5
    motion     op 8 on k_conv_tile8's masked epilogue       against masked_blur, op 5
    disk       op 9 on k_conv_window's masked epilogue      against masked_blur, op 6
    sr_rank1   op 11, binomial 13 x 13 at s = 4             against custom_sr, op 7
    sr_taps    op 10, a radius-4 disk (49 taps) at s = 4    against custom_sr, op 2
The noise maps are one per image: sigma = sqrt(0.03^2 + 0.1^2 g) (1 + 0.1 b) with the smooth g of the tests' map N and 5 %
random pixels at inf; the masks of the masked twins are those maps' finite pixels.  The weighted systems run with
sigma_y2 = 1, the twins with sigma_s = 0.05.  Both operators of a row live in one process and are timed alternately after a
warm-up by the scheme of masked_blur_time.py: per repetition one device-event window around SOLVES solves capped at LO
iterations and one around SOLVES solves capped at HI (rtol far below reach), the difference divided by the
SOLVES * (HI - LO) iterations between them, so the solves' fixed part (W b, first apply, initialisation, final copy) drops out.
Each row gives, per operator, the median, minimum and maximum over the repetitions (the same-route spread) and the
difference of the medians.
    python profiles/tools/noise_map_time.py [--batch 8] [--m 0,16] [--case gaussian,motion,disk,sr_rank1,sr_taps] [--reps 7]
                                            [--lo 16] [--hi 48]
        (a system that stops below --hi - `stopped_below_cap`, with the fewest iterations seen - needs smaller caps)
    python profiles/tools/noise_map_time.py --once --m 0
        (--once: warm-up + ONE LO-iteration solve of every operator, for a rocprofv3 --kernel-trace --stats run)"""
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
CASES = {"gaussian": ("weighted_blur", "masked_blur", 1), "motion": ("weighted_blur", "masked_blur", 1),
         "disk": ("weighted_blur", "masked_blur", 1), "sr_rank1": ("weighted_sr", "custom_sr", 4),
         "sr_taps": ("weighted_sr", "custom_sr", 4)}


def psf(case):
    from custom_psf_time import disk_psf
    from custom_sr_time import binomial_psf
    from free_hunch_amd.measurements import KERNEL_DIR
    if case == "disk":
        return disk_psf()
    if case == "sr_rank1":
        return binomial_psf(13)
    if case == "sr_taps":
        yy, xx = np.mgrid[-4:5, -4:5]
        k = (yy ** 2 + xx ** 2 <= 16).astype(np.float64)
        return k / k.sum()
    return np.load(os.path.join(KERNEL_DIR, {"gaussian": "gaussian_ks61_std3.0.npy", "motion": "motion_ks61_std0.5.npy"}[case]))


def noise_map(n, b):
    yy, xx = np.mgrid[0:n, 0:n]
    g = 0.5 + 0.5 * np.sin(2 * np.pi * yy / n) * np.cos(2 * np.pi * xx / n)
    sig = np.sqrt(0.03 ** 2 + 0.1 ** 2 * g) * (1.0 + 0.1 * b)
    sig[np.random.default_rng(900 + b).random((n, n)) < 0.05] = np.inf
    return sig


class Solve:
    """fh_cg_solve_batched of one operator over the covariances `covs`, every image with its own noise map / mask"""

    def __init__(self, name, case, covs, dev):
        import inputs
        from free_hunch_amd import _lib
        from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
        from free_hunch_amd.measurements import get_operator
        B, scale = len(covs), CASES[case][2]
        n = S // scale
        self.lib, self.B = _lib, B
        self.ctx = _lib.Context.get(S, 3 * B, 0, slot=6300 + 2 * B + int(name.startswith("weighted")))
        self.ctx.set_exclusive(True)
        kw = dict(device=dev, sigma_s=0.05, in_shape=(1, 3, S, S), kernel=psf(case))
        if scale > 1:
            kw["scale_factor"] = scale
        if name.startswith("weighted"):
            self.ops = [get_operator(name=name, noise_map=noise_map(n, b), **kw) for b in range(B)]
            tabs = [o.weights for o in self.ops]
        elif name == "masked_blur":
            self.ops = [get_operator(name=name, mask=np.isfinite(noise_map(n, b)).astype(np.float64), **kw) for b in range(B)]
            tabs = [o.mask for o in self.ops]
        else:
            self.ops, tabs = [get_operator(name=name, **kw)], []
        self.prob, self.keep = _problem(self.ops[0], covs[0], _solver_sigma_y2(self.ops[0]))
        self.per = _lib.FhBatch()
        self.per.nimg = B
        for b, cov in enumerate(covs):
            self.per.D[b], self.per.r[b], self.per.B[b], self.per.M[b] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(),
                                                                         cov.famC.B.data_ptr(), cov.C.M_dev.data_ptr())
            if tabs:
                t = tabs[b].to(device=dev, dtype=F64).contiguous()
                self.keep.append(t)
                self.per.mask[b] = t.data_ptr()
        self.b = inputs.randn((B, 3, n, n), 77).to(dev).contiguous()
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
    ap.add_argument("--case", default="gaussian,motion,disk,sr_rank1,sr_taps")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lo", type=int, default=LO)
    ap.add_argument("--hi", type=int, default=HI)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import channel_ops_time as cot
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.cuda.stream(torch.cuda.Stream()):  # a capturable stream: the iterations replay as graphs, as in the sampler
        for m in [int(v) for v in a.m.split(",")]:
            covs = cot.covariances(a.batch, m, dev)
            for case in a.case.split(","):
                names = CASES[case][:2]
                solves = {name: Solve(name, case, covs, dev) for name in names}
                for s in solves.values():  # warm-up: graph capture, lazy kernel loading
                    s.run(a.lo)
                torch.cuda.synchronize()
                if a.once:
                    for s in solves.values():
                        s.run(a.lo)
                    torch.cuda.synchronize()
                    continue
                for s in solves.values():
                    s.window_ms(a.hi)
                us = {name: [] for name in names}
                for _ in range(a.reps):  # alternating: both operators see the same clocks and neighbours
                    for name, s in solves.items():
                        lo, hi = s.window_ms(a.lo), s.window_ms(a.hi)
                        us[name].append((hi - lo) / (SOLVES * (a.hi - a.lo)) * 1e3)
                row = dict(case=case, B=a.batch, m=m, caps=[a.lo, a.hi], op_weighted=int(solves[names[0]].prob.op),
                           op_twin=int(solves[names[1]].prob.op), fold_sym=int(solves[names[0]].prob.fold_sym),
                           stopped_below_cap=any(s.short for s in solves.values()),
                           fewest_iterations=min(s.fewest for s in solves.values()))
                for name in names:
                    t = sorted(us[name])
                    row[name] = dict(us_per_iteration=round(t[len(t) // 2], 2), min=round(t[0], 2), max=round(t[-1], 2))
                row["weighted_minus_twin_us"] = round(row[names[0]]["us_per_iteration"] - row[names[1]]["us_per_iteration"], 2)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
