"""The launch shape bench.py times (BASELINE.json configs[1]): 8 images in lock-step at 256 x 256, gaussian_blur, shipped
DCT prior - the folded-blur DCT bases, the batched CG (grid z = image, per-image diagonal in the m = 0 epilogue of the
symmetric DCT pass), the batched cov-branch - against eight per-image `conditional_sampler` runs, plus the solver-level
check of the batched m = 0 path asked for by the round-2 review (distinct per-image diagonals at S = 128 / 256)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inputs
import nets
from test_hip_parity import T, _base_kwargs, _hip_op, maxabs

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "free-hunch_amd", "data")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _batch_inputs(B, S, dev, opname="gaussian_blur"):
    ops, ys, noise = [], [], []
    for b in range(B):
        op = _hip_op(opname, S, dev)
        op.ctx_slot = b
        ops.append(op)
        x0 = inputs.smooth_image(S, 170 + b).to(dev)
        y = op.forward(x0, noiseless=True)
        ys.append(y + 0.1 * inputs.randn(tuple(y.shape), 180 + b, torch.float32).to(dev))
        noise.append(inputs.randn((1, 3, S, S), 190 + b, torch.float32))
    return ops, ys, torch.cat(noise).to(dev)


def _lists(trace):
    return ([t["niter"] for t in trace], [t["k"] for t in trace], [t["branch"] for t in trace])


@pytest.mark.parametrize("fold", ["folded", "taps"])
def test_batched8_256_equals_per_image_bitwise_denoiser(dev, fold, monkeypatch):
    """B = 8, 256 x 256, gaussian_blur, dct_diagonal, Heun-8 with the default thresholds: calls 0-5 run with m = 0 (sigma >
    10), the rest with m = 2 .. 4.  The denoiser is the closed-form Gaussian-prior one (elementwise float64: its values do
    not depend on the batch size), so the batched and the per-image runs see identical inputs and every difference would
    come from the Free Hunch kernels: the CG of this configuration stops un-converged on a cond ~ 1e6 system (rounding-chaotic
    iteration counts, tests/test_cg_sensitivity.py), so IDENTICAL niter lists mean the batched kernel sequence reproduces
    the per-image one to the last bit.  The std threshold is moved to 0.075 so that both the vjp and the cov branch (the
    batched C . mat sequence) occur.  `taps`: the same with FH_NO_FOLD=1 (blur as tap-list passes instead of folded into
    the DCT bases)."""
    from free_hunch_amd import measurements
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_batched
    if fold == "taps":
        monkeypatch.setenv("FH_NO_FOLD", "1")
    measurements._FOLD_CACHE.clear()
    B, S = 8, 256
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(DATA, {"denoiser_mean_error_threshold": 0.075})
    ops, ys, noise = _batch_inputs(B, S, dev)
    run = dict(num_steps=8, sigma_min=0.002, sigma_max=80, rho=7, solver="heun")
    xb = conditional_sampler_batched(net, noise, ys, ops, **run, **kw)
    tb = [m.trace for m in conditional_sampler_batched.last_mechanisms]
    assert any(t["k"] == 0 for t in tb[0]) and tb[0][-1]["k"] >= 2  # m = 0 and m > 0 calls
    branches = {t["branch"] for tr in tb for t in tr}
    assert branches == {"vjp", "cov"}, branches
    worst = 0.0
    for b in range(B):
        x1, _, _ = conditional_sampler(net, noise[b:b + 1], None, None, measurement=ys[b], operator=ops[b], **run, **kw)
        t1 = conditional_sampler.last_mechanism.trace
        assert _lists(t1) == _lists(tb[b]), (b, _lists(t1), _lists(tb[b]))
        worst = max(worst, maxabs(x1, xb[b:b + 1]))
    assert worst < 1e-9, worst  # north-star tolerance is 1e-3; identical iteration lists leave only last-bit differences
    measurements._FOLD_CACHE.clear()


def test_batched8_256_equals_per_image_hip_unet(dev):
    """The same launch shape with the HIP UNet in the loop (256 x 256, ImageNet-256 block structure at 32 channels, output
    layer damped by 0.05: the denoiser of the recorded `*_damped` fixtures) on the inpainting operator with max_rtol = 1e-6,
    i.e. the configuration of ip256_heun12_tight_damped, which reproduces the reference's recording to 1.4e-4.  The UNet
    sums over a different tile partition at batch 8 than at batch 1 (1e-6 relative); an un-converged CG would amplify that to
    O(1) (see above), a converged one leaves the trajectory's own gain on it.  (Measured with gaussian_blur instead: 1.5e-4 ..
    1.1e-3 over the eight images at max_rtol = 1e-9 - the blur systems amplify ~10x more than the mask; that operator is
    covered bitwise by the test above.)  Identical k and branch lists, iteration counts within 3 %, outputs within 1e-3."""
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_batched
    B, S = 8, 256
    net = nets.damped_hip_net(inputs.SMALL_C, 13, dev)
    kw = _base_kwargs(DATA, {"max_rtol": 1e-6})
    ops, ys, noise = _batch_inputs(B, S, dev, "inpainting")
    run = dict(num_steps=6, sigma_min=0.002, sigma_max=80, rho=7, solver="heun")
    xb = conditional_sampler_batched(net, noise, ys, ops, **run, **kw)
    tb = [m.trace for m in conditional_sampler_batched.last_mechanisms]
    errs = []
    for b in range(B):
        x1, _, _ = conditional_sampler(net, noise[b:b + 1], None, None, measurement=ys[b], operator=ops[b], **run, **kw)
        t1 = conditional_sampler.last_mechanism.trace
        n1, k1, b1 = _lists(t1)
        nb, kb, bb = _lists(tb[b])
        assert k1 == kb and b1 == bb, (b, k1, kb, b1, bb)
        # (measured over random masks: 0 .. 2.4 % on the long high-sigma solves - the batch-8 UNet's 1e-6 rounding difference
        # moved through cond ~ 1e6 systems; the masks are reproducible since conftest seeds the global generators per test)
        assert all(abs(p - q) <= 0.03 * p + 2 for p, q in zip(n1, nb)), (b, n1, nb)
        errs.append(maxabs(x1, xb[b:b + 1]))
    print("batched vs per-image, HIP UNet, max-abs per image:", ["%.2e" % e for e in errs], flush=True)
    assert max(errs) < 1e-3, errs


# ---------------------------------------------------------------- solver level: batched m = 0 path, distinct diagonals
def _solver_case(S, opname, dev, nimg=3):
    """nimg covariance models with DISTINCT diagonals (different noise levels after one time update each, no factor
    columns: the m = 0 path whose diagonal apply rides in the symmetric DCT pass's epilogue, indexed per image), one
    measurement each."""
    from free_hunch_amd import covariance as hc
    import tempfile
    d = 3 * S * S
    data = DATA
    if S != 256:
        data = tempfile.mkdtemp()
        dv = torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
        torch.save(dv, os.path.join(data, "dct_variance.pt"))
    mask = None
    if opname == "inpainting":
        g = np.random.default_rng(5)
        mask = torch.from_numpy((g.random((1, 1, S, S)) > 0.7).astype(np.float32)).repeat(1, 3, 1, 1)
    ops, covs, ys, xs = [], [], [], []
    for b in range(nimg):
        op = _hip_op(opname, S, dev, mask)
        op.ctx_slot = b
        cov = hc.CovarianceHessianBFGSDCT(data, 80.0 ** 2, d, device=dev, use_precalculated_info=True, ctx_slot=b)
        x = inputs.randn((1, 3, S, S), 300 + b).to(dev) * 40.0
        cov.update_time_step(x, 80.0, [40.0, 25.0, 12.0][b % 3], -x / 80.0 ** 2 * 0.5)  # distinct D per image
        x0 = inputs.smooth_image(S, 310 + b).to(dev)
        y = op.forward(x0, noiseless=True)
        ys.append(y + 0.1 * inputs.randn(tuple(y.shape), 320 + b, torch.float32).to(dev))
        xs.append((0.3 * x0).to(F64))
        ops.append(op)
        covs.append(cov)
    return ops, covs, ys, xs


def _solve_both(S, opname, dev, sigma_t, max_rtol=1.0):
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda, solve_customcuda_batched
    ops, covs, ys, xs = _solver_case(S, opname, dev)
    assert len({float(c.C.D.sum()) for c in covs}) == len(covs)
    infos_b = []
    mats_b = solve_customcuda_batched(ops, ys, xs, covs, max_rtol, sigma_t, infos_b, exclusive=True)
    singles, infos_1 = [], []
    for b in range(len(ops)):
        info = []
        singles.append(solve_customcuda(ops[b], ys[b], xs[b], covs[b], max_rtol, sigma_t, info))
        infos_1.append(info[0])
    return mats_b, infos_b, singles, infos_1


@pytest.mark.parametrize("S", [128, 256])
@pytest.mark.parametrize("opname", ["gaussian_blur", "inpainting"])
def test_batched_cg_m0_distinct_diagonals_equals_single(dev, S, opname):
    """fh_cg_solve_batched at m = 0 with a different diagonal per image (S % 128 == 0: the symmetric DCT kernel with the
    diagonal covariance apply in its epilogue, `fh_diag_tab` indexed by plane / 3) against per-image fh_cg_solve: identical
    iteration counts and solutions to 1e-12, for the folded-blur path (gaussian_blur) and a non-folded operator; two noise
    levels (an un-converged solve at rtol 0.6 and a converged one)."""
    for sigma_t in (30.0, 0.4):
        mats_b, infos_b, singles, infos_1 = _solve_both(S, opname, dev, sigma_t)
        for b, one in enumerate(singles):
            assert infos_b[b]["niter"] == infos_1[b]["niter"], (sigma_t, b, infos_b[b], infos_1[b])
            assert maxabs(mats_b[b:b + 1], one) <= 1e-12 * float(one.abs().max()), (sigma_t, b)
        assert len({i["niter"] for i in infos_b}) > 1 or sigma_t < 1  # the images really are different systems


_NOSYM_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}, {gold!r}]
import test_timed_path as t
dev = torch.device("cuda:0")
out = {{}}
for opname in ("gaussian_blur", "inpainting"):
    mats_b, infos_b, _s, _i = t._solve_both(128, opname, dev, 80.0, 1e-10)
    out[opname] = mats_b.cpu().numpy()
    out[opname + "_niter"] = np.array([i["niter"] for i in infos_b])
np.savez(sys.argv[1], **out)
"""


def test_batched_cg_m0_symmetric_dct_equals_dense_passes(dev, tmp_path):
    """The same batched m = 0 solves with FH_DCT_NOSYM=1 (dense DCT GEMM passes, diagonal apply as its own kernel; the switch
    is read once per process, hence the child process), solved to rtol = 1e-10 (sigma_t = 80 with max_rtol = 1e-10) so that
    the solution is a property of the system: the two summation orders of the same products agree to 1e-9 of max|mat|
    (measured 5e-12 / 9e-11), iteration counts within 2 %."""
    path = str(tmp_path / "nosym.npz")
    src = _NOSYM_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), gold=os.path.join(ROOT, "tests", "golden"))
    env = dict(os.environ, FH_DCT_NOSYM="1")
    subprocess.run([sys.executable, "-c", src, path], check=True, env=env, timeout=600)
    ref = np.load(path)
    for opname in ("gaussian_blur", "inpainting"):
        mats_b, infos_b, _s, _i = _solve_both(128, opname, dev, 80.0, 1e-10)
        err = maxabs(mats_b, ref[opname]) / float(np.abs(ref[opname]).max())
        print("sym vs dense DCT passes", opname, "%.2e" % err, [i["niter"] for i in infos_b], list(ref[opname + "_niter"]), flush=True)
        assert err < 1e-9, (opname, err)
        assert all(abs(i["niter"] - int(n)) <= 0.02 * int(n) + 1 for i, n in zip(infos_b, ref[opname + "_niter"])), opname


# ---------------------------------------------------------------- batched covariance updates (one launch sequence for B images)
@pytest.mark.parametrize("S", [64, 100, 256])  # 100: d = 30000 = 39 * 768 + 48, no multiple of any kernel's row block
def test_batched_covariance_updates_equal_per_image_bitwise(dev, S):
    """fh_cov_time_update_batched / fh_cov_space_update_batched (the update kernels with the image as a grid dimension and
    per-image pointer tables) against the per-object update_time_step / update_space_step on three images with different
    data: after every update the four representations (D, r, inner matrix, factor base) of every image and the returned
    mean / score are BITWISE equal - the batched launch is the same arithmetic per image.  8 time + 8 space updates
    (m = 0 .. 16 columns), scripted vectors, shipped DCT prior."""
    import tempfile
    from free_hunch_amd import covariance as hc
    d, nimg, shape = 3 * S * S, 3, (1, 3, S, S)
    data = DATA
    if S != 256:
        data = tempfile.mkdtemp()
        torch.save(torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous(),
                   os.path.join(data, "dct_variance.pt"))
    mk = lambda b: hc.CovarianceHessianBFGSDCT(data, 80.0 ** 2, d, device=dev, use_precalculated_info=True, ctx_slot=b)  # noqa: E731
    single, batch = [mk(b) for b in range(nimg)], [mk(10 + b) for b in range(nimg)]
    scripts = [inputs.script(400 + b, shape, 8, 10.0, neg_gamma_at=3 if b == 1 else None, sig_end=1.0) for b in range(nimg)]
    assert hc.CovarianceHessianBFGS.can_batch(batch)

    def state(c):
        out = []
        for rep, fam in ((c.C, c.famC), (c.Ci, c.famC), (c.H, c.famH), (c.Hi, c.famH)):
            out += [rep.D, rep.r, rep.M_dev[: rep.m, : rep.m], fam.B[: fam.m]]
        return out

    for si in range(len(scripts[0])):
        what = scripts[0][si][0]
        args = [scripts[b][si][1] for b in range(nimg)]
        cat = lambda key: torch.cat([a[key] for a in args], 0).to(dev)  # noqa: E731
        if what == "time":
            ms, ss = zip(*[single[b].update_time_step(args[b]["x"].to(dev), args[b]["sigma"], args[b]["sigma_next"],
                                                      args[b]["score"].to(dev)) for b in range(nimg)])
            mb, sb = hc.CovarianceHessianBFGS.update_time_step_batched(batch, cat("x"), args[0]["sigma"], args[0]["sigma_next"],
                                                                       cat("score"))
            for b in range(nimg):
                assert torch.equal(ms[b], mb[b:b + 1]) and torch.equal(ss[b], sb[b:b + 1]), (si, b)
        else:
            for b in range(nimg):
                single[b].update_space_step(args[b]["m0"].to(dev), args[b]["m1"].to(dev), args[b]["sigma"], args[b]["x"].to(dev),
                                            args[b]["xn"].to(dev))
            hc.CovarianceHessianBFGS.update_space_step_batched(batch, cat("m0"), cat("m1"), args[0]["sigma"], cat("x"), cat("xn"))
        for b in range(nimg):
            assert single[b].k == batch[b].k and single[b].famC.m == batch[b].famC.m
            for i, (p, q) in enumerate(zip(state(single[b]), state(batch[b]))):
                assert torch.equal(p, q), (si, what, b, i)
    assert batch[0].famC.m == 16


def test_two_lockstep_groups_equal_one_group(dev):
    """bench.py's default launch: the 8 images of a GPU as TWO lock-step groups on two host threads / streams (the Free Hunch
    phase of one group overlaps the UNet phase of the other).  With the batch-invariant Gaussian-prior denoiser the two groups
    must reproduce the single-group run bit for bit: no scratch, context or graph cache is shared between groups."""
    import bench
    net = nets.gauss_net(256, dev)
    images = bench.smooth_images(8, 256, 7)
    outs = []
    for groups in (1, 2):
        outs.append(bench.run_batch(net, images, list(range(8)), "gaussian_blur", 6, "heun", dev, DATA, groups).cpu())
        torch.cuda.synchronize()
        if groups == 2:
            assert len(bench.run_batch.cg_iters) == 8
    assert torch.equal(outs[0], outs[1])
