"""Colorization (fh_problem.op = 3: one measurement plane per image, A = a weighted channel sum) and denoising (A = I)
through the Free Hunch solver on the device.

The oracle's `system()` knows four operator names, so A and A^T are written here in torch float64 and combined with the
oracle's covariance (`fo.make_covariance`), its `cg()` and the scripted updates of tests/golden/inputs.py.  Unequal channel
weights everywhere the default is not the point: equal weights would hide a channel permutation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import inputs
import nets
from test_hip_parity import T, _base_kwargs, maxabs

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "free-hunch_amd", "data")
W = (0.299, 0.587, 0.114)
SIGMA_S = 0.05


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _wt(like):
    return torch.tensor(W, dtype=F64, device=like.device).view(1, 3, 1, 1)


def A(x):
    """[N,3,S,S] -> [N,1,S,S] in torch float64"""
    return (x.to(F64) * _wt(x)).sum(1, keepdim=True)


def At(u):
    """[N,1,S,S] -> [N,3,S,S] in torch float64"""
    return u.to(F64) * _wt(u)


def _col_op(S, dev, slot=0, weights=W):
    from free_hunch_amd.measurements import get_operator
    op = get_operator(name="colorization", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), channel_weights=weights)
    op.ctx_slot = slot
    return op


def _run_script(cov, steps, dev=None):
    for what, a in steps:
        to = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
        if what == "time":
            cov.update_time_step(to(a["x"]), a["sigma"], a["sigma_next"], to(a["score"]))
        else:
            cov.update_space_step(to(a["m0"]), to(a["m1"]), a["sigma"], to(a["x"]), to(a["xn"]))


def _cov_pair(kind, S, tmp, dev, gold, n_script, seed=1200):
    """(oracle covariance, device covariance) after the same `2 * n_script` scripted updates (0: the initial state)."""
    from oracle import fh_oracle as fo
    from free_hunch_amd import covariance as hc
    d = 3 * S * S
    if kind == "dct_diagonal":
        torch.save(T(gold("solver")["dct_variance64"]), os.path.join(tmp, "dct_variance.pt"))
        hip = hc.CovarianceHessianBFGSDCT(tmp, 80.0 ** 2, d, device=dev, use_precalculated_info=True)
    else:
        hip = hc.CovarianceHessianBFGS(1, 80.0 ** 2, d, device=dev)
    orc = fo.make_covariance(kind, tmp, 80.0 ** 2, d)
    if n_script:
        steps = inputs.script(seed, (1, 3, S, S), n_script, 80.0)
        _run_script(orc, steps)
        _run_script(hip, steps, dev)
        assert hip.k == orc.k and hip.famC.m == 2 * n_script
    return orc, hip


def _amm(cov, prob, u):
    from free_hunch_amd import _lib
    out = torch.empty_like(u)
    _lib.check(cov.ctx.lib.fh_amm(cov.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), _lib.stream()), "fh_amm")
    return out


def _oracle_amm(orc, s2):
    def A_mm(u):
        S = int(round(u.numel() ** 0.5))
        u4 = u.reshape(1, 1, S, S)
        return (s2 * u4 + A(orc.denoiser_cov_vector_dot(At(u4)))).flatten()
    return A_mm


# ---------------------------------------------------------------- 1. the channel-mix kernel
@pytest.mark.parametrize("nimg", [1, 4])
@pytest.mark.parametrize("S", [64, 256])
def test_channel_mix_vs_torch_f64(dev, S, nimg):
    """fh_channel_mix forward and adjoint against torch float64 (1e-14 relative) and <A x, v> = <x, A^T v> on the same
    inputs (1e-12 relative, the form of test_operator_adjoint_identity_f64)."""
    from free_hunch_amd import _lib
    ctx = _lib.Context.get(S, 3, 0)
    w = torch.tensor(W, dtype=F64, device=dev)
    x = inputs.randn((nimg, 3, S, S), 11 + S + nimg).to(dev)
    v = inputs.randn((nimg, 1, S, S), 12 + S + nimg).to(dev)
    ax = ctx.channel_mix(x, torch.empty(nimg, 1, S, S, dtype=F64, device=dev), w, adjoint=False)
    atv = ctx.channel_mix(v, torch.empty(nimg, 3, S, S, dtype=F64, device=dev), w, adjoint=True)
    ref_f, ref_a = A(x), At(v)
    e_f = maxabs(ax, ref_f) / float(ref_f.abs().max())
    e_a = maxabs(atv, ref_a) / float(ref_a.abs().max())
    lhs, rhs = float((ax * v).sum()), float((x * atv).sum())
    print(f"channel_mix S={S} nimg={nimg}: forward {e_f:.2e} adjoint {e_a:.2e} identity {abs(lhs - rhs) / max(1.0, abs(lhs)):.2e}",
          flush=True)
    assert e_f <= 1e-14 and e_a <= 1e-14
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_operator_class_runs_the_kernel(dev):
    """ColorizationOperator: shapes, dtype round trip, noise level and the default weights = the reference's mean(dim=1)."""
    S = 64
    x = inputs.smooth_image(S, 3).to(dev)
    op = _col_op(S, dev)
    y = op.forward(x, noiseless=True)
    assert tuple(y.shape) == (1, 1, S, S) and y.dtype == x.dtype
    assert maxabs(y, A(x)) < 1e-6
    for back in (op.transpose(y), op.forward_adjoint(y)):
        assert tuple(back.shape) == (1, 3, S, S) and maxabs(back, At(y)) < 1e-6
    y2, flat = op.forward(x, flatten=True, noiseless=True)
    assert tuple(flat.shape) == (1, S * S)
    assert abs(float((op.forward(x) - y).std()) - SIGMA_S) < 0.1 * SIGMA_S
    mean_op = _col_op(S, dev, weights=None)
    assert maxabs(mean_op.forward(x, noiseless=True), x.mean(dim=1, keepdim=True)) < 1e-6


# ---------------------------------------------------------------- 2. one application of A_mm
@pytest.mark.parametrize("kind,S,n_script", [("dct_diagonal", 64, 0), ("dct_diagonal", 64, 4), ("identity", 16, 0),
                                             ("identity", 16, 4)])
def test_amm_colorization_vs_oracle_covariance(dev, gold, tmp_path, kind, S, n_script):
    """fh_amm with op = 3 against sigma_y^2 u + A (C (A^T u)), C = the oracle covariance's denoiser_cov_vector_dot, before any
    update (m = 0) and after 8 scripted updates (4 time + 4 space, m = 8): 1e-8 relative, the bound test_covariance_vs_oracle
    holds the apply to; symmetry <u, A_mm v> = <A_mm u, v> to 1e-9 as in test_cg_full_size_residual_property."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    orc, hip = _cov_pair(kind, S, str(tmp_path), dev, gold, n_script)
    op = _col_op(S, dev)
    s2 = _sigma_y2(op)
    prob, keep = _problem(op, hip, s2)
    assert prob.op == 3 and prob.ntaps == 3 and prob.m == 2 * n_script and prob.use_dct == int(kind != "identity")
    u = inputs.randn((1, 1, S, S), 21).to(dev)
    v = inputs.randn((1, 1, S, S), 22).to(dev)
    au, av = _amm(hip, prob, u), _amm(hip, prob, v)
    ref = _oracle_amm(orc, s2)(u.cpu().flatten()).reshape(1, 1, S, S)
    err = maxabs(au, ref) / float(ref.abs().max())
    l, r = float((u * av).sum()), float((au * v).sum())
    print(f"amm op=3 {kind} S={S} m={prob.m}: {err:.2e}, symmetry {abs(l - r) / max(abs(l), 1.0):.2e}", flush=True)
    assert err <= 1e-8
    assert abs(l - r) <= 1e-9 * max(abs(l), 1.0)


@pytest.mark.parametrize("n_script", [0, 2])
def test_amm_colorization_one_plane_route_equals_three_plane_route_256(dev, n_script):
    """At 256 x 256 with the shipped prior the one-plane route (symmetric DCT kernel on one plane per image; at m = 0 the
    diagonal D_eff = sum_c w_c^2 D_c in its epilogue) against the same product assembled from the three-plane pieces that
    the other operators use: A^T in torch, the device covariance's own dct2 / apply / idct2 over three planes, A in torch.
    Both sides are float64 sums of the same products in different orders: 1e-12 of max|ref| leaves four decimal orders above
    the unit roundoff for the two 256-term DCT sums and the prior's dynamic range."""
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 256
    cov = hc.CovarianceHessianBFGSDCT(DATA, 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True)
    if n_script:
        _run_script(cov, inputs.script(700, (1, 3, S, S), n_script, 10.0, sig_end=1.0), dev)
    op = _col_op(S, dev)
    s2 = _sigma_y2(op)
    prob, keep = _problem(op, cov, s2)
    assert prob.m == 2 * n_script
    u = inputs.randn((1, 1, S, S), 23).to(dev)
    got = _amm(cov, prob, u)
    ref = s2 * u + A(cov.denoiser_cov_vector_dot(At(u).contiguous()))
    err = maxabs(got, ref) / float(ref.abs().max())
    print(f"amm op=3 S=256 m={prob.m}: one-plane vs three-plane route {err:.2e}", flush=True)
    assert err <= 1e-12


# ---------------------------------------------------------------- 3. the solve against the oracle's cg()
@pytest.mark.parametrize("n_script", [4, 0])
def test_solve_colorization_vs_oracle_cg(dev, gold, tmp_path, n_script):
    """solve_customcuda on the colorization system against fo.cg on the same system written in torch (64 x 64, golden DCT
    prior, weights 0.299 / 0.587 / 0.114, sigma_s = 0.05): after six iterations on both sides mat agrees to 1e-5 (the `short`
    bound of the teacher-forced trajectory tests); at rtol = 1e-6 the oracle reports `optimal` and the device solution's true
    residual, recomputed with an independent fh_amm, is <= 1.05 rtol ||b||."""
    from oracle import fh_oracle as fo
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda
    S = 64
    orc, hip = _cov_pair("dct_diagonal", S, str(tmp_path), dev, gold, n_script)
    op = _col_op(S, dev)
    s2 = _sigma_y2(op)
    x_true = inputs.smooth_image(S, 31).to(F64)
    y = A(x_true) + SIGMA_S * inputs.randn((1, 1, S, S), 32)
    x0_mean = x_true + 0.05 * inputs.randn((1, 3, S, S), 33)
    A_mm = _oracle_amm(orc, s2)
    b = (y - A(x0_mean)).flatten()
    # six iterations on both sides
    m6h = solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, rtol=1e-300, maxiter=6)
    sol6, info6 = fo.cg(A_mm, b, rtol=0.0, maxiter=6)
    m6o = At(sol6.reshape(1, 1, S, S))
    short = maxabs(m6o, m6h) / float(m6o.abs().max())
    assert info6["niter"] == 6 and tuple(m6h.shape) == (1, 3, S, S)
    # converged solve
    rtol = 1e-6
    _sol, info_o = fo.cg(A_mm, b, rtol=rtol)
    info_h = []
    solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, info_h, rtol=rtol)
    u_h = solve_customcuda.last_solution.clone()
    assert tuple(u_h.shape) == (1, 1, S, S)
    prob, keep = _problem(op, hip, s2)
    bd = b.reshape(1, 1, S, S).to(dev)
    res = float((bd - _amm(hip, prob, u_h)).norm())
    print(f"colorization solve m={2 * n_script}: short {short:.2e}; rtol 1e-6: oracle {info_o['niter']} it, device "
          f"{info_h[0]['niter']} it, true residual {res / float(bd.norm()):.3e} ||b||", flush=True)
    assert short <= 1e-5
    assert info_o["optimal"], info_o  # the system itself is sound: the reference's cg() converges on it
    assert info_h[0]["optimal"] and 1 <= info_h[0]["niter"] < 5000
    assert res <= 1.05 * rtol * float(bd.norm())


# ---------------------------------------------------------------- 4. batched solve = single solves
def _batch_case(S, dev, n_script, nimg=4):
    """nimg colorization systems with distinct covariance states.  Image 0's right-hand side is constant over the plane:
    without factor columns that is an eigenvector of A C A^T (the DC coefficient) and with a few columns close to one, so
    its CG stops after one iteration while the other images run on - the per-image `done` skip of every kernel in the loop is exercised."""
    import tempfile
    from free_hunch_amd import covariance as hc
    d = 3 * S * S
    data = DATA
    if S != 256:
        data = tempfile.mkdtemp()
        dv = torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
        torch.save(dv, os.path.join(data, "dct_variance.pt"))
    ops, covs, ys, xs = [], [], [], []
    for b in range(nimg):
        op = _col_op(S, dev, slot=b)
        cov = hc.CovarianceHessianBFGSDCT(data, 80.0 ** 2, d, device=dev, use_precalculated_info=True, ctx_slot=b)
        if n_script:
            _run_script(cov, inputs.script(500 + b, (1, 3, S, S), n_script, 10.0, sig_end=1.0), dev)
        else:  # one time update each: distinct diagonals, no factor columns
            x = inputs.randn((1, 3, S, S), 300 + b).to(dev) * 40.0
            cov.update_time_step(x, 80.0, [40.0, 25.0, 12.0, 30.0][b % 4], -x / 80.0 ** 2 * 0.5)
        x0 = inputs.smooth_image(S, 310 + b).to(dev)
        if b == 0:
            ys.append(torch.full((1, 1, S, S), 0.5, dtype=torch.float32, device=dev))
            xs.append(torch.zeros(1, 3, S, S, dtype=F64, device=dev))
        else:
            ys.append(op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 1, S, S), 320 + b, torch.float32).to(dev))
            xs.append((0.3 * x0).to(F64))
        ops.append(op)
        covs.append(cov)
    return ops, covs, ys, xs


@pytest.mark.parametrize("S,n_script", [(256, 0), (256, 2), (64, 0)])
def test_batched_colorization_solve_equals_single(dev, S, n_script):
    """fh_cg_solve_batched with op = 3 for 4 images against four fh_cg_solve calls, by the rule of
    test_batched_cg_m0_distinct_diagonals_equals_single: identical iteration counts, solutions to 1e-12 of max|mat|.
    S = 256: the symmetric DCT kernel on one plane per image (m = 0 with D_eff in its epilogue; m = 4 with the broadcast /
    apply / reduce kernels between the passes); S = 64: the dense DCT passes."""
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda, solve_customcuda_batched
    ops, covs, ys, xs = _batch_case(S, dev, n_script)
    assert all(c.famC.m == 2 * n_script for c in covs)
    # the images really are different systems: distinct diagonals (m = 0) / distinct factor bases (the scripted updates
    # shift every diagonal by the same amounts and differ in the appended columns)
    distinct = {float(c.famC.B[: c.famC.m].sum()) if n_script else float(c.C.D.sum()) for c in covs}
    assert len(distinct) == len(covs)
    sigma_t = 0.4  # rtol_func(0.4) = 9e-3
    infos_b = []
    mats_b = solve_customcuda_batched(ops, ys, xs, covs, 1.0, sigma_t, infos_b, exclusive=True)
    assert tuple(mats_b.shape) == (4, 3, S, S)
    n_b = [i["niter"] for i in infos_b]
    for b in range(4):
        info = []
        one = solve_customcuda(ops[b], ys[b], xs[b], covs[b], 1.0, sigma_t, info)
        assert infos_b[b]["niter"] == info[0]["niter"], (b, n_b, info[0])
        assert infos_b[b]["optimal"] and info[0]["optimal"]
        assert maxabs(mats_b[b:b + 1], one) <= 1e-12 * float(one.abs().max()), b
    print(f"batched colorization S={S} m={2 * n_script}: iterations {n_b}", flush=True)
    assert n_b[0] + 3 <= min(n_b[1:]), n_b  # image 0 finished several iterations before the others: the `done` skip ran


# ---------------------------------------------------------------- 5. denoising = inpainting with an all-ones mask
def test_noise_solve_equals_inpainting_with_ones_mask_bitwise(dev, gold, tmp_path):
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda
    from free_hunch_amd.measurements import get_operator
    S = 64
    _orc, hip = _cov_pair("dct_diagonal", S, str(tmp_path), dev, gold, 2)
    noise_op = get_operator(name="noise", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S))
    inp_op = get_operator(name="inpainting", device=dev, sigma_s=SIGMA_S, mask=torch.ones(1, 3, S, S),
                          mask_opt={"mask_type": "random", "mask_prob_range": (0.1, 0.3), "image_size": S})
    assert _problem(noise_op, hip, _sigma_y2(noise_op))[0].op == 0
    x_true = inputs.smooth_image(S, 41).to(dev)
    y = noise_op.forward(x_true, noiseless=True) + SIGMA_S * inputs.randn((1, 3, S, S), 42, torch.float32).to(dev)
    x0_mean = (x_true + 0.05 * inputs.randn((1, 3, S, S), 43, torch.float32).to(dev)).to(F64)
    i_n, i_i = [], []
    m_n = solve_customcuda(noise_op, y, x0_mean, hip, 1.0, 0.4, i_n)
    m_i = solve_customcuda(inp_op, y, x0_mean, hip, 1.0, 0.4, i_i)
    assert i_n[0]["niter"] == i_i[0]["niter"] >= 1 and i_n[0]["optimal"]
    assert torch.equal(m_n, m_i)
    assert tuple(noise_op.forward(x_true).shape) == (1, 3, S, S)
    assert abs(float((noise_op.forward(x_true) - x_true).std()) - SIGMA_S) < 0.1 * SIGMA_S


# ---------------------------------------------------------------- 6. the comparison methods
def _torch_baseline(name, x_t, sigma, y, s2, lam=10.0):
    """One guidance call of the mechanism with torch float64 operators and the Gaussian-prior denoiser.  A A^T = q I
    (q = sum_c w_c^2) and the variance is constant over the image, so every method's linear solve has a closed form."""
    q = float(sum(w * w for w in W))
    x_t = x_t.detach().clone().requires_grad_()
    x0 = inputs.gauss_prior_denoise(x_t, sigma)
    s_2 = sigma ** 2
    if name == "dps":
        (g,) = torch.autograd.grad(-torch.linalg.norm(y.to(F64) - A(x0)), x_t)
        return (x0 + g * s_2).detach()
    if name == "diffpir":
        var = s_2 / lam
        mat = At((y.to(F64) - A(x0.detach())) / (var * q + s2))
        return (x0 + mat * var).detach()
    if name == "pigdm":
        var = s_2 / (1 + s_2)
    else:  # tmpd: row sums of the denoiser's Jacobian times sigma^2 - here a constant field
        (jr,) = torch.autograd.grad(x0.sum(), x_t, retain_graph=True)
        var = float((jr * s_2).flatten()[0])
        assert float((jr * s_2 - var).abs().max()) == 0.0
    mat = At((y.to(F64) - A(x0.detach())) / (var * q + s2))
    (g,) = torch.autograd.grad((mat * x0).sum(), x_t)
    return (x0 + g * s_2).detach()


@pytest.mark.parametrize("name", ["pigdm", "tmpd", "diffpir", "dps"])
def test_baselines_run_on_colorization(dev, name):
    """One guidance call of each comparison method with the colorization operator and the Gaussian-prior denoiser of
    tests/nets.py, against the same method in torch float64: within 5e-4 of max(1, max|ref|), the per-call bound of
    test_baseline_calls_teacher_forced_vs_oracle."""
    from free_hunch_amd.conditioning_mechanisms import _sigma_y2, choose_conditioning_mechanism
    S, sigma = 64, 2.0
    net = nets.gauss_net(S, dev)
    op = _col_op(S, dev)
    mech = choose_conditioning_mechanism(name)(1.0, op, False, init_denoiser_variance=1, init_noise_variance=80.0 ** 2,
                                               data_dim=3 * S * S, pigdm_posthoc_scaling=False, max_rtol=1.0,
                                               diffpir_lambda=10.0)
    x_true = inputs.smooth_image(S, 51).to(dev)
    y = op.forward(x_true, noiseless=True) + SIGMA_S * inputs.randn((1, 1, S, S), 52, torch.float32).to(dev)
    x_t = (x_true.to(F64) + sigma * inputs.randn((1, 3, S, S), 53).to(dev))
    sig = torch.tensor(sigma, dtype=F64, device=dev)
    out = mech(x_t.clone(), net, y, sig).detach()
    ref = _torch_baseline(name, x_t, sig, y, _sigma_y2(op))
    err = maxabs(out, ref) / max(1.0, float(ref.abs().max()))
    moved = maxabs(ref, inputs.gauss_prior_denoise(x_t, sig))
    print(f"{name} on colorization: {err:.2e} (guidance moved the estimate by {moved:.2e})", flush=True)
    assert tuple(out.shape) == (1, 3, S, S) and moved > 1e-3
    assert err < 5e-4, err


# ---------------------------------------------------------------- 7. the lock-step sampler
def test_lockstep_colorization_equals_per_image_and_is_consistent(dev, gold, tmp_path):
    """conditional_sampler_grouped(groups = 1) over 4 colorization images against per-image conditional_sampler runs by the
    rule of test_batched_equals_per_image (identical niter and k lists, outputs within 1e-3), with the batch-invariant
    Gaussian-prior denoiser; and measurement consistency: rms(A x - y) of the guided run is below that of the same run with
    cond_scaling = 0 on the same noise."""
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_grouped
    B, S = 4, 64
    torch.save(torch.from_numpy(gold("trajectories")["dct_variance64"]), tmp_path / "dct_variance.pt")
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(tmp_path, {})
    ops, ys, noise = [], [], []
    for b in range(B):
        op = _col_op(S, dev, slot=b)
        ops.append(op)
        x0 = 0.5 * inputs.smooth_image(S, 70 + b).to(dev)
        ys.append(op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 1, S, S), 80 + b, torch.float32).to(dev))
        noise.append(inputs.randn((1, 3, S, S), 90 + b, torch.float32))
    noise = torch.cat(noise).to(dev)
    run = dict(num_steps=6, sigma_min=0.002, sigma_max=80, rho=7, solver="heun")
    xb = conditional_sampler_grouped(net, noise, ys, ops, groups=1, **run, **kw)
    torch.cuda.synchronize()
    tb = [m.trace for m in conditional_sampler_grouped.last_mechanisms]
    assert tuple(xb.shape) == (B, 3, S, S)
    for b in range(B):
        x1, _, _ = conditional_sampler(net, noise[b:b + 1], None, None, measurement=ys[b], operator=ops[b], **run, **kw)
        t1 = conditional_sampler.last_mechanism.trace
        assert [t["niter"] for t in t1] == [t["niter"] for t in tb[b]], b
        assert [t["k"] for t in t1] == [t["k"] for t in tb[b]], b
        assert float((x1 - xb[b:b + 1]).abs().max()) < 1e-3
    x_free = conditional_sampler_grouped(net, noise, ys, ops, groups=1, **run, **dict(kw, cond_scaling=0.0))
    torch.cuda.synchronize()
    y_all = torch.cat(ys).to(F64)
    rms = lambda x: float((A(x) - y_all).pow(2).mean().sqrt())  # noqa: E731
    print(f"lock-step colorization: rms(A x - y) guided {rms(xb):.4f}, unguided {rms(x_free):.4f}; iterations "
          f"{[t['niter'] for t in tb[0]]}", flush=True)
    assert rms(xb) < rms(x_free)


# ---------------------------------------------------------------- 8. the CLI
def test_cli_colorization_and_noise(tmp_path):
    import PIL.Image
    sys.path.insert(0, ROOT)
    from bench import smooth_images
    import generate_conditional as gc
    data = tmp_path / "data"
    data.mkdir()
    for i, im in enumerate(smooth_images(2, 256, 7)):
        PIL.Image.fromarray(im.permute(1, 2, 0).numpy(), "RGB").save(data / f"img{i:08d}.png")
    common = [f"--dataset_path={data}", "--synthetic_weights=ffhq", "--num_steps=3", "--solver=euler", "--total_images=2",
              "--max_batch_size=2"]
    names = ["000000_000000.png", "000001_000000.png"]
    for sub, extra, mode in (("col", ["--operator_name=colorization", "--conditioning_mechanism=online_covariance",
                                      "--image_base_covariance=dct_diagonal"], "L"),
                             ("noise", ["--operator_name=noise", "--conditioning_mechanism=dps"], "RGB")):
        out = tmp_path / sub
        gc.main([f"--outdir={out}"] + common + extra)
        for folder in ("images", "cond_images", "forward_images"):
            assert sorted(os.listdir(out / folder)) == names, (sub, folder)
        for n in names:
            im = PIL.Image.open(out / "images" / n)
            assert im.mode == "RGB" and im.size == (256, 256) and np.asarray(im).std() > 0
            fw = PIL.Image.open(out / "forward_images" / n)
            assert fw.mode == mode and fw.size == (256, 256) and np.asarray(fw).std() > 0
        txt = open(out / "results.txt").read()
        assert "PSNR" in txt and "SSIM" in txt


# ---------------------------------------------------------------- 9. unknown operator codes
def test_amm_rejects_unknown_op_without_launching(dev, gold, tmp_path):
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 64
    _orc, hip = _cov_pair("dct_diagonal", S, str(tmp_path), dev, gold, 0)
    op = _col_op(S, dev)
    prob, keep = _problem(op, hip, _sigma_y2(op))
    u = inputs.randn((1, 3, S, S), 61).to(dev)
    out = torch.full_like(u, 123.0)
    info = _lib.FhCgInfo()
    for code in (7, -1, 4):
        prob.op = code
        rc = hip.ctx.lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), _lib.stream())
        assert rc < 0, (code, rc)
        rc = hip.ctx.lib.fh_cg_solve(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), 1e-3, 0.0, 10, C.byref(info),
                                     _lib.stream())
        assert rc < 0, (code, rc)
    # op = 3 reads and writes 16 bytes at a time: a measurement buffer that is only 8-byte aligned is refused as well
    prob.op = 3
    rc = hip.ctx.lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr() + 8, out.data_ptr(), _lib.stream())
    assert rc < 0, rc
    rc = hip.ctx.lib.fh_cg_solve(hip.ctx.h, C.byref(prob), u.data_ptr() + 8, out.data_ptr(), 1e-3, 0.0, 10, C.byref(info),
                                 _lib.stream())
    assert rc < 0, rc
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())  # nothing was launched
