"""User-supplied PSFs on the device: the dense-window convolution (fh_conv_window, fh_problem.op = 4) from the kernel up to the
CLI, and a separable custom PSF on the route of the shipped Gaussian.

The oracle's `system()` takes any PSF under the name "gaussian_blur"; `otf_double=True` makes its FFT blur the exact circular
convolution with the float32 taps, which is what the kernels compute."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import inputs
import nets
from test_channel_ops_gpu import _amm, _cov_pair, _run_script
from test_custom_psf_host import disk_psf
from test_hip_parity import _base_kwargs, maxabs

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "free-hunch_amd", "data")
SIGMA_S = 0.05


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _disk_op(S, dev, slot=0):
    from free_hunch_amd.measurements import get_operator
    op = get_operator(name="custom_blur", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), kernel=disk_psf())
    op.ctx_slot = slot
    return op


def _oracle_op(S, psf=None):
    from oracle import fh_oracle as fo
    return fo.OracleOperator("gaussian_blur", (1, 3, S, S), SIGMA_S, kernel=disk_psf() if psf is None else psf, otf_double=True)


# ---------------------------------------------------------------- 1. the kernel against the defining sums
def _window(kh, kw, zero, seed):
    """Random non-symmetric kh x kw PSF about its centre at (kh // 2, kw // 2) as a [2hy+1][2hx+1] window (float64)."""
    rng = np.random.default_rng(seed)
    k = rng.standard_normal((kh, kw)) * (rng.random((kh, kw)) >= zero)
    k[0, 0], k[-1, -1] = 0.7, -0.4  # the full extent is always populated
    cy, cx = kh // 2, kw // 2
    hy, hx = max(cy, kh - 1 - cy), max(cx, kw - 1 - cx)
    win = np.zeros((2 * hy + 1, 2 * hx + 1))
    win[hy - cy: hy - cy + kh, hx - cx: hx - cx + kw] = k
    return win, hy, hx


def _direct_sums(x, win, hy, hx, adjoint):
    """out[p][i][j] = sum_{a,b} win[a+hy][b+hx] x[p][(i -+ a) mod S][(j -+ b) mod S] in float64: the sum over b of one window row
    is the product with the S x S circulant of that row (its entries are the row's weights, summed where 2 hx + 1 > S wraps
    two taps onto one sample), the sum over a adds the 2 hy + 1 row-shifted products."""
    S = x.shape[-1]
    sgn = 1 if adjoint else -1
    j = np.arange(S)
    out = np.zeros_like(x)
    for a in range(-hy, hy + 1):
        circ = np.zeros((S, S))  # circ[j'][j] = sum_b w[b] [j' = (j + sgn b) mod S]
        for b in range(-hx, hx + 1):
            np.add.at(circ, ((j + sgn * b) % S, j), win[a + hy, b + hx])
        out += np.roll(x, -sgn * a, axis=1) @ circ
    return out


def _run_window(ctx, xd, wd, hy, hx, adjoint):
    out = torch.full_like(xd, float("nan"))
    ctx.conv_window(xd, out, (wd, hy, hx), xd.shape[0], adjoint)
    return out


@pytest.mark.parametrize("S,kh,kw,zero,planes", [
    (64, 61, 61, 0.0, 3),   # the shipped PSFs' size, dense: 3721 taps, one tile row of two tiles
    (96, 65, 65, 0.3, 3),   # the largest window (137 KiB of LDS), partial tiles in both directions, zeros inside
    (64, 60, 34, 0.0, 3),   # even sizes: unequal sides about the centre
    (48, 9, 33, 0.0, 3),    # image smaller than the 64-row tile; a last tap block of one tap
    (64, 1, 1, 0.0, 3),     # no halo at all
    (256, 61, 61, 0.0, 6),  # 8 x 4 tiles, two images' planes
    # sides that are no multiple of 16 (the table of tests/test_ragged_sizes_gpu.py)
    (100, 61, 61, 0.0, 3),  # S % 8 = 4: the last tile column has 4 live outputs of a thread's 8, the last tile row 36 of 64
    (250, 9, 33, 0.0, 3),   # S = 2 mod 4, 250 = 7 * 32 + 26 = 3 * 64 + 58
    (20, 65, 65, 0.3, 3),   # a window larger than the image: every staged row and column wraps more than once
    (6, 1, 1, 0.0, 3),      # an image smaller than a thread's 8 outputs
])
def test_conv_window_matches_the_direct_sums(dev, S, kh, kw, zero, planes):
    """fh_conv_window forward and adjoint against the defining circular sums in NumPy float64, at the bounds
    test_conv_circ_matches_a_direct_sum holds the tap-list kernels to: 1e-12 max(1, max|ref|) per output and
    <A x, v> = <x, A^T v> to 1e-10.  Float64 sums of these windows in different orders differ by at most 6.1e-15 max|ref|."""
    from free_hunch_amd import _lib
    win, hy, hx = _window(kh, kw, zero, S * 131 + kh * 17 + kw)
    rng = np.random.default_rng(S + kh)
    x, v = rng.standard_normal((planes, S, S)), rng.standard_normal((planes, S, S))
    ctx = _lib.Context.get(S, planes, 0)
    xd, vd, wd = (torch.from_numpy(t).to(dev) for t in (x, v, win))
    got_f, got_a = _run_window(ctx, xd, wd, hy, hx, False), _run_window(ctx, vd, wd, hy, hx, True)
    torch.cuda.synchronize()
    ref_f, ref_a = _direct_sums(x, win, hy, hx, False), _direct_sums(v, win, hy, hx, True)
    e_f, e_a = np.abs(got_f.cpu().numpy() - ref_f).max(), np.abs(got_a.cpu().numpy() - ref_a).max()
    lhs, rhs = float((got_f * vd).sum()), float((xd * got_a).sum())
    print(f"conv_window S={S} {kh}x{kw} planes={planes}: forward {e_f / max(1.0, np.abs(ref_f).max()):.2e} adjoint "
          f"{e_a / max(1.0, np.abs(ref_a).max()):.2e} identity {abs(lhs - rhs) / max(1.0, abs(lhs)):.2e}", flush=True)
    assert e_f < 1e-12 * max(1.0, np.abs(ref_f).max())  # (a NaN left in `out` fails both)
    assert e_a < 1e-12 * max(1.0, np.abs(ref_a).max())
    assert abs(lhs - rhs) < 1e-10 * max(1.0, abs(lhs))


# ---------------------------------------------------------------- 2. one fma chain per output
def test_conv_window_planes_do_not_depend_on_the_plane_count(dev):
    from free_hunch_amd import _lib
    S = 96
    win, hy, hx = _window(61, 61, 0.0, 3)
    x = np.random.default_rng(4).standard_normal((3, S, S))
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(win).to(dev)
    x12 = xd.repeat(4, 1, 1).contiguous()
    for adjoint in (False, True):
        o3 = _run_window(_lib.Context.get(S, 3, 0), xd, wd, hy, hx, adjoint)
        o12 = _run_window(_lib.Context.get(S, 12, 0), x12, wd, hy, hx, adjoint)
        for rep in range(4):
            assert torch.equal(o12[3 * rep: 3 * rep + 3], o3), (adjoint, rep)


def test_conv_window_rejects_bad_arguments(dev):
    from free_hunch_amd import _lib
    S = 64
    ctx = _lib.Context.get(S, 3, 0)
    x = torch.zeros(3, S, S, dtype=F64, device=dev)
    out = torch.full_like(x, 123.0)
    w = torch.ones(7, 7, dtype=F64, device=dev)
    call = lambda *a: ctx.lib.fh_conv_window(*a, _lib.stream())  # noqa: E731
    p = lambda t: t.data_ptr()  # noqa: E731
    assert call(None, p(x), p(out), p(w), 3, 3, 3, 0) == _lib.FH_EINVAL
    assert call(ctx.h, None, p(out), p(w), 3, 3, 3, 0) == _lib.FH_EINVAL
    assert call(ctx.h, p(x), None, p(w), 3, 3, 3, 0) == _lib.FH_EINVAL
    assert call(ctx.h, p(x), p(out), None, 3, 3, 3, 0) == _lib.FH_EINVAL
    assert call(ctx.h, p(out), p(out), p(w), 3, 3, 3, 0) == _lib.FH_EINVAL
    for hy, hx, planes in ((33, 3, 3), (3, 33, 3), (-1, 3, 3), (3, -1, 3), (3, 3, 0)):
        assert call(ctx.h, p(x), p(out), p(w), hy, hx, planes, 0) == _lib.FH_EINVAL, (hy, hx, planes)
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())  # nothing was launched


# ---------------------------------------------------------------- 3. one application of A_mm
@pytest.mark.parametrize("kind,n_script", [("dct_diagonal", 0), ("dct_diagonal", 4), ("identity", 0), ("identity", 4)])
def test_amm_window_vs_oracle_covariance(dev, gold, tmp_path, kind, n_script):
    """fh_amm with op = 4 (disk PSF, 64 x 64) against sigma_y^2 u + A C A^T u from the oracle's covariance and its FFT blur with
    a complex128 OTF, before any update (m = 0) and after 8 scripted updates (m = 8): 1e-8 relative and symmetry to 1e-9, the
    bounds of test_amm_colorization_vs_oracle_covariance."""
    from oracle import fh_oracle as fo
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 64
    orc, hip = _cov_pair(kind, S, str(tmp_path), dev, gold, n_script)
    op = _disk_op(S, dev)
    s2 = _sigma_y2(op)
    prob, keep = _problem(op, hip, s2)
    assert prob.op == 4 and prob.ntaps == 41 * 41 and prob.halo == 64 * 20 + 20 and prob.stride == 1 and prob.ntaps2 == 0
    assert prob.m == 2 * n_script and prob.use_dct == int(kind != "identity")
    assert not (prob.tap_dy or prob.tap_dx or prob.tap2_w or prob.fold_fwd_w)
    oop = _oracle_op(S)
    x = inputs.smooth_image(S, 3).to(F64)
    y = oop.forward(x)
    A_mm, _b, _back, _shape = fo.system(oop, y, x, orc)
    u = inputs.randn((1, 3, S, S), 21).to(dev)
    v = inputs.randn((1, 3, S, S), 22).to(dev)
    au, av = _amm(hip, prob, u), _amm(hip, prob, v)
    ref = A_mm(u.cpu().flatten()).reshape(1, 3, S, S)
    err = maxabs(au, ref) / float(ref.abs().max())
    l, r = float((u * av).sum()), float((au * v).sum())
    print(f"amm op=4 {kind} m={prob.m}: {err:.2e}, symmetry {abs(l - r) / max(abs(l), 1.0):.2e}", flush=True)
    assert err <= 1e-8
    assert abs(l - r) <= 1e-9 * max(abs(l), 1.0)


def test_amm_refuses_inconsistent_window_fields_without_launching(dev, gold, tmp_path):
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 64
    _orc, hip = _cov_pair("dct_diagonal", S, str(tmp_path), dev, gold, 0)
    op = _disk_op(S, dev)
    u = inputs.randn((1, 3, S, S), 61).to(dev)
    out = torch.full_like(u, 123.0)
    info = _lib.FhCgInfo()
    some = u.data_ptr()
    for field, value in (("ntaps", 41 * 41 - 1), ("halo", 64 * 20 + 19), ("halo", 64 * 33 + 20), ("halo", -1), ("stride", 2),
                         ("tap_w", None), ("tap_dy", some), ("tap_dx", some), ("ntaps2", 1), ("tap2_dy", some), ("tap2_dx", some),
                         ("tap2_w", some), ("fold_fwd_w", some), ("fold_fwd_h", some), ("fold_inv_w", some), ("fold_inv_h", some)):
        prob, keep = _problem(op, hip, _sigma_y2(op))
        setattr(prob, field, value)
        rc = hip.ctx.lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
        rc = hip.ctx.lib.fh_cg_solve(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), 1e-3, 0.0, 10, C.byref(info),
                                     _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())  # nothing was launched


# ---------------------------------------------------------------- 4. the solve against the oracle's cg()
@pytest.mark.parametrize("kind", ["dct_diagonal", "identity"])
def test_solve_window_vs_oracle_cg(dev, gold, tmp_path, kind):
    """solve_customcuda on the disk-PSF system (64 x 64, sigma_s = 0.05) against fo.cg on the same system: six iterations on
    both sides agree to 1e-5; at rtol = 1e-6 the device reports `optimal` before the 5000-iteration cap and its solution's
    true residual, recomputed with an independent fh_amm, is <= 1.05 rtol ||b||.  (The oracle's cg() is optimal on this system
    after 767 iterations with the golden DCT prior and after 17 with the identity prior.)"""
    from oracle import fh_oracle as fo
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda
    S = 64
    orc, hip = _cov_pair(kind, S, str(tmp_path), dev, gold, 0)
    op, oop = _disk_op(S, dev), _oracle_op(S)
    x_true = inputs.smooth_image(S, 31).to(F64)
    y = oop.forward(x_true, noise=inputs.randn((1, 3, S, S), 32))
    x0_mean = x_true + 0.05 * inputs.randn((1, 3, S, S), 33)
    A_mm, b, back, _shape = fo.system(oop, y, x0_mean, orc)
    m6h = solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, rtol=1e-300, maxiter=6)
    sol6, info6 = fo.cg(A_mm, b, rtol=0.0, maxiter=6)
    m6o = back(sol6)
    short = maxabs(m6o, m6h) / float(m6o.abs().max())
    assert info6["niter"] == 6 and tuple(m6h.shape) == (1, 3, S, S)
    rtol = 1e-6
    info_h = []
    solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, info_h, rtol=rtol)
    u_h = solve_customcuda.last_solution.clone()
    prob, keep = _problem(op, hip, _sigma_y2(op))
    bd = b.reshape(1, 3, S, S).to(dev)
    res = float((bd - _amm(hip, prob, u_h)).norm())
    print(f"window solve {kind}: short {short:.2e}; rtol 1e-6: device {info_h[0]['niter']} it, true residual "
          f"{res / float(bd.norm()):.3e} ||b||", flush=True)
    assert short <= 1e-5
    assert info_h[0]["optimal"] and 1 <= info_h[0]["niter"] < 5000
    assert res <= 1.05 * rtol * float(bd.norm())


# ---------------------------------------------------------------- 5. batched solve = single solves
def test_batched_window_solve_equals_single(dev, tmp_path):
    """fh_cg_solve_batched with op = 4 for 4 images against four fh_cg_solve calls by the rule of
    test_batched_colorization_solve_equals_single: identical iteration counts, solutions to 1e-12 of max|mat|.  Image 0's
    right-hand side is constant over the image, an eigenvector of A (its DC gain) and of the diagonal DCT-basis covariance: its
    CG stops after one iteration and every kernel of the loop, the window kernel included, skips its planes from then on."""
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda, solve_customcuda_batched
    S, nimg = 64, 4
    dv = torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
    torch.save(dv, tmp_path / "dct_variance.pt")
    ops, covs, ys, xs = [], [], [], []
    for b in range(nimg):
        op = _disk_op(S, dev, slot=b)
        cov = hc.CovarianceHessianBFGSDCT(str(tmp_path), 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=b)
        x = inputs.randn((1, 3, S, S), 300 + b).to(dev) * 40.0  # one time update each: distinct diagonals, no factor columns
        cov.update_time_step(x, 80.0, [40.0, 25.0, 12.0, 30.0][b], -x / 80.0 ** 2 * 0.5)
        x0 = inputs.smooth_image(S, 310 + b).to(dev)
        if b == 0:
            ys.append(torch.full((1, 3, S, S), 0.5, dtype=torch.float32, device=dev))
            xs.append(torch.zeros(1, 3, S, S, dtype=F64, device=dev))
        else:
            ys.append(op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 3, S, S), 320 + b, torch.float32).to(dev))
            xs.append((0.3 * x0).to(F64))
        ops.append(op)
        covs.append(cov)
    assert len({float(c.C.D.sum()) for c in covs}) == nimg and all(c.famC.m == 0 for c in covs)
    sigma_t = 0.4  # rtol_func(0.4) = 9e-3
    infos_b = []
    mats_b = solve_customcuda_batched(ops, ys, xs, covs, 1.0, sigma_t, infos_b, exclusive=True)
    assert tuple(mats_b.shape) == (nimg, 3, S, S)
    n_b = [i["niter"] for i in infos_b]
    for b in range(nimg):
        info = []
        one = solve_customcuda(ops[b], ys[b], xs[b], covs[b], 1.0, sigma_t, info)
        assert infos_b[b]["niter"] == info[0]["niter"], (b, n_b, info[0])
        assert infos_b[b]["optimal"] and info[0]["optimal"]
        assert maxabs(mats_b[b:b + 1], one) <= 1e-12 * float(one.abs().max()), b
    print(f"batched window solve: iterations {n_b}", flush=True)
    assert n_b[0] < min(n_b[1:]), n_b  # image 0 finished first: the `done` skip ran


def test_batched_solve_refuses_different_psfs(dev, tmp_path):
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda_batched
    from free_hunch_amd.measurements import get_operator
    S = 64
    ops = [_disk_op(S, dev, 0), get_operator(name="custom_blur", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S),
                                             kernel=disk_psf(radius=15.0))]
    covs = [hc.CovarianceHessianBFGS(1, 80.0 ** 2, 3 * S * S, device=dev, ctx_slot=b) for b in range(2)]
    z = torch.zeros(1, 3, S, S, dtype=F64, device=dev)
    with pytest.raises(AssertionError, match="PSF"):
        solve_customcuda_batched(ops, [z, z], [z, z], covs, 1.0, 0.4)


# ---------------------------------------------------------------- 6. the operator class, a separable PSF, sampler, CLI
def test_operator_class_runs_the_window_kernel(dev):
    S = 64
    x = inputs.smooth_image(S, 3).to(dev)
    op, oop = _disk_op(S, dev), _oracle_op(S)
    assert op.taps.window is not None
    y = op.forward(x, noiseless=True)
    assert tuple(y.shape) == (1, 3, S, S) and y.dtype == x.dtype
    assert maxabs(y, oop.forward(x.cpu().to(F64))) < 1e-6
    for back in (op.transpose(y), op.forward_adjoint(y)):
        assert tuple(back.shape) == (1, 3, S, S) and back.dtype == y.dtype
        assert maxabs(back, oop.transpose(y.cpu().to(F64))) < 1e-6
    y2, flat = op.forward(x, flatten=True, noiseless=True)
    assert tuple(flat.shape) == (1, 3 * S * S) and torch.equal(y2, y)
    assert abs(float((op.forward(x) - y).std()) - SIGMA_S) < 0.1 * SIGMA_S
    FB, FBC, F2B, FBFy = op.pre_calculated
    assert tuple(FB.shape) == (1, 1, S, S) and abs(float(FB[0, 0, 0, 0].real) - 1.0) < 1e-5  # DC gain = sum of the PSF


def test_separable_custom_psf_takes_the_shipped_gaussians_route(dev, gold, tmp_path):
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    from free_hunch_amd.measurements import KERNEL_DIR, get_operator
    S = 64
    _orc, hip = _cov_pair("dct_diagonal", S, str(tmp_path), dev, gold, 0)
    kw = dict(device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S))
    cus = get_operator(name="custom_blur", kernel_path=os.path.join(KERNEL_DIR, "gaussian_ks61_std3.0.npy"), **kw)
    gau = get_operator(name="gaussian_blur", kernel_size=61, intensity=3.0, **kw)
    assert cus.taps.sep is not None and cus.taps.window is None
    pc, keep_c = _problem(cus, hip, _sigma_y2(cus))
    pg, keep_g = _problem(gau, hip, _sigma_y2(gau))
    assert pc.op == pg.op == 1 and pc.ntaps2 == pg.ntaps2 > 0
    for f in ("ntaps", "halo", "halo2", "stride", "fold_sym", "sigma_y2"):
        assert getattr(pc, f) == getattr(pg, f), f
    assert bool(pc.fold_fwd_w) == bool(pg.fold_fwd_w) and bool(pc.fold_inv_h) == bool(pg.fold_inv_h)
    x = inputs.smooth_image(S, 5).to(dev)
    assert torch.equal(cus.forward(x, noiseless=True), gau.forward(x, noiseless=True))
    assert torch.equal(cus.transpose(x), gau.transpose(x))


def test_lockstep_window_blur_equals_per_image(dev, gold, tmp_path):
    """conditional_sampler_grouped(groups = 1) over two disk-blurred images against per-image conditional_sampler runs by the
    rule of test_batched_equals_per_image (identical niter and k lists, outputs within 1e-3), Euler with 4 steps and the
    batch-invariant Gaussian-prior denoiser."""
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_grouped
    B, S = 2, 64
    torch.save(torch.from_numpy(gold("trajectories")["dct_variance64"]), tmp_path / "dct_variance.pt")
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(tmp_path, {})
    ops, ys, noise = [], [], []
    for b in range(B):
        op = _disk_op(S, dev, slot=b)
        ops.append(op)
        x0 = 0.5 * inputs.smooth_image(S, 70 + b).to(dev)
        ys.append(op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 3, S, S), 80 + b, torch.float32).to(dev))
        noise.append(inputs.randn((1, 3, S, S), 90 + b, torch.float32))
    noise = torch.cat(noise).to(dev)
    run = dict(num_steps=4, sigma_min=0.002, sigma_max=80, rho=7, solver="euler")
    xb = conditional_sampler_grouped(net, noise, ys, ops, groups=1, **run, **kw)
    torch.cuda.synchronize()
    tb = [m.trace for m in conditional_sampler_grouped.last_mechanisms]
    assert tuple(xb.shape) == (B, 3, S, S) and bool(torch.isfinite(xb).all())
    for b in range(B):
        x1, _, _ = conditional_sampler(net, noise[b:b + 1], None, None, measurement=ys[b], operator=ops[b], **run, **kw)
        t1 = conditional_sampler.last_mechanism.trace
        assert [t["niter"] for t in t1] == [t["niter"] for t in tb[b]], b
        assert [t["k"] for t in t1] == [t["k"] for t in tb[b]], b
        assert float((x1 - xb[b:b + 1]).abs().max()) < 1e-3
    print(f"lock-step window blur: iterations {[t['niter'] for t in tb[0]]}", flush=True)


def test_cli_custom_blur(tmp_path):
    import PIL.Image
    sys.path.insert(0, ROOT)
    from bench import smooth_images
    import generate_conditional as gc
    data = tmp_path / "data"
    data.mkdir()
    for i, im in enumerate(smooth_images(2, 256, 7)):
        PIL.Image.fromarray(im.permute(1, 2, 0).numpy(), "RGB").save(data / f"img{i:08d}.png")
    np.save(tmp_path / "disk.npy", disk_psf())
    out = tmp_path / "out"
    # (sigma_min = 0.5 keeps the last call's CG tolerance, rtol_func(sigma), near 1e-2 instead of 1e-14)
    gc.main([f"--outdir={out}", f"--dataset_path={data}", "--synthetic_weights=ffhq", "--num_steps=3", "--solver=euler",
             "--sigma_min=0.5", "--total_images=2", "--max_batch_size=2", "--operator_name=custom_blur",
             f"--kernel_path={tmp_path / 'disk.npy'}", "--conditioning_mechanism=online_covariance",
             "--image_base_covariance=dct_diagonal"])
    names = ["000000_000000.png", "000001_000000.png"]
    for folder in ("images", "forward_images"):
        assert sorted(os.listdir(out / folder)) == names, folder
        for n in names:
            im = PIL.Image.open(out / folder / n)
            assert im.mode == "RGB" and im.size == (256, 256) and np.asarray(im).std() > 0
    txt = open(out / "results.txt").read()
    assert "PSNR" in txt and "SSIM" in txt
