"""`varying_blur` on the device: the blended operator pair (fh_conv_blend, fused and chain routes) and fh_problem.op = 14 from one
application of A_mm up to the CLI.

The reference is built here from the oracle's primitives: with FB_k = p2o(PSF_k) in complex128 (float64 copies of the float32
PSFs the operator holds) and U_k the operator's maps,
    fwd(v)  = sum_k U_k * ifft2(FB_k fft2(v)).real
    adj(u)  = sum_k ifft2(conj(FB_k) fft2(U_k * u)).real
    A_mm(u) = s2 u + fwd(C(adj(u))),   C = the oracle covariance's denoiser_cov_vector_dot,  s2 = clip(sigma_s, 0.001)^2.
The PSFs are `test_varying_blur_host.psf_family`: non-rank-1, ragged lists (49 / 64 / a few taps), optionally one streak that
reaches 32; the maps `grid_blend_weights` or random finite maps with negative entries.  Sides: 64 and 96 (whole tiles), 80, 100
and 60 (ragged against the 32 x 64 and 32 x 16 tiles: the edge guards), one case at 256.  The bars are those of
tests/test_burst_sr_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import inputs
import nets
import test_custom_sr_gpu as srt
from test_burst_sr_host import PSF7
from test_channel_ops_gpu import _amm, _run_script
from test_hip_parity import _base_kwargs, maxabs
from test_varying_blur_host import psf_family, random_maps

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "free-hunch_amd", "data")
SIGMA_S = 0.05
GRID = {1: (1, 1), 4: (2, 2), 9: (3, 3), 16: (4, 4)}
# (S, K, wide PSF, maps)
CASES = [(64, 1, False, "grid"), (64, 4, False, "grid"), (96, 9, False, "grid"), (96, 16, False, "random"),
         (80, 4, True, "grid"), (100, 9, False, "random"), (100, 4, True, "random"), (60, 16, False, "grid")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _op(S, K, dev, wide=False, maps="grid", slot=0, kernels=None, blend=None):
    from free_hunch_amd.measurements import get_operator
    kw = dict(psf_grid=GRID[K]) if (maps == "grid" and blend is None) else dict(blend=random_maps(K, S) if blend is None else blend)
    op = get_operator(name="varying_blur", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S),
                      kernels=psf_family(K, wide) if kernels is None else kernels, **kw)
    op.ctx_slot = slot
    return op


def _route(op, adjoint):
    from free_hunch_amd import _lib
    out = (C.c_int32 * 6)()
    ft = op.frame_taps
    assert _lib.load().fh_conv_blend_plan(op.in_shape[-1], ft.nframes, ft.max_taps, ft.halo, 3, adjoint, out) == 0
    return out[0]


def _switch(monkeypatch, route):
    if route == "chain":
        monkeypatch.setenv("FH_BLEND_FUSED", "0")
    else:
        monkeypatch.delenv("FH_BLEND_FUSED", raising=False)


class Ref:
    """the reference pair of a varying-blur operator, float64 on the CPU"""

    def __init__(self, op):
        from oracle import fh_oracle as fo
        S = op.in_shape[-1]
        self.FB = [fo.p2o(torch.from_numpy(k.astype(np.float64))[None, None], (S, S)) for k in op.kernels]
        assert self.FB[0].dtype == torch.complex128
        self.U = op.blend.cpu()  # [K,3,S,S]
        self.s2 = torch.tensor([SIGMA_S], dtype=torch.float32).clip(min=0.001) ** 2  # the oracle's blur rule

    def fwd(self, v):
        F = torch.fft.fft2(v)
        return sum(U * torch.fft.ifft2(FB * F).real for U, FB in zip(self.U, self.FB))

    def adj(self, u):
        return sum(torch.fft.ifft2(torch.conj(FB) * torch.fft.fft2(U * u)).real for U, FB in zip(self.U, self.FB))

    def system(self, orc, shape):
        def A_mm(u):
            u = u.reshape(shape)
            return (self.s2 * u + self.fwd(orc.denoiser_cov_vector_dot(self.adj(u)))).flatten()
        return A_mm


def _pair(op, x, u, dev, planes):
    """fh_conv_blend forward of x and adjoint of u ([N,3,S,S] each) on a context of `planes` planes, outputs pre-filled with NaN"""
    from free_hunch_amd import _lib
    S = op.in_shape[-1]
    N = planes // 3
    ctx = _lib.Context.get(S, planes, 0)
    nan = lambda: torch.full((N, 3, S, S), float("nan"), dtype=F64, device=dev)  # noqa: E731
    f = ctx.blur_blend(x[:N].contiguous(), nan(), op.frame_taps, op.blend, planes)
    a = ctx.blur_blend(u[:N].contiguous(), nan(), op.frame_taps, op.blend, planes, adjoint=True)
    torch.cuda.synchronize()
    return f, a


# ---------------------------------------------------------------- 1. the operator pair against the reference
@pytest.mark.parametrize("S,K,wide,maps", CASES + [(256, 4, False, "grid")])
def test_operator_pair_against_the_reference(dev, S, K, wide, maps):
    """forward and adjoint within 1e-12 max(1, max|ref|) for 3 and for 9 planes (a NaN left in the output fails); the first image
    of the 9-plane run equals the 3-plane run bit for bit; <A x, u> = <x, A^T u> to 1e-10.  Every case plans the fused route."""
    op = _op(S, K, dev, wide, maps)
    assert (_route(op, 0), _route(op, 1)) == (1, 1)
    ref = Ref(op)
    x, u = inputs.randn((3, 3, S, S), 11), inputs.randn((3, 3, S, S), 12)
    rf, ra = ref.fwd(x), ref.adj(u)
    got = {}
    for planes in (3, 9):
        N = planes // 3
        f, a = _pair(op, x.to(dev), u.to(dev), dev, planes)
        e_f, e_a = maxabs(f, rf[:N]), maxabs(a, ra[:N])
        print(f"blend S={S} K={K} wide={wide} {maps} planes={planes}: forward {e_f / max(1.0, float(rf.abs().max())):.2e} adjoint "
              f"{e_a / max(1.0, float(ra.abs().max())):.2e}", flush=True)
        assert e_f < 1e-12 * max(1.0, float(rf[:N].abs().max()))
        assert e_a < 1e-12 * max(1.0, float(ra[:N].abs().max()))
        got[planes] = (f, a)
    assert torch.equal(got[9][0][:1], got[3][0]) and torch.equal(got[9][1][:1], got[3][1])
    f, a = got[9]
    lhs, rhs = float((f * u.to(dev)).sum()), float((x.to(dev) * a).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


# ---------------------------------------------------------------- 2. fused = chain, bit for bit
@pytest.mark.parametrize("S,K,wide,maps", CASES)
def test_fused_route_equals_the_chain_bit_for_bit(dev, tmp_path_factory, monkeypatch, S, K, wide, maps):
    """FH_BLEND_FUSED=0 against the default: forward and adjoint of fh_conv_blend on 9 planes, and A_mm (the forward blend with
    its sigma_y^2 u add) on op 14, agree in every bit"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    op = _op(S, K, dev, wide, maps)
    x, u = inputs.randn((3, 3, S, S), 13).to(dev), inputs.randn((3, 3, S, S), 14).to(dev)
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.op == 14
    _switch(monkeypatch, "fused")
    f1, a1 = _pair(op, x, u, dev, 9)
    amm1 = _amm(hip, prob, u[:1].contiguous())
    _switch(monkeypatch, "chain")
    f0, a0 = _pair(op, x, u, dev, 9)
    amm0 = _amm(hip, prob, u[:1].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(f0, f1) and torch.equal(a0, a1) and torch.equal(amm0, amm1)
    assert bool(torch.isfinite(amm1).all()) and float(amm1.abs().max()) > 0


# ---------------------------------------------------------------- 3. degenerate cases, bit for bit
@pytest.mark.parametrize("route", ["fused", "chain"])
@pytest.mark.parametrize("S,wide", [(64, False), (80, True), (60, False)])
def test_one_psf_with_an_all_ones_map_equals_fh_conv_circ(dev, monkeypatch, route, S, wide):
    from free_hunch_amd import _lib
    _switch(monkeypatch, route)
    op = _op(S, 1, dev, kernels=[psf_family(4, wide)[3]], blend=np.ones((1, S, S)))
    x, u = inputs.randn((3, 3, S, S), 15).to(dev), inputs.randn((3, 3, S, S), 16).to(dev)
    ctx = _lib.Context.get(S, 9, 0)
    cf = ctx.conv(x, torch.empty(3, 3, S, S, dtype=F64, device=dev), op.frames[0], 9, 1, False)
    ca = ctx.conv(u, torch.empty(3, 3, S, S, dtype=F64, device=dev), op.frames[0], 9, 1, True)
    f, a = _pair(op, x, u, dev, 9)
    assert torch.equal(f, cf) and torch.equal(a, ca)


@pytest.mark.parametrize("route", ["fused", "chain"])
@pytest.mark.parametrize("n_script", [0, 4])
def test_amm_one_psf_equals_op_1(dev, tmp_path_factory, monkeypatch, n_script, route):
    """K = 1 with an all-ones map is custom_blur on its plain tap list (the PSF is not rank-1: no 1-D passes, no fold): the
    same bits from fh_amm"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    from free_hunch_amd.measurements import get_operator
    _switch(monkeypatch, route)
    S = 64
    psf = psf_family(2)[1]
    _orc, hip = srt._cov_pair(S, n_script, tmp_path_factory, dev)
    op = _op(S, 1, dev, kernels=[psf], blend=np.ones((1, S, S)))
    one = get_operator(name="custom_blur", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), kernel=psf)
    p14, k14 = _problem(op, hip, _sigma_y2(op))
    p1, k1 = _problem(one, hip, _sigma_y2(one))
    assert p14.op == 14 and p1.op == 1 and p1.ntaps2 == 0 and not p1.fold_fwd_w and p14.sigma_y2 == p1.sigma_y2
    assert p1.ntaps == p14.ntaps == 64 and p14.m == 2 * n_script
    u = inputs.randn((1, 3, S, S), 23).to(dev)
    assert torch.equal(_amm(hip, p14, u), _amm(hip, p1, u))


@pytest.mark.parametrize("route", ["fused", "chain"])
@pytest.mark.parametrize("S,K", [(64, 4), (100, 9)])
def test_one_hot_maps_over_identical_psfs(dev, monkeypatch, route, S, K):
    """K copies of one PSF under one-hot maps (every pixel belongs to exactly one PSF) are that PSF's blur: the forward blend
    adds exact zeros to one exact product with 1, so it equals fh_conv_circ bit for bit.  The adjoint splits the input into K
    disjoint pieces and adds K separately rounded convolutions - the same operator, another summation order - so it is held to
    the reference's bar, 1e-12 max(1, max|ref|), not to the bits."""
    from free_hunch_amd import _lib
    _switch(monkeypatch, route)
    owner = torch.from_numpy(np.random.default_rng(3).integers(0, K, (3, S, S)))
    hot = np.stack([(owner == k).numpy().astype(np.float64) for k in range(K)])  # [K,3,S,S]
    psf = psf_family(2)[1]
    op = _op(S, K, dev, kernels=[psf] * K, blend=hot)
    x, u = inputs.randn((3, 3, S, S), 17).to(dev), inputs.randn((3, 3, S, S), 18).to(dev)
    ctx = _lib.Context.get(S, 9, 0)
    cf = ctx.conv(x, torch.empty(3, 3, S, S, dtype=F64, device=dev), op.frames[0], 9, 1, False)
    ca = ctx.conv(u, torch.empty(3, 3, S, S, dtype=F64, device=dev), op.frames[0], 9, 1, True)
    f, a = _pair(op, x, u, dev, 9)
    assert torch.equal(f, cf)
    assert maxabs(a, ca) < 1e-12 * max(1.0, float(ca.abs().max()))


@pytest.mark.parametrize("route", ["fused", "chain"])
@pytest.mark.parametrize("S", [64, 100])
def test_delta_psfs_give_the_piecewise_roll(dev, monkeypatch, route, S):
    """delta PSFs with another integer shift per quadrant: y = the scene rolled by (-dy_k, -dx_k) inside quadrant k, exactly (a
    PSF displaced by (dy, dx) samples the scene at (i + dy, j + dx), `shifted_psf`); the adjoint scatters the quadrants back"""
    from free_hunch_amd.measurements import shifted_psf
    _switch(monkeypatch, route)
    shifts = [(0, 0), (3, -2), (-5, 7), (32, -32)]
    h = S // 2
    quad = np.zeros((4, S, S))
    quad[0, :h, :h] = quad[1, :h, h:] = quad[2, h:, :h] = quad[3, h:, h:] = 1.0
    op = _op(S, 4, dev, kernels=[shifted_psf(np.ones((1, 1)), dy, dx) for dy, dx in shifts], blend=quad)
    assert [t.n for t in op.frames] == [1, 1, 1, 1] and (op.frame_taps.hy, op.frame_taps.hx) == (32, 32)
    x = inputs.randn((1, 3, S, S), 19).to(dev)
    q = torch.from_numpy(quad).to(dev)
    y = op.forward(x, noiseless=True)
    want = sum(q[k] * torch.roll(x, (-dy, -dx), (-2, -1)) for k, (dy, dx) in enumerate(shifts))
    assert y.dtype == x.dtype and tuple(y.shape) == tuple(op.out_shape) == (1, 3, S, S) and torch.equal(y, want)
    back = op.transpose(y)
    assert torch.equal(back, sum(torch.roll(q[k] * y, (dy, dx), (-2, -1)) for k, (dy, dx) in enumerate(shifts)))
    assert torch.equal(back, op.forward_adjoint(y)) and torch.equal(back, op.transpose(y.reshape(1, -1), flatten=True))
    torch.manual_seed(7)
    noisy = op.forward(x)
    torch.manual_seed(7)  # ONE draw at the image's shape
    assert torch.equal(noisy, y + op.sigma_s.to(y.dtype) * torch.randn(1, 3, S, S, dtype=y.dtype, device=dev))
    assert op._last_y is noisy
    fl, flat = op.forward(x, flatten=True, noiseless=True)
    assert torch.equal(fl, y) and tuple(flat.shape) == (1, 3 * S * S)


# ---------------------------------------------------------------- 4. one application of A_mm
def _amm_case(dev, tmp_factory, S, K, wide, maps, n_script):
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    orc, hip = srt._cov_pair(S, n_script, tmp_factory, dev)
    op = _op(S, K, dev, wide, maps)
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.op == 14 and prob.stride == 1 and prob.m == 2 * n_script and prob.use_dct == 1 and prob.ntaps2 == K
    shape = (1, 3, S, S)
    A_mm = Ref(op).system(orc, shape)
    u, v = inputs.randn(shape, 21).to(dev), inputs.randn(shape, 22).to(dev)
    au, av = _amm(hip, prob, u), _amm(hip, prob, v)
    ref = A_mm(u.cpu().flatten()).reshape(shape)
    err = maxabs(au, ref) / float(ref.abs().max())
    l, r = float((u * av).sum()), float((au * v).sum())
    print(f"amm op=14 S={S} K={K} wide={wide} {maps} m={prob.m}: {err:.2e}, symmetry {abs(l - r) / max(abs(l), 1.0):.2e}", flush=True)
    assert err <= 1e-8
    assert abs(l - r) <= 1e-9 * max(abs(l), 1.0)


@pytest.mark.parametrize("n_script", [0, 4])
@pytest.mark.parametrize("S,K,wide,maps", [(64, 4, False, "grid"), (64, 16, False, "random"), (96, 9, False, "grid"),
                                           (80, 4, True, "grid"), (100, 9, False, "random"), (60, 1, False, "grid")])
def test_amm_vs_reference_system(dev, tmp_path_factory, S, K, wide, maps, n_script):
    """fh_amm with op = 14 against s2 u + fwd(C(adj(u))) on the shipped DCT prior cut to S, before any update (m = 0) and after 4
    scripted update pairs (m = 8): 1e-8 of max|ref| and symmetry to 1e-9, the bars of test_burst_sr_gpu"""
    _amm_case(dev, tmp_path_factory, S, K, wide, maps, n_script)


def test_amm_vs_reference_system_at_the_real_size(dev, tmp_path_factory):
    _amm_case(dev, tmp_path_factory, 256, 4, False, "grid", 0)


def test_identity_prior_stays_on_op_14(dev):
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 64
    op = _op(S, 4, dev)
    cov = hc.ScalarCovariance(0.7, 3 * S * S, dev)  # C = 0.7 I in image space, what the scalar-variance mechanisms solve with
    prob, keep = _problem(op, cov, _sigma_y2(op))
    assert prob.op == 14 and prob.use_dct == 0 and prob.stride == 1 and prob.ntaps2 == 4 and not prob.fold_fwd_w
    shape = (1, 3, S, S)
    u = inputs.randn(shape, 24).to(dev)
    ref = Ref(op)
    want = float(ref.s2) * u.cpu() + 0.7 * ref.fwd(ref.adj(u.cpu()))
    assert maxabs(_amm(cov, prob, u), want) <= 1e-8 * float(want.abs().max())


# ---------------------------------------------------------------- 5. the solve
def _solve_inputs(op, S):
    ref = Ref(op)
    x_true = inputs.smooth_image(S, 31).to(F64)
    y = ref.fwd(x_true) + SIGMA_S * inputs.randn((1, 3, S, S), 32)
    x0_mean = x_true + 0.05 * inputs.randn((1, 3, S, S), 33)
    return ref, y, x0_mean, (y - ref.fwd(x0_mean)).flatten()


@pytest.mark.parametrize("S,K,wide", [(64, 4, False), (100, 9, False), (80, 4, True)])
def test_six_iterations_vs_oracle_cg(dev, tmp_path_factory, S, K, wide):
    """six forced iterations on both sides agree to 1e-5 of max|mat|"""
    from oracle import fh_oracle as fo
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda
    orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    op = _op(S, K, dev, wide)
    ref, y, x0_mean, b = _solve_inputs(op, S)
    m6h = solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, rtol=1e-300, maxiter=6)
    sol6, info6 = fo.cg(ref.system(orc, tuple(y.shape)), b, rtol=0.0, maxiter=6)
    m6o = ref.adj(sol6.reshape(y.shape))
    short = maxabs(m6o, m6h) / float(m6o.abs().max())
    print(f"varying-blur solve S={S} K={K}: six iterations {short:.2e}", flush=True)
    assert info6["niter"] == 6 and tuple(m6h.shape) == (1, 3, S, S)
    assert short <= 1e-5


def test_converged_solve_meets_its_tolerance(dev, tmp_path_factory):
    """(64, K = 4 on a 2 x 2 grid, sigma_s = 0.05, m = 0) at rtol = 1e-4: `optimal` before the 5000-iteration cap, and the true
    residual of the returned solution, recomputed with an independent fh_amm, is <= 1.05 rtol ||b||"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda
    S = 64
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    op = _op(S, 4, dev)
    _ref, y, x0_mean, b = _solve_inputs(op, S)
    rtol, info_h = 1e-4, []
    solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, info_h, rtol=rtol)
    u_h = solve_customcuda.last_solution.clone()
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.op == 14 and prob.m == 0 and tuple(u_h.shape) == tuple(y.shape)
    bd = b.reshape(y.shape).to(dev)
    res = float((bd - _amm(hip, prob, u_h)).norm())
    print(f"varying-blur solve rtol 1e-4: device {info_h[0]['niter']} it, true residual {res / float(bd.norm()):.3e} ||b||", flush=True)
    assert info_h[0]["optimal"] and 1 <= info_h[0]["niter"] < 5000
    assert res <= 1.05 * rtol * float(bd.norm())


@pytest.mark.parametrize("route", ["fused", "chain"])
@pytest.mark.parametrize("n_script", [0, 4])
def test_batched_solve_equals_single(dev, tmp_path, monkeypatch, n_script, route):
    """fh_cg_solve_batched with op = 14 over 2 images with their own measurements and covariances against per-image solves by the
    rule of test_burst_sr_gpu.test_batched_solve_equals_single: identical iteration counts, `mat` within 1e-12 of max|mat|.  The
    images stop at different iterations, so the kernels skip the finished image from then on, on either route."""
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda, solve_customcuda_batched
    _switch(monkeypatch, route)
    S, nimg = 64, 2
    dv = torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
    torch.save(dv, tmp_path / "dct_variance.pt")
    ops, covs, ys, xs = [], [], [], []
    for b in range(nimg):
        op = _op(S, 4, dev, slot=b)
        cov = hc.CovarianceHessianBFGSDCT(str(tmp_path), 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=b)
        if n_script:
            _run_script(cov, inputs.script(1300 + b, (1, 3, S, S), n_script, 80.0, sig_end=[20.0, 0.5][b]), dev)
        else:
            x = inputs.randn((1, 3, S, S), 300 + b).to(dev) * 40.0
            cov.update_time_step(x, 80.0, [40.0, 12.0][b], -x / 80.0 ** 2 * 0.5)
        x0 = inputs.smooth_image(S, 310 + b).to(dev)
        ys.append(op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 3, S, S), 320 + b, torch.float32).to(dev))
        xs.append((0.3 * x0).to(F64))
        ops.append(op)
        covs.append(cov)
    assert all(c.famC.m == 2 * n_script for c in covs) and _problem(ops[0], covs[0], _sigma_y2(ops[0]))[0].op == 14
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
    print(f"batched varying-blur solve m={2 * n_script} {route}: iterations {n_b}", flush=True)
    assert min(n_b) < max(n_b), n_b  # an image finished first: the `done` skip ran


def test_batched_solve_refuses_different_psfs_and_maps(dev):
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda_batched
    S = 64
    covs = [hc.CovarianceHessianBFGS(1, 80.0 ** 2, 3 * S * S, device=dev, ctx_slot=b) for b in range(2)]
    z = torch.zeros(1, 3, S, S, dtype=F64, device=dev)
    fam = psf_family(4)
    ops = [_op(S, 4, dev, slot=0), _op(S, 4, dev, slot=1, kernels=fam[:3] + [fam[3] * 2])]  # one PSF differs
    with pytest.raises(AssertionError, match="PSF"):
        solve_customcuda_batched(ops, [z, z], [z, z], covs, 1.0, 0.4)
    ops = [_op(S, 4, dev, slot=0), _op(S, 4, dev, slot=1, maps="random")]
    with pytest.raises(AssertionError, match="blend maps"):
        solve_customcuda_batched(ops, [z, z], [z, z], covs, 1.0, 0.4)


@pytest.mark.parametrize("route", ["fused", "chain"])
def test_graph_is_not_replayed_for_other_offsets_or_routes(dev, tmp_path_factory, monkeypatch, route):
    """The chain route slices the tap lists on the host, so a captured chunk of CG iterations holds the list boundaries.  Two
    operators whose problems agree in every field and pointer but not in the offsets BEHIND tap2_dy - permuted ragged lists
    written into the same device buffers - must not share a cached graph: the second solve equals, bit for bit, the solve of a
    freshly built operator with the permuted lists, and differs from the first.  Then the switch flips: the solve on the other
    route (whose graph is another entry of the cache) gives the same bits."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda
    from free_hunch_amd.measurements import shifted_psf
    _switch(monkeypatch, route)
    S = 64
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    p49, p64, p56 = PSF7, shifted_psf(PSF7, 0.5, 0.5), shifted_psf(PSF7, 0.5, 0)
    maps = random_maps(3, S)
    a, b = _op(S, 3, dev, kernels=[p49, p64, p56], blend=maps), _op(S, 3, dev, kernels=[p49, p56, p64], blend=maps)
    fa, fb = a.frame_taps, b.frame_taps
    assert [t.n for t in a.frames] == [49, 64, 56] and [t.n for t in b.frames] == [49, 56, 64]
    assert (fa.n, fa.max_taps, fa.halo) == (fb.n, fb.max_taps, fb.halo) and fa.off.tolist() != fb.off.tolist()
    y = inputs.randn((1, 3, S, S), 41).to(dev)
    x0 = inputs.smooth_image(S, 42).to(dev).to(F64)
    solve = lambda op: solve_customcuda(op, y, x0, hip, 1.0, 1.0, rtol=1e-300, maxiter=16).clone()  # noqa: E731
    pa, keep_a = _problem(a, hip, _sigma_y2(a))
    first = solve(a)
    for dst, src in ((fa.dy, fb.dy), (fa.dx, fb.dx), (fa.w, fb.w), (fa.off, fb.off)):  # the same buffers, the other operator
        dst.copy_(src)
    a.kernels, a.frames = b.kernels, b.frames
    torch.cuda.synchronize()
    pa2, keep_a2 = _problem(a, hip, _sigma_y2(a))
    assert all(getattr(pa, f) == getattr(pa2, f) for f in ("tap_dy", "tap_dx", "tap_w", "tap2_dy", "ntaps", "ntaps2", "halo", "halo2"))
    second, fresh = solve(a), solve(b)
    assert torch.equal(second, fresh)
    assert not torch.equal(second, first) and bool(torch.isfinite(second).all())
    _switch(monkeypatch, "fused" if route == "chain" else "chain")
    assert torch.equal(solve(b), fresh)


# ---------------------------------------------------------------- 6. refusals without a launch
def test_op14_refuses_bad_problems_without_launching(dev, tmp_path_factory):
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 64
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    op = _op(S, 4, dev)  # lists of 49, 64, 6 and 49 taps: offsets 0, 49, 113, 119, 168
    u = inputs.randn((1, 3, S, S), 61).to(dev)
    out = torch.full_like(u, 123.0)
    info = _lib.FhCgInfo()
    some = u.data_ptr()
    bad_off = torch.tensor([0, 49, 40, 119, 168], dtype=torch.int32, device=dev)  # not increasing: refused once read back
    long_off = torch.tensor([0, 30, 95, 119, 168], dtype=torch.int32, device=dev)  # a list longer than halo2
    short_off = torch.tensor([0, 49, 113, 119, 160], dtype=torch.int32, device=dev)  # does not end at ntaps
    for field, value in (("stride", 0), ("stride", 2), ("stride", 4), ("ntaps2", 0), ("ntaps2", -1), ("ntaps2", 17),
                         ("halo2", 0), ("halo2", 1025), ("halo2", 63), ("halo2", 41), ("ntaps", 3), ("ntaps", 167), ("ntaps", 257),
                         ("tap_dy", None), ("tap_dx", None), ("tap_w", None),
                         ("tap2_dy", None), ("tap2_dy", bad_off.data_ptr()), ("tap2_dy", long_off.data_ptr()),
                         ("tap2_dy", short_off.data_ptr()), ("tap2_w", None),
                         ("tap2_dx", some), ("fold_fwd_w", some), ("fold_fwd_h", some), ("fold_inv_w", some),
                         ("fold_inv_h", some), ("fold_sym", 1), ("mask", some), ("halo", 6), ("halo", -5), ("halo", 1000 + 64 * 33),
                         ("halo", 1000 + 33), ("use_dct", 2), ("use_dct", -1), ("planes", 6), ("d", 3 * S * S - 1), ("op", 15)):
        prob, keep = _problem(op, hip, _sigma_y2(op))
        assert prob.op == 14
        setattr(prob, field, value)
        rc = hip.ctx.lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
        rc = hip.ctx.lib.fh_cg_solve(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), 1e-3, 0.0, 10, C.byref(info),
                                     _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
    prob, keep = _problem(op, hip, _sigma_y2(op))  # the batched entry point: no per-image mask on op 14
    per = _lib.FhBatch()
    per.nimg = 1
    per.D[0], per.r[0], per.B[0], per.M[0], per.mask[0] = prob.D, prob.r, prob.B, prob.M, some
    rtol = (C.c_double * 1)(1e-3)
    rc = hip.ctx.lib.fh_cg_solve_batched(hip.ctx.h, C.byref(prob), C.byref(per), u.data_ptr(), out.data_ptr(), rtol, 0.0, 10,
                                         C.byref(info), _lib.stream())
    assert rc == _lib.FH_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())  # nothing was launched


def test_conv_blend_refuses_bad_arguments_without_launching(dev):
    from free_hunch_amd import _lib
    S = 64
    op = _op(S, 4, dev)
    ft = op.frame_taps
    ctx = _lib.Context.get(S, 3, 0)
    x = torch.zeros(1, 3, S, S, dtype=F64, device=dev)
    out = torch.full((2, 3, S, S), 123.0, dtype=F64, device=dev)
    call = lambda *a: ctx.lib.fh_conv_blend(*a, _lib.stream())  # noqa: E731
    p = lambda t: t.data_ptr()  # noqa: E731
    # (ctx, in, out, dy, dx, w, frame_off | nframes, max_frame_taps, halo | blend | planes, adjoint)
    good = [ctx.h, p(x), p(out), p(ft.dy), p(ft.dx), p(ft.w), p(ft.off), ft.nframes, ft.max_taps, ft.halo, p(op.blend), 3, 0]
    assert len(good) == 13
    for missing in (0, 1, 2, 3, 4, 5, 6, 10):
        args = list(good)
        args[missing] = None
        assert call(*args) == _lib.FH_EINVAL, missing
    bad_off = torch.tensor([0, 49, 40, 119, 168], dtype=torch.int32, device=dev)
    long_off = torch.tensor([0, 30, 95, 119, 168], dtype=torch.int32, device=dev)
    zero_off = torch.tensor([1, 49, 113, 119, 168], dtype=torch.int32, device=dev)
    for index, value in ((7, 0), (7, -1), (7, 17), (8, 0), (8, 1025), (8, 63), (9, 6), (9, -3), (9, 999), (9, 1000 + 64 * 33),
                         (9, 1000 + 33), (11, 0), (11, 4), (11, -3), (12, 2), (12, -1), (6, p(bad_off)), (6, p(long_off)),
                         (6, p(zero_off))):
        args = list(good)
        args[index] = value
        assert call(*args) == _lib.FH_EINVAL, (index, value)
    args = list(good)
    args[2] = args[1]  # in == out
    assert call(*args) == _lib.FH_EINVAL
    args = list(good)
    args[11] = 6  # more planes than the context holds
    assert call(*args) == _lib.FH_ESIZE
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())


# ---------------------------------------------------------------- 7. end to end
def test_lockstep_varying_blur_equals_per_image(dev, gold, tmp_path):
    """conditional_sampler_grouped(groups = 1) over two images against per-image conditional_sampler runs by the rule of
    test_burst_sr_gpu.test_lockstep_burst_equals_per_image: identical niter and k lists, outputs within 1e-3; Euler with 4 steps,
    nets.gauss_net, sigma_min = 0.5"""
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_grouped
    B, S = 2, 64
    torch.save(torch.from_numpy(gold("trajectories")["dct_variance64"]), tmp_path / "dct_variance.pt")
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(tmp_path, {})
    ops, ys, noise = [], [], []
    for b in range(B):
        op = _op(S, 4, dev, slot=b)
        ops.append(op)
        x0 = 0.5 * inputs.smooth_image(S, 70 + b).to(dev)
        ys.append(op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 3, S, S), 80 + b, torch.float32).to(dev))
        noise.append(inputs.randn((1, 3, S, S), 90 + b, torch.float32))
    noise = torch.cat(noise).to(dev)
    run = dict(num_steps=4, sigma_min=0.5, sigma_max=80, rho=7, solver="euler")
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
    print(f"lock-step varying blur: iterations {[t['niter'] for t in tb[0]]}", flush=True)


@pytest.mark.parametrize("mechanism", ["dps", "diffpir"])
def test_adjoint_based_mechanisms_run(dev, tmp_path, mechanism):
    """DPS and DiffPIR reach the operator through forward / forward_adjoint / transpose only: two Euler steps stay finite"""
    from free_hunch_amd.sampler import conditional_sampler
    S = 64
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(tmp_path, {"conditioning_mechanism": mechanism})
    op = _op(S, 4, dev)
    x0 = 0.5 * inputs.smooth_image(S, 75).to(dev)
    y = op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 3, S, S), 85, torch.float32).to(dev)
    noise = inputs.randn((1, 3, S, S), 95, torch.float32).to(dev)
    x1, _, _ = conditional_sampler(net, noise, None, None, measurement=y, operator=op, num_steps=3, sigma_min=0.5, sigma_max=80,
                                   rho=7, solver="euler", **kw)
    assert tuple(x1.shape) == (1, 3, S, S) and bool(torch.isfinite(x1).all())


@pytest.mark.parametrize("route", ["fused", "chain"])
def test_cli_varying_blur(tmp_path, monkeypatch, route):
    import PIL.Image
    sys.path.insert(0, ROOT)
    from bench import smooth_images
    import generate_conditional as gc
    _switch(monkeypatch, route)
    data = tmp_path / "data"
    data.mkdir()
    for i, im in enumerate(smooth_images(2, 256, 7)):
        PIL.Image.fromarray(im.permute(1, 2, 0).numpy(), "RGB").save(data / f"img{i:08d}.png")
    fam = psf_family(4)
    side = max(max(k.shape) for k in fam)
    side += 1 - side % 2
    stack = np.zeros((4, side, side))
    for k, psf in enumerate(fam):  # odd sides: centred padding keeps every centre at size // 2
        py, px = (side - psf.shape[0]) // 2, (side - psf.shape[1]) // 2
        stack[k, py:py + psf.shape[0], px:px + psf.shape[1]] = psf
    np.save(tmp_path / "psfs.npy", stack)
    out = tmp_path / "out"
    gc.main([f"--outdir={out}", f"--dataset_path={data}", "--synthetic_weights=ffhq", "--num_steps=3", "--solver=euler",
             "--sigma_min=0.5", "--total_images=2", "--max_batch_size=2", "--operator_name=varying_blur",
             f"--kernel_path={tmp_path / 'psfs.npy'}", "--psf_grid=2x2",
             "--conditioning_mechanism=online_covariance", "--image_base_covariance=dct_diagonal"])
    names = ["000000_000000.png", "000001_000000.png"]
    for folder in ("images", "cond_images", "forward_images"):  # the measurement is full size: it is written
        assert sorted(os.listdir(out / folder)) == names, folder
        for n in names:
            im = PIL.Image.open(out / folder / n)
            assert im.mode == "RGB" and im.size == (256, 256) and np.asarray(im).std() > 0
    txt = open(out / "results.txt").read()
    assert "PSNR" in txt and "SSIM" in txt
