"""`weighted_burst_sr` on the device: a per-pixel noise map on the burst, fh_problem.op = 13 (op 12's fields with the weights
w = 1 / sigma in the mask field, [K][3][So][So] per image), from one application of A_mm up to the CLI.

The device solves the whitened system  A_mm(u) = u + W A C A^T W u  (Python passes sigma_y2 = 1).  The reference pair of the
burst is test_burst_sr_gpu.Ref (complex128 OTFs of the float32 PSFs the operator holds), the covariance the oracle's:
    ref(u) = u + w fwd(C(adj(w u))),    b = w (y - fwd(x0)),    mat = adj(w sol).
Shapes: fused (64, 4) K = 4 integer shifts, (96, 3) three ragged fractional frames, (64, 2) K = 4; chain (80, 4) fractional,
(60, 3) integer (So = 20).  Map F3: frame k = noise_map_n3(So) (1 + 0.5 k) - channels and frames both differ, about 11 % inf."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import inputs
import nets
import test_burst_sr_gpu as bt
import test_custom_sr_gpu as srt
import test_masked_blur_gpu as mb
from test_burst_sr_gpu import CHAIN, FOUR, FUSED, Ref
from test_burst_sr_host import FRACTIONAL, PSF7, integer_shifts
from test_channel_ops_gpu import _amm, _run_script
from test_custom_sr_host import binomial_psf
from test_hip_parity import _base_kwargs, maxabs
from test_noise_map_gpu import _weighted_ref
from test_noise_map_host import noise_map_n, noise_map_n3
from test_weighted_burst_host import map_f3

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_S = bt.SIGMA_S
# (S, s, frame set): the smallest shapes at which each route exists
SHAPES = [(64, 4, "four"), (96, 3, "frac"), (64, 2, "int"), (80, 4, "frac"), (60, 3, "int")]
assert all((S, s) in FUSED for S, s, _k in SHAPES[:3]) and all((S, s) in CHAIN for S, s, _k in SHAPES[3:])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _nframes(s, kind):
    return len(bt._shifts(s, kind))


def _wop(S, s, kind, dev, slot=0, shifts=None, kernels=None, **noise):
    """weighted_burst_sr on the frames of test_burst_sr_gpu._op; the noise source defaults to map F3"""
    from free_hunch_amd.measurements import get_operator
    shifts = bt._shifts(s, kind) if shifts is None else shifts
    if not any(k in noise for k in ("noise_map", "frame_sigmas")):
        noise["noise_map"] = map_f3(S // s, len(shifts))
    op = get_operator(name="weighted_burst_sr", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), scale_factor=s,
                      kernels=[PSF7] if kernels is None else kernels, frame_shifts=shifts, **noise)
    op.ctx_slot = slot
    return op


def _env(monkeypatch, route):
    if route == "chain":
        monkeypatch.setenv("FH_FRAMES_FUSED", "0")
    else:
        monkeypatch.delenv("FH_FRAMES_FUSED", raising=False)


def _problem13(op, cov):
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
    prob, keep = _problem(op, cov, _solver_sigma_y2(op))
    assert prob.op == 13 and prob.sigma_y2 == 1.0 and prob.mask == op.weights.data_ptr()
    return prob, keep


# ---------------------------------------------------------------- 1. all-ones weights are op 12, K = 1 is op 10, bit for bit
@pytest.mark.parametrize("n_script", [0, 4])
@pytest.mark.parametrize("S,s,kind,route", [(64, 4, "four", "fused"), (64, 4, "four", "chain"), (80, 4, "frac", "fused")])
def test_all_ones_weights_equal_op_12_bitwise(dev, tmp_path_factory, monkeypatch, S, s, kind, route, n_script):
    """op 13 with w = 1 and sigma_y2 = s2 of the twin against op 12: fh_amm and a 6-iteration solve under torch.equal, on the
    fused kernel, on the forced chain and on the shape that only has the chain"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    _env(monkeypatch, route)
    So = S // s
    _orc, hip = srt._cov_pair(S, n_script, tmp_path_factory, dev)
    wop, cop = _wop(S, s, kind, dev, noise_map=np.ones((So, So))), bt._op(S, s, kind, dev)
    assert bool((wop.weights == 1).all()) and bt._route(cop, 0) == int((S, s) in FUSED)
    p12, k12 = _problem(cop, hip, _sigma_y2(cop))
    p13, k13 = _problem(wop, hip, _sigma_y2(cop))
    assert (p12.op, p13.op) == (12, 13) and p13.mask and not p12.mask and p13.m == p12.m == 2 * n_script
    for f in ("ntaps", "ntaps2", "halo", "halo2", "stride", "fold_sym", "sigma_y2", "use_dct"):
        assert getattr(p13, f) == getattr(p12, f), f
    shape = (1, 3 * wop.nframes, So, So)
    u, b = inputs.randn(shape, 21).to(dev), inputs.randn(shape, 22).to(dev)
    assert torch.equal(_amm(hip, p13, u), _amm(hip, p12, u))
    sw, iw = mb._cg(hip, p13, b, 1e-300, 6)
    sc, ic = mb._cg(hip, p12, b, 1e-300, 6)
    assert iw.niter == ic.niter == 6 and iw.b_norm == ic.b_norm and iw.residual_norm == ic.residual_norm
    assert bool(torch.isfinite(sw).all()) and torch.equal(sw, sc)


@pytest.mark.parametrize("route", ["fused", "chain"])
@pytest.mark.parametrize("n_script", [0, 4])
def test_one_frame_equals_op_10_bitwise(dev, tmp_path_factory, monkeypatch, n_script, route):
    """K = 1 is weighted_sr on its tap list (FH_NO_FOLD=1 keeps the rank-1 PSF off the rectangular bases), map N3: the same
    bits from fh_amm and from six iterations"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
    from free_hunch_amd.measurements import get_operator
    monkeypatch.setenv("FH_NO_FOLD", "1")
    _env(monkeypatch, route)
    S, s = 64, 4
    So = S // s
    _orc, hip = srt._cov_pair(S, n_script, tmp_path_factory, dev)
    wop = _wop(S, s, "one", dev, noise_map=noise_map_n3(So))
    one = get_operator(name="weighted_sr", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), scale_factor=s, kernel=PSF7,
                       noise_map=noise_map_n3(So))
    assert torch.equal(wop.weights, one.weights)
    p13, k13 = _problem13(wop, hip)
    p10, k10 = _problem(one, hip, _solver_sigma_y2(one))
    assert p10.op == 10 and p10.sigma_y2 == 1.0
    u, b = inputs.randn((1, 3, So, So), 23).to(dev), inputs.randn((1, 3, So, So), 24).to(dev)
    assert torch.equal(_amm(hip, p13, u), _amm(hip, p10, u))
    s13, i13 = mb._cg(hip, p13, b, 1e-300, 6)
    s10, i10 = mb._cg(hip, p10, b, 1e-300, 6)
    assert i13.niter == i10.niter == 6 and i13.residual_norm == i10.residual_norm and torch.equal(s13, s10)


# ---------------------------------------------------------------- 2. fused = chain, bit for bit
@pytest.mark.parametrize("n_script", [0, 4])
@pytest.mark.parametrize("S,s,kind", SHAPES[:3])
def test_fused_route_equals_the_chain_bit_for_bit(dev, tmp_path_factory, monkeypatch, S, s, kind, n_script):
    """fh_amm of op 13 with map F3: the WEIGHTED epilogue of k_conv_dec_frames against k_mask behind every frame's pass"""
    _orc, hip = srt._cov_pair(S, n_script, tmp_path_factory, dev)
    op = _wop(S, s, kind, dev)
    assert (bt._route(op, 0), bt._route(op, 1)) == (1, 1)
    prob, keep = _problem13(op, hip)
    u = inputs.randn(tuple(op.out_shape), 14).to(dev)
    _env(monkeypatch, "fused")
    fused = _amm(hip, prob, u)
    _env(monkeypatch, "chain")
    chain = _amm(hip, prob, u)
    torch.cuda.synchronize()
    assert torch.equal(fused, chain) and bool(torch.isfinite(fused).all()) and float((fused - u).abs().max()) > 0


# ---------------------------------------------------------------- 3. one application of A_mm against the reference
def _ref_system(ref, cov_dot, w, shape):
    def A_ref(u):
        u = u.reshape(shape)
        return (u + w * ref.fwd(cov_dot(ref.adj(w * u)))).flatten()
    return A_ref


def _amm_case(dev, tmp_factory, S, s, kind, n_script):
    orc, hip = srt._cov_pair(S, n_script, tmp_factory, dev)
    op = _wop(S, s, kind, dev)
    prob, keep = _problem13(op, hip)
    K, shape = op.nframes, tuple(op.out_shape)
    assert prob.stride == s and prob.m == 2 * n_script and prob.use_dct == 1 and prob.ntaps2 == K
    w = op.weights.cpu()
    A_ref = _ref_system(Ref(op), orc.denoiser_cov_vector_dot, w, shape)
    u, v = inputs.randn(shape, 21).to(dev), inputs.randn(shape, 22).to(dev)
    au, av = _amm(hip, prob, u), _amm(hip, prob, v)
    ref = A_ref(u.cpu().flatten()).reshape(shape)
    err = maxabs(au, ref) / float(ref.abs().max())
    l, r = float((u * av).sum()), float((au * v).sum())
    print(f"amm op=13 S={S} s={s} K={K} m={prob.m}: {err:.2e}, symmetry {abs(l - r) / max(abs(l), 1.0):.2e}", flush=True)
    assert err <= 1e-8
    assert abs(l - r) <= 1e-9 * max(abs(l), 1.0)
    zero = op.weights == 0
    assert int(zero.sum()) > 0 and torch.equal(au[zero], u[zero])  # A_mm(u) = u exactly where w = 0


@pytest.mark.parametrize("n_script", [0, 4])
@pytest.mark.parametrize("S,s,kind", SHAPES)
def test_amm_vs_reference_system(dev, tmp_path_factory, S, s, kind, n_script):
    """fh_amm with op = 13 and map F3 against u + W fwd(C(adj(W u))) on the shipped DCT prior cut to S, m = 0 and m = 8: 1e-8 of
    max|ref| and symmetry to 1e-9, the bars of test_burst_sr_gpu.test_amm_vs_reference_system"""
    _amm_case(dev, tmp_path_factory, S, s, kind, n_script)


def test_amm_vs_reference_system_at_the_real_size(dev, tmp_path_factory):
    _amm_case(dev, tmp_path_factory, 256, 4, "int", 0)  # K = 16


def test_amm_identity_prior(dev):
    from free_hunch_amd import covariance as hc
    S, s = 64, 4
    op = _wop(S, s, "four", dev)
    cov = hc.ScalarCovariance(0.7, 3 * S * S, dev)
    prob, keep = _problem13(op, cov)
    assert prob.use_dct == 0 and prob.ntaps2 == 4 and not prob.fold_fwd_w
    u = inputs.randn(tuple(op.out_shape), 24).to(dev)
    want = _ref_system(Ref(op), lambda t: 0.7 * t, op.weights.cpu(), tuple(op.out_shape))(u.cpu()).reshape(op.out_shape)
    got = _amm(cov, prob, u)
    assert maxabs(got, want) <= 1e-8 * float(want.abs().max())
    assert torch.equal(got[op.weights == 0], u[op.weights == 0])


# ---------------------------------------------------------------- 4. consistency with the device's own op 12
@pytest.mark.parametrize("S,s,kind", [(256, 4, "four"), (96, 3, "frac")])
def test_weighted_amm_is_consistent_with_op_12(dev, tmp_path_factory, S, s, kind):
    """op 13 against the restatement u + w (A12(w u) - s2 w u) from the device's own op 12: the two differ in products with w and
    one subtraction, 1e-12 of max|ref|"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    wop, cop = _wop(S, s, kind, dev), bt._op(S, s, kind, dev)
    s2 = _sigma_y2(cop)
    p13, k13 = _problem13(wop, hip)
    p12, k12 = _problem(cop, hip, s2)
    u = inputs.randn(tuple(wop.out_shape), 31).to(dev)
    got = _amm(hip, p13, u)
    ref = _weighted_ref(lambda t: _amm(hip, p12, t.contiguous()), wop.weights, s2, u)
    err = maxabs(got, ref) / float(ref.abs().max())
    print(f"op 13 against op 12 S={S} s={s} K={wop.nframes}: {err:.2e}", flush=True)
    assert err <= 1e-12
    assert torch.equal(got[wop.weights == 0], u[wop.weights == 0])


# ---------------------------------------------------------------- 5. the solve
def _weighted_solve_inputs(op, S, s):
    """test_burst_sr_gpu._solve_inputs (same seeds) with the measurement noise scaled per entry by the operator's map and zero
    where it is inf: (ref, w, y, x0_mean, b = w (y - fwd(x0_mean)) flattened), on the CPU"""
    So, K = S // s, op.nframes
    ref = Ref(op)
    sig, w = op.noise_map.cpu(), op.weights.cpu()
    x_true = inputs.smooth_image(S, 31).to(F64)
    noise = torch.where(w > 0, sig, torch.zeros_like(sig)) * inputs.randn((1, 3 * K, So, So), 32)
    y = torch.where(w > 0, ref.fwd(x_true) + noise, torch.zeros_like(noise))
    x0_mean = x_true + 0.05 * inputs.randn((1, 3, S, S), 33)
    return ref, w, y, x0_mean, (w * (y - ref.fwd(x0_mean))).flatten()


SIX = [(64, 4, "four", {}), (96, 3, "frac", {}), (64, 2, "int", dict(frame_sigmas=(0.02, 0.05, 0.1, 0.3), mosaic="rggb"))]


@pytest.mark.parametrize("S,s,kind,noise", SIX, ids=["64-4-F3", "96-3-F3", "64-2-sigmas-rggb"])
def test_six_iterations_vs_oracle_cg(dev, tmp_path_factory, S, s, kind, noise):
    """six forced iterations on the whitened system on both sides agree to 1e-5 of max|mat|"""
    from oracle import fh_oracle as fo
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda
    orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    op = _wop(S, s, kind, dev, **noise)
    ref, w, y, x0_mean, b = _weighted_solve_inputs(op, S, s)
    m6h = solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, rtol=1e-300, maxiter=6)
    sol6, info6 = fo.cg(_ref_system(ref, orc.denoiser_cov_vector_dot, w, tuple(y.shape)), b, rtol=0.0, maxiter=6)
    m6o = ref.adj(w * sol6.reshape(y.shape))
    short = maxabs(m6o, m6h) / float(m6o.abs().max())
    print(f"weighted burst solve S={S} s={s} K={op.nframes}: six iterations {short:.2e}", flush=True)
    assert info6["niter"] == 6 and tuple(m6h.shape) == (1, 3, S, S)
    assert short <= 1e-5


def test_converged_solve_meets_its_tolerance(dev, tmp_path_factory):
    """(64, 4, K = 4, map F3, m = 0) at rtol = 1e-4: `optimal` below the 5000-iteration cap (the oracle's cg() on exactly this
    system stops `optimal` after 570 iterations), the true residual recomputed with an independent fh_amm is <= 1.05 rtol ||b||,
    and the solution and the pre-image of mat are exactly 0 where w = 0"""
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda
    S, s = 64, 4
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    op = _wop(S, s, "four", dev)
    _ref, _w, y, x0_mean, b = _weighted_solve_inputs(op, S, s)
    rtol, info_h = 1e-4, []
    solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, info_h, rtol=rtol)
    u_h = solve_customcuda.last_solution.clone()
    prob, keep = _problem13(op, hip)
    assert prob.m == 0 and tuple(u_h.shape) == tuple(y.shape)
    bd = b.reshape(y.shape).to(dev)
    res = float((bd - _amm(hip, prob, u_h)).norm())
    print(f"weighted burst solve rtol 1e-4: device {info_h[0]['niter']} it, true residual {res / float(bd.norm()):.3e} ||b||",
          flush=True)
    assert info_h[0]["optimal"] and 1 <= info_h[0]["niter"] < 5000
    assert res <= 1.05 * rtol * float(bd.norm())
    zero = op.weights == 0
    assert bool((u_h[zero] == 0).all()) and bool(((op.weights * u_h)[zero] == 0).all())


# ---------------------------------------------------------------- 7. the closed form
@pytest.mark.parametrize("S", [32, 20])
def test_permutation_burst_against_the_closed_form(dev, S):
    """1 x 1 PSFs [[1]], s = 2 and the K = 4 integer shifts: the frames sample disjoint phases, A is a permutation, and with a
    scalar covariance c the whitened system is diagonal, (1 + w_i^2 c) u_i = b_i with b = w (y - A x0):
    u_i = w_i (y - A x0)_i / (1 + w_i^2 c) and mat = A^T W u, solved to rtol = 1e-12.  The map is frame k = noise_map_n(So)
    (1 + 0.25 k), sigma 0.03 .. 0.182: condition number (1 + c / 0.03^2) / (1 + c / 0.182^2) = 33, below the 42 of
    test_heteroscedastic_denoising_against_the_closed_form, whose 1e-10 bars these are.  S = 32 fused (So = 16), S = 20 chain."""
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda
    from free_hunch_amd.covariance import ScalarCovariance
    s, c = 2, 0.3
    So = S // s
    nmap = np.stack([np.stack([noise_map_n(So) * (1 + 0.25 * k)] * 3) for k in range(4)])
    op = _wop(S, s, "int", dev, kernels=[np.array([[1.0]])], noise_map=nmap)
    assert op.nframes == 4 and all(t.n == 1 for t in op.frames) and bt._route(op, 0) == int(So % 16 == 0)
    x0 = inputs.smooth_image(S, 41).to(dev).to(F64)
    x1 = x0 + 0.2 * inputs.randn((1, 3, S, S), 42).to(dev)
    y = op.forward(x1, noiseless=True)
    ax0 = op._conv(x0)
    assert torch.equal(torch.sort(ax0.flatten())[0], torch.sort(x0.flatten())[0])  # A is a permutation
    info = []
    mat = solve_customcuda(op, y, x0, ScalarCovariance(c, 3 * S * S, dev, 0), 1.0, 1.0, info, rtol=1e-12)
    w = op.weights
    want_u = w * (y - ax0) / (1.0 + w * w * c)
    want_m = op._conv(w * want_u, adjoint=True)
    u = solve_customcuda.last_solution
    err_u, err_m = maxabs(u, want_u) / float(want_u.abs().max()), maxabs(mat, want_m) / float(want_m.abs().max())
    print(f"permutation burst S={S}: {info[0]['niter']} iterations, u {err_u:.2e}, mat {err_m:.2e}", flush=True)
    assert 1 <= info[0]["niter"] < 5000 and err_u <= 1e-10 and err_m <= 1e-10
    assert bool((u[w == 0] == 0).all())


# ---------------------------------------------------------------- 8. a uniform map is the scalar operator
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("S,s,kind", [(64, 4, "four"), (96, 3, "frac")])
def test_uniform_map_is_the_scalar_operator(dev, tmp_path_factory, S, s, kind, prior):
    """frame_sigmas = [0.05] * K against burst_sr with sigma_s = 0.05, both from x0 = 0 (`scipy_cg`; test_noise_map_gpu's
    test_uniform_map_is_the_scalar_operator explains why): the 6-iteration mats agree to 1e-5 of the max.  The reference's own
    two runs are 2.2e-10 / 4.1e-10 (DCT prior) and 2.6e-8 / 4.6e-8 (identity prior) apart at these two shapes.  No iteration
    counts: these systems take over a thousand iterations."""
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda
    if prior == "dct_diagonal":
        _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    else:
        hip = hc.CovarianceHessianBFGS(1, 80.0 ** 2, 3 * S * S, device=dev)
    K = _nframes(s, kind)
    wop, cop = _wop(S, s, kind, dev, frame_sigmas=[SIGMA_S] * K), bt._op(S, s, kind, dev)
    assert bool((wop.noise_map == SIGMA_S).all())
    _ref, y, x0_mean, _b = bt._solve_inputs(cop, S, s)
    y, x0_mean = y.to(dev), x0_mean.to(dev)
    mw = solve_customcuda(wop, y, x0_mean, hip, 1.0, 1.0, rtol=1e-300, scipy_cg=True, maxiter=6)
    mc = solve_customcuda(cop, y, x0_mean, hip, 1.0, 1.0, rtol=1e-300, scipy_cg=True, maxiter=6)
    dist = maxabs(mw, mc) / float(mc.abs().max())
    print(f"uniform map against burst_sr S={S} s={s} K={K} {prior}: 6-iteration mat distance {dist:.3e}", flush=True)
    assert float(mc.abs().max()) > 0 and dist <= 1e-5


# ---------------------------------------------------------------- 9. batched = single
def _three_maps(So, K):
    return [dict(noise_map=map_f3(So, K)), dict(frame_sigmas=(0.02, 0.05, 0.1, 0.3)[:K]), dict(noise_map=np.full((So, So), SIGMA_S))]


@pytest.mark.parametrize("route", ["fused", "chain"])
@pytest.mark.parametrize("n_script", [0, 4])
def test_batched_solve_equals_single(dev, tmp_path, monkeypatch, n_script, route):
    """fh_cg_solve_batched with op = 13 over 3 images with their own maps (F3, frame_sigmas, uniform), measurements and
    covariances against per-image solves by the rule of test_burst_sr_gpu.test_batched_solve_equals_single: identical iteration
    counts, `mat` within 1e-12 of max|mat|, and the images stop at different iterations"""
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda, solve_customcuda_batched
    _env(monkeypatch, route)
    S, s, nimg = 64, 4, 3
    So = S // s
    dv = torch.load(os.path.join(bt.DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
    torch.save(dv, tmp_path / "dct_variance.pt")
    ops, covs, ys, xs = [], [], [], []
    for b, noise in enumerate(_three_maps(So, 4)):
        op = _wop(S, s, "four", dev, slot=b, **noise)
        cov = hc.CovarianceHessianBFGSDCT(str(tmp_path), 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=b)
        if n_script:
            _run_script(cov, inputs.script(1300 + b, (1, 3, S, S), n_script, 80.0, sig_end=[20.0, 2.0, 0.5][b]), dev)
        else:
            x = inputs.randn((1, 3, S, S), 300 + b).to(dev) * 40.0
            cov.update_time_step(x, 80.0, [40.0, 25.0, 12.0][b], -x / 80.0 ** 2 * 0.5)
        x0 = inputs.smooth_image(S, 310 + b).to(dev)
        sig = torch.where(op.mask > 0, op.noise_map, torch.zeros_like(op.noise_map)).float()
        ys.append((op.forward(x0, noiseless=True) + sig * inputs.randn((1, 12, So, So), 320 + b, torch.float32).to(dev)) * op.mask.float())
        xs.append((0.3 * x0).to(F64))
        ops.append(op)
        covs.append(cov)
    assert all(c.famC.m == 2 * n_script for c in covs) and _problem13(ops[0], covs[0])[0].op == 13
    assert not torch.equal(ops[0].weights, ops[1].weights) and not torch.equal(ops[1].weights, ops[2].weights)
    sigma_t = 0.4  # rtol_func(0.4) = 9e-3
    infos_b = []
    mats_b = solve_customcuda_batched(ops, ys, xs, covs, 1.0, sigma_t, infos_b, exclusive=True)
    assert tuple(mats_b.shape) == (nimg, 3, S, S)
    n_b = [i["niter"] for i in infos_b]
    print(f"batched weighted burst solve m={2 * n_script} {route}: iterations {n_b}", flush=True)
    for b in range(nimg):
        info = []
        one = solve_customcuda(ops[b], ys[b], xs[b], covs[b], 1.0, sigma_t, info)
        assert infos_b[b]["niter"] == info[0]["niter"], (b, n_b, info[0])
        assert infos_b[b]["optimal"] and info[0]["optimal"]
        assert maxabs(mats_b[b:b + 1], one) <= 1e-12 * float(one.abs().max()), b
    assert min(n_b) < max(n_b), n_b  # an image finished first: the `done` skip ran


def test_batched_solve_refuses_different_psfs_and_factors(dev):
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda_batched
    S = 64
    covs = [hc.CovarianceHessianBFGS(1, 80.0 ** 2, 3 * S * S, device=dev, ctx_slot=b) for b in range(2)]
    z = torch.zeros(1, 3, S, S, dtype=F64, device=dev)
    sig = dict(frame_sigmas=[0.1] * 4)
    ops = [_wop(S, 4, "four", dev, slot=0, **sig), _wop(S, 4, "four", dev, slot=1, shifts=FOUR[:3] + [(2, 3)], **sig)]
    with pytest.raises(AssertionError, match="PSF"):
        solve_customcuda_batched(ops, [z, z], [z, z], covs, 1.0, 0.4)
    ops = [_wop(S, 4, "four", dev, slot=0, **sig), _wop(S, 2, "four", dev, slot=1, **sig)]
    with pytest.raises(AssertionError, match="scale_factor"):
        solve_customcuda_batched(ops, [z, z], [z, z], covs, 1.0, 0.4)


# ---------------------------------------------------------------- 10. no stale graph
@pytest.mark.parametrize("S,s,switch", [(80, 4, None), (64, 4, "0")])
def test_chain_graph_is_not_replayed_for_other_frame_offsets(dev, tmp_path_factory, monkeypatch, S, s, switch):
    """test_burst_sr_gpu's scenario on op 13: permuted ragged frames written into the same device buffers, with the same
    weights.  The struct and the batch table cannot tell the two bursts apart; the second solve equals, bit for bit, the solve of
    a freshly built operator with the permuted frames, and differs from the first."""
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda
    _env(monkeypatch, "fused" if switch is None else "chain")
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    a, b = _wop(S, s, None, dev, shifts=bt.RAGGED_A), _wop(S, s, None, dev, shifts=bt.RAGGED_B)
    fa, fb = a.frame_taps, b.frame_taps
    assert [t.n for t in a.frames] == [49, 64, 56] and [t.n for t in b.frames] == [49, 56, 64]
    assert (fa.n, fa.max_taps, fa.halo) == (fb.n, fb.max_taps, fb.halo) and fa.off.tolist() != fb.off.tolist()
    assert torch.equal(a.weights, b.weights)
    So = S // s
    y = inputs.randn((1, 9, So, So), 41).to(dev)
    x0 = inputs.smooth_image(S, 42).to(dev).to(F64)
    solve = lambda op: solve_customcuda(op, y, x0, hip, 1.0, 1.0, rtol=1e-300, maxiter=16).clone()  # noqa: E731
    before = bytes(_problem13(a, hip)[0])
    first = solve(a)
    for dst, src in ((fa.dy, fb.dy), (fa.dx, fb.dx), (fa.w, fb.w), (fa.off, fb.off)):  # the same buffers, the other burst
        dst.copy_(src)
    a.kernels, a.frames = b.kernels, b.frames
    torch.cuda.synchronize()
    assert bytes(_problem13(a, hip)[0]) == before
    second, fresh = solve(a), solve(b)
    assert torch.equal(second, fresh)
    assert not torch.equal(second, first) and bool(torch.isfinite(second).all())


@pytest.mark.parametrize("route", ["fused", "chain"])
def test_weights_overwritten_in_place_are_read_again(dev, tmp_path_factory, monkeypatch, route):
    """solve, overwrite the weights in place with another map, solve again: the cached graph holds the weights' pointer, not
    their values - the second solve equals, bit for bit, the solve of a freshly built operator with that map"""
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda
    _env(monkeypatch, route)
    S, s = 64, 4
    So = S // s
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    a, b = _wop(S, s, "four", dev), _wop(S, s, "four", dev, frame_sigmas=(0.02, 0.05, 0.1, 0.3), mosaic="grbg")
    y = inputs.randn((1, 12, So, So), 43).to(dev)
    x0 = inputs.smooth_image(S, 44).to(dev).to(F64)
    solve = lambda op: solve_customcuda(op, y, x0, hip, 1.0, 1.0, rtol=1e-300, maxiter=16).clone()  # noqa: E731
    before = bytes(_problem13(a, hip)[0])
    first = solve(a)
    for name in ("weights", "noise_map", "mask"):
        getattr(a, name).copy_(getattr(b, name))
    torch.cuda.synchronize()
    assert bytes(_problem13(a, hip)[0]) == before
    second, fresh = solve(a), solve(b)
    assert torch.equal(second, fresh)
    assert not torch.equal(second, first) and bool(torch.isfinite(second).all())


# ---------------------------------------------------------------- 11. refusals without a launch
def test_op13_refuses_bad_problems_without_launching(dev, tmp_path_factory):
    from free_hunch_amd import _lib
    S, s, nimg = 64, 4, 3
    So = S // s
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    op = _wop(S, s, "four", dev)  # K = 4 frames of 49 taps
    u = inputs.randn((1, 12, So, So), 61).to(dev)
    out = torch.full_like(u, 123.0)
    info = _lib.FhCgInfo()
    some = u.data_ptr()
    bad_off = torch.tensor([0, 49, 40, 147, 196], dtype=torch.int32, device=dev)  # not increasing: refused once read back
    long_off = torch.tensor([0, 50, 98, 147, 196], dtype=torch.int32, device=dev)  # a frame longer than halo2
    # op 12's list without ("mask", some) - a mask is what op 13 wants - plus the null mask and the next op code
    for field, value in (("stride", 1), ("stride", 0), ("stride", 5), ("stride", 3), ("stride", 8), ("ntaps2", 0), ("ntaps2", -1),
                         ("ntaps2", 17), ("halo2", 0), ("halo2", 1025), ("halo2", 48), ("ntaps", 3), ("ntaps", 197),
                         ("tap2_dy", None), ("tap2_dy", bad_off.data_ptr()), ("tap2_dy", long_off.data_ptr()),
                         ("tap2_dx", some), ("tap2_w", some), ("fold_fwd_w", some), ("fold_fwd_h", some), ("fold_inv_w", some),
                         ("fold_inv_h", some), ("fold_sym", 1), ("halo", 6), ("mask", None), ("op", 14)):
        prob, keep = _problem13(op, hip)
        setattr(prob, field, value)
        rc = hip.ctx.lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
        rc = hip.ctx.lib.fh_cg_solve(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), 1e-3, 0.0, 10, C.byref(info),
                                     _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())  # nothing was launched
    prob, keep = _problem13(op, hip)  # a batch of 3 with one null per->mask[i]
    ctx = _lib.Context.get(S, 3 * nimg, 0, slot=4323)
    b = inputs.randn((nimg, 12, So, So), 62).to(dev)
    outb = torch.full_like(b, 123.0)
    rtols = (C.c_double * nimg)(*([1e-3] * nimg))
    infos = (_lib.FhCgInfo * nimg)()
    for missing in range(nimg):
        per = _lib.FhBatch()
        per.nimg = nimg
        for i in range(nimg):
            per.D[i], per.r[i], per.B[i], per.M[i] = prob.D, prob.r, prob.B, prob.M
            per.mask[i] = None if i == missing else prob.mask
        rc = ctx.lib.fh_cg_solve_batched(ctx.h, C.byref(prob), C.byref(per), b.data_ptr(), outb.data_ptr(), rtols, 0.0, 10, infos,
                                         _lib.stream())
        assert rc == _lib.FH_EINVAL, (missing, rc)
    torch.cuda.synchronize()
    assert bool((outb == 123.0).all())


# ---------------------------------------------------------------- 12. the operator class on the device
@pytest.mark.parametrize("S,s,kind", [(64, 4, "four"), (60, 3, "int")])
def test_operator_class_on_the_device(dev, S, s, kind):
    wop, cop = _wop(S, s, kind, dev), bt._op(S, s, kind, dev)
    K, So = wop.nframes, S // s
    shape = (1, 3 * K, So, So)
    assert tuple(wop.noise_map.shape) == shape and wop.noise_map.dtype == F64 and wop.weights.device.type == "cuda"
    x = inputs.smooth_image(S, 3).to(dev)
    y = wop.forward(x, noiseless=True)
    assert tuple(y.shape) == shape and y.dtype == x.dtype
    assert torch.equal(y, cop.forward(x, noiseless=True) * wop.mask.to(x.dtype))
    torch.manual_seed(7)
    noisy = wop.forward(x)
    torch.manual_seed(7)  # ONE draw at the shape of the whole burst, scaled by the map, zero where it is inf
    sig = torch.where(wop.mask > 0, wop.noise_map, torch.zeros_like(wop.noise_map)).to(x.dtype)
    keep = wop.mask.to(x.dtype)
    assert torch.equal(noisy, (cop.forward(x, noiseless=True) + sig * torch.randn(*shape, dtype=x.dtype, device=dev)) * keep)
    assert bool((noisy[wop.mask == 0] == 0).all()) and not torch.equal(noisy, y)
    x64, v64 = inputs.randn((1, 3, S, S), 81).to(dev), inputs.randn(shape, 82).to(dev)
    ax = wop.forward(x64, noiseless=True)
    for adj in (wop.transpose(v64), wop.forward_adjoint(v64), wop.transpose(v64.reshape(1, -1), flatten=True)):
        lhs, rhs = float((ax * v64).sum()), float((x64 * adj).sum())
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs)), (lhs, rhs)
        assert torch.equal(adj, cop.transpose(wop.mask * v64))  # the adjoint is unweighted
    y2, flat = wop.forward(x, flatten=True, noiseless=True)
    assert tuple(flat.shape) == (1, 3 * K * So * So) and torch.equal(y2, y) and torch.equal(flat.reshape(shape), y)
    raw = _wop(S, s, kind, dev, frame_sigmas=[0.05] * K, mosaic="rggb")
    yr = raw.forward(x + 2.0, noiseless=True)  # a positive scene: every sampled site reads a non-zero value
    assert bool(((yr.reshape(K, 3, So, So) != 0).sum(1) == 1).all())  # exactly one channel per site and frame


# ---------------------------------------------------------------- 13. the lock-step sampler
def test_lockstep_weighted_burst_equals_per_image(dev, gold, tmp_path):
    """conditional_sampler_grouped(groups = 1) over two images with DIFFERENT maps (F3, and frame_sigmas on an rggb mosaic)
    against per-image conditional_sampler runs by the rule of test_lockstep_burst_equals_per_image: identical niter and k lists,
    outputs within 1e-3; Euler with 4 steps, nets.gauss_net, sigma_min = 0.5"""
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_grouped
    B, S, s = 2, 64, 4
    So = S // s
    torch.save(torch.from_numpy(gold("trajectories")["dct_variance64"]), tmp_path / "dct_variance.pt")
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(tmp_path, {})
    ops, ys, noise = [], [], []
    for b, src in enumerate(({}, dict(frame_sigmas=(0.02, 0.05, 0.1, 0.3), mosaic="rggb"))):
        op = _wop(S, s, "four", dev, slot=b, **src)
        ops.append(op)
        x0 = 0.5 * inputs.smooth_image(S, 70 + b).to(dev)
        sig = torch.where(op.mask > 0, op.noise_map, torch.zeros_like(op.noise_map)).float()
        ys.append((op.forward(x0, noiseless=True) + sig * inputs.randn((1, 12, So, So), 80 + b, torch.float32).to(dev)) * op.mask.float())
        noise.append(inputs.randn((1, 3, S, S), 90 + b, torch.float32))
    assert not torch.equal(ops[0].weights, ops[1].weights)
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
    print(f"lock-step weighted burst SR: iterations {[t['niter'] for t in tb[0]]} / {[t['niter'] for t in tb[1]]}", flush=True)


# ---------------------------------------------------------------- 14. the CLI
@pytest.mark.parametrize("route", ["sigmas_mosaic", "sensor"])
def test_cli_weighted_burst_sr(tmp_path, route):
    import PIL.Image
    sys.path.insert(0, ROOT)
    from bench import smooth_images
    import generate_conditional as gc
    data = tmp_path / "data"
    data.mkdir()
    for i, im in enumerate(smooth_images(2, 256, 7)):
        PIL.Image.fromarray(im.permute(1, 2, 0).numpy(), "RGB").save(data / f"img{i:08d}.png")
    np.save(tmp_path / "psf.npy", binomial_psf(13, 13))
    out = tmp_path / "out"
    extra = ["--frame_sigmas=0.02,0.05,0.1,0.3", "--mosaic=rggb"] if route == "sigmas_mosaic" else \
        ["--noise_gain=0.01", "--noise_read_sigma=0.01"]
    gc.main([f"--outdir={out}", f"--dataset_path={data}", "--synthetic_weights=ffhq", "--num_steps=3", "--solver=euler",
             "--sigma_min=0.5", "--total_images=2", "--max_batch_size=2", "--operator_name=weighted_burst_sr",
             f"--kernel_path={tmp_path / 'psf.npy'}", "--scale_factor=4", "--frame_shifts=0,0;0,2;2,0;2,2",
             "--conditioning_mechanism=online_covariance", "--image_base_covariance=dct_diagonal"] + extra)
    names = ["000000_000000.png", "000001_000000.png"]
    for folder in ("images", "cond_images"):
        assert sorted(os.listdir(out / folder)) == names, folder
        for n in names:
            im = PIL.Image.open(out / folder / n)
            assert im.mode == "RGB" and im.size == (256, 256) and np.asarray(im).std() > 0
    assert os.listdir(out / "forward_images") == []  # low-resolution measurements are not written, as for burst_sr
    lines = dict(line.split(": ") for line in open(out / "results.txt").read().strip().split("\n"))
    assert set(lines) == {"PSNR", "SSIM", "images"} and lines["images"] == "2"
