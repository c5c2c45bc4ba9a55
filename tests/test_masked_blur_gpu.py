"""Deblurring with a validity mask on the device: A = M B (fh_problem.op = 5: the fields of op 1, op = 6: those of op 4, both
with a mask), from the kernels' masked epilogues up to the CLI.

The oracle knows the unmasked blur only: `fo.system` of OracleOperator("gaussian_blur", kernel=psf, otf_double=True) gives
A0(u) = s2 u + B C B^T u, and the masked operator is restated from it as  s2 u + M (A0(M u) - s2 M u)."""
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
SHIPPED = {"gaussian": "gaussian_ks61_std3.0.npy", "motion": "motion_ks61_std0.5.npy"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _psf(kind):
    """the PSF named `kind`; an array is a PSF of the caller's own (tests/test_ragged_ops_gpu.py: PSFs that fit a small side)"""
    if isinstance(kind, np.ndarray):
        return kind
    return disk_psf() if kind == "disk" else np.load(os.path.join(DATA, "kernels", SHIPPED[kind]))


def _mask_a(S=64):
    """The reference mask: a border of 8 times a 10 % random drop shared by the channels; 50.2 % of the pixels are kept."""
    m = np.zeros((1, S, S))
    m[:, 8: S - 8, 8: S - 8] = 1.0
    m = m * (np.random.default_rng(5).random((1, S, S)) >= 0.1)
    return np.ascontiguousarray(np.broadcast_to(m, (3, S, S)))


def _random_mask(S, seed):
    """10 % random zeros, per channel."""
    return (np.random.default_rng(seed).random((3, S, S)) >= 0.1).astype(np.float64)


def _mop(kind, S, dev, slot=0, **mask_kw):
    from free_hunch_amd.measurements import get_operator
    op = get_operator(name="masked_blur", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), kernel=_psf(kind), **mask_kw)
    op.ctx_slot = slot
    return op


def _cop(kind, S, dev, slot=0):
    from free_hunch_amd.measurements import get_operator
    op = get_operator(name="custom_blur", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), kernel=_psf(kind))
    op.ctx_slot = slot
    return op


def _oracle_op(S, kind):
    from oracle import fh_oracle as fo
    return fo.OracleOperator("gaussian_blur", (1, 3, S, S), SIGMA_S, kernel=_psf(kind), otf_double=True)


def _dct_cov(S, tmp, dev, slot=0):
    """The shipped DCT prior cut to S x S, as test_batched_window_solve_equals_single builds it."""
    from free_hunch_amd import covariance as hc
    data = DATA
    if S != 256:
        data = str(tmp)
        dv = torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
        torch.save(dv, os.path.join(data, "dct_variance.pt"))
    return hc.CovarianceHessianBFGSDCT(data, 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=slot)


def _cg(cov, prob, b, rtol, maxiter=5000):
    from free_hunch_amd import _lib
    sol = torch.full_like(b, float("nan"))
    info = _lib.FhCgInfo()
    _lib.check(cov.ctx.lib.fh_cg_solve(cov.ctx.h, C.byref(prob), b.data_ptr(), sol.data_ptr(), rtol, 0.0, maxiter, C.byref(info),
                                       _lib.stream()), "fh_cg_solve")
    return sol, info


def _plan_kernel(S, ntaps, halo):
    from free_hunch_amd import _lib
    out = (C.c_int32 * 6)()
    assert _lib.load().fh_conv_circ_plan(S, ntaps, halo, 3, 1, 0, out) == 0
    return out[0]


def _masked_ref(a0, mask, s2, u):
    """s2 u + M (A0(M u) - s2 M u) from an unmasked operator a0 (a callable on [1,3,S,S] tensors)."""
    mu = mask * u
    return s2 * u + mask * (a0(mu) - s2 * mu)


# ---------------------------------------------------------------- 1. an all-ones mask is the unmasked operator, bit for bit
def _twin_problems(kind, S, cov, dev):
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    mop, cop = _mop(kind, S, dev, mask=np.ones((S, S))), _cop(kind, S, dev)
    pm, keep_m = _problem(mop, cov, _sigma_y2(mop))
    pc, keep_c = _problem(cop, cov, _sigma_y2(cop))
    assert pm.op == pc.op + (4 if pc.op == 1 else 2) and pm.mask and not pc.mask
    for f in ("ntaps", "ntaps2", "halo", "halo2", "stride", "fold_sym", "sigma_y2", "m", "use_dct"):
        assert getattr(pm, f) == getattr(pc, f), f
    return pm, pc, (keep_m, keep_c, mop, cop)  # (the operators own the tap lists the problems point to)


@pytest.mark.parametrize("kind,S,prior,n_script,route", [
    ("gaussian", 128, "dct", 0, "fold_sym"),    # the mask rides in the inverse k_dct_sym pass's table, D in the forward one
    ("gaussian", 128, "dct", 4, "fold_sym"),    # m = 8: the table of the inverse pass alone
    ("gaussian", 64, "dct", 0, "fold_dense"),   # k_gemm_f64 passes, finished by k_mask
    ("gaussian", 64, "identity", 0, "conv1d"),  # the pair of 1-D passes, the last one with the masked epilogue
    ("motion", 64, "dct", 0, "taps"),           # the tap-list kernel's masked epilogue
    ("disk", 64, "dct", 0, "window"),           # k_conv_window's masked epilogue
])
def test_all_ones_mask_equals_the_unmasked_twin_bitwise(dev, tmp_path, kind, S, prior, n_script, route):
    from free_hunch_amd import covariance as hc
    cov = _dct_cov(S, tmp_path, dev) if prior == "dct" else hc.CovarianceHessianBFGS(1, 80.0 ** 2, 3 * S * S, device=dev)
    if n_script:
        _run_script(cov, inputs.script(1200, (1, 3, S, S), n_script, 80.0), dev)
    pm, pc, keep = _twin_problems(kind, S, cov, dev)
    assert pm.m == 2 * n_script
    if route == "fold_sym":
        assert pm.op == 5 and pm.fold_sym == 1 and pm.fold_inv_h
    elif route == "fold_dense":
        assert pm.op == 5 and pm.fold_sym == 0 and pm.fold_inv_h
    elif route == "conv1d":
        assert pm.op == 5 and pm.ntaps2 > 0 and not pm.fold_inv_h and _plan_kernel(S, pm.ntaps2, pm.halo2) in (0, 1)
    elif route == "taps":
        assert pm.op == 5 and pm.ntaps2 == 0 and pm.tap_dy and not pm.fold_inv_h
    else:
        assert pm.op == 6 and not pm.tap_dy
    u = inputs.randn((1, 3, S, S), 21).to(dev)
    assert torch.equal(_amm(cov, pm, u), _amm(cov, pc, u))
    b = inputs.randn((1, 3, S, S), 22).to(dev)
    sm, im = _cg(cov, pm, b, 1e-6)
    sc, ic = _cg(cov, pc, b, 1e-6)
    print(f"all-ones mask, {kind} S={S} {prior} m={pm.m} ({route}): {im.niter} iterations", flush=True)
    assert im.niter == ic.niter >= 1 and im.optimal == ic.optimal
    assert torch.equal(sm, sc)


def test_all_ones_mask_equals_the_unmasked_twin_on_the_tile8_kernel_256(dev, tmp_path):
    S = 256
    cov = _dct_cov(S, tmp_path, dev)
    pm, pc, keep = _twin_problems("motion", S, cov, dev)
    assert _plan_kernel(S, pm.ntaps, pm.halo) == 2  # k_conv_tile8
    u = inputs.randn((1, 3, S, S), 23).to(dev)
    assert torch.equal(_amm(cov, pm, u), _amm(cov, pc, u))


# ---------------------------------------------------------------- 2. one application against the oracle
@pytest.mark.parametrize("n_script", [0, 4])
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("kind", ["disk", "gaussian", "motion"])
def test_amm_with_mask_a_vs_oracle(dev, gold, tmp_path, kind, prior, n_script):
    """fh_amm (ops 5 / 6, 64 x 64, mask A) against the restatement from the oracle's unmasked system: 1e-8 of max|ref|,
    <u, A v> = <A u, v> to 1e-9 - the project's bounds for fh_amm - and out == sigma_y^2 u EXACTLY where the mask is 0."""
    from oracle import fh_oracle as fo
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 64
    orc, hip = _cov_pair(prior, S, str(tmp_path), dev, gold, n_script)
    mask = _mask_a(S)
    assert abs(mask.mean() - 0.502) < 5e-4
    op = _mop(kind, S, dev, mask=mask)
    s2 = _sigma_y2(op)
    prob, keep = _problem(op, hip, s2)
    assert prob.op == (6 if kind == "disk" else 5) and prob.m == 2 * n_script and prob.mask
    oop = _oracle_op(S, kind)
    x = inputs.smooth_image(S, 3).to(F64)
    A0, _b, _back, _shape = fo.system(oop, oop.forward(x), x, orc)
    a0 = lambda t: A0(t.flatten()).reshape(1, 3, S, S)  # noqa: E731
    mk = torch.from_numpy(mask)[None]
    u = inputs.randn((1, 3, S, S), 21)
    v = inputs.randn((1, 3, S, S), 22)
    au, av = _amm(hip, prob, u.to(dev)), _amm(hip, prob, v.to(dev))
    ref = _masked_ref(a0, mk, s2, u)
    err = maxabs(au, ref) / float(ref.abs().max())
    l, r = float((u.to(dev) * av).sum()), float((au * v.to(dev)).sum())
    print(f"amm masked {kind} {prior} m={prob.m}: {err:.2e}, symmetry {abs(l - r) / max(abs(l), 1.0):.2e}", flush=True)
    assert err <= 1e-8
    assert abs(l - r) <= 1e-9 * max(abs(l), 1.0)
    off = (mk == 0)
    assert torch.equal(au.cpu()[off], (s2 * u)[off])


# ---------------------------------------------------------------- 3. the masked operator against the device's unmasked one
@pytest.mark.parametrize("kind", ["gaussian", "motion"])
@pytest.mark.parametrize("S", [128, 256])
def test_masked_amm_is_consistent_with_the_unmasked_amm(dev, tmp_path, kind, S):
    """mask_border = -1 and 10 % random zeros at the sizes of the symmetric DCT passes (the Gaussian folds into them: the masks
    are the inverse pass's table; the motion PSF runs k_conv_tile8's masked epilogue) against the restatement from the device's
    own op = 1: the two differ in exact products with 0 / 1 and one subtraction, 1e-12 of max|ref|."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    cov = _dct_cov(S, tmp_path, dev)
    mop, cop = _mop(kind, S, dev, mask=_random_mask(S, 7 + S), mask_border=-1), _cop(kind, S, dev)
    assert mop.mask_border == (mop.taps.hy, mop.taps.hx) and 0.3 < float(mop.mask.mean()) < 0.9
    s2 = _sigma_y2(mop)
    pm, keep_m = _problem(mop, cov, s2)
    pc, keep_c = _problem(cop, cov, s2)
    assert (pm.op, pc.op) == (5, 1) and pm.fold_sym == pc.fold_sym == int(kind == "gaussian")
    u = inputs.randn((1, 3, S, S), 31).to(dev)
    got = _amm(cov, pm, u)
    ref = _masked_ref(lambda t: _amm(cov, pc, t.contiguous()), mop.mask, s2, u)
    err = maxabs(got, ref) / float(ref.abs().max())
    print(f"masked vs unmasked amm {kind} S={S}: {err:.2e}", flush=True)
    assert err <= 1e-12
    assert torch.equal(got[mop.mask == 0], (s2 * u)[mop.mask == 0])


# ---------------------------------------------------------------- 4. refusals before any launch
WINDOW_FIELDS = (("ntaps", 41 * 41 - 1), ("halo", 64 * 20 + 19), ("halo", 64 * 33 + 20), ("halo", -1), ("tap_w", None),
                 ("tap_dy", "some"), ("tap_dx", "some"), ("ntaps2", 1), ("tap2_dy", "some"), ("tap2_dx", "some"),
                 ("tap2_w", "some"), ("fold_fwd_w", "some"), ("fold_fwd_h", "some"), ("fold_inv_w", "some"),
                 ("fold_inv_h", "some"))


@pytest.mark.parametrize("kind", ["motion", "disk"])
def test_masked_ops_refuse_bad_problems_without_launching(dev, gold, tmp_path, kind):
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 64
    _orc, hip = _cov_pair("dct_diagonal", S, str(tmp_path), dev, gold, 0)
    op = _mop(kind, S, dev, mask=_mask_a(S))
    u = inputs.randn((1, 3, S, S), 61).to(dev)
    out = torch.full_like(u, 123.0)
    info = _lib.FhCgInfo()
    cases = [("mask", None), ("stride", 2), ("stride", 0), ("op", 7), ("op", -1)]
    if kind == "disk":
        cases += list(WINDOW_FIELDS)
    for field, value in cases:
        prob, keep = _problem(op, hip, _sigma_y2(op))
        assert prob.op == (6 if kind == "disk" else 5)
        setattr(prob, field, u.data_ptr() if value == "some" else value)
        rc = hip.ctx.lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
        rc = hip.ctx.lib.fh_cg_solve(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), 1e-3, 0.0, 10, C.byref(info),
                                     _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())  # nothing was launched


@pytest.mark.parametrize("kind", ["motion", "disk"])
def test_batched_solve_refuses_a_null_mask_without_launching(dev, gold, tmp_path, kind):
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S, nimg = 64, 3
    _orc, hip = _cov_pair("dct_diagonal", S, str(tmp_path), dev, gold, 0)
    op = _mop(kind, S, dev, mask=_mask_a(S))
    prob, keep = _problem(op, hip, _sigma_y2(op))
    ctx = _lib.Context.get(S, 3 * nimg, 0, slot=4321)
    b = inputs.randn((nimg, 3, S, S), 62).to(dev)
    out = torch.full_like(b, 123.0)
    rtols = (C.c_double * nimg)(*([1e-3] * nimg))
    infos = (_lib.FhCgInfo * nimg)()
    for missing in range(nimg):
        per = _lib.FhBatch()
        per.nimg = nimg
        for i in range(nimg):
            per.D[i], per.r[i], per.B[i], per.M[i] = prob.D, prob.r, prob.B, prob.M
            per.mask[i] = None if i == missing else prob.mask
        rc = ctx.lib.fh_cg_solve_batched(ctx.h, C.byref(prob), C.byref(per), b.data_ptr(), out.data_ptr(), rtols, 0.0, 10, infos,
                                         _lib.stream())
        assert rc == _lib.FH_EINVAL, (missing, rc)
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())


# ---------------------------------------------------------------- 5. the solve against the oracle's cg()
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("kind", ["disk", "motion", "gaussian"])
def test_masked_solve_vs_oracle_cg(dev, gold, tmp_path, kind, prior):
    """solve_customcuda on the masked system (64 x 64, mask A, sigma_s = 0.05) against fo.cg on its restatement: six iterations
    on both sides agree to 1e-5; at rtol = 1e-6 the device reports `optimal` below the 5000-iteration cap and the true residual
    of its solution, recomputed with an independent fh_amm, is <= 1.05 rtol ||b||.  The oracle's cg() needs, with the DCT prior /
    the identity prior: disk 594 / 26, motion 1272 / 92, Gaussian 2111 / 95 iterations - the cap is never why a case passes."""
    from oracle import fh_oracle as fo
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda
    S = 64
    orc, hip = _cov_pair(prior, S, str(tmp_path), dev, gold, 0)
    mask = _mask_a(S)
    mk = torch.from_numpy(mask)[None]
    op, oop = _mop(kind, S, dev, mask=mask), _oracle_op(S, kind)
    s2 = _sigma_y2(op)
    x_true = inputs.smooth_image(S, 31).to(F64)
    y_full = oop.forward(x_true, noise=inputs.randn((1, 3, S, S), 32))
    x0_mean = x_true + 0.05 * inputs.randn((1, 3, S, S), 33)
    A0, b0, back, _shape = fo.system(oop, y_full, x0_mean, orc)
    A_mm = lambda t: _masked_ref(lambda w: A0(w.flatten()).reshape(1, 3, S, S), mk, s2, t.reshape(1, 3, S, S)).flatten()  # noqa: E731
    b = (mk * b0.reshape(1, 3, S, S)).flatten()
    y = (mk * y_full).to(dev)
    m6h = solve_customcuda(op, y, x0_mean.to(dev), hip, 1.0, 1.0, rtol=1e-300, maxiter=6)
    sol6, info6 = fo.cg(A_mm, b, rtol=0.0, maxiter=6)
    m6o = back(mk.flatten() * sol6)
    short = maxabs(m6o, m6h) / float(m6o.abs().max())
    assert info6["niter"] == 6 and tuple(m6h.shape) == (1, 3, S, S)
    rtol = 1e-6
    info_h = []
    solve_customcuda(op, y, x0_mean.to(dev), hip, 1.0, 1.0, info_h, rtol=rtol)
    u_h = solve_customcuda.last_solution.clone()
    prob, keep = _problem(op, hip, s2)
    bd = b.reshape(1, 3, S, S).to(dev)
    res = float((bd - _amm(hip, prob, u_h)).norm())
    print(f"masked solve {kind} {prior}: short {short:.2e}; rtol 1e-6: device {info_h[0]['niter']} it, true residual "
          f"{res / float(bd.norm()):.3e} ||b||", flush=True)
    assert short <= 1e-5
    assert info_h[0]["optimal"] and 1 <= info_h[0]["niter"] < 5000
    assert res <= 1.05 * rtol * float(bd.norm())
    assert bool((u_h[mk.to(dev) == 0] == 0).all())


# ---------------------------------------------------------------- 6. the solve masks b itself
@pytest.mark.parametrize("kind", ["disk", "motion", "gaussian"])
def test_solve_masks_its_right_hand_side(dev, gold, tmp_path, kind):
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 64
    _orc, hip = _cov_pair("dct_diagonal", S, str(tmp_path), dev, gold, 0)
    op = _mop(kind, S, dev, mask=_mask_a(S))
    prob, keep = _problem(op, hip, _sigma_y2(op))
    b = inputs.randn((1, 3, S, S), 71).to(dev)
    assert float(b[op.mask == 0].abs().min()) > 0
    s_raw, i_raw = _cg(hip, prob, b, 1e-4)
    s_msk, i_msk = _cg(hip, prob, (op.mask * b).contiguous(), 1e-4)
    assert i_raw.niter == i_msk.niter >= 2 and i_raw.optimal and i_msk.optimal
    assert i_raw.b_norm == i_msk.b_norm and abs(i_raw.b_norm - float((op.mask * b).norm())) <= 1e-12 * i_raw.b_norm  # ||M b||
    assert torch.equal(s_raw, s_msk)
    assert bool((s_raw[op.mask == 0] == 0).all()) and float(s_raw.abs().max()) > 0


# ---------------------------------------------------------------- 7. batched solve = single solves
def _four_masks(kind, S):
    rng = np.random.default_rng(11)
    return [dict(mask=np.ones((S, S))),                                       # image 0: A = B, see below
            dict(mask=_mask_a(S)),
            dict(mask_border=-1),
            dict(mask=(rng.random((3, S, S)) >= 0.2).astype(np.float64), mask_border=3)]


@pytest.mark.parametrize("kind", ["disk", "motion"])
def test_batched_masked_solve_equals_single(dev, tmp_path, kind):
    """fh_cg_solve_batched with ops 6 / 5 for 4 images with four different masks against four fh_cg_solve calls, by the rule of
    test_batched_window_solve_equals_single: identical iteration counts, solutions to 1e-12 of max|mat|.  Image 0 has the
    all-ones mask and a right-hand side that is constant over the image - an eigenvector of B (its DC gain) and of the diagonal
    DCT-basis covariance - so its CG stops after one iteration and every kernel of the loop skips its planes from then on."""
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda, solve_customcuda_batched
    S, nimg = 64, 4
    dv = torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
    torch.save(dv, tmp_path / "dct_variance.pt")
    ops, covs, ys, xs = [], [], [], []
    for b, mask_kw in enumerate(_four_masks(kind, S)):
        op = _mop(kind, S, dev, slot=b, **mask_kw)
        cov = hc.CovarianceHessianBFGSDCT(str(tmp_path), 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=b)
        x = inputs.randn((1, 3, S, S), 300 + b).to(dev) * 40.0  # one time update each: distinct diagonals, no factor columns
        cov.update_time_step(x, 80.0, [40.0, 25.0, 12.0, 30.0][b], -x / 80.0 ** 2 * 0.5)
        x0 = inputs.smooth_image(S, 310 + b).to(dev)
        if b == 0:
            ys.append(torch.full((1, 3, S, S), 0.5, dtype=torch.float32, device=dev))
            xs.append(torch.zeros(1, 3, S, S, dtype=F64, device=dev))
        else:
            ys.append(op.forward(x0, noiseless=True) + (SIGMA_S * inputs.randn((1, 3, S, S), 320 + b, torch.float32).to(dev))
                      * op.mask.float())
            xs.append((0.3 * x0).to(F64))
        ops.append(op)
        covs.append(cov)
    assert len({float(o.mask.sum()) for o in ops}) == nimg and all(c.famC.m == 0 for c in covs)
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
    print(f"batched masked solve ({kind}): iterations {n_b}", flush=True)
    assert n_b[0] < min(n_b[1:]), n_b  # image 0 finished first: the `done` skip ran


def test_batched_masked_solve_refuses_different_psfs(dev):
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda_batched
    from free_hunch_amd.measurements import get_operator
    S = 64
    ops = [_mop("disk", S, dev, 0, mask_border=4),
           get_operator(name="masked_blur", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), kernel=disk_psf(radius=15.0),
                        mask_border=4)]
    covs = [hc.CovarianceHessianBFGS(1, 80.0 ** 2, 3 * S * S, device=dev, ctx_slot=b) for b in range(2)]
    z = torch.zeros(1, 3, S, S, dtype=F64, device=dev)
    with pytest.raises(AssertionError, match="PSF"):
        solve_customcuda_batched(ops, [z, z], [z, z], covs, 1.0, 0.4)


# ---------------------------------------------------------------- 8. the operator class on the device
@pytest.mark.parametrize("kind", ["disk", "motion", "gaussian"])
def test_operator_class_on_the_device(dev, kind):
    S = 64
    mop, cop = _mop(kind, S, dev, mask=_mask_a(S)), _cop(kind, S, dev)
    assert tuple(mop.mask.shape) == (1, 3, S, S) and mop.mask.device.type == "cuda"
    x = inputs.smooth_image(S, 3).to(dev)
    y = mop.forward(x, noiseless=True)
    assert tuple(y.shape) == (1, 3, S, S) and y.dtype == x.dtype
    assert torch.equal(y, mop.mask.to(x.dtype) * cop.forward(x, noiseless=True))
    x64, v64 = inputs.randn((1, 3, S, S), 81).to(dev), inputs.randn((1, 3, S, S), 82).to(dev)
    ax = mop.forward(x64, noiseless=True)
    for adj in (mop.transpose(v64), mop.forward_adjoint(v64)):
        lhs, rhs = float((ax * v64).sum()), float((x64 * adj).sum())
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs)), (lhs, rhs)
        assert torch.equal(adj, cop.transpose(mop.mask * v64))
    torch.manual_seed(5)
    yn = mop.forward(x)
    after_masked = torch.randn(4, device=dev)
    torch.manual_seed(5)
    cop.forward(x)
    assert torch.equal(after_masked, torch.randn(4, device=dev))  # the same RNG consumption as custom_blur
    kept = mop.mask > 0
    assert abs(float((yn - y)[kept].std()) - SIGMA_S) < 0.1 * SIGMA_S
    assert bool((yn[~kept] == 0).all()) and bool((y[~kept] == 0).all())
    y2, flat = mop.forward(x, flatten=True, noiseless=True)
    assert tuple(flat.shape) == (1, 3 * S * S) and torch.equal(y2, y)
    assert tuple(mop.get_kernel().shape) == (1, 1, 61, 61) and tuple(mop.pre_calculated[0].shape) == (1, 1, S, S)


# ---------------------------------------------------------------- 9. the lock-step sampler
def test_lockstep_masked_blur_equals_per_image(dev, gold, tmp_path):
    """conditional_sampler_grouped(groups = 1) over two disk-blurred images with DIFFERENT masks against per-image
    conditional_sampler runs by the rule of test_lockstep_window_blur_equals_per_image (identical niter and k lists, outputs
    within 1e-3), Euler with 4 steps and that test's denoiser, nets.gauss_net."""
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_grouped
    B, S = 2, 64
    torch.save(torch.from_numpy(gold("trajectories")["dct_variance64"]), tmp_path / "dct_variance.pt")
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(tmp_path, {})
    ops, ys, noise = [], [], []
    for b, mask_kw in enumerate((dict(mask=_mask_a(S)), dict(mask_border=-1))):
        op = _mop("disk", S, dev, slot=b, **mask_kw)
        ops.append(op)
        x0 = 0.5 * inputs.smooth_image(S, 70 + b).to(dev)
        ys.append((op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 3, S, S), 80 + b, torch.float32).to(dev))
                  * op.mask.float())
        noise.append(inputs.randn((1, 3, S, S), 90 + b, torch.float32))
    assert not torch.equal(ops[0].mask, ops[1].mask)
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
    print(f"lock-step masked blur: iterations {[t['niter'] for t in tb[0]]} / {[t['niter'] for t in tb[1]]}", flush=True)


# ---------------------------------------------------------------- 10. the CLI
def test_cli_masked_blur(tmp_path):
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
             "--sigma_min=0.5", "--total_images=2", "--max_batch_size=2", "--operator_name=masked_blur",
             f"--kernel_path={tmp_path / 'disk.npy'}", "--mask_border=-1", "--conditioning_mechanism=online_covariance",
             "--image_base_covariance=dct_diagonal"])
    names = ["000000_000000.png", "000001_000000.png"]
    for folder in ("images", "forward_images"):
        assert sorted(os.listdir(out / folder)) == names, folder
        for n in names:
            im = PIL.Image.open(out / folder / n)
            assert im.mode == "RGB" and im.size == (256, 256) and np.asarray(im).std() > 0
    for n in names:  # y = 0 in the band of the disk's reach (20 pixels) is coded as 128; inside, the blurred image is not flat
        fwd = np.asarray(PIL.Image.open(out / "forward_images" / n)).astype(np.int64)
        band = np.ones((256, 256), dtype=bool)
        band[20:236, 20:236] = False
        assert (fwd[band] == 128).all() and fwd[~band].std() > 0 and (fwd[20, 20:236] != 128).any()
    txt = open(out / "results.txt").read()
    assert "PSNR" in txt and "SSIM" in txt
