"""The float64 solver side (csrc/fh_kernels.hip) at image sides that are no multiple of 16.

fh_context_create admits every even side from 2 to 256, but every other GPU test of the solver runs at a multiple of 16
(16, 48, 64, 80, 96, 128, 256), where d = 3 S^2 is a whole number of 768-row blocks, S % 4 == 0 and S % 8 == 0: the tail
guards of the row loops, the guarded staging of k_gemm_f64 and the partial tiles of the convolution kernels never ran.

    S    d = 3 S^2                   what it exercises
    2    12                          (DCT only) one guarded 4-element staging segment cut after 2
    6    108                         less than one 128-row sweep of one block; image smaller than every tile; S = 2 mod 4
    20   1200   = 768 + 432          second block: three full 128-row sweeps, then 48 rows (24 live lanes)
    40   4800   = 6 * 768 + 192      GEMM K = one full 32-chunk + 8; one ragged output tile beyond column 32
    100  30000  = 39 * 768 + 48      S % 8 = 4: 32-wide tiles end with 4 live columns, 64-tall tiles with 36 rows;
                                     k_gram: 64 rows per block, 469 live blocks, the last with 48 rows
    250  187500 = 244 * 768 + 108    near the limit; S = 2 mod 4; 250 = 7 * 32 + 26;
                                     k_gram: 384 rows per block, the last live block has 108 rows

Every output buffer handed to an entry point is NaN before the call and is followed by a tail of 4096 sentinel doubles
that must be unchanged after it: an output that was not written and a write past a ragged edge both fail.  The convolution
kernels at these sides are in test_conv_circ_matches_a_direct_sum (tests/test_edge_cases.py),
test_conv_window_matches_the_direct_sums (tests/test_custom_psf_gpu.py) and the CHAIN cases of tests/test_burst_sr_gpu.py;
which kernel each shape reaches is held on the host by tests/test_conv_circ_plan.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import inputs
from test_hip_parity import _hip_op, _mk_pair, maxabs

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "free-hunch_amd", "data", "kernels")
TAIL = 4096
SENTINEL = -7.25e77


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Guarded:
    """An output buffer of `shape` filled with NaN, with TAIL sentinel doubles behind it in the same allocation."""

    def __init__(self, shape, dev, init=None):
        n = int(np.prod(shape))
        self.full = torch.full((n + TAIL,), float("nan"), dtype=F64, device=dev)
        self.full[n:] = SENTINEL
        self.out = self.full[:n].view(*shape)
        if init is not None:
            self.out.copy_(init)

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.full[-TAIL:] == SENTINEL).all()), (what, "wrote past the end of its output")
        assert not bool(torch.isnan(self.out).any()), (what, "left outputs unwritten")
        return self.out


def _prior(S, tmp):
    """dct_variance[c][i][j] = (1 + 0.1 c) / (1 + (i^2 + j^2) / (S^2 / 16)) as <tmp>/dct_variance.pt (no fixture is committed)"""
    i = torch.arange(S, dtype=F64)
    c = torch.arange(3, dtype=F64)
    dv = (1 + 0.1 * c)[:, None, None] / (1 + (i[None, :, None] ** 2 + i[None, None, :] ** 2) / (S * S / 16))
    torch.save(dv.contiguous(), os.path.join(str(tmp), "dct_variance.pt"))


# ---------------------------------------------------------------- 1. DCT
@pytest.mark.parametrize("planes", [3, 7])
@pytest.mark.parametrize("S", [2, 6, 20, 40, 100, 250])
def test_dct_matches_scipy_at_ragged_sides(dev, S, planes):
    """Context.dct2d forward, inverse and in place (k_gemm_f64 on guarded scalar loads: no side here is a multiple of 32)
    against scipy.fft.dctn at the bounds of test_dct_matches_scipy_and_roundtrips (tests/test_hip_parity.py):
    1e-12 max(1, max|ref|), round trip 1e-12, energy 1e-9."""
    import scipy.fft
    from free_hunch_amd import _lib
    ctx = _lib.Context.get(S, planes, 0)
    x = inputs.randn((planes, S, S), 7 + S + planes)
    xd = x.to(dev)
    ref = scipy.fft.dctn(x.numpy(), type=2, norm="ortho", axes=(-2, -1))
    bound = 1e-12 * max(1.0, np.abs(ref).max())
    g = Guarded((planes, S, S), dev)
    ctx.dct2d(xd, out=g.out)
    X = g.check("forward")
    e_f = maxabs(X, ref)
    g = Guarded((planes, S, S), dev)
    ctx.dct2d(X, out=g.out, inverse=True)
    e_b = maxabs(g.check("inverse"), x)
    energy = abs(float((X ** 2).sum()) - float((x ** 2).sum())) / float((x ** 2).sum())
    g = Guarded((planes, S, S), dev, init=xd)
    ctx.dct2d(g.out, out=g.out)
    e_i = maxabs(g.check("in place"), ref)
    print(f"dct2d S={S} planes={planes}: forward {e_f:.2e} round trip {e_b:.2e} in place {e_i:.2e} energy {energy:.2e} "
          f"(max|ref| {np.abs(ref).max():.2f})", flush=True)
    assert e_f < bound and e_i < bound
    assert e_b < 1e-12
    assert energy < 1e-9


@pytest.mark.parametrize("S,So", [(20, 5), (40, 10), (100, 25), (250, 125)])
def test_dct_rect_matches_matmul_at_ragged_sides(dev, S, So):
    """fh_dct_rect with random rectangular bases, forward ([S][So] bases, [So][So] planes -> [S][S]) and inverse ([So][S],
    [S][S] -> [So][So]), against P_h X P_w^T in NumPy float64, for 3 and for 7 planes, by the convention and the bound of
    test_dct_rect_matches_numpy_matmul (tests/test_custom_sr_gpu.py): 1e-12 max(1, max|ref|).  Odd So: the 16-byte staging
    loads give way to scalar ones; So = 5: a K range of one 4-element staging segment + 1."""
    from free_hunch_amd import _lib
    rng = np.random.default_rng(1000 * S + So)
    Pw_f, Ph_f = rng.standard_normal((S, So)) / np.sqrt(So), rng.standard_normal((S, So)) / np.sqrt(So)
    Pw_i, Ph_i = rng.standard_normal((So, S)) / np.sqrt(S), rng.standard_normal((So, S)) / np.sqrt(S)
    u, v = rng.standard_normal((7, So, So)), rng.standard_normal((7, S, S))
    ref_f, ref_i = Ph_f @ u @ Pw_f.T, Ph_i @ v @ Pw_i.T  # (broadcast over the planes)
    dv_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    for planes in (3, 7):
        ctx = _lib.Context.get(S, planes, 0)
        g = Guarded((planes, S, S), dev)
        ctx.dct_rect(dv_(u[:planes]), g.out, dv_(Pw_f), dv_(Ph_f), So)
        e_f = np.abs(g.check("forward").cpu().numpy() - ref_f[:planes]).max()
        g = Guarded((planes, So, So), dev)
        ctx.dct_rect(dv_(v[:planes]), g.out, dv_(Pw_i), dv_(Ph_i), So, inverse=True)
        e_i = np.abs(g.check("inverse").cpu().numpy() - ref_i[:planes]).max()
        print(f"dct_rect S={S} So={So} planes={planes}: forward {e_f / max(1.0, np.abs(ref_f).max()):.2e} inverse "
              f"{e_i / max(1.0, np.abs(ref_i).max()):.2e}", flush=True)
        assert e_f < 1e-12 * max(1.0, np.abs(ref_f[:planes]).max())
        assert e_i < 1e-12 * max(1.0, np.abs(ref_i[:planes]).max())


# ---------------------------------------------------------------- 2. representation apply
REP_M = [0, 1, 5, 8, 9, 33]  # the `m & ~7` body and its tail; column counts that do not fill the 4-wave x kColChunk sweep


@pytest.mark.parametrize("S", [6, 20, 40, 100, 250])
def test_rep_apply_at_ragged_sides(dev, S):
    """fh_rep_apply at d = 3 S^2 that is no multiple of the 768-row block (the `ok` tails of k_rep_dots / k_rep_apply2) against
    D z + r (B^T (M (B (r z)))) in torch float64 on the CPU, bound 1e-10 max|ref| - the one
    test_cov_apply_single_sweep_equals_two_pass_bitwise (tests/test_hip_parity256.py) holds fh_rep_apply to.
    fh_rep_apply_batched with 3 images equals the single calls bit for bit (test_rep_apply_batched_matches_single), and on
    set_exclusive(2) - where d % 768 != 0 must keep the two-pass kernels - the result is bitwise that of set_exclusive(0)
    with no time-out reported (test_cov_apply_single_sweep_equals_two_pass_bitwise)."""
    from free_hunch_amd import _lib
    d, nimg, mmax, ldm = 3 * S * S, 3, max(REP_M), 64
    assert d % 768 != 0
    ctx = _lib.Context.get(S, 3 * nimg, 64, slot=78)
    g = torch.Generator().manual_seed(100 * S + 1)
    Bs = [torch.randn(mmax, d, generator=g, dtype=F64) for _ in range(nimg)]
    Ds = [torch.rand(d, generator=g, dtype=F64) + 0.5 for _ in range(nimg)]
    rs = [torch.rand(d, generator=g, dtype=F64) + 0.5 for _ in range(nimg)]
    Ms = [torch.randn(ldm, ldm, generator=g, dtype=F64) for _ in range(nimg)]
    z = torch.randn(nimg, d, generator=g, dtype=F64)
    Bd, Dd, rd, Md = ([t.to(dev) for t in ts] for ts in (Bs, Ds, rs, Ms))
    zd = z.to(dev)
    worst = 0.0
    for m in REP_M:
        per = _lib.FhBatch()
        per.nimg = nimg
        Bm = [b[:m].contiguous() if m else None for b in Bd]  # column j at B + j d
        for i in range(nimg):
            per.D[i], per.r[i], per.M[i] = Dd[i].data_ptr(), rd[i].data_ptr(), Md[i].data_ptr()
            per.B[i] = Bm[i].data_ptr() if m else None
        singles = []
        for i in range(nimg):
            one = Guarded((d,), dev)
            ctx.rep_apply(Dd[i], rd[i], Bm[i], Md[i], zd[i].contiguous(), one.out, m)
            got = one.check(("single", m, i))
            ref = Ds[i] * z[i]
            if m:
                ref = ref + rs[i] * (Bs[i][:m].T @ (Ms[i][:m, :m] @ (Bs[i][:m] @ (rs[i] * z[i]))))
            err = maxabs(got, ref) / float(ref.abs().max())
            worst = max(worst, err)
            assert err < 1e-10, (m, i, err)
            singles.append(got)

        def batched():
            b = Guarded((nimg, d), dev)
            _lib.check(ctx.lib.fh_rep_apply_batched(ctx.h, C.byref(per), ldm, zd.data_ptr(), b.out.data_ptr(), d, m, _lib.stream()),
                       "fh_rep_apply_batched")
            return b.check(("batched", m))

        two_pass = batched()
        for i in range(nimg):
            assert torch.equal(two_pass[i], singles[i]), (m, i)
        ctx.set_exclusive(2)
        try:
            assert torch.equal(batched(), two_pass), m
            one = Guarded((d,), dev)
            ctx.rep_apply(Dd[0], rd[0], Bm[0], Md[0], zd[0].contiguous(), one.out, m)
            assert torch.equal(one.check(("exclusive", m)), singles[0]), m
            ctx.status()
        finally:
            ctx.set_exclusive(0)
    print(f"rep_apply S={S} d={d}: largest error over m in {REP_M} and {nimg} images {worst:.2e} max|ref|", flush=True)


# ---------------------------------------------------------------- 3. covariance updates against the oracle
COV_CASES = [(6, 6), (20, 6), (40, 6), (100, 6), (250, 4)]  # (S, n): n time + n space updates, a negative curvature pair at 3


@pytest.mark.parametrize("ci", range(len(COV_CASES)))
def test_covariance_vs_oracle_at_ragged_sides(dev, tmp_path, ci):
    """The scripted time / space updates and the assertions of test_covariance_vs_oracle (tests/test_hip_parity.py), kind
    dct_diagonal: predicted means and scores, denoiser_cov_vector_dot, the column counts, C (C^-1 z) = z and H (H^-1 z) = z
    (1e-7, as there), everything else at that test's 1e-8 relative.  k_gram, k_gram_reduce, k_invert_diag / k_forward_diag,
    k_space_prep / k_space_commit and the dot kernels at d that their row blocks do not divide; every other case on
    set_exclusive(2)."""
    S, n = COV_CASES[ci]
    meta = dict(kind="dct_diagonal", shape=(1, 3, S, S), kw={}, sigma0=80.0, n=n, neg=3, only_cov=False)
    _prior(S, tmp_path)
    orc, hip = _mk_pair(meta, str(tmp_path), dev)
    hip.ctx.set_exclusive(2 * (ci % 2))
    worst = dict(mean=0.0, score=0.0, apply=0.0, inverse=0.0)
    try:
        steps = inputs.script(900 + ci, meta["shape"], n, meta["sigma0"], meta["neg"])
        probe = inputs.randn(meta["shape"], 950 + ci)
        tol = 1e-8
        for si, (what, a) in enumerate(steps):
            if what == "time":
                mo, so = orc.update_time_step(a["x"], a["sigma"], a["sigma_next"], a["score"], only_covariance=False)
                mh, sh = hip.update_time_step(a["x"].to(dev), a["sigma"], a["sigma_next"], a["score"].to(dev), only_covariance=False)
                sc = max(1.0, float(mo.abs().max()))
                worst["mean"], worst["score"] = max(worst["mean"], maxabs(mh, mo) / sc), max(worst["score"], maxabs(sh, so) / sc)
                assert maxabs(mh, mo) < tol * sc, (si, "mean")
                assert maxabs(sh, so) < tol * sc, (si, "score")
            else:
                orc.update_space_step(a["m0"], a["m1"], a["sigma"], a["x"], a["xn"])
                hip.update_space_step(a["m0"].to(dev), a["m1"].to(dev), a["sigma"], a["x"].to(dev), a["xn"].to(dev))
            assert hip.k == orc.k
            zz = probe.to(dev).double().reshape(-1)
            for rep_a, rep_b, fam in ((hip.C, hip.Ci, hip.famC), (hip.H, hip.Hi, hip.famH)):
                t_ = hip._apply(rep_b, fam, zz, torch.empty_like(zz))
                back = hip._apply(rep_a, fam, t_, torch.full_like(zz, float("nan")))
                worst["inverse"] = max(worst["inverse"], maxabs(back, zz) / float(zz.abs().max()))
                assert maxabs(back, zz) < 1e-7 * float(zz.abs().max()), (si, "inverse consistency", fam is hip.famC)
            ro = orc.denoiser_cov_vector_dot(probe)
            rh = hip.denoiser_cov_vector_dot(probe.to(dev))
            worst["apply"] = max(worst["apply"], maxabs(rh, ro) / max(1.0, float(ro.abs().max())))
            assert maxabs(rh, ro) < tol * max(1.0, float(ro.abs().max())), (si, "apply")
        assert hip.k == orc.k and hip.famC.m > 0
    finally:
        hip.ctx.set_exclusive(0)
        print(f"covariance S={S} n={n} k={hip.k}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()), flush=True)


# ---------------------------------------------------------------- 4. the whole system and CG
def _oracle_op(name, S, mask):
    import scipy.io
    from oracle import fh_oracle as fo
    if name == "inpainting":
        return fo.OracleOperator(name, (1, 3, S, S), 0.1, mask=mask)
    if name == "gaussian_blur":
        k = np.load(os.path.join(KERNELS, "gaussian_ks61_std3.0.npy"))
        oop = fo.OracleOperator(name, (1, 3, S, S), 0.1, kernel=k, otf_double=True)
        oop.pre_calculated = fo.pre_calculate(torch.zeros(1, 3, S, S, dtype=F64), oop._k(), 1)
        return oop
    k = scipy.io.loadmat(os.path.join(KERNELS, "kernels_bicubicx234.mat"))["kernels"][0, 2].astype(np.float64)
    oop = fo.OracleOperator(name, (1, 3, S, S), 0.1, kernel=k, scale_factor=4, otf_double=True)
    oop.pre_calculated = fo.pre_calculate(torch.zeros(1, 3, S // 4, S // 4, dtype=F64), oop._k(), 4)
    return oop


def _updated_pair(S, tmp, dev, seed, slot=0, oracle=True):
    """oracle and device covariance (dct_diagonal, the prior of _prior) after 4 scripted updates: m = 4 columns"""
    from oracle import fh_oracle as fo
    from free_hunch_amd import covariance as hc
    d = 3 * S * S
    orc = fo.make_covariance("dct_diagonal", str(tmp), 80.0 ** 2, d) if oracle else None
    hip = hc.CovarianceHessianBFGSDCT(str(tmp), 80.0 ** 2, d, device=dev, use_precalculated_info=True, ctx_slot=slot)
    for what, a in inputs.script(seed, (1, 3, S, S), 2, 80.0):
        for cov, to in ((orc, lambda t: t), (hip, lambda t: t.to(dev))):
            if cov is None:
                continue
            if what == "time":
                cov.update_time_step(to(a["x"]), a["sigma"], a["sigma_next"], to(a["score"]))
            else:
                cov.update_space_step(to(a["m0"]), to(a["m1"]), a["sigma"], to(a["x"]), to(a["xn"]))
    assert hip.famC.m == 4 and (orc is None or hip.k == orc.k)
    return orc, hip


def _amm(ctx, prob, u):
    from free_hunch_amd import _lib
    g = Guarded(tuple(u.shape), u.device)
    _lib.check(ctx.lib.fh_amm(ctx.h, C.byref(prob), u.data_ptr(), g.out.data_ptr(), _lib.stream()), "fh_amm")
    return g.check("fh_amm")


@pytest.mark.parametrize("name,S", [("inpainting", 100), ("gaussian_blur", 100), ("super_resolution", 100), ("gaussian_blur", 250)])
def test_system_and_cg_at_ragged_sides(dev, tmp_path, name, S):
    """fh_amm and fh_cg_solve with the operators of test_operators_vs_reference_golden / test_cg_full_size_residual_property at
    sides that are no multiple of 16, after 4 scripted covariance updates (m = 4):
      * fh_amm against the oracle's system(op, y, x0_mean, cov) applied to a seeded u (blur OTFs in complex128): 1e-8 max|ref|,
        and <u, A v> = <A u, v> to 1e-9 - the fh_amm bounds of the ops 3 .. 12 tests (test_amm_window_vs_oracle_covariance);
      * fh_cg_solve at rtol 1e-6 under the 5000-iteration cap: optimal, and the true residual recomputed with an independent
        fh_amm is <= 1.05 rtol ||b|| (test_cg_full_size_residual_property).
    gaussian_blur runs its folded bases on k_gemm_f64 (the symmetric passes need S % 128 == 0), super_resolution (So = 25; the
    oracle's operator accepts the side) k_conv_direct and k_conv_tile with zero insertion, inpainting k_mask and the dense
    DCT passes."""
    from oracle import fh_oracle as fo
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    _prior(S, tmp_path)
    orc, hip = _updated_pair(S, tmp_path, dev, 4300 + S)
    mask = fo.random_mask(S, (0.6, 0.8), np.random.default_rng(17)) if name == "inpainting" else None
    op, oop = _hip_op(name, S, dev, mask), _oracle_op(name, S, mask)
    So = S // 4 if name == "super_resolution" else S
    shape = (1, 3, So, So)
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.m == 4 and prob.use_dct == 1 and prob.op == {"inpainting": 0, "gaussian_blur": 1, "super_resolution": 2}[name]
    A_mm, _b, _back, _shape = fo.system(oop, torch.zeros(shape, dtype=F64), torch.zeros(1, 3, S, S, dtype=F64), orc)
    ctx = hip.ctx
    u, v = inputs.randn(shape, 21).to(dev).contiguous(), inputs.randn(shape, 22).to(dev).contiguous()
    au, av = _amm(ctx, prob, u), _amm(ctx, prob, v)
    ref = A_mm(u.cpu().flatten()).reshape(shape)
    err = maxabs(au, ref) / float(ref.abs().max())
    l, r = float((u * av).sum()), float((au * v).sum())
    sym = abs(l - r) / max(abs(l), 1.0)
    b = inputs.randn(shape, 5).to(dev).contiguous()
    sol = Guarded(shape, dev)
    info = _lib.FhCgInfo()
    rtol = 1e-6
    _lib.check(ctx.lib.fh_cg_solve(ctx.h, C.byref(prob), b.data_ptr(), sol.out.data_ptr(), rtol, 0.0, 5000, C.byref(info),
                                   _lib.stream()), "fh_cg_solve")
    x = sol.check("fh_cg_solve")
    res = float((b - _amm(ctx, prob, x.contiguous())).norm()) / float(b.norm())
    print(f"system {name} S={S}: amm {err:.2e} max|ref|, symmetry {sym:.2e}, cg {info.niter} iterations, true residual "
          f"{res:.3e} ||b||", flush=True)
    assert err <= 1e-8
    assert sym <= 1e-9
    assert info.optimal == 1 and 1 <= info.niter < 5000
    assert res <= 1.05 * rtol


def test_batched_cg_equals_single_solves_at_a_ragged_side(dev, tmp_path):
    """fh_cg_solve_batched with 3 images at S = 100 (gaussian_blur on its folded bases, m = 4) against three fh_cg_solve calls
    by the rule of test_batched_cg_with_a_finished_image (tests/test_edge_cases.py): identical iteration counts and flags,
    solutions within 1e-12 max(1, max|single|).  The middle image has a zero right-hand side and stops at once: at this side
    the rows of an image (300) are no multiple of the 32 / 64 rows of a k_gemm_f64 tile, so tiles of the first DCT pass hold
    rows of a finished and of a running image.  (A k_gemm_f64 that skips such a tile by the image of its first row alone
    leaves rows 600 .. 607 of the third image stale: that image then ran into the 400-iteration cap instead of stopping
    after 25.)"""
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S, nimg = 100, 3
    d = 3 * S * S
    _prior(S, tmp_path)
    covs = [_updated_pair(S, tmp_path, dev, 100 + i, slot=i + 1, oracle=False)[1] for i in range(nimg)]
    op = _hip_op("gaussian_blur", S, dev)
    b = torch.stack([inputs.randn((d,), 40).to(dev), torch.zeros(d, dtype=F64, device=dev), inputs.randn((d,), 42).to(dev)])
    singles, keeps = [], []
    for i in range(nimg):
        prob, keep = _problem(op, covs[i], _sigma_y2(op))
        sol = Guarded((d,), dev)
        info = _lib.FhCgInfo()
        ctx = covs[i].ctx
        _lib.check(ctx.lib.fh_cg_solve(ctx.h, C.byref(prob), b[i].contiguous().data_ptr(), sol.out.data_ptr(), 1e-5, 0.0, 400,
                                       C.byref(info), _lib.stream()), "cg")
        singles.append((sol.check(("single", i)), info.niter, info.optimal))
        keeps.append(keep)
    bctx = _lib.Context.get(S, 3 * nimg, 0, slot=6100)
    shared, keep0 = _problem(op, covs[0], _sigma_y2(op))
    per = _lib.FhBatch()
    per.nimg = nimg
    for i, cov in enumerate(covs):
        per.D[i], per.r[i], per.B[i], per.M[i] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(), cov.famC.B.data_ptr(),
                                                  cov.C.M_dev.data_ptr())
    sol = Guarded((nimg, d), dev)
    infos = (_lib.FhCgInfo * nimg)()
    rt = (C.c_double * nimg)(*([1e-5] * nimg))
    _lib.check(bctx.lib.fh_cg_solve_batched(bctx.h, C.byref(shared), C.byref(per), b.data_ptr(), sol.out.data_ptr(), rt, 0.0, 400,
                                            infos, _lib.stream()), "cg batched")
    got = sol.check("fh_cg_solve_batched")
    errs = [float((got[i] - singles[i][0]).abs().max()) / max(1.0, float(singles[i][0].abs().max())) for i in range(nimg)]
    print(f"batched cg S={S}: iterations {[infos[i].niter for i in range(nimg)]} (single {[s[1] for s in singles]}), "
          f"difference {max(errs):.2e}", flush=True)
    for i in range(nimg):
        assert infos[i].niter == singles[i][1] and infos[i].optimal == singles[i][2], (i, infos[i].niter, singles[i][1])
        assert errs[i] <= 1e-12, i
    assert infos[1].niter == 1 and not infos[1].optimal
    assert min(infos[0].niter, infos[2].niter) > 1
