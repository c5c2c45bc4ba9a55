"""The operator systems of fh_problem.op 3 .. 12 at image sides that are no multiple of 16.

tests/test_ragged_sizes_gpu.py runs the whole system (fh_amm, fh_cg_solve, fh_cg_solve_batched) at ragged sides for ops 0, 1
and 2 only; every system-level test of colorization (3), window blur (4), masked blur (5, 6), folded SR (7), the noise-map
operators (8 .. 11) and burst SR (12) runs at S in {64, 96, 128, 256}.  amm_launch gives those operators routes of their own:
k_dct_rect with its per-image tables and p.Ap partials inside the system, k_channel_mix around the dense DCT, the masked
epilogues of k_conv1d / k_conv_tile8 / k_conv_window, a k_mask pass behind k_conv_tile / k_conv_direct / the dense folded
passes, k_mask over 3 So^2 measurements with So odd, k_cg_init_w / k_cg_step2_w - each with a `states` skip of finished images.

    S    So (s)               what it exercises beyond the table of test_ragged_sizes_gpu.py
    6    -                    colorization: pairs = 18, less than one block of k_channel_mix
    20   10 (2)               k_dct_rect: one 32 x 32 tile per plane, K = one chunk, every edge guarded
    36   9 (4), 12 (3)        odd So: scalar staging in k_dct_rect, k_mask over 243 doubles per image
    40   10 (4)               k_conv_window: two tiles across, the second with 8 live columns
    100  25 (4), 20 (5)       So = 25 odd: 3 So^2 = 1875 measurements, no multiple of 256; 4 x 4 k_dct_rect tiles, the last with
                              4 live rows / columns; k_conv_tile8 tiles end with 4 live columns, k_conv_window's with 36 rows
    250  125 (2), 25 (10)     8 x 8 k_dct_rect tiles, the last with 26 live rows; inverse pass A keeps a 32 x 258 slice resident
    60   20 (3)               burst SR on the chain route: K = 9 launches per image, each with its own `states` block

Sides the operators refuse by their own rules: custom_sr / weighted_sr need an 8 x 8 measurement, so (20, 4) (So = 5) is not
admitted.  It is replaced by (20, 2) - the same image side, So = 10 - and by (36, 4), the nearest admitted ragged side at
s = 4, So = 9 odd.  The oracle's blur / SR operators expand the PSF into an S x S array and raise where it is wider than the
image: below S = 61 the PSFs are the 9 x 13 binomial, the 9 x 9 and 21 x 21 disks and a 15 x 15 disk that fills its window
(a dense window at S = 40).  No ragged side reaches k_conv_dec / k_conv_up (they need So % 16 == 0 / S % 16 s == 0, hence
S % 16 == 0, held by tests/test_conv_circ_plan.py): every decimating tap-list pass here is k_conv_direct forward and
k_conv_tile with zero insertion back.

Every output handed to an entry point is a `Guarded` buffer: NaN before the call, with a sentinel tail that must be unchanged
after it.  The bounds are the project's own: fh_amm against the oracle 1e-8 max|ref| and symmetry 1e-9
(test_amm_window_vs_oracle_covariance), masked / weighted against the device's own twin 1e-12 max|ref|
(test_masked_amm_is_consistent_with_the_unmasked_amm), fh_cg_solve at rtol 1e-6 `optimal` under the 5000-iteration cap with a
true residual <= 1.05 rtol ||b|| (test_system_and_cg_at_ragged_sides), batched against single solves identical counts and
1e-12 max(1, max|single|) (test_batched_cg_with_a_finished_image)."""
import ctypes as C

import numpy as np
import pytest
import torch

import inputs
import test_burst_sr_gpu as bt
import test_custom_sr_gpu as srt
import test_masked_blur_gpu as mb
import test_noise_map_gpu as nm
from test_channel_ops_gpu import _col_op, _cov_pair, _oracle_amm
from test_custom_psf_host import disk_psf
from test_hip_parity import maxabs
from test_ragged_sizes_gpu import Guarded, _amm, _prior, _updated_pair

pytestmark = pytest.mark.gpu
F64 = torch.float64
RTOL = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def sparse_psf():
    """61 x 61 with about 10 % random non-zeros, normalised: a tap list too wide for k_conv_tile8's LDS (k_conv_tile)"""
    rng = np.random.default_rng(61)
    k = (rng.random((61, 61)) < 0.1) * rng.uniform(0.2, 1.0, (61, 61))
    k[30, 30] = k[0, 3] = k[60, 57] = k[5, 0] = k[55, 60] = 1.0  # the extents reach 30 in both axes
    return k / k.sum()


# blur PSFs by name: the shipped ones ("gaussian", "motion", "disk": mb._psf) and the two of this file
OWN_PSFS = {"disk15": disk_psf(radius=7.3, size=15), "sparse61": sparse_psf()}


def _k(kind):
    return OWN_PSFS.get(kind, kind)


def ragged_mask(S, seed):
    """0/1 per channel and pixel, about 60 % kept"""
    m = (np.random.default_rng(seed).random((3, S, S)) >= 0.4).astype(np.float64)
    assert 0.3 < m.mean() < 0.9
    return m


def ragged_noise_map(n, seed):
    """sigma per channel and pixel, uniform in 0.03 .. 0.1 (weights 10 .. 33, no two alike), inf on about 30 %"""
    rng = np.random.default_rng(seed)
    sig = rng.uniform(0.03, 0.1, (3, n, n))
    sig[rng.random((3, n, n)) < 0.3] = np.inf
    assert 0.3 < np.isfinite(sig).mean() < 0.9
    return sig


def _covs(prior, S, m, tmp, dev, seed):
    """(oracle covariance, device covariance) with m = 0 or 4 factor columns: the dct_diagonal prior of `_prior` (m = 4:
    `_updated_pair`) or the identity prior (two scripted update pairs)"""
    from oracle import fh_oracle as fo
    from free_hunch_amd import covariance as hc
    assert m in (0, 4)
    if prior == "identity":
        orc, hip = _cov_pair("identity", S, str(tmp), dev, None, m // 2, seed=seed)
    else:
        _prior(S, tmp)
        if m:
            orc, hip = _updated_pair(S, tmp, dev, seed)
        else:
            d = 3 * S * S
            orc = fo.make_covariance("dct_diagonal", str(tmp), 80.0 ** 2, d)
            hip = hc.CovarianceHessianBFGSDCT(str(tmp), 80.0 ** 2, d, device=dev, use_precalculated_info=True)
    assert hip.famC.m == m and hip.use_dct == (prior != "identity")
    return orc, hip


def _cg(ctx, prob, b, rtol, maxiter):
    from free_hunch_amd import _lib
    sol = Guarded(tuple(b.shape), b.device)
    info = _lib.FhCgInfo()
    _lib.check(ctx.lib.fh_cg_solve(ctx.h, C.byref(prob), b.data_ptr(), sol.out.data_ptr(), rtol, 0.0, maxiter, C.byref(info),
                                   _lib.stream()), "fh_cg_solve")
    return sol.check("fh_cg_solve"), info


def _check_system(tag, ctx, prob, shape, ref, dev, solve=True, support=None):
    """fh_amm against `ref` (a callable on a CPU tensor of `shape`) and, with `solve`, fh_cg_solve at rtol 1e-6; prints the four
    figures, asserts the bounds of the module docstring and returns (u, A u) on the device.  support: the 0/1 mask of a masked
    operator - its right-hand side is M b."""
    u, v = inputs.randn(shape, 21).to(dev).contiguous(), inputs.randn(shape, 22).to(dev).contiguous()
    au, av = _amm(ctx, prob, u), _amm(ctx, prob, v)
    want = ref(u.cpu())
    err = maxabs(au, want) / float(want.abs().max())
    l, r = float((u * av).sum()), float((au * v).sum())
    sym = abs(l - r) / max(abs(l), 1.0)
    line = f"ragged {tag}: amm {err:.2e} max|ref|, symmetry {sym:.2e}"
    if solve:
        b = inputs.randn(shape, 5).to(dev)
        b = (b if support is None else support * b).contiguous()
        x, info = _cg(ctx, prob, b, RTOL, 5000)
        res = float((b - _amm(ctx, prob, x.contiguous())).norm()) / float(b.norm())
        line += f", cg {info.niter} iterations, true residual {res:.3e} ||b||"
    print(line, flush=True)
    assert err <= 1e-8
    assert sym <= 1e-9
    if solve:
        assert info.optimal == 1 and 1 <= info.niter < 5000
        assert res <= 1.05 * RTOL
    return u, au


def _twin_error(tag, got, ref):
    err = maxabs(got, ref) / float(ref.abs().max())
    print(f"ragged {tag}: against the device's own twin {err:.2e} max|ref|", flush=True)
    assert err <= 1e-12


def _plan_kernels(S, ntaps, halo, stride):
    """(forward, adjoint) kernel ids of fh_conv_circ for this tap list: 0 / 1 k_conv1d, 2 k_conv_tile8, 3 k_conv_tile,
    4 k_conv_dec, 5 k_conv_up, 6 k_conv_direct"""
    from free_hunch_amd import _lib
    got = []
    for adjoint in (0, 1):
        out = (C.c_int32 * 6)()
        assert _lib.load().fh_conv_circ_plan(S, ntaps, halo, 3, stride, adjoint, out) == 0
        got.append(out[0])
    return tuple(got)


# ================================================================ 1. one application and one solve per operator
# ---------------------------------------------------------------- op 3
@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("S", [6, 20, 100, 250])
def test_colorization_at_ragged_sides(dev, tmp_path, S, prior, m):
    """op 3 against sigma_y^2 u + A (C (A^T u)) with the oracle's covariance: k_channel_mix<true / false> with pairs = S^2 / 2
    (18 at S = 6: part of one block; 31250 at S = 250: 122 blocks + 18 pairs) around the dense dct2d_launch on ONE plane per
    image - no ragged side takes the symmetric D_eff route.  Fails for a k_channel_mix<false> that reads channels 1 and 2 at
    a plane stride of `pairs` rounded down to 128 (= pairs at every multiple of 16; confirmed on a scratch build: all 16 cases
    failed, tests/test_channel_ops_gpu.py did not notice), or whose `i >= pairs` guard is dropped (the sentinel tail)."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    orc, hip = _covs(prior, S, m, tmp_path, dev, 4300 + S)
    op = _col_op(S, dev)
    s2 = _sigma_y2(op)
    prob, keep = _problem(op, hip, s2)
    assert prob.op == 3 and prob.ntaps == 3 and prob.m == m and prob.use_dct == int(prior != "identity") and S % 128 != 0
    A_mm = _oracle_amm(orc, s2)
    shape = (1, 1, S, S)
    _check_system(f"op 3 S={S} {prior} m={m}", hip.ctx, prob, shape, lambda u: A_mm(u.flatten()).reshape(shape), dev,
                  solve=S != 250)


# ---------------------------------------------------------------- ops 4, 5, 6
BLUR_CASES = [("disk15", 40), ("disk", 100), ("gaussian", 100), ("gaussian", 250), ("motion", 100), ("sparse61", 100)]


def _blur_route(prob, kind, prior, S, base):
    """asserts the route of a blur problem (base = 1 / 5 / 8: unmasked, masked, weighted) as the 64-pixel tests assert theirs"""
    if kind in ("disk", "disk15"):  # the dense window: k_conv_window[_masked]
        assert prob.op == {1: 4, 5: 6, 8: 9}[base] and not prob.tap_dy and prob.ntaps2 == 0 and not prob.fold_fwd_w
        return
    assert prob.op == base and prob.tap_dy and prob.fold_sym == 0
    if kind == "gaussian" and prior == "dct_diagonal":  # folded dense: k_gemm_f64 passes (+ k_mask); no k_dct_sym at S % 128 != 0
        assert prob.fold_fwd_w and prob.fold_inv_h and prob.ntaps2 > 0
    elif kind == "gaussian":  # the pair of 1-D passes
        assert not prob.fold_fwd_w and prob.ntaps2 > 0
        assert _plan_kernels(S, prob.ntaps, prob.halo, 1) == (0, 0) and _plan_kernels(S, prob.ntaps2, prob.halo2, 1) == (1, 1)
    else:  # the 2-D tap list: motion on k_conv_tile8, the wide sparse PSF on k_conv_tile
        assert not prob.fold_fwd_w and prob.ntaps2 == 0
        assert _plan_kernels(S, prob.ntaps, prob.halo, 1) == ((2, 2) if kind == "motion" else (3, 3))


def _oracle_blur(S, kind, orc):
    """A0(u) = s2 u + B C B^T u of the oracle's unmasked blur, on [1,3,S,S] CPU tensors"""
    from oracle import fh_oracle as fo
    oop = mb._oracle_op(S, _k(kind))
    x = torch.zeros(1, 3, S, S, dtype=F64)
    A0, _b, _back, _shape = fo.system(oop, oop.forward(x), x, orc)
    return lambda t: A0(t.flatten()).reshape(1, 3, S, S)


@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("S", [40, 100])
def test_window_blur_at_ragged_sides(dev, tmp_path, S, prior, m):
    """op 4 (custom_blur with a dense disk: 15 x 15 at S = 40, the 41 x 41 window of the 61 x 61 disk at S = 100) against the
    oracle's blur system.  Fails for a k_conv_window whose last tile of a row (8 live columns at S = 40, 4 at S = 100) wraps
    its halo by the tile width instead of by S."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    kind = "disk15" if S == 40 else "disk"
    orc, hip = _covs(prior, S, m, tmp_path, dev, 4400 + S)
    op = mb._cop(_k(kind), S, dev)
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.m == m and prob.use_dct == int(prior != "identity") and not prob.mask
    _blur_route(prob, kind, prior, S, 1)
    _check_system(f"op 4 {kind} S={S} {prior} m={m}", hip.ctx, prob, (1, 3, S, S), _oracle_blur(S, kind, orc), dev)


@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("kind,S", BLUR_CASES)
def test_masked_blur_at_ragged_sides(dev, tmp_path, kind, S, prior, m):
    """ops 5 / 6 with a random per-channel mask (60 % kept) against the restatement from the oracle's unmasked system, against
    the device's own unmasked twin (1e-12), out == sigma_y^2 u EXACTLY off the mask, and the solve of M b.  Routes: the Gaussian
    on dense folded k_gemm_f64 passes finished by k_mask (DCT prior) or on k_conv1d's masked epilogue (identity prior), motion
    on k_conv_tile8's masked epilogue, the wide sparse PSF on k_conv_tile + k_mask, the disks on k_conv_window_masked.  Fails
    for a masked epilogue that reads the mask at a row pitch of S rounded down to the 16-grid instead of S (confirmed on
    scratch builds for k_conv_tile8, k_conv1d and k_conv_window each: the motion, the identity-prior Gaussian and the disk
    cases failed; tests/test_masked_blur_gpu.py and tests/test_noise_map_gpu.py, all at multiples of 16, did not notice)."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    orc, hip = _covs(prior, S, m, tmp_path, dev, 4500 + S)
    mask = ragged_mask(S, 7 + S)
    mop, cop = mb._mop(_k(kind), S, dev, mask=mask), mb._cop(_k(kind), S, dev)
    s2 = _sigma_y2(mop)
    pm, keep_m = _problem(mop, hip, s2)
    pc, keep_c = _problem(cop, hip, s2)
    assert pm.m == m and pm.use_dct == int(prior != "identity") and pm.mask and not pc.mask
    _blur_route(pm, kind, prior, S, 5)
    tag = f"op {pm.op} {kind} S={S} {prior} m={m}"
    a0 = _oracle_blur(S, kind, orc)
    mk = torch.from_numpy(mask)[None]
    u, au = _check_system(tag, hip.ctx, pm, (1, 3, S, S), lambda t: mb._masked_ref(a0, mk, s2, t), dev, solve=S != 250,
                          support=mop.mask)
    off = mk == 0
    assert torch.equal(au.cpu()[off], (s2 * u.cpu())[off])
    _twin_error(tag, au, mb._masked_ref(lambda t: _amm(hip.ctx, pc, t.contiguous()), mop.mask, s2, u))


# ---------------------------------------------------------------- ops 7, 2
SR_FOLDED = [(20, 2), (36, 4), (40, 4), (100, 4), (100, 5), (250, 2), (250, 10), (36, 3)]  # (20, 4): see the module docstring
SR_TAPS = [(100, 4, "disk9"), (100, 4, "disk21"), (36, 3, "disk9"), (36, 3, "disk21")]


def _oracle_sr(S, s, psf, orc):
    """A0(u) = s2 u + A C A^T u of the oracle's SR system with this PSF, on [1,3,So,So] CPU tensors"""
    from oracle import fh_oracle as fo
    So = S // s
    oop = srt._oracle_op(S, s, psf)
    x = torch.zeros(1, 3, S, S, dtype=F64)
    A0, _b, _back, shape = fo.system(oop, srt._oracle_forward(oop, x), x, orc)
    assert tuple(shape) == (1, 3, So, So)
    return lambda t: A0(t.flatten()).reshape(1, 3, So, So)


def _sr_route(prob, op, s, want_op, prior="dct_diagonal"):
    assert prob.op == want_op and prob.stride == s and prob.use_dct == int(prior != "identity") and prob.fold_sym == 0
    assert bool(prob.fold_fwd_w) == bool(prob.fold_inv_h) == (want_op in (7, 11)) and prob.ntaps == op.taps.n and prob.ntaps2 == 0
    if want_op in (2, 10):  # no ragged side tiles k_conv_dec / k_conv_up
        assert _plan_kernels(op.in_shape[-1], prob.ntaps, prob.halo, s) == (6, 3)


@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("S,s", SR_FOLDED)
def test_folded_sr_at_ragged_sides(dev, tmp_path, S, s, m):
    """op 7 (9 x 13 binomial PSF on the rectangular bases) against the oracle's SR system: k_dct_rect inside the system, with
    the covariance's diagonal as forward pass B's table (m = 0) and add / p.Ap partials in inverse pass B, at So = 9, 25, 125
    (odd: scalar staging) and 10, 12, 20.  (20, 4) is refused by custom_sr (a 5 x 5 measurement): (20, 2) and (36, 4) stand
    in.  Fails for a k_dct_rect whose epilogue table is offset by (p % 3) (KO rounded down to 4) R per plane (confirmed on a
    scratch build: the m = 0 cases at S = 250, where forward pass B carries the diagonal, failed), and for one that zero pads
    K to whole chunks but reads `in` rows at the padded pitch."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    orc, hip = _covs("dct_diagonal", S, m, tmp_path, dev, 4600 + S + s)
    op = srt._sr_op(S, s, dev)
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.m == m and not prob.mask
    _sr_route(prob, op, s, 7)
    So = S // s
    _check_system(f"op 7 S={S} s={s} m={m}", hip.ctx, prob, (1, 3, So, So), _oracle_sr(S, s, None, orc), dev, solve=S != 250)


@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("S,s,key", SR_TAPS)
def test_tap_list_sr_at_ragged_sides(dev, tmp_path, S, s, key, prior, m):
    """op 2 through custom_sr with a disk PSF (49 and 317 taps) against the oracle's SR system: k_conv_tile with zero
    insertion back and k_conv_direct forward with add = sigma_y^2 u, So = 25 (odd) and 12.  Fails for a k_conv_direct whose
    flat index is split by S instead of So, and for a k_conv_tile that zero-inserts at s * (S // 16 s) tiles."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    orc, hip = _covs(prior, S, m, tmp_path, dev, 4700 + S + s)
    op = srt._sr_op(S, s, dev, nm.SR_PSFS[key])
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.m == m and not prob.mask
    _sr_route(prob, op, s, 2, prior)
    So = S // s
    _check_system(f"op 2 {key} S={S} s={s} {prior} m={m}", hip.ctx, prob, (1, 3, So, So), _oracle_sr(S, s, nm.SR_PSFS[key], orc), dev)


# ---------------------------------------------------------------- ops 8 .. 11
def _weighted_case(dev, tag, hip, orc_a0, S, s, key, want_op, solve):
    """ops 8 .. 11 with a random per-channel noise map against the restatement from the oracle's unweighted system (`orc_a0`),
    out == u exactly where w = 0, against the device's own unweighted twin (1e-12), and the solve"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, _solver_sigma_y2
    n = S if s is None else S // s
    wop, cop = nm._wop(S, s, _k(key), ragged_noise_map(n, 11 + S), dev), nm._twin(S, s, _k(key), dev)
    s2 = _sigma_y2(cop)
    pw, keep_w = _problem(wop, hip, _solver_sigma_y2(wop))
    pc, keep_c = _problem(cop, hip, s2)
    assert pw.op == want_op == nm.TWIN_OP[pc.op] and pw.mask and not pc.mask and pw.sigma_y2 == 1.0 and pw.m == pc.m
    w = wop.weights.cpu()
    assert len(torch.unique(w[w > 0])) > 0.99 * int((w > 0).sum())  # the weights differ from pixel to pixel
    shape = (1, 3, n, n)
    u, au = _check_system(tag, hip.ctx, pw, shape, lambda t: nm._weighted_ref(orc_a0, w, s2, t), dev, solve=solve)
    off = w == 0
    assert int(off.sum()) > 0 and torch.equal(au.cpu()[off], u.cpu()[off])
    _twin_error(tag, au, nm._weighted_ref(lambda t: _amm(hip.ctx, pc, t.contiguous()), wop.weights, s2, u))
    return pw, wop


@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("kind", ["gaussian", "motion", "disk"])
def test_weighted_blur_at_ragged_sides(dev, tmp_path, kind, prior, m):
    """ops 8 / 9 at S = 100 on the routes of the masked blur, with weights in place of the mask and k_cg_init_w / k_cg_step2_w
    keeping W p beside p.  Fails for a k_cg_step2_w that writes W p for the first 3 S^2 rounded down to whole blocks of 256
    only, so that the tail keeps W r0 (confirmed on a scratch build: every solve of ops 8 .. 11 here and the all-ones-weights
    cases failed; of tests/test_noise_map_gpu.py only the two SR cases with So = 12 and 8 noticed, no blur case did)."""
    S = 100
    orc, hip = _covs(prior, S, m, tmp_path, dev, 4800 + S)
    tag = f"op {9 if kind == 'disk' else 8} {kind} S={S} {prior} m={m}"
    pw, _wop = _weighted_case(dev, tag, hip, _oracle_blur(S, kind, orc), S, None, kind, 9 if kind == "disk" else 8, True)
    assert pw.m == m and pw.use_dct == int(prior != "identity")
    _blur_route(pw, kind, prior, S, 8)


@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("S,s,key", [(100, 4, "binomial"), (250, 2, "binomial"), (20, 2, "binomial"), (36, 4, "binomial")] + SR_TAPS)
def test_weighted_sr_at_ragged_sides(dev, tmp_path, S, s, key, prior, m):
    """op 11 (rank-1 PSF: the weights are inverse pass B's table of k_dct_rect, [3][So][So] per image) and op 10 (disk PSFs:
    k_conv_direct to the spare vector, then k_mask over 3 So^2 = 1875 / 432 measurements; so is the binomial PSF under the
    identity prior, at So = 25, 125, 10 and 9).  (20, 4) is refused by weighted_sr:
    (20, 2) and (36, 4) stand in.  Fails for a k_mask launched over 3 S^2 instead of 3 So^2 behind a decimating pass (the
    sentinel tail), and for a k_dct_rect that takes the weights of channel p % 3 at a plane stride of (So rounded down to 4) So
    (confirmed on a scratch build: every op 11 case failed; the 64- and 96-pixel tests, So = 16 and 12, did not notice)."""
    want_op = 11 if key == "binomial" and prior == "dct_diagonal" else 10
    orc, hip = _covs(prior, S, m, tmp_path, dev, 4900 + S + s)
    tag = f"op {want_op} {key} S={S} s={s} {prior} m={m}"
    pw, wop = _weighted_case(dev, tag, hip, _oracle_sr(S, s, nm.SR_PSFS[key], orc), S, s, key, want_op, S != 250)
    assert pw.m == m
    _sr_route(pw, wop, s, want_op, prior)


# ---------------------------------------------------------------- op 12
@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("prior", ["dct_diagonal", "identity"])
@pytest.mark.parametrize("S,s,kind", [(100, 4, "int"), (100, 4, "one"), (60, 3, "int"), (60, 3, "one")])
def test_burst_sr_at_ragged_sides(dev, tmp_path, S, s, kind, prior, m):
    """op 12 with K = s^2 integer shifts and with K = 1 frame of the 7 x 7 binomial PSF against s2 u + fwd(C(adj(u))) of
    test_burst_sr_gpu.Ref: the chain route (no ragged side is fused), K k_conv_tile launches that add into one image and K
    k_conv_direct launches into the frame-major measurement of 3 K So^2 doubles.  Fails for a chain that offsets frame k by
    3 So (So rounded down to 4) (confirmed on a scratch build: the K = 16 cases at So = 25 failed, as did the (100, 4) cases of
    test_operator_pair_against_the_reference), and for an adjoint chain whose first frame adds to an unwritten output."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    orc, hip = _covs(prior, S, m, tmp_path, dev, 5000 + S + s)
    op = bt._op(S, s, kind, dev)
    K, So = op.nframes, S // s
    assert K == (1 if kind == "one" else s * s) and (bt._route(op, 0), bt._route(op, 1)) == (0, 0)
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.op == 12 and prob.stride == s and prob.m == m and prob.ntaps2 == K and not prob.mask
    assert prob.use_dct == int(prior != "identity")
    shape = (1, 3 * K, So, So)
    A_mm = bt.Ref(op).system(orc, shape)
    _check_system(f"op 12 S={S} s={s} K={K} {prior} m={m}", hip.ctx, prob, shape, lambda u: A_mm(u.flatten()).reshape(shape), dev)


# ---------------------------------------------------------------- all-ones masks and weights
@pytest.mark.parametrize("kind,prior", [("gaussian", "dct_diagonal"), ("gaussian", "identity"), ("motion", "dct_diagonal"),
                                        ("sparse61", "dct_diagonal"), ("disk", "dct_diagonal")])
def test_all_ones_mask_equals_the_unmasked_twin_bitwise_at_100(dev, tmp_path, kind, prior):
    """the rule of test_all_ones_mask_equals_the_unmasked_twin_bitwise at S = 100: fh_amm and the solve at rtol 1e-6 of ops
    5 / 6 with an all-ones mask equal ops 1 / 4 in every bit - the k_mask pass behind the dense folded passes and behind
    k_conv_tile, and the masked epilogues of k_conv1d, k_conv_tile8 and k_conv_window on their partial tiles.  Fails for a
    masked epilogue that forms mask * t + s2 * u in another order than the unmasked fma(s2, u, t)."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 100
    _orc, hip = _covs(prior, S, 0, tmp_path, dev, 5100)
    mop, cop = mb._mop(_k(kind), S, dev, mask=np.ones((S, S))), mb._cop(_k(kind), S, dev)
    pm, keep_m = _problem(mop, hip, _sigma_y2(mop))
    pc, keep_c = _problem(cop, hip, _sigma_y2(cop))
    assert pm.op == pc.op + (4 if pc.op == 1 else 2) and pm.mask and not pc.mask
    for f in ("ntaps", "ntaps2", "halo", "halo2", "stride", "fold_sym", "sigma_y2", "m", "use_dct"):
        assert getattr(pm, f) == getattr(pc, f), f
    _blur_route(pm, kind, prior, S, 5)
    u = inputs.randn((1, 3, S, S), 21).to(dev)
    assert torch.equal(_amm(hip.ctx, pm, u), _amm(hip.ctx, pc, u))
    b = inputs.randn((1, 3, S, S), 22).to(dev)
    sm, im = _cg(hip.ctx, pm, b, RTOL, 5000)
    sc, ic = _cg(hip.ctx, pc, b, RTOL, 5000)
    print(f"ragged all-ones mask {kind} {prior} S={S}: {im.niter} iterations", flush=True)
    assert im.niter == ic.niter >= 1 and im.optimal == ic.optimal
    assert torch.equal(sm, sc)


@pytest.mark.parametrize("s,key,want_op", [(None, "gaussian", 8), (None, "motion", 8), (None, "disk", 9), (4, "binomial", 11),
                                           (4, "disk9", 10)])
def test_all_ones_weights_equal_the_unweighted_twin_bitwise_at_100(dev, tmp_path, s, key, want_op):
    """the rule of test_all_ones_weights_equal_the_unweighted_twin_bitwise at S = 100 (So = 25): ops 8 .. 11 with all-ones
    weights and the twin's sigma_y2 against ops 1 / 4 / 7 / 2 - fh_amm and a 6-iteration solve (rtol = 1e-300) in every bit.
    Fails for a k_cg_step2_w whose W p differs from p on a ragged tail."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S = 100
    n = S if s is None else S // s
    _orc, hip = _covs("dct_diagonal", S, 0, tmp_path, dev, 5200)
    wop, cop = nm._wop(S, s, key, np.ones((n, n)), dev), nm._twin(S, s, key, dev)
    assert bool((wop.weights == 1).all())
    pc, keep_c = _problem(cop, hip, _sigma_y2(cop))
    pw, keep_w = _problem(wop, hip, _sigma_y2(cop))
    assert pw.op == want_op == nm.TWIN_OP[pc.op] and pw.mask and not pc.mask
    for f in ("ntaps", "ntaps2", "halo", "halo2", "stride", "fold_sym", "sigma_y2", "m", "use_dct"):
        assert getattr(pw, f) == getattr(pc, f), f
    u = inputs.randn((1, 3, n, n), 21).to(dev)
    assert torch.equal(_amm(hip.ctx, pw, u), _amm(hip.ctx, pc, u))
    b = inputs.randn((1, 3, n, n), 22).to(dev)
    sw, iw = _cg(hip.ctx, pw, b, 1e-300, 6)
    sc, ic = _cg(hip.ctx, pc, b, 1e-300, 6)
    assert iw.niter == ic.niter == 6 and iw.b_norm == ic.b_norm and iw.residual_norm == ic.residual_norm
    assert torch.equal(sw, sc)


# ================================================================ 2. batched solves in which an image finishes
def _family(name, dev):
    """(S, three operators that share the PSF and differ in mask / noise map where the operator has one, measurement shape)"""
    if name == "op3":
        return 100, [_col_op(100, dev, slot=i) for i in range(3)], (1, 100, 100)
    if name in ("op5", "op6"):
        kind = "gaussian" if name == "op5" else "disk"
        return 100, [mb._mop(kind, 100, dev, slot=i, mask=ragged_mask(100, 200 + i)) for i in range(3)], (3, 100, 100)
    if name.startswith("op7"):
        S, s = (100, 4) if name == "op7_100_4" else (250, 10)
        return S, [srt._sr_op(S, s, dev, slot=i) for i in range(3)], (3, S // s, S // s)
    if name in ("op10", "op11"):
        key = "disk9" if name == "op10" else "binomial"
        return 100, [nm._wop(100, 4, key, ragged_noise_map(25, 300 + i), dev, slot=i) for i in range(3)], (3, 25, 25)
    assert name == "op12"
    return 100, [bt._op(100, 4, "int", dev, slot=i) for i in range(3)], (48, 25, 25)


FAMILY_OP = {"op3": 3, "op5": 5, "op6": 6, "op7_100_4": 7, "op7_250_10": 7, "op10": 10, "op11": 11, "op12": 12}


def _batched_against_singles(name, dev, tmp, b, rtols, maxiter):
    """three fh_cg_solve calls and one fh_cg_solve_batched on the same systems: ([(solution, niter, optimal)], solution [3, n],
    infos); images 0 and 2 have distinct covariances (m = 4), every image its own mask / weights"""
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
    S, ops, mshape = _family(name, dev)
    nimg = 3
    _prior(S, tmp)
    covs = [_updated_pair(S, tmp, dev, 100 + i, slot=i + 1, oracle=False)[1] for i in range(nimg)]
    probs = [_problem(ops[i], covs[i], _solver_sigma_y2(ops[i])) for i in range(nimg)]
    has_map = FAMILY_OP[name] in (5, 6, 10, 11)
    assert all(p.op == FAMILY_OP[name] and p.m == 4 and bool(p.mask) == has_map for p, _keep in probs)
    if has_map:
        assert len({float(keep[-1].sum()) for _p, keep in probs}) == nimg  # three different masks / noise maps
    singles = []
    for i in range(nimg):
        x, info = _cg(covs[i].ctx, probs[i][0], b[i].contiguous(), rtols[i], maxiter)
        singles.append((x, info.niter, info.optimal))
    bctx = _lib.Context.get(S, 3 * nimg, 0, slot=6200)
    per = _lib.FhBatch()
    per.nimg = nimg
    for i, cov in enumerate(covs):
        per.D[i], per.r[i], per.B[i], per.M[i] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(), cov.famC.B.data_ptr(),
                                                  cov.C.M_dev.data_ptr())
        if has_map:
            per.mask[i] = probs[i][1][-1].data_ptr()  # (_problem keeps the mask / the weights last)
    sol = Guarded(tuple(b.shape), dev)
    infos = (_lib.FhCgInfo * nimg)()
    _lib.check(bctx.lib.fh_cg_solve_batched(bctx.h, C.byref(probs[0][0]), C.byref(per), b.data_ptr(), sol.out.data_ptr(),
                                            (C.c_double * nimg)(*rtols), 0.0, maxiter, infos, _lib.stream()), "cg batched")
    got = sol.check("fh_cg_solve_batched")
    errs = [float((got[i] - singles[i][0]).abs().max()) / max(1.0, float(singles[i][0].abs().max())) for i in range(nimg)]
    print(f"ragged batched cg {name}: iterations {[infos[i].niter for i in range(nimg)]} (single {[s[1] for s in singles]}), "
          f"difference {max(errs):.2e}", flush=True)
    for i in range(nimg):
        assert infos[i].niter == singles[i][1] and infos[i].optimal == singles[i][2], (i, infos[i].niter, singles[i][1])
        assert errs[i] <= 1e-12, (i, errs[i])
    return infos


@pytest.mark.parametrize("name", list(FAMILY_OP))
def test_batched_solve_with_a_finished_image_at_ragged_sides(dev, tmp_path, name):
    """fh_cg_solve_batched with 3 images, the middle one with a zero right-hand side, against three fh_cg_solve calls by the
    rule of test_batched_cg_with_a_finished_image (rtol 1e-5, 400-iteration cap).  From the first iteration on every kernel of
    the loop skips planes 3 .. 5 (op 3: plane 1; op 12: frames 16 .. 31), and at these sides an image's rows or its 3 So^2 =
    1875 measurements are no multiple of any tile or block.  Fails for a k_dct_rect that tests `done` of plane p (clamped to
    the batch) instead of image p / 3 (confirmed on a scratch build: op 7 at both sides and op 11 failed, as did the 64-pixel
    batched SR tests), for a k_mask that offsets image i by i times n rounded down to 256 (confirmed: ops 5, 6, 10 and 11
    failed, no 64-pixel test of these operators noticed), and for a chain that hands frame k of image i the control block of
    image 0."""
    S, _ops, mshape = _family(name, dev)
    b = torch.stack([inputs.randn(mshape, 40).to(dev), torch.zeros(mshape, dtype=F64, device=dev), inputs.randn(mshape, 42).to(dev)])
    infos = _batched_against_singles(name, dev, tmp_path, b, [1e-5] * 3, 400)
    assert infos[1].niter == 1 and not infos[1].optimal
    assert min(infos[0].niter, infos[2].niter) > 1


@pytest.mark.parametrize("name", ["op7_100_4", "op5"])
def test_batched_solve_with_an_image_leaving_mid_solve_at_ragged_sides(dev, tmp_path, name):
    """the construction of test_dct_streams_gpu.solver_cases: a per-image rtol of 1e6 for the middle image (met within the
    first iterations, with a direction and a residual that are not zero) and 1e-30 for the other two under a 40-iteration cap,
    against single solves with the same tolerances.  No float64 residual meets 1e-30 ||b||, so the other two are never
    `optimal`: they run on to the cap (op 5) or until the reference's p.Ap break ends them (op 7: 1875 unknowns per image are
    solved to rounding level before the cap), well after the middle image has left.  Fails for a pass that goes on writing the
    planes of the image that left: its solution would move after its last iteration."""
    S, _ops, mshape = _family(name, dev)
    b = torch.stack([inputs.randn(mshape, 50 + i).to(dev) for i in range(3)])
    infos = _batched_against_singles(name, dev, tmp_path, b, [1e-30, 1e6, 1e-30], 40)
    n = [i.niter for i in infos]
    assert infos[1].optimal and not infos[0].optimal and not infos[2].optimal
    assert n[1] + 8 <= min(n[0], n[2]) <= max(n[0], n[2]) <= 40, n  # the others ran on for more than one chunk of 8 iterations
