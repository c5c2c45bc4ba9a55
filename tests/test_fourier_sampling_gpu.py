"""`fourier_sampling` on the device: the Hartley butterfly (fh_hartley_fix), the transform (fh_hartley2d) and fh_problem.op = 15
from one application of A_mm up to the CLI.

The reference is tests/_fourier_restatement.py: H x = Re - Im of numpy.fft.fft2(norm="ortho"), the butterfly in the kernel's own
order of operations, and A_mm(u) = sigma_y2 u + W H C H W u on the oracle's covariance and cg.  Every output a test hands to an
entry point itself is a `G64`: NaN before the call, sentinels behind it in the same allocation.  Sides: 2 (every point is its own
reflection), 6, 16, 30 (even, off the 16 and 32 grids), 64, 128 and one case each at 256."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import _fourier_restatement as fr
import inputs
import nets
import test_custom_sr_gpu as srt
from test_channel_ops_gpu import _run_script
from test_hip_parity import _base_kwargs, maxabs

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "free-hunch_amd", "data")
SIGMA_S = 0.05
TAIL, SENTINEL = 64, -12345.678


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class G64:
    """a float64 output buffer of `shape` filled with NaN (or `fill`), with TAIL sentinels behind it in the same allocation"""

    def __init__(self, shape, dev, fill=float("nan")):
        n = int(np.prod(shape))
        self.full = torch.full((n + TAIL,), fill, dtype=F64, device=dev)
        self.full[n:] = SENTINEL
        self.out = self.full[:n].view(*shape)

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.full[-TAIL:] == SENTINEL).all()), (what, "wrote past the end of its output")
        assert not bool(torch.isnan(self.out).any()), (what, "left outputs unwritten")
        return self.out

    def untouched(self, fill):
        torch.cuda.synchronize()
        return bool((self.full[-TAIL:] == SENTINEL).all()) and bool((self.out == fill).all())


def _op(S, dev, slot=0, **kw):
    from free_hunch_amd.measurements import get_operator
    if not any(k in kw for k in ("mask", "mask_path", "pattern")):
        kw.update(pattern="cartesian", acceleration=4.0)
    op = get_operator(name="fourier_sampling", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), **kw)
    op.ctx_slot = slot
    return op


def _sigma_map(S, seed):
    """standard deviations in [0.05, 0.5] with a block of unmeasured (inf) frequencies"""
    s = 0.05 + 0.45 * np.random.default_rng(seed).random((3, S, S))
    s[:, S // 4: S // 4 + max(1, S // 8), :] = np.inf
    return s


def _amm(cov, prob, u, what="fh_amm"):
    from free_hunch_amd import _lib
    g = G64(tuple(u.shape), u.device)
    _lib.check(cov.ctx.lib.fh_amm(cov.ctx.h, C.byref(prob), u.data_ptr(), g.out.data_ptr(), _lib.stream()), "fh_amm")
    return g.check(what)


_IDENT = {}


def _pair(S, n_script, use_dct, tmp_factory, dev):
    """(oracle covariance, device covariance): the shipped DCT prior cut to S (`test_custom_sr_gpu._cov_pair`), or the identity
    basis with unit variance, after `n_script` scripted update pairs; built once, only read"""
    if use_dct:
        return srt._cov_pair(S, n_script, tmp_factory, dev)
    from oracle import fh_oracle as fo
    from free_hunch_amd import covariance as hc
    if (S, n_script) not in _IDENT:
        d = 3 * S * S
        hip = hc.CovarianceHessianBFGS(1, 80.0 ** 2, d, device=dev)
        orc = fo.make_covariance("identity", None, 80.0 ** 2, d)
        if n_script:
            steps = inputs.script(1200, (1, 3, S, S), n_script, 80.0)
            _run_script(orc, steps)
            _run_script(hip, steps, dev)
            assert hip.k == orc.k and hip.famC.m == 2 * n_script
        _IDENT[(S, n_script)] = (orc, hip)
    return _IDENT[(S, n_script)]


# ---------------------------------------------------------------- 1. the butterfly
@pytest.mark.parametrize("planes", [1, 3, 51])
@pytest.mark.parametrize("S", [2, 6, 30, 256])
def test_hartley_fix(dev, S, planes):
    """bit for bit against numpy in the stated order without weights and add; within 2 ulp with both; self-conjugate points pass
    through exactly under all-ones weights.  51 planes take a second trip over the 48 planes of grid y."""
    from free_hunch_amd import _lib
    ctx = _lib.Context.get(S, 51, 0)
    lib, st = ctx.lib, _lib.stream()
    T = inputs.randn((planes, S, S), 100 + S + planes)
    Td = T.to(dev)
    plan = (C.c_int32 * 15)()
    assert lib.fh_hartley2d_plan(S, planes, plan) == 0 and plan[11] == min(planes, 48)
    g = G64((planes, S, S), dev)
    assert lib.fh_hartley_fix(ctx.h, Td.data_ptr(), g.out.data_ptr(), None, None, 0.0, planes, st) == 0
    want = torch.from_numpy(fr.butterfly(T.numpy()))
    assert torch.equal(g.check("fh_hartley_fix").cpu(), want)
    if S == 2:
        assert torch.equal(g.out.cpu(), T)
    # weights [3][S][S] (plane p reads channel p % 3) and add
    w, add, scale = inputs.randn((3, S, S), 7 + S).abs(), inputs.randn((planes, S, S), 8 + S), 0.37
    wp = w[torch.arange(planes) % 3]
    g = G64((planes, S, S), dev)
    wd, ad = w.to(dev), add.to(dev)
    assert lib.fh_hartley_fix(ctx.h, Td.data_ptr(), g.out.data_ptr(), wd.data_ptr(), ad.data_ptr(), scale, planes, st) == 0
    ref = fr.butterfly_weighted(T.numpy(), wp.numpy(), add.numpy(), scale)
    got = g.check("fh_hartley_fix, weights and add").cpu().numpy()
    assert (np.abs(got - ref) <= 2 * np.spacing(np.abs(ref))).all()
    # all-ones weights, no add: the same bits as no weights, and self-conjugate points equal the input
    ones = torch.ones(3, S, S, dtype=F64, device=dev)
    g = G64((planes, S, S), dev)
    assert lib.fh_hartley_fix(ctx.h, Td.data_ptr(), g.out.data_ptr(), ones.data_ptr(), None, 0.0, planes, st) == 0
    got = g.check("fh_hartley_fix, unit weights").cpu()
    assert torch.equal(got, want)
    sc = [0, S // 2]
    assert torch.equal(got[:, sc][:, :, sc], T[:, sc][:, :, sc])


def test_hartley_fix_refusals(dev):
    from free_hunch_amd import _lib
    S = 30
    ctx = _lib.Context.get(S, 3, 0)
    lib, st = ctx.lib, _lib.stream()
    x = inputs.randn((3, S, S), 5).to(dev)
    keep = x.clone()
    g = G64((3, S, S), dev, fill=123.0)
    o = g.out.data_ptr()
    assert lib.fh_hartley_fix(ctx.h, x.data_ptr(), x.data_ptr(), None, None, 0.0, 3, st) == _lib.FH_EINVAL  # in == out
    assert lib.fh_hartley_fix(ctx.h, None, o, None, None, 0.0, 3, st) == _lib.FH_EINVAL
    assert lib.fh_hartley_fix(ctx.h, x.data_ptr(), None, None, None, 0.0, 3, st) == _lib.FH_EINVAL
    assert lib.fh_hartley_fix(None, x.data_ptr(), o, None, None, 0.0, 3, st) == _lib.FH_EINVAL
    for planes in (0, -3, 65536):
        assert lib.fh_hartley_fix(ctx.h, x.data_ptr(), o, None, None, 0.0, planes, st) == _lib.FH_EINVAL
    assert lib.fh_hartley_fix(ctx.h, x.data_ptr(), o, None, None, 0.0, 6, st) == _lib.FH_ESIZE  # beyond the context's planes
    assert lib.fh_hartley_fix(ctx.h, x.data_ptr() + 8, o, None, None, 0.0, 1, st) == _lib.FH_EINVAL  # 16-byte accesses
    assert lib.fh_hartley_fix(ctx.h, x.data_ptr(), o, None, o, 1.0, 3, st) == _lib.FH_EINVAL  # add == out
    assert lib.fh_hartley_fix(ctx.h, x.data_ptr(), o, o, None, 0.0, 3, st) == _lib.FH_EINVAL  # w == out
    Hc = torch.eye(S, dtype=F64, device=dev)
    assert lib.fh_hartley2d(ctx.h, x.data_ptr(), o, None, 3, st) == _lib.FH_EINVAL
    assert lib.fh_hartley2d(ctx.h, None, o, Hc.data_ptr(), 3, st) == _lib.FH_EINVAL
    assert lib.fh_hartley2d(ctx.h, x.data_ptr(), o, Hc.data_ptr(), 0, st) == _lib.FH_EINVAL
    assert lib.fh_hartley2d(ctx.h, x.data_ptr(), o, Hc.data_ptr(), 6, st) == _lib.FH_ESIZE
    assert g.untouched(123.0) and torch.equal(x, keep)


# ---------------------------------------------------------------- 2. the transform
@pytest.mark.parametrize("S", [16, 30, 128, 256])
def test_hartley2d(dev, S):
    """against Re - Im of numpy's orthonormal fft2 at the bar test_custom_sr_gpu holds fh_dct_rect to, 1e-12 max(1, max|ref|);
    applied twice it returns the input to the same bar; 9 planes repeat the 3-plane bits"""
    from free_hunch_amd import _lib
    from free_hunch_amd.measurements import folded_dct_hartley_bases
    Hc = torch.from_numpy(folded_dct_hartley_bases(S)[0]).to(dev)
    x = inputs.randn((9, S, S), 40 + S)
    ref = fr.hartley2(x)
    bar = 1e-12 * max(1.0, float(ref.abs().max()))
    got = {}
    for planes in (3, 9):
        ctx = _lib.Context.get(S, planes, 0)
        g = G64((planes, S, S), dev)
        ctx.hartley2d(x[:planes].to(dev).contiguous(), g.out, Hc)
        got[planes] = g.check("fh_hartley2d")
        e = maxabs(got[planes], ref[:planes])
        print(f"hartley2d S={S} planes={planes}: {e / max(1.0, float(ref.abs().max())):.2e}", flush=True)
        assert e <= bar
        g2 = G64((planes, S, S), dev)
        ctx.hartley2d(got[planes], g2.out, Hc)
        assert maxabs(g2.check("fh_hartley2d twice"), x[:planes]) <= 1e-12 * max(1.0, float(x.abs().max()))
    assert torch.equal(got[9][:3], got[3])
    y = x[:3].to(dev).clone()  # in place
    _lib.Context.get(S, 3, 0).hartley2d(y, y, Hc)
    torch.cuda.synchronize()
    assert torch.equal(y, got[3])


# ---------------------------------------------------------------- 3. one application of A_mm
def _amm_op(S, dev, kind, slot=0):
    return _op(S, dev, slot, noise_map=_sigma_map(S, 3)) if kind == "map" else _op(S, dev, slot)


@pytest.mark.parametrize("kind", ["mask", "map"])
@pytest.mark.parametrize("use_dct", [1, 0])
@pytest.mark.parametrize("n_script", [0, 4])
@pytest.mark.parametrize("S", [30, 64, 128])
def test_amm_vs_restated_system(dev, tmp_path_factory, S, n_script, use_dct, kind):
    """fh_amm with op = 15 against sigma_y2 u + W H C H W u: 1e-8 of max|ref|, symmetry to 1e-9, and exactly sigma_y2 u where the
    weight is 0 - a 0/1 cartesian mask with sigma_y2 = s^2, and a 1 / sigma map with sigma_y2 = 1"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
    orc, hip = _pair(S, n_script, use_dct, tmp_path_factory, dev)
    op = _amm_op(S, dev, kind)
    s2 = _solver_sigma_y2(op)
    assert s2 == (1.0 if kind == "map" else pytest.approx(SIGMA_S ** 2))
    prob, keep = _problem(op, hip, s2)
    assert prob.op == 15 and prob.m == 2 * n_script and prob.use_dct == use_dct and prob.mask == keep[-1].data_ptr()
    shape = (1, 3, S, S)
    sysm = fr.System(op.weights, orc, s2)
    u, v = inputs.randn(shape, 21).to(dev), inputs.randn(shape, 22).to(dev)
    au, av = _amm(hip, prob, u), _amm(hip, prob, v)
    ref = sysm.A_mm(u.cpu().flatten()).reshape(shape)
    err = maxabs(au, ref) / float(ref.abs().max())
    l, r = float((u * av).sum()), float((au * v).sum())
    print(f"amm op=15 S={S} m={prob.m} use_dct={use_dct} {kind}: {err:.2e}, symmetry {abs(l - r) / max(abs(l), 1.0):.2e}", flush=True)
    assert err <= 1e-8
    assert abs(l - r) <= 1e-9 * max(abs(l), 1.0)
    off = op.weights == 0
    assert bool(off.any()) and torch.equal(au[off], (s2 * u)[off])


def test_amm_at_the_real_size(dev, tmp_path_factory):
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
    S = 256
    orc, hip = _pair(S, 0, 1, tmp_path_factory, dev)
    op = _op(S, dev)
    prob, keep = _problem(op, hip, _solver_sigma_y2(op))
    shape = (1, 3, S, S)
    u = inputs.randn(shape, 23).to(dev)
    ref = fr.System(op.weights, orc, prob.sigma_y2).A_mm(u.cpu().flatten()).reshape(shape)
    assert maxabs(_amm(hip, prob, u), ref) <= 1e-8 * float(ref.abs().max())


@pytest.mark.parametrize("n_script", [0, 4])
def test_full_sampling_equals_denoising_through_the_transform(dev, tmp_path_factory, n_script):
    """all-ones weights: A_mm15(u) = H A_mm0(H u), op 0 the all-ones-mask operator the project already trusts; the bar is
    1e-12 max(1, max|ref|) with ref the op-0 route's output"""
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
    from free_hunch_amd.measurements import get_operator
    S = 64
    _orc, hip = _pair(S, n_script, 1, tmp_path_factory, dev)
    op = _op(S, dev, mask=np.ones((S, S)))
    ident = get_operator(name="noise", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S))
    p15, k15 = _problem(op, hip, _solver_sigma_y2(op))
    p0, k0 = _problem(ident, hip, _solver_sigma_y2(ident))
    assert p15.op == 15 and p0.op == 0 and p15.sigma_y2 == p0.sigma_y2 and p15.m == 2 * n_script
    u = inputs.randn((1, 3, S, S), 25).to(dev)
    Hc = op.hartley_basis()
    ctx = _lib.Context.get(S, 3, 0)
    hu = ctx.hartley2d(u, torch.empty_like(u), Hc)
    ref = ctx.hartley2d(_amm(hip, p0, hu), torch.empty_like(u), Hc)
    got = _amm(hip, p15, u)
    e, scale = maxabs(got, ref), max(1.0, float(ref.abs().max()))
    print(f"op 15 against H op 0 H, m={p15.m}: {e / scale:.2e}", flush=True)
    assert e <= 1e-12 * scale


# ---------------------------------------------------------------- 4. the solve
def _solve_inputs(op, S):
    w = op.mask.cpu()
    x_true = inputs.smooth_image(S, 31).to(F64)
    y = w * (fr.hartley2(x_true) + SIGMA_S * inputs.randn((1, 3, S, S), 32))
    x0_mean = x_true + 0.05 * inputs.randn((1, 3, S, S), 33)
    return y, x0_mean


@pytest.mark.parametrize("S", [64, 256])
def test_six_iterations_vs_oracle_cg(dev, tmp_path_factory, S):
    """six forced iterations on both sides agree to 1e-5 of max|mat|"""
    from oracle import fh_oracle as fo
    from free_hunch_amd.conditioning_mechanisms import _solver_sigma_y2, solve_customcuda
    orc, hip = _pair(S, 0, 1, tmp_path_factory, dev)
    op = _op(S, dev)
    y, x0_mean = _solve_inputs(op, S)
    sysm = fr.System(op.weights, orc, _solver_sigma_y2(op))
    m6h = solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, rtol=1e-300, maxiter=6)
    sol6, info6 = fo.cg(sysm.A_mm, sysm.rhs(y, x0_mean), rtol=0.0, maxiter=6)
    m6o = sysm.mat(sol6)
    short = maxabs(m6o, m6h) / float(m6o.abs().max())
    print(f"fourier solve S={S}: six iterations {short:.2e}", flush=True)
    assert info6["niter"] == 6 and tuple(m6h.shape) == (1, 3, S, S)
    assert short <= 1e-5


def test_converged_solve_meets_its_tolerance(dev, tmp_path_factory):
    """(64, cartesian R = 4, sigma_s = 0.05, m = 0) at rtol = 1e-6 - the oracle's cg needs 827 iterations for this system on the
    CPU, inside the 5000 cap: the device reports `optimal`, and the true residual of the returned solution, recomputed with an
    independent fh_amm, is <= 1.05 rtol ||b||"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2, solve_customcuda
    S = 64
    orc, hip = _pair(S, 0, 1, tmp_path_factory, dev)
    op = _op(S, dev)
    y, x0_mean = _solve_inputs(op, S)
    rtol, info_h = 1e-6, []
    solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, info_h, rtol=rtol)
    u_h = solve_customcuda.last_solution.clone()
    prob, keep = _problem(op, hip, _solver_sigma_y2(op))
    bd = fr.System(op.weights, orc, prob.sigma_y2).rhs(y, x0_mean).reshape(y.shape).to(dev)
    res = float((bd - _amm(hip, prob, u_h)).norm())
    print(f"fourier solve rtol 1e-6: device {info_h[0]['niter']} it, true residual {res / float(bd.norm()):.3e} ||b||", flush=True)
    assert info_h[0]["optimal"] and 1 <= info_h[0]["niter"] < 5000
    assert res <= 1.05 * rtol * float(bd.norm())


def test_batched_solve_equals_single(dev, tmp_path):
    """fh_cg_solve_batched with op = 15 over 3 images with three different masks - cartesian, radial, and cartesian under a noise
    map with an inf block - and their own covariances and measurements, against per-image solves: identical iteration counts,
    `mat` within 1e-12 of max|mat|.  The images stop at different iterations, so the kernels skip a finished image from then on."""
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2, solve_customcuda, solve_customcuda_batched
    S, nimg = 64, 3
    dv = torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
    torch.save(dv, tmp_path / "dct_variance.pt")
    flat = np.full((S, S), 0.1)
    kws = [dict(pattern="cartesian", acceleration=4.0, noise_map=flat), dict(pattern="radial", acceleration=3.0, seed=4, noise_map=2 * flat),
           dict(pattern="cartesian", acceleration=2.0, seed=9, noise_map=_sigma_map(S, 6))]
    ops, covs, ys, xs = [], [], [], []
    for b in range(nimg):
        op = _op(S, dev, slot=b, **kws[b])
        cov = hc.CovarianceHessianBFGSDCT(str(tmp_path), 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=b)
        x = inputs.randn((1, 3, S, S), 300 + b).to(dev) * 40.0
        cov.update_time_step(x, 80.0, [40.0, 12.0, 3.0][b], -x / 80.0 ** 2 * 0.5)
        x0 = inputs.smooth_image(S, 310 + b).to(dev)
        torch.manual_seed(320 + b)
        ys.append(op.forward(x0))
        xs.append((0.3 * x0).to(F64))
        ops.append(op)
        covs.append(cov)
    assert len({o.mask.cpu().numpy().tobytes() for o in ops}) == 3 and bool(torch.isinf(ops[2].noise_map).any())
    assert _problem(ops[0], covs[0], _solver_sigma_y2(ops[0]))[0].op == 15 and all(_solver_sigma_y2(o) == 1.0 for o in ops)
    sigma_t = 0.4  # rtol_func(0.4) = 9e-3
    infos_b = []
    mats_b = solve_customcuda_batched(ops, ys, xs, covs, 1.0, sigma_t, infos_b, exclusive=True)
    assert tuple(mats_b.shape) == (nimg, 3, S, S) and bool(torch.isfinite(mats_b).all())
    n_b = [i["niter"] for i in infos_b]
    for b in range(nimg):
        info = []
        one = solve_customcuda(ops[b], ys[b], xs[b], covs[b], 1.0, sigma_t, info)
        assert infos_b[b]["niter"] == info[0]["niter"], (b, n_b, info[0])
        assert infos_b[b]["optimal"] and info[0]["optimal"]
        assert maxabs(mats_b[b:b + 1], one) <= 1e-12 * float(one.abs().max()), b
    print(f"batched fourier solve: iterations {n_b}", flush=True)
    assert min(n_b) < max(n_b), n_b  # an image finished first: the `done` skip ran


def test_batched_solve_refuses_mixed_noise_models(dev):
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda_batched
    S = 64
    covs = [hc.CovarianceHessianBFGS(1, 80.0 ** 2, 3 * S * S, device=dev, ctx_slot=b) for b in range(2)]
    z = torch.zeros(1, 3, S, S, dtype=F64, device=dev)
    ops = [_op(S, dev, slot=0), _op(S, dev, slot=1, noise_map=np.full((S, S), 0.1))]
    with pytest.raises(AssertionError, match="noise map"):
        solve_customcuda_batched(ops, [z, z], [z, z], covs, 1.0, 0.4)


def _own_cov(S, dev, tmp_path, slot):
    """a device covariance on the shipped DCT prior cut to S with a context of its own (`slot`): no earlier solve on the legacy
    stream has switched its graphs off"""
    from free_hunch_amd import covariance as hc
    dv = torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
    torch.save(dv, tmp_path / "dct_variance.pt")
    return hc.CovarianceHessianBFGSDCT(str(tmp_path), 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=slot)


def test_graph_reads_the_weights_at_replay(dev, tmp_path, monkeypatch):
    """On a capturable stream (the legacy null stream refuses capture and would run every chunk eagerly) and a context of its
    own: a second solve with other weight VALUES under the same pointers - the same problem struct, so the cached graph of CG
    iterations is replayed - gives, bit for bit, the solve of a freshly built operator with those weights, and differs from the
    first: the kernels read the weights at every replay.  The replayed solves then equal, bit for bit, the same solves launched
    eagerly (FH_NO_GRAPH=1): the tail butterfly's p.Ap partials under replay are checked by value."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2, solve_customcuda
    S = 64
    monkeypatch.delenv("FH_NO_GRAPH", raising=False)
    hip = _own_cov(S, dev, tmp_path, 41)
    a = _op(S, dev, noise_map=_sigma_map(S, 3))
    b = _op(S, dev, noise_map=_sigma_map(S, 4))
    first_weights = a.weights.clone()
    assert torch.equal(a.mask, b.mask) and not torch.equal(a.weights, b.weights)
    y = inputs.randn((1, 3, S, S), 41).to(dev) * a.mask
    x0 = inputs.smooth_image(S, 42).to(dev).to(F64)
    solve = lambda op: solve_customcuda(op, y, x0, hip, 1.0, 1.0, rtol=1e-300, maxiter=16).clone()  # noqa: E731
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        pa, keep_a = _problem(a, hip, _solver_sigma_y2(a))
        first = solve(a)
        a.weights.copy_(b.weights)
        torch.cuda.synchronize()
        pa2, keep_a2 = _problem(a, hip, _solver_sigma_y2(a))
        assert bytes(pa) == bytes(pa2)
        second, fresh = solve(a), solve(b)
        torch.cuda.synchronize()
        assert torch.equal(second, fresh)
        assert not torch.equal(second, first) and bool(torch.isfinite(second).all())
        monkeypatch.setenv("FH_NO_GRAPH", "1")  # read by the library at every solve
        eager_second = solve(a)
        a.weights.copy_(first_weights)
        eager_first = solve(a)
        torch.cuda.synchronize()
    assert torch.equal(eager_second, second) and torch.equal(eager_first, first)


# ---------------------------------------------------------------- 5. refusals without a launch
def test_op15_refuses_bad_problems_without_launching(dev, tmp_path_factory):
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _solver_sigma_y2
    S = 64
    _orc, hip = _pair(S, 0, 1, tmp_path_factory, dev)
    op = _op(S, dev)
    u = inputs.randn((1, 3, S, S), 61).to(dev)
    g = G64((1, 3, S, S), dev, fill=123.0)
    out = g.out
    info = _lib.FhCgInfo()
    some = u.data_ptr()
    lib = hip.ctx.lib
    prob, keep = _problem(op, hip, _solver_sigma_y2(op))  # the valid problem runs
    good = G64((1, 3, S, S), dev)
    assert lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr(), good.out.data_ptr(), _lib.stream()) == 0
    good.check("fh_amm, the valid problem")
    for field, value in (("mask", None), ("fold_fwd_w", None), ("fold_fwd_h", None), ("fold_inv_w", None), ("fold_inv_h", None),
                         ("fold_sym", 1), ("stride", 2), ("stride", 0), ("ntaps", 1), ("ntaps2", 1), ("halo", 1), ("halo2", 1),
                         ("tap_dy", some), ("tap_dx", some), ("tap_w", some), ("tap2_dy", some), ("tap2_dx", some), ("tap2_w", some),
                         ("planes", 6), ("d", 3 * S * S - 1), ("d", 3 * S * S + 1), ("use_dct", 2), ("use_dct", -1), ("op", 16)):
        prob, keep = _problem(op, hip, _solver_sigma_y2(op))
        assert prob.op == 15
        setattr(prob, field, value)
        rc = lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
        for scipy_mode in (0, 1):  # with cg_scipy = 1 no apply precedes k_cg_init: the solve refuses by itself
            prob.cg_scipy = scipy_mode
            rc = lib.fh_cg_solve(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), 1e-3, 0.0, 10, C.byref(info), _lib.stream())
            assert rc == _lib.FH_EINVAL, (field, value, scipy_mode, rc)
    prob, keep = _problem(op, hip, _solver_sigma_y2(op))  # the batched entry point: a null per->mask[i]
    per = _lib.FhBatch()
    per.nimg = 1
    per.D[0], per.r[0], per.B[0], per.M[0], per.mask[0] = prob.D, prob.r, prob.B, prob.M, None
    rtol = (C.c_double * 1)(1e-3)
    rc = lib.fh_cg_solve_batched(hip.ctx.h, C.byref(prob), C.byref(per), u.data_ptr(), out.data_ptr(), rtol, 0.0, 10,
                                 C.byref(info), _lib.stream())
    assert rc == _lib.FH_EINVAL
    per.mask[0] = prob.mask + 8  # the weights are read 16 bytes at a time
    rc = lib.fh_cg_solve_batched(hip.ctx.h, C.byref(prob), C.byref(per), u.data_ptr(), out.data_ptr(), rtol, 0.0, 10,
                                 C.byref(info), _lib.stream())
    assert rc == _lib.FH_EINVAL
    prob, keep = _problem(op, hip, _solver_sigma_y2(op))  # b, x and fh_amm's operands: 16-byte aligned, out not u
    for scipy_mode in (0, 1):
        prob.cg_scipy = scipy_mode
        for bp, xp in ((u.data_ptr() + 8, out.data_ptr()), (u.data_ptr(), out.data_ptr() + 8)):
            assert lib.fh_cg_solve(hip.ctx.h, C.byref(prob), bp, xp, 1e-3, 0.0, 10, C.byref(info), _lib.stream()) == _lib.FH_EINVAL
    prob.cg_scipy = 0
    assert lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr() + 8, out.data_ptr(), _lib.stream()) == _lib.FH_EINVAL
    assert lib.fh_amm(hip.ctx.h, C.byref(prob), out.data_ptr(), out.data_ptr(), _lib.stream()) == _lib.FH_EINVAL  # out == u
    assert g.untouched(123.0)  # nothing was launched


# ---------------------------------------------------------------- 6. through the stack
def test_operator_methods(dev):
    """forward = mask * (H x + n) with ONE draw at the grid's shape, transpose = forward_adjoint = H (mask * v), for the scalar
    level and for a noise map"""
    S = 30
    x = inputs.randn((1, 3, S, S), 71).to(dev)
    for kw in ({}, dict(noise_map=_sigma_map(S, 5))):
        op = _op(S, dev, **kw)
        hx = fr.hartley2(x.cpu()).to(dev)
        y = op.forward(x, noiseless=True)
        assert y.dtype == x.dtype and tuple(y.shape) == (1, 3, S, S) and maxabs(y, op.mask * hx) <= 1e-12 * float(hx.abs().max())
        assert bool((y[op.mask == 0] == 0).all())
        torch.manual_seed(7)
        noisy = op.forward(x)
        torch.manual_seed(7)
        n = torch.randn(1, 3, S, S, dtype=y.dtype, device=dev)
        sig = op.sigma_s.to(y.dtype) if op.noise_map is None else torch.where(op.mask > 0, op.noise_map, torch.zeros_like(op.noise_map))
        assert maxabs(noisy, op.mask * (hx + sig * n)) <= 1e-12 * float(hx.abs().max()) and op._last_y is noisy
        back = op.transpose(y)
        assert maxabs(back, fr.hartley2((op.mask * y).cpu())) <= 1e-12 * float(hx.abs().max())
        assert torch.equal(back, op.forward_adjoint(y)) and torch.equal(back, op.transpose(y.reshape(1, -1), flatten=True))
        v = inputs.randn((1, 3, S, S), 72).to(dev)
        lhs, rhs = float((op.forward(x, noiseless=True) * v).sum()), float((x * op.forward_adjoint(v)).sum())
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_lockstep_online_covariance_runs(dev, gold, tmp_path):
    """conditional_sampler_grouped (online_covariance, the batched solve) over two images with their own masks, then one
    per-image run: completion and finite outputs"""
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_grouped
    B, S = 2, 64
    torch.save(torch.from_numpy(gold("trajectories")["dct_variance64"]), tmp_path / "dct_variance.pt")
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(tmp_path, {})
    ops, ys, noise = [], [], []
    for b in range(B):
        op = _op(S, dev, slot=b, pattern="cartesian", acceleration=4.0, seed=b)
        ops.append(op)
        ys.append(op.forward(0.5 * inputs.smooth_image(S, 70 + b).to(dev)))
        noise.append(inputs.randn((1, 3, S, S), 90 + b, torch.float32))
    noise = torch.cat(noise).to(dev)
    run = dict(num_steps=3, sigma_min=0.5, sigma_max=80, rho=7, solver="euler")
    xb = conditional_sampler_grouped(net, noise, ys, ops, groups=1, **run, **kw)
    x1, _, _ = conditional_sampler(net, noise[:1], None, None, measurement=ys[0], operator=ops[0], **run, **kw)
    torch.cuda.synchronize()
    assert tuple(xb.shape) == (B, 3, S, S) and bool(torch.isfinite(xb).all())
    assert tuple(x1.shape) == (1, 3, S, S) and bool(torch.isfinite(x1).all())


@pytest.mark.parametrize("mechanism", ["dps", "diffpir"])
def test_other_mechanisms_run(dev, tmp_path, mechanism):
    """DPS reaches the operator through forward / forward_adjoint, DiffPIR through the solver on the identity basis (use_dct = 0,
    P = Hc): two Euler steps stay finite"""
    from free_hunch_amd.sampler import conditional_sampler
    S = 64
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(tmp_path, {"conditioning_mechanism": mechanism, "diffpir_lambda": 10.0})
    op = _op(S, dev)
    y = op.forward(0.5 * inputs.smooth_image(S, 75).to(dev))
    noise = inputs.randn((1, 3, S, S), 95, torch.float32).to(dev)
    x1, _, _ = conditional_sampler(net, noise, None, None, measurement=y, operator=op, num_steps=3, sigma_min=0.5, sigma_max=80,
                                   rho=7, solver="euler", **kw)
    assert tuple(x1.shape) == (1, 3, S, S) and bool(torch.isfinite(x1).all())


def test_cli_fourier_sampling(tmp_path):
    import PIL.Image
    sys.path.insert(0, ROOT)
    from bench import smooth_images
    import generate_conditional as gc
    data = tmp_path / "data"
    data.mkdir()
    for i, im in enumerate(smooth_images(1, 256, 7)):
        PIL.Image.fromarray(im.permute(1, 2, 0).numpy(), "RGB").save(data / f"img{i:08d}.png")
    out = tmp_path / "out"
    gc.main([f"--outdir={out}", f"--dataset_path={data}", "--synthetic_weights=ffhq", "--num_steps=3", "--solver=euler",
             "--sigma_min=0.5", "--total_images=1", "--max_batch_size=1", "--operator_name=fourier_sampling",
             "--kspace_pattern=cartesian", "--kspace_acceleration=4",
             "--conditioning_mechanism=online_covariance", "--image_base_covariance=dct_diagonal"])
    names = ["000000_000000.png"]
    for folder in ("images", "cond_images", "forward_images"):  # forward_images holds the zero-filled reconstruction A0^T y
        assert sorted(os.listdir(out / folder)) == names, folder
        im = PIL.Image.open(out / folder / names[0])
        assert im.mode == "RGB" and im.size == (256, 256) and np.asarray(im).std() > 0
    txt = open(out / "results.txt").read()
    assert "PSNR" in txt and "SSIM" in txt
