"""`burst_sr` on the device: the multi-frame operator pair (fh_conv_frames, fused and chain routes), fh_problem.op = 12 from one
application of A_mm up to the CLI.

The reference is built here from the oracle's primitives: with FB_k = p2o(PSF_k) in complex128 (float64 PSFs, the float32 values
the operator holds),
    fwd(v)  = stack_k decimate(ifft2(FB_k fft2(v)).real, s)            [N,3,S,S]   -> [N,3K,So,So], channel 3 k + c
    adj(u)  = sum_k ifft2(conj(FB_k) fft2(zero_insert(u_k, s))).real   [N,3K,So,So] -> [N,3,S,S]
    A_mm(u) = s2 u + fwd(C(adj(u))),   C = the oracle covariance's denoiser_cov_vector_dot.
The frames come from the 7 x 7 binomial PSF under `shifted_psf`: K = s^2 integer shifts, three fractional shifts (49, 64 and 64
taps: ragged frames) and K = 1.  The bars are those of tests/test_custom_sr_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import inputs
import nets
import test_custom_sr_gpu as srt
from test_burst_sr_host import FRACTIONAL, PSF7, integer_shifts
from test_channel_ops_gpu import _amm, _run_script
from test_custom_sr_host import binomial_psf
from test_hip_parity import _base_kwargs, maxabs

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "free-hunch_amd", "data")
SIGMA_S = 0.05
FUSED = [(64, 2), (64, 4), (96, 3)]
# So = 20: neither frame kernel tiles the image; (100, 4) and (60, 3): sides that are no multiple of 16, So = 25 (odd) and 20
CHAIN = [(80, 4), (100, 4), (60, 3)]
FOUR = [(0, 0), (0, 2), (2, 0), (2, 2)]  # K = 4 integer shifts at s = 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _shifts(s, kind):
    return {"int": integer_shifts(s), "frac": FRACTIONAL, "one": [(0, 0)], "four": FOUR}[kind]


def _op(S, s, kind, dev, slot=0, shifts=None):
    from free_hunch_amd.measurements import get_operator
    op = get_operator(name="burst_sr", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), scale_factor=s, kernels=[PSF7],
                      frame_shifts=_shifts(s, kind) if shifts is None else shifts)
    op.ctx_slot = slot
    return op


def _route(op, adjoint):
    from free_hunch_amd import _lib
    out = (C.c_int32 * 6)()
    ft = op.frame_taps
    assert _lib.load().fh_conv_frames_plan(op.in_shape[-1], ft.nframes, ft.max_taps, ft.halo, 3, op.scale_factor, adjoint, out) == 0
    return out[0]


class Ref:
    """the reference pair of a burst operator, float64 on the CPU"""

    def __init__(self, op):
        from oracle import fh_oracle as fo
        self.fo, self.s, S = fo, op.scale_factor, op.in_shape[-1]
        self.FB = [fo.p2o(torch.from_numpy(k.astype(np.float64))[None, None], (S, S)) for k in op.kernels]
        assert self.FB[0].dtype == torch.complex128
        self.s2 = torch.tensor([SIGMA_S], dtype=torch.float32).clip(min=0.001).clip(min=1e-2) ** 2  # the oracle's SR rule

    def fwd(self, v):
        F = torch.fft.fft2(v)
        return torch.cat([self.fo.decimate(torch.fft.ifft2(FB * F).real, self.s) for FB in self.FB], 1)

    def adj(self, u):
        return sum(torch.fft.ifft2(torch.conj(FB) * torch.fft.fft2(self.fo.zero_insert(u[:, 3 * k:3 * k + 3], self.s))).real
                   for k, FB in enumerate(self.FB))

    def system(self, orc, shape):
        def A_mm(u):
            u = u.reshape(shape)
            return (self.s2 * u + self.fwd(orc.denoiser_cov_vector_dot(self.adj(u)))).flatten()
        return A_mm


def _pair(op, x, u, dev, planes):
    """fh_conv_frames forward of x [N,3,S,S] and adjoint of u [N,3K,So,So] on a context of `planes` planes, outputs pre-filled
    with NaN"""
    from free_hunch_amd import _lib
    S, s, K = op.in_shape[-1], op.scale_factor, op.nframes
    N = planes // 3
    ctx = _lib.Context.get(S, planes, 0)
    f = ctx.blur_frames(x[:N].contiguous(), torch.full((N, 3 * K, S // s, S // s), float("nan"), dtype=F64, device=dev),
                        op.frame_taps, planes, s)
    a = ctx.blur_frames(u[:N].contiguous(), torch.full((N, 3, S, S), float("nan"), dtype=F64, device=dev), op.frame_taps, planes, s,
                        adjoint=True)
    torch.cuda.synchronize()
    return f, a


# ---------------------------------------------------------------- 1. the operator pair against the reference
@pytest.mark.parametrize("S,s,kind", [(S, s, k) for S, s in FUSED + CHAIN for k in ("int", "frac", "one")] + [(256, 4, "int")])
def test_operator_pair_against_the_reference(dev, S, s, kind):
    """forward and adjoint within 1e-12 max(1, max|ref|) for 3 and for 9 planes (a NaN left in the output fails); the first image
    of the 9-plane run equals the 3-plane run bit for bit; <A x, u> = <x, A^T u> to 1e-10."""
    op = _op(S, s, kind, dev)
    K, So = op.nframes, S // s
    assert (_route(op, 0), _route(op, 1)) == ((0, 0) if (S, s) in CHAIN else (1, 1))
    ref = Ref(op)
    x, u = inputs.randn((3, 3, S, S), 11), inputs.randn((3, 3 * K, So, So), 12)
    rf, ra = ref.fwd(x), ref.adj(u)
    got = {}
    for planes in (3, 9):
        N = planes // 3
        f, a = _pair(op, x.to(dev), u.to(dev), dev, planes)
        e_f, e_a = maxabs(f, rf[:N]), maxabs(a, ra[:N])
        print(f"frames S={S} s={s} K={K} planes={planes}: forward {e_f / max(1.0, float(rf.abs().max())):.2e} adjoint "
              f"{e_a / max(1.0, float(ra.abs().max())):.2e}", flush=True)
        assert e_f < 1e-12 * max(1.0, float(rf[:N].abs().max()))
        assert e_a < 1e-12 * max(1.0, float(ra[:N].abs().max()))
        got[planes] = (f, a)
    assert torch.equal(got[9][0][:1], got[3][0]) and torch.equal(got[9][1][:1], got[3][1])
    f, a = got[9]
    lhs, rhs = float((f * u.to(dev)).sum()), float((x.to(dev) * a).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


# ---------------------------------------------------------------- 2. fused = chain, bit for bit
@pytest.mark.parametrize("S,s", FUSED)
@pytest.mark.parametrize("kind", ["int", "frac"])
def test_fused_route_equals_the_chain_bit_for_bit(dev, tmp_path_factory, monkeypatch, S, s, kind):
    """FH_FRAMES_FUSED=0 against the default: forward and adjoint of fh_conv_frames on 9 planes, and A_mm (the forward with its
    sigma_y^2 u add) on op 12, agree in every bit."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    op = _op(S, s, kind, dev)
    K, So = op.nframes, S // s
    x, u = inputs.randn((3, 3, S, S), 13).to(dev), inputs.randn((3, 3 * K, So, So), 14).to(dev)
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    prob, keep = _problem(op, hip, _sigma_y2(op))
    monkeypatch.delenv("FH_FRAMES_FUSED", raising=False)
    f1, a1 = _pair(op, x, u, dev, 9)
    amm1 = _amm(hip, prob, u[:1].contiguous())
    monkeypatch.setenv("FH_FRAMES_FUSED", "0")
    f0, a0 = _pair(op, x, u, dev, 9)
    amm0 = _amm(hip, prob, u[:1].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(f0, f1) and torch.equal(a0, a1) and torch.equal(amm0, amm1)
    assert bool(torch.isfinite(amm1).all()) and float(amm1.abs().max()) > 0


@pytest.mark.parametrize("S,s", FUSED + CHAIN)
def test_one_frame_equals_fh_conv_circ_on_both_routes(dev, monkeypatch, S, s):
    from free_hunch_amd import _lib
    op = _op(S, s, "one", dev)
    So = S // s
    x, u = inputs.randn((3, 3, S, S), 15).to(dev), inputs.randn((3, 3, So, So), 16).to(dev)
    ctx = _lib.Context.get(S, 9, 0)
    cf = ctx.conv(x, torch.empty(3, 3, So, So, dtype=F64, device=dev), op.frames[0], 9, s, False)
    ca = ctx.conv(u, torch.empty(3, 3, S, S, dtype=F64, device=dev), op.frames[0], 9, s, True)
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("FH_FRAMES_FUSED", raising=False)
        else:
            monkeypatch.setenv("FH_FRAMES_FUSED", switch)
        f, a = _pair(op, x, u, dev, 9)
        assert torch.equal(f, cf) and torch.equal(a, ca), switch


# ---------------------------------------------------------------- 3. integer shifts mean what the docstring says
@pytest.mark.parametrize("S,s", FUSED + CHAIN)
def test_integer_shift_is_a_roll_of_the_scene(dev, S, s):
    """frame k of forward(x, noiseless=True) equals custom_sr's forward of roll(x, (-dy_k, -dx_k)) with the unshifted PSF, bit for
    bit: the frame samples the blurred scene at (s i + dy_k, s j + dx_k)"""
    from free_hunch_amd.measurements import get_operator
    op = _op(S, s, "int", dev)
    one = get_operator(name="custom_sr", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), scale_factor=s, kernel=PSF7)
    x = inputs.randn((1, 3, S, S), 17).to(dev)
    y = op.forward(x, noiseless=True)
    assert tuple(y.shape) == tuple(op.out_shape) == (1, 3 * s * s, S // s, S // s) and y.dtype == x.dtype
    for k, (dy, dx) in enumerate(integer_shifts(s)):
        assert torch.equal(y[:, 3 * k:3 * k + 3], one.forward(torch.roll(x, (-dy, -dx), (-2, -1)), noiseless=True)), (k, dy, dx)
    back = op.transpose(y)
    assert tuple(back.shape) == (1, 3, S, S) and torch.equal(back, op.forward_adjoint(y))
    assert torch.equal(back, op.transpose(y.reshape(1, -1), flatten=True))
    torch.manual_seed(7)
    noisy = op.forward(x)
    torch.manual_seed(7)  # ONE draw at the shape of the whole burst
    assert torch.equal(noisy, y + op.sigma_s.to(y.dtype) * torch.randn(*op.out_shape, dtype=y.dtype, device=dev))


# ---------------------------------------------------------------- 4. one application of A_mm
def _amm_case(dev, tmp_factory, S, s, kind, n_script):
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    So = S // s
    orc, hip = srt._cov_pair(S, n_script, tmp_factory, dev)
    op = _op(S, s, kind, dev)
    K = op.nframes
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.op == 12 and prob.stride == s and prob.m == 2 * n_script and prob.use_dct == 1 and prob.ntaps2 == K
    shape = (1, 3 * K, So, So)
    A_mm = Ref(op).system(orc, shape)
    u, v = inputs.randn(shape, 21).to(dev), inputs.randn(shape, 22).to(dev)
    au, av = _amm(hip, prob, u), _amm(hip, prob, v)
    ref = A_mm(u.cpu().flatten()).reshape(shape)
    err = maxabs(au, ref) / float(ref.abs().max())
    l, r = float((u * av).sum()), float((au * v).sum())
    print(f"amm op=12 S={S} s={s} K={K} m={prob.m}: {err:.2e}, symmetry {abs(l - r) / max(abs(l), 1.0):.2e}", flush=True)
    assert err <= 1e-8
    assert abs(l - r) <= 1e-9 * max(abs(l), 1.0)


@pytest.mark.parametrize("n_script", [0, 4])
@pytest.mark.parametrize("S,s,kind", [(64, 2, "int"), (64, 4, "int"), (64, 4, "frac"), (96, 3, "int"), (96, 3, "frac"),
                                      (80, 4, "int"), (80, 4, "frac")])
def test_amm_vs_reference_system(dev, tmp_path_factory, S, s, kind, n_script):
    """fh_amm with op = 12 against s2 u + fwd(C(adj(u))) on the shipped DCT prior cut to S, before any update (m = 0) and after 4
    scripted update pairs (m = 8): 1e-8 of max|ref| and symmetry to 1e-9, the bars of test_amm_folded_sr_vs_oracle_system"""
    _amm_case(dev, tmp_path_factory, S, s, kind, n_script)


def test_amm_vs_reference_system_at_the_real_size(dev, tmp_path_factory):
    _amm_case(dev, tmp_path_factory, 256, 4, "int", 0)


@pytest.mark.parametrize("n_script", [0, 4])
def test_amm_one_frame_equals_op_2(dev, tmp_path_factory, monkeypatch, n_script):
    """K = 1 is custom_sr on its tap list (FH_NO_FOLD=1 keeps the rank-1 PSF off the rectangular bases): the same bits"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    from free_hunch_amd.measurements import get_operator
    monkeypatch.setenv("FH_NO_FOLD", "1")
    S, s = 64, 4
    _orc, hip = srt._cov_pair(S, n_script, tmp_path_factory, dev)
    op = _op(S, s, "one", dev)
    one = get_operator(name="custom_sr", device=dev, sigma_s=SIGMA_S, in_shape=(1, 3, S, S), scale_factor=s, kernel=PSF7)
    p12, k12 = _problem(op, hip, _sigma_y2(op))
    p2, k2 = _problem(one, hip, _sigma_y2(one))
    assert p12.op == 12 and p2.op == 2 and p12.sigma_y2 == p2.sigma_y2
    u = inputs.randn((1, 3, S // s, S // s), 23).to(dev)
    assert torch.equal(_amm(hip, p12, u), _amm(hip, p2, u))


def test_identity_prior_stays_on_op_12(dev):
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S, s = 64, 4
    op = _op(S, s, "four", dev)
    cov = hc.ScalarCovariance(0.7, 3 * S * S, dev)  # C = 0.7 I in image space, what the scalar-variance mechanisms solve with
    prob, keep = _problem(op, cov, _sigma_y2(op))
    assert prob.op == 12 and prob.use_dct == 0 and prob.stride == 4 and prob.ntaps2 == 4 and not prob.fold_fwd_w
    shape = (1, 12, S // s, S // s)
    u = inputs.randn(shape, 24).to(dev)
    ref = Ref(op)
    want = float(ref.s2) * u.cpu() + 0.7 * ref.fwd(ref.adj(u.cpu()))
    assert maxabs(_amm(cov, prob, u), want) <= 1e-8 * float(want.abs().max())


# ---------------------------------------------------------------- 5. the solve
def _solve_inputs(op, S, s):
    So, K = S // s, op.nframes
    ref = Ref(op)
    x_true = inputs.smooth_image(S, 31).to(F64)
    y = ref.fwd(x_true) + SIGMA_S * inputs.randn((1, 3 * K, So, So), 32)
    x0_mean = x_true + 0.05 * inputs.randn((1, 3, S, S), 33)
    return ref, y, x0_mean, (y - ref.fwd(x0_mean)).flatten()


@pytest.mark.parametrize("S,s,kind", [(64, 4, "four"), (96, 3, "frac")])
def test_six_iterations_vs_oracle_cg(dev, tmp_path_factory, S, s, kind):
    """six forced iterations on both sides agree to 1e-5 of max|mat|"""
    from oracle import fh_oracle as fo
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda
    orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    op = _op(S, s, kind, dev)
    ref, y, x0_mean, b = _solve_inputs(op, S, s)
    m6h = solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, rtol=1e-300, maxiter=6)
    sol6, info6 = fo.cg(ref.system(orc, tuple(y.shape)), b, rtol=0.0, maxiter=6)
    m6o = ref.adj(sol6.reshape(y.shape))
    short = maxabs(m6o, m6h) / float(m6o.abs().max())
    print(f"burst solve S={S} s={s} K={op.nframes}: six iterations {short:.2e}", flush=True)
    assert info6["niter"] == 6 and tuple(m6h.shape) == (1, 3, S, S)
    assert short <= 1e-5


def test_converged_solve_meets_its_tolerance(dev, tmp_path_factory):
    """(64, 4, K = 4 integer shifts, sigma_s = 0.05, m = 0) at rtol = 1e-4: `optimal` before the 5000-iteration cap, and the true
    residual of the returned solution, recomputed with an independent fh_amm, is <= 1.05 rtol ||b||.  (The oracle's cg() on this
    kind of system stops `optimal` after roughly 1400 iterations; 1e-6 on the K = s^2 systems would sit near the cap.)"""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda
    S, s = 64, 4
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    op = _op(S, s, "four", dev)
    _ref, y, x0_mean, b = _solve_inputs(op, S, s)
    rtol, info_h = 1e-4, []
    solve_customcuda(op, y.to(dev), x0_mean.to(dev), hip, 1.0, 1.0, info_h, rtol=rtol)
    u_h = solve_customcuda.last_solution.clone()
    prob, keep = _problem(op, hip, _sigma_y2(op))
    assert prob.op == 12 and prob.m == 0 and tuple(u_h.shape) == tuple(y.shape)
    bd = b.reshape(y.shape).to(dev)
    res = float((bd - _amm(hip, prob, u_h)).norm())
    print(f"burst solve rtol 1e-4: device {info_h[0]['niter']} it, true residual {res / float(bd.norm()):.3e} ||b||", flush=True)
    assert info_h[0]["optimal"] and 1 <= info_h[0]["niter"] < 5000
    assert res <= 1.05 * rtol * float(bd.norm())


# ---------------------------------------------------------------- 6. batched = single
@pytest.mark.parametrize("route", ["fused", "chain"])
@pytest.mark.parametrize("n_script", [0, 4])
def test_batched_solve_equals_single(dev, tmp_path, monkeypatch, n_script, route):
    """fh_cg_solve_batched with op = 12 over 2 images with their own measurements and covariances against per-image solves by the
    rule of test_batched_folded_sr_solve_equals_single: identical iteration counts, `mat` within 1e-12 of max|mat|.  The images
    stop at different iterations, so the kernels skip the finished image from then on - on the chain (FH_FRAMES_FUSED=0) every
    launch carries ONE image and asks that image's own control block."""
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda, solve_customcuda_batched
    if route == "chain":
        monkeypatch.setenv("FH_FRAMES_FUSED", "0")
    else:
        monkeypatch.delenv("FH_FRAMES_FUSED", raising=False)
    S, s, nimg = 64, 4, 2
    So = S // s
    dv = torch.load(os.path.join(DATA, "dct_variance.pt"), weights_only=True)[:, :S, :S].contiguous()
    torch.save(dv, tmp_path / "dct_variance.pt")
    ops, covs, ys, xs = [], [], [], []
    for b in range(nimg):
        op = _op(S, s, "four", dev, slot=b)
        cov = hc.CovarianceHessianBFGSDCT(str(tmp_path), 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=b)
        if n_script:
            _run_script(cov, inputs.script(1300 + b, (1, 3, S, S), n_script, 80.0, sig_end=[20.0, 0.5][b]), dev)
        else:
            x = inputs.randn((1, 3, S, S), 300 + b).to(dev) * 40.0
            cov.update_time_step(x, 80.0, [40.0, 12.0][b], -x / 80.0 ** 2 * 0.5)
        x0 = inputs.smooth_image(S, 310 + b).to(dev)
        ys.append(op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 12, So, So), 320 + b, torch.float32).to(dev))
        xs.append((0.3 * x0).to(F64))
        ops.append(op)
        covs.append(cov)
    assert all(c.famC.m == 2 * n_script for c in covs) and _problem(ops[0], covs[0], _sigma_y2(ops[0]))[0].op == 12
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
    print(f"batched burst solve m={2 * n_script} {route}: iterations {n_b}", flush=True)
    assert min(n_b) < max(n_b), n_b  # an image finished first: the `done` skip ran


RAGGED_A = [(0, 0), (0.5, 0.5), (0.5, 0)]  # 49, 64 and 56 taps
RAGGED_B = [(0, 0), (0.5, 0), (0.5, 0.5)]  # 49, 56 and 64 taps: same total, same longest frame, same extents


@pytest.mark.parametrize("S,s,switch", [(80, 4, None), (64, 4, "0")])
def test_chain_graph_is_not_replayed_for_other_frame_offsets(dev, tmp_path_factory, monkeypatch, S, s, switch):
    """The chain route slices the tap lists on the host, so a captured chunk of CG iterations holds the frame boundaries.  Two
    bursts whose problems agree in every field and pointer but not in the offsets BEHIND tap2_dy - permuted ragged frames written
    into the same device buffers, as an allocator hands them back - must not share a cached graph: the second solve equals, bit
    for bit, the solve of a freshly built operator with the permuted frames, and differs from the first."""
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2, solve_customcuda
    if switch is None:
        monkeypatch.delenv("FH_FRAMES_FUSED", raising=False)
    else:
        monkeypatch.setenv("FH_FRAMES_FUSED", switch)
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    a, b = _op(S, s, None, dev, shifts=RAGGED_A), _op(S, s, None, dev, shifts=RAGGED_B)
    fa, fb = a.frame_taps, b.frame_taps
    assert [t.n for t in a.frames] == [49, 64, 56] and [t.n for t in b.frames] == [49, 56, 64]
    assert (fa.n, fa.max_taps, fa.halo) == (fb.n, fb.max_taps, fb.halo) and fa.off.tolist() != fb.off.tolist()
    if switch is None:
        assert (_route(a, 0), _route(a, 1)) == (0, 0)
    So = S // s
    y = inputs.randn((1, 9, So, So), 41).to(dev)
    x0 = inputs.smooth_image(S, 42).to(dev).to(F64)
    solve = lambda op: solve_customcuda(op, y, x0, hip, 1.0, 1.0, rtol=1e-300, maxiter=16).clone()  # noqa: E731
    before = bytes(_problem(a, hip, _sigma_y2(a))[0])
    first = solve(a)
    for dst, src in ((fa.dy, fb.dy), (fa.dx, fb.dx), (fa.w, fb.w), (fa.off, fb.off)):  # the same buffers, the other burst
        dst.copy_(src)
    a.kernels, a.frames = b.kernels, b.frames
    torch.cuda.synchronize()
    assert bytes(_problem(a, hip, _sigma_y2(a))[0]) == before  # the struct, pointers included, cannot tell the two apart
    second, fresh = solve(a), solve(b)
    assert torch.equal(second, fresh)
    assert not torch.equal(second, first) and bool(torch.isfinite(second).all())


def test_batched_solve_refuses_different_psfs_and_factors(dev):
    from free_hunch_amd import covariance as hc
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda_batched
    S = 64
    covs = [hc.CovarianceHessianBFGS(1, 80.0 ** 2, 3 * S * S, device=dev, ctx_slot=b) for b in range(2)]
    z = torch.zeros(1, 3, S, S, dtype=F64, device=dev)
    ops = [_op(S, 4, "four", dev, slot=0), _op(S, 4, "four", dev, slot=1, shifts=FOUR[:3] + [(2, 3)])]  # one frame differs
    with pytest.raises(AssertionError, match="PSF"):
        solve_customcuda_batched(ops, [z, z], [z, z], covs, 1.0, 0.4)
    ops = [_op(S, 4, "four", dev, slot=0), _op(S, 2, "four", dev, slot=1)]
    with pytest.raises(AssertionError, match="scale_factor"):
        solve_customcuda_batched(ops, [z, z], [z, z], covs, 1.0, 0.4)


# ---------------------------------------------------------------- 7. refusals without a launch
def test_op12_refuses_bad_problems_without_launching(dev, tmp_path_factory):
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    S, s = 64, 4
    So = S // s
    _orc, hip = srt._cov_pair(S, 0, tmp_path_factory, dev)
    op = _op(S, s, "four", dev)  # K = 4 frames of 49 taps
    u = inputs.randn((1, 12, So, So), 61).to(dev)
    out = torch.full_like(u, 123.0)
    info = _lib.FhCgInfo()
    some = u.data_ptr()
    bad_off = torch.tensor([0, 49, 40, 147, 196], dtype=torch.int32, device=dev)  # not increasing: refused once read back
    long_off = torch.tensor([0, 50, 98, 147, 196], dtype=torch.int32, device=dev)  # a frame longer than halo2
    for field, value in (("stride", 1), ("stride", 0), ("stride", 5), ("stride", 3), ("stride", 8), ("ntaps2", 0), ("ntaps2", -1),
                         ("ntaps2", 17), ("halo2", 0), ("halo2", 1025), ("halo2", 48), ("ntaps", 3), ("ntaps", 197),
                         ("tap2_dy", None), ("tap2_dy", bad_off.data_ptr()), ("tap2_dy", long_off.data_ptr()),
                         ("tap2_dx", some), ("tap2_w", some), ("fold_fwd_w", some), ("fold_fwd_h", some), ("fold_inv_w", some),
                         ("fold_inv_h", some), ("fold_sym", 1), ("mask", some), ("halo", 6), ("op", 13)):
        prob, keep = _problem(op, hip, _sigma_y2(op))
        assert prob.op == 12
        setattr(prob, field, value)
        rc = hip.ctx.lib.fh_amm(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
        rc = hip.ctx.lib.fh_cg_solve(hip.ctx.h, C.byref(prob), u.data_ptr(), out.data_ptr(), 1e-3, 0.0, 10, C.byref(info),
                                     _lib.stream())
        assert rc == _lib.FH_EINVAL, (field, value, rc)
    prob, keep = _problem(op, hip, _sigma_y2(op))  # the batched entry point: no mask on the low-resolution measurement
    per = _lib.FhBatch()
    per.nimg = 1
    per.D[0], per.r[0], per.B[0], per.M[0], per.mask[0] = prob.D, prob.r, prob.B, prob.M, some
    rtol = (C.c_double * 1)(1e-3)
    rc = hip.ctx.lib.fh_cg_solve_batched(hip.ctx.h, C.byref(prob), C.byref(per), u.data_ptr(), out.data_ptr(), rtol, 0.0, 10,
                                         C.byref(info), _lib.stream())
    assert rc == _lib.FH_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())  # nothing was launched


def test_conv_frames_refuses_bad_arguments_without_launching(dev):
    from free_hunch_amd import _lib
    S, s = 64, 4
    op = _op(S, s, "four", dev)
    ft = op.frame_taps
    ctx = _lib.Context.get(S, 3, 0)
    x = torch.zeros(1, 3, S, S, dtype=F64, device=dev)
    out = torch.full((2, 12, S // s, S // s), 123.0, dtype=F64, device=dev)
    call = lambda *a: ctx.lib.fh_conv_frames(*a, _lib.stream())  # noqa: E731
    p = lambda t: t.data_ptr()  # noqa: E731
    good = (ctx.h, p(x), p(out), p(ft.dy), p(ft.dx), p(ft.w), p(ft.off))
    tail = (ft.nframes, ft.max_taps, ft.halo, 3, s, 0)
    for missing in range(7):
        args = list(good)
        args[missing] = None
        assert call(*args, *tail) == _lib.FH_EINVAL, missing
    for change in ((0, 0), (0, 17), (1, 0), (1, 1025), (1, 48), (2, 6), (3, 0), (3, 4), (4, 1), (4, 5), (4, 3), (5, 2)):
        t = list(tail)
        t[change[0]] = change[1]
        assert call(*good, *t) == _lib.FH_EINVAL, change
    assert call(ctx.h, p(x), p(x), *good[3:], *tail) == _lib.FH_EINVAL  # in == out
    assert call(*good, ft.nframes, ft.max_taps, ft.halo, 6, s, 0) == _lib.FH_ESIZE  # more planes than the context holds
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())


# ---------------------------------------------------------------- 8. the lock-step sampler
def test_lockstep_burst_equals_per_image(dev, gold, tmp_path):
    """conditional_sampler_grouped(groups = 1) over two images against per-image conditional_sampler runs by the rule of
    test_lockstep_folded_sr_equals_per_image: identical niter and k lists, outputs within 1e-3; Euler with 4 steps, nets.gauss_net,
    sigma_min = 0.5 (the last call's CG tolerance stays near 1e-2)"""
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_grouped
    B, S, s = 2, 64, 4
    So = S // s
    torch.save(torch.from_numpy(gold("trajectories")["dct_variance64"]), tmp_path / "dct_variance.pt")
    net = nets.gauss_net(S, dev)
    kw = _base_kwargs(tmp_path, {})
    ops, ys, noise = [], [], []
    for b in range(B):
        op = _op(S, s, "four", dev, slot=b)
        ops.append(op)
        x0 = 0.5 * inputs.smooth_image(S, 70 + b).to(dev)
        ys.append(op.forward(x0, noiseless=True) + SIGMA_S * inputs.randn((1, 12, So, So), 80 + b, torch.float32).to(dev))
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
    print(f"lock-step burst SR: iterations {[t['niter'] for t in tb[0]]}", flush=True)


# ---------------------------------------------------------------- 9. the CLI
def test_cli_burst_sr(tmp_path):
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
    gc.main([f"--outdir={out}", f"--dataset_path={data}", "--synthetic_weights=ffhq", "--num_steps=3", "--solver=euler",
             "--sigma_min=0.5", "--total_images=2", "--max_batch_size=2", "--operator_name=burst_sr",
             f"--kernel_path={tmp_path / 'psf.npy'}", "--scale_factor=4", "--frame_shifts=0,0;0,2;2,0;2,2",
             "--conditioning_mechanism=online_covariance", "--image_base_covariance=dct_diagonal"])
    names = ["000000_000000.png", "000001_000000.png"]
    for folder in ("images", "cond_images"):
        assert sorted(os.listdir(out / folder)) == names, folder
        for n in names:
            im = PIL.Image.open(out / folder / n)
            assert im.mode == "RGB" and im.size == (256, 256) and np.asarray(im).std() > 0
    assert os.listdir(out / "forward_images") == []  # low-resolution measurements are not written, as for custom_sr
    txt = open(out / "results.txt").read()
    assert "PSNR" in txt and "SSIM" in txt
