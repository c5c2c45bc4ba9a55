"""Host-side checks of `burst_sr` (multi-frame super-resolution, one PSF per frame): registry and attributes, every refusal,
`shifted_psf`, the CLI flags, the operator code and name lists, and the launch plan of fh_conv_frames.  No GPU: the operators
are built on device="cpu" and the plan queries need neither a context nor a device."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_custom_sr_host import binomial_psf

LDS_OPT_IN = 100 * 1024  # kLdsOptIn: the dynamic-LDS opt-in the frame kernels share with k_conv_dec / k_conv_up
PSF7 = binomial_psf(7, 7)


def integer_shifts(s):
    return [(a, b) for a in range(s) for b in range(s)]


FRACTIONAL = [(0.0, 0.0), (0.5, 1.25), (2.75, 0.5)]  # K = 3: 49, 64 and 64 taps - ragged frames


def _burst(S=64, **kw):
    from free_hunch_amd.measurements import get_operator
    kw.setdefault("scale_factor", 4)
    if "kernels" not in kw and "kernel_path" not in kw:
        kw["kernels"] = [PSF7]
        kw.setdefault("frame_shifts", integer_shifts(2))
    return get_operator(name="burst_sr", device="cpu", sigma_s=0.05, in_shape=(1, 3, S, S), **kw)


# ---------------------------------------------------------------- registry and attributes
def test_registry_and_attributes(tmp_path):
    from free_hunch_amd.measurements import BurstSROperator, LinearOperator, Taps, shifted_psf
    op = _burst(scale_factor=4, frame_shifts=integer_shifts(4))
    assert isinstance(op, BurstSROperator) and isinstance(op, LinearOperator) and op.name == "burst_sr"
    assert op.nframes == 16 and op.scale_factor == 4 and op.out_shape == (1, 48, 16, 16) and tuple(op.in_shape) == (1, 3, 64, 64)
    assert len(op.frames) == 16 and all(isinstance(t, Taps) and t.n == 49 for t in op.frames)
    assert len(op.kernels) == 16 and all(k.dtype == np.float32 for k in op.kernels)
    assert op.folded_bases() is None and op.folded_sr_bases() is None
    ft = op.frame_taps
    assert ft.n == 16 * 49 and ft.max_taps == 49 and ft.off.dtype == torch.int32 and ft.off.tolist() == [49 * k for k in range(17)]
    assert (ft.hy, ft.hx) == (6, 6) and ft.halo == 1000 + 64 * 6 + 6  # a shift of 3 moves the reach from 3 to 6
    for k, (dy, dx) in enumerate(integer_shifts(4)):  # the operator rounds shifted_psf's result to float32, nothing else
        assert np.array_equal(op.kernels[k], shifted_psf(PSF7, dy, dx).astype(np.float32))
    ragged = _burst(frame_shifts=FRACTIONAL)
    assert ragged.nframes == 3 and [t.n for t in ragged.frames] == [49, 64, 64] and ragged.frame_taps.max_taps == 64
    assert ragged.frame_taps.off.tolist() == [0, 49, 113, 177] and ragged.out_shape == (1, 9, 16, 16)
    # K PSFs from a list, from a [K, kh, kw] array, from a file; one shift per PSF
    stack = np.stack([PSF7, binomial_psf(7, 7)[::-1].copy() * 0.5, PSF7 * 2])
    np.save(tmp_path / "burst.npy", stack)
    np.save(tmp_path / "one.npy", PSF7)
    for op in (_burst(kernels=list(stack)), _burst(kernels=stack), _burst(kernel_path=str(tmp_path / "burst.npy"))):
        assert op.nframes == 3 and all(np.array_equal(k, s.astype(np.float32)) for k, s in zip(op.kernels, stack))
    op = _burst(kernels=list(stack), frame_shifts=[(0, 0), (1, 0), (0, 1)])
    assert np.array_equal(op.kernels[1], shifted_psf(stack[1], 1, 0).astype(np.float32))
    op = _burst(kernel_path=str(tmp_path / "one.npy"), frame_shifts="0,0;0.5,1.25;2.75,0.5")  # the command line's string
    assert op.nframes == 3 and all(np.array_equal(a, b) for a, b in zip(op.kernels, ragged.kernels))
    assert _burst(kernels=[PSF7]).nframes == 1 and _burst(scale_factor=2.0).scale_factor == 2
    assert _burst(S=96, scale_factor=3, frame_shifts=integer_shifts(3)).out_shape == (1, 27, 32, 32)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [None, 0, 1, -2, 5, 8, 2.5, "4", True])
def test_scale_factor_must_be_2_3_or_4(bad):
    with pytest.raises(ValueError, match="burst_sr.*scale_factor must be 2, 3 or 4"):
        _burst(scale_factor=bad)


def test_factor_must_divide_and_leave_8_by_8():
    with pytest.raises(ValueError, match="burst_sr.*divide"):
        _burst(S=64, scale_factor=3)
    with pytest.raises(ValueError, match="burst_sr.*8 x 8"):
        _burst(S=28, scale_factor=4)
    assert _burst(S=32, scale_factor=4).out_shape == (1, 12, 8, 8)


def test_frame_count_is_1_to_s_squared():
    with pytest.raises(ValueError, match="burst_sr.*5 frames.*s\\^2 = 4"):
        _burst(scale_factor=2, frame_shifts=integer_shifts(2) + [(0.5, 0.5)])
    with pytest.raises(ValueError, match="burst_sr.*17 frames"):
        _burst(scale_factor=4, frame_shifts=integer_shifts(4) + [(0.5, 0.5)])
    with pytest.raises(ValueError, match="burst_sr"):
        _burst(kernels=[])
    assert _burst(scale_factor=2, frame_shifts=integer_shifts(2)).nframes == 4


def test_psf_sources_and_shift_counts(tmp_path):
    from free_hunch_amd.measurements import get_operator
    np.save(tmp_path / "one.npy", PSF7)
    with pytest.raises(ValueError, match="burst_sr needs exactly one of kernels"):
        get_operator(name="burst_sr", device="cpu", sigma_s=0.05, in_shape=(1, 3, 64, 64), scale_factor=4)
    with pytest.raises(ValueError, match="burst_sr needs exactly one of kernels"):
        _burst(kernels=[PSF7], kernel_path=str(tmp_path / "one.npy"))
    with pytest.raises(ValueError, match="burst_sr.*2 frame_shifts for 3 PSFs"):
        _burst(kernels=[PSF7, PSF7, PSF7], frame_shifts=[(0, 0), (1, 1)])
    with pytest.raises(ValueError, match="burst_sr.*frame_shifts"):
        _burst(kernels=[PSF7], frame_shifts="0,0;1")
    with pytest.raises(ValueError, match="burst_sr.*frame_shifts"):
        _burst(kernels=[PSF7], frame_shifts="0,zero")
    with pytest.raises(ValueError, match="burst_sr.*frame_shifts"):
        _burst(kernels=[PSF7], frame_shifts=[(0, float("nan"))])
    np.save(tmp_path / "four_d.npy", np.zeros((2, 2, 3, 3)))
    with pytest.raises(ValueError, match="burst_sr.*\\[K, kh, kw\\]"):
        _burst(kernel_path=str(tmp_path / "four_d.npy"))
    with pytest.raises(ValueError, match="burst_sr.*2-D"):
        _burst(kernels=[np.ones(3)])


def test_every_frame_psf_is_checked_by_name():
    with pytest.raises(ValueError, match="burst_sr: the PSF of frame 1 is all zero"):
        _burst(kernels=[PSF7, np.zeros((3, 3))])
    with pytest.raises(ValueError, match="burst_sr: the PSF of frame 1 is all zero"):
        _burst(kernels=[PSF7, np.full((3, 3), 1e-60)])  # zero once rounded to float32
    for bad in (np.nan, np.inf, 1e60):  # 1e60 rounds to inf in float32
        k = PSF7.copy()
        k[2, 3] = bad
        with pytest.raises(ValueError, match="burst_sr: the PSF of frame 0 has a non-finite"):
            _burst(kernels=[k, PSF7])
    wide = np.zeros((67, 3))
    wide[0, 1] = wide[33, 1] = 0.5
    with pytest.raises(ValueError, match="burst_sr: the PSF of frame 1 reaches \\(33, 0\\)"):
        _burst(kernels=[PSF7, wide])
    with pytest.raises(ValueError, match="burst_sr: the PSF of frame 1 reaches"):  # the shift counts: 3 + 30 = 33
        _burst(kernels=[PSF7], frame_shifts=[(0, 0), (30, 0)])
    dense = np.full((33, 33), 1.0 / 1089)
    with pytest.raises(ValueError, match="burst_sr: the PSF of frame 2 has 1089 non-zeros, a tap list holds 1024"):
        _burst(kernels=[PSF7, PSF7, dense])
    assert _burst(kernels=[np.full((32, 32), 1.0 / 1024)]).frames[0].n == 1024  # the limit itself is allowed


# ---------------------------------------------------------------- shifted_psf
def test_shifted_psf_integer_shift_moves_entries_exactly():
    from free_hunch_amd.measurements import shifted_psf
    rng = np.random.default_rng(5)
    k = rng.standard_normal((5, 7))
    for dy, dx in ((0, 0), (1, 0), (0, -2), (3, 2), (-4, 5)):
        out = shifted_psf(k, dy, dx)
        assert out.dtype == np.float64 and out.shape[0] % 2 == 1 and out.shape[1] % 2 == 1
        cy, cx = out.shape[0] // 2, out.shape[1] // 2
        want = np.zeros_like(out)
        for a, b in itertools.product(range(5), range(7)):  # the entry at offset (a - 2, b - 3) lands on (a - 2 - dy, b - 3 - dx)
            want[cy + a - 2 - dy, cx + b - 3 - dx] = k[a, b]
        assert np.array_equal(out, want), (dy, dx)


def test_shifted_psf_sign_convention_on_an_asymmetric_psf():
    """A frame displaced by (dy, dx) samples the blurred scene at (i + dy, j + dx): (B x)[i + dy] = sum_d k[d] x[i + dy - d], so the
    tap at offset d moves to d - dy - UP for a positive dy, LEFT for a positive dx - and the shifted blur of an image equals the
    unshifted blur of the image rolled by (-dy, -dx)."""
    from free_hunch_amd.measurements import shifted_psf
    k = np.zeros((3, 3))
    k[0, 2], k[1, 1] = 1.0, 2.0  # offsets (-1, +1) and (0, 0)
    out = shifted_psf(k, 1, -1)
    want = np.zeros((5, 5))
    want[0, 4], want[1, 3] = 1.0, 2.0  # offsets (-2, +2) and (-1, +1)
    assert np.array_equal(out, want)

    def blur(img, psf):  # circular, centre at size // 2
        acc = np.zeros_like(img)
        for a, b in zip(*np.nonzero(psf)):
            acc += psf[a, b] * np.roll(img, (a - psf.shape[0] // 2, b - psf.shape[1] // 2), (0, 1))
        return acc
    img = np.random.default_rng(6).standard_normal((12, 12))
    assert np.allclose(blur(img, out), blur(np.roll(img, (-1, 1), (0, 1)), k), rtol=0, atol=1e-14)
    assert np.allclose(blur(img, out), np.roll(blur(img, k), (-1, 1), (0, 1)), rtol=0, atol=1e-14)


def test_shifted_psf_fractional_part_is_bilinear_and_keeps_the_sum():
    from free_hunch_amd.measurements import shifted_psf
    delta = np.ones((1, 1))
    half = shifted_psf(delta, 0, 0.5)
    assert half.shape == (1, 3) and np.array_equal(half, [[0.5, 0.5, 0.0]])  # offsets -1 and 0, centre at index 1
    assert np.array_equal(shifted_psf(delta, 0.5, 0), [[0.5], [0.5], [0.0]])
    q = shifted_psf(delta, 0.25, 0.5)  # the 2 x 2 bilinear kernel
    assert np.array_equal(q[:2, :2], [[0.125, 0.125], [0.375, 0.375]]) and np.count_nonzero(q) == 4
    assert np.array_equal(shifted_psf(delta, -0.75, 0), [[0.0], [0.25], [0.75]])  # floor(-0.75) = -1, fraction 0.25
    rng = np.random.default_rng(7)
    for dy, dx in ((0.5, 1.25), (2.75, 0.5), (-3.3, 0.1), (1.0 / 3.0, -2.0 / 7.0), (4, 0.999)):
        for k in (PSF7, rng.random((6, 9))):
            out = shifted_psf(k, dy, dx)
            assert abs(out.sum() - k.sum()) <= 1e-15 * max(1.0, abs(k.sum())), (dy, dx)
            assert out.shape[0] // 2 * 2 + 1 == out.shape[0] and out.shape[1] // 2 * 2 + 1 == out.shape[1]
    with pytest.raises(ValueError, match="shifted_psf"):
        shifted_psf(np.ones(3), 0, 0)
    with pytest.raises(ValueError, match="shifted_psf"):
        shifted_psf(PSF7, float("inf"), 0)


# ---------------------------------------------------------------- solver tables and the CLI
def test_op_code_and_name_lists():
    from free_hunch_amd import conditioning_mechanisms as cm
    row = cm._OPS["burst_sr"]
    assert cm._op_code("burst_sr") == row.op == 12 and row.decimating and "'burst_sr'" in cm._BAD_OPERATOR
    assert row.layout != "mask" and row.unit_sigma != "always"  # neither a 0/1-mask operator nor a noise-map one
    for name in ("gaussian_blur", "custom_blur", "masked_blur", "custom_sr", "weighted_blur", "weighted_sr"):
        assert f"'{name}'" in cm._BAD_OPERATOR  # the older names stay
    assert cm._sigma_y2(_burst()) == pytest.approx(0.05 ** 2)
    small = _burst()
    small.sigma_s = torch.Tensor([0.001])
    assert cm._sigma_y2(small) == pytest.approx(1e-4, rel=1e-6)  # the SR rule: clip at 1e-2
    with pytest.raises(ValueError, match="Invalid operator name"):
        cm.choose_solver("burst", None, None, None)


def test_problem_fields_for_op_12():
    from free_hunch_amd import conditioning_mechanisms as cm

    class Cov:  # what _problem reads of a covariance
        use_dct, data_dim = True, 3 * 64 * 64

        class famC:
            m, B = 0, torch.zeros(1, dtype=torch.float64)

        class C:
            D = r = torch.zeros(1, dtype=torch.float64)
            M_dev = torch.zeros(1, 8, dtype=torch.float64)
    op = _burst(frame_shifts=FRACTIONAL)
    p, keep = cm._problem(op, Cov, 0.0025)
    ft = op.frame_taps
    assert (p.op, p.stride, p.ntaps, p.ntaps2, p.halo2, p.halo, p.use_dct, p.fold_sym) == (12, 4, 177, 3, 64, ft.halo, 1, 0)
    assert p.tap_dy == ft.dy.data_ptr() and p.tap_dx == ft.dx.data_ptr() and p.tap_w == ft.w.data_ptr()
    assert p.tap2_dy == ft.off.data_ptr() and not p.tap2_dx and not p.tap2_w and not p.mask
    assert not (p.fold_fwd_w or p.fold_fwd_h or p.fold_inv_w or p.fold_inv_h)
    assert all(any(t is k for k in keep) for t in (ft.dy, ft.dx, ft.w, ft.off))  # kept alive with the problem


def test_config_flags(tmp_path):
    from free_hunch_amd.config import SCHEMA, load_config
    assert SCHEMA["frame_shifts"] == (str, "")
    psf = f"--kernel_path={tmp_path}/psf.npy"
    shifts = "--frame_shifts=0,0;0.5,1.25;2,2"
    o = load_config([f"--outdir={tmp_path}", "--operator_name=burst_sr", psf, "--scale_factor=4", shifts])
    assert o.operator_name == "burst_sr" and o.kernel_path == f"{tmp_path}/psf.npy" and o.scale_factor == 4
    assert o.frame_shifts == "0,0;0.5,1.25;2,2"
    assert load_config([f"--outdir={tmp_path}", "--operator_name=burst_sr", psf, "--scale_factor=2"]).frame_shifts == ""
    with pytest.raises(SystemExit, match="burst_sr needs --kernel_path"):
        load_config([f"--outdir={tmp_path}", "--operator_name=burst_sr", "--scale_factor=4", shifts])
    for other in ("custom_sr", "custom_blur", "weighted_sr", "super_resolution", "gaussian_blur"):
        args = [f"--outdir={tmp_path}", f"--operator_name={other}", shifts]
        if other in ("custom_sr", "custom_blur", "weighted_sr"):
            args.append(psf)
        if other == "weighted_sr":
            args.append(f"--noise_map_path={tmp_path}/map.npy")
        with pytest.raises(SystemExit, match="--frame_shifts belongs to --operator_name=burst_sr"):
            load_config(args)
    with pytest.raises(SystemExit, match="custom_sr.*burst_sr"):  # --kernel_path stays refused elsewhere, and names who reads it
        load_config([f"--outdir={tmp_path}", "--operator_name=gaussian_blur", psf])
    with pytest.raises(SystemExit, match="masked_blur"):
        load_config([f"--outdir={tmp_path}", "--operator_name=burst_sr", psf, "--mask_border=2"])


# ---------------------------------------------------------------- the launch plan of fh_conv_frames
def _plan(S, K, taps, hy, hx, planes, s, adjoint, halo=None):
    from free_hunch_amd import _lib
    out = (C.c_int32 * 6)(*([7] * 6))
    rc = _lib.load().fh_conv_frames_plan(S, K, taps, 1000 + 64 * hy + hx if halo is None else halo, planes, s, adjoint, out)
    return rc, list(out)


def _lds(s, hy, hx, taps, adjoint):
    """conv_dec_lds / conv_up_lds of csrc/fh_kernels.hip, restated"""
    if not adjoint:
        hq = -(-hx // s)
        R, Wp = 15 * s + 1 + 2 * hy, 16 + 2 * hq + 1
        return ((s * R * Wp + 1) & ~1) * 8 + taps * 16
    cap = ((2 * hy + s) // s + 1) * ((2 * hx + s) // s + 1)
    Hu, Wu, T = 16 + 2 * (-(-hy // s)), 16 + 2 * (-(-hx // s)) + 1, 16 * s
    return (2 * s * s * cap + ((Hu * Wu + 1) & ~1) + T * (T + 1)) * 8


def test_plan_route_rule_over_every_legal_argument():
    """fused exactly where the direction's single-frame kernel tiles the image (So % 16 == 0 forward, S % 16 s == 0 adjoint) and
    the LDS for the union extents - tap staging for the longest frame - fits the opt-in; the chain otherwise.  The frame count
    changes nothing: the plane count is the only grid field that is not the image's."""
    from free_hunch_amd import _lib
    seen = {0: 0, 1: 0}
    for S in (64, 80, 96, 128, 256):
        for s in (2, 3, 4):
            if S % s:
                assert _plan(S, 1, 49, 3, 3, 3, s, 0)[0] == _lib.FH_EINVAL
                continue
            for hy, hx, taps, adjoint in itertools.product((0, 1, 6, 17, 32), (0, 3, 16, 32), (1, 49, 300, 1024), (0, 1)):
                answers = {K: _plan(S, K, taps, hy, hx, 3, s, adjoint) for K in sorted({1, 2, s * s})}
                assert len({(rc, tuple(out)) for rc, out in answers.values()}) == 1, (S, s, hy, hx, taps, adjoint)
                rc, out = answers[1]
                tiles = (S // s) % 16 == 0 if not adjoint else S % (16 * s) == 0
                fits = _lds(s, hy, hx, taps, adjoint) <= LDS_OPT_IN
                if rc != 0:  # the chain's own kernels do not fit either: refused by size, never fused
                    assert rc == _lib.FH_ESIZE and not (tiles and fits) and out == [0] * 6
                    continue
                assert out[0] == int(tiles and fits), (S, s, hy, hx, taps, adjoint, out)
                assert out[4] == 256
                seen[out[0]] += 1
                if out[0]:
                    n = S // (16 * s)
                    assert out[1:4] == [n, n, 3] and out[5] == _lds(s, hy, hx, taps, adjoint) <= LDS_OPT_IN
                    rc9, out9 = _plan(S, s * s, taps, hy, hx, 9, s, adjoint)  # more planes: grid z only
                    assert rc9 == 0 and out9 == out[:3] + [9] + out[4:]
                else:  # one launch of the chain: fh_conv_circ's plan for 3 planes and the longest frame
                    ref = (C.c_int32 * 6)()
                    assert _lib.load().fh_conv_circ_plan(S, taps, 1000 + 64 * hy + hx, 3, s, adjoint, ref) == 0
                    assert out[1:] == list(ref)[1:]
    assert seen[0] > 100 and seen[1] > 100
    # the shapes the device tests rely on, with the 7 x 7 binomial PSF under shifts up to s - 1
    for S, s, fused in ((64, 2, 1), (64, 4, 1), (96, 3, 1), (80, 4, 0), (256, 4, 1)):
        for adjoint in (0, 1):
            rc, out = _plan(S, s * s, 64, 3 + s, 3 + s, 3, s, adjoint)
            assert rc == 0 and out[0] == fused, (S, s, adjoint, out)


def test_plan_refuses_illegal_arguments():
    from free_hunch_amd import _lib
    good = dict(S=64, K=4, taps=49, hy=4, hx=4, planes=3, s=4, adjoint=0)
    assert _plan(**good)[0] == 0
    bad = [dict(S=0), dict(S=63), dict(S=258), dict(s=1), dict(s=5), dict(s=0), dict(s=-2), dict(s=3), dict(K=0), dict(K=-1),
           dict(K=17), dict(s=2, K=5), dict(taps=0), dict(taps=1025), dict(hy=33), dict(hx=33), dict(planes=0), dict(planes=4),
           dict(planes=-3), dict(adjoint=2), dict(adjoint=-1), dict(halo=6), dict(halo=-7), dict(halo=-105), dict(halo=999)]
    for change in bad:
        rc, out = _plan(**{**good, **change})
        assert rc == _lib.FH_EINVAL and out == [0] * 6, change
    assert _lib.load().fh_conv_frames_plan(64, 4, 49, 1260, 3, 4, 0, None) == _lib.FH_EINVAL
    assert _plan(**{**good, "planes": 65538})[0] == _lib.FH_ESIZE  # the plane is grid dimension z
