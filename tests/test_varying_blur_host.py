"""Host-side checks of `varying_blur` (a PSF that changes across the field: K blurs blended per pixel, fh_problem.op = 14):
registry and attributes, every constructor refusal, `grid_blend_weights`, the launch plan of fh_conv_blend, the problem fields,
the CLI flags and the operator code tables.  No GPU: the operators are built on device="cpu" and the plan queries need neither
a context nor a device."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_burst_sr_host import PSF7

LDS_DEFAULT, LDS_OPT_IN = 64 * 1024, 100 * 1024  # kLdsDefault / kLdsOptIn of csrc/fh_kernels.hip


def psf_family(K, wide=False):
    """K non-rank-1 PSFs with ragged tap lists: the 7 x 7 binomial PSF moved by an integer shift (49 taps), by a fractional shift
    (64 taps), and a diagonal streak with one off-diagonal entry (6 + 2 j taps), in turn.  `wide`: the last PSF is a 65 x 65
    diagonal streak, reach 32 - the widest tile the kernels stage."""
    from free_hunch_amd.measurements import shifted_psf

    def peaked(k):  # the binomial PSF is an outer product and stays one under a shift: a taller peak makes it rank 2
        k = k.copy()
        k[np.unravel_index(k.argmax(), k.shape)] *= 1.25
        return k
    out = []
    for k in range(K):
        j = k // 3
        if k % 3 == 0:
            out.append(peaked(shifted_psf(PSF7, j, -j)))
        elif k % 3 == 1:
            out.append(peaked(shifted_psf(PSF7, 0.5 + j, 1.25)))
        else:
            n = 5 + 2 * j
            streak = np.eye(n) / n
            streak[0, n - 1] = 0.1
            out.append(streak)
    if wide:
        out[-1] = np.eye(65) / 65.0
    return out


def random_maps(K, S, seed=5):
    """finite maps with negative entries, no partition of unity: any such maps are a valid linear A"""
    return np.random.default_rng(seed).standard_normal((K, 3, S, S))


def _vb(S=64, device="cpu", **kw):
    from free_hunch_amd.measurements import get_operator
    if "kernels" not in kw and "kernel_path" not in kw:
        kw["kernels"] = psf_family(4)
    if not any(k in kw for k in ("blend", "blend_path", "psf_grid")):
        kw["psf_grid"] = (2, 2)
    return get_operator(name="varying_blur", device=device, sigma_s=0.05, in_shape=(1, 3, S, S), **kw)


# ---------------------------------------------------------------- registry and attributes
def test_registry_and_attributes(tmp_path):
    from free_hunch_amd.measurements import FrameTaps, LinearOperator, Taps, VaryingBlurOperator, grid_blend_weights
    op = _vb()
    assert isinstance(op, VaryingBlurOperator) and isinstance(op, LinearOperator) and op.name == "varying_blur"
    assert op.nframes == 4 and tuple(op.in_shape) == tuple(op.out_shape) == (1, 3, 64, 64)
    assert len(op.frames) == 4 and all(isinstance(t, Taps) for t in op.frames) and isinstance(op.frame_taps, FrameTaps)
    assert [t.n for t in op.frames] == [49, 64, 6, 49]  # ragged lists
    assert len(op.kernels) == 4 and all(k.dtype == np.float32 for k in op.kernels)
    assert all(np.array_equal(k, p.astype(np.float32)) for k, p in zip(op.kernels, psf_family(4)))  # float32 rounding, nothing else
    ft = op.frame_taps
    assert ft.n == 168 and ft.max_taps == 64 and ft.off.dtype == torch.int32 and ft.off.tolist() == [0, 49, 113, 119, 168]
    assert (ft.hy, ft.hx) == (4, 5) and ft.halo == 1000 + 64 * 4 + 5  # the fractional shift (0.5, 1.25) moves the reach from 3
    assert op.blend.dtype == torch.float64 and tuple(op.blend.shape) == (4, 3, 64, 64)
    want = np.broadcast_to(grid_blend_weights(64, 2, 2)[:, None], (4, 3, 64, 64))
    assert np.array_equal(op.blend.numpy(), want)
    assert op.folded_bases() is None and op.folded_sr_bases() is None
    assert float(op.sigma_s) == pytest.approx(0.05)
    # the maps: [K,S,S], [K,3,S,S], [3K,S,S], a tensor, a file; psf_grid as a string
    maps = random_maps(4, 64)
    np.save(tmp_path / "maps.npy", maps)
    np.save(tmp_path / "psfs.npy", np.stack([np.pad(PSF7, 1) * (k + 1) for k in range(4)]))
    for kw in (dict(blend=maps), dict(blend=maps.reshape(12, 64, 64)), dict(blend=torch.from_numpy(maps)),
               dict(blend_path=str(tmp_path / "maps.npy"))):
        assert np.array_equal(_vb(**kw).blend.numpy(), maps)
    one = _vb(blend=maps[:, 0])
    assert np.array_equal(one.blend.numpy(), np.broadcast_to(maps[:, :1], (4, 3, 64, 64)))
    assert np.array_equal(_vb(psf_grid="2x2").blend.numpy(), want) and np.array_equal(_vb(psf_grid="4X1").blend.numpy()[3, 0],
                                                                                       grid_blend_weights(64, 4, 1)[3])
    filed = _vb(kernel_path=str(tmp_path / "psfs.npy"), psf_grid="1x4")
    assert filed.nframes == 4 and np.array_equal(filed.kernels[2], (np.pad(PSF7, 1) * 3).astype(np.float32))
    assert _vb(kernels=np.stack([PSF7, PSF7 * 2]), psf_grid=(1, 2)).nframes == 2
    assert _vb(kernels=PSF7, psf_grid=(1, 1)).nframes == 1 and _vb(kernels=psf_family(16), psf_grid=(4, 4)).nframes == 16
    wide = _vb(S=96, kernels=psf_family(4, wide=True))
    assert (wide.frame_taps.hy, wide.frame_taps.hx) == (32, 32) and wide.frames[-1].n == 65


def test_constructor_refusals(tmp_path):
    maps = random_maps(4, 64)
    np.save(tmp_path / "maps.npy", maps)
    np.save(tmp_path / "psfs.npy", np.stack([PSF7] * 4))
    np.save(tmp_path / "bad.npy", np.zeros((2, 2, 7, 7)))
    fam = psf_family(4)
    with pytest.raises(ValueError, match="varying_blur needs exactly one of kernels"):
        _vb(kernels=None, kernel_path=None, psf_grid=(2, 2))
    with pytest.raises(ValueError, match="varying_blur needs exactly one of kernels"):
        _vb(kernels=fam, kernel_path=str(tmp_path / "psfs.npy"))
    with pytest.raises(ValueError, match=r"varying_blur: .*bad.npy must hold a \[K, kh, kw\] array"):
        _vb(kernel_path=str(tmp_path / "bad.npy"))
    with pytest.raises(ValueError, match="varying_blur: every PSF must be a non-empty 2-D array"):
        _vb(kernels=[PSF7, np.zeros(7)], psf_grid=(1, 2))
    with pytest.raises(ValueError, match="varying_blur: 17 PSFs; the number of PSFs K is 1 .. 16"):
        _vb(kernels=[PSF7] * 17, psf_grid=(17, 1))
    with pytest.raises(ValueError, match="varying_blur: every PSF must be a non-empty 2-D array"):
        _vb(kernels=[], psf_grid=(1, 1))
    for kw in (dict(blend=None, blend_path=None, psf_grid=None), dict(blend=maps, psf_grid=(2, 2)),
               dict(blend=maps, blend_path=str(tmp_path / "maps.npy")), dict(blend_path=str(tmp_path / "maps.npy"), psf_grid="2x2"),
               dict(blend=maps, blend_path=str(tmp_path / "maps.npy"), psf_grid="2x2")):
        with pytest.raises(ValueError, match="varying_blur needs exactly one of blend"):
            _vb(kernels=fam, **kw)
    for grid in ("2", "2x", "axb", "2x2x2", (2,), (2.5, 2), "0x4", (-2, -2)):
        with pytest.raises(ValueError, match="varying_blur: psf_grid is"):
            _vb(psf_grid=grid)
    with pytest.raises(ValueError, match="varying_blur: psf_grid 3 x 2 holds 6 nodes for 4 PSFs"):
        _vb(psf_grid=(3, 2))
    for shape in ((3, 64, 64), (4, 32, 32), (4, 2, 64, 64), (64, 64), (1, 4, 3, 64, 64)):
        with pytest.raises(ValueError, match="varying_blur: the blend maps must have shape"):
            _vb(blend=np.ones(shape))
    for bad in (np.nan, np.inf, -np.inf):
        m = maps.copy()
        m[2, 1, 5, 7] = bad
        with pytest.raises(ValueError, match="varying_blur: the blend maps have a non-finite entry"):
            _vb(blend=m)
    m = maps.copy()
    m[3] = 0.0
    with pytest.raises(ValueError, match="varying_blur: the blend map of PSF 3 is all zero"):
        _vb(blend=m)
    # per PSF, custom_blur's rules with the index in the message
    k = PSF7.copy()
    k[0, 0] = np.nan
    with pytest.raises(ValueError, match="varying_blur: PSF 1 has a non-finite entry"):
        _vb(kernels=[PSF7, k, PSF7, PSF7])
    with pytest.raises(ValueError, match="varying_blur: PSF 1 has a non-finite entry"):  # overflows float32
        _vb(kernels=[PSF7, PSF7 * 1e40, PSF7, PSF7])
    with pytest.raises(ValueError, match="varying_blur: PSF 2 is all zero"):
        _vb(kernels=[PSF7, PSF7, np.zeros((7, 7)), PSF7])
    far = np.zeros((67, 67))
    far[0, 33] = 1.0
    with pytest.raises(ValueError, match=r"varying_blur: PSF 3 reaches \(33, 0\)"):
        _vb(S=96, kernels=[PSF7, PSF7, PSF7, far])
    with pytest.raises(ValueError, match="varying_blur: PSF 0 has 1089 non-zeros, a tap list holds 1024"):
        _vb(S=96, kernels=[np.ones((33, 33)), PSF7, PSF7, PSF7])


# ---------------------------------------------------------------- grid_blend_weights
def test_grid_blend_weights():
    from free_hunch_amd.measurements import grid_blend_weights
    for S, rows, cols in ((64, 2, 2), (60, 3, 3), (100, 4, 4), (80, 1, 3), (96, 16, 1), (256, 3, 3), (8, 1, 1), (10, 2, 5)):
        w = grid_blend_weights(S, rows, cols)
        assert w.dtype == np.float64 and w.shape == (rows * cols, S, S) and w.flags["C_CONTIGUOUS"]
        assert np.abs(w.sum(0) - 1.0).max() <= 1e-15 and w.min() >= 0.0 and w.max() <= 1.0
        g = w.reshape(rows, cols, S, S)
        # the mirror image of the grid: node (i, j) seen from the other corner
        assert np.abs(g - g[::-1, ::-1, ::-1, ::-1]).max() <= 1e-15
        # a tensor product: every map is the outer product of its own marginals along the two axes
        hy, hx = grid_blend_weights(S, rows, 1)[:, :, 0], grid_blend_weights(S, 1, cols)[:, 0, :]
        assert np.array_equal(g, hy[:, None, :, None] * hx[None, :, None, :])
    assert np.array_equal(grid_blend_weights(8, 1, 1), np.ones((1, 8, 8)))
    assert np.array_equal(grid_blend_weights(8, 1, 2)[:, 3], grid_blend_weights(8, 1, 2)[:, 0])  # one node along y: constant in y
    # 2 nodes over 64 pixels: nodes at 16 and 48 (pixel j sits at j + 0.5); constant beyond them, no wrap-around, linear between
    h = grid_blend_weights(64, 2, 1)[0, :, 0]
    assert np.array_equal(h[:16], np.ones(16)) and np.array_equal(h[48:], np.zeros(16))
    assert np.allclose(h[16:48], 1.0 - (np.arange(16, 48) + 0.5 - 16) / 32, rtol=0, atol=1e-15)
    # at a node the map is 1: S = 6, 3 nodes at 1, 3, 5 -> pixels 0 / 1 see weights (1, 0, 0) and (0.75, 0.25, 0)
    t = grid_blend_weights(6, 3, 1)[:, :, 0]
    assert np.allclose(t[:, 0], [1, 0, 0]) and np.allclose(t[:, 1], [0.75, 0.25, 0]) and np.allclose(t[:, 5], [0, 0, 1])
    with pytest.raises(ValueError, match="grid_blend_weights"):
        grid_blend_weights(64, 0, 2)


# ---------------------------------------------------------------- the launch plan of fh_conv_blend
def _plan(S, K, taps, hy, hx, planes, adjoint, halo=None):
    from free_hunch_amd import _lib
    out = (C.c_int32 * 6)(*([7] * 6))
    rc = _lib.load().fh_conv_blend_plan(S, K, taps, 1000 + 64 * hy + hx if halo is None else halo, planes, adjoint, out)
    return rc, list(out)


def _lds(nr, hy, hx, taps):
    """conv_blend_lds of csrc/fh_kernels.hip, restated"""
    return (((32 + 2 * hx) * (8 * nr + 2 * hy) + 1) & ~1) * 8 + taps * 16


def test_plan_rule_over_every_legal_argument():
    """always fused (the 32 x 16 tile at extents 32 with 1024 taps is 76 KiB, inside the opt-in): the 32 x 64 tile where its LDS
    fits 64 KiB, else the 32 x 16 tile; edge guards, so the grid is the ceiling of the side over the tile.  Neither the PSF
    count nor the direction changes the launch."""
    assert _lds(2, 32, 32, 1024) == 96 * 80 * 8 + 1024 * 16 == 76 * 1024 <= LDS_OPT_IN
    seen = {2: 0, 8: 0}
    for S in (60, 64, 80, 96, 100, 256):
        for hy, hx, taps in itertools.product((0, 1, 6, 17, 32), (0, 3, 16, 32), (1, 49, 300, 1024)):
            answers = {(K, a): _plan(S, K, taps, hy, hx, 3, a) for K in (1, 4, 16) for a in (0, 1)}
            assert len({(rc, tuple(out)) for rc, out in answers.values()}) == 1, (S, hy, hx, taps)
            rc, out = answers[(1, 0)]
            nr = 8 if _lds(8, hy, hx, taps) <= LDS_DEFAULT else 2
            seen[nr] += 1
            assert rc == 0 and out == [1, -(-S // 32), -(-S // (8 * nr)), 3, 256, _lds(nr, hy, hx, taps)], (S, hy, hx, taps, out)
            assert out[5] <= (LDS_DEFAULT if nr == 8 else LDS_OPT_IN)
            rc9, out9 = _plan(S, 9, taps, hy, hx, 9, 1)  # more planes: grid z only
            assert rc9 == 0 and out9 == out[:3] + [9] + out[4:]
    assert seen[2] > 50 and seen[8] > 50
    # the shapes the device tests rely on: the family's reach at K = 4 and at K = 16, and the wide PSF's 32
    for S in (64, 96, 80, 100, 60, 256):
        assert _plan(S, 4, 64, 4, 5, 3, 0)[1][:3] == [1, -(-S // 32), -(-S // 64)]
        assert _plan(S, 16, 64, 8, 8, 9, 1)[1][:4] == [1, -(-S // 32), -(-S // 64), 9]
        assert _plan(S, 4, 65, 32, 32, 3, 0)[1] == [1, -(-S // 32), -(-S // 16), 3, 256, 96 * 80 * 8 + 65 * 16]


def test_plan_refuses_illegal_arguments():
    from free_hunch_amd import _lib
    good = dict(S=64, K=4, taps=49, hy=4, hx=4, planes=3, adjoint=0)
    assert _plan(**good)[0] == 0
    bad = [dict(S=0), dict(S=63), dict(S=258), dict(K=0), dict(K=-1), dict(K=17), dict(taps=0), dict(taps=1025), dict(hy=33),
           dict(hx=33), dict(planes=0), dict(planes=4), dict(planes=-3), dict(adjoint=2), dict(adjoint=-1), dict(halo=6),
           dict(halo=-7), dict(halo=-105), dict(halo=999)]
    for change in bad:
        rc, out = _plan(**{**good, **change})
        assert rc == _lib.FH_EINVAL and out == [0] * 6, change
    assert _lib.load().fh_conv_blend_plan(64, 4, 49, 1260, 3, 0, None) == _lib.FH_EINVAL
    assert _plan(**{**good, "planes": 65538}) == (_lib.FH_ESIZE, [0] * 6)  # the plane is grid dimension z


# ---------------------------------------------------------------- solver tables, the problem, the CLI
def test_op_code_and_name_lists():
    from free_hunch_amd import conditioning_mechanisms as cm
    name = "varying_blur"
    row = cm._OPS[name]
    assert cm._op_code(name) == row.op == 14
    # not decimating, no noise map, not the frames' layout, no single shared PSF, no 0/1-mask operator
    assert not row.decimating and row.unit_sigma != "always" and row.layout == "blend" and "share the PSF" not in row.shares
    older = {"inpainting": 0, "gaussian_blur": 1, "motion_blur": 1, "custom_blur": 1, "super_resolution": 2, "colorization": 3,
             "noise": 0, "masked_blur": 5, "custom_sr": 2, "weighted_blur": 8, "weighted_sr": 10, "burst_sr": 12,
             "weighted_burst_sr": 13}
    assert {k: cm._op_code(k) for k in older} == older and set(cm._OPS) == set(older) | {name, "fourier_sampling"}
    assert cm._BAD_OPERATOR.rstrip(".").endswith("'varying_blur'") and all(f"'{k}'" in cm._BAD_OPERATOR for k in older)
    op = _vb()
    assert cm._solver_sigma_y2(op) == cm._sigma_y2(op) == pytest.approx(0.05 ** 2)  # the blur rule: no 1e-2 clip ...
    tiny = _vb()
    tiny.sigma_s = torch.Tensor([0.0001])
    assert cm._sigma_y2(tiny) == pytest.approx(0.001 ** 2)  # ... the 0.001 one
    with pytest.raises(ValueError, match="Invalid operator name"):
        cm.choose_solver("varying", None, None, None)


def test_problem_fields_for_op_14():
    from free_hunch_amd import conditioning_mechanisms as cm

    class Cov:  # what _problem reads of a covariance
        use_dct, data_dim, device = True, 3 * 64 * 64, torch.device("cpu")

        class famC:
            m, B = 0, torch.zeros(1, dtype=torch.float64)

        class C:
            D = r = torch.zeros(1, dtype=torch.float64)
            M_dev = torch.zeros(1, 8, dtype=torch.float64)
    op = _vb(blend=random_maps(4, 64))
    p, keep = cm._problem(op, Cov, cm._solver_sigma_y2(op))
    ft = op.frame_taps
    assert (p.op, p.stride, p.ntaps, p.ntaps2, p.halo2, p.halo, p.use_dct, p.fold_sym) == (14, 1, 168, 4, 64, ft.halo, 1, 0)
    assert p.tap_dy == ft.dy.data_ptr() and p.tap_dx == ft.dx.data_ptr() and p.tap_w == ft.w.data_ptr()
    assert p.tap2_dy == ft.off.data_ptr() and not p.tap2_dx and not p.mask
    assert p.tap2_w == keep[-1].data_ptr() and torch.equal(keep[-1], op.blend) and tuple(keep[-1].shape) == (4, 3, 64, 64)
    assert keep[-1].dtype == torch.float64 and keep[-1].is_contiguous()
    assert not (p.fold_fwd_w or p.fold_fwd_h or p.fold_inv_w or p.fold_inv_h)
    assert all(any(t is k for k in keep) for t in (ft.dy, ft.dx, ft.w, ft.off))  # kept alive with the problem
    assert p.sigma_y2 == pytest.approx(0.05 ** 2) and p.planes == 3 and p.d == 3 * 64 * 64
    Cov.use_dct = False
    assert cm._problem(op, Cov, 1.0)[0].use_dct == 0


def test_config_flags(tmp_path):
    from free_hunch_amd.config import SCHEMA, load_config
    assert SCHEMA["blend_path"] == (str, "") and SCHEMA["psf_grid"] == (str, "")
    base = [f"--outdir={tmp_path}", "--operator_name=varying_blur"]
    psf, maps, grid = f"--kernel_path={tmp_path}/psfs.npy", f"--blend_path={tmp_path}/maps.npy", "--psf_grid=2x2"
    o = load_config(base + [psf, grid])
    assert o.operator_name == "varying_blur" and o.psf_grid == "2x2" and o.blend_path == "" and o.kernel_path == f"{tmp_path}/psfs.npy"
    o = load_config(base + [psf, maps])
    assert o.blend_path == f"{tmp_path}/maps.npy" and o.psf_grid == ""
    assert load_config([f"--outdir={tmp_path}"]).blend_path == "" and load_config([f"--outdir={tmp_path}"]).psf_grid == ""
    with pytest.raises(SystemExit, match="varying_blur needs --kernel_path"):
        load_config(base + [grid])
    for none_or_both in ([], [maps, grid]):
        with pytest.raises(SystemExit, match="varying_blur needs its blend maps: exactly one of --blend_path=FILE.npy and --psf_grid=RxC"):
            load_config(base + [psf] + none_or_both)
    for other in ("custom_blur", "burst_sr", "weighted_blur", "gaussian_blur", "super_resolution"):
        args = [f"--outdir={tmp_path}", f"--operator_name={other}"]
        if other in ("custom_blur", "burst_sr", "weighted_blur"):
            args.append(psf)
        if other == "weighted_blur":
            args.append(f"--noise_map_path={tmp_path}/map.npy")
        for flag in (maps, grid):
            with pytest.raises(SystemExit, match="--blend_path and --psf_grid belong to --operator_name=varying_blur"):
                load_config(args + [flag])
    # the flags of the other operators stay refused on varying_blur, and --kernel_path names it last among its readers
    with pytest.raises(SystemExit, match="--frame_shifts belongs to --operator_name=burst_sr"):
        load_config(base + [psf, grid, "--frame_shifts=0,0;1,1"])
    with pytest.raises(SystemExit, match="masked_blur"):
        load_config(base + [psf, grid, "--mask_border=2"])
    with pytest.raises(SystemExit, match="weighted_blur / weighted_sr"):
        load_config(base + [psf, grid, f"--noise_map_path={tmp_path}/map.npy"])
    with pytest.raises(SystemExit, match="--frame_sigmas and --mosaic belong to"):
        load_config(base + [psf, grid, "--mosaic=rggb"])
    with pytest.raises(SystemExit, match="custom_sr.*burst_sr.*weighted_burst_sr / varying_blur; operator 'gaussian_blur'"):
        load_config([f"--outdir={tmp_path}", "--operator_name=gaussian_blur", psf])


def test_exported_symbols_and_header():
    import os
    from free_hunch_amd import _lib
    assert {"fh_conv_blend", "fh_conv_blend_plan"} <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.fh_conv_blend.restype is C.c_int and len(lib.fh_conv_blend.argtypes) == 14
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fh_hip.h")).read()
    assert "int fh_conv_blend(" in header and "int fh_conv_blend_plan(" in header and "14 spatially varying blur" in header
