"""Host-side checks of `custom_sr` (super-resolution with the caller's PSF and factor): registry and attributes, every refusal,
the folded rectangular bases against direct circular sums, the launch plan of fh_dct_rect and the CLI flags.  No GPU: the
operators are built on device="cpu" and the plan queries need neither a context nor a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_custom_psf_host import disk_psf

LDS_OPT_IN = 140 * 1024  # the dynamic-LDS opt-in k_dct_rect shares with k_dct_sym


def binomial(n):
    """[1, 1] / 2 convolved n times: n + 1 weights, exact in float32 (and so are their outer products) up to n = 23"""
    v = np.array([1.0])
    for _ in range(n):
        v = np.convolve(v, [0.5, 0.5])
    return v


def binomial_psf(rows, cols):
    return np.outer(binomial(rows - 1), binomial(cols - 1))


def box_psf(s):
    return np.full((s, s), 1.0 / s ** 2)


def _sr(S=64, **kw):
    from free_hunch_amd.measurements import get_operator
    kw.setdefault("scale_factor", 4)
    if "kernel" not in kw and "kernel_path" not in kw:
        kw["kernel"] = box_psf(4)
    return get_operator(name="custom_sr", device="cpu", sigma_s=0.05, in_shape=(1, 3, S, S), **kw)


def test_registry_and_attributes(tmp_path):
    from free_hunch_amd.measurements import CustomBlurOperator, CustomSROperator, Taps
    k = binomial_psf(7, 5)
    np.save(tmp_path / "psf.npy", k)
    for op in (_sr(kernel=k, scale_factor=2), _sr(kernel_path=str(tmp_path / "psf.npy"), scale_factor=2)):
        assert isinstance(op, CustomSROperator) and isinstance(op, CustomBlurOperator) and op.name == "custom_sr"
        assert op.scale_factor == 2 and op.out_shape == (1, 3, 32, 32) and tuple(op.in_shape) == (1, 3, 64, 64)
        assert isinstance(op.taps, Taps) and op.taps.n == 35 and op.taps.sep is not None
        assert tuple(op.get_kernel().shape) == (1, 1, 7, 5) and op.get_kernel().dtype == torch.float32
        assert np.array_equal(op.get_kernel()[0, 0].numpy().astype(np.float64), k)  # used as given, exact in float32
        assert op.folded_bases() is None  # the stride-1 fold is not this operator's
    assert _sr(scale_factor=4.0).scale_factor == 4 and _sr(scale_factor=np.int64(8)).scale_factor == 8
    assert _sr(S=256, scale_factor=16, kernel=box_psf(16)).out_shape == (1, 3, 16, 16)
    disk = _sr(kernel=disk_psf(radius=4.0, size=9))
    assert disk.taps.sep is None and disk.taps.n == 49 and disk.folded_sr_bases() is None


@pytest.mark.parametrize("bad", [None, 0, -2, 17, 2.5, "4", True])
def test_scale_factor_must_be_an_integer_from_2_to_16(bad):
    with pytest.raises(ValueError, match="custom_sr"):
        _sr(scale_factor=bad)


def test_scale_factor_one_points_to_custom_blur():
    with pytest.raises(ValueError, match="custom_sr.*custom_blur"):
        _sr(scale_factor=1)


def test_sizes_are_checked():
    with pytest.raises(ValueError, match="custom_sr.*divide"):
        _sr(S=64, scale_factor=3)
    with pytest.raises(ValueError, match="custom_sr.*8 x 8"):
        _sr(S=64, scale_factor=16)
    assert _sr(S=64, scale_factor=8).out_shape == (1, 3, 8, 8)


def test_psf_checks_are_custom_blurs(tmp_path):
    for bad in (np.ones(7), np.zeros((5, 5)), np.array([[1.0, np.nan], [0.5, 0.5]]), np.ones((67, 3))):
        with pytest.raises(ValueError):
            _sr(kernel=bad)
    np.save(tmp_path / "psf.npy", box_psf(4))
    with pytest.raises(ValueError):
        _sr(kernel=box_psf(4), kernel_path=str(tmp_path / "psf.npy"))
    with pytest.raises(ValueError):
        from free_hunch_amd.measurements import get_operator
        get_operator(name="custom_sr", device="cpu", sigma_s=0.05, in_shape=(1, 3, 64, 64), scale_factor=4)


def test_more_taps_than_a_list_holds_are_refused():
    """a rank-1 PSF too: the tap list is the route of everything outside the folded solve"""
    with pytest.raises(ValueError, match="custom_sr.*out of scope"):
        _sr(kernel=disk_psf())  # 1305 non-zeros
    with pytest.raises(ValueError, match="custom_sr.*out of scope"):
        _sr(kernel=np.full((33, 33), 1.0 / 33 ** 2))  # 1089 non-zeros, rank 1


def test_a_list_the_decimating_kernels_cannot_stage_is_refused():
    """What fh_conv_circ_plan refuses at this stride, the constructor refuses with the operator's name: about 900 taps spread
    over 65 x 65 at stride 8.  The adjoint of a stride above 4 runs on k_conv_tile, whose 80 x 96 staged tile and tap table
    (72 KB) exceed its 64 KB of LDS (FH_ESIZE); the forward runs on the direct kernel."""
    from free_hunch_amd import _lib
    from free_hunch_amd.measurements import Taps
    rng = np.random.default_rng(6)
    k = np.zeros((65, 65))
    k.flat[rng.choice(65 * 65, 900, replace=False)] = 1.0
    k[0, 0] = k[64, 64] = 1.0
    t = Taps(k, "cpu")
    out = (C.c_int32 * 6)()
    plan = _lib.load().fh_conv_circ_plan
    assert 900 <= t.n <= Taps.MAX_TAPS and plan(256, t.n, t.halo, 3, 8, 0, out) == 0
    assert plan(256, t.n, t.halo, 3, 8, 1, out) == _lib.FH_ESIZE
    with pytest.raises(ValueError, match="custom_sr.*tap list"):
        _sr(S=256, kernel=k, scale_factor=8)
    assert _sr(S=256, kernel=k[24:41, 24:41], scale_factor=8).out_shape == (1, 3, 32, 32)  # the 17 x 17 middle of it runs


def _direct(k, S, s, u, v):
    """dct2(A^T u) and A(idct2(v)) from the circular sums that define A (centre at size // 2), numpy float64"""
    from free_hunch_amd.measurements import dct_basis_longdouble
    Cm = dct_basis_longdouble(S).astype(np.float64)
    dy, dx = np.arange(k.shape[0]) - k.shape[0] // 2, np.arange(k.shape[1]) - k.shape[1] // 2
    up = np.zeros((S, S))
    up[::s, ::s] = u
    at, bl, img = np.zeros((S, S)), np.zeros((S, S)), Cm.T @ v @ Cm
    for a, ya in enumerate(dy):
        for b, xb in enumerate(dx):
            at += k[a, b] * np.roll(np.roll(up, -ya, 0), -xb, 1)   # A^T: out[i][j] = sum w up[(i + dy) % S][(j + dx) % S]
            bl += k[a, b] * np.roll(np.roll(img, ya, 0), xb, 1)    # B:   out[i][j] = sum w x[(i - dy) % S][(j - dx) % S]
    return Cm @ at @ Cm.T, bl[::s, ::s]


@pytest.mark.parametrize("S,s,psf", [(64, 2, binomial_psf(7, 5)), (64, 4, box_psf(4)), (64, 8, binomial_psf(13, 13)),
                                     (96, 8, binomial_psf(13, 13))])
def test_folded_sr_bases_reproduce_the_direct_sums(S, s, psf):
    from free_hunch_amd.measurements import Taps, folded_dct_blur_bases, folded_dct_sr_bases
    k = psf.astype(np.float32).astype(np.float64)
    assert np.array_equal(k, psf)  # exact in float32
    col, row = Taps(k, "cpu").sep
    args = (col.dy.numpy(), col.w.numpy(), row.dx.numpy(), row.w.numpy(), S)
    G_row, G_col, G_row_t, G_col_t = folded_dct_sr_bases(*args, s)
    P_row, P_col, _, _ = folded_dct_blur_bases(*args)
    So = S // s
    assert G_row.shape == G_col.shape == (S, So) and G_row_t.shape == G_col_t.shape == (So, S)
    assert all(m.dtype == np.float64 and m.flags.c_contiguous for m in (G_row, G_col, G_row_t, G_col_t))
    assert np.array_equal(G_row, P_row[:, ::s]) and np.array_equal(G_col, P_col[:, ::s])
    assert np.array_equal(G_row_t, G_row.T) and np.array_equal(G_col_t, G_col.T)
    rng = np.random.default_rng(S + s)
    u, v = rng.standard_normal((So, So)), rng.standard_normal((S, S))
    ref_f, ref_i = _direct(k, S, s, u, v)
    e_f = np.abs(G_col @ u @ G_row.T - ref_f).max() / np.abs(ref_f).max()
    e_i = np.abs(G_col.T @ v @ G_row - ref_i).max() / np.abs(ref_i).max()
    print(f"folded SR bases S={S} s={s}: forward {e_f:.2e} inverse {e_i:.2e}")
    assert e_f < 1e-12 and e_i < 1e-12


def test_folded_sr_bases_of_the_operator(monkeypatch):
    op = _sr(kernel=binomial_psf(7, 5), scale_factor=2)
    mats = op.folded_sr_bases()
    assert [tuple(m.shape) for m in mats] == [(64, 32), (64, 32), (32, 64), (32, 64)]
    assert all(m.dtype == torch.float64 and m.is_contiguous() for m in mats)
    assert op.folded_sr_bases() is mats  # cached
    assert _sr(kernel=binomial_psf(7, 5), scale_factor=4).folded_sr_bases()[0].shape == (64, 16)  # the factor is in the key
    monkeypatch.setenv("FH_NO_FOLD", "1")
    assert op.folded_sr_bases() is None


def test_rect_plan_for_every_legal_size():
    from free_hunch_amd import _lib
    plan = _lib.load().fh_dct_rect_plan
    out = (C.c_int32 * 10)()
    worst = 0
    for S in range(16, 257, 2):
        for s in range(2, 17):
            So = S // s
            if S % s or So < 8:
                continue
            for planes in (3, 24, 48):
                for inverse in (0, 1):
                    assert plan(S, So, planes, inverse, out) == 0, (S, So, planes, inverse)
                    for gx, gy, gz, block, lds in (tuple(out[:5]), tuple(out[5:])):
                        assert block == 256 and 1 <= gz <= planes and gx >= 1 and gy >= 1
                        assert 0 < lds <= LDS_OPT_IN, (S, So, list(out))
                        worst = max(worst, lds)
                    ko, r_a, r_b = (So, S, So) if inverse else (S, So, S)
                    assert out[1] == out[6] == -(-ko // 32) and out[0] == -(-r_a // 32) and out[5] == -(-r_b // 32)
    assert worst == (32 * 258 + 2 * 32 * 34) * 8  # a 32-row slice of a 256-wide basis and two staging buffers


@pytest.mark.parametrize("S,So,planes", [(0, 8, 3), (63, 9, 3), (258, 129, 3), (64, 0, 3), (64, -4, 3), (64, 65, 3), (64, 16, 0),
                                         (64, 16, 65536)])
def test_rect_plan_rejects_bad_sizes(S, So, planes):
    from free_hunch_amd import _lib
    lib = _lib.load()
    out = (C.c_int32 * 10)(*([7] * 10))
    assert lib.fh_dct_rect_plan(S, So, planes, 0, out) == _lib.FH_EINVAL
    assert list(out) == [0] * 10
    assert lib.fh_dct_rect_plan(64, 16, 3, 0, None) == _lib.FH_EINVAL


def test_solver_names_the_operator():
    from free_hunch_amd.conditioning_mechanisms import _BAD_OPERATOR, _OPS, _op_code, _sigma_y2
    assert _op_code("custom_sr") == 2 == _op_code("super_resolution")
    assert "custom_sr" in _BAD_OPERATOR and "custom_blur" in _BAD_OPERATOR and "masked_blur" in _BAD_OPERATOR
    assert "share the PSF" in _OPS["custom_sr"].shares
    # the SR rule: sigma_s is clipped at 1e-2 before squaring
    from free_hunch_amd.measurements import get_operator
    small = get_operator(name="custom_sr", device="cpu", sigma_s=0.001, in_shape=(1, 3, 64, 64), scale_factor=4, kernel=box_psf(4))
    assert _sigma_y2(small) == float(torch.tensor([1e-2]).float() ** 2)
    assert _sigma_y2(_sr()) == float(torch.tensor([0.05]).float() ** 2)


def test_config_flags(tmp_path):
    from free_hunch_amd.config import load_config
    psf = f"--kernel_path={tmp_path}/psf.npy"
    o = load_config([f"--outdir={tmp_path}", "--operator_name=custom_sr", psf, "--scale_factor=8"])
    assert o.operator_name == "custom_sr" and o.kernel_path == f"{tmp_path}/psf.npy" and o.scale_factor == 8
    with pytest.raises(SystemExit, match="kernel_path"):
        load_config([f"--outdir={tmp_path}", "--operator_name=custom_sr", "--scale_factor=8"])
    with pytest.raises(SystemExit, match="masked_blur"):
        load_config([f"--outdir={tmp_path}", "--operator_name=custom_sr", psf, "--mask_border=2"])
    with pytest.raises(SystemExit, match="custom_sr"):  # --kernel_path stays refused elsewhere, and names who reads it
        load_config([f"--outdir={tmp_path}", "--operator_name=super_resolution", psf])
