"""Host-side checks of user-supplied PSFs: how `measurements.Taps` classifies a PSF (rank-1 passes, tap list, dense window),
the validation of `custom_blur`, the launch plan of fh_conv_window and the CLI flag.  No GPU: the operators are built on
device="cpu" and the plan queries need neither a context nor a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

# the largest dynamic LDS k_conv_window may ask for: its opt-in is sized for the 65 x 65 window, 96 x 129 tile doubles +
# 65 x 80 weights, and a CU has 160 KiB
LDS_LIMIT = (96 * 129 + 65 * 80) * 8


def disk_psf(radius=20.3, size=61):
    """Defocus disk, normalised: 1305 non-zeros at radius 20.3 on 61 x 61."""
    yy, xx = np.mgrid[-(size // 2): size - size // 2, -(size // 2): size - size // 2]
    k = (yy ** 2 + xx ** 2 <= radius ** 2).astype(np.float64)
    return k / k.sum()


def _custom(**kw):
    from free_hunch_amd.measurements import get_operator
    return get_operator(name="custom_blur", device="cpu", sigma_s=0.05, in_shape=(1, 3, 64, 64), **kw)


def test_shipped_psfs_keep_their_routes():
    from free_hunch_amd.measurements import KERNEL_DIR, Taps
    g = Taps(np.load(os.path.join(KERNEL_DIR, "gaussian_ks61_std3.0.npy")), "cpu")
    assert g.sep is not None and g.window is None
    m = Taps(np.load(os.path.join(KERNEL_DIR, "motion_ks61_std0.5.npy")), "cpu")
    assert m.sep is None and m.window is None and 1 < m.n <= Taps.MAX_TAPS


def test_disk_gets_a_window_with_its_own_extent():
    from free_hunch_amd.measurements import Taps
    k = disk_psf()
    t = Taps(k, "cpu")
    assert t.n == 1305 and t.sep is None and t.window is not None
    win, hy, hx = t.window
    assert (hy, hx) == (20, 20) and tuple(win.shape) == (41, 41) and win.dtype == torch.float64
    k32 = k.astype(np.float32).astype(np.float64)  # rounded to float32 like the shipped PSFs
    assert np.array_equal(win.numpy(), k32[10:51, 10:51]) and float(win.sum()) == float(k32.sum())


def test_even_sized_dense_psf_is_padded_about_its_centre():
    """60 x 34, centre at (30, 17): rows reach 30 up and 29 down, columns 17 left and 16 right -> a 61 x 35 window whose last
    row and last column are zero."""
    from free_hunch_amd.measurements import Taps
    k = np.random.default_rng(5).uniform(0.1, 1.0, (60, 34))
    t = Taps(k, "cpu")
    assert t.n == 2040 and t.sep is None
    win, hy, hx = t.window
    assert (hy, hx) == (30, 17) and tuple(win.shape) == (61, 35)
    assert np.array_equal(win.numpy()[:60, :34], k.astype(np.float32).astype(np.float64))
    assert not win[60].any() and not win[:, 34].any()


def test_a_psf_that_fills_half_its_window_gets_one():
    """The routing rule below 1024 taps: the window kernel multiplies (2hy+1) x (2hx+1 rounded up to 16) entries per output
    and measured 2.25x faster per multiply-add than the tap-list kernel, so a list with at least half that many taps goes
    to it and a sparser one stays."""
    from free_hunch_amd.measurements import Taps
    rng = np.random.default_rng(7)
    full = rng.uniform(0.1, 1.0, (31, 31))  # 961 taps of 31 x 32
    sparse = full * (rng.random((31, 31)) < 0.3)
    sparse[0, 0] = sparse[30, 30] = 1.0
    t_full, t_sparse = Taps(full, "cpu"), Taps(sparse, "cpu")
    assert t_full.n == 961 and t_full.window is not None and t_full.window[1:] == (15, 15)
    assert 2 * t_sparse.n < 31 * 32 and t_sparse.window is None
    # 1-D lists stay on the 1-D kernels, and the decimating operator's 25 x 25 PSF keeps its tap-list kernels at its stride
    assert Taps(np.ones((1, 9)), "cpu").window is None and Taps(np.ones((9, 1)), "cpu").window is None


def test_super_resolution_keeps_the_tap_list_problem():
    from free_hunch_amd.conditioning_mechanisms import _OPS, _op_code
    from free_hunch_amd.measurements import get_operator
    sr = get_operator(name="super_resolution", device="cpu", sigma_s=0.05, in_shape=(1, 3, 64, 64), scale_factor=4)
    assert _op_code(sr.name) == 2 and sr.taps.n == 625  # dense, but op = 4 is emitted for blur operators only (_problem)
    assert _OPS[sr.name].window is None and _OPS["custom_blur"].window == 4


def test_sparse_psf_beyond_the_tile_kernels_lds_gets_a_window():
    """602 taps spread over 65 x 65 are within the tap-list limit, but their halo leaves no room for them in the tile
    kernels' LDS (fh_conv_circ_plan: FH_ESIZE): such a list is sent to the window kernel instead of failing at the first call."""
    from free_hunch_amd import _lib
    from free_hunch_amd.measurements import Taps
    rng = np.random.default_rng(6)
    k = np.zeros((65, 65))
    k.flat[rng.choice(65 * 65, 600, replace=False)] = 1.0
    k[0, 0] = k[64, 64] = 1.0
    t = Taps(k, "cpu")
    out = (C.c_int32 * 6)()
    assert t.n <= Taps.MAX_TAPS and _lib.load().fh_conv_circ_plan(256, t.n, t.halo, 3, 1, 0, out) == _lib.FH_ESIZE
    assert t.window is not None and t.window[1:] == (32, 32)


def test_custom_blur_operator_on_cpu(tmp_path):
    from free_hunch_amd.measurements import CustomBlurOperator, _BlurOperator
    k = disk_psf()
    np.save(tmp_path / "psf.npy", k)
    for op in (_custom(kernel=k), _custom(kernel_path=str(tmp_path / "psf.npy"))):
        assert isinstance(op, CustomBlurOperator) and isinstance(op, _BlurOperator) and op.name == "custom_blur"
        assert op.taps.window is not None and tuple(op.in_shape) == (1, 3, 64, 64)
        assert tuple(op.get_kernel().shape) == (1, 1, 61, 61) and op.get_kernel().dtype == torch.float32
        assert float(op.sigma_s) == pytest.approx(0.05)
    # used as given: not normalised
    assert float(_custom(kernel=3.0 * k).taps.window[0].sum()) == pytest.approx(3.0, rel=1e-6)


@pytest.mark.parametrize("bad", [np.ones(7), np.ones((2, 3, 3)), np.zeros((5, 5)), np.array([[1.0, np.nan], [0.5, 0.5]]),
                                 np.array([[1.0, np.inf], [0.5, 0.5]]), np.ones((67, 3)), np.ones((3, 66))])
def test_bad_psfs_are_rejected(bad):
    with pytest.raises(ValueError):
        _custom(kernel=bad)


def test_kernel_and_kernel_path_exclude_each_other(tmp_path):
    np.save(tmp_path / "psf.npy", disk_psf())
    with pytest.raises(ValueError):
        _custom()
    with pytest.raises(ValueError):
        _custom(kernel=disk_psf(), kernel_path=str(tmp_path / "psf.npy"))


def test_solver_names_the_operator():
    from free_hunch_amd.conditioning_mechanisms import _BAD_OPERATOR, _op_code, _sigma_y2
    assert _op_code("custom_blur") == 1 and "custom_blur" in _BAD_OPERATOR
    assert _sigma_y2(_custom(kernel=disk_psf())) == float(torch.tensor([0.05]).float().clip(min=0.001) ** 2)


def test_window_plan_for_every_extent():
    from free_hunch_amd import _lib
    plan = _lib.load().fh_conv_window_plan
    out = (C.c_int32 * 5)()
    worst = 0
    for S in (48, 64, 96, 256):
        for hy in range(33):
            for hx in range(33):
                assert plan(S, hy, hx, 6, out) == 0, (S, hy, hx)
                gx, gy, gz, block, lds = out
                assert block == 256 and gz == 6 and 0 < lds <= LDS_LIMIT, (S, hy, hx, list(out))
                assert gx * 32 >= S > (gx - 1) * 32 and gy * 64 >= S > (gy - 1) * 64  # 64 x 32 output tiles cover the image once
                worst = max(worst, lds)
    assert worst == LDS_LIMIT  # the limit is what the 65 x 65 window needs, not a round number above it


@pytest.mark.parametrize("S,hy,hx,planes", [(64, 33, 0, 3), (64, 0, 33, 3), (64, -1, 0, 3), (64, 0, -1, 3), (64, 3, 3, 0),
                                            (63, 3, 3, 3), (258, 3, 3, 3), (0, 3, 3, 3)])
def test_window_plan_rejects_bad_arguments(S, hy, hx, planes):
    from free_hunch_amd import _lib
    lib = _lib.load()
    out = (C.c_int32 * 5)(*([7] * 5))
    assert lib.fh_conv_window_plan(S, hy, hx, planes, out) == _lib.FH_EINVAL
    assert list(out) == [0] * 5
    assert lib.fh_conv_window_plan(64, 3, 3, 3, None) == _lib.FH_EINVAL


def test_tap_list_plan_still_refuses_more_than_1024_taps():
    from free_hunch_amd import _lib
    out = (C.c_int32 * 6)()
    assert _lib.load().fh_conv_circ_plan(256, 1025, 1000 + 64 * 20 + 20, 3, 1, 0, out) == _lib.FH_EINVAL


def test_config_key_and_cli_messages(tmp_path):
    from free_hunch_amd.config import SCHEMA, load_config
    assert SCHEMA["kernel_path"] == (str, "")
    assert load_config([f"--outdir={tmp_path}"]).kernel_path == ""
    o = load_config([f"--outdir={tmp_path}", "--operator_name=custom_blur", f"--kernel_path={tmp_path}/psf.npy"])
    assert o.operator_name == "custom_blur" and o.kernel_path == f"{tmp_path}/psf.npy"
    with pytest.raises(SystemExit, match="kernel_path"):
        load_config([f"--outdir={tmp_path}", "--operator_name=custom_blur"])
    with pytest.raises(SystemExit, match="custom_blur"):
        load_config([f"--outdir={tmp_path}", "--operator_name=motion_blur", f"--kernel_path={tmp_path}/psf.npy"])
