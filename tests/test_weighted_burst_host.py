"""Host-side checks of `weighted_burst_sr` (burst_sr with a per-pixel noise map on every frame, fh_problem.op = 13): the
constructor's refusals, the accepted map shapes, `frame_sigmas`, `bayer_sites` and `mosaic`, the op-code tables, the problem
fields and the CLI flags.  No GPU: the operators are built on device="cpu"."""
import numpy as np
import pytest
import torch

from test_burst_sr_host import FRACTIONAL, PSF7, integer_shifts
from test_noise_map_host import noise_map_n, noise_map_n3

S, SO = 64, 16


def _wb(S=S, **kw):
    from free_hunch_amd.measurements import get_operator
    kw.setdefault("scale_factor", 4)
    if "kernels" not in kw and "kernel_path" not in kw:
        kw["kernels"] = [PSF7]
        kw.setdefault("frame_shifts", integer_shifts(2))  # K = 4
    return get_operator(name="weighted_burst_sr", device="cpu", sigma_s=0.05, in_shape=(1, 3, S, S), **kw)


def map_f3(n, K):
    """Map F3: frame k = noise_map_n3(n) * (1 + 0.5 k), [K, 3, n, n] - channels and frames both differ"""
    return np.stack([noise_map_n3(n) * (1 + 0.5 * k) for k in range(K)])


# ---------------------------------------------------------------- registry, shapes, floor
def test_registry_and_attributes(tmp_path):
    from free_hunch_amd.measurements import BurstSROperator, WeightedBurstSROperator, _NoiseMap
    f3 = map_f3(SO, 4)
    np.save(tmp_path / "map.npy", f3)
    for op in (_wb(noise_map=f3), _wb(noise_map_path=str(tmp_path / "map.npy")), _wb(noise_map=torch.from_numpy(f3))):
        assert isinstance(op, WeightedBurstSROperator) and isinstance(op, BurstSROperator) and isinstance(op, _NoiseMap)
        assert op.name == "weighted_burst_sr" and op.nframes == 4 and op.out_shape == (1, 12, SO, SO) and op.mosaic is None
        assert tuple(op.noise_map.shape) == tuple(op.weights.shape) == tuple(op.mask.shape) == (1, 12, SO, SO)
        assert op.noise_map.dtype == op.weights.dtype == op.mask.dtype == torch.float64
        assert np.array_equal(op.noise_map[0].numpy(), f3.reshape(12, SO, SO))  # every entry of F3 is above the floor
        assert float(op.sigma_s) == pytest.approx(0.05)  # accepted and stored
    fin = torch.from_numpy(np.isfinite(f3.reshape(1, 12, SO, SO)))
    assert torch.equal(op.mask > 0, fin) and torch.equal(op.weights > 0, fin) and bool((op.weights[~fin] == 0).all())
    assert torch.equal(op.weights[fin], 1.0 / op.noise_map[fin]) and bool(torch.isfinite(op.weights).all())
    assert abs(float((~fin).double().mean()) - 0.11) < 0.03  # about 11 % inf


def test_the_five_accepted_shapes():
    K = 4
    n2, n3, f3 = noise_map_n(SO), noise_map_n3(SO), map_f3(SO, K)
    same = np.broadcast_to(n2, (1, 3 * K, SO, SO))
    assert np.array_equal(_wb(noise_map=n2).noise_map.numpy(), same)  # [So,So]: every channel of every frame
    assert np.array_equal(_wb(noise_map=n3).noise_map.numpy(), np.tile(n3, (K, 1, 1))[None])  # [3,So,So]: every frame
    for a in (f3, f3.reshape(3 * K, SO, SO), f3.reshape(1, 3 * K, SO, SO)):
        assert np.array_equal(_wb(noise_map=a).noise_map.numpy(), f3.reshape(1, 3 * K, SO, SO))
    one = _wb(frame_shifts=[(0, 0)], noise_map=n3)  # K = 1: [3,So,So] is also [3K,So,So], the same map
    assert np.array_equal(one.noise_map.numpy(), n3[None])
    m = np.full((K, 3, SO, SO), 0.05)
    m[1, 2, 0, 0], m[1, 2, 0, 1], m[1, 2, 0, 2] = 1e-5, 0.005, np.inf
    op = _wb(noise_map=m)  # the decimating floor 0.01, and weights = 0 where inf
    assert op.noise_map[0, 5, 0, 0] == 0.01 and op.noise_map[0, 5, 0, 1] == 0.01 and op.weights[0, 5, 0, 1] == 100.0
    assert torch.isinf(op.noise_map[0, 5, 0, 2]) and op.weights[0, 5, 0, 2] == 0.0 and op.mask[0, 5, 0, 2] == 0.0
    assert op.noise_map[0, 5, 1, 1] == 0.05 and op.weights[0, 4, 0, 0] == 20.0


def test_frame_sigmas_give_constant_planes():
    op = _wb(frame_sigmas=(0.02, 0.05, 0.1, 0.3))
    for k, v in enumerate((0.02, 0.05, 0.1, 0.3)):
        assert bool((op.noise_map[0, 3 * k: 3 * k + 3] == v).all()) and bool((op.weights[0, 3 * k: 3 * k + 3] == 1.0 / v).all())
    assert torch.equal(_wb(frame_sigmas="0.02,0.05,0.1,0.3").noise_map, op.noise_map)  # the command line's string
    drop = _wb(frame_sigmas=[0.02, np.inf, 0.1, "inf"])  # inf drops a frame
    assert bool((drop.mask[0, 3:6] == 0).all()) and bool((drop.mask[0, 9:12] == 0).all()) and bool((drop.mask[0, 0:3] == 1).all())
    assert bool((_wb(frame_sigmas=[0.001] * 4).noise_map == 0.01).all())  # the floor


# ---------------------------------------------------------------- refusals
def test_noise_source_refusals(tmp_path):
    m = noise_map_n(SO)
    np.save(tmp_path / "map.npy", m)
    path = str(tmp_path / "map.npy")
    with pytest.raises(ValueError, match="weighted_burst_sr needs exactly one"):
        _wb()
    for two in (dict(noise_map=m, noise_map_path=path), dict(noise_map=m, frame_sigmas=[0.1] * 4),
                dict(noise_map_path=path, frame_sigmas=[0.1] * 4)):
        with pytest.raises(ValueError, match="weighted_burst_sr needs exactly one"):
            _wb(**two)
    for bad in (np.ones((SO, SO + 1)), np.ones((64, 64)), np.ones((2, SO, SO)), np.ones((4, SO, SO)), np.ones((3, 3, SO, SO)),
                np.ones((1, 3, SO, SO)), np.ones((4, 3, 8, 8)), np.ones(SO)):
        with pytest.raises(ValueError, match=r"weighted_burst_sr: the noise map must have shape \(16, 16\), \(3, 16, 16\), "
                                             r"\(4, 3, 16, 16\), \(12, 16, 16\) or \(1, 12, 16, 16\)"):
            _wb(noise_map=bad)
    for value, word in ((np.nan, "NaN"), (0.0, "<= 0"), (-0.1, "<= 0"), (-np.inf, "<= 0")):
        bad = m.copy()
        bad[3, 4] = value
        with pytest.raises(ValueError, match=f"weighted_burst_sr.*{word}"):
            _wb(noise_map=bad)
    with pytest.raises(ValueError, match="weighted_burst_sr.*all inf"):
        _wb(noise_map=np.full((SO, SO), np.inf))
    with pytest.raises(ValueError, match="weighted_burst_sr.*all inf"):
        _wb(frame_sigmas=[np.inf] * 4)
    for bad in ([0.1] * 3, [0.1] * 5, "0.1,0.2", [0.1]):
        with pytest.raises(ValueError, match="weighted_burst_sr.*frame_sigmas for 4 frames"):
            _wb(frame_sigmas=bad)
    with pytest.raises(ValueError, match="weighted_burst_sr.*<= 0"):
        _wb(frame_sigmas=[0.1, 0.0, 0.1, 0.1])
    with pytest.raises(ValueError, match="weighted_burst_sr.*NaN"):
        _wb(frame_sigmas=[0.1, np.nan, 0.1, 0.1])
    with pytest.raises(ValueError, match="weighted_burst_sr: frame_sigmas is"):
        _wb(frame_sigmas="0.1,x,0.1,0.1")
    for bad in ("rgbg", "bayer", 3, "rgg"):
        with pytest.raises(ValueError, match="weighted_burst_sr: mosaic is None or one of rggb, bggr, grbg, gbrg"):
            _wb(noise_map=m, mosaic=bad)


def test_the_parents_refusals_still_fire():
    m = noise_map_n(SO)
    with pytest.raises(ValueError, match="burst_sr.*scale_factor must be 2, 3 or 4"):
        _wb(noise_map=m, scale_factor=5)
    with pytest.raises(ValueError, match="burst_sr.*5 frames.*s\\^2 = 4"):
        _wb(noise_map=m, scale_factor=2, frame_shifts=[(0, 0)] * 5)
    with pytest.raises(ValueError, match="burst_sr needs exactly one of kernels"):
        _wb(noise_map=m, kernels=None)
    with pytest.raises(ValueError, match="burst_sr: the PSF of frame 1 is all zero"):
        _wb(noise_map=m, kernels=[PSF7, np.zeros((3, 3))])


# ---------------------------------------------------------------- mosaics
def test_bayer_sites():
    from free_hunch_amd.measurements import bayer_sites
    expect = {"rggb": [[0, 1], [1, 2]], "bggr": [[2, 1], [1, 0]], "grbg": [[1, 0], [2, 1]], "gbrg": [[1, 2], [0, 1]]}
    for pattern, cell in expect.items():
        for n in (4, 7):
            sites = bayer_sites(n, pattern)
            assert sites.shape == (3, n, n) and sites.dtype == bool
            assert (sites.sum(0) == 1).all()  # exactly one channel per site
            for y in range(n):
                for x in range(n):
                    assert sites[cell[y % 2][x % 2], y, x]
        assert np.array_equal(bayer_sites(4, pattern.upper()), bayer_sites(4, pattern))
    assert bayer_sites(4, "rggb")[1].sum() == 8 and bayer_sites(7, "rggb")[0].sum() == 16  # odd n: 4 x 4 red sites
    for bad in ("rgbg", "", None, 4):
        with pytest.raises(ValueError, match="bayer_sites"):
            bayer_sites(4, bad)


def test_mosaic_composes_with_each_source(tmp_path):
    from free_hunch_amd.measurements import bayer_sites
    K = 4
    f3 = map_f3(SO, K)
    np.save(tmp_path / "map.npy", f3)
    sites = np.tile(bayer_sites(SO, "grbg"), (K, 1, 1))[None]
    for kw in (dict(noise_map=f3), dict(noise_map_path=str(tmp_path / "map.npy")), dict(frame_sigmas=[0.02, 0.05, 0.1, 0.3])):
        plain, raw = _wb(**kw), _wb(mosaic="grbg", **kw)
        assert raw.mosaic == "grbg"
        assert np.array_equal(raw.noise_map.numpy(), np.where(sites, plain.noise_map.numpy(), np.inf))
        assert np.array_equal(raw.mask.numpy(), plain.mask.numpy() * sites)
        assert np.array_equal(raw.weights.numpy(), plain.weights.numpy() * sites)
    raw = _wb(frame_sigmas=[0.1] * 4, mosaic="RGGB")
    assert bool((raw.mask[0].reshape(K, 3, SO, SO).sum(1) == 1).all())  # one channel per site and frame
    assert _wb(frame_sigmas=[0.1] * 4, mosaic="").mosaic is None and _wb(frame_sigmas=[0.1] * 4, mosaic=None).mosaic is None


# ---------------------------------------------------------------- solver tables and the CLI
def test_op_code_and_name_lists():
    from free_hunch_amd import conditioning_mechanisms as cm
    name = "weighted_burst_sr"
    row = cm._OPS[name]
    assert cm._op_code(name) == row.op == 13 and row.decimating and row.unit_sigma == "always" and row.layout == "frames"
    assert "share the PSF" not in row.shares and row.layout != "mask" and cm._OPS["burst_sr"].unit_sigma != "always"
    for older in ("gaussian_blur", "custom_blur", "masked_blur", "custom_sr", "weighted_blur", "weighted_sr", "burst_sr", name):
        assert f"'{older}'" in cm._BAD_OPERATOR
    op = _wb(frame_sigmas=[0.1] * 4)
    assert cm._solver_sigma_y2(op) == 1.0 and cm._sigma_y2(op) == pytest.approx(0.05 ** 2)
    with pytest.raises(ValueError, match="Invalid operator name"):
        cm.choose_solver("weighted_burst", None, None, None)


def test_problem_fields_for_op_13():
    from free_hunch_amd import conditioning_mechanisms as cm

    class Cov:  # what _problem reads of a covariance
        use_dct, data_dim, device = True, 3 * 64 * 64, torch.device("cpu")

        class famC:
            m, B = 0, torch.zeros(1, dtype=torch.float64)

        class C:
            D = r = torch.zeros(1, dtype=torch.float64)
            M_dev = torch.zeros(1, 8, dtype=torch.float64)
    op = _wb(frame_shifts=FRACTIONAL, noise_map=map_f3(SO, 3))
    p, keep = cm._problem(op, Cov, cm._solver_sigma_y2(op))
    ft = op.frame_taps
    assert (p.op, p.stride, p.ntaps, p.ntaps2, p.halo2, p.halo, p.use_dct, p.fold_sym) == (13, 4, 177, 3, 64, ft.halo, 1, 0)
    assert p.tap_dy == ft.dy.data_ptr() and p.tap_dx == ft.dx.data_ptr() and p.tap_w == ft.w.data_ptr()
    assert p.tap2_dy == ft.off.data_ptr() and not p.tap2_dx and not p.tap2_w
    assert not (p.fold_fwd_w or p.fold_fwd_h or p.fold_inv_w or p.fold_inv_h)
    assert all(any(t is k for k in keep) for t in (ft.dy, ft.dx, ft.w, ft.off))
    assert p.mask == keep[-1].data_ptr() and torch.equal(keep[-1], op.weights) and tuple(keep[-1].shape) == (1, 9, SO, SO)
    assert p.sigma_y2 == 1.0 and p.planes == 3 and p.d == 3 * 64 * 64


def test_config_flags(tmp_path):
    from free_hunch_amd.config import SCHEMA, load_config
    assert SCHEMA["frame_sigmas"] == (str, "") and SCHEMA["mosaic"] == (str, "")
    base = [f"--outdir={tmp_path}", "--operator_name=weighted_burst_sr", f"--kernel_path={tmp_path}/psf.npy", "--scale_factor=4"]
    shifts, sig, path = "--frame_shifts=0,0;0.5,1.25;2,2", "--frame_sigmas=0.02,0.05,inf", f"--noise_map_path={tmp_path}/map.npy"
    gain, read = "--noise_gain=0.01", "--noise_read_sigma=0.02"
    o = load_config(base + [shifts, sig, "--mosaic=rggb"])
    assert o.operator_name == "weighted_burst_sr" and o.frame_sigmas == "0.02,0.05,inf" and o.mosaic == "rggb"
    assert o.frame_shifts == "0,0;0.5,1.25;2,2" and o.noise_map_path == "" and o.noise_gain is None
    o = load_config(base + [path])
    assert o.noise_map_path == f"{tmp_path}/map.npy" and o.frame_sigmas == "" and o.mosaic == ""
    o = load_config(base + [gain, read, "--mosaic=bggr"])
    assert o.noise_gain == 0.01 and o.noise_read_sigma == 0.02 and o.mosaic == "bggr"
    for none_or_two in ([], [sig, path], [sig, gain, read], [path, gain, read], [sig, path, gain, read]):
        with pytest.raises(SystemExit, match="weighted_burst_sr needs a noise map: exactly one of"):
            load_config(base + none_or_two)
    for half in ([gain], [read], [sig, gain]):
        with pytest.raises(SystemExit, match="--noise_gain and --noise_read_sigma go together"):
            load_config(base + half)
    with pytest.raises(SystemExit, match="burst_sr needs --kernel_path"):
        load_config([f"--outdir={tmp_path}", "--operator_name=weighted_burst_sr", "--scale_factor=4", sig])
    with pytest.raises(SystemExit, match="masked_blur"):
        load_config(base + [sig, "--mask_border=2"])
    for other in ("burst_sr", "weighted_sr", "gaussian_blur"):
        args = [f"--outdir={tmp_path}", f"--operator_name={other}"]
        if other != "gaussian_blur":
            args.append(f"--kernel_path={tmp_path}/psf.npy")
        if other == "weighted_sr":
            args.append(path)
        for flag in (sig, "--mosaic=rggb"):
            with pytest.raises(SystemExit, match="--frame_sigmas and --mosaic belong to --operator_name=weighted_burst_sr"):
                load_config(args + [flag])
    with pytest.raises(SystemExit, match="weighted_blur / weighted_sr"):  # the noise flags stay refused elsewhere
        load_config([f"--outdir={tmp_path}", "--operator_name=burst_sr", f"--kernel_path={tmp_path}/psf.npy", path])
    with pytest.raises(SystemExit, match="custom_sr.*burst_sr.*weighted_burst_sr"):
        load_config([f"--outdir={tmp_path}", "--operator_name=gaussian_blur", f"--kernel_path={tmp_path}/psf.npy"])
