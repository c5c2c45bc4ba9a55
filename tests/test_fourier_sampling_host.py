"""Host-side checks of `fourier_sampling` (undersampled k-space measured in the Hartley domain, fh_problem.op = 15): the folded
bases, the numpy restatement the device tests lean on, `kspace_mask`, the complex <-> Hartley converters with their noise rules,
the operator's mask handling, the solver tables and the CLI flags.  No GPU: operators are built on device="cpu"."""
import ctypes as C

import numpy as np
import pytest
import torch

import _fourier_restatement as fr


def _op(S=30, **kw):
    from free_hunch_amd.measurements import get_operator
    if not any(k in kw for k in ("mask", "mask_path", "pattern")):
        kw.update(pattern="cartesian", acceleration=4.0)
    return get_operator(name="fourier_sampling", device="cpu", sigma_s=0.05, in_shape=(1, 3, S, S), **kw)


# ---------------------------------------------------------------- bases
@pytest.mark.parametrize("S", [6, 30, 256])
def test_bases(S):
    from free_hunch_amd.measurements import dct_basis_longdouble, folded_dct_hartley_bases
    Hc, P = folded_dct_hartley_bases(S, True)
    assert Hc.dtype == P.dtype == np.float64 and Hc.shape == P.shape == (S, S) and Hc.flags["C_CONTIGUOUS"] and P.flags["C_CONTIGUOUS"]
    assert np.array_equal(Hc, Hc.T)
    assert np.abs(Hc @ Hc - np.eye(S)).max() <= 1e-14
    assert np.abs(Hc - fr.cas_basis(S)).max() <= 1e-15 * S  # the plain float64 formula loses a few ulps to its angle
    # P = C_dct Hc against an independent extended-precision product, to 1 ulp of float64
    ld = np.longdouble
    k = (np.arange(S)[:, None] * np.arange(S)[None, :]) % S
    a = k.astype(ld) * (2 * np.arccos(ld(-1)) / S)
    want = dct_basis_longdouble(S) @ ((np.cos(a) + np.sin(a)) / np.sqrt(ld(S)))
    ulp = np.spacing(np.maximum(np.abs(want.astype(np.float64)), np.finfo(np.float64).tiny))
    assert (np.abs(P.astype(ld) - want) <= ulp).all()
    assert np.abs(P @ P.T - np.eye(S)).max() <= 1e-13  # orthogonal: the product of two orthogonal matrices
    Hc0, P0 = folded_dct_hartley_bases(S, False)
    assert np.array_equal(Hc0, Hc) and np.array_equal(P0, Hc)
    for bad in (0, 1, 7, -2):
        with pytest.raises(ValueError, match="folded_dct_hartley_bases"):
            folded_dct_hartley_bases(bad)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("S", [6, 16, 30])
def test_restatement(S):
    from free_hunch_amd.measurements import folded_dct_hartley_bases
    Hc, _P = folded_dct_hartley_bases(S)
    rng = np.random.default_rng(S)
    X, Y = rng.standard_normal((3, S, S)), rng.standard_normal((3, S, S))
    T = Hc @ X @ Hc
    F = np.fft.fft2(X, norm="ortho")
    assert np.abs(fr.butterfly(T) - (F.real - F.imag)).max() <= 1e-13
    assert np.abs(fr.hartley2(X) - (F.real - F.imag)).max() == 0.0
    assert np.abs(fr.butterfly(fr.butterfly(T)) - T).max() <= 1e-15 * max(1.0, np.abs(T).max())  # R is an involution
    assert np.abs(fr.hartley2(fr.hartley2(X)) - X).max() <= 1e-13  # H H = I
    assert np.abs(Hc @ fr.butterfly(fr.butterfly(Hc @ X @ Hc)) @ Hc - X).max() <= 1e-13
    lhs, rhs = float((fr.hartley2(X) * Y).sum()), float((X * fr.hartley2(Y)).sum())  # A0 = A0^T: the dot test
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    lhs, rhs = float((fr.butterfly(X) * Y).sum()), float((X * fr.butterfly(Y)).sum())  # R = R^T
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    # Re F = (H[k] + H[-k]) / 2, Im F = (H[-k] - H[k]) / 2
    H = fr.hartley2(X)
    assert np.abs(0.5 * (H + fr.reflect(H)) - F.real).max() <= 1e-14 and np.abs(0.5 * (fr.reflect(H) - H) - F.imag).max() <= 1e-14
    # at S = 2 every point is its own reflection and R is the identity, bit for bit
    Z = rng.standard_normal((3, 2, 2))
    assert np.array_equal(fr.butterfly(Z), Z)


# ---------------------------------------------------------------- kspace_mask
@pytest.mark.parametrize("S", [30, 64, 256])
@pytest.mark.parametrize("pattern", ["cartesian", "radial"])
def test_kspace_mask(S, pattern):
    from free_hunch_amd.measurements import kspace_mask
    for acc, cf, seed in ((4.0, 0.08, 0), (2.0, 0.0, 3), (8, 0.04, 11)):
        m = kspace_mask(S, pattern, acc, cf, seed)
        assert m.dtype == np.float64 and m.shape == (S, S) and np.isin(m, (0.0, 1.0)).all()
        assert np.array_equal(m, fr.reflect(m)), "not symmetric under the point reflection"
        assert m[0, 0] == 1.0
        assert np.array_equal(m, kspace_mask(S, pattern, acc, cf, seed))
        assert not np.array_equal(m, kspace_mask(S, pattern, acc, cf, seed + 1))
        if pattern == "cartesian":
            assert (m == m[:, :1]).all()  # whole lines along one axis
            assert abs(m.mean() - (1.0 / acc + cf)) <= 2.0 / S  # one +-u line pair
            nc = cf * S
            band = np.minimum(np.arange(S), S - np.arange(S)) <= (nc - 2.0) / 2.0  # every line the band surely holds
            assert m[band, 0].all()
        else:
            assert 0 < m.sum() < S * S and m[1, 0] + m[0, 1] + m[1, 1] + m[S - 1, 1] >= 1  # spokes leave DC
    assert kspace_mask(S, pattern, 1.0, 0.0, 0).mean() > (0.99 if pattern == "cartesian" else 0.5)


def test_kspace_mask_refusals():
    from free_hunch_amd.measurements import kspace_mask
    good = dict(S=64, pattern="cartesian", acceleration=4.0, center_fraction=0.08, seed=0)
    assert kspace_mask(**good).any()
    for change in (dict(S=63), dict(S=0), dict(pattern="spiral"), dict(pattern=None), dict(acceleration=0.5), dict(acceleration=0),
                   dict(acceleration=float("nan")), dict(acceleration=float("inf")), dict(acceleration="fast"),
                   dict(center_fraction=-0.1), dict(center_fraction=1.0), dict(center_fraction=float("nan")), dict(seed=-1),
                   dict(seed=0.5), dict(seed=True)):
        with pytest.raises(ValueError, match="kspace_mask"):
            kspace_mask(**{**good, **change})


# ---------------------------------------------------------------- the converters
def test_converters_round_trip():
    from free_hunch_amd.measurements import hartley_to_kspace, kspace_mask, kspace_to_hartley
    S = 30
    rng = np.random.default_rng(5)
    X = rng.standard_normal((3, S, S))
    F = np.fft.fft2(X, norm="ortho")
    full = np.ones((S, S))
    y, ms, nm = kspace_to_hartley(F, full, 0.1)
    assert np.array_equal(ms, full) and np.allclose(nm, 0.1, rtol=1e-15, atol=0) and np.abs(y - fr.hartley2(X)).max() <= 1e-14
    assert np.abs(hartley_to_kspace(y) - F).max() <= 1e-14
    # an undersampled symmetric mask: the data on the mask round-trip, both ways
    m = kspace_mask(S, "radial", 3.0, 0.0, 2)
    y, ms, nm = kspace_to_hartley(F * m, m, 0.1)
    assert np.array_equal(ms, m) and np.array_equal(y, y * m) and np.abs(y - fr.hartley2(X) * m).max() <= 1e-14
    back = hartley_to_kspace(y, ms)
    assert np.abs(back - F * m).max() <= 1e-14
    y2, ms2, nm2 = kspace_to_hartley(back, ms, 0.1)
    assert np.abs(y2 - y).max() <= 1e-15 and np.array_equal(ms2, ms) and np.allclose(nm2, nm, rtol=1e-15, atol=0)
    for bad in (dict(F=F[..., :-1]), dict(mask=np.ones((S, S + 2))), dict(mask=full * 0.5), dict(sigma=0.0), dict(sigma=-1.0),
                dict(sigma=np.ones((3, 3))), dict(mask=np.zeros((S, S)))):
        with pytest.raises(ValueError, match="kspace_to_hartley"):
            kspace_to_hartley(**{**dict(F=F, mask=full, sigma=0.1), **bad})


def test_converter_noise_rules_on_a_six_grid():
    """S = 6 has four self-conjugate points, (0,0), (0,3), (3,0), (3,3).  One of a pair measured: the conjugate is filled in and
    both Hartley entries carry sqrt(2) sigma; both measured: averaged, sigma; self-conjugate: the imaginary part is dropped, sigma.
    The rules are then confirmed by sampling: the whitened Hartley noise has unit variance and no correlation in a pair."""
    from free_hunch_amd.measurements import kspace_to_hartley
    S, sig = 6, 0.3
    selfc = [(0, 0), (0, 3), (3, 0), (3, 3)]
    rng = np.random.default_rng(9)
    F = rng.standard_normal((S, S)) + 1j * rng.standard_normal((S, S))  # NOT Hermitian: the two of a pair disagree
    m = np.zeros((S, S))
    m[1, 2] = 1.0                # only k of the pair (1,2) / (5,4)
    m[2, 1] = m[4, 5] = 1.0      # both of the pair (2,1) / (4,5)
    m[0, 3] = m[3, 3] = 1.0      # two self-conjugate points
    y, ms, nm = kspace_to_hartley(F, m, sig)
    assert ms.sum() == 6 and ms[5, 4] == 1.0 and ms[1, 2] == 1.0 and np.array_equal(ms, fr.reflect(ms))
    assert np.isinf(nm[ms == 0]).all() and (y[ms == 0] == 0).all()
    a, b = F[1, 2].real, F[1, 2].imag
    assert y[1, 2] == pytest.approx(a - b, abs=1e-15) and y[5, 4] == pytest.approx(a + b, abs=1e-15)
    assert nm[1, 2] == pytest.approx(np.sqrt(2) * sig, rel=1e-15) and nm[5, 4] == pytest.approx(np.sqrt(2) * sig, rel=1e-15)
    avg = 0.5 * (F[2, 1] + np.conj(F[4, 5]))
    assert y[2, 1] == pytest.approx(avg.real - avg.imag, abs=1e-15) and y[4, 5] == pytest.approx(avg.real + avg.imag, abs=1e-15)
    assert nm[2, 1] == pytest.approx(sig, rel=1e-15) and nm[4, 5] == pytest.approx(sig, rel=1e-15)
    for p in ((0, 3), (3, 3)):
        assert y[p] == pytest.approx(F[p].real, abs=1e-15) and nm[p] == pytest.approx(sig, rel=1e-15)
    assert all((2 * u) % S == 0 and (2 * v) % S == 0 for u, v in selfc)
    # a sigma map: the pair's two levels combine as sqrt((s_k^2 + s_-k^2) / 2)
    smap = np.full((S, S), sig)
    smap[4, 5] = 2 * sig
    nm2 = kspace_to_hartley(F, m, smap)[2]
    assert nm2[2, 1] == pytest.approx(sig * np.sqrt(2.5), rel=1e-15) and nm2[4, 5] == pytest.approx(sig * np.sqrt(2.5), rel=1e-15)
    # sampling: complex noise with per-component sigma on the measured samples
    n = 40000
    noise = sig * (rng.standard_normal((n, S, S)) + 1j * rng.standard_normal((n, S, S)))
    yn = kspace_to_hartley(noise, m, sig)[0]
    white = yn[:, ms > 0] / nm[ms > 0]
    assert np.abs(white.var(0) - 1.0).max() < 0.05
    corr = np.corrcoef(white.T)
    assert np.abs(corr - np.eye(corr.shape[0])).max() < 0.03


# ---------------------------------------------------------------- the operator's mask handling
def test_operator_masks(tmp_path):
    from free_hunch_amd.measurements import FourierSamplingOperator, LinearOperator, kspace_mask
    S = 30
    op = _op(S)
    assert isinstance(op, FourierSamplingOperator) and isinstance(op, LinearOperator) and op.name == "fourier_sampling"
    assert tuple(op.in_shape) == tuple(op.out_shape) == (1, 3, S, S) and op.noise_map is None and op.weights is op.mask
    want = kspace_mask(S, "cartesian", 4.0, 0.08, 0)
    assert op.mask.dtype == torch.float64 and np.array_equal(op.mask.numpy(), np.broadcast_to(want, (1, 3, S, S)))
    assert op.folded_bases() is None and op.folded_sr_bases() is None
    assert not np.array_equal(_op(S, pattern="cartesian", acceleration=4.0, seed=5).mask.numpy(), op.mask.numpy())
    # an unsymmetric user mask is OR-ed with its point reflection
    m = np.zeros((S, S))
    m[0, 0] = m[1, 2] = m[7, 0] = 1.0
    got = _op(S, mask=m).mask.numpy()[0, 0]
    sym = m.copy()
    sym[S - 1, S - 2] = sym[S - 7, 0] = 1.0
    assert np.array_equal(got, sym)
    np.save(tmp_path / "m.npy", m)
    assert np.array_equal(_op(S, mask_path=str(tmp_path / "m.npy")).mask.numpy()[0, 1], sym)
    per_channel = np.stack([m, sym, np.ones((S, S))])
    assert np.array_equal(_op(S, mask=torch.from_numpy(per_channel)).mask.numpy()[0], np.stack([sym, sym, np.ones((S, S))]))
    assert np.array_equal(_op(S, mask=per_channel[None]).mask.numpy()[0, 0], sym)
    # refusals
    with pytest.raises(ValueError, match="fourier_sampling: the mask is all zero"):
        _op(S, mask=np.zeros((S, S)))
    for shape in ((S, S + 2), (2, S, S), (S,), (1, 1, S, S)):
        with pytest.raises(ValueError, match="fourier_sampling: the mask must have shape"):
            _op(S, mask=np.ones(shape))
    for bad in (0.5, 2.0, -1.0, np.nan):
        mm = np.ones((S, S))
        mm[3, 3] = bad
        with pytest.raises(ValueError, match="fourier_sampling: the mask has an entry other than 0 and 1"):
            _op(S, mask=mm)
    for kw in (dict(mask=None, mask_path=None, pattern=None), dict(mask=m, pattern="radial"),
               dict(mask=m, mask_path=str(tmp_path / "m.npy")), dict(mask_path=str(tmp_path / "m.npy"), pattern="cartesian")):
        with pytest.raises(ValueError, match="fourier_sampling needs exactly one of mask"):
            from free_hunch_amd.measurements import get_operator
            get_operator(name="fourier_sampling", device="cpu", sigma_s=0.05, in_shape=(1, 3, S, S), **kw)
    with pytest.raises(ValueError, match="kspace_mask"):
        _op(S, pattern="spiral")
    with pytest.raises(ValueError, match="even side"):
        _op(31)
    # a noise map: weights = 1 / sigma on the mask, 0 off it or where inf; floor 0.001; the _NoiseMap checks
    nm = np.full((S, S), 0.2)
    nm[0, 0] = 1e-5
    nm[2:4] = np.inf
    w = _op(S, mask=np.ones((S, S)), noise_map=nm)
    assert w.weights[0, 0, 0, 0] == 1000.0 and float(w.weights[0, 1, 5, 5]) == 5.0 and not w.weights[0, :, 2:4].any()
    assert np.isinf(w.noise_map[0, :, 2:4].numpy()).all() and np.array_equal(w.mask.numpy(), (w.weights > 0).numpy().astype(np.float64))
    both = _op(S, noise_map=nm)
    assert np.array_equal(both.mask.numpy()[0, 0], want * np.isfinite(nm)) and np.isinf(both.noise_map.numpy()[both.mask.numpy() == 0]).all()
    for bad in (0.0, -0.1, np.nan):
        b = nm.copy()
        b[5, 5] = bad
        with pytest.raises(ValueError, match="fourier_sampling: the noise map has"):
            _op(S, noise_map=b)
    off = np.full((S, S), np.inf)
    off[0, 1] = 0.1  # finite only where the symmetrised mask below is 0
    with pytest.raises(ValueError, match="fourier_sampling: no frequency is both on the mask and finite"):
        _op(S, mask=sym, noise_map=off)


# ---------------------------------------------------------------- solver tables, the problem
def test_solver_tables():
    from free_hunch_amd import conditioning_mechanisms as cm
    name = "fourier_sampling"
    assert cm._op_code(name) == 15 and cm._op_code("varying_blur") == 14 and cm._op_code("noise") == 0 and cm._op_code("fourier") is None
    row = cm._OPS[name]
    assert row.op == 15 and len(cm._OPS) == 15 and [n for n, r in cm._OPS.items() if r.op == 15] == [name]
    assert f"'{name}'" in cm._BAD_OPERATOR and cm._BAD_OPERATOR.rstrip(".").endswith("'varying_blur'")
    # not decimating, unit sigma only with a noise map, not the frames' layout, no shared PSF, no 0/1-mask operator
    assert not row.decimating and row.unit_sigma == "noise_map" and row.layout == "hartley" and "share the PSF" not in row.shares
    op = _op()
    assert cm._solver_sigma_y2(op) == cm._sigma_y2(op) == pytest.approx(0.05 ** 2)
    tiny = _op()
    tiny.sigma_s = torch.Tensor([0.0001])
    assert cm._solver_sigma_y2(tiny) == pytest.approx(0.001 ** 2)  # the blur rule's clip
    assert cm._solver_sigma_y2(_op(noise_map=np.full((30, 30), 0.2))) == 1.0
    with pytest.raises(ValueError, match="Invalid operator name"):
        cm.choose_solver("fourier", None, None, None)


def test_problem_fields_for_op_15():
    from free_hunch_amd import conditioning_mechanisms as cm
    from free_hunch_amd.measurements import folded_dct_hartley_bases
    S = 30

    class Cov:  # what _problem reads of a covariance
        use_dct, data_dim, device = True, 3 * S * S, torch.device("cpu")

        class famC:
            m, B = 0, torch.zeros(1, dtype=torch.float64)

        class C:
            D = r = torch.zeros(1, dtype=torch.float64)
            M_dev = torch.zeros(1, 8, dtype=torch.float64)
    op = _op(S, noise_map=np.full((S, S), 0.5))
    p, keep = cm._problem(op, Cov, cm._solver_sigma_y2(op))
    assert (p.op, p.stride, p.ntaps, p.ntaps2, p.halo, p.halo2, p.use_dct, p.fold_sym, p.planes, p.d) == (15, 1, 0, 0, 0, 0, 1, 0, 3, 3 * S * S)
    assert not (p.tap_dy or p.tap_dx or p.tap_w or p.tap2_dy or p.tap2_dx or p.tap2_w) and p.sigma_y2 == 1.0
    assert p.fold_fwd_w == p.fold_fwd_h and p.fold_inv_w == p.fold_inv_h and p.fold_fwd_w != p.fold_inv_w
    P, Pt, w = keep[-3:]
    assert p.fold_fwd_w == P.data_ptr() and p.fold_inv_w == Pt.data_ptr() and p.mask == w.data_ptr()
    want = folded_dct_hartley_bases(S, True)[1]
    assert np.array_equal(P.numpy(), want) and np.array_equal(Pt.numpy(), want.T) and Pt.is_contiguous()
    assert torch.equal(w, op.weights) and w.dtype == torch.float64 and w.is_contiguous() and tuple(w.shape) == (1, 3, S, S)
    Cov.use_dct = False
    p0, keep0 = cm._problem(op, Cov, 1.0)
    assert p0.use_dct == 0 and np.array_equal(keep0[-3].numpy(), folded_dct_hartley_bases(S, False)[0])


# ---------------------------------------------------------------- the CLI flags
def test_config_flags(tmp_path):
    from free_hunch_amd.config import SCHEMA, load_config
    assert SCHEMA["kspace_pattern"] == (str, "") and SCHEMA["kspace_acceleration"] == (float, None)
    assert SCHEMA["kspace_center_fraction"] == (float, None) and SCHEMA["kspace_seed"] == (int, None)
    base = [f"--outdir={tmp_path}", "--operator_name=fourier_sampling"]
    mask, nmap = f"--mask_path={tmp_path}/m.npy", f"--noise_map_path={tmp_path}/n.npy"
    pat, acc = "--kspace_pattern=cartesian", "--kspace_acceleration=4"
    o = load_config(base + [pat, acc])
    assert (o.kspace_pattern, o.kspace_acceleration, o.kspace_center_fraction, o.kspace_seed, o.mask_path) == ("cartesian", 4.0, None, None, "")
    o = load_config(base + ["--kspace_pattern=radial", "--kspace_acceleration=6.5", "--kspace_center_fraction=0.04", "--kspace_seed=3", nmap])
    assert (o.kspace_pattern, o.kspace_acceleration, o.kspace_center_fraction, o.kspace_seed) == ("radial", 6.5, 0.04, 3)
    assert o.noise_map_path == f"{tmp_path}/n.npy"
    o = load_config(base + [mask, nmap])
    assert o.mask_path == f"{tmp_path}/m.npy" and o.kspace_pattern == ""
    for none_or_both in ([], [mask, pat, acc]):
        with pytest.raises(SystemExit, match="fourier_sampling needs its sampling mask: exactly one of --mask_path=FILE.npy and --kspace_pattern"):
            load_config(base + none_or_both)
    with pytest.raises(SystemExit, match="--kspace_pattern is cartesian or radial"):
        load_config(base + ["--kspace_pattern=spiral", acc])
    with pytest.raises(SystemExit, match="--kspace_pattern needs --kspace_acceleration"):
        load_config(base + [pat])
    for extra in (acc, "--kspace_center_fraction=0.1", "--kspace_seed=1"):
        with pytest.raises(SystemExit, match="go with --kspace_pattern, not with --mask_path"):
            load_config(base + [mask, extra])
    with pytest.raises(SystemExit, match="--mask_border belongs to --operator_name=masked_blur"):
        load_config(base + [mask, "--mask_border=2"])
    with pytest.raises(SystemExit, match="operator 'fourier_sampling' reads --noise_map_path only"):
        load_config(base + [mask, "--noise_gain=0.1", "--noise_read_sigma=0.01"])
    with pytest.raises(SystemExit, match="--kernel_path is the PSF of"):
        load_config(base + [mask, f"--kernel_path={tmp_path}/k.npy"])
    with pytest.raises(SystemExit, match="--frame_shifts belongs to"):
        load_config(base + [mask, "--frame_shifts=0,0"])
    # the --kspace_* flags are refused everywhere else, and the two shared flags keep their other owners
    psf = f"--kernel_path={tmp_path}/k.npy"
    for other, extra in (("gaussian_blur", []), ("custom_blur", [psf]), ("inpainting", []), ("varying_blur", [psf, "--psf_grid=2x2"]),
                         ("masked_blur", [psf, "--mask_border=2"]), ("weighted_blur", [psf, nmap])):
        args = [f"--outdir={tmp_path}", f"--operator_name={other}"] + extra
        load_config(args)
        for flag in (pat, acc, "--kspace_center_fraction=0.1", "--kspace_seed=0"):
            with pytest.raises(SystemExit, match="belong to --operator_name=fourier_sampling"):
                load_config(args + [flag])
    with pytest.raises(SystemExit, match="--mask_path and --mask_border belong to --operator_name=masked_blur"):
        load_config([f"--outdir={tmp_path}", "--operator_name=gaussian_blur", mask])
    with pytest.raises(SystemExit, match="--noise_map_path, --noise_gain and --noise_read_sigma belong to"):
        load_config([f"--outdir={tmp_path}", "--operator_name=gaussian_blur", nmap])
    assert load_config([f"--outdir={tmp_path}", "--operator_name=masked_blur", psf, mask]).mask_path


# ---------------------------------------------------------------- the library's surface
def test_exported_symbols_header_and_plan():
    import os
    from free_hunch_amd import _lib
    names = {"fh_hartley_fix", "fh_hartley2d", "fh_hartley2d_plan"}
    assert names <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.fh_hartley_fix.restype is C.c_int and len(lib.fh_hartley_fix.argtypes) == 8 and len(lib.fh_hartley2d.argtypes) == 6
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fh_hip.h")).read()
    assert all(f"int {n}(" in header for n in names) and "15 Fourier sampling" in header
    out = (C.c_int32 * 15)(*([7] * 15))
    rect = (C.c_int32 * 10)()
    for S, planes in ((2, 1), (6, 3), (30, 3), (64, 9), (128, 24), (256, 3), (256, 24), (256, 48), (256, 51), (170, 3), (172, 3)):
        assert lib.fh_hartley2d_plan(S, planes, out) == 0 and lib.fh_dct_rect_plan(S, S, planes, 0, rect) == 0
        assert list(out)[:10] == list(rect)
        units = S // 2 + 1
        trips = -(-units // 85)
        gx = -(-units // trips)
        assert list(out)[10:] == [gx, min(planes, 48), 1, 256, 16 * S], (S, planes, list(out))
        assert 3 * gx <= 256 and gx * trips >= units  # the p.Ap partials of an image fit the consumer's 256
    assert list(out)[10] == 44  # S = 172: 87 row pairs in two trips
    for S, planes in ((0, 3), (7, 3), (258, 3), (64, 0), (64, 65536)):
        assert lib.fh_hartley2d_plan(S, planes, out) == _lib.FH_EINVAL and list(out) == [0] * 15
    assert lib.fh_hartley2d_plan(64, 3, None) == _lib.FH_EINVAL
