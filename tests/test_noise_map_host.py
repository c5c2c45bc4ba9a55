"""Host-side checks of `weighted_blur` / `weighted_sr` (a per-pixel noise map in the solver): registry and attributes, every
refusal of the map, clipping, the weights and the mask derived from inf, `poisson_gaussian_sigma`, the op-code tables and the
CLI flags.  No GPU: the operators are built on device="cpu"."""
import numpy as np
import pytest
import torch

from test_custom_psf_host import disk_psf
from test_custom_sr_host import binomial_psf, box_psf

S = 64


def noise_map_n(n):
    """Map N: sigma = sqrt(0.03^2 + 0.1^2 g), g = 0.5 + 0.5 sin(2 pi y / n) cos(2 pi x / n) (0.03 .. 0.104), inf where
    default_rng(5).random((n, n)) < 0.1; one map for the three channels."""
    yy, xx = np.mgrid[0:n, 0:n]
    g = 0.5 + 0.5 * np.sin(2 * np.pi * yy / n) * np.cos(2 * np.pi * xx / n)
    sig = np.sqrt(0.03 ** 2 + 0.1 ** 2 * g)
    sig[np.random.default_rng(5).random((n, n)) < 0.1] = np.inf
    return sig


def noise_map_n3(n):
    """Map N3: N with channel c multiplied by (1, 1.5, 2)[c] - a wrong plane offset shows."""
    return np.stack([noise_map_n(n) * f for f in (1.0, 1.5, 2.0)])


def _wb(**kw):
    from free_hunch_amd.measurements import get_operator
    if "kernel" not in kw and "kernel_path" not in kw:
        kw["kernel"] = binomial_psf(9, 13)
    return get_operator(name="weighted_blur", device="cpu", sigma_s=0.05, in_shape=(1, 3, S, S), **kw)


def _wsr(**kw):
    from free_hunch_amd.measurements import get_operator
    kw.setdefault("scale_factor", 4)
    if "kernel" not in kw and "kernel_path" not in kw:
        kw["kernel"] = box_psf(4)
    return get_operator(name="weighted_sr", device="cpu", sigma_s=0.05, in_shape=(1, 3, S, S), **kw)


def test_map_n_is_the_stated_one():
    m = noise_map_n(S)
    fin = np.isfinite(m)
    assert abs(fin.mean() - 0.89) < 0.01 and 0.03 <= m[fin].min() and m[fin].max() <= 0.1045
    m3 = noise_map_n3(S)
    assert m3.shape == (3, S, S) and np.array_equal(np.isfinite(m3[2]), fin) and np.array_equal(m3[1][fin], 1.5 * m[fin])


def test_registry_and_attributes(tmp_path):
    from free_hunch_amd.measurements import CustomBlurOperator, CustomSROperator, WeightedBlurOperator, WeightedSROperator
    m = noise_map_n(S)
    np.save(tmp_path / "map.npy", m)
    for op in (_wb(noise_map=m), _wb(noise_map_path=str(tmp_path / "map.npy")), _wb(noise_map=torch.from_numpy(m))):
        assert isinstance(op, WeightedBlurOperator) and isinstance(op, CustomBlurOperator) and op.name == "weighted_blur"
        assert tuple(op.noise_map.shape) == tuple(op.weights.shape) == tuple(op.mask.shape) == (1, 3, S, S)
        assert op.noise_map.dtype == op.weights.dtype == torch.float64
        assert np.array_equal(op.noise_map[0, 1].numpy(), m)  # every entry of N is above the floor: kept as given
        assert float(op.sigma_s) == pytest.approx(0.05) and op.taps.sep is not None
    m16 = noise_map_n(16)
    op = _wsr(noise_map=m16)
    assert isinstance(op, WeightedSROperator) and isinstance(op, CustomSROperator) and op.name == "weighted_sr"
    assert op.scale_factor == 4 and op.out_shape == (1, 3, 16, 16) and tuple(op.noise_map.shape) == (1, 3, 16, 16)
    assert op.folded_bases() is None
    for shape_of in (lambda a: a, lambda a: np.stack([a] * 3), lambda a: np.stack([a] * 3)[None]):
        assert torch.equal(_wb(noise_map=shape_of(m)).weights, _wb(noise_map=m).weights)
        assert torch.equal(_wsr(noise_map=shape_of(m16)).weights, op.weights)
    assert not torch.equal(_wb(noise_map=noise_map_n3(S)).weights[0, 0], _wb(noise_map=noise_map_n3(S)).weights[0, 2])


def test_weights_and_mask_follow_inf():
    m = noise_map_n(S)
    op = _wb(noise_map=m)
    fin = torch.from_numpy(np.isfinite(m))
    for c in range(3):
        assert torch.equal(op.mask[0, c] > 0, fin) and torch.equal(op.weights[0, c] > 0, fin)
        assert bool((op.weights[0, c][~fin] == 0).all()) and bool(torch.isinf(op.noise_map[0, c][~fin]).all())
        assert torch.equal(op.weights[0, c][fin], 1.0 / op.noise_map[0, c][fin])
    assert set(np.unique(op.mask.numpy())) == {0.0, 1.0} and bool(torch.isfinite(op.weights).all())


def test_finite_entries_are_clipped_from_below_like_sigma_y2():
    m = np.full((S, S), 0.05)
    m[0, 0], m[0, 1], m[0, 2] = 1e-5, 0.005, np.inf
    op = _wb(noise_map=m)
    assert op.noise_map[0, 0, 0, 0] == 0.001 and op.weights[0, 0, 0, 0] == 1000.0  # blur: 0.001
    assert op.noise_map[0, 0, 0, 1] == 0.005 and op.noise_map[0, 0, 1, 1] == 0.05 and torch.isinf(op.noise_map[0, 0, 0, 2])
    m16 = np.full((16, 16), 0.05)
    m16[0, 0], m16[0, 1], m16[0, 2] = 1e-5, 0.005, np.inf
    sr = _wsr(noise_map=m16)
    assert sr.noise_map[0, 0, 0, 0] == 0.01 and sr.noise_map[0, 0, 0, 1] == 0.01 and sr.weights[0, 2, 0, 1] == 100.0  # SR: 0.01
    assert sr.noise_map[0, 0, 1, 1] == 0.05 and sr.weights[0, 0, 0, 2] == 0.0


def test_refusals_name_the_rule(tmp_path):
    good = np.full((S, S), 0.05)
    with pytest.raises(ValueError, match="exactly one"):
        _wb()
    np.save(tmp_path / "map.npy", good)
    with pytest.raises(ValueError, match="exactly one"):
        _wb(noise_map=good, noise_map_path=str(tmp_path / "map.npy"))
    with pytest.raises(ValueError, match="exactly one"):
        _wsr()
    for bad_shape in ((S, S + 1), (2, S, S), (1, 1, S, S), (S,), (16, 16)):
        with pytest.raises(ValueError, match="shape"):
            _wb(noise_map=np.full(bad_shape, 0.05))
    with pytest.raises(ValueError, match="shape"):  # the SR map lives at the low-resolution side
        _wsr(noise_map=good)
    for value, word in ((np.nan, "NaN"), (0.0, "<= 0"), (-0.1, "<= 0"), (-np.inf, "<= 0")):
        bad = good.copy()
        bad[3, 4] = value
        with pytest.raises(ValueError, match=word):
            _wb(noise_map=bad)
        bad16 = np.full((16, 16), 0.05)
        bad16[3, 4] = value
        with pytest.raises(ValueError, match=word):
            _wsr(noise_map=bad16)
    with pytest.raises(ValueError, match="all inf"):
        _wb(noise_map=np.full((S, S), np.inf))
    with pytest.raises(ValueError, match="PSF"):  # the parent's PSF checks stay
        _wb(noise_map=good, kernel=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="custom_sr"):  # and the parent's factor checks
        _wsr(noise_map=np.full((16, 16), 0.05), scale_factor=3)
    with pytest.raises(ValueError, match="per-pixel weights are not supported"):  # masked_blur keeps its own rule
        from free_hunch_amd.measurements import get_operator
        get_operator(name="masked_blur", device="cpu", sigma_s=0.05, in_shape=(1, 3, S, S), kernel=box_psf(3), mask=0.5 * np.ones((S, S)))


def test_poisson_gaussian_sigma_values():
    from free_hunch_amd.measurements import poisson_gaussian_sigma as pgs
    g, r = 0.01, 0.02
    y = np.array([-1.0, 0.0, 1.0, -3.0, 5.0])
    want = 2.0 * np.sqrt(g * np.array([0.0, 0.5, 1.0, 0.0, 1.0]) + r ** 2)
    assert np.allclose(pgs(y, g, r), want, rtol=1e-15, atol=0)
    assert pgs(y, g, r)[0] == 2 * r and pgs(y, 0.0, r).tolist() == [2 * r] * 5  # read noise alone below black
    t = pgs(torch.from_numpy(y), g, r)
    assert torch.is_tensor(t) and t.dtype == torch.float64 and np.allclose(t.numpy(), want, rtol=1e-15, atol=0)
    assert pgs(torch.zeros(2, 3, dtype=torch.float32), g, r).dtype == torch.float32
    for bad in ((-0.1, 0.01), (0.01, -1.0), (float("nan"), 0.01), (0.0, 0.0)):
        with pytest.raises(ValueError, match="gain"):
            pgs(y, *bad)


def test_op_code_tables():
    from free_hunch_amd import conditioning_mechanisms as cm
    wb, ws = cm._OPS["weighted_blur"], cm._OPS["weighted_sr"]
    assert cm._op_code("weighted_blur") == wb.op == 8 and cm._op_code("weighted_sr") == ws.op == 10
    assert "share the PSF" in wb.shares and "share the PSF" in ws.shares and ws.decimating
    assert not wb.decimating and wb.layout != "mask" and ws.layout != "mask"
    for name in ("gaussian_blur", "custom_blur", "masked_blur", "custom_sr", "weighted_blur", "weighted_sr"):
        assert f"'{name}'" in cm._BAD_OPERATOR
    assert cm._solver_sigma_y2(_wb(noise_map=np.full((S, S), 0.05))) == 1.0
    with pytest.raises(ValueError, match="Invalid operator name"):
        cm.choose_solver("weighted", None, None, None)


def test_problem_routes_follow_the_parents():
    """_problem on a stand-in covariance (no device): a sparse or rank-1 PSF stays op 8, a dense window becomes op 9, a
    rank-1 PSF at a factor op 11 under the DCT prior and op 10 under the identity prior or with a PSF that is not rank-1."""
    from types import SimpleNamespace as NS
    from free_hunch_amd import conditioning_mechanisms as cm
    z = torch.zeros(4, dtype=torch.float64)

    def cov(use_dct):
        rep = NS(D=z, r=z, M_dev=torch.zeros(1, 8, dtype=torch.float64))
        return NS(use_dct=use_dct, data_dim=3 * S * S, famC=NS(m=0, B=z), C=rep, device=torch.device("cpu"))

    m, m16 = noise_map_n(S), noise_map_n(16)
    motion = np.zeros((9, 9))
    motion[4, :] = 1.0 / 9
    motion[2, 3] = 0.01
    cases = [(_wb(noise_map=m, kernel=motion), True, 8), (_wb(noise_map=m), False, 8), (_wb(noise_map=m, kernel=disk_psf()), True, 9),
             (_wsr(noise_map=m16), True, 11), (_wsr(noise_map=m16), False, 10),
             (_wsr(noise_map=m16, kernel=disk_psf(radius=4.0, size=9)), True, 10)]
    for op, use_dct, want in cases:
        p, keep = cm._problem(op, cov(use_dct), cm._solver_sigma_y2(op))
        assert p.op == want and p.sigma_y2 == 1.0 and p.mask == keep[-1].data_ptr() and torch.equal(keep[-1], op.weights)
        assert p.stride == (4 if want >= 10 else 1) and bool(p.fold_fwd_w) == (want == 11 or (want == 8 and use_dct and op.taps.sep is not None))


def test_cli_flags(tmp_path):
    from free_hunch_amd.config import load_config
    base = [f"--outdir={tmp_path}", "--kernel_path=psf.npy"]
    o = load_config(base + ["--operator_name=weighted_blur", "--noise_map_path=map.npy"])
    assert o.noise_map_path == "map.npy" and o.noise_gain is None and o.noise_read_sigma is None
    o = load_config(base + ["--operator_name=weighted_sr", "--scale_factor=4", "--noise_gain=0.01", "--noise_read_sigma=0.02"])
    assert (o.noise_gain, o.noise_read_sigma, o.scale_factor, o.noise_map_path) == (0.01, 0.02, 4, "")
    for name in ("weighted_blur", "weighted_sr"):
        with pytest.raises(SystemExit, match="kernel_path"):
            load_config([f"--outdir={tmp_path}", f"--operator_name={name}", "--noise_map_path=map.npy"])
        with pytest.raises(SystemExit, match="noise map"):  # neither form
            load_config(base + [f"--operator_name={name}"])
        with pytest.raises(SystemExit, match="not both"):
            load_config(base + [f"--operator_name={name}", "--noise_map_path=map.npy", "--noise_gain=0.01", "--noise_read_sigma=0.01"])
        for half in ("--noise_gain=0.01", "--noise_read_sigma=0.01"):
            with pytest.raises(SystemExit, match="go together"):
                load_config(base + [f"--operator_name={name}", half])
        with pytest.raises(SystemExit, match="masked_blur"):  # the mask flags stay masked_blur's
            load_config(base + [f"--operator_name={name}", "--noise_map_path=map.npy", "--mask_border=3"])
    for flag in ("--noise_map_path=map.npy", "--noise_gain=0.01", "--noise_read_sigma=0.01"):
        for other in (["--operator_name=custom_blur"] + base[1:], ["--operator_name=gaussian_blur"],
                      ["--operator_name=masked_blur", "--mask_border=3"] + base[1:], ["--operator_name=custom_sr"] + base[1:]):
            with pytest.raises(SystemExit, match="weighted_blur / weighted_sr"):
                load_config([f"--outdir={tmp_path}", flag] + other)
    with pytest.raises(SystemExit, match="kernel_path"):  # --kernel_path stays refused elsewhere
        load_config([f"--outdir={tmp_path}", "--operator_name=inpainting", "--kernel_path=psf.npy"])
