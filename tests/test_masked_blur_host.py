"""Host-side checks of `masked_blur` (y = M (B x + n)): the registry, the validation of the mask arguments, how the mask is
broadcast and combined with the border, the solver's op code and the CLI flags.  No GPU: the operators are built on
device="cpu"."""
import os

import numpy as np
import pytest
import torch

from test_custom_psf_host import disk_psf

S = 64


def _masked(**kw):
    from free_hunch_amd.measurements import get_operator
    kw.setdefault("kernel", disk_psf())
    return get_operator(name="masked_blur", device="cpu", sigma_s=0.05, in_shape=(1, 3, S, S), **kw)


def _random_mask(shape, seed=5):
    return (np.random.default_rng(seed).random(shape) >= 0.1).astype(np.float64)


def _band(hy, hx):
    m = np.zeros((1, 3, S, S))
    m[..., hy: S - hy, hx: S - hx] = 1.0
    return torch.from_numpy(m)


def test_registry_has_the_operator():
    from free_hunch_amd.measurements import __OPERATOR__, CustomBlurOperator, MaskedBlurOperator
    assert __OPERATOR__["masked_blur"] is MaskedBlurOperator and issubclass(MaskedBlurOperator, CustomBlurOperator)
    assert __OPERATOR__["custom_blur"] is CustomBlurOperator and CustomBlurOperator.name == "custom_blur"
    op = _masked(mask_border=3)
    assert op.name == "masked_blur" and op.taps.window is not None
    assert tuple(op.get_kernel().shape) == (1, 1, 61, 61) and op.get_kernel().dtype == torch.float32


def test_no_mask_argument_points_to_custom_blur():
    with pytest.raises(ValueError, match="custom_blur"):
        _masked()
    with pytest.raises(ValueError, match="custom_blur"):
        _masked(mask_border=0, mask_path="")


@pytest.mark.parametrize("shape", [(S,), (S, S - 1), (2, S, S), (1, 1, S, S), (2, 3, S, S), (S // 2, S // 2)])
def test_wrong_mask_shapes_are_rejected(shape):
    with pytest.raises(ValueError, match="shape"):
        _masked(mask=np.ones(shape))


def test_bad_mask_entries_are_rejected(tmp_path):
    m = np.ones((S, S))
    for value, word in ((0.5, "other than 0 and 1"), (2.0, "other than 0 and 1"), (-1.0, "other than 0 and 1"),
                        (np.nan, "non-finite"), (np.inf, "non-finite")):
        bad = m.copy()
        bad[3, 4] = value
        with pytest.raises(ValueError, match=word):
            _masked(mask=bad)
        with pytest.raises(ValueError, match=word):
            _masked(mask=torch.from_numpy(bad))
    with pytest.raises(ValueError, match="all zero"):
        _masked(mask=np.zeros((S, S)))
    inner = np.zeros((S, S))
    inner[:5] = 1.0  # the array keeps only rows that the border drops
    with pytest.raises(ValueError, match="all zero"):
        _masked(mask=inner, mask_border=5)
    np.save(tmp_path / "m.npy", m)
    with pytest.raises(ValueError, match="not both"):
        _masked(mask=m, mask_path=str(tmp_path / "m.npy"))


@pytest.mark.parametrize("n", [S // 2, S // 2 + 1, S])
def test_a_border_that_leaves_nothing_is_rejected(n):
    with pytest.raises(ValueError, match="border"):
        _masked(mask_border=n)
    assert float(_masked(mask_border=S // 2 - 1).mask.sum()) == 3 * 2 * 2


def test_negative_borders_other_than_the_psf_reach_are_rejected():
    with pytest.raises(ValueError, match="mask_border"):
        _masked(mask_border=-2)


def test_psf_errors_are_those_of_custom_blur():
    with pytest.raises(ValueError, match="PSF"):
        _masked(kernel=np.zeros((5, 5)), mask_border=1)
    with pytest.raises(ValueError):
        _masked(kernel=None, mask_border=1)


def test_mask_shapes_broadcast_to_1_3_S_S():
    m2 = _random_mask((S, S))
    m3 = _random_mask((3, S, S), 6)
    for given, want in ((m2, np.broadcast_to(m2, (1, 3, S, S))), (m3, m3[None]), (m3[None], m3[None]),
                        (torch.from_numpy(m2), np.broadcast_to(m2, (1, 3, S, S))), (m3.astype(np.float32), m3[None]),
                        (m2.astype(bool), np.broadcast_to(m2, (1, 3, S, S))), (m2.astype(np.uint8), np.broadcast_to(m2, (1, 3, S, S)))):
        op = _masked(mask=given)
        assert tuple(op.mask.shape) == (1, 3, S, S) and op.mask.dtype == torch.float64
        assert np.array_equal(op.mask.numpy(), want)


def test_border_and_array_multiply():
    m2 = _random_mask((S, S))
    op = _masked(mask=m2, mask_border=8)
    want = np.broadcast_to(m2, (1, 3, S, S)) * _band(8, 8).numpy()
    assert np.array_equal(op.mask.numpy(), want) and op.mask_border == (8, 8)
    assert torch.equal(_masked(mask_border=8).mask, _band(8, 8))
    assert torch.equal(_masked(mask=np.ones((S, S)), mask_border=0).mask, torch.ones(1, 3, S, S, dtype=torch.float64))


def test_border_minus_one_is_the_psf_reach():
    from free_hunch_amd.measurements import KERNEL_DIR
    disk = _masked(mask_border=-1)
    assert (disk.taps.hy, disk.taps.hx) == (20, 20) and disk.mask_border == (20, 20)
    assert torch.equal(disk.mask, _band(20, 20))
    motion = _masked(kernel=None, kernel_path=os.path.join(KERNEL_DIR, "motion_ks61_std0.5.npy"), mask_border=-1)
    k = np.load(os.path.join(KERNEL_DIR, "motion_ks61_std0.5.npy")).astype(np.float32)
    ys, xs = np.nonzero(k)
    hy, hx = int(np.abs(ys - 30).max()), int(np.abs(xs - 30).max())
    assert hy != hx and (motion.taps.hy, motion.taps.hx) == (hy, hx)
    assert torch.equal(motion.mask, _band(hy, hx))


def test_npy_mask_and_array_mask_give_equal_operators(tmp_path):
    for shape in ((S, S), (3, S, S), (1, 3, S, S)):
        m = _random_mask(shape, 7)
        np.save(tmp_path / "m.npy", m)
        a, b = _masked(mask=m, mask_border=2), _masked(mask_path=str(tmp_path / "m.npy"), mask_border=2)
        assert torch.equal(a.mask, b.mask) and torch.equal(a.taps.kernel, b.taps.kernel)
        assert torch.equal(a.taps.window[0], b.taps.window[0]) and float(a.sigma_s) == float(b.sigma_s)


def test_solver_names_the_operator():
    from free_hunch_amd.conditioning_mechanisms import _BAD_OPERATOR, _op_code, _sigma_y2
    assert _op_code("masked_blur") == 5 and _op_code("custom_blur") == 1
    assert "masked_blur" in _BAD_OPERATOR and "custom_blur" in _BAD_OPERATOR
    assert _sigma_y2(_masked(mask_border=1)) == float(torch.tensor([0.05]).float().clip(min=0.001) ** 2)  # the blur rule


def test_config_keys_and_cli_messages(tmp_path):
    from free_hunch_amd.config import SCHEMA, load_config
    assert SCHEMA["mask_path"] == (str, "") and SCHEMA["mask_border"] == (int, 0)
    o = load_config([f"--outdir={tmp_path}"])
    assert o.mask_path == "" and o.mask_border == 0
    base = [f"--outdir={tmp_path}", "--operator_name=masked_blur"]
    psf, mask = f"--kernel_path={tmp_path}/psf.npy", f"--mask_path={tmp_path}/m.npy"
    o = load_config(base + [psf, mask, "--mask_border=-1"])
    assert o.operator_name == "masked_blur" and o.mask_path == f"{tmp_path}/m.npy" and o.mask_border == -1
    assert load_config(base + [psf, "--mask_border=4"]).mask_border == 4
    assert load_config(base + [psf, mask]).mask_border == 0
    with pytest.raises(SystemExit, match="kernel_path"):  # masked_blur without a PSF
        load_config(base + [mask])
    with pytest.raises(SystemExit, match="mask"):         # masked_blur without either mask flag
        load_config(base + [psf])
    for other in ("custom_blur", "gaussian_blur"):        # a mask flag with another operator
        extra = [psf] if other == "custom_blur" else []
        with pytest.raises(SystemExit, match="masked_blur"):
            load_config([f"--outdir={tmp_path}", f"--operator_name={other}", mask] + extra)
        with pytest.raises(SystemExit, match="masked_blur"):
            load_config([f"--outdir={tmp_path}", f"--operator_name={other}", "--mask_border=3"] + extra)
    with pytest.raises(SystemExit, match="kernel_path"):  # --kernel_path stays refused elsewhere
        load_config([f"--outdir={tmp_path}", "--operator_name=motion_blur", psf])
