"""Host-side checks of the colorization and denoising operators: the registry, shapes, weights, the solver's operator
codes and the CLI flags.  Nothing here touches the library or a GPU: both constructors must work on device="cpu"."""
import pytest
import torch


def _get(name, **kw):
    from free_hunch_amd.measurements import get_operator
    return get_operator(name=name, device="cpu", sigma_s=0.05, in_shape=(1, 3, 64, 64), kernel_size=61, intensity=1.0,
                        scale_factor=4, mask_opt={"mask_type": "random", "image_size": 64}, **kw)


def test_registry_resolves_both_names_on_cpu():
    from free_hunch_amd import _lib
    from free_hunch_amd.measurements import ColorizationOperator, DenoiseOperator
    before = dict(_lib.Context._cache)
    col, den = _get("colorization"), _get("noise")
    assert isinstance(col, ColorizationOperator) and col.name == "colorization"
    assert isinstance(den, DenoiseOperator) and den.name == "noise"
    assert _lib.Context._cache == before  # no context was created: the constructors call nothing in the library
    assert col.device == torch.device("cpu") and den.device == torch.device("cpu")
    assert float(col.sigma_s) == pytest.approx(0.05) and float(den.sigma_s) == pytest.approx(0.05)


def test_shapes_and_default_weights():
    col, den = _get("colorization"), _get("noise")
    assert tuple(col.in_shape) == (1, 3, 64, 64) and tuple(col.out_shape) == (1, 1, 64, 64)
    assert col.channel_weights == (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)  # the reference's mean(dim=1)
    assert tuple(den.in_shape) == (1, 3, 64, 64) and tuple(den.out_shape) == (1, 3, 64, 64)
    assert tuple(den.mask.shape) == (1, 3, 64, 64) and bool((den.mask == 1).all())
    w = _get("colorization", channel_weights=(0.299, 0.587, 0.114)).channel_weights
    assert w == (0.299, 0.587, 0.114)


def test_denoise_operator_is_the_identity_plus_noise():
    den = _get("noise")
    x = torch.randn(2, 3, 64, 64)
    assert torch.equal(den.forward(x, noiseless=True), x)
    assert torch.equal(den.transpose(x), x) and torch.equal(den.forward_adjoint(x), x)
    y, flat = den.forward(x, flatten=True, noiseless=True)
    assert tuple(flat.shape) == (2, 3 * 64 * 64)
    noisy = den.forward(x)
    assert float((noisy - x).std()) == pytest.approx(0.05, rel=0.05)  # sigma_s * randn over 24576 samples


@pytest.mark.parametrize("bad", [(0.5, 0.5), (0.1, 0.2, 0.3, 0.4), (0.3, float("nan"), 0.3), (0.3, float("inf"), 0.3),
                                 ("a", "b", "c"), 0.3])
def test_bad_channel_weights_are_rejected(bad):
    with pytest.raises(ValueError):
        _get("colorization", channel_weights=bad)


def test_solver_operator_codes():
    from free_hunch_amd.conditioning_mechanisms import _op_code, _sigma_y2
    assert _op_code("colorization") == 3 and _op_code("noise") == 0
    assert _op_code("inpainting") == 0 and _op_code("gaussian_blur") == 1 and _op_code("motion_blur") == 1
    assert _op_code("super_resolution") == 2
    # the clip(min=0.001) rule of blur and inpainting, in float32 like the reference
    assert _sigma_y2(_get("colorization")) == float(torch.tensor([0.05]).float().clip(min=0.001) ** 2)
    col0 = _get("colorization")
    col0.sigma_s = torch.Tensor([0.0])
    assert _sigma_y2(col0) == float(torch.tensor([0.001]).float() ** 2)


def test_cli_config_accepts_both_operator_names(tmp_path):
    from free_hunch_amd.config import load_config
    for name in ("colorization", "noise"):
        o = load_config([f"--outdir={tmp_path}", f"--operator_name={name}"])
        assert o.operator_name == name
        assert _get(o.operator_name).name == name
    assert not hasattr(load_config([f"--outdir={tmp_path}"]), "channel_weights")  # a Python-API option only
