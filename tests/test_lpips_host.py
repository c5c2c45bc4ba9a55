"""Host-side checks of the LPIPS feature (no GPU): weight files, packing, flags, and the properties of the PyTorch
restatement (tests/_lpips_restatement.py) that the device tests measure against.  The lpips package is not installed
here: parity with the package itself is unpinned at that boundary."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from free_hunch_amd import lpips  # noqa: E402
import _lpips_restatement as R  # noqa: E402


def test_structure_constants():
    assert lpips.VGG_CONVS == R.CONVS and lpips.VGG_TAPS == R.TAPS and lpips.VGG_POOLS == R.POOLS
    assert lpips.SHIFT == R.SHIFT and lpips.SCALE == R.SCALE
    assert lpips.TAP_CHANNELS == (64, 128, 256, 512, 512)


def test_save_load_round_trip_is_exact(tmp_path):
    state = lpips.seeded_weights(0)
    assert len(state) == 26 + 5
    vp, lp = str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth")
    lpips.save_weights(state, vp, lp)
    vgg, lin = torch.load(vp, weights_only=True), torch.load(lp, weights_only=True)
    assert sorted(vgg) == sorted(k for k in state if k.startswith("features."))
    assert sorted(lin) == [f"lin{t}.model.1.weight" for t in range(5)] and tuple(lin["lin2.model.1.weight"].shape) == (1, 256, 1, 1)
    back = lpips.load_weights(vp, lp)
    assert sorted(back) == sorted(state)
    for k in state:
        assert back[k].dtype == torch.float32 and torch.equal(back[k], state[k]), k
    again = lpips.seeded_weights(0)
    assert all(torch.equal(again[k], state[k]) for k in state)
    assert not torch.equal(lpips.seeded_weights(1)["features.0.weight"], state["features.0.weight"])


def test_seeded_weights_follow_the_stated_distributions():
    state = lpips.seeded_weights(0)
    w = state["features.17.weight"]
    assert tuple(w.shape) == (512, 256, 3, 3) and abs(float(w.std()) / (2.0 / (256 * 9)) ** 0.5 - 1) < 0.01
    assert abs(float(state["features.28.bias"].std()) / 0.05 - 1) < 0.15
    for t, c in enumerate(lpips.TAP_CHANNELS):
        lin = state[f"lin{t}.model.1.weight"]
        assert float(lin.min()) >= 0 and float(lin.max()) < 2.0 / c


def test_load_ignores_classifier_and_accepts_both_lin_spellings(tmp_path):
    state = lpips.seeded_weights(3)
    vgg = {k: v for k, v in state.items() if k.startswith("features.")}
    vgg["classifier.0.weight"], vgg["classifier.0.bias"] = torch.zeros(8, 8), torch.zeros(8)
    lin = {f"lins.{t}.model.1.weight": state[f"lin{t}.model.1.weight"] for t in range(5)}
    vp, lp = str(tmp_path / "v.pth"), str(tmp_path / "l.pth")
    torch.save(vgg, vp)
    torch.save(lin, lp)
    back = lpips.load_weights(vp, lp)
    assert sorted(back) == sorted(state) and all(torch.equal(back[k], state[k]) for k in state)


@pytest.mark.parametrize("which,key,how", [("vgg", "features.12.bias", "missing"), ("vgg", "features.5.weight", "shape"),
                                           ("lin", "lin3.model.1.weight", "missing"), ("lin", "lin1.model.1.weight", "shape")])
def test_bad_files_raise_value_error_naming_the_key(tmp_path, which, key, how):
    state = lpips.seeded_weights(0)
    if how == "missing":
        del state[key]
    else:
        state[key] = state[key][..., :1].clone() if which == "vgg" else state[key][:, :-1].clone()
    vp, lp = str(tmp_path / "v.pth"), str(tmp_path / "l.pth")
    lpips.save_weights(state, vp, lp)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        lpips.load_weights(vp, lp)


def test_missing_file_raises(tmp_path):
    vp, lp = str(tmp_path / "v.pth"), str(tmp_path / "l.pth")
    lpips.save_weights(lpips.seeded_weights(0), vp, lp)
    with pytest.raises(FileNotFoundError):
        lpips.load_weights(vp, str(tmp_path / "nope.pth"))


def test_first_layer_packing_pads_input_channels_with_zeros():
    state = lpips.seeded_weights(0)
    w, b = state["features.0.weight"], state["features.0.bias"]
    c = lpips.pack_conv(w, b)
    assert (c.ci, c.ci_p, c.co) == (3, 32, 64) and tuple(c.wf.shape) == (64, 9, 32)
    assert torch.count_nonzero(c.wf[:, :, 3:]) == 0
    assert torch.equal(c.wf[:, :, :3], w.permute(0, 2, 3, 1).reshape(64, 9, 3)) and torch.equal(c.b, b)
    # the exact split: three bf16 planes [3][taps][K/32][rows][32] that add up to the fp32 weight
    planes = c.wx_f.float().sum(0)  # [9][1][64][32]
    assert torch.equal(planes.permute(2, 0, 1, 3).reshape(64, 9, 32), c.wf)
    assert c.wd is None and c.wx_d is None  # no backward copies


def test_prep_table_is_the_float64_formula_rounded_once():
    tab = lpips.prep_table()
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (3, 256)
    v = torch.arange(256, dtype=torch.float64)
    for c in range(3):
        want = (((v / 255.0 - 0.5) * 2.0 - R.SHIFT[c]) / R.SCALE[c]).to(torch.float32)
        assert torch.equal(tab[c], want)


def test_config_defaults_and_pairing():
    from free_hunch_amd.config import load_config
    o = load_config(["--outdir=x"])
    assert o.lpips_vgg_path == "" and o.lpips_lin_path == ""
    o = load_config(["--outdir=x", "--lpips_vgg_path=a.pth", "--lpips_lin_path=b.pth"])
    assert (o.lpips_vgg_path, o.lpips_lin_path) == ("a.pth", "b.pth")
    for arg in ("--lpips_vgg_path=a.pth", "--lpips_lin_path=b.pth"):
        with pytest.raises(SystemExit):
            load_config(["--outdir=x", arg])


def test_cpu_tensors_are_refused():
    from free_hunch_amd import _lib
    from free_hunch_amd.pipeline import lpips_u8
    a = torch.zeros(1, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(_lib.FhError):
        lpips_u8(a, a, None)
    with pytest.raises(_lib.FhError):
        lpips.LPIPS(lpips.seeded_weights(0), "cpu")


def test_restatement_is_a_sane_distance():
    """d(a, a) == 0, d(a, b) == d(b, a), strictly increasing in the noise level"""
    from bench import smooth_images
    state = lpips.seeded_weights(0)
    a = smooth_images(4, 64, 7)
    assert torch.count_nonzero(R.lpips_layers(state, a, a)) == 0
    prev = torch.zeros(4, dtype=torch.float64)
    for std in R.NOISE_STD:
        b = R.noisy(a, std)
        d_ab, d_ba = R.lpips_layers(state, a, b), R.lpips_layers(state, b, a)
        assert d_ab.dtype == torch.float64 and tuple(d_ab.shape) == (4, 5)
        assert torch.equal(d_ab, d_ba)
        d = d_ab.sum(1)
        assert bool((d > prev).all()), (std, d, prev)
        prev = d
