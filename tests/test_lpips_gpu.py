"""LPIPS on the device against the PyTorch restatement of the published forward pass (tests/_lpips_restatement.py).
The lpips package, torchvision and the published weights are not available here, so the kernels are pinned to that
restatement with `seeded_weights(0)`: parity with the package itself is unpinned at that boundary.

The bound of the whole-metric comparison is not a constant: float32 PyTorch is the arithmetic the reference runs LPIPS in,
so `e32 = max relative |d_float32 - d_float64|` over ALL cases is measured on the CPU and the device has to stay within
8 x e32 of the float64 evaluation (one e32 for the totals, one per layer)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MARGIN = 8.0


def _rel(x, ref):
    return float(((x - ref).abs() / ref.abs()).max())


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def state():
    from free_hunch_amd import lpips
    return lpips.seeded_weights(0)


@pytest.fixture(scope="module")
def model(dev, state):
    from free_hunch_amd import lpips
    return lpips.LPIPS(state, dev)


def _cases():
    """(name, a, b): four shapes x (three noise levels + one different-image case)"""
    from bench import smooth_images
    import _lpips_restatement as R
    bases = [("64x64", smooth_images(4, 64, 7)), ("256x256", smooth_images(2, 256, 7)),
             ("48x80", smooth_images(3, 80, 7)[:, :, :48, :80].contiguous()),
             ("50x36", smooth_images(1, 50, 7)[:, :, :50, :36].contiguous())]
    out = []
    for name, a in bases:
        for std in R.NOISE_STD:
            out.append((f"{name} noise {std:g}", a, R.noisy(a, std)))
        # a different image: the batch rolled by one (a single image is rolled in space instead)
        other = torch.roll(a, 1, 0) if a.shape[0] > 1 else torch.roll(a, (a.shape[2] // 2, a.shape[3] // 2), (2, 3))
        out.append((f"{name} other image", a, other.contiguous()))
    return out


@pytest.fixture(scope="module")
def measured(state):
    """float64 and float32 CPU evaluations of every case and the bounds that follow from them"""
    import _lpips_restatement as R
    rows = []
    for name, a, b in _cases():
        d64 = R.lpips_layers(state, a, b, torch.float64)
        d32 = R.lpips_layers(state, a, b, torch.float32).double()
        rows.append((name, a, b, d64, d32))
    e32_total = max(_rel(d32.sum(1), d64.sum(1)) for _n, _a, _b, d64, d32 in rows)
    e32_layer = [max(_rel(d32[:, t], d64[:, t]) for _n, _a, _b, d64, d32 in rows) for t in range(5)]
    print(f"\nLPIPS float32-vs-float64 on the CPU: totals e32 = {e32_total:.3e}, per layer "
          + ", ".join(f"{e:.3e}" for e in e32_layer))
    return rows, e32_total, e32_layer


# ---------------------------------------------------------------------------------------------- the small kernels
@pytest.mark.parametrize("shape", [(2, 16, 16), (3, 37, 50), (1, 256, 256)])
def test_prep_is_bitwise_the_table(dev, model, shape):
    import _lpips_restatement as R
    n, H, W = shape
    g = torch.Generator().manual_seed(11)
    a = torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, generator=g)
    b = torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, generator=g)
    x = model._prep(a.to(dev), b.to(dev)).cpu()
    assert tuple(x.shape) == (2 * n, H, W, 32) and torch.count_nonzero(x[..., 3:]) == 0
    v = torch.cat([a, b]).to(torch.float64)
    want = ((v / 255.0 - 0.5) * 2.0 - torch.tensor(R.SHIFT, dtype=torch.float64).view(1, 3, 1, 1)) \
        / torch.tensor(R.SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    assert torch.equal(x[..., :3], want.to(torch.float32).permute(0, 2, 3, 1))


@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (3, 37, 51, 128), (1, 7, 9, 512), (2, 50, 36, 64)])
def test_relu_and_relu_pool_are_bitwise_pytorch(dev, model, shape):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, generator=g)
    pooled = model._relu_pool(x.to(dev)).cpu()
    want = F.max_pool2d(F.relu(x).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert pooled.shape == want.shape and torch.equal(pooled, want)
    y = x.to(dev).clone()
    assert torch.equal(model._relu(y).cpu(), F.relu(x))


@pytest.mark.parametrize("n,H,W,C", [(2, 37, 50, 64), (3, 16, 16, 128), (2, 37, 50, 256), (2, 16, 16, 512), (1, 3, 2, 512),
                                     (2, 256, 256, 64), (1, 37, 50, 128), (2, 9, 12, 512)])
def test_tap_kernel_against_float64(dev, model, n, H, W, C):
    """seeded float32 features with negative entries (ReLU on read) and pixels that are all zero (or all negative) in one or
    both halves; <= 1e-10 relative to the float64 PyTorch evaluation of the same float32 inputs (the bar test_metrics.py uses
    for its float64 SSIM sums)"""
    import _lpips_restatement as R
    g = torch.Generator().manual_seed(C + H)
    feat = torch.randn(2 * n, H, W, C, generator=g) + 0.3
    feat[0, 0, 0] = 0.0                 # zero in a only
    feat[n, 1, 1] = 0.0                 # zero in b only
    feat[0, 2, 1] = 0.0                 # zero in both
    feat[n, 2, 1] = -feat[n, 2, 1].abs()  # ... through the ReLU
    feat[n - 1, H - 1, W - 1] = -1.0    # last pixel of the a half
    lin = torch.rand(C, generator=g) * (2.0 / C)
    got = model.tap(feat.to(dev), lin.to(dev)).cpu()
    want = R.tap_value(feat, lin)
    again = model.tap(feat.to(dev), lin.to(dev)).cpu()
    rel = _rel(got, want)
    print(f"\ntap kernel n={n} {H}x{W} C={C}: max relative difference {rel:.3e}")
    assert torch.equal(got, again)
    assert rel <= 1e-10


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_tap_kernel_of_identical_halves_is_exactly_zero(dev, model, C):
    g = torch.Generator().manual_seed(C)
    half = torch.randn(2, 19, 23, C, generator=g)
    got = model.tap(torch.cat([half, half]).to(dev), (torch.rand(C, generator=g) * (2.0 / C)).to(dev))
    assert torch.count_nonzero(got) == 0, got


def test_tap_kernel_rejects_other_channel_counts(dev, model):
    from free_hunch_amd import _lib
    feat = torch.zeros(2, 4, 4, 96, device=dev)
    with pytest.raises(_lib.FhError):
        model.tap(feat, torch.zeros(96, device=dev))


# ---------------------------------------------------------------------------------------------- the whole metric
def test_whole_metric_within_the_float32_bound(dev, model, measured):
    """Measured on MI355X (profiles/lpips.md): see the figures printed by this test."""
    rows, e32_total, e32_layer = measured
    worst_total, worst_layer = 0.0, [0.0] * 5
    for name, a, b, d64, _d32 in rows:
        got = model(a.to(dev), b.to(dev), per_layer=True).cpu()
        tot = model(a.to(dev), b.to(dev)).cpu()
        assert got.dtype == torch.float64 and tuple(got.shape) == (a.shape[0], 5) and tuple(tot.shape) == (a.shape[0],)
        assert torch.equal(tot, (((got[:, 0] + got[:, 1]) + got[:, 2]) + got[:, 3]) + got[:, 4])  # summed in tap order
        r_tot = _rel(tot, d64.sum(1))
        r_lay = [_rel(got[:, t], d64[:, t]) for t in range(5)]
        print(f"{name}: d = {float(d64.sum(1).min()):.3e} .. {float(d64.sum(1).max()):.3e}, device vs float64 total "
              f"{r_tot:.3e}, per layer " + ", ".join(f"{r:.3e}" for r in r_lay))
        worst_total = max(worst_total, r_tot)
        worst_layer = [max(w, r) for w, r in zip(worst_layer, r_lay)]
    print(f"device vs float64: totals {worst_total:.3e} (bound {MARGIN * e32_total:.3e}), per layer "
          + ", ".join(f"{w:.3e} ({MARGIN * e:.3e})" for w, e in zip(worst_layer, e32_layer)))
    assert worst_total <= MARGIN * e32_total
    for t in range(5):
        assert worst_layer[t] <= MARGIN * e32_layer[t], (t, worst_layer[t], e32_layer[t])


def test_identity_determinism_symmetry_and_batching(dev, model, measured):
    rows, e32_total, _ = measured
    bound = MARGIN * e32_total
    for name, a, b, d64, _d32 in rows:
        if "noise 8" not in name and "other" not in name:
            continue
        A, B = a.to(dev), b.to(dev)
        # both halves of the batch run the same code on the same bits
        assert torch.count_nonzero(model(A, A, per_layer=True)) == 0, name
        assert torch.count_nonzero(model(B, B)) == 0, name
        d1, d2 = model(A, B, per_layer=True), model(A, B, per_layer=True)
        assert torch.equal(d1, d2), name
        d_ab, d_ba = d1.sum(1).cpu(), model(B, A).cpu()
        ref = d64.sum(1)
        single = torch.cat([model(A[i: i + 1], B[i: i + 1]) for i in range(A.shape[0])]).cpu()
        print(f"{name}: (a,b) vs (b,a) {_rel(d_ab, d_ba):.3e}, batch vs one-by-one {_rel(d_ab, single):.3e}")
        # the two orders and the two batchings agree with each other within the bound, and each with the float64 value
        assert _rel(d_ab, d_ba) <= bound and _rel(d_ba, d_ab) <= bound, name
        assert _rel(d_ab, single) <= bound and _rel(single, d_ab) <= bound, name
        assert _rel(d_ab, ref) <= bound and _rel(d_ba, ref) <= bound and _rel(single, ref) <= bound, name


def test_more_pairs_than_one_pass(dev, model):
    """N > 8 runs in passes of at most 8 pairs; every pair gets the value it gets alone within float32 noise"""
    from bench import smooth_images
    import _lpips_restatement as R
    a = smooth_images(11, 32, 5)
    b = R.noisy(a, 8.0)
    d = model(a.to(dev), b.to(dev)).cpu()
    assert tuple(d.shape) == (11,) and bool((d > 0).all())
    tail = model(a[8:].to(dev), b[8:].to(dev)).cpu()
    assert torch.equal(d[8:], tail)  # the second pass IS that call


def test_precision_mode_is_isolated_and_restored(dev, model):
    from bench import smooth_images
    from free_hunch_amd import _lib
    import _lpips_restatement as R
    lib = _lib.load()
    a = smooth_images(2, 64, 7)
    A, B = a.to(dev), R.noisy(a, 8.0).to(dev)
    assert lib.fh_unet_get_precision() == 0
    d0 = model(A, B, per_layer=True)
    try:
        for mode in (3, 1, 4):
            assert lib.fh_unet_set_precision(mode) == 0
            d = model(A, B, per_layer=True)
            assert lib.fh_unet_get_precision() == mode
            assert torch.equal(d, d0), mode
    finally:
        lib.fh_unet_set_precision(0)
    assert lib.fh_unet_get_precision() == 0
    assert lib.fh_unet_set_precision(5) != 0 and lib.fh_unet_get_precision() == 0


def test_malformed_inputs_are_refused_by_name(dev, model):
    ok = torch.zeros(2, 3, 16, 16, dtype=torch.uint8, device=dev)
    for bad in (ok.float(), ok[:, :2], ok[:, :, :15], ok[:, :, :, :15], ok[0]):
        with pytest.raises(ValueError, match="LPIPS takes"):
            model(ok, bad)
        with pytest.raises(ValueError, match="LPIPS takes"):
            model(bad, bad)
    with pytest.raises(ValueError, match="LPIPS takes"):
        model(ok, ok[:1])  # two batch sizes
    with pytest.raises(ValueError, match="tap"):
        model.tap(torch.zeros(3, 4, 4, 64, device=dev), model.lins[0])          # odd batch: no two halves
    with pytest.raises(ValueError, match="tap"):
        model.tap(torch.zeros(2, 4, 4, 64, device=dev), model.lins[1])          # 128 weights for 64 channels
    with pytest.raises(ValueError, match="tap"):
        model.tap(torch.zeros(2, 4, 4, 64, device=dev, dtype=torch.float64), model.lins[0])


def test_cpu_inputs_are_refused(dev, model):
    from free_hunch_amd import _lib
    from free_hunch_amd.pipeline import lpips_u8
    a = torch.zeros(1, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(_lib.FhError):
        model(a, a)
    with pytest.raises(_lib.FhError):
        lpips_u8(a, a.to(dev), model)


# ---------------------------------------------------------------------------------------------- the CLI
def _cli_data(tmp_path):
    import PIL.Image
    from bench import smooth_images
    data = tmp_path / "data"
    data.mkdir()
    for i, im in enumerate(smooth_images(2, 256, 7)):
        PIL.Image.fromarray(im.permute(1, 2, 0).numpy(), "RGB").save(data / f"img{i:08d}.png")
    return data


def _cli_args(out, data):
    return [f"--outdir={out}", f"--dataset_path={data}", "--synthetic_weights=ffhq", "--num_steps=3", "--total_images=2",
            "--max_batch_size=2", "--operator_name=inpainting", "--inpainting_prob_lower=0.6", "--inpainting_prob_upper=0.8",
            "--solver=euler", "--conditioning_mechanism=online_covariance", "--image_base_covariance=dct_diagonal"]


def test_cli_reports_lpips(tmp_path, dev, state, model):
    import numpy as np
    import PIL.Image
    import generate_conditional as gc
    from free_hunch_amd import lpips
    from free_hunch_amd.pipeline import lpips_u8
    data = _cli_data(tmp_path)
    vp, lp = str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth")
    lpips.save_weights(state, vp, lp)

    # a missing file stops the run before anything is sampled or written
    out0 = tmp_path / "out_missing"
    with pytest.raises(FileNotFoundError):
        gc.main(_cli_args(out0, data) + [f"--lpips_vgg_path={vp}", f"--lpips_lin_path={tmp_path / 'nope.pth'}"])
    assert not out0.exists() or os.listdir(out0) == []

    out = tmp_path / "out"
    gc.main(_cli_args(out, data) + [f"--lpips_vgg_path={vp}", f"--lpips_lin_path={lp}"])
    lines = open(out / "results.txt").read().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["PSNR", "SSIM", "LPIPS", "images"], lines
    names = sorted(os.listdir(out / "images"))
    assert names == ["000000_000000.png", "000001_000000.png"]
    load = lambda sub: torch.from_numpy(np.stack([np.asarray(PIL.Image.open(out / sub / n).convert("RGB")) for n in names])
                                        ).permute(0, 3, 1, 2).contiguous().to(dev)
    want = float(lpips_u8(load("images"), load("cond_images"), model).mean())
    assert want > 0
    assert lines[2] == f"LPIPS: {want:.4f}", (lines[2], want)

    # without the flags: today's three lines
    out2 = tmp_path / "out_plain"
    gc.main(_cli_args(out2, data))
    lines2 = open(out2 / "results.txt").read().splitlines()
    assert [ln.split(":")[0] for ln in lines2] == ["PSNR", "SSIM", "images"], lines2
    assert lines2[2] == lines[3]
