"""--posterior_samples through the CLI on the GPU: one run shaped like tests/test_cli_gpu.py (one 256 x 256 PNG, seeded
FFHQ-architecture weights) with three members in one lock-step batch, and the same run without the flag."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_DIRS = ("posterior_samples", "posterior_mean", "posterior_std")
NEW_LINES = ("posterior_samples:", "PSNR(mean):", "SSIM(mean):", "spread:", "skill:", "spread/skill:", "coverage(1 sigma):",
             "coverage(2 sigma):")


def test_cli_posterior_samples(tmp_path):
    import PIL.Image
    sys.path.insert(0, ROOT)
    from bench import smooth_images
    import generate_conditional as gc
    data = tmp_path / "data"
    data.mkdir()
    PIL.Image.fromarray(smooth_images(1, 256, 7)[0].permute(1, 2, 0).numpy(), "RGB").save(data / "img00000000.png")
    flags = [f"--dataset_path={data}", "--synthetic_weights=ffhq", "--num_steps=2", "--total_images=1", "--max_batch_size=3",
             "--operator_name=inpainting", "--inpainting_prob_lower=0.6", "--inpainting_prob_upper=0.8", "--solver=euler",
             "--conditioning_mechanism=online_covariance", "--image_base_covariance=dct_diagonal"]
    out = tmp_path / "out"
    t0 = time.perf_counter()
    gc.main([f"--outdir={out}", "--posterior_samples=3"] + flags)
    print(f"CLI run with --posterior_samples=3: {time.perf_counter() - t0:.1f} s", flush=True)
    load = lambda *p: np.asarray(PIL.Image.open(os.path.join(out, *p)))
    for sub in ("images", "cond_images", "forward_images", "posterior_mean"):
        assert sorted(os.listdir(out / sub)) == ["000000_000000.png"], sub
    assert sorted(os.listdir(out / "posterior_samples")) == [f"000000_000000_{k:03d}.png" for k in range(3)]
    assert sorted(os.listdir(out / "posterior_std")) == ["000000_000000.npy", "000000_000000.png"]
    samples = [load("posterior_samples", f"000000_000000_{k:03d}.png") for k in range(3)]
    assert all(s.shape == (256, 256, 3) and s.dtype == np.uint8 for s in samples)
    assert all(not np.array_equal(samples[a], samples[b]) for a in range(3) for b in range(a + 1, 3))
    assert np.array_equal(load("images", "000000_000000.png"), samples[0])
    mean = load("posterior_mean", "000000_000000.png").astype(np.float64)
    assert np.abs(mean - np.mean([s.astype(np.float64) for s in samples], axis=0)).max() <= 1.0 + 1e-9
    std = np.load(out / "posterior_std" / "000000_000000.npy")
    assert std.shape == (3, 256, 256) and std.dtype == np.float32 and np.isfinite(std).all() and std.min() >= 0 and std.max() > 0
    std_png = load("posterior_std", "000000_000000.png")
    assert np.array_equal(std_png, np.minimum(255, np.round(4.0 * std)).astype(np.uint8).transpose(1, 2, 0))
    lines = open(out / "results.txt").read().splitlines()
    assert [l.split(":")[0] for l in lines[:3]] == ["PSNR", "SSIM", "images"] and lines[2] == "images: 1"
    assert [l.split(": ")[0] + ":" for l in lines[3:]] == list(NEW_LINES)
    value = {l.split(": ")[0]: float(l.split(": ")[1]) for l in lines}
    assert lines[3] == "posterior_samples: 3"
    assert 0.0 <= value["coverage(1 sigma)"] <= value["coverage(2 sigma)"] <= 1.0
    assert value["spread"] > 0 and value["skill"] > 0
    assert abs(value["spread/skill"] - np.sqrt(4.0 / 3.0) * value["spread"] / value["skill"]) < 1e-2 * value["spread/skill"] + 1e-3

    # the flag absent: today's outputs, none of the new directories or lines - and member 0 above was this run's image
    plain = tmp_path / "plain"
    t0 = time.perf_counter()
    gc.main([f"--outdir={plain}"] + flags)
    print(f"CLI run without the flag: {time.perf_counter() - t0:.1f} s", flush=True)
    assert sorted(os.listdir(plain)) == ["cond_images", "forward_images", "images", "results.txt"]
    text = open(plain / "results.txt").read()
    assert not any(k in text for k in NEW_LINES) and [l.split(":")[0] for l in text.splitlines()] == ["PSNR", "SSIM", "images"]
    assert np.array_equal(np.asarray(PIL.Image.open(plain / "forward_images" / "000000_000000.png")),
                          load("forward_images", "000000_000000.png"))  # the same measurement
