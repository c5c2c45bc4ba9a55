"""bench.py's command line: a plain run prints the headline line only (the legs beside it are behind --full), and
--dump-outputs writes what the timed path returned in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_float32_and_bounded(tmp_path, monkeypatch):
    """The images as float32, unchanged; beyond the size limit a fixed sample of whole images with their indices."""
    import bench
    imgs = torch.randint(0, 256, (5, 3, 16, 16), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    bench.dump_outputs(str(tmp_path / "all"), imgs)
    x = np.load(tmp_path / "all" / "images.npy")
    assert x.dtype == np.float32 and np.array_equal(x, imgs.numpy())
    assert not (tmp_path / "all" / "images_index.npy").exists()

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * x[0].nbytes + 1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), imgs)
    xa, ia = np.load(tmp_path / "a" / "images.npy"), np.load(tmp_path / "a" / "images_index.npy")
    assert xa.dtype == np.float32 and ia.dtype == np.float64 and len(xa) == 2
    assert np.array_equal(xa, imgs.numpy()[ia.astype(np.int64)])
    assert np.array_equal(xa, np.load(tmp_path / "b" / "images.npy"))  # the same sample every time


@pytest.mark.gpu
def test_plain_run_prints_headline_only_and_dumps_last_step(tmp_path):
    """A small plain run: the contract's keys, exactly --steps timed steps, none of the --full legs, and the images of
    the last timed step in DIR/images.npy."""
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0", "--batch", "2",
           "--groups", "1", "--num-steps", "3", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 2 and line["warmup"] == 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * 2 / (2 * line["ms_per_step"] / 1e3)) <= 1e-3 * line["value"]
    assert not [k for k in line if k.startswith("roofline") or k in ("half_split_mode", "cpu_baseline")], sorted(line)
    x = np.load(out / "images.npy")
    assert x.dtype == np.float32 and x.shape == (2, 3, 256, 256)
    assert x.min() >= 0 and x.max() <= 255 and np.array_equal(x, np.round(x)) and x.std() > 0
