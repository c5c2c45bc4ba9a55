"""Host side of the DCT-variance prior tool (free-hunch_amd/frequency_analysis.py): file selection, image loading, the
atomic write, the rank logic over gloo and `finalize`'s arithmetic.  The device accumulation is replaced by an injected
host function (SciPy's orthonormal DCT, the suite's stand-in for torch_dct), as tests/test_distributed_gloo.py does for the
sampler; the GPU side is tests/test_frequency_prior_gpu.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _dct(u8):
    import scipy.fft
    x = np.asarray(u8).astype(np.float64) / 127.5 - 1
    return scipy.fft.dctn(x, type=2, norm="ortho", axes=(-2, -1))


def host_moments(u8, state):
    """fh_dct_moments_u8 restated on the host"""
    from free_hunch_amd import frequency_analysis as fa
    z = torch.from_numpy(_dct(u8.numpy()))
    return fa.Moments(state.sum + z.sum(0), state.sumsq + (z ** 2).sum(0), state.count + len(u8))


def _write_folder(root, n, hw=(16, 16), seed=3):
    """n random RGB PNGs in two class folders; returns the sorted paths (the order the tool must use)"""
    import PIL.Image
    g = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        d = os.path.join(root, "cls_b" if i % 2 else "cls_a")
        os.makedirs(d, exist_ok=True)
        p = os.path.join(d, f"img_{i:03d}.png")
        PIL.Image.fromarray(g.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)).save(p)
        paths.append(p)
    return sorted(paths)


def _load_rgb(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path).convert("RGB")).transpose(2, 0, 1)


def _spy(seen):
    def fn(u8, state):
        seen.append(u8.clone())
        return host_moments(u8, state)
    return fn


# ---------------------------------------------------------------- files, loading, writing
def test_file_order_and_num(tmp_path):
    from free_hunch_amd import frequency_analysis as fa
    paths = _write_folder(str(tmp_path), 7)
    assert [os.path.basename(os.path.dirname(p)) for p in paths] == ["cls_a"] * 4 + ["cls_b"] * 3
    for num, want in ((5, paths[:5]), (0, paths), (100, paths)):
        seen = []
        st = fa.run(str(tmp_path), _spy(seen), "cpu", num=num, size=16, batch=2, workers=3)
        got = torch.cat(seen).numpy()
        assert st.count == len(want) and got.shape == (len(want), 3, 16, 16) and got.dtype == np.uint8
        assert [len(b) for b in seen] == [2] * (len(want) // 2) + [1] * (len(want) % 2)  # uneven tail
        for a, p in zip(got, want):
            assert (a == _load_rgb(p)).all(), p
    # default output: DIR/dct_variance.pt, float32 [3,S,S], the variance (not the second moment) of the files used
    out = torch.load(tmp_path / "dct_variance.pt", weights_only=True)
    z = _dct(np.stack([_load_rgb(p) for p in paths]))
    ref = (z ** 2).mean(0) - z.mean(0) ** 2
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, 16, 16)
    assert np.abs(out.numpy() - ref).max() <= 2.0 ** -23 * ref.max()
    assert np.abs(out.numpy() - (z ** 2).mean(0)).max() > 0.1 * ref.max()  # the mean is not negligible on these files


def test_stats_out_and_report_line(tmp_path, capsys):
    from free_hunch_amd import frequency_analysis as fa
    paths = _write_folder(str(tmp_path / "data"), 6)
    out, stats = str(tmp_path / "prior.pt"), str(tmp_path / "stats.npz")
    fa.run(str(tmp_path / "data"), host_moments, "cpu", num=0, size=16, out=out, batch=4, workers=2, stats_out=stats)
    z = _dct(np.stack([_load_rgb(p) for p in paths]))
    s = np.load(stats)
    assert int(s["count"]) == 6 and s["mean"].dtype == s["variance"].dtype == np.float64
    assert np.abs(s["mean"] - z.mean(0)).max() <= 1e-13 * np.abs(z).max()
    assert np.abs(s["variance"] - z.var(0)).max() <= 1e-12 * z.var(0).max()
    assert not os.path.exists(tmp_path / "data" / "dct_variance.pt")  # --out given: nothing beside the images
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("frequency_analysis:")]
    assert len(line) == 1 and "6 images at 16 x 16" in line[0] and out in line[0] and "min variance" in line[0]


def test_grayscale_and_rgba_become_rgb(tmp_path):
    import PIL.Image
    from free_hunch_amd import frequency_analysis as fa
    g = np.random.default_rng(5)
    PIL.Image.fromarray(g.integers(0, 256, (16, 16), dtype=np.uint8), "L").save(tmp_path / "a_gray.png")
    PIL.Image.fromarray(g.integers(0, 256, (16, 16, 4), dtype=np.uint8), "RGBA").save(tmp_path / "b_rgba.png")
    PIL.Image.fromarray(g.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(tmp_path / "c_rgb.jpg")
    seen = []
    fa.run(str(tmp_path), _spy(seen), "cpu", num=0, size=16, batch=8, workers=2)
    got = torch.cat(seen).numpy()
    assert got.shape == (3, 3, 16, 16)
    for a, name in zip(got, ("a_gray.png", "b_rgba.png", "c_rgb.jpg")):
        assert (a == _load_rgb(tmp_path / name)).all(), name
    assert (got[0][0] == got[0][1]).all() and (got[0][1] == got[0][2]).all()  # grey: three equal planes


def test_resize_is_pil_bilinear(tmp_path):
    """The reference's transform (do_frequency_analysis.py:12-16): torchvision's Resize on a PIL image = PIL bilinear.
    The sampler's own loader (pipeline.load_image_u8) resizes bicubically and is not what this tool uses."""
    import PIL.Image
    from free_hunch_amd import frequency_analysis as fa
    from free_hunch_amd.pipeline import load_image_u8
    paths = _write_folder(str(tmp_path), 2, hw=(20, 24), seed=9)
    got = fa.load_image_u8_bilinear(paths[0], 16)
    img = PIL.Image.open(paths[0]).convert("RGB")
    assert img.size == (24, 20)
    want = np.asarray(img.resize((16, 16), PIL.Image.BILINEAR)).transpose(2, 0, 1)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 16, 16) and (got.numpy() == want).all()
    assert (got != load_image_u8(paths[0], 16)).any()  # the two filters do differ on this image
    seen = []
    fa.run(str(tmp_path), _spy(seen), "cpu", num=0, size=16, batch=4, workers=1)  # and the tool goes through that loader
    assert (seen[0][0].numpy() == want).all()


def test_failure_leaves_the_target_untouched(tmp_path):
    from free_hunch_amd import frequency_analysis as fa
    _write_folder(str(tmp_path / "data"), 5)
    out = tmp_path / "data" / "dct_variance.pt"
    torch.save(torch.full((3, 16, 16), 7.0), out)
    before, mtime = out.read_bytes(), os.path.getmtime(out)
    calls = []

    def failing(u8, state):
        calls.append(len(u8))
        if len(calls) == 2:
            raise RuntimeError("device lost")
        return host_moments(u8, state)

    with pytest.raises(RuntimeError, match="device lost"):
        fa.run(str(tmp_path / "data"), failing, "cpu", num=0, size=16, batch=2, workers=2)
    assert out.read_bytes() == before and os.path.getmtime(out) == mtime
    assert sorted(os.listdir(tmp_path / "data")) == ["cls_a", "cls_b", "dct_variance.pt"]  # no temporary left behind
    # too few images: finalize refuses, and again nothing is written
    with pytest.raises(ValueError, match="at least 2 images"):
        fa.run(str(tmp_path / "data"), host_moments, "cpu", num=1, size=16, batch=2, workers=2)
    assert out.read_bytes() == before
    # and a good run replaces it
    fa.run(str(tmp_path / "data"), host_moments, "cpu", num=0, size=16, batch=2, workers=2)
    assert float(torch.load(out, weights_only=True).max()) != 7.0
    assert sorted(os.listdir(tmp_path / "data")) == ["cls_a", "cls_b", "dct_variance.pt"]


def test_no_images_is_an_error(tmp_path):
    from free_hunch_amd import frequency_analysis as fa
    with pytest.raises(SystemExit, match="no images"):
        fa.run(str(tmp_path), host_moments, "cpu")


def test_device_function_has_no_cpu_fallback():
    from free_hunch_amd import _lib
    from free_hunch_amd import frequency_analysis as fa
    with pytest.raises(_lib.FhError, match="no CPU fallback"):
        fa.dct_moments(torch.zeros(2, 3, 16, 16, dtype=torch.uint8), device="cpu")


# ---------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, data, outdir, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from free_hunch_amd import frequency_analysis as fa
    from test_frequency_prior_host import host_moments
    calls, real = [], {}
    for name in ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast", "reduce", "gather", "barrier",
                 "all_gather_object", "broadcast_object_list", "reduce_scatter", "all_to_all", "send", "recv"):
        real[name] = getattr(dist, name)
        setattr(dist, name, lambda *a, _n=name, **k: (calls.append(_n), real[_n](*a, **k))[1])
    local = []

    def fn(u8, state):
        local.append(len(u8))
        return host_moments(u8, state)

    out = os.path.join(outdir, f"prior_rank{rank}.pt")  # a path per rank: whoever writes shows
    st = fa.run(data, fn, "cpu", num=0, size=16, out=out, batch=3, workers=2, rank=rank, world=world)
    for name, f in real.items():
        setattr(dist, name, f)
    q.put((rank, sum(local), st.sum.numpy().copy(), st.sumsq.numpy().copy(), st.count, calls))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_all_reduce(tmp_path):
    """7 images over 2 ranks (4 + 3): the merged moments equal the single-process ones, ONE collective, rank 0 writes.
    Bound: the ranks add the same 7 terms per coefficient in another order; re-ordering a sum of n terms moves it by at
    most (n - 1) eps sum |term|, so both moments are held to 1e-13 of their sum of magnitudes (for sumsq, whose terms are
    positive, that is 1e-13 relative per element)."""
    total, world = 7, 2
    data = str(tmp_path / "data")
    paths = _write_folder(data, total)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, data, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    z = _dct(np.stack([_load_rgb(p) for p in paths]))
    s_ref, q_ref = z.sum(0), (z ** 2).sum(0)
    assert sorted(n for _r, n, *_ in res) == [3, 4]  # uneven shard
    for rank, n_local, s, qq, count, calls in res:
        assert n_local == len(range(rank, total, world))
        assert count == total
        assert (np.abs(s - s_ref) <= 1e-13 * np.abs(z).sum(0)).all()
        assert (np.abs(qq - q_ref) <= 1e-13 * q_ref).all()
        assert calls == ["all_reduce"], calls
    assert os.path.exists(tmp_path / "prior_rank0.pt") and not os.path.exists(tmp_path / "prior_rank1.pt")
    v = torch.load(tmp_path / "prior_rank0.pt", weights_only=True).numpy()
    assert np.abs(v - z.var(0)).max() <= 2.0 ** -23 * z.var(0).max() + 1e-12


def test_merge_adds_partial_states():
    from free_hunch_amd import frequency_analysis as fa
    g = torch.Generator().manual_seed(2)
    parts = [fa.Moments(torch.rand(3, 4, 4, generator=g, dtype=torch.float64),
                        torch.rand(3, 4, 4, generator=g, dtype=torch.float64), c) for c in (4, 3, 0)]
    m = fa.merge(parts)
    assert m.count == 7
    assert torch.equal(m.sum, parts[0].sum + parts[1].sum + parts[2].sum)
    assert torch.equal(m.sumsq, parts[0].sumsq + parts[1].sumsq + parts[2].sumsq)


# ---------------------------------------------------------------- finalize
def test_finalize_arithmetic_and_errors():
    """mean = sum / N, variance = sumsq / N - mean^2 in float64 (do_frequency_analysis.py:52-53).  Each of the four
    operations is correctly rounded in torch and in numpy alike; the bound allows a few ulps of the larger operand sumsq / N
    in case one side fuses the multiply into the subtraction."""
    from free_hunch_amd import frequency_analysis as fa
    g = np.random.default_rng(11)
    N = 37
    z = g.standard_normal((N, 3, 8, 8)) * g.uniform(0.01, 20.0, (3, 8, 8)) + g.uniform(-5, 5, (3, 8, 8))
    s, q = z.sum(0), (z ** 2).sum(0)
    mean, var = fa.finalize(fa.Moments(torch.from_numpy(s), torch.from_numpy(q), N))
    assert mean.dtype == var.dtype == torch.float64 and tuple(var.shape) == (3, 8, 8)
    assert (np.abs(mean.numpy() - s / N) <= EPS * np.abs(s / N)).all()
    assert (np.abs(var.numpy() - (q / N - (s / N) ** 2)) <= 4 * EPS * (q / N)).all()
    assert np.abs(var.numpy() - z.var(0)).max() <= 1e-12 * z.var(0).max()  # and it is the variance
    with pytest.raises(ValueError, match="at least 2 images"):
        fa.finalize(fa.Moments(torch.from_numpy(z[0]), torch.from_numpy(z[0] ** 2), 1))
    with pytest.raises(ValueError, match="at least 2 images"):
        fa.finalize(fa.empty_moments(8, "cpu"))
    same = torch.from_numpy(z[0])
    with pytest.raises(ValueError, match="no positive variance"):  # three identical images
        fa.finalize(fa.Moments(3 * same, 3 * same ** 2, 3))
    one_bad = torch.from_numpy(q.copy())
    one_bad[1, 2, 3] = float(0.5 * s[1, 2, 3] ** 2 / N)  # a single coefficient is enough
    with pytest.raises(ValueError, match="1 of 192"):
        fa.finalize(fa.Moments(torch.from_numpy(s), one_bad, N))
    nan = torch.from_numpy(q.copy())
    nan[0, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="no positive variance"):
        fa.finalize(fa.Moments(torch.from_numpy(s), nan, N))


def test_cli_announces_the_prior_in_use():
    """generate_conditional.py names the dct_variance.pt it runs with, so that the fall-back to the shipped ImageNet file
    is visible (source check: the CLI itself needs the GPU, tests/test_cli_gpu.py)."""
    src = open(os.path.join(ROOT, "generate_conditional.py")).read()
    assert 'print(f"dct_variance: ' in src and "free_hunch_amd.frequency_analysis" in src
