"""Host side of the denoiser-error table tool (free-hunch_amd/recon_mse.py): the numpy restatement of its noise generator
against the published Philox known answers, the shipped table against the tool's own grid and validation, `finalize` /
`load_table`, level selection, and the rank logic over gloo with the device loop replaced by an injected host function
(tests/_recon_restatement.py), as tests/test_frequency_prior_host.py does for the prior tool.  The GPU side is
tests/test_recon_mse_gpu.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _recon_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = os.path.join(ROOT, "free-hunch_amd", "data", "recon_mse.pt")


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    """The three Philox4x32-10 vectors of the Random123 distribution (kat_vectors): without them the GPU test would compare the
    kernel with an unverified twin."""
    got = rr.philox4x32_10(ctr, key)
    assert " ".join(f"{int(v):08x}" for v in got) == want
    # and vectorised: the same words in every slot of an array counter
    arr = rr.philox4x32_10(tuple(np.full(5, c, dtype=np.uint64) for c in ctr), key)
    assert all((a == g).all() for a, g in zip(arr, got))


def test_restated_noise_moments():
    """36 864 samples (three 64 x 64 images, as the GPU test draws them): |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n) -
    five standard errors of the two estimators for unit normals."""
    seed = 0x100000007
    z = np.concatenate([rr.normals(seed, i, 3, 3 * 64 * 64) for i in (0, 5, 70000)])
    n = z.size
    assert n == 36864 and np.isfinite(z).all()
    print(f"mean {z.mean():+.4e} (bound {5 / np.sqrt(n):.4e}), var - 1 {z.var() - 1:+.4e} (bound {5 * np.sqrt(2 / n):.4e})")
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    # the key separates images, levels and seeds
    base = rr.normals(seed, 5, 3, 64)
    for other in (rr.normals(seed, 6, 3, 64), rr.normals(seed, 5, 4, 64), rr.normals(seed + 1, 5, 3, 64),
                  rr.normals(seed + (1 << 32), 5, 3, 64)):
        assert not np.array_equal(base, other)


# ---------------------------------------------------------------- the shipped table
def test_shipped_table_loads_and_matches_the_grid():
    from free_hunch_amd import recon_mse as rm
    t = rm.load_table(SHIPPED)
    assert rm.load_table() is t  # None = the shipped file, and it is read once
    assert set(t) == {"sigmas", "mse_list", "errors"} and tuple(t["errors"].shape) == (1001, 100)
    mse, err = t["mse_list"].double(), t["errors"].double()
    d = float((mse - err.mean(1)).abs().max())
    print(f"mse_list vs errors.mean(1): {d:.3e} = {d / float(mse.max()):.3e} of the maximum")
    assert d <= 2e-6 * float(mse.max())
    lv = rm.default_levels()
    assert lv.dtype == torch.float64 and tuple(lv.shape) == (1001,) and float(lv[-1]) == 0.0
    s = t["sigmas"].double()
    rel = float(((lv[:1000] - s[:1000]).abs() / lv[:1000]).max())
    print(f"default_levels() vs the shipped sigmas: {rel:.3e} relative")
    assert rel <= 1e-5 and float(s[1000]) == 0.0
    assert int((lv < 0.2).sum()) == 206


# ---------------------------------------------------------------- finalize / load_table
def _good(L=8, N=5):
    from free_hunch_amd import recon_mse as rm
    g = np.random.default_rng(3)
    return torch.from_numpy(g.uniform(0.01, 0.2, (L + 1, N))), rm.levels_grid(L)


def test_finalize_arithmetic():
    from free_hunch_amd import recon_mse as rm
    e, s = _good()
    t = rm.finalize(e, s)
    assert set(t) == {"sigmas", "mse_list", "errors"} and all(v.dtype == torch.float32 for v in t.values())
    assert torch.equal(t["mse_list"], e.mean(1).to(torch.float32))  # the float64 mean, then cast
    assert torch.equal(t["errors"], e.to(torch.float32)) and torch.equal(t["sigmas"], s.to(torch.float32))


def test_finalize_and_load_table_refuse(tmp_path):
    from free_hunch_amd import recon_mse as rm
    e, s = _good()
    bad = e.clone()
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        rm.finalize(bad, s)
    bad = e.clone()
    bad[3, 0] = -1e-9
    with pytest.raises(ValueError, match="negative"):
        rm.finalize(bad, s)
    with pytest.raises(ValueError, match="one row per sigma"):
        rm.finalize(e[:-1], s)
    with pytest.raises(ValueError, match="at least 2 images"):
        rm.finalize(e[:, :1], s)
    high = s[s >= 0.2]
    with pytest.raises(ValueError, match="no level below"):
        rm.finalize(e[: len(high)], high)
    good = rm.finalize(e, s)
    cases = {
        "nan": ({**good, "mse_list": torch.full_like(good["mse_list"], float("nan"))}, "non-finite"),
        "negative": ({**good, "mse_list": -good["mse_list"]}, "negative"),
        "lengths": ({**good, "mse_list": good["mse_list"][:-1]}, "one length"),
        "two_d": ({**good, "sigmas": good["sigmas"][None]}, "1-D"),
        "above": ({"sigmas": good["sigmas"][:3], "mse_list": good["mse_list"][:3]}, "no level below"),
        "keys": ({"sigma": good["sigmas"], "mse_list": good["mse_list"]}, "expected a dict"),
        "extra": ({**good, "more": good["sigmas"]}, "expected a dict"),
        "tensor": (good["mse_list"], "expected a dict"),
    }
    for name, (obj, msg) in cases.items():
        p = str(tmp_path / f"{name}.pt")
        torch.save(obj, p)
        with pytest.raises(ValueError, match=msg):
            rm.load_table(p)
    p = str(tmp_path / "good.pt")
    torch.save(good, p)
    t = rm.load_table(p)
    assert torch.equal(t["mse_list"], good["mse_list"])
    torch.save({k: good[k] for k in ("sigmas", "mse_list")}, p)  # `errors` is optional: consumers do not read it
    os.utime(p, (1, 1))
    assert set(rm.load_table(p)) == {"sigmas", "mse_list"}


def test_sigma_max_keeps_the_described_levels():
    """--sigma-max X: the levels <= X, the first one above X, and sigma = 0 - with their indices in the full grid, which key
    the noise."""
    from free_hunch_amd import recon_mse as rm
    grid = rm.default_levels()
    assert rm.select_levels(grid) == list(range(1001))
    ids = rm.select_levels(grid, 0.2)
    assert ids == list(range(1000 - 206, 1001)) and len(ids) == 207  # 205 non-zero levels below 0.2, one above, and 0
    assert float(grid[ids[0]]) > 0.2 and float(grid[ids[1]]) <= 0.2 and float(grid[ids[-1]]) == 0.0
    small = rm.levels_grid(6)
    edm = (80 ** (1 / 7) + np.arange(6) / 5 * (0.01 ** (1 / 7) - 80 ** (1 / 7))) ** 7  # 80, 26.8, 7.33, 1.49, 0.189, 0.01
    assert np.allclose(small.numpy(), np.append(edm, 0.0), rtol=1e-12, atol=0) and 0.18 < float(small[4]) < 0.2
    assert rm.select_levels(small, 0.2) == [3, 4, 5, 6]
    assert rm.select_levels(small, 100.0) == list(range(7))
    assert rm.select_levels(small, 0.005) == [5, 6]
    assert rm.select_levels(small, float(small[4])) == [3, 4, 5, 6]  # a level equal to X is kept as "<= X"


def test_device_function_has_no_cpu_fallback():
    from free_hunch_amd import _lib
    from free_hunch_amd import recon_mse as rm
    with pytest.raises(_lib.FhError, match="no CPU fallback"):
        rm.level_errors(None, torch.zeros(2, 3, 16, 16, dtype=torch.uint8), [0, 1], [1.0], [0], 0)


# ---------------------------------------------------------------- the tool on the host
def _write_folder(root, n, size=64, seed=3):
    import PIL.Image
    g = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        d = os.path.join(root, "cls_b" if i % 2 else "cls_a")
        os.makedirs(d, exist_ok=True)
        p = os.path.join(d, f"img_{i:03d}.png")
        PIL.Image.fromarray(g.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(p)
        paths.append(p)
    return sorted(paths)


def host_levels(u8, img_index, sigmas, level_ids, seed):
    """level_errors restated on the host with the closed-form Gaussian-prior denoiser"""
    return torch.from_numpy(rr.errors(rr.gauss_denoise(), u8.numpy(), img_index, sigmas, level_ids, seed))


def test_run_writes_the_table_and_reports(tmp_path, capsys):
    import PIL.Image
    from free_hunch_amd import recon_mse as rm
    data = str(tmp_path / "data")
    paths = _write_folder(data, 7)
    seen = []

    def fn(u8, idx, sg, ids, seed):
        seen.append((tuple(u8.shape), list(idx), list(ids), seed))
        return host_levels(u8, idx, sg, ids, seed)

    stats = str(tmp_path / "stats.npz")
    sig, err = rm.run(data, fn, "cpu", num=5, size=64, batch=3, seed=11, levels=6, stats_out=stats)
    assert seen == [((3, 3, 64, 64), [0, 1, 2], list(range(7)), 11), ((2, 3, 64, 64), [3, 4], list(range(7)), 11)]
    assert tuple(err.shape) == (7, 5) and err.dtype == torch.float64 and torch.equal(sig, rm.levels_grid(6))
    u8 = np.stack([np.asarray(PIL.Image.open(p).convert("RGB")).transpose(2, 0, 1) for p in paths[:5]])
    ref = rr.errors(rr.gauss_denoise(), u8, range(5), sig, range(7), 11)  # all five in one batch: same numbers
    assert np.array_equal(err.numpy(), ref)
    assert (err[-1] == 0).all() and float(err[0].mean()) > 10 * float(err[-2].mean())
    t = rm.load_table(os.path.join(data, "recon_mse.pt"))
    assert torch.equal(t["errors"], err.float()) and torch.equal(t["mse_list"], err.mean(1).float())
    st = np.load(stats)
    assert np.array_equal(st["errors"], ref) and list(st["level_ids"]) == list(range(7)) and int(st["seed"]) == 11
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("recon_mse:")]
    assert len(line) == 1 and "5 images at 64 x 64, 7 levels" in line[0] and os.path.join(data, "recon_mse.pt") in line[0]
    for i, what in ((0, "largest"), (4, "first below 0.2"), (5, "smallest non-zero")):
        assert f"{float(t['mse_list'][i]):.6g} at sigma = {float(sig[i]):.6g} ({what})" in line[0], line[0]
    assert sorted(os.listdir(data)) == ["cls_a", "cls_b", "recon_mse.pt"]  # no temporary left behind
    # --sigma-max: fewer levels, the SAME numbers at the levels kept (the noise is keyed by the index in the full grid)
    out2 = str(tmp_path / "low.pt")
    sig2, err2 = rm.run(data, host_levels, "cpu", num=5, size=64, batch=5, seed=11, levels=6, sigma_max=0.2, out=out2)
    assert torch.equal(sig2, sig[3:]) and torch.equal(err2, err[3:])
    assert torch.equal(rm.load_table(out2)["sigmas"], sig[3:].float())
    with pytest.raises(ValueError, match="at least 2 images"):
        rm.run(data, host_levels, "cpu", num=1, size=64, levels=6, out=str(tmp_path / "one.pt"))
    assert not os.path.exists(tmp_path / "one.pt")
    with pytest.raises(SystemExit, match="no images"):
        rm.run(str(tmp_path / "stats.npz") + ".d", host_levels, "cpu")


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
    from free_hunch_amd import recon_mse as rm
    from test_recon_mse_host import host_levels
    calls, real = [], {}
    for name in ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast", "reduce", "gather", "barrier",
                 "all_gather_object", "broadcast_object_list", "reduce_scatter", "all_to_all", "send", "recv"):
        real[name] = getattr(dist, name)
        setattr(dist, name, lambda *a, _n=name, **k: (calls.append(_n), real[_n](*a, **k))[1])
    local = []

    def fn(u8, idx, sg, ids, seed):
        local.extend(idx)
        return host_levels(u8, idx, sg, ids, seed)

    out = os.path.join(outdir, f"table_rank{rank}.pt")  # a path per rank: whoever writes shows
    _sig, err = rm.run(data, fn, "cpu", num=0, size=64, out=out, batch=3, seed=5, levels=6, rank=rank, world=world)
    for name, f in real.items():
        setattr(dist, name, f)
    q.put((rank, local, err.numpy().copy(), calls))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_all_reduce_same_file(tmp_path):
    """7 images over 2 ranks (4 + 3), batch 3: every rank holds the merged [L, N] buffer, ONE collective, rank 0 writes - and
    the file is bitwise the single-process one: every column is computed by one rank and merged by adding zeros."""
    from free_hunch_amd import recon_mse as rm
    total, world = 7, 2
    data = str(tmp_path / "data")
    _write_folder(data, total)
    single = str(tmp_path / "single.pt")
    _sig, err1 = rm.run(data, host_levels, "cpu", num=0, size=64, out=single, batch=3, seed=5, levels=6)
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
    for rank, local, err, calls in res:
        assert local == list(range(rank, total, world))
        assert np.array_equal(err, err1.numpy())
        assert calls == ["all_reduce"], calls
    assert os.path.exists(tmp_path / "table_rank0.pt") and not os.path.exists(tmp_path / "table_rank1.pt")
    assert (tmp_path / "table_rank0.pt").read_bytes() == (tmp_path / "single.pt").read_bytes()


def test_peng_analytic_reads_the_table_it_is_given(tmp_path):
    """The scalar-variance plugin needs no device to be built: below sigma = 0.2 its variance is the nearest level's entry of
    the table at `recon_mse_path`, of the shipped table without one; above, sigma^2 / (1 + sigma^2) either way."""
    from free_hunch_amd import recon_mse as rm
    from free_hunch_amd.conditioning_mechanisms import choose_conditioning_mechanism
    path = str(tmp_path / "recon_mse.pt")
    torch.save({"sigmas": torch.tensor([80.0, 1.0, 0.15, 0.05, 0.0]), "mse_list": torch.tensor([0.2, 0.1, 0.0123, 0.004, 0.0])},
               path)
    cls = choose_conditioning_mechanism("peng_analytic")
    own, default = cls(1.0, None, False, data_dim=12, recon_mse_path=path), cls(1.0, None, False, data_dim=12)
    assert default.recon_mse is rm.load_table() and own.recon_mse is rm.load_table(path)
    s = torch.tensor(0.12, dtype=torch.float64)
    assert float(own._variance(s)) == pytest.approx(0.0123) and float(own._variance(s / 2)) == pytest.approx(0.004)
    shipped = rm.load_table()
    assert float(default._variance(s)) == float(shipped["mse_list"][(shipped["sigmas"] - s).abs().argmin()])
    big = torch.tensor(3.0, dtype=torch.float64)
    assert float(own._variance(big)) == float(default._variance(big)) == pytest.approx(0.9)


def test_cli_announces_the_table_in_use():
    """generate_conditional.py names the recon_mse.pt it runs with (source check: the CLI itself needs the GPU,
    tests/test_recon_mse_gpu.py)."""
    src = open(os.path.join(ROOT, "generate_conditional.py")).read()
    assert 'print(f"recon_mse: ' in src and "free_hunch_amd.recon_mse" in src
