"""Posterior ensembles, the host side: the ABI of fh_ensemble_stats, the numpy restatement of its definition, member seeds, the
unit listing and the flag.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _ensemble_restatement as er


# ---------------------------------------------------------------- 1. ABI
def test_symbols_exported_with_prototypes():
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    lib = _lib.load()
    dp = _lib.c_dp
    want = {"fh_ensemble_scratch_doubles": ([ctypes.c_int, ctypes.c_int], ctypes.c_int64),
            "fh_ensemble_stats": ([dp, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, ctypes.c_void_p], ctypes.c_int)}
    for name, (args, res) in want.items():
        assert name in _lib.exported_symbols()
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is res, name
    # the scratch size needs no device: [N][chunks][4] doubles, the chunking a function of n alone; 0 for a shape the call refuses
    one = lib.fh_ensemble_scratch_doubles(1, 3 * 256 * 256)
    assert one > 0 and one % 4 == 0 and lib.fh_ensemble_scratch_doubles(5, 3 * 256 * 256) == 5 * one
    assert lib.fh_ensemble_scratch_doubles(1, 1) == 4
    assert lib.fh_ensemble_scratch_doubles(0, 10) == 0 and lib.fh_ensemble_scratch_doubles(1, 0) == 0


# ---------------------------------------------------------------- 2. the restatement
def test_restatement_identical_members():
    """Three identical members: no spread, and an element is covered exactly where the truth is the mean.  The values are
    eighths of a grey level, for which (v + v + v) / 3 is exact; for a general double that mean is an ulp off in one case out of
    six, and std is then of the order of 1e-14, not 0."""
    rng = np.random.default_rng(1)
    v = np.repeat(rng.integers(0, 255 * 8 + 1, (1, 500)) / 8.0, 3, axis=0)
    truth = np.where(rng.random(500) < 0.5, np.floor(v[0]), 255 - np.floor(v[0])).astype(np.uint8)
    r = er.stats_of_values(v, truth)
    assert np.all(r["m"] == v[0]) and np.all(r["SS"] == 0.0) and np.all(r["std"] == 0.0) and r["spread2"] == 0.0
    for c in (1, 2):
        assert r[f"covered{c}"].dtype == bool and np.array_equal(r[f"covered{c}"], truth == v[0])
    assert 0 < r["count1"] == r["count2"] < 500 and r["cover1"] == r["count1"] / 500.0
    r = er.stats_of_values(np.full((3, 4), 17.0), np.array([17, 18, 16, 17], dtype=np.uint8))
    assert np.all(r["std"] == 0.0) and list(r["covered1"]) == [True, False, False, True] == list(r["covered2"])
    assert r["cover1"] == 0.5 and r["spread2"] == 0.0 and r["skill2"] == 0.5
    # through the sampler's units as well: x = 0 is 127.5 in every member
    r = er.ensemble_stats(np.zeros((3, 2)), np.array([127, 128], dtype=np.uint8))
    assert np.all(r["std"] == 0.0) and r["count2"] == 0 and list(r["mean_u8"]) == [128, 128]


def test_restatement_two_members():
    r = er.stats_of_values(np.array([[10.0], [20.0]]), np.array([18], dtype=np.uint8))
    assert r["m"][0] == 15.0 and r["SS"][0] == 50.0 and r["mean_u8"][0] == 15
    assert r["std"][0] == np.float32(np.sqrt(50.0)) and r["spread2"] == 50.0 and r["skill2"] == 9.0
    # d2 K (K - 1) = 18 against c^2 SS (K + 1) = 150 c^2: covered; a truth 9 levels off (162) only at 2 sigma
    assert r["covered1"][0] and r["covered2"][0]
    r = er.stats_of_values(np.array([[10.0], [20.0]]), np.array([24], dtype=np.uint8))
    assert not r["covered1"][0] and r["covered2"][0]
    assert er.stats_of_values(np.array([[10.0], [20.0]]))["skill2"] == -1.0


def test_restatement_clips_before_the_mean():
    r = er.ensemble_stats(np.array([[3.0], [-1.0]]))  # 510 -> 255, 0: the mean is 127.5, not 255
    assert r["m"][0] == 127.5 and r["mean_u8"][0] == 128
    r = er.ensemble_stats(np.array([[-5.0, 0.0], [-1.0, 0.0]]))
    assert r["m"][0] == 0.0 and r["std"][0] == 0.0 and r["m"][1] == 127.5
    assert not er.fair(er.ensemble_stats(np.array([[3.0], [-1.0]])))  # m + 0.5 = 128: the floor sits on an integer
    assert er.fair(er.ensemble_stats(np.array([[0.3], [0.1]]), np.array([150], dtype=np.uint8)))


# ---------------------------------------------------------------- 3. seeds
def test_member_seeds():
    from free_hunch_amd.ensemble import member_noise, member_seed, noise_seed, unit_key
    keys = (0, 1, 2**31 - 1)
    assert all(member_seed(key, 0) == key for key in keys)
    seeds = [member_seed(key, k) for key in keys for k in range(64)]
    assert len(set(seeds)) == len(seeds) and max(seeds) < 2**63
    key = unit_key(7, 3)
    assert key == (3 * 1000003 + 7) % (1 << 31)
    today = torch.randn((1, 3, 16, 16), generator=torch.Generator().manual_seed(key), dtype=torch.float32)
    assert torch.equal(member_noise(key, 0, 16), today)
    # torch's CPU generator reads 32 bits of a seed: seeded with member_seed itself, members k and k + 2 would share their noise.
    # All 64 members of a unit draw different noise, at the smallest and the largest key too
    for key in keys + (key,):
        draws = [member_noise(key, k, 4) for k in range(64)]
        assert len({d.numpy().tobytes() for d in draws}) == 64, key
        assert len({noise_seed(key, k) for k in range(64)}) == 64 and noise_seed(key, 0) == key


# ---------------------------------------------------------------- 4. the unit listing
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_units_stay_on_one_rank(world):
    from free_hunch_amd.ensemble import list_units
    from free_hunch_amd.pipeline import shard_indices
    total, seeds, K = 11, [0, 5], 3
    owner = {}
    for rank in range(world):
        units = list_units(shard_indices(total, rank, world), seeds, K)
        for (i, sd), grp in itertools.groupby(units, key=lambda u: u[:2]):
            assert [u[2] for u in grp] == list(range(K))  # adjacent, in member order
            assert (i, sd) not in owner  # one run of K members, on one rank
            owner[(i, sd)] = rank
    assert sorted(owner) == [(i, sd) for i in range(total) for sd in seeds]


def test_units_of_one_member_are_todays():
    from free_hunch_amd.ensemble import list_units
    mine, seeds = [1, 4, 7], [0, 2]
    assert list_units(mine, seeds, 1) == [(i, sd, 0) for i in mine for sd in seeds]
    assert [u[:2] for u in list_units(mine, seeds)] == [(i, sd) for i in mine for sd in seeds]


# ---------------------------------------------------------------- 5. the flag
def test_flag_default_and_refusals():
    from free_hunch_amd.config import SCHEMA, load_config
    assert SCHEMA["posterior_samples"] == (int, 1)
    assert load_config(["--outdir=x"]).posterior_samples == 1
    assert load_config(["--outdir=x", "--posterior_samples=64"]).posterior_samples == 64
    for bad in ("0", "65", "-3"):
        with pytest.raises(SystemExit) as e:
            load_config(["--outdir=x", f"--posterior_samples={bad}"])
        assert "--posterior_samples" in str(e.value)


def test_ensemble_stats_refuses_cpu_tensors():
    from free_hunch_amd._lib import FhError
    from free_hunch_amd.ensemble import ensemble_stats
    with pytest.raises(FhError):
        ensemble_stats(torch.zeros(2, 1, 4, 4, dtype=torch.float64))
