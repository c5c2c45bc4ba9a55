"""Posterior ensembles on the GPU: fh_ensemble_stats against its numpy restatement (tests/_ensemble_restatement.py), its
refusals, the unit building of the CLI and `sample_ensemble` against the per-image sampler."""
import os
import sys

import numpy as np
import pytest
import torch

import _ensemble_restatement as er
import nets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# n -> an image shape with that many elements: 1; odd and below one chunk; 3 x 30 x 30; 3 x 64 x 64 (six chunks of 2048); two
# chunks plus one element (odd: the scalar route, and a last chunk of one element)
SHAPES = {1: (1, 1, 1), 49: (1, 7, 7), 2700: (3, 30, 30), 12288: (3, 64, 64), 4097: (1, 1, 4097)}
MEMBERS = (2, 3, 17, 64)
_CASES = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _case(n, K):
    """Three ensembles x [3,K,n] = 1.15 (smooth + 0.3 randn) - both clips occur from n = 49 on - with a truth drawn about the
    same smooth signal, and the restatement of each ensemble with and without it.  Built once per (n, K) and left unchanged; the
    seed is a function of (n, K) for which `er.fair` holds (asserted: the exact comparisons below are fair)."""
    if (n, K) not in _CASES:
        rng = np.random.default_rng(100 * n + K)
        p = np.arange(n)
        smooth = np.stack([np.sin(2 * np.pi * 3 * (p + 0.5) / max(n, 2) + 0.7 * e) for e in range(3)])  # [3, n]
        x = 1.15 * (smooth[:, None, :] + 0.3 * rng.standard_normal((3, K, n)))
        truth = np.clip(np.floor(127.5 * (smooth + 0.3 * rng.standard_normal((3, n))) + 128.0), 0, 255).astype(np.uint8)
        ref = [er.ensemble_stats(x[e], truth[e]) for e in range(3)]
        bare = [er.ensemble_stats(x[e]) for e in range(3)]
        assert all(er.fair(r) for r in ref), (n, K)
        if n >= 49:
            v = er.to_u8_units(x)
            assert (v == 0.0).any() and (v == 255.0).any()
        _CASES[(n, K)] = (x, truth, ref, bare)
    return _CASES[(n, K)]


def _compare(st, e, ref, with_truth, what):
    """ensemble e of the device result `st` (batched form) against the restatement `ref`"""
    n = ref["m"].size
    assert np.array_equal(st.mean_u8[e].cpu().numpy().reshape(n), ref["mean_u8"]), what
    std = st.std[e].cpu().numpy().reshape(n)
    assert std.dtype == np.float32 and np.array_equal(std.view(np.uint32), ref["std"].view(np.uint32)), what
    spread2, skill2, c1, c2 = (float(t[e]) for t in (st.spread2, st.skill2, st.cover1, st.cover2))
    assert abs(spread2 - ref["spread2"]) <= 1e-10 * ref["spread2"], (what, spread2, ref["spread2"])
    if with_truth:
        assert abs(skill2 - ref["skill2"]) <= 1e-10 * ref["skill2"], (what, skill2, ref["skill2"])
        assert (round(c1 * n), round(c2 * n)) == (ref["count1"], ref["count2"]), what
        assert (c1, c2) == (ref["cover1"], ref["cover2"]), what  # count / n, one rounding on either side
    else:
        assert (skill2, c1, c2) == (-1.0, -1.0, -1.0), what


# ---------------------------------------------------------------- 1. the kernel against the restatement
@pytest.mark.parametrize("K", MEMBERS)
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_stats_match_restatement(dev, n, K):
    from free_hunch_amd.ensemble import ensemble_stats
    x, truth, ref, bare = _case(n, K)
    xd = torch.from_numpy(x).to(dev).reshape((3, K) + SHAPES[n])
    td = torch.from_numpy(truth).to(dev).reshape((3,) + SHAPES[n])
    for N in (3, 1):
        st = ensemble_stats(xd[:N], td[:N])
        assert tuple(st.mean_u8.shape) == (N,) + SHAPES[n] == tuple(st.std.shape) and tuple(st.spread2.shape) == (N,)
        for e in range(N):
            _compare(st, e, ref[e], True, (n, K, N, e, "truth"))
        st = ensemble_stats(xd[:N])
        for e in range(N):
            _compare(st, e, bare[e], False, (n, K, N, e, "no truth"))
    # the one-ensemble form: [K,C,H,W] in, one image and 0-d numbers out
    one = ensemble_stats(xd[0], td[0])
    assert tuple(one.mean_u8.shape) == SHAPES[n] and one.cover1.dim() == 0
    assert torch.equal(one.mean_u8, st.mean_u8[0]) and torch.equal(one.std, st.std[0])
    assert float(one.spread2) == float(st.spread2[0]) and float(one.cover2) == ref[0]["cover2"]


# ---------------------------------------------------------------- 2. batch independence, and the two load routes
def test_batch_independence(dev):
    """ensemble 1 of an N = 3 call equals the same ensemble computed alone, bit for bit, for all outputs"""
    from free_hunch_amd.ensemble import ensemble_stats
    n, K = 12288, 17
    x, truth, _, _ = _case(n, K)
    xd = torch.from_numpy(x).to(dev).reshape((3, K) + SHAPES[n])
    td = torch.from_numpy(truth).to(dev).reshape((3,) + SHAPES[n])
    full, alone = ensemble_stats(xd, td), ensemble_stats(xd[1:2], td[1:2])
    for a, b in zip(full, alone):
        assert torch.equal(a[1:2], b)
    assert not torch.equal(full.mean_u8[0], full.mean_u8[1])


def test_unaligned_samples_take_the_scalar_route(dev):
    """an even n with x off the 16-byte grid reads element by element: the same bits as the 16-byte loads"""
    from free_hunch_amd import _lib
    from free_hunch_amd.ensemble import ensemble_stats
    n, K = 2700, 3
    x, truth, ref, _ = _case(n, K)
    lib = _lib.load()
    buf = torch.zeros(K * n + 1, dtype=torch.float64, device=dev)
    buf[1:] = torch.from_numpy(x[0]).to(dev).reshape(-1)
    xs = buf[1:]
    assert xs.data_ptr() % 16 == 8
    td = torch.from_numpy(truth[0]).to(dev)
    mean_u8 = torch.empty(n, dtype=torch.uint8, device=dev)
    std = torch.empty(n, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.fh_ensemble_scratch_doubles(1, n), dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    assert lib.fh_ensemble_stats(xs.data_ptr(), td.data_ptr(), 1, K, n, mean_u8.data_ptr(), std.data_ptr(), scratch.data_ptr(),
                                 out.data_ptr(), _lib.stream()) == 0
    st = ensemble_stats(xs.clone().reshape((K,) + SHAPES[n]), td.reshape(SHAPES[n]))
    assert torch.equal(st.mean_u8.reshape(-1), mean_u8) and torch.equal(st.std.reshape(-1), std)
    assert out.tolist() == [float(st.spread2), float(st.skill2), float(st.cover1), float(st.cover2)]
    assert np.array_equal(mean_u8.cpu().numpy(), ref[0]["mean_u8"])


# ---------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_outputs_alone(dev):
    from free_hunch_amd import _lib
    lib = _lib.load()
    n, K = 96, 3
    x = torch.zeros(65 * n, dtype=torch.float64, device=dev)
    truth = torch.zeros(n, dtype=torch.uint8, device=dev)
    mean_u8 = torch.full((n,), 0xAB, dtype=torch.uint8, device=dev)
    std = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    scratch = torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    out = torch.full((4,), 7.0, dtype=torch.float64, device=dev)
    good = dict(x=x.data_ptr(), truth=truth.data_ptr(), N=1, K=K, n=n, mean_u8=mean_u8.data_ptr(), std=std.data_ptr(),
                scratch=scratch.data_ptr(), out=out.data_ptr())

    def call(**over):
        a = {**good, **over}
        return lib.fh_ensemble_stats(a["x"], a["truth"], a["N"], a["K"], a["n"], a["mean_u8"], a["std"], a["scratch"], a["out"],
                                     _lib.stream())

    assert call(K=1) == _lib.FH_EINVAL and call(K=65) == _lib.FH_EINVAL
    assert call(n=0) == _lib.FH_EINVAL and call(N=0) == _lib.FH_EINVAL
    for name in ("x", "mean_u8", "std", "scratch", "out"):
        assert call(**{name: None}) == _lib.FH_EINVAL, name
    assert call(N=65536) == _lib.FH_ESIZE  # (refused before any launch: the buffers hold one ensemble)
    torch.cuda.synchronize()
    assert bool((mean_u8 == 0xAB).all()) and bool((std == 7.0).all()) and bool((scratch == 7.0).all()) and bool((out == 7.0).all())
    assert call() == 0 and call(truth=None) == 0  # the same arguments are accepted once they are in range
    torch.cuda.synchronize()
    assert bool((mean_u8 == 128).all()) and bool((std == 0.0).all()) and out.tolist() == [0.0, -1.0, -1.0, -1.0]


# ---------------------------------------------------------------- 4. unit building, through the function the CLI calls
def _dataset(tmp_path, S):
    import PIL.Image
    sys.path.insert(0, ROOT)
    from bench import smooth_images
    data = tmp_path / "data"
    data.mkdir()
    PIL.Image.fromarray(smooth_images(1, S, 7)[0].permute(1, 2, 0).numpy(), "RGB").save(data / "img00000000.png")
    return data


@pytest.mark.parametrize("operator", ["inpainting", "motion_blur"])
def test_members_share_the_problem(dev, tmp_path, operator):
    """K = 3 with max_batch_size = 2: the ensemble straddles two batches"""
    from free_hunch_amd import ensemble as ens
    from free_hunch_amd.config import load_config
    from free_hunch_amd.pipeline import list_images
    S, K = 64, 3
    data = _dataset(tmp_path, S)
    o = load_config([f"--outdir={tmp_path}", f"--dataset_path={data}", f"--operator_name={operator}", f"--posterior_samples={K}",
                     "--max_batch_size=2", "--inpainting_prob_lower=0.6", "--inpainting_prob_upper=0.8", "--seeds=4"])
    files = list_images(o.dataset_path)
    units = ens.list_units([0], o.seeds, o.posterior_samples)
    assert units == [(0, 4, 0), (0, 4, 1), (0, 4, 2)]
    ops, ys, noise, slots, carry = [], [], [], [], None
    for s in range(0, K, o.max_batch_size):
        chunk = units[s: s + o.max_batch_size]
        b_ops, b_ys, b_noise, imgs, carry = ens.build_batch(o, files, chunk, S, dev, carry)
        assert [op.ctx_slot for op in b_ops] == list(range(len(chunk)))  # the position in ITS batch
        assert all(im.dtype == torch.uint8 and tuple(im.shape) == (3, S, S) for im in imgs)
        ops, ys, noise = ops + b_ops, ys + b_ys, noise + b_noise
    # a rebuilt measurement (no carry) is the same one, bit for bit
    r_ops, r_ys, _, _, _ = ens.build_batch(o, files, units[2:], S, dev, None)
    ops, ys = ops + r_ops, ys + r_ys
    content = (lambda op: op.mask) if operator == "inpainting" else (lambda op: op.taps.kernel)
    for op, y in zip(ops[1:], ys[1:]):
        assert op is not ops[0] and torch.equal(content(op), content(ops[0]))
        assert y.dtype == ys[0].dtype and torch.equal(y, ys[0])
    if operator == "inpainting":
        kept = float(ops[0].mask.float().mean())
        assert 0.15 < kept < 0.45  # a random mask that drops 60 .. 80 %
    key = ens.unit_key(0, 4)
    assert torch.equal(noise[0], torch.randn((1, 3, S, S), generator=torch.Generator().manual_seed(key), dtype=torch.float32))
    for a in range(K):
        for b in range(a + 1, K):
            assert not torch.equal(noise[a], noise[b])


# ---------------------------------------------------------------- 5. sample_ensemble against the per-image sampler
def test_sample_ensemble_equals_per_image(dev, tmp_path):
    """K = 4 members through the lock-step route (the default two groups) against `conditional_sampler` alone on (noise_k, y) by
    the rule of tests/test_batched_sampler.py: equal niter and k traces, outputs within 1e-3 - and members further apart than that"""
    from free_hunch_amd import ensemble as ens
    from free_hunch_amd.config import load_config
    from free_hunch_amd.pipeline import list_images
    from free_hunch_amd.sampler import conditional_sampler, conditional_sampler_grouped
    S, K = 64, 4
    data = _dataset(tmp_path, S)
    o = load_config([f"--outdir={tmp_path}", f"--dataset_path={data}", "--operator_name=inpainting", f"--posterior_samples={K}",
                     "--inpainting_prob_lower=0.6", "--inpainting_prob_upper=0.8"])
    ops, ys, noise, imgs, _ = ens.build_batch(o, list_images(o.dataset_path), ens.list_units([0], [0], K), S, dev)
    net = nets.gauss_net(S, dev)
    kw = dict(conditioning_mechanism="online_covariance", cond_scaling=1.0, clip_x0_mean=False, max_vector_count=100000,
              dataset_path=str(tmp_path), image_base_covariance="identity", denoiser_mean_error_threshold=0.2,
              use_analytical_score_time_update=True, project_to_diagonal=False, space_step_update_threshold=10.0,
              space_step_update_lower_threshold=1.0, max_rtol=1.0, do_space_updates=True)
    run = dict(num_steps=4, sigma_min=0.002, sigma_max=80, rho=7, solver="heun")
    x = ens.sample_ensemble(net, ops, ys[0], torch.cat(noise), **run, **kw)
    torch.cuda.synchronize()
    traces = [m.trace for m in conditional_sampler_grouped.last_mechanisms]
    assert tuple(x.shape) == (K, 3, S, S) and x.dtype == torch.float64 and bool(torch.isfinite(x).all())
    for k in range(K):
        x1, _, _ = conditional_sampler(net, noise[k].to(dev), None, None, measurement=ys[0], operator=ops[k], **run, **kw)
        t1 = conditional_sampler.last_mechanism.trace
        assert [t["niter"] for t in t1] == [t["niter"] for t in traces[k]], k
        assert [t["k"] for t in t1] == [t["k"] for t in traces[k]], k
        assert float((x1 - x[k:k + 1]).abs().max()) < 1e-3, k
    for a in range(K):
        for b in range(a + 1, K):
            assert float((x[a] - x[b]).abs().max()) > 1e-3, (a, b)
    st = ens.ensemble_stats(x, imgs[0].to(dev))
    assert float(st.std.max()) > 0 and 0.0 <= float(st.cover1) <= float(st.cover2) <= 1.0
