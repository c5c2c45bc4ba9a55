"""The denoiser-error table on the device (free-hunch_amd/recon_mse.py, fh_noisy_u8, fh_sqerr_u8) against the numpy restatement
of tests/_recon_restatement.py, whose generator tests/test_recon_mse_host.py pins to the published Philox known answers.

Inputs: uint8 images round((smooth_image(S, 100 + i) + 1) * 127.5), the quantisation of tests/test_frequency_prior_gpu.py.

Tolerances (each derived where it is used): fh_noisy_u8 one float32 ulp per element (the sum is formed in float64 on both sides
and rounded once; the device's log / sincos may differ from numpy's in the last bits of the float64, which moves the float32
only at a rounding tie); fh_sqerr_u8 1e-12 relative (a float64 sum of 3 S^2 <= 196 608 non-negative terms in any order is within
n eps = 4.4e-11 in the worst case and ~sqrt(n) eps = 1e-13 typically); whole tables 1e-6 relative per entry (a one-ulp difference
in one x_t element moves a per-image sum by ~1e-7 relative at most, the float32 store of D adds 2^-23 per element)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _recon_restatement as rr
import inputs
import nets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x100000007  # both key words non-zero
INDEX = (0, 5, 70000)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _quantise(x):
    return np.round((np.clip(x, -1.0, 1.0) + 1.0) * 127.5).astype(np.uint8)


_IMAGES = {}


def _images(n, size=64):
    """uint8 [n,3,size,size] on the host (numpy), computed once per size and shared"""
    have = _IMAGES.get(size, np.zeros((0, 3, size, size), dtype=np.uint8))
    if len(have) < n:
        more = [_quantise(inputs.smooth_image(size, 100 + i)[0].numpy().astype(np.float64)) for i in range(len(have), n)]
        have = _IMAGES[size] = np.concatenate([have, np.stack(more)])
    return have[:n]


def _noisy_rc(u8, index, sigma, level, seed, out=None):
    from free_hunch_amd import _lib
    lib = _lib.load()
    n, S = u8.shape[0], u8.shape[-1]
    out = torch.full(tuple(u8.shape), float("nan"), dtype=torch.float32, device=u8.device) if out is None else out
    idx = (ctypes.c_int64 * len(index))(*index)
    rc = lib.fh_noisy_u8(u8.data_ptr(), idx, n, S, float(sigma), level, seed, out.data_ptr(), _lib.stream())
    return rc, out


def _noisy(u8, index, sigma, level=3, seed=SEED):
    rc, out = _noisy_rc(u8, index, sigma, level, seed)
    assert rc == 0
    return out.cpu().numpy()


def _sqerr(D, u8):
    from free_hunch_amd import _lib
    lib = _lib.load()
    n, S = u8.shape[0], u8.shape[-1]
    words = int(lib.fh_sqerr_u8_scratch_doubles(n, S))
    assert words >= n
    scratch = torch.full((words,), float("nan"), dtype=torch.float64, device=u8.device)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=u8.device)
    _lib.check(lib.fh_sqerr_u8(D.data_ptr(), u8.data_ptr(), n, S, scratch.data_ptr(), out.data_ptr(), _lib.stream()), "fh_sqerr_u8")
    return out.cpu().numpy()


# ---------------------------------------------------------------- fh_noisy_u8
def test_noisy_matches_the_restatement_to_one_ulp(dev):
    u8 = _images(3)
    got = _noisy(torch.from_numpy(u8).to(dev), INDEX, 1.7)
    ref = rr.noisy(u8, INDEX, 3, 1.7, SEED)
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape == (3, 3, 64, 64)
    differ = int((got != ref).sum())
    worst = float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)).max())
    print(f"fh_noisy_u8 vs restatement: {differ} of {got.size} elements not bitwise equal, worst {worst:.2f} ulp", flush=True)
    assert np.isfinite(got).all()
    assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)).all()
    noise = (got.astype(np.float64) - rr.x32(u8)) / 1.7  # and it is unit noise on top of the image, not the image alone
    assert abs(noise.mean()) <= 5 / np.sqrt(noise.size) + 1e-6 and abs(noise.var() - 1) <= 5 * np.sqrt(2 / noise.size) + 1e-6


def test_noise_is_keyed_by_seed_image_level_only(dev):
    u8 = torch.from_numpy(_images(3)).to(dev)
    full = _noisy(u8, INDEX, 1.7)
    alone = _noisy(u8[2:3].contiguous(), INDEX[2:], 1.7)
    assert np.array_equal(alone[0], full[2])  # n = 1 against slot 2 of n = 3
    rev = _noisy(u8.flip(0).contiguous(), INDEX[::-1], 1.7)
    assert np.array_equal(rev[::-1], full)  # another order
    many = _noisy(u8.repeat(7, 1, 1, 1)[:20].contiguous(), (INDEX * 7)[:20], 1.7)  # more images than one launch carries
    assert np.array_equal(many[:3], full) and np.array_equal(many[18], full[0]) and np.array_equal(many[19], full[1])
    for other in (_noisy(u8, INDEX, 1.7, seed=SEED + 1), _noisy(u8, INDEX, 1.7, seed=SEED + (1 << 32)),
                  _noisy(u8, INDEX, 1.7, level=4), _noisy(u8, (0, 5, 70001), 1.7)[2:]):
        assert (other != full[-len(other):]).mean() > 0.99
    same_image = _noisy(u8[:1].repeat(2, 1, 1, 1).contiguous(), (1, 2), 1.7)
    assert (same_image[0] != same_image[1]).mean() > 0.99  # the image index is in the key, not the pixels


def test_sigma_zero_returns_the_encoded_image(dev):
    from free_hunch_amd.sampler import StandardRGBEncoder
    u8 = _images(3)
    got = _noisy(torch.from_numpy(u8).to(dev), INDEX, 0.0)
    assert np.array_equal(got, rr.x32(u8))
    assert np.array_equal(got, StandardRGBEncoder().encode(torch.from_numpy(u8)).numpy())  # what the sampler sees


def test_noisy_refuses_bad_arguments(dev):
    from free_hunch_amd import _lib
    odd = torch.zeros((1, 3, 63, 63), dtype=torch.uint8, device=dev)
    rc, out = _noisy_rc(odd, (0,), 1.0, 0, 0)
    assert rc == _lib.FH_EINVAL
    u8 = torch.from_numpy(_images(2)).to(dev)
    keep = torch.full((2, 3, 64, 64), 7.0, dtype=torch.float32, device=dev)
    for index in ((0, -1), (1 << 32, 0)):
        assert _noisy_rc(u8, index, 1.0, 0, 0, out=keep)[0] == _lib.FH_EINVAL
    assert _noisy_rc(u8, ((1 << 32) - 1, 0), 1.0, 0, 0, out=keep.clone())[0] == 0  # the largest index
    lib = _lib.load()
    idx = (ctypes.c_int64 * 2)(0, 1)
    assert lib.fh_noisy_u8(u8.data_ptr(), idx, 0, 64, 1.0, 0, 0, keep.data_ptr(), _lib.stream()) == _lib.FH_EINVAL
    assert lib.fh_noisy_u8(u8.data_ptr(), idx, 2, 64, -1.0, 0, 0, keep.data_ptr(), _lib.stream()) == _lib.FH_EINVAL
    assert lib.fh_noisy_u8(u8.data_ptr(), idx, 2, 64, 1.0, 0, 0, keep.data_ptr() + 4, _lib.stream()) == _lib.FH_EINVAL
    assert lib.fh_noisy_u8(None, idx, 2, 64, 1.0, 0, 0, keep.data_ptr(), _lib.stream()) == _lib.FH_EINVAL
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all())  # a refused call writes nothing
    assert lib.fh_sqerr_u8_scratch_doubles(2, 63) == 0
    d = torch.zeros(2, dtype=torch.float64, device=dev)
    assert lib.fh_sqerr_u8(keep.data_ptr(), odd.data_ptr(), 1, 63, d.data_ptr(), d.data_ptr(), _lib.stream()) == _lib.FH_EINVAL


# ---------------------------------------------------------------- fh_sqerr_u8
@pytest.mark.parametrize("S, n", [(64, 5), (256, 8)])
def test_sqerr_matches_numpy_and_is_slot_independent(dev, S, n):
    u8 = _images(n, S)
    D = torch.randn((n, 3, S, S), generator=torch.Generator().manual_seed(S + n), dtype=torch.float32)
    u8d, Dd = torch.from_numpy(u8).to(dev), D.to(dev)
    got = _sqerr(Dd, u8d)
    ref = rr.sqerr(D.numpy(), u8)
    rel = float((np.abs(got - ref) / ref).max())
    print(f"fh_sqerr_u8 S = {S}, n = {n}: sums {ref.min():.6g} .. {ref.max():.6g}, worst relative difference {rel:.3e}", flush=True)
    assert (ref > 0.5 * 3 * S * S).all() and rel <= 1e-12
    alone = _sqerr(Dd[3:4].contiguous(), u8d[3:4].contiguous())
    assert alone[0] == got[3]  # bitwise: alone and at slot 3
    rev = _sqerr(Dd.flip(0).contiguous(), u8d.flip(0).contiguous())
    assert np.array_equal(rev[::-1], got)
    x = torch.from_numpy(rr.x32(u8)).to(dev)
    assert (_sqerr(x, u8d) == 0).all()  # D = x32: exactly 0
    one = x.clone()
    one[n - 1, 2, S - 1, S - 1] += 0.5  # the last element of the last image is inside the sum
    last = _sqerr(one, u8d)
    assert (last[:-1] == 0).all() and abs(last[-1] - 0.25) <= 1e-6


# ---------------------------------------------------------------- end to end, closed-form denoiser
def _write_pngs(root, u8):
    import PIL.Image
    os.makedirs(root, exist_ok=True)
    for i, im in enumerate(u8):
        PIL.Image.fromarray(im.transpose(1, 2, 0)).save(os.path.join(root, f"img_{i:03d}.png"))


def test_tool_with_a_batch_independent_denoiser(dev, tmp_path, capsys):
    """`main` with nets.gauss_net (elementwise float64 torch ops: no dependence on the batch) injected: 5 images, batch 2 (a ragged
    last batch), 6 levels plus sigma = 0.  GaussPriorNet overrides the preconditioner's forward, so there is no clamp on either
    side.  Every entry within 1e-6 relative of the restatement, the sigma = 0 row exactly 0, and the file of --batch 5 bitwise
    the file of --batch 2."""
    from free_hunch_amd import recon_mse as rm
    u8 = _images(5)
    data = str(tmp_path / "data")
    _write_pngs(data, u8)
    net = nets.gauss_net(64, dev)
    stats = str(tmp_path / "stats.npz")
    rm.main(["--data", data, "--size", "64", "--num", "5", "--batch", "2", "--levels", "6", "--seed", "9",
             "--stats-out", stats], net=net)
    rm.main(["--data", data, "--size", "64", "--num", "5", "--batch", "5", "--levels", "6", "--seed", "9",
             "--out", str(tmp_path / "b5.pt")], net=net)
    sig = rm.levels_grid(6)
    ref = rr.errors(rr.gauss_denoise(inputs.GAUSS_PRIOR_VAR), u8, range(5), sig, range(7), 9)
    got = np.load(stats)["errors"]
    assert got.shape == ref.shape == (7, 5) and got.dtype == np.float64
    rel = np.abs(got[:-1] - ref[:-1]) / ref[:-1]
    rows = ref.mean(1)
    print(f"table vs restatement: worst relative difference {float(rel.max()):.3e}; row means {rows[0]:.4g} .. {rows[-2]:.4g}",
          flush=True)
    assert (rel <= 1e-6).all()
    assert (got[-1] == 0).all() and (ref[-1] == 0).all()  # sigma = 0
    assert rows[:-1].max() > 10 * rows[:-1].min()  # a result that ignores sigma, or divides by another count, cannot pass
    t = rm.load_table(os.path.join(data, "recon_mse.pt"))
    assert torch.equal(t["errors"], torch.from_numpy(got).float()) and torch.equal(t["sigmas"], sig.float())
    assert open(os.path.join(data, "recon_mse.pt"), "rb").read() == open(tmp_path / "b5.pt", "rb").read()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("recon_mse:")]
    assert len(lines) == 2 and "5 images at 64 x 64, 7 levels" in lines[0]
    # --sigma-max keeps the numbers of the levels it keeps
    rm.main(["--data", data, "--size", "64", "--num", "5", "--batch", "3", "--levels", "6", "--seed", "9", "--sigma-max", "0.2",
             "--out", str(tmp_path / "low.pt")], net=net)
    low = rm.load_table(str(tmp_path / "low.pt"))
    assert torch.equal(low["sigmas"], t["sigmas"][3:]) and torch.equal(low["errors"], t["errors"][3:])


# ---------------------------------------------------------------- end to end, the HIP UNet
def test_level_errors_through_the_hip_unet(dev):
    """level_errors with the HIP UNet (SMALL_A, damped weights) behind the preconditioner, 4 images in one batch, 3 levels,
    against the same net called from torch on the restated x_t in the same batch and the numpy squared error: 1e-6 relative.
    This pins layout and plumbing (NCHW order, the sigma that reaches the net, the image each sum belongs to), not arithmetic."""
    from free_hunch_amd import recon_mse as rm
    u8 = _images(4)
    net = nets.damped_hip_net(inputs.SMALL_A, 11, dev)
    grid = rm.levels_grid(6)
    ids = [2, 3, 4]
    index = [3, 0, 12, 7]
    got = rm.level_errors(net, torch.from_numpy(u8).to(dev), index, grid[ids], ids, 21).cpu().numpy()

    def denoise(x_t, sigma):
        with torch.no_grad():
            return net(torch.from_numpy(x_t).to(dev), torch.tensor(sigma, dtype=torch.float64, device=dev))[0].float().cpu().numpy()

    ref = rr.errors(denoise, u8, index, grid[ids], ids, 21)
    rel = np.abs(got - ref) / ref
    print(f"HIP UNet table vs torch-side restatement: worst relative difference {float(rel.max()):.3e}; "
          f"errors {ref.min():.4g} .. {ref.max():.4g}", flush=True)
    assert got.shape == (3, 4) and (ref > 0).all() and (rel <= 1e-6).all()
    # the images differ by far more than the tolerance at every level (100 x 1e-6 relative), so a swapped column would show
    assert (np.abs(ref[:, 0] - ref[:, 1]) > 1e-4 * ref[:, :2].max(1)).all()


# ---------------------------------------------------------------- consumers
def _small_table(path, value):
    sig = torch.tensor([80.0, 1.0, 0.15, 0.05, 0.0])
    torch.save({"sigmas": sig, "mse_list": torch.tensor([0.2, 0.1, value, value / 2, 0.0])}, path)
    return path


def test_mechanisms_hold_the_table_they_are_given(dev, tmp_path):
    from free_hunch_amd import recon_mse as rm
    from free_hunch_amd.conditioning_mechanisms import choose_conditioning_mechanism
    from free_hunch_amd.sampler import _make_mechanism
    from test_hip_parity import _base_kwargs, _hip_op
    path = _small_table(str(tmp_path / "recon_mse.pt"), 0.0123)
    op = _hip_op("gaussian_blur", 64, dev)
    d = 3 * 64 * 64
    shipped = rm.load_table()
    kw = dict(max_vector_count=100000, image_base_covariance="identity", denoiser_mean_error_threshold=0.2,
              use_analytical_score_time_update=True, project_to_diagonal=False, space_step_update_threshold=10.0,
              space_step_update_lower_threshold=1.0, max_rtol=1.0, do_space_updates=True, solver_type="customcuda")
    cls = choose_conditioning_mechanism("online_covariance")
    own = cls(1.0, op, False, 1, 80.0 ** 2, d, recon_mse_path=path, **kw)
    assert float(own.recon_mse["mse_list"][2]) == pytest.approx(0.0123) and own.recon_mse["sigmas"].numel() == 5
    assert cls(1.0, op, False, 1, 80.0 ** 2, d, **kw).recon_mse is shipped
    for name in ("online_covariance", "peng_analytic"):  # and through the sampler's constructor call
        o = _base_kwargs(str(tmp_path), {"conditioning_mechanism": name, "image_base_covariance": "identity"})
        assert _make_mechanism(o, op, 80.0, d).recon_mse is shipped
        assert _make_mechanism({**o, "recon_mse_path": path}, op, 80.0, d).recon_mse is rm.load_table(path)


def test_cli_uses_and_names_the_datasets_table(tmp_path, capsys):
    """One image, three Euler steps, Peng-analytic (it reads the table at the last step, sigma < 0.2) over a dataset folder with
    its own recon_mse.pt: the run prints the line naming that file and the plugin holds it."""
    import PIL.Image
    sys.path.insert(0, ROOT)
    from bench import smooth_images
    import generate_conditional as gc
    from free_hunch_amd.sampler import conditional_sampler
    data = tmp_path / "data"
    data.mkdir()
    PIL.Image.fromarray(smooth_images(1, 256, 9)[0].permute(1, 2, 0).numpy(), "RGB").save(data / "img00000000.png")
    path = _small_table(str(data / "recon_mse.pt"), 0.0321)
    out = tmp_path / "out"
    gc.main([f"--outdir={out}", f"--dataset_path={data}", "--synthetic_weights=ffhq", "--num_steps=3", "--total_images=1",
             "--max_batch_size=1", "--operator_name=gaussian_blur", "--solver=euler", "--conditioning_mechanism=peng_analytic"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("recon_mse:")]
    assert lines == [f"recon_mse: {path}"], lines
    mech = conditional_sampler.last_mechanism
    assert float(mech.recon_mse["mse_list"][2]) == pytest.approx(0.0321)
    assert "PSNR" in open(out / "results.txt").read()
