"""The per-sigma denoiser-error table `recon_mse.pt`: for every noise level sigma of a grid, the mean squared error per element
(in [-1, 1] units) of the denoiser on images of the dataset, E |D(x + sigma eps, sigma) - x|^2 / (3 S^2).  `use_analytic_var_at_end`
(Free Hunch) and the Peng-analytic baseline replace the covariance below sigma = 0.2 by this scalar (reference:
conditioning_mechanisms.py:87-110, :225-226, :273-276, which ships the ImageNet table and no producer of it).

    python -m free_hunch_amd.recon_mse --data DIR [--num 100] [--size 256] [--out DIR/recon_mse.pt] [--batch 8] [--seed 0]
                                       [--sigma-max X] [--levels K] [--stats-out FILE.npz]
                                       [--openai_state_dict_path F --openai_setup_path F | --synthetic_weights ffhq|imagenet]
                                       [--unet_dtype fp32|bf16|fp16] [--unet_backend hip|torch]

reads the first `--num` images of DIR as the sampler does (`pipeline.list_images`, `pipeline.load_image_u8`) and, for every level,
runs `fh_noisy_u8` -> net(x_t, sigma) -> `fh_sqerr_u8` on the GPU: one sigma per UNet call, the images batched.  The noise is
Philox4x32-10 keyed by (seed, image index, level index of the full grid, element), so a table does not depend on `--batch`, on
`--sigma-max` or on the number of ranks.  Under torchrun image i goes to rank i mod world, every rank fills its columns of a
zero [levels, images] float64 buffer and ONE all_reduce merges them (adding zeros: exact); rank 0 writes.

The file is the reference's dict of float32 tensors: `sigmas [L]` (the EDM grid of K steps from 80 down to 0.01, rho = 7, then 0),
`mse_list [L]` (the float64 mean over images, then cast) and `errors [L, N]`.  Consumers pick the nearest level,
(sigmas - sigma).abs().argmin(), and only below sigma = 0.2: `--sigma-max 0.2` computes just those levels (plus the first above
and sigma = 0), about a fifth of the work."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

F64 = torch.float64
THRESHOLD = 0.2  # consumers read the table below this sigma (mle_sigma_thres)
SHIPPED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "recon_mse.pt")
_TABLES = {}


# ---- levels ------------------------------------------------------------------------------------------------------------
def levels_grid(steps):
    """float64 [steps + 1]: the EDM grid get_sigma_steps("edm", steps, 0.01, 80, 7) (no round_sigma) followed by sigma = 0."""
    from .sampler import get_sigma_steps
    if steps < 2:
        raise ValueError(f"a grid needs at least 2 steps, got {steps}")
    return torch.cat([get_sigma_steps("edm", steps, 0.01, 80.0, 7.0), torch.zeros(1, dtype=F64)])


def default_levels():
    """The 1001 sigma of the shipped table."""
    return levels_grid(1000)


def select_levels(sigmas, sigma_max=None):
    """Indices into `sigmas` (descending, ending in 0) of the levels to compute: all of them, or with `sigma_max` the levels
    <= sigma_max, the first one above it (so that every sigma below sigma_max finds its nearest level in the table) and 0."""
    s = [float(v) for v in sigmas]
    if sigma_max is None:
        return list(range(len(s)))
    keep = [i for i, v in enumerate(s) if v <= sigma_max]
    above = [i for i, v in enumerate(s) if v > sigma_max]
    if above:
        keep.append(min(above, key=lambda i: s[i]))
    return sorted(keep)


# ---- the device loop ---------------------------------------------------------------------------------------------------
def level_errors(net, images_u8, img_index, sigmas, level_ids, seed):
    """float64 [L, n] on the images' device: the per-image mean squared error of net at the L levels.  images_u8: uint8
    [n,3,S,S] on the GPU; img_index: the n global indices of the images (noise key); sigmas, level_ids: the L levels and their
    indices in the full grid (noise key); net(x, sigma) -> (D, ...).  Nothing in the loop waits for the device."""
    if not (torch.is_tensor(images_u8) and images_u8.is_cuda):
        raise _lib.FhError("level_errors runs on the GPU (there is no CPU fallback)")
    n, ch, S, S2 = images_u8.shape
    if images_u8.dtype != torch.uint8 or ch != 3 or S != S2:
        raise ValueError(f"expected uint8 [n,3,S,S], got {images_u8.dtype} {tuple(images_u8.shape)}")
    if len(img_index) != n or len(sigmas) != len(level_ids):
        raise ValueError("one index per image and one level id per sigma")
    lib, dev = _lib.load(), images_u8.device
    imgs = images_u8.contiguous()
    idx = (C.c_int64 * n)(*[int(i) for i in img_index])
    sig = [float(s) for s in sigmas]
    with torch.cuda.device(dev), torch.no_grad():
        sig_dev = torch.tensor(sig, dtype=F64, device=dev)
        x_t = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
        scratch = torch.empty(int(lib.fh_sqerr_u8_scratch_doubles(n, S)), dtype=F64, device=dev)
        out = torch.empty((len(sig), n), dtype=F64, device=dev)
        for k, (s, level) in enumerate(zip(sig, level_ids)):
            _lib.check(lib.fh_noisy_u8(_lib.ptr(imgs), idx, n, S, s, int(level), int(seed) & (2 ** 64 - 1), _lib.ptr(x_t),
                                       _lib.stream()), "fh_noisy_u8")
            D = net(x_t, sig_dev[k])[0].to(torch.float32).contiguous()
            if tuple(D.shape) != (n, 3, S, S):
                raise ValueError(f"the denoiser returned {tuple(D.shape)} for {(n, 3, S, S)}")
            _lib.check(lib.fh_sqerr_u8(_lib.ptr(D), _lib.ptr(imgs), n, S, _lib.ptr(scratch), out[k].data_ptr(), _lib.stream()),
                       "fh_sqerr_u8")
        return out / (3 * S * S)


# ---- the table ---------------------------------------------------------------------------------------------------------
def _validate(sigmas, mse_list, what):
    if sigmas.dim() != 1 or mse_list.dim() != 1 or sigmas.numel() != mse_list.numel() or sigmas.numel() == 0:
        raise ValueError(f"{what}: sigmas and mse_list must be 1-D of one length, got {tuple(sigmas.shape)} and "
                         f"{tuple(mse_list.shape)}")
    if not bool(torch.isfinite(sigmas).all()) or not bool(torch.isfinite(mse_list).all()):
        raise ValueError(f"{what}: non-finite entries")
    if bool((mse_list < 0).any()) or bool((sigmas < 0).any()):
        raise ValueError(f"{what}: negative entries")
    if not bool((sigmas < THRESHOLD).any()):
        raise ValueError(f"{what}: no level below sigma = {THRESHOLD}, the only range in which the table is read")


def finalize(errors, sigmas):
    """errors float64 [L, N] (per level and image), sigmas [L] -> the file's dict {sigmas, mse_list, errors} in float32;
    mse_list is the float64 mean over the images, then cast.  Raises ValueError for fewer than 2 images, non-finite or negative
    entries, and a grid without a level below 0.2."""
    errors = torch.as_tensor(errors).to(F64).cpu()
    sigmas = torch.as_tensor(sigmas).to(F64).cpu().reshape(-1)
    if errors.dim() != 2 or errors.shape[0] != sigmas.numel():
        raise ValueError(f"errors must be [levels, images] with one row per sigma, got {tuple(errors.shape)} for "
                         f"{sigmas.numel()} levels")
    if errors.shape[1] < 2:
        raise ValueError(f"a mean error needs at least 2 images, got {errors.shape[1]}")
    if not bool(torch.isfinite(errors).all()):
        raise ValueError("errors: non-finite entries")
    if bool((errors < 0).any()):
        raise ValueError("errors: negative entries")
    mse = errors.mean(1)
    _validate(sigmas, mse, "recon_mse")
    return {"sigmas": sigmas.to(torch.float32).contiguous(), "mse_list": mse.to(torch.float32).contiguous(),
            "errors": errors.to(torch.float32).contiguous()}


def load_table(path=None):
    """The validated dict of a recon_mse.pt (None: the shipped ImageNet table), read once per (path, modification time) as
    covariance._load_cached does: the plugins are constructed per image."""
    path = SHIPPED if path is None else path
    key = (os.path.abspath(path), os.path.getmtime(path))
    if key not in _TABLES:
        t = torch.load(path, weights_only=True)
        if not isinstance(t, dict) or not {"sigmas", "mse_list"} <= set(t) or not set(t) <= {"sigmas", "mse_list", "errors"}:
            raise ValueError(f"{path}: expected a dict with sigmas, mse_list (and errors), got "
                             f"{sorted(t) if isinstance(t, dict) else type(t).__name__}")
        if not all(torch.is_tensor(v) and v.is_floating_point() for v in t.values()):
            raise ValueError(f"{path}: every entry must be a floating-point tensor")
        _validate(t["sigmas"], t["mse_list"], path)
        if "errors" in t and (t["errors"].dim() != 2 or t["errors"].shape[0] != t["sigmas"].numel()):
            raise ValueError(f"{path}: errors must be [levels, images], got {tuple(t['errors'].shape)}")
        _TABLES[key] = t
    return _TABLES[key]


# ---- the tool ----------------------------------------------------------------------------------------------------------
def run(data, level_fn, device, num=100, size=256, out=None, batch=8, seed=0, sigma_max=None, levels=1000, stats_out=None,
        rank=0, world=1):
    """The whole tool for one rank.  level_fn(images_u8 [n,3,size,size] on the host, img_index, sigmas, level_ids, seed) ->
    float64 [L, n] computes one batch of images at all levels (`level_errors` on the GPU; the CPU tests inject a host function).
    Image i of the listing goes to rank i mod world; with world > 1 the ranks issue ONE all_reduce of the [L, N] buffer and
    rank 0 writes.  Returns (sigmas [L], errors [L, N]) float64 on every rank."""
    import torch.distributed as dist

    from .frequency_analysis import _save_atomic
    from .pipeline import list_images, load_image_u8, shard_indices
    device = torch.device(device)
    files = list_images(data)
    if num > 0:
        files = files[:num]
    if not files:
        raise SystemExit(f"no images under {data}")
    out = out or os.path.join(data, "recon_mse.pt")
    grid = levels_grid(levels)
    level_ids = select_levels(grid, sigma_max)
    sigmas = grid[level_ids]
    mine = shard_indices(len(files), rank, world)
    errors = torch.zeros((len(level_ids), len(files)), dtype=F64, device=device)
    for s in range(0, len(mine), max(1, batch)):
        chunk = mine[s: s + max(1, batch)]
        u8 = torch.stack([load_image_u8(files[i], size) for i in chunk])
        errors[:, chunk] = level_fn(u8, chunk, sigmas, level_ids, seed).to(device)
        print(f"[rank {rank}] images {chunk[0]} .. {chunk[-1]}: {len(level_ids)} levels queued", flush=True)
    if world > 1:
        dist.all_reduce(errors, op=dist.ReduceOp.SUM)
    if rank == 0:
        table = finalize(errors, sigmas)
        _save_atomic(out, lambda f: torch.save(table, f))
        if stats_out:
            import numpy as np
            _save_atomic(stats_out, lambda f: np.savez(f, sigmas=sigmas.numpy(), errors=errors.cpu().numpy(),
                                                       level_ids=np.asarray(level_ids, dtype=np.int64), seed=np.int64(seed)))
        mse, sg = table["mse_list"].double(), [float(v) for v in sigmas]
        below = max((i for i, v in enumerate(sg) if v < THRESHOLD), key=lambda i: sg[i])
        small = min((i for i, v in enumerate(sg) if v > 0), key=lambda i: sg[i])
        top = max(range(len(sg)), key=lambda i: sg[i])
        at = lambda i: f"{float(mse[i]):.6g} at sigma = {sg[i]:.6g}"
        print(f"recon_mse: {len(files)} images at {size} x {size}, {len(sg)} levels, MSE {at(top)} (largest), {at(below)} "
              f"(first below {THRESHOLD}), {at(small)} (smallest non-zero), wrote {out}", flush=True)
    return sigmas, errors


def build_net(a, device):
    """The denoiser of generate_conditional.py, from the same model flags."""
    from . import unet as hu
    from .precond import iDDPMLinearPrecond
    if a.synthetic_weights:
        cfg = {"ffhq": hu.FFHQ256, "imagenet": hu.IMAGENET256}[a.synthetic_weights]
        model = hu.UNetModel(cfg, backend=a.unet_backend, dtype=a.unet_dtype)
        model.load_state_dict(hu.seeded_state(cfg, 0))
    else:
        model, cfg = hu.load_model(a.openai_state_dict_path, a.openai_setup_path, backend=a.unet_backend,
                                   dtype=None if a.unet_dtype == "fp32" else a.unet_dtype)
    return iDDPMLinearPrecond(model.to(device).eval(), cfg.image_size, 3).to(device)


def main(argv=None, net=None):
    """`net`: a denoiser to use instead of the one the model flags describe (any net(x, sigma) -> (D, ...) on the device)."""
    import argparse

    from .config import SCHEMA
    ap = argparse.ArgumentParser(prog="python -m free_hunch_amd.recon_mse", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", required=True, help="image folder (searched recursively for .png / .jpg / .jpeg)")
    ap.add_argument("--num", type=int, default=100, help="use the first NUM images of the sorted listing; 0 = all")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None, help="default: DATA/recon_mse.pt")
    ap.add_argument("--batch", type=int, default=8, help="images per UNet call")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sigma-max", type=float, default=None,
                    help="only the levels <= X, the first above X and 0 (0.2 covers everything the sampler reads)")
    ap.add_argument("--levels", type=int, default=1000, help="steps of the EDM grid 80 .. 0.01 (sigma = 0 is appended)")
    ap.add_argument("--stats-out", default=None, help="also write float64 sigmas, errors, level ids and the seed as .npz")
    for key in ("openai_state_dict_path", "openai_setup_path", "synthetic_weights", "unet_dtype", "unet_backend"):
        ap.add_argument(f"--{key}", default=SCHEMA[key][1])
    a = ap.parse_args(argv)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl")
    try:
        net = build_net(a, device) if net is None else net
        res = getattr(net, "img_resolution", a.size)
        if res != a.size:
            raise SystemExit(f"--size {a.size} does not match the model's resolution {res}")
        run(a.data, lambda u8, idx, sg, ids, seed: level_errors(net, u8.to(device), idx, sg, ids, seed), device, num=a.num,
            size=a.size, out=a.out, batch=a.batch, seed=a.seed, sigma_max=a.sigma_max, levels=a.levels,
            stats_out=a.stats_out, rank=rank, world=world)
    finally:
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
