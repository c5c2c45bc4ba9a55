"""DCT-variance prior from a set of images (reference: do_frequency_analysis.py:1-72): the per-coefficient variance
E[z^2] - E[z]^2 of the orthonormal 2-D DCT z of images scaled to [-1, 1] - the `dct_variance.pt` that
`CovarianceHessianBFGSDCT` loads (online_update_bfgs.py:343).

    python -m free_hunch_amd.frequency_analysis --data DIR [--num 500] [--size 256] [--out DIR/dct_variance.pt]
                                                [--batch 32] [--workers 8] [--stats-out FILE.npz]

reads the first `--num` images of DIR (`pipeline.list_images` order), resizes them as the reference's transform does
(PIL, RGB, bilinear) and accumulates sum z and sum z^2 on the GPU (`fh_dct_moments_u8`: uint8 ingest, the `fh_dct2d`
passes, one thread per coefficient pair adding the images in index order).  Under torchrun image i goes to rank
i mod world and the ranks exchange one packed float64 buffer [sum | sumsq | count] in a single all_reduce.

The sums and the variance are float64; the file holds the variance cast to float32, as the reference saves it.  The
reference accumulates in float32: its own arithmetic is about 4e-6 relative (per element, worst case on smooth test
images) away from float64, so a file written here agrees with one the reference wrote to that rounding, not bit for bit.

`dct_variance()` below is the older helper and returns the SECOND MOMENT E[z^2], which is not what the sampler's prior
is; use `dct_prior()`."""
from __future__ import annotations

import os
from collections import namedtuple

import torch

from . import _lib

Moments = namedtuple("Moments", "sum sumsq count")  # float64 [3,S,S], float64 [3,S,S], int


def dct_variance(images_u8, device="cuda", batch=16):
    """images_u8: uint8 [N,3,S,S] (CPU or GPU).  Returns float32 [3,S,S] = mean over images of dct2(x)^2 with
    x = u8 / 127.5 - 1: the second moment E[z^2].  The reference saves the variance E[z^2] - E[z]^2
    (do_frequency_analysis.py:52-53), which is much smaller at DC and the low frequencies: `dct_prior` computes that."""
    N, C, S, S2 = images_u8.shape
    assert C == 3 and S == S2
    dev = torch.device(device)
    ctx = _lib.Context.get(S, 3 * batch, 0, slot=1000)
    acc = torch.zeros(3, S, S, dtype=torch.float64, device=dev)
    for s in range(0, N, batch):
        x = images_u8[s: s + batch].to(dev).to(torch.float64) / 127.5 - 1
        n = x.shape[0]
        if n < batch:  # keep the plane count the context was built for
            x = torch.cat([x, torch.zeros(batch - n, 3, S, S, dtype=torch.float64, device=dev)])
        z = ctx.dct2d(x.contiguous())
        acc += (z[:n] ** 2).sum(0)
    return (acc / N).to(torch.float32)


def empty_moments(S, device):
    z = torch.zeros(2, 3, S, S, dtype=torch.float64, device=device)
    return Moments(z[0], z[1], 0)


def dct_moments(images_u8, device="cuda", batch=32, state=None):
    """Adds the DCT moments of images_u8 (uint8 [N,3,S,S], CPU or GPU) to `state` (None: zeros) on `device` and returns
    the new state.  The state's tensors are updated in place by the kernel, every coefficient adds the images in index
    order: the sums do not depend on `batch` or on how a stream of images is split into calls."""
    N, C, S, S2 = images_u8.shape
    if images_u8.dtype != torch.uint8 or C != 3 or S != S2:
        raise ValueError(f"expected uint8 [N,3,S,S], got {images_u8.dtype} {tuple(images_u8.shape)}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.FhError("dct_moments runs on the GPU (there is no CPU fallback)")
    with torch.cuda.device(dev):
        if state is None:
            state = empty_moments(S, dev)
        ctx = _lib.Context.get(S, 3 * batch, 0, slot=1001)
        work = torch.empty(min(batch, max(N, 1)) * 3 * S * S, dtype=torch.float64, device=dev)
        for s in range(0, N, batch):
            x = images_u8[s: s + batch].to(dev, non_blocking=True).contiguous()
            ctx.dct_moments_u8(x, work, state.sum, state.sumsq)
    return Moments(state.sum, state.sumsq, state.count + N)


def merge(states):
    """Sum of partial moments (e.g. one state per rank)."""
    states = list(states)
    return Moments(torch.stack([s.sum for s in states]).sum(0), torch.stack([s.sumsq for s in states]).sum(0),
                   sum(int(s.count) for s in states))


def finalize(state):
    """(mean, variance), float64 [3,S,S]: mean = sum / N, variance = sumsq / N - mean^2 (do_frequency_analysis.py:52-53
    in float64).  Raises ValueError for N < 2 and if any variance is not strictly positive (beyond float64's rounding
    of sumsq / N): the sampler divides by this diagonal."""
    N = int(state.count)
    if N < 2:
        raise ValueError(f"a variance needs at least 2 images, got {N}")
    mean = state.sum.to(torch.float64) / N
    m2 = state.sumsq.to(torch.float64) / N
    var = m2 - mean ** 2
    # zero, negative or NaN - or positive only as rounding residue of the subtraction (identical images leave either sign)
    bad = ~(var > 4 * 2.0 ** -52 * m2)
    if bool(bad.any()):
        raise ValueError(f"{int(bad.sum())} of {var.numel()} DCT coefficients have no positive variance over these {N} "
                         f"images (min {float(var.min()):.3e}): the images are identical or too few")
    return mean, var


def dct_prior(images_u8, device="cuda", batch=32):
    """float32 [3,S,S]: the DCT-variance prior of images_u8 (uint8 [N,3,S,S]), as the reference saves it."""
    return finalize(dct_moments(images_u8, device, batch))[1].to(torch.float32)


# ---- the tool ----------------------------------------------------------------------------------------------------------
def load_image_u8_bilinear(path, size):
    """uint8 [3,size,size] as the reference's transform produces it before ToTensor (do_frequency_analysis.py:12-16):
    PIL, RGB, torchvision's Resize default on PIL images = bilinear.  (pipeline.load_image_u8, the sampler's loader,
    resizes bicubically.)"""
    import numpy as np
    import PIL.Image
    img = PIL.Image.open(path).convert("RGB")
    if img.size != (size, size):
        img = img.resize((size, size), PIL.Image.BILINEAR)
    return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1)


def _pack(state):
    return torch.cat([state.sum.reshape(-1), state.sumsq.reshape(-1),
                      torch.tensor([float(state.count)], dtype=torch.float64, device=state.sum.device)])


def _unpack(buf, S):
    n = 3 * S * S
    return Moments(buf[:n].view(3, S, S), buf[n: 2 * n].view(3, S, S), int(round(float(buf[2 * n]))))


def _save_atomic(path, write):
    """write(file object) into a temporary beside `path`, then rename: covariance._load_cached keys on the modification
    time and a sampler running beside the tool never reads half a file."""
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            write(f)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def run(data, moments_fn, device, num=500, size=256, out=None, batch=32, workers=8, stats_out=None, rank=0, world=1):
    """The whole tool for one rank.  moments_fn(images_u8 [n,3,size,size] on the host, state) -> state accumulates one
    batch (`dct_moments` on the GPU; the CPU tests inject a host function).  Image i of the listing goes to rank
    i mod world; with world > 1 the ranks issue ONE all_reduce of the packed moments and rank 0 writes.  Returns the
    merged Moments on every rank."""
    from concurrent.futures import ThreadPoolExecutor

    import torch.distributed as dist

    from .pipeline import list_images, shard_indices
    device = torch.device(device)
    files = list_images(data)
    if num > 0:
        files = files[:num]
    if not files:
        raise SystemExit(f"no images under {data}")
    out = out or os.path.join(data, "dct_variance.pt")
    mine = shard_indices(len(files), rank, world)
    chunks = [mine[s: s + batch] for s in range(0, len(mine), batch)]
    on_gpu = device.type == "cuda"
    stage = torch.empty((2, batch, 3, size, size), dtype=torch.uint8)  # decode target, two batches deep
    if on_gpu:
        stage = stage.pin_memory()
    copied = [None, None]  # per staging slot: the event after which the device no longer reads it
    state = empty_moments(size, device)

    def decode(dst, path):
        dst.copy_(load_image_u8_bilinear(path, size))

    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
        def submit(k):
            if copied[k % 2] is not None:
                copied[k % 2].synchronize()
            return [pool.submit(decode, stage[k % 2][j], files[i]) for j, i in enumerate(chunks[k])]

        pending = submit(0) if chunks else []
        for k, chunk in enumerate(chunks):
            for f in pending:
                f.result()
            pending = submit(k + 1) if k + 1 < len(chunks) else []  # decoded while the device works on batch k
            state = moments_fn(stage[k % 2][: len(chunk)], state)
            if on_gpu:
                copied[k % 2] = torch.cuda.Event()
                copied[k % 2].record()
    if world > 1:
        buf = _pack(state)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        state = _unpack(buf, size)
    if rank == 0:
        mean, var = finalize(state)
        var32 = var.to(torch.float32).cpu().contiguous()
        _save_atomic(out, lambda f: torch.save(var32, f))
        if stats_out:
            import numpy as np
            _save_atomic(stats_out, lambda f: np.savez(f, mean=mean.cpu().numpy(), variance=var.cpu().numpy(),
                                                       count=np.int64(state.count)))
        dc = ", ".join(f"{float(v):.6g}" for v in var[:, 0, 0])
        print(f"frequency_analysis: {state.count} images at {size} x {size}, DC variance (R, G, B) = ({dc}), "
              f"min variance {float(var.min()):.6g}, wrote {out}", flush=True)
    return state


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m free_hunch_amd.frequency_analysis", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", required=True, help="image folder (searched recursively for .png / .jpg / .jpeg)")
    ap.add_argument("--num", type=int, default=500, help="use the first NUM images of the sorted listing; 0 = all")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None, help="default: DATA/dct_variance.pt")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workers", type=int, default=8, help="decoding threads")
    ap.add_argument("--stats-out", default=None, help="also write float64 mean, variance and count as .npz")
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
        run(a.data, lambda u8, st: dct_moments(u8, device, a.batch, st), device, num=a.num, size=a.size, out=a.out,
            batch=a.batch, workers=a.workers, stats_out=a.stats_out, rank=rank, world=world)
    finally:
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
