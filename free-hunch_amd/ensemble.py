"""Posterior ensembles: K samples of ONE measurement, and what their spread says about it.

A unit of the CLI is (image, seed); with `--posterior_samples=K` it has K members.  The unit's key seeds everything that defines the
inverse problem - the operator's random content (an inpainting mask, a k-space pattern) and the measurement with its noise - so
the members share it bit for bit; member k differs in its initial noise alone (and in the churn noise of the per-image route),
seeded with `member_seed(key, k)` (`noise_seed` is its 32-bit form for torch's CPU generator).  Member 0 is the run without the flag.

`ensemble_stats` (fh_ensemble_stats, csrc/fh_ensemble.hip) turns the samples into the mean image (the MMSE estimate), the
per-pixel standard deviation and, against a ground truth, the calibration sums: spread^2, skill^2 and the covered fractions at
1 and 2 sigma.  The truth is judged as a (K + 1)-th draw: about the mean of K draws it has variance s^2 (1 + 1/K)."""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib

MAX_MEMBERS = 64  # fh_ensemble_stats: 2 <= K <= 64

EnsembleStats = namedtuple("EnsembleStats", "mean_u8 std spread2 skill2 cover1 cover2")


def ensemble_stats(x, truth=None):
    """x: float64 samples [K,C,H,W] (one ensemble) or [N,K,C,H,W] in the sampler's units, on the device; truth: uint8 [C,H,W] /
    [N,C,H,W] or None.  Returns EnsembleStats: mean_u8 uint8 and std float32 (8-bit units) shaped like one image per ensemble;
    spread2, skill2, cover1, cover2 float64 [N] (0-d for one ensemble), the last three -1 without a truth."""
    if not x.is_cuda or (truth is not None and not truth.is_cuda):
        raise _lib.FhError("ensemble_stats runs on the device (libfh_hip.so); there is no CPU fallback")
    assert x.dtype == torch.float64 and x.dim() in (4, 5), "x: float64 [K,C,H,W] or [N,K,C,H,W]"
    single = x.dim() == 4
    x = (x[None] if single else x).contiguous()
    N, K = x.shape[:2]
    img = tuple(x.shape[2:])
    n = int(np.prod(img))
    if truth is not None:
        assert truth.dtype == torch.uint8 and tuple(truth.shape) == (img if single else (N,) + img), "truth: uint8, one image per ensemble"
        truth = truth.contiguous()
    lib = _lib.load()
    mean_u8 = torch.empty((N,) + img, dtype=torch.uint8, device=x.device)
    std = torch.empty((N,) + img, dtype=torch.float32, device=x.device)
    scratch = torch.empty(max(1, int(lib.fh_ensemble_scratch_doubles(N, n))), dtype=torch.float64, device=x.device)
    out = torch.empty((N, 4), dtype=torch.float64, device=x.device)
    _lib.check(lib.fh_ensemble_stats(x.data_ptr(), None if truth is None else truth.data_ptr(), N, K, n, mean_u8.data_ptr(),
                                     std.data_ptr(), scratch.data_ptr(), out.data_ptr(), _lib.stream()), "fh_ensemble_stats")
    pick = (lambda t: t[0]) if single else (lambda t: t)
    return EnsembleStats(pick(mean_u8), pick(std), *(pick(out[:, j]) for j in range(4)))


def unit_key(image_index, seed):
    """The RNG key of the unit (image, seed), below 2^31: independent of the world size."""
    return (seed * 1000003 + image_index) % (1 << 31)


def member_seed(key, k):
    """The seed of member k's own noise.  key < 2^31, so the values of different (key, k) never collide; member 0 has the key."""
    return key + (k << 31)


def noise_seed(key, k):
    """`member_seed(key, k)` folded to the 32 bits torch's CPU generator reads: mt19937 is seeded with the low word of a seed, so
    member_seed itself would give members k and k + 2 the same noise.  low word + high word * 0x9E3779B1 (odd) mod 2^32 is the key
    for member 0 and distinct for the 64 members of a unit (the high word is k >> 1 < 32, the low word key or key + 2^31)."""
    s = member_seed(key, k)
    return ((s & 0xFFFFFFFF) + (s >> 32) * 0x9E3779B1) & 0xFFFFFFFF


def member_noise(key, k, S):
    """Member k's initial noise [1,3,S,S] float32 (CPU generator: the same values on every device); member 0's is the noise of
    the run without ensembles, torch.randn(generator=torch.Generator().manual_seed(key))."""
    return torch.randn((1, 3, S, S), generator=torch.Generator().manual_seed(noise_seed(key, k)), dtype=torch.float32)


def list_units(image_indices, seeds, members=1):
    """(image, seed, member) in the order the CLI runs them: the reference repeats every image once per seed
    (generate_conditional.py:378-390), and the members of a unit are adjacent."""
    return [(i, sd, k) for i in image_indices for sd in seeds for k in range(members)]


def default_groups(batch):
    """Lock-step groups per GPU: two from 4 images on (the Free Hunch phase of one overlaps the UNet phase of the other: +7 % at
    batch 8 on MI355X); FH_LOCKSTEP_GROUPS=1 runs the batch as one group."""
    return int(os.environ.get("FH_LOCKSTEP_GROUPS", "2")) if batch >= 4 else 1


def build_batch(o, files, chunk, S, device, carry=None):
    """What one lock-step batch of the CLI needs.  `o`: the config namespace, `files`: the image listing, `chunk`: (image, seed,
    member) triples.  Returns (ops, ys, noise, imgs, carry): per position b an operator carrying ctx_slot = b, its measurement,
    the member's initial noise [1,3,S,S] float32 (CPU) and the uint8 ground truth [3,S,S] (CPU).

    Every member re-seeds the global generators with the UNIT's key before its operator is built, so the members' random content
    (inpainting mask, k-space pattern) is identical; the measurement is drawn once, by the first member of the unit in the batch,
    and the others take that tensor.  `carry` = the batch's last unit and its measurement: hand it to the next call and
    an ensemble that straddles two batches keeps its measurement."""
    from .measurements import get_operator, poisson_gaussian_sigma
    from .pipeline import load_image_u8
    from .sampler import StandardRGBEncoder
    enc = StandardRGBEncoder()
    ops, ys, noise, imgs = [], [], [], []
    for b, (i, sd, k) in enumerate(chunk):
        key = unit_key(i, sd)
        np.random.seed(key)
        torch.manual_seed(key)
        op_kw = dict(device=device, sigma_s=o.noise_sigma, kernel_size=o.kernel_size, intensity=o.intensity,
                     scale_factor=o.scale_factor, in_shape=(1, 3, S, S), kernel_path=o.kernel_path or None,
                     mask_path=o.mask_path or None, mask_border=o.mask_border, frame_shifts=o.frame_shifts or None,
                     frame_sigmas=o.frame_sigmas or None, mosaic=o.mosaic or None,
                     blend_path=o.blend_path or None, psf_grid=o.psf_grid or None,
                     pattern=o.kspace_pattern or None, acceleration=o.kspace_acceleration,
                     center_fraction=0.08 if o.kspace_center_fraction is None else o.kspace_center_fraction,
                     seed=0 if o.kspace_seed is None else o.kspace_seed,
                     mask_opt={"mask_type": o.inpainting_type, "mask_len_range": (64, 156),
                               "mask_prob_range": (o.inpainting_prob_lower, o.inpainting_prob_upper)
                               if o.inpainting_type == "random" else (0.1, 0.3), "image_size": S})
        img = load_image_u8(files[i], S)
        x_true = enc.encode(img[None].to(device))
        y, raw = carry[1:] if carry is not None and carry[0] == (i, sd) else (None, None)  # an earlier member's measurement
        clean_name = {"weighted_blur": "custom_blur", "weighted_sr": "custom_sr", "weighted_burst_sr": "burst_sr"}
        if o.operator_name in clean_name and o.noise_gain is not None:
            # a Poisson-Gaussian sensor: the measurement is synthesised here with the noise level of the clean signal A0 x,
            # and the solver gets the map estimated from the measurement itself - what a user with real data would have
            if raw is None:
                clean = get_operator(name=clean_name[o.operator_name], **op_kw)
                clean.ctx_slot = b
                ax = clean.forward(x_true, noiseless=True)
                raw = ax + poisson_gaussian_sigma(ax, o.noise_gain, o.noise_read_sigma) * torch.randn_like(ax)
            op = get_operator(name=o.operator_name, noise_map=poisson_gaussian_sigma(raw, o.noise_gain, o.noise_read_sigma),
                              **op_kw)
            y = raw * op.mask.to(raw.dtype)  # (all ones without a mosaic: a raw frame reads 0 off its pattern)
        else:
            op = get_operator(name=o.operator_name, noise_map_path=o.noise_map_path or None, **op_kw)
        op.ctx_slot = b
        if y is None:
            y = op.forward(x_true, noiseless=False)
        carry = ((i, sd), y, raw)
        imgs.append(img)
        ops.append(op)
        ys.append(y)
        noise.append(member_noise(key, k, S))
    return ops, ys, noise, imgs, carry


_CHURN_KEYS = ("S_churn", "S_min", "S_max", "S_noise")


def sample_batch(net, operators, ys, noise, groups=None, churn_seeds=None, **kw):
    """One batch through the sampler the CLI chooses: `conditional_sampler_grouped` (lock-step, `groups` groups) for
    online_covariance without churn, else image by image through `conditional_sampler` (batch 1, as in the reference), the churn
    noise of image b from a device generator seeded with churn_seeds[b].  operators[b] carries ctx_slot = b; noise: [B,3,S,S]
    float32 or a list of [1,3,S,S]; **kw: the loop's and the plugin's options.  Returns x [B,3,S,S] float64."""
    from .sampler import conditional_sampler, conditional_sampler_grouped
    noise = torch.cat(list(noise)) if isinstance(noise, (list, tuple)) else noise
    device = ys[0].device
    churn = {k: kw.pop(k) for k in _CHURN_KEYS if k in kw}
    if kw["conditioning_mechanism"] == "online_covariance" and churn.get("S_churn", 0) == 0:
        groups = default_groups(len(operators)) if groups is None else groups
        return conditional_sampler_grouped(net, noise.to(device), list(ys), list(operators), groups=groups, **kw)
    churn_seeds = [0] * len(operators) if churn_seeds is None else churn_seeds
    gens = [torch.Generator(device).manual_seed(s) for s in churn_seeds]
    return torch.cat([conditional_sampler(
        net, noise[b:b + 1].to(device), None, None, **churn, measurement=ys[b], operator=operators[b],
        randn_like=lambda t, g=gens[b]: torch.randn(t.shape, generator=g, dtype=t.dtype, device=t.device),
        **kw)[0].detach() for b in range(len(operators))])


def sample_ensemble(net, operators, y, noise, groups=None, churn_seeds=None, **kw):
    """K posterior samples of the ONE measurement y: operators = K operator objects of the same content, operator k carrying
    ctx_slot = k; noise [K,3,S,S] float32, one initial noise per member.  Returns [K,3,S,S] float64 (`ensemble_stats` reads it)."""
    return sample_batch(net, operators, [y] * len(operators), noise, groups=groups, churn_seeds=churn_seeds, **kw)
