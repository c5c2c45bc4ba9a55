"""What the Python side hands the solver, pinned per operator configuration: every scalar of `fh_problem`, which tensor of
`keep` every pointer field addresses, and the shape, dtype and contiguity of every `keep` entry - on the DCT and on the identity
basis - against a table recorded once.  Also the per-name facts (op code, stride, the sigma rules, the mask field) and the
refusal of an unknown name.  No GPU: operators are built on device="cpu", the covariance is a stand-in with the attributes
`_problem` reads, and the library's plan functions need no device.  `CONFIGS` and `make` are shared with
test_solver_paths_gpu.py."""
import types

import numpy as np
import pytest
import torch

from test_custom_psf_host import disk_psf
from test_custom_sr_host import binomial_psf

F64 = torch.float64
SCALARS = ("op", "stride", "planes", "d", "ntaps", "halo", "ntaps2", "halo2", "fold_sym", "use_dct", "sigma_y2")
POINTERS = ("D", "r", "B", "M", "tap_dy", "tap_dx", "tap_w", "mask", "tap2_dy", "tap2_dx", "tap2_w",
            "fold_fwd_w", "fold_fwd_h", "fold_inv_w", "fold_inv_h")
NAMES = ("inpainting", "noise", "colorization", "gaussian_blur", "motion_blur", "super_resolution", "custom_blur", "masked_blur",
         "custom_sr", "weighted_blur", "weighted_sr", "burst_sr", "weighted_burst_sr", "varying_blur", "fourier_sampling")


def sparse_psf():
    """9 x 9 with ten non-zeros, not rank-1, normalised: runs on the tap-list kernels"""
    k = np.zeros((9, 9))
    for y, x, w in ((0, 2, 1), (1, 7, 2), (2, 6, 1), (3, 3, 3), (4, 0, 1), (4, 4, 8), (5, 2, 3), (6, 8, 2), (7, 1, 2), (8, 5, 1)):
        k[y, x] = w
    return k / k.sum()


def random_mask(S, seed):
    """0/1 per channel and pixel, about 60 % kept"""
    return (np.random.default_rng(1000 + seed).random((3, S, S)) >= 0.4).astype(np.float64)


def random_noise_map(shape, seed):
    """sigma uniform in 0.03 .. 0.1, inf on about 30 %"""
    rng = np.random.default_rng(2000 + seed)
    sig = rng.uniform(0.03, 0.1, shape)
    sig[rng.random(shape) < 0.3] = np.inf
    return sig


# configuration -> (operator name, keywords as a function of (S, seed)); decimating operators other than super_resolution run x 2
CONFIGS = {
    "inpainting": ("inpainting", lambda S, seed: dict(mask_opt={"image_size": S}, mask=torch.from_numpy(random_mask(S, seed))[None])),
    "noise": ("noise", lambda S, seed: {}),
    "colorization": ("colorization", lambda S, seed: {}),
    "gaussian_blur": ("gaussian_blur", lambda S, seed: dict(kernel_size=61, intensity=3.0)),
    "motion_blur": ("motion_blur", lambda S, seed: dict(kernel_size=61, intensity=0.5)),
    "super_resolution": ("super_resolution", lambda S, seed: {}),
    "custom_blur-binomial": ("custom_blur", lambda S, seed: dict(kernel=binomial_psf(5, 3))),
    "custom_blur-sparse": ("custom_blur", lambda S, seed: dict(kernel=sparse_psf())),
    "custom_blur-disk": ("custom_blur", lambda S, seed: dict(kernel=disk_psf())),
    "masked_blur-sparse": ("masked_blur", lambda S, seed: dict(kernel=sparse_psf(), mask=random_mask(S, seed))),
    "masked_blur-disk": ("masked_blur", lambda S, seed: dict(kernel=disk_psf(), mask=random_mask(S, seed))),
    "masked_blur-binomial-border": ("masked_blur", lambda S, seed: dict(kernel=binomial_psf(5, 3), mask_border=-1)),
    "custom_sr-binomial": ("custom_sr", lambda S, seed: dict(kernel=binomial_psf(5, 3), scale_factor=2)),
    "custom_sr-sparse": ("custom_sr", lambda S, seed: dict(kernel=sparse_psf(), scale_factor=2)),
    "weighted_blur-sparse": ("weighted_blur", lambda S, seed: dict(kernel=sparse_psf(), noise_map=random_noise_map((3, S, S), seed))),
    "weighted_blur-disk": ("weighted_blur", lambda S, seed: dict(kernel=disk_psf(), noise_map=random_noise_map((3, S, S), seed))),
    "weighted_sr-binomial": ("weighted_sr", lambda S, seed: dict(kernel=binomial_psf(5, 3), scale_factor=2,
                                                                 noise_map=random_noise_map((3, S // 2, S // 2), seed))),
    "weighted_sr-sparse": ("weighted_sr", lambda S, seed: dict(kernel=sparse_psf(), scale_factor=2,
                                                               noise_map=random_noise_map((3, S // 2, S // 2), seed))),
    "burst_sr": ("burst_sr", lambda S, seed: dict(kernels=[binomial_psf(5, 3)], frame_shifts=[(0, 0), (1, 0.5)], scale_factor=2)),
    "weighted_burst_sr": ("weighted_burst_sr", lambda S, seed: dict(kernels=[binomial_psf(5, 3)], frame_shifts=[(0, 0), (1, 0.5)],
                                                                    scale_factor=2,
                                                                    noise_map=random_noise_map((6, S // 2, S // 2), seed))),
    "varying_blur": ("varying_blur", lambda S, seed: dict(kernels=[binomial_psf(5, 3), sparse_psf()], psf_grid=(1, 2))),
    "fourier_sampling-pattern": ("fourier_sampling", lambda S, seed: dict(pattern="cartesian", acceleration=4.0, seed=seed)),
    "fourier_sampling-noise_map": ("fourier_sampling", lambda S, seed: dict(pattern="cartesian", acceleration=4.0, seed=seed,
                                                                            noise_map=random_noise_map((S, S), seed))),
}


def make(config, S=64, device="cpu", seed=0, sr_factor=4, sigma_s=0.05):
    """the operator of a configuration on an S x S image; `seed` varies its mask or noise map, `sr_factor` is super_resolution's"""
    from free_hunch_amd.measurements import get_operator
    name, kw = CONFIGS[config]
    kw = kw(S, seed)
    if name == "super_resolution":
        kw["scale_factor"] = sr_factor
    return get_operator(name=name, device=device, sigma_s=sigma_s, in_shape=(1, 3, S, S), **kw)


def stand_in_cov(S, use_dct):
    """what `_problem` and the solves' argument checks read of a covariance"""
    class Cov:
        data_dim, device, ctx = 3 * S * S, torch.device("cpu"), None

        class famC:
            m, B = 0, torch.zeros(1, dtype=F64)

        class C:
            D, r = torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64)
            M_dev = torch.zeros(1, 8, dtype=F64)
    Cov.use_dct, Cov.S = use_dct, S
    return Cov


def snapshot(op, cov):
    """(scalars, 'field=index of its tensor in keep ...' of the non-null pointers - or taps.dy, col.w, ... for a tap list of
    the operator's own `taps` / `taps.sep` - and 'dtype[shape] ...' of keep; '!' = not contiguous, '?' = a pointer to neither)"""
    from free_hunch_amd import conditioning_mechanisms as cm
    p, keep = cm._problem(op, cov, cm._solver_sigma_y2(op))
    where = {}
    for i, t in enumerate(keep):
        where.setdefault(t.data_ptr(), i)
    taps = getattr(op, "taps", None)  # a single PSF's tap lists live on the operator, not in keep
    lists = {"taps": taps, **dict(zip(("col", "row"), getattr(taps, "sep", None) or ()))}
    for label, t in lists.items():
        for f in ("dy", "dx", "w") if t is not None else ():
            where.setdefault(getattr(t, f).data_ptr(), f"{label}.{f}")
    ptrs = " ".join(f"{f}={where.get(getattr(p, f), '?')}" for f in POINTERS if getattr(p, f))
    short = {torch.float64: "f64", torch.float32: "f32", torch.int32: "i32"}
    kept = " ".join(f"{short[t.dtype]}{list(t.shape)}{'' if t.is_contiguous() else '!'}".replace(" ", "") for t in keep)
    return tuple(getattr(p, f) for f in SCALARS), ptrs, kept


# recorded from the commit before the solver table existed: (config, basis) -> snapshot; S = 64, sigma_s = 0.05
EXPECTED = {
    ('inpainting', 'dct'): ((0, 1, 3, 12288, 0, 0, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,64,64]'),
    ('inpainting', 'identity'): ((0, 1, 3, 12288, 0, 0, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,64,64]'),
    ('noise', 'dct'): ((0, 1, 3, 12288, 0, 0, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,64,64]'),
    ('noise', 'identity'): ((0, 1, 3, 12288, 0, 0, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,64,64]'),
    ('colorization', 'dct'): ((3, 1, 3, 12288, 3, 0, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_w=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[3]'),
    ('colorization', 'identity'): ((3, 1, 3, 12288, 3, 0, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_w=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[3]'),
    ('gaussian_blur', 'dct'): ((1, 1, 3, 12288, 25, -13, 25, -113, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=col.dy tap_dx=col.dx tap_w=col.w tap2_dy=row.dy tap2_dx=row.dx tap2_w=row.w fold_fwd_w=4 fold_fwd_h=5 fold_inv_w=6 fold_inv_h=7',
        'f64[1] f64[1] f64[1] f64[1,8] f64[64,64] f64[64,64] f64[64,64] f64[64,64]'),
    ('gaussian_blur', 'identity'): ((1, 1, 3, 12288, 25, -13, 25, -113, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=col.dy tap_dx=col.dx tap_w=col.w tap2_dy=row.dy tap2_dx=row.dx tap2_w=row.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('motion_blur', 'dct'): ((1, 1, 3, 12288, 217, 2864, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('motion_blur', 'identity'): ((1, 1, 3, 12288, 217, 2864, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('super_resolution', 'dct'): ((2, 4, 3, 12288, 625, 1780, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('super_resolution', 'identity'): ((2, 4, 3, 12288, 625, 1780, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('custom_blur-binomial', 'dct'): ((1, 1, 3, 12288, 5, -3, 3, -102, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=col.dy tap_dx=col.dx tap_w=col.w tap2_dy=row.dy tap2_dx=row.dx tap2_w=row.w fold_fwd_w=4 fold_fwd_h=5 fold_inv_w=6 fold_inv_h=7',
        'f64[1] f64[1] f64[1] f64[1,8] f64[64,64] f64[64,64] f64[64,64] f64[64,64]'),
    ('custom_blur-binomial', 'identity'): ((1, 1, 3, 12288, 5, -3, 3, -102, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=col.dy tap_dx=col.dx tap_w=col.w tap2_dy=row.dy tap2_dx=row.dx tap2_w=row.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('custom_blur-sparse', 'dct'): ((1, 1, 3, 12288, 10, 1260, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('custom_blur-sparse', 'identity'): ((1, 1, 3, 12288, 10, 1260, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('custom_blur-disk', 'dct'): ((4, 1, 3, 12288, 1681, 1300, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_w=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[41,41]'),
    ('custom_blur-disk', 'identity'): ((4, 1, 3, 12288, 1681, 1300, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_w=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[41,41]'),
    ('masked_blur-sparse', 'dct'): ((5, 1, 3, 12288, 10, 1260, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,64,64]'),
    ('masked_blur-sparse', 'identity'): ((5, 1, 3, 12288, 10, 1260, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,64,64]'),
    ('masked_blur-disk', 'dct'): ((6, 1, 3, 12288, 1681, 1300, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_w=4 mask=5',
        'f64[1] f64[1] f64[1] f64[1,8] f64[41,41] f64[1,3,64,64]'),
    ('masked_blur-disk', 'identity'): ((6, 1, 3, 12288, 1681, 1300, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_w=4 mask=5',
        'f64[1] f64[1] f64[1] f64[1,8] f64[41,41] f64[1,3,64,64]'),
    ('masked_blur-binomial-border', 'dct'): ((5, 1, 3, 12288, 5, -3, 3, -102, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=col.dy tap_dx=col.dx tap_w=col.w mask=8 tap2_dy=row.dy tap2_dx=row.dx tap2_w=row.w fold_fwd_w=4 fold_fwd_h=5 fold_inv_w=6 fold_inv_h=7',
        'f64[1] f64[1] f64[1] f64[1,8] f64[64,64] f64[64,64] f64[64,64] f64[64,64] f64[1,3,64,64]'),
    ('masked_blur-binomial-border', 'identity'): ((5, 1, 3, 12288, 5, -3, 3, -102, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=col.dy tap_dx=col.dx tap_w=col.w mask=4 tap2_dy=row.dy tap2_dx=row.dx tap2_w=row.w',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,64,64]'),
    ('custom_sr-binomial', 'dct'): ((7, 2, 3, 12288, 15, 1129, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w fold_fwd_w=4 fold_fwd_h=5 fold_inv_w=6 fold_inv_h=7',
        'f64[1] f64[1] f64[1] f64[1,8] f64[64,32] f64[64,32] f64[32,64] f64[32,64]'),
    ('custom_sr-binomial', 'identity'): ((2, 2, 3, 12288, 15, 1129, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('custom_sr-sparse', 'dct'): ((2, 2, 3, 12288, 10, 1260, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('custom_sr-sparse', 'identity'): ((2, 2, 3, 12288, 10, 1260, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
    ('weighted_blur-sparse', 'dct'): ((8, 1, 3, 12288, 10, 1260, 0, 0, 0, 1, 1.0),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,64,64]'),
    ('weighted_blur-sparse', 'identity'): ((8, 1, 3, 12288, 10, 1260, 0, 0, 0, 0, 1.0),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,64,64]'),
    ('weighted_blur-disk', 'dct'): ((9, 1, 3, 12288, 1681, 1300, 0, 0, 0, 1, 1.0),
        'D=0 r=1 B=2 M=3 tap_w=4 mask=5',
        'f64[1] f64[1] f64[1] f64[1,8] f64[41,41] f64[1,3,64,64]'),
    ('weighted_blur-disk', 'identity'): ((9, 1, 3, 12288, 1681, 1300, 0, 0, 0, 0, 1.0),
        'D=0 r=1 B=2 M=3 tap_w=4 mask=5',
        'f64[1] f64[1] f64[1] f64[1,8] f64[41,41] f64[1,3,64,64]'),
    ('weighted_sr-binomial', 'dct'): ((11, 2, 3, 12288, 15, 1129, 0, 0, 0, 1, 1.0),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w mask=8 fold_fwd_w=4 fold_fwd_h=5 fold_inv_w=6 fold_inv_h=7',
        'f64[1] f64[1] f64[1] f64[1,8] f64[64,32] f64[64,32] f64[32,64] f64[32,64] f64[1,3,32,32]'),
    ('weighted_sr-binomial', 'identity'): ((10, 2, 3, 12288, 15, 1129, 0, 0, 0, 0, 1.0),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,32,32]'),
    ('weighted_sr-sparse', 'dct'): ((10, 2, 3, 12288, 10, 1260, 0, 0, 0, 1, 1.0),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,32,32]'),
    ('weighted_sr-sparse', 'identity'): ((10, 2, 3, 12288, 10, 1260, 0, 0, 0, 0, 1.0),
        'D=0 r=1 B=2 M=3 tap_dy=taps.dy tap_dx=taps.dx tap_w=taps.w mask=4',
        'f64[1] f64[1] f64[1] f64[1,8] f64[1,3,32,32]'),
    ('burst_sr', 'dct'): ((12, 2, 3, 12288, 35, 1194, 2, 20, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=4 tap_dx=5 tap_w=6 tap2_dy=7',
        'f64[1] f64[1] f64[1] f64[1,8] i32[35] i32[35] f64[35] i32[3]'),
    ('burst_sr', 'identity'): ((12, 2, 3, 12288, 35, 1194, 2, 20, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=4 tap_dx=5 tap_w=6 tap2_dy=7',
        'f64[1] f64[1] f64[1] f64[1,8] i32[35] i32[35] f64[35] i32[3]'),
    ('weighted_burst_sr', 'dct'): ((13, 2, 3, 12288, 35, 1194, 2, 20, 0, 1, 1.0),
        'D=0 r=1 B=2 M=3 tap_dy=4 tap_dx=5 tap_w=6 mask=8 tap2_dy=7',
        'f64[1] f64[1] f64[1] f64[1,8] i32[35] i32[35] f64[35] i32[3] f64[1,6,32,32]'),
    ('weighted_burst_sr', 'identity'): ((13, 2, 3, 12288, 35, 1194, 2, 20, 0, 0, 1.0),
        'D=0 r=1 B=2 M=3 tap_dy=4 tap_dx=5 tap_w=6 mask=8 tap2_dy=7',
        'f64[1] f64[1] f64[1] f64[1,8] i32[35] i32[35] f64[35] i32[3] f64[1,6,32,32]'),
    ('varying_blur', 'dct'): ((14, 1, 3, 12288, 25, 1260, 2, 15, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=4 tap_dx=5 tap_w=6 tap2_dy=7 tap2_w=8',
        'f64[1] f64[1] f64[1] f64[1,8] i32[25] i32[25] f64[25] i32[3] f64[2,3,64,64]'),
    ('varying_blur', 'identity'): ((14, 1, 3, 12288, 25, 1260, 2, 15, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=4 tap_dx=5 tap_w=6 tap2_dy=7 tap2_w=8',
        'f64[1] f64[1] f64[1] f64[1,8] i32[25] i32[25] f64[25] i32[3] f64[2,3,64,64]'),
    ('fourier_sampling-pattern', 'dct'): ((15, 1, 3, 12288, 0, 0, 0, 0, 0, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 mask=6 fold_fwd_w=4 fold_fwd_h=4 fold_inv_w=5 fold_inv_h=5',
        'f64[1] f64[1] f64[1] f64[1,8] f64[64,64] f64[64,64] f64[1,3,64,64]'),
    ('fourier_sampling-pattern', 'identity'): ((15, 1, 3, 12288, 0, 0, 0, 0, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 mask=6 fold_fwd_w=4 fold_fwd_h=4 fold_inv_w=5 fold_inv_h=5',
        'f64[1] f64[1] f64[1] f64[1,8] f64[64,64] f64[64,64] f64[1,3,64,64]'),
    ('fourier_sampling-noise_map', 'dct'): ((15, 1, 3, 12288, 0, 0, 0, 0, 0, 1, 1.0),
        'D=0 r=1 B=2 M=3 mask=6 fold_fwd_w=4 fold_fwd_h=4 fold_inv_w=5 fold_inv_h=5',
        'f64[1] f64[1] f64[1] f64[1,8] f64[64,64] f64[64,64] f64[1,3,64,64]'),
    ('fourier_sampling-noise_map', 'identity'): ((15, 1, 3, 12288, 0, 0, 0, 0, 0, 0, 1.0),
        'D=0 r=1 B=2 M=3 mask=6 fold_fwd_w=4 fold_fwd_h=4 fold_inv_w=5 fold_inv_h=5',
        'f64[1] f64[1] f64[1] f64[1,8] f64[64,64] f64[64,64] f64[1,3,64,64]'),
    ('gaussian_blur@128', 'dct'): ((1, 1, 3, 49152, 25, -13, 25, -113, 1, 1, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=col.dy tap_dx=col.dx tap_w=col.w tap2_dy=row.dy tap2_dx=row.dx tap2_w=row.w fold_fwd_w=4 fold_fwd_h=5 fold_inv_w=6 fold_inv_h=7',
        'f64[1] f64[1] f64[1] f64[1,8] f64[2,64,64] f64[2,64,64] f64[2,64,64] f64[2,64,64]'),
    ('gaussian_blur@128', 'identity'): ((1, 1, 3, 49152, 25, -13, 25, -113, 0, 0, 0.002500000176951289),
        'D=0 r=1 B=2 M=3 tap_dy=col.dy tap_dx=col.dx tap_w=col.w tap2_dy=row.dy tap2_dx=row.dx tap2_w=row.w',
        'f64[1] f64[1] f64[1] f64[1,8]'),
}

# config -> (op code of the name, stride, scale_factor or None, _sigma_y2 and _solver_sigma_y2 at sigma_s = 0.0001 and at 0.05,
# fh_problem.mask set)
FACTS = {
    'inpainting': (0, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, True),
    'noise': (0, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, True),
    'colorization': (3, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, False),
    'gaussian_blur': (1, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, False),
    'motion_blur': (1, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, False),
    'super_resolution': (2, 4, 4, 9.999999747378752e-05, 9.999999747378752e-05, 0.002500000176951289, 0.002500000176951289, False),
    'custom_blur-binomial': (1, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, False),
    'custom_blur-sparse': (1, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, False),
    'custom_blur-disk': (1, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, False),
    'masked_blur-sparse': (5, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, True),
    'masked_blur-disk': (5, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, True),
    'masked_blur-binomial-border': (5, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, True),
    'custom_sr-binomial': (2, 2, 2, 9.999999747378752e-05, 9.999999747378752e-05, 0.002500000176951289, 0.002500000176951289, False),
    'custom_sr-sparse': (2, 2, 2, 9.999999747378752e-05, 9.999999747378752e-05, 0.002500000176951289, 0.002500000176951289, False),
    'weighted_blur-sparse': (8, 1, None, 1.0000001111620804e-06, 1.0, 0.002500000176951289, 1.0, True),
    'weighted_blur-disk': (8, 1, None, 1.0000001111620804e-06, 1.0, 0.002500000176951289, 1.0, True),
    'weighted_sr-binomial': (10, 2, 2, 9.999999747378752e-05, 1.0, 0.002500000176951289, 1.0, True),
    'weighted_sr-sparse': (10, 2, 2, 9.999999747378752e-05, 1.0, 0.002500000176951289, 1.0, True),
    'burst_sr': (12, 2, 2, 9.999999747378752e-05, 9.999999747378752e-05, 0.002500000176951289, 0.002500000176951289, False),
    'weighted_burst_sr': (13, 2, 2, 9.999999747378752e-05, 1.0, 0.002500000176951289, 1.0, True),
    'varying_blur': (14, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, False),
    'fourier_sampling-pattern': (15, 1, None, 1.0000001111620804e-06, 1.0000001111620804e-06, 0.002500000176951289, 0.002500000176951289, True),
    'fourier_sampling-noise_map': (15, 1, None, 1.0000001111620804e-06, 1.0, 0.002500000176951289, 1.0, True),
}


def _facts(config):
    from free_hunch_amd import conditioning_mechanisms as cm
    sig = []
    for s in (0.0001, 0.05):
        op = make(config, sigma_s=s)
        sig += [cm._sigma_y2(op), cm._solver_sigma_y2(op)]
    p, _keep = cm._problem(op, stand_in_cov(64, True), cm._solver_sigma_y2(op))
    return (cm._op_code(op.name), p.stride, getattr(op, "scale_factor", None), *sig, bool(p.mask))


@pytest.mark.parametrize("basis", ["dct", "identity"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_problem_of_every_configuration(config, basis):
    got = snapshot(make(config), stand_in_cov(64, basis == "dct"))
    assert "?" not in got[1]
    assert got == EXPECTED[config, basis]


@pytest.mark.parametrize("basis", ["dct", "identity"])
def test_gaussian_blur_packs_symmetric_halves_from_128(basis):
    got = snapshot(make("gaussian_blur", S=128), stand_in_cov(128, basis == "dct"))
    assert got == EXPECTED["gaussian_blur@128", basis]
    assert got[0][SCALARS.index("fold_sym")] == (1 if basis == "dct" else 0)
    assert EXPECTED["gaussian_blur", "dct"][0][SCALARS.index("fold_sym")] == 0


def test_every_op_code_is_reached():
    assert {v[0][0] for v in EXPECTED.values()} == set(range(16))


def test_facts_of_every_name():
    assert {CONFIGS[c][0] for c in FACTS} == set(NAMES) and set(FACTS) == set(CONFIGS)
    assert {c: _facts(c) for c in CONFIGS} == FACTS


def test_unknown_name_is_refused_everywhere():
    from free_hunch_amd import conditioning_mechanisms as cm
    assert cm._op_code("bogus") is None
    op, cov, x = types.SimpleNamespace(name="bogus"), stand_in_cov(64, True), torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="Invalid operator name"):
        cm.solve_customcuda(op, x, x, cov, 1.0, 1.0)
    with pytest.raises(ValueError, match="Invalid operator name"):
        cm.solve_customcuda_batched([op, op], [x, x], [x, x], [cov, cov], 1.0, 1.0)
    with pytest.raises(ValueError, match="Invalid operator name"):
        cm.choose_solver("bogus", op, x, x, covariance_model=cov)
