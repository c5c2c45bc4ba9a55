"""The denoiser-error table of free-hunch_amd/recon_mse.py restated in numpy (helper of tests/test_recon_mse_host.py and
tests/test_recon_mse_gpu.py; not a test): Philox4x32-10 in uint64 arithmetic, the Box-Muller mapping and the noisy image in
float64, and the whole `errors` computation for a denoiser given as a callable.  Written from include/fh_hip.h's description of
fh_noisy_u8 / fh_sqerr_u8, not from the kernels."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two; returns the four output words as uint64 arrays < 2^32."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def box_muller(ra, rb):
    ua, ub = (ra.astype(np.float64) + 0.5) * 2.0 ** -32, (rb.astype(np.float64) + 0.5) * 2.0 ** -32
    rad = np.sqrt(-2.0 * np.log(ua))
    ang = 2 * np.pi * ub
    return rad * np.cos(ang), rad * np.sin(ang)


def normals(seed, image, level, count):
    """float64 [count] (count % 4 == 0): eps of elements 0 .. count - 1 of image `image` at level `level`."""
    assert count % 4 == 0
    q = np.arange(count // 4, dtype=np.uint64)
    r = philox4x32_10((q, image, level, 0), (seed & MASK, (seed >> 32) & MASK))
    z0, z1 = box_muller(r[0], r[1])
    z2, z3 = box_muller(r[2], r[3])
    return np.stack([z0, z1, z2, z3], axis=1).reshape(-1)


def x32(u8):
    """the sampler's StandardRGBEncoder in float32: u8 / 127.5 - 1, both operations rounded to float32"""
    return np.asarray(u8).astype(np.float32) / np.float32(127.5) - np.float32(1.0)


def noisy64(u8, image, level, sigma, seed):
    """float64 [3,S,S]: (double) x32 + sigma eps, before its single rounding to float32"""
    u8 = np.asarray(u8)
    return x32(u8).astype(np.float64) + float(sigma) * normals(seed, image, level, u8.size).reshape(u8.shape)


def noisy(u8_batch, img_index, level, sigma, seed):
    """float32 [n,3,S,S]: fh_noisy_u8"""
    return np.stack([noisy64(u, i, level, sigma, seed).astype(np.float32) for u, i in zip(np.asarray(u8_batch), img_index)])


def sqerr(D, u8_batch):
    """float64 [n]: fh_sqerr_u8 (the float32 D against x32, differences and sum in float64)"""
    d = np.asarray(D).astype(np.float32).astype(np.float64) - x32(u8_batch).astype(np.float64)
    return (d ** 2).reshape(len(d), -1).sum(1)


def errors(denoise, u8_batch, img_index, sigmas, level_ids, seed):
    """float64 [L, n]: level_errors.  denoise(x_t float32 [n,3,S,S], sigma) -> D [n,3,S,S] (stored as float32)."""
    u8_batch = np.asarray(u8_batch)
    per_image = u8_batch[0].size
    return np.stack([sqerr(denoise(noisy(u8_batch, img_index, lv, s, seed), float(s)), u8_batch) / per_image
                     for s, lv in zip([float(v) for v in sigmas], level_ids)])


def gauss_denoise(var=0.25):
    """inputs.gauss_prior_denoise in float64 on the float32 x_t"""
    return lambda x_t, sigma: x_t.astype(np.float64) * (var / (var + sigma ** 2))
