"""numpy restatement of `fourier_sampling` (fh_problem.op = 15): the orthonormal 2-D discrete Hartley transform as
Re - Im of numpy.fft.fft2(norm="ortho"), the butterfly R in the order the kernel evaluates it, and the whitened system
    A_mm(u) = sigma_y2 u + W H C H W u
on the oracle's covariance classes, for the oracle's cg.  Written from the definitions (Bracewell's cas transform), float64 on
the CPU.  Not a test module: shared by tests/test_fourier_sampling_host.py and tests/test_fourier_sampling_gpu.py."""
import numpy as np
import torch


def reflect(a):
    """a[..., (-u) % S, (-v) % S]"""
    return np.roll(np.flip(a, axis=(-2, -1)), 1, axis=(-2, -1))


def hartley2(x):
    """H x = Re F x - Im F x over the last two axes (numpy array or CPU tensor in, the same kind out)"""
    if torch.is_tensor(x):
        return torch.from_numpy(hartley2(x.detach().cpu().numpy()))
    F = np.fft.fft2(np.asarray(x, dtype=np.float64), norm="ortho")
    return F.real - F.imag


def butterfly(T):
    """R(T)[u][v] = 1/2 ((T[u][v] + T[-u][v]) + (T[u][-v] - T[-u][-v])) with the sums in exactly that order: the bits of
    fh_hartley_fix without weights and add"""
    T = np.asarray(T, dtype=np.float64)
    Tu = np.roll(np.flip(T, axis=-2), 1, axis=-2)  # T[-u][v]
    Tv = np.roll(np.flip(T, axis=-1), 1, axis=-1)  # T[u][-v]
    return 0.5 * ((T + Tu) + (Tv - reflect(T)))


def _split(a):
    c = 134217729.0 * a  # Veltkamp: 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def butterfly_weighted(T, w, add, add_scale):
    """fma(add_scale, add, w * R(T)) with w * R(T) rounded.  The fma is restated with error-free transformations - the product's
    rounding error (Dekker) and the sum's (Knuth) are added back - so the result is within one ulp of the exact value also where
    the two terms cancel, which an 80-bit product is not."""
    r = np.asarray(w, dtype=np.float64) * butterfly(T)
    a, b = np.full_like(r, float(add_scale)), np.broadcast_to(np.asarray(add, dtype=np.float64), r.shape)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    ep = ((ah * bh - p) + ah * bl + al * bh) + al * bl  # a * b = p + ep exactly
    s = p + r
    bb = s - p
    es = (p - (s - bb)) + (r - bb)  # p + r = s + es exactly
    return s + (es + ep)


def cas_basis(S):
    """Hc[u][n] = (cos + sin)(2 pi u n / S) / sqrt(S) straight from the formula in float64"""
    k = np.arange(S)
    a = 2.0 * np.pi * ((k[:, None] * k[None, :]) % S) / S
    return (np.cos(a) + np.sin(a)) / np.sqrt(S)


class System:
    """the whitened system of one image: w the weights [1,3,S,S] (CPU tensor), orc the oracle covariance, s2 = sigma_y2"""

    def __init__(self, w, orc, s2):
        self.w, self.orc, self.s2 = w.detach().cpu().to(torch.float64), orc, float(s2)

    def A_mm(self, u):
        shape = self.w.shape
        u = u.reshape(shape)
        t = self.orc.denoiser_cov_vector_dot(hartley2(self.w * u))
        return (self.s2 * u + self.w * hartley2(t)).flatten()

    def rhs(self, y, x0_mean):
        """W (y - H x0)"""
        return (self.w * (y.cpu().to(torch.float64) - hartley2(x0_mean.cpu().to(torch.float64)))).flatten()

    def mat(self, sol):
        """A0^T W u"""
        return hartley2(self.w * sol.reshape(self.w.shape))
