"""Measurement operators of the Free Hunch path on the device (reference:
measurement_utils/measurements.py:25-246, utils_sisr.py:9-96, resizer.py:8-160).

Same registry (`get_operator(name, **kwargs)`), same constructor keywords, same attributes the solvers read
(`name`, `sigma_s`, `in_shape`, `mask`, `scale_factor`).  The reference applies the blur through FFTs of a
zero-padded, rolled PSF (`p2o`); a circular convolution with the PSF's non-zero taps is the same linear map,
so the operators carry a sparse tap list (`taps`) that libfh_hip.so consumes.  `pre_calculated`
(FB, FBC, F2B, FBFy) is still offered for code that wants the transfer functions, computed lazily.
"""
from __future__ import annotations

import ctypes
import hashlib
import os

import numpy as np
import scipy.io
import torch

from . import _lib

F64 = torch.float64
_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
KERNEL_DIR = os.path.join(_DATA, "kernels")

__OPERATOR__ = {}


def register_operator(name):
    def wrapper(cls):
        if __OPERATOR__.get(name, None):
            raise NameError(f"Name {name} is already registered!")
        cls.name = name
        __OPERATOR__[name] = cls
        return cls
    return wrapper


def get_operator(name, **kwargs):
    if __OPERATOR__.get(name, None) is None:
        raise NameError(f"Name {name} is not defined.")
    return __OPERATOR__[name](**kwargs)


# ---------------------------------------------------------------------------------------------- argument checks
# Written once for the operators below; each takes the operator's name (`who`) for its messages.
def _checked_psf(k, who, what="the PSF", shifted=False, max_taps=None):
    """`k` rounded to float32 like the shipped PSFs, after the checks every caller's PSF passes: finite (also once rounded), not all
    zero, at most 32 from its centre at index size // 2 and, for a tap-list-only operator, at most `max_taps` non-zeros"""
    with np.errstate(over="ignore"):
        k = np.asarray(k, dtype=np.float32)
    if not np.isfinite(k).all():
        raise ValueError(f"{who}: {what} has a non-finite entry (also after rounding to float32)")
    if not k.any():
        raise ValueError(f"{who}: {what} is all zero")
    ys, xs = np.nonzero(k)
    hy, hx = int(np.abs(ys - k.shape[0] // 2).max()), int(np.abs(xs - k.shape[1] // 2).max())
    if max(hy, hx) > 32:
        raise ValueError(f"{who}: {what} reaches ({hy}, {hx}) samples from its centre at index size // 2" +
                         (" (its shift included); the kernels stage at most 32" if shifted else
                          "; the kernels stage at most 32 (PSFs up to 65 x 65)"))
    if max_taps is not None and ys.size > max_taps:
        raise ValueError(f"{who}: {what} has {ys.size} non-zeros, a tap list holds {max_taps}")
    return k


def _load_psfs(who, kernels, kernel_path, each):
    """K PSFs as float64 arrays from `kernels` (K 2-D arrays, a [K, kh, kw] array or one 2-D array) or from a .npy of the same;
    the caller has checked that exactly one of the two is given"""
    if kernels is None:
        arr = np.load(kernel_path)
        if arr.ndim not in (2, 3):
            raise ValueError(f"{who}: {kernel_path} must hold a [K, kh, kw] array or one 2-D PSF, got shape {tuple(arr.shape)}")
        psfs = [arr] if arr.ndim == 2 else list(arr)
    else:
        psfs = [kernels] if (isinstance(kernels, np.ndarray) and kernels.ndim == 2) else list(kernels)
    psfs = [np.asarray(k, dtype=np.float64) for k in psfs]
    if not psfs or any(k.ndim != 2 or k.size == 0 for k in psfs):
        raise ValueError(f"{who}: every {each} must be a non-empty 2-D array")
    return psfs


def _integer(s):
    """int(s) of an integral number that is no bool, else None"""
    ok = isinstance(s, (int, float, np.integer, np.floating)) and not isinstance(s, bool) and float(s) == int(s)
    return int(s) if ok else None


def _check_factor(who, S, s):
    """the scale factor s divides the image side S and leaves at least 8 x 8 measurements"""
    if S % s != 0:
        raise ValueError(f"{who}: scale_factor {s} does not divide the image side {S}")
    if S // s < 8:
        raise ValueError(f"{who}: scale_factor {s} leaves a {S // s} x {S // s} measurement of a {S} x {S} image; at "
                         "least 8 x 8 is required")


def _plan_refusal(plan, *args):
    """(adjoint, code) of the first direction for which the library's launch plan `plan(*args, adjoint, out)` finds no kernel,
    None when both run; asked of the library itself, which needs no device"""
    fn, out = getattr(_lib.load(), plan), (ctypes.c_int32 * 6)()
    for adjoint in (0, 1):
        rc = fn(*args, adjoint, out)
        if rc != 0:
            return adjoint, rc
    return None


def _load_array(who, what, value, path, shapes=None):
    """an array, a tensor or the .npy at `path` (when `value` is None), with one of `shapes` if given; float64"""
    a = np.load(path) if value is None else (value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value))
    if shapes is not None and tuple(a.shape) not in shapes:
        raise ValueError(f"{who}: {what} must have shape " + ", ".join(str(s) for s in shapes[:-1]) +
                         f" or {shapes[-1]}, got {tuple(a.shape)}")
    return np.asarray(a, dtype=np.float64)


def _image_shapes(n):
    return (n, n), (3, n, n), (1, 3, n, n)


class _TapList:
    def __init__(self, k, device):
        ys, xs = np.nonzero(k)
        cy, cx = k.shape[0] // 2, k.shape[1] // 2
        dy, dx, w = (ys - cy).astype(np.int32), (xs - cx).astype(np.int32), np.ascontiguousarray(k[ys, xs], dtype=np.float64)
        # what the fold cache knows the list by: equal lists share their folded bases without reading the device copies back
        self.digest = hashlib.sha1(dy.tobytes() + dx.tobytes() + w.tobytes()).hexdigest()
        self.n = int(ys.size)
        hy, hx = int(np.abs(ys - cy).max()), int(np.abs(xs - cx).max())
        self.hy, self.hx = hy, hx
        # fh_conv_circ halo code: for 1-D lists -(h+1) (column kernel, dx = 0) / -(h+101) (row kernel), else both extents
        # (1000 + 64 hy + hx), so that the kernel stages only the halo the taps reach
        self.halo = -(hy + 1) if (hx == 0 and hy > 0) else (-(hx + 101) if (hy == 0 and hx > 0) else 1000 + 64 * hy + hx)
        self.dy, self.dx, self.w = (torch.from_numpy(a).to(device) for a in (dy, dx, w))


class Taps(_TapList):
    """Non-zero PSF entries as (dy, dx, w) with the PSF centre at index size//2 (p2o's roll, utils_sisr.py:37-38).
    A numerically rank-1 PSF (the shipped Gaussian: second singular value 1e-8 of the first once rounded to float32,
    1e-16 before) is additionally split into a column and a row tap list (`sep`), so that the blur runs as two 1-D
    passes: 2 x 25 instead of 625 taps per pixel.  The rank-1 factor differs from the float32 taps by < 1e-7
    relative, the same size as the float32 rounding of the PSF / the complex64 OTF the reference blurs with.
    A PSF that is not rank-1 and has more non-zeros than a tap list may hold (MAX_TAPS; a measured PSF, a defocus disk)
    additionally gets `window` = (device tensor [2hy+1][2hx+1], hy, hx): the PSF about its centre, zero padded to odd sides
    (fh_conv_window).  So does a PSF that fills at least half of its window: the window kernel's time goes with the window's
    area, rows padded to whole blocks of 16 taps, the tap-list kernel's with the number of taps, and per multiply-add the
    window kernel measured 2.25x faster (a full 31 x 31 window at 256 x 256: 91.5 us against 205.8 us,
    profiles/custom_psf.md) - half is that ratio with a margin.  The shipped motion PSF fills 11 % of its window."""
    MAX_TAPS = 1024  # kMaxTaps of csrc/fh_kernels.hip

    def __init__(self, kernel, device):
        k = np.asarray(kernel, dtype=np.float32).astype(np.float64)  # the reference holds the PSF in float32
        super().__init__(k, device)
        self.kernel = torch.from_numpy(k.astype(np.float32))
        self.sep = None
        if min(k.shape) > 1:
            u, sv, vt = np.linalg.svd(k)
            if sv[1] <= 1e-6 * sv[0]:
                col, row = u[:, 0] * np.sqrt(sv[0]), vt[0] * np.sqrt(sv[0])
                if col.sum() < 0:
                    col, row = -col, -row
                col[np.abs(col) < 1e-12 * np.abs(col).max()] = 0.0
                row[np.abs(row) < 1e-12 * np.abs(row).max()] = 0.0
                self.sep = (_TapList(col[:, None], device), _TapList(row[None, :], device))
        self.window = None
        area = (2 * self.hy + 1) * (-(-(2 * self.hx + 1) // 16) * 16)  # what k_conv_window multiplies per output
        if self.sep is None and min(k.shape) > 1 and (self.n > self.MAX_TAPS or 2 * self.n >= area or not self._tap_list_fits()):
            ys, xs = np.nonzero(k)
            win = np.zeros((2 * self.hy + 1, 2 * self.hx + 1))
            win[ys - k.shape[0] // 2 + self.hy, xs - k.shape[1] // 2 + self.hx] = k[ys, xs]
            self.window = (torch.from_numpy(win).to(device), self.hy, self.hx)

    def _tap_list_fits(self):
        """False where fh_conv_circ has no stride-1 launch for this list (wide extents with several hundred taps overflow the
        tile kernels' LDS: FH_ESIZE); asked of the library's own plan, which needs no device."""
        return _plan_refusal("fh_conv_circ_plan", 256, self.n, self.halo, 3, 1) is None


def dct_basis_longdouble(S):
    """Orthonormal DCT-II matrix C[k][n] = s_k cos(pi (2n + 1) k / 2S) in extended precision (the same formula the
    context's device basis is built from, csrc/fh_kernels.hip: fh_context_create)."""
    ld = np.longdouble
    k = np.arange(S, dtype=ld)[:, None]
    n = np.arange(S, dtype=ld)[None, :]
    C = np.cos(np.arccos(ld(-1)) * (2 * n + 1) * k / (2 * ld(S)))  # arccos(-1) = pi in extended precision
    C *= np.sqrt(ld(2) / ld(S))
    C[0] *= np.sqrt(ld(0.5))
    return C


def folded_dct_blur_bases(col_dy, col_w, row_dx, row_w, S):
    """The two 1-D passes of a separable circular blur folded into the 2-D DCT that follows / precedes them inside the CG
    operator A C A^T (C lives in the DCT basis):  with the blur A(X) = F_col X F_row^T,
        dct2(A^T u)  = P_col u P_row^T,        A(idct2(v)) = P_col^T v P_row,        P = C_dct F^T,
    so the four image passes of the two blurs disappear into the (dense) DCT passes.  F is circulant,
    F[i][i'] = sum_t w_t [i' = (i - d_t) mod S], hence P[k][n] = sum_t w_t C[k][(n - d_t) mod S] - formed in extended
    precision and rounded once.  Returns float64 (P_row, P_col, P_row^T, P_col^T), C-contiguous [S][S]."""
    P_row, P_col = _fold_longdouble(row_dx, row_w, S), _fold_longdouble(col_dy, col_w, S)
    f = lambda M: np.ascontiguousarray(M.astype(np.float64))
    return f(P_row), f(P_col), f(P_row.T), f(P_col.T)


def _fold_longdouble(offsets, weights, S):
    """P[k][n] = sum_t w_t C[k][(n - d_t) mod S] in extended precision (folded_dct_blur_bases)"""
    C = dct_basis_longdouble(S)
    P = np.zeros((S, S), dtype=np.longdouble)
    for d, w in zip(offsets, weights):
        P += np.longdouble(w) * np.roll(C, int(d), axis=1)
    return P


def folded_dct_sr_bases(col_dy, col_w, row_dx, row_w, S, s):
    """`folded_dct_blur_bases` for blur + decimation by s (s divides S, So = S / s):  A(X) = Dec_s F_col X F_row^T Dec_s^T, and
    with G[k][j] = P[k][j s] - P with every s-th column kept, [S][So] -
        dct2(A^T u)  = G_col u G_row^T,        A(idct2(v)) = G_col^T v G_row
    (A^T zero-inserts u, which selects those columns of P).  The extended-precision P is subsampled before the single
    rounding.  Returns float64 (G_row, G_col, G_row^T, G_col^T), C-contiguous, [S][So] and [So][S]."""
    if s < 1 or S % s != 0:
        raise ValueError(f"folded_dct_sr_bases: the factor {s} does not divide the image side {S}")
    G_row, G_col = _fold_longdouble(row_dx, row_w, S)[:, ::s], _fold_longdouble(col_dy, col_w, S)[:, ::s]
    f = lambda M: np.ascontiguousarray(M.astype(np.float64))
    return f(G_row), f(G_col), f(G_row.T), f(G_col.T)


def pack_symmetric_halves(P):
    """If the S x S basis P has the DCT's mirror symmetry P[k][S-1-n] = (-1)^k P[k][n] (the DCT itself; a SYMMETRIC blur
    folded into it), return the packed half bases of fh_problem.fold_sym = 1 (include/fh_hip.h): forward [Pe; Po] with
    Pe[j][n] = P[2j][n], Po[j][n] = P[2j+1][n], and inverse [Qe; Qo] = [Pe^T; Po^T], each float64 [2][S/2][S/2]; else None."""
    S = P.shape[0]
    if S % 128 != 0:  # k_dct_sym works on K chunks of 64 of the half range
        return None
    H = S // 2
    sign = np.where(np.arange(S) % 2 == 0, 1.0, -1.0)[:, None]
    if np.abs(P[:, ::-1] * sign - P).max() > 1e-13 * np.abs(P).max():
        return None
    Pe, Po = P[0::2, :H], P[1::2, :H]
    fwd = np.ascontiguousarray(np.stack([Pe, Po]))
    inv = np.ascontiguousarray(np.stack([Pe.T, Po.T]))
    return fwd, inv


_FOLD_CACHE = {}  # (kind, S, factor, device, digests of the column and row tap lists) -> folded bases on the device


class LinearOperator:
    """What the operators share.  A subclass supplies `apply`; `forward`, `transpose` and `forward_adjoint` follow from it,
    from `_noise`, from `mask` (where the operator has one it multiplies the adjoint's argument) and from `out_shape` (the
    measurement's shape, the image's where absent)."""
    device = None

    ctx_slot = 0  # scratch-context slot; the batched sampler gives every concurrent image its own
    decimates = False  # A ends with [..., ::scale_factor, ::scale_factor]
    keeps_last_y = True  # `forward` remembers its result for `pre_calculated`

    def _ctx(self):
        S = self.in_shape[-1]
        return _lib.Context.get(S, 3, 128, self.ctx_slot)

    def apply(self, x, adjoint=False, ctx=None):
        """A x, or A^T x, of an NCHW tensor with any N, in float64: the noiseless measurement the solver's system is built on.
        `ctx`: the scratch context to run on, None = the operator's own choice (the batched solve passes its batch's)."""
        return self._conv(x, self.scale_factor if self.decimates else 1, adjoint, ctx)

    def _conv(self, x, stride=1, adjoint=False, ctx=None):
        """float64 circular convolution of an NCHW tensor with self.taps; returns float64."""
        S = self.in_shape[-1]
        x64 = x.detach().to(device=self.device, dtype=F64).contiguous()
        so = S if (adjoint or stride == 1) else S // stride
        out = torch.empty(x64.shape[0], x64.shape[1], so, so, dtype=F64, device=self.device)
        planes = x64.shape[0] * x64.shape[1]
        return (self._ctx() if ctx is None else ctx).blur(x64, out, self.taps, planes, stride, adjoint)

    def forward(self, data, flatten=False, noiseless=False):
        # the noise is drawn once, at the measurement's shape (an operator's mask or noise map comes in through `_noise`)
        y = self._noise(self.apply(data).to(data.dtype), noiseless)
        if self.keeps_last_y:
            self._last_y = y
        if flatten:
            return y, y.reshape(y.shape[0], -1)
        return y

    def _apply_adjoint(self, v):
        mask = getattr(self, "mask", None)
        return self.apply(v if mask is None else v * mask.to(v.dtype), adjoint=True).to(v.dtype)

    def transpose(self, y, flatten=False):
        if flatten:
            y = y.reshape(y.shape[0], *getattr(self, "out_shape", self.in_shape)[-3:])
        return self._apply_adjoint(y)

    def forward_adjoint(self, v):
        """exact adjoint of the noiseless `forward` (A^T (mask * v) with a mask), for DPS"""
        return self._apply_adjoint(v)

    def _folded(self, kind, factor, build):
        """`build(col_dy, col_w, row_dx, row_w)` of the separable PSF's two tap lists, once per (kind, size, factor, device,
        PSF) and shared by all instances - None when the PSF is not rank-1 or FH_NO_FOLD=1"""
        sep = getattr(getattr(self, "taps", None), "sep", None)
        if sep is None or os.environ.get("FH_NO_FOLD") == "1":
            return None
        col, row = sep
        key = (kind, self.in_shape[-1], factor, str(self.device), col.digest, row.digest)
        if key not in _FOLD_CACHE:
            _FOLD_CACHE[key] = build(col.dy.cpu().numpy(), col.w.cpu().numpy(), row.dx.cpu().numpy(), row.w.cpu().numpy())
        return _FOLD_CACHE[key]

    def folded_bases(self):
        """(device copies of `folded_dct_blur_bases` for this operator's separable PSF, packed-symmetric flag) - None when
        the PSF is not rank-1 or the operator decimates; built once per (PSF, size, device), shared by all instances."""
        def build(*lists):
            mats = folded_dct_blur_bases(*lists, self.in_shape[-1])
            hw, hh = pack_symmetric_halves(mats[0]), pack_symmetric_halves(mats[1])
            sym = hw is not None and hh is not None and os.environ.get("FH_DCT_NOSYM") is None
            if sym:  # (fold_fwd_w, fold_fwd_h, fold_inv_w, fold_inv_h) as packed halves
                mats = (hw[0], hh[0], hw[1], hh[1])
            return tuple(torch.from_numpy(m).to(self.device) for m in mats), sym
        return None if self.decimates else self._folded("blur", 1, build)

    def folded_sr_bases(self):
        return None  # (only a single rank-1 PSF with a decimation folds into rectangular bases: CustomSROperator)

    def _noise(self, y, noiseless):
        if not noiseless:
            y = y + self.sigma_s.to(y.dtype) * torch.randn_like(y)
        return y

    @property
    def pre_calculated(self):
        """(FB, FBC, F2B, FBFy) as utils_sisr.pre_calculate would return them for the last measurement."""
        k = self.taps.kernel.to(self.device)
        S = self.in_shape[-1]
        otf = torch.zeros(1, 1, S, S, device=self.device)
        otf[..., : k.shape[0], : k.shape[1]] = k
        otf = torch.roll(otf, (-(k.shape[0] // 2), -(k.shape[1] // 2)), dims=(-2, -1))
        FB = torch.fft.fftn(otf, dim=(-2, -1))
        FBC = torch.conj(FB)
        y = getattr(self, "_last_y", None)
        FBFy = None
        if y is not None:
            sf = self.scale_factor if self.decimates else 1
            up = torch.zeros(y.shape[0], y.shape[1], S, S, device=self.device, dtype=y.dtype)
            up[..., ::sf, ::sf] = y
            FBFy = FBC * torch.fft.fftn(up, dim=(-2, -1))
        return FB, FBC, torch.abs(FB) ** 2, FBFy


class _BlurOperator(LinearOperator):
    kernel_file = None

    def __init__(self, in_shape, kernel_size, intensity, sigma_s, device, **kwargs):
        self.device = torch.device(device)
        self.kernel_size = kernel_size
        self.kernel = np.load(os.path.join(KERNEL_DIR, self.kernel_file))
        self.taps = Taps(self.kernel, self.device)
        self.sigma_s = torch.Tensor([sigma_s]).to(self.device)
        self.in_shape = in_shape

    def get_kernel(self):
        return self.taps.kernel.view(1, 1, *self.taps.kernel.shape).to(self.device)


@register_operator(name="gaussian_blur")
class GaussialBlurOperator(_BlurOperator):  # (sic) the reference's class name, measurements.py:164
    kernel_file = "gaussian_ks61_std3.0.npy"


@register_operator(name="motion_blur")
class MotionBlurOperator(_BlurOperator):  # measurements.py:126 (weights come from the shipped .npy, :135-136)
    kernel_file = "motion_ks61_std0.5.npy"


@register_operator(name="custom_blur")
class CustomBlurOperator(_BlurOperator):
    """Circular blur with the caller's own PSF: `kernel_path` (a 2-D .npy) or `kernel` (a 2-D array), rounded to float32 like
    the shipped PSFs and used AS GIVEN - not normalised, centre at index size // 2 in both axes.  A rank-1 PSF runs as two
    1-D passes (and folds into the DCT passes), a sparse one on the tap-list kernels, a dense one on fh_conv_window
    (`Taps`).  The extent about the centre is at most 32 in either axis (PSFs up to 65 x 65)."""

    def __init__(self, in_shape, sigma_s, device, kernel_path=None, kernel=None, **kwargs):
        if (kernel_path is None or kernel_path == "") == (kernel is None):
            raise ValueError("custom_blur needs exactly one of kernel_path (a 2-D .npy file) and kernel (a 2-D array)")
        k = np.load(kernel_path) if kernel is None else np.asarray(kernel)
        if k.ndim != 2 or k.size == 0:
            raise ValueError(f"custom_blur: the PSF must be a 2-D array, got shape {tuple(k.shape)}")
        k = _checked_psf(k, "custom_blur")
        self.device = torch.device(device)
        self.kernel_size = tuple(k.shape)  # (rows, columns)
        self.kernel = k
        self.taps = Taps(k, self.device)
        self.sigma_s = torch.Tensor([sigma_s]).to(self.device)
        self.in_shape = in_shape


@register_operator(name="masked_blur")
class MaskedBlurOperator(CustomBlurOperator):
    """Blur with a validity mask, y = M (B x + n): B the circular blur of `custom_blur` (same PSF arguments, same checks,
    same kernels), M a 0/1 mask (1 = pixel measured) that drops what the circular model cannot explain - saturated, dead or
    occluded pixels, and the band along the edges that a real camera did not wrap around.
      mask        array / tensor [S,S], [3,S,S] or [1,3,S,S], entries exactly 0 or 1
      mask_path   a .npy of the same shapes (instead of `mask`)
      mask_border N >= 0: N pixels on every side are dropped; -1: the PSF's reach, hy rows top and bottom, hx columns left
                  and right (`taps.hy`, `taps.hx`)
    Border and array multiply.  `mask` is [1,3,S,S] on the device, like InpaintingOperator.mask."""

    def __init__(self, in_shape, sigma_s, device, kernel_path=None, kernel=None, mask=None, mask_path=None, mask_border=0,
                 **kwargs):
        super().__init__(in_shape, sigma_s, device, kernel_path=kernel_path, kernel=kernel)
        S = int(in_shape[-1])
        mask_path = mask_path or None
        mask_border = int(mask_border or 0)
        if mask is not None and mask_path is not None:
            raise ValueError("masked_blur takes mask (an array) or mask_path (a .npy file), not both")
        if mask is None and mask_path is None and mask_border == 0:
            raise ValueError("masked_blur needs a mask: mask, mask_path or a non-zero mask_border (for a blur without a mask "
                             "use custom_blur)")
        if mask_border < -1:
            raise ValueError(f"masked_blur: mask_border is a pixel count >= 0, or -1 for the PSF's reach; got {mask_border}")
        m = np.ones((1, 3, S, S))
        if mask is not None or mask_path is not None:
            a = _load_array("masked_blur", "the mask", mask, mask_path, _image_shapes(S))
            if not np.isfinite(a).all():
                raise ValueError("masked_blur: the mask has a non-finite entry")
            if not np.isin(a, (0.0, 1.0)).all():
                raise ValueError("masked_blur: the mask has an entry other than 0 and 1 (per-pixel weights are not supported)")
            m = m * a.reshape((1, 1, S, S) if a.ndim == 2 else (1, 3, S, S))
        by, bx = (self.taps.hy, self.taps.hx) if mask_border == -1 else (mask_border, mask_border)
        if 2 * max(by, bx) >= S:
            raise ValueError(f"masked_blur: a border of ({by}, {bx}) pixels on every side leaves nothing of a {S} x {S} image")
        if by > 0:
            m[..., :by, :] = 0.0
            m[..., S - by:, :] = 0.0
        if bx > 0:
            m[..., :, :bx] = 0.0
            m[..., :, S - bx:] = 0.0
        if not m.any():
            raise ValueError("masked_blur: the mask (array times border) is all zero - no pixel is measured")
        self.mask_border = (by, bx)
        self.mask = torch.from_numpy(m).to(self.device)  # float64 [1,3,S,S]

    def _noise(self, y, noiseless):
        # the noise is drawn for the full image (custom_blur's RNG consumption), then masked
        return super()._noise(y, noiseless) * self.mask.to(y.dtype)


@register_operator(name="custom_sr")
class CustomSROperator(CustomBlurOperator):
    """Super-resolution with the caller's own PSF and factor: y = (B x)[..., ::s, ::s] + sigma_s n, B the circular blur of
    `custom_blur` (same PSF arguments and checks: `kernel_path` or `kernel`, used as given, centre at index size // 2),
    s = `scale_factor`, an integer 2 .. 16 that divides the image side and leaves at least 8 x 8 measurements.  Unlike
    `super_resolution` the measurement IS the solver's A: `forward` is blur + decimation, `transpose` its exact adjoint.
    Every route outside the folded solve runs the PSF's tap list (k_conv_dec / k_conv_up), so the PSF has at most
    `Taps.MAX_TAPS` non-zeros; a rank-1 PSF (box, Gaussian, binomial) additionally folds into rectangular DCT bases
    (`folded_sr_bases`, fh_problem.op = 7)."""
    decimates = True

    def __init__(self, in_shape, sigma_s, device, scale_factor=None, kernel_path=None, kernel=None, **kwargs):
        s = _integer(scale_factor)
        if s == 1:
            raise ValueError("custom_sr: scale_factor = 1 does not decimate - use custom_blur for a blur at full resolution")
        if s is None or not 2 <= s <= 16:
            raise ValueError(f"custom_sr: scale_factor must be an integer from 2 to 16, got {scale_factor!r}")
        super().__init__(in_shape, sigma_s, device, kernel_path=kernel_path, kernel=kernel)
        S = int(in_shape[-1])
        _check_factor("custom_sr", S, s)
        if self.taps.n > Taps.MAX_TAPS:
            raise ValueError(f"custom_sr: the PSF has {self.taps.n} non-zeros, a tap list holds {Taps.MAX_TAPS}; a decimating "
                             "dense-window kernel is out of scope")
        refused = _plan_refusal("fh_conv_circ_plan", S, self.taps.n, self.taps.halo, 3, s)
        if refused:
            raise ValueError(f"custom_sr: no kernel runs this PSF's tap list ({self.taps.n} taps reaching ({self.taps.hy}, "
                             f"{self.taps.hx})) at stride {s} on a {S} x {S} image (adjoint = {refused[0]}, code {refused[1]})")
        self.scale_factor = s
        self.out_shape = (1, 3, S // s, S // s)

    def folded_sr_bases(self):
        """device copies of `folded_dct_sr_bases` (G_row, G_col, G_row^T, G_col^T) for a rank-1 PSF - None when the PSF is not
        rank-1 or FH_NO_FOLD=1; built once per (PSF, size, factor, device), shared by all instances."""
        S, s = self.in_shape[-1], self.scale_factor
        return self._folded("sr", s, lambda *lists: tuple(torch.from_numpy(m).to(self.device)
                                                          for m in folded_dct_sr_bases(*lists, S, s)))


def shifted_psf(psf, dy, dx):
    """The PSF of a frame displaced by (dy, dx) high-resolution pixels: the frame samples the blurred scene at
    (s i + dy, s j + dx), and (B x)[i + dy] = sum_d k[d] x[i + dy - d] = sum_d' k[d' + dy] x[i - d'] - the PSF translated by
    (-dy, -dx): a POSITIVE dy moves the entries UP (towards smaller row indices), a positive dx to the LEFT.  The integer part
    moves entries exactly; the fractional part f in [0, 1) samples between two pixels, (1 - f) k[. + n] + f k[. + n + 1], the
    2 x 2 bilinear kernel in two dimensions.  float64; the result is zero padded to odd sides with the centre kept at
    size // 2, and the sum of the entries is preserved."""
    k = np.asarray(psf, dtype=np.float64)
    if k.ndim != 2 or k.size == 0:
        raise ValueError(f"shifted_psf: the PSF must be a 2-D array, got shape {tuple(k.shape)}")
    dy, dx = float(dy), float(dx)
    if not (np.isfinite(dy) and np.isfinite(dx)):
        raise ValueError(f"shifted_psf: the shift must be finite, got ({dy}, {dx})")

    def axis(a, shift, ax):
        """translate by -shift along `ax`; `a` has its centre at size // 2, so has the result"""
        n = int(np.floor(shift))
        f = shift - n
        size, c = a.shape[ax], a.shape[ax] // 2
        lo, hi = -c - n - (1 if f > 0 else 0), size - 1 - c - n  # offsets the entries land on
        H = max(abs(lo), abs(hi), 0)
        shape = list(a.shape)
        shape[ax] = 2 * H + 1
        out = np.zeros(shape)
        sl = [slice(None)] * a.ndim
        start = H - c - n  # index of the entry that had index 0
        sl[ax] = slice(start, start + size)
        if f > 0:
            out[tuple(sl)] = (1.0 - f) * a
            sl[ax] = slice(start - 1, start - 1 + size)
            out[tuple(sl)] += f * a
        else:
            out[tuple(sl)] = a
        return out

    return axis(axis(k, dy, 0), dx, 1)


class FrameTaps:
    """The tap lists of a burst's K frames (`Taps` each) concatenated in frame order for fh_conv_frames / fh_problem.op = 12:
    dy, dx, w [n], `off` int32 [K + 1] frame offsets (on the device), `max_taps` the longest frame, (hy, hx) the extents over
    all frames and `halo` their 2-D code."""

    def __init__(self, frames, device):
        self.nframes = len(frames)
        counts = [t.n for t in frames]
        self.n, self.max_taps = int(sum(counts)), int(max(counts))
        self.hy, self.hx = max(t.hy for t in frames), max(t.hx for t in frames)
        self.halo = 1000 + 64 * self.hy + self.hx
        self.dy = torch.cat([t.dy for t in frames]).contiguous()
        self.dx = torch.cat([t.dx for t in frames]).contiguous()
        self.w = torch.cat([t.w for t in frames]).contiguous()
        self.off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(device)


def parse_frame_shifts(shifts):
    """`frame_shifts` as a list of (dy, dx) floats: a sequence of pairs, or the command line's "dy,dx;dy,dx;..." string"""
    if isinstance(shifts, str):
        try:
            shifts = [tuple(float(v) for v in pair.split(",")) for pair in shifts.split(";") if pair.strip()]
        except ValueError:
            raise ValueError(f"burst_sr: frame_shifts is 'dy,dx;dy,dx;...' with numbers, got {shifts!r}") from None
    out = [tuple(float(v) for v in np.asarray(p, dtype=np.float64).ravel()) for p in shifts]
    if not out or any(len(p) != 2 or not np.isfinite(p).all() for p in out):
        raise ValueError(f"burst_sr: frame_shifts is a non-empty list of finite (dy, dx) pairs, got {shifts!r}")
    return out


class _ImageOperator(LinearOperator):
    """Operators whose kernels take whole images [N, 3, S, S] and check the planes their context holds (fh_conv_frames,
    fh_conv_blend, fh_hartley2d)."""

    def _conv(self, x, stride=None, adjoint=False, ctx=None):
        """`apply` under the name the tap-list operators use (`stride` is the operator's own whatever the caller passes)"""
        return self.apply(x, adjoint, ctx)

    def _images(self, x, shape, ctx):
        """(x in float64 on the device, N, the context for its 3 N planes) after the shape check [N, *shape]"""
        S = self.in_shape[-1]
        x64 = x.detach().to(device=self.device, dtype=F64).contiguous()
        N = x64.shape[0]
        assert tuple(x64.shape[1:]) == shape, f"{self.name}: expected [N,{','.join(str(n) for n in shape)}], got {tuple(x64.shape)}"
        if ctx is None:
            ctx = self._ctx() if N == 1 else _lib.Context.get(S, 3 * N, 0, self.ctx_slot)
        return x64, N, ctx

    def _set_frames(self, psfs, who, what, shifted=False):
        """`kernels`, `frames` (`Taps` each) and `frame_taps` of K PSFs, each through `_checked_psf` as `what.format(index)`"""
        self.kernels = [_checked_psf(k, who, what.format(i), shifted, Taps.MAX_TAPS) for i, k in enumerate(psfs)]
        self.frames = [Taps(k, self.device) for k in self.kernels]
        self.frame_taps = FrameTaps(self.frames, self.device)
        self.nframes = len(psfs)


@register_operator(name="burst_sr")
class BurstSROperator(_ImageOperator):
    """Multi-frame super-resolution: K low-resolution frames of one scene, each with its own PSF,
        y_k = (B_k x)[..., ::s, ::s] + sigma_s n_k,   k = 0 .. K - 1,
    B_k the circular blur of `custom_blur` (centre at index size // 2, rounded to float32, used as given), s = `scale_factor`
    in {2, 3, 4}, a divisor of the image side that leaves at least 8 x 8 measurements, and 1 <= K <= s^2.  A frame's displacement
    is part of its PSF: `frame_shifts` = K pairs (dy, dx) in high-resolution pixels translates the PSFs through `shifted_psf`
    (frame k samples the blurred scene at (s i + dy_k, s j + dx_k)).
      kernels       K 2-D arrays (or a [K, kh, kw] array)
      kernel_path   a .npy with a [K, kh, kw] array, or with one 2-D PSF (then every shift applies to it)
      frame_shifts  None, K pairs, or the string "dy,dx;dy,dx;..."; one PSF is repeated for every shift, K PSFs take one each
    One sigma_s covers all frames.  The measurement is frame-major: [1, 3 K, So, So] with channel 3 k + c.  `forward` and
    `transpose` are one A (fh_conv_frames); the solver's system is fh_problem.op = 12.  Every frame's PSF has at most
    `Taps.MAX_TAPS` non-zeros and reaches at most 32 from its centre."""
    decimates = True

    def __init__(self, in_shape, sigma_s, device, scale_factor=None, kernels=None, kernel_path=None, frame_shifts=None, **kwargs):
        s = _integer(scale_factor)
        if s not in (2, 3, 4):
            raise ValueError(f"burst_sr: scale_factor must be 2, 3 or 4, got {scale_factor!r}")
        S = int(in_shape[-1])
        _check_factor("burst_sr", S, s)
        if (kernel_path is None or kernel_path == "") == (kernels is None):
            raise ValueError("burst_sr needs exactly one of kernels (K 2-D arrays) and kernel_path (a .npy file with a "
                             "[K, kh, kw] array, or one 2-D PSF beside frame_shifts)")
        psfs = _load_psfs("burst_sr", kernels, kernel_path, "frame's PSF")
        if frame_shifts is not None and not (isinstance(frame_shifts, str) and frame_shifts == ""):
            shifts = parse_frame_shifts(frame_shifts)
            if len(psfs) == 1:
                psfs = psfs * len(shifts)
            if len(shifts) != len(psfs):
                raise ValueError(f"burst_sr: {len(shifts)} frame_shifts for {len(psfs)} PSFs; give one shift per frame (or one PSF "
                                 "for all shifts)")
            psfs = [shifted_psf(k, dy, dx) for k, (dy, dx) in zip(psfs, shifts)]
        K = len(psfs)
        if not 1 <= K <= s * s:
            raise ValueError(f"burst_sr: {K} frames at scale_factor {s}; the number of frames K is 1 .. s^2 = {s * s} (the "
                             "measurement is never longer than the image)")
        self.device = torch.device(device)
        self._set_frames(psfs, "burst_sr", "the PSF of frame {}", shifted=True)
        ft = self.frame_taps
        refused = _plan_refusal("fh_conv_frames_plan", S, K, ft.max_taps, ft.halo, 3, s)
        if refused:
            raise ValueError(f"burst_sr: no kernel runs these tap lists (at most {ft.max_taps} taps per frame reaching "
                             f"({ft.hy}, {ft.hx})) at stride {s} on a {S} x {S} image (adjoint = {refused[0]}, code {refused[1]})")
        self.scale_factor = s
        self.sigma_s = torch.Tensor([sigma_s]).to(self.device)
        self.in_shape = in_shape
        self.out_shape = (1, 3 * K, S // s, S // s)

    def apply(self, x, adjoint=False, ctx=None):
        """all frames' blur + decimation of an NCHW tensor [N,3,S,S] -> [N,3K,So,So] (frame-major), or the adjoint back;
        float64"""
        S, s = self.in_shape[-1], self.scale_factor
        y_shape = (3 * self.nframes, S // s, S // s)
        x64, N, ctx = self._images(x, y_shape if adjoint else (3, S, S), ctx)
        out = torch.empty(N, *((3, S, S) if adjoint else y_shape), dtype=F64, device=self.device)
        return ctx.blur_frames(x64, out, self.frame_taps, 3 * N, s, adjoint)


def grid_blend_weights(S, rows, cols):
    """Blend maps of a rows x cols grid of PSFs over an S x S image, float64 [rows * cols, S, S], row-major over the grid:
    the tensor product of 1-D hat functions whose nodes sit at the cell centres (i + 0.5) S / n (pixel j at coordinate
    j + 0.5).  Beyond the outermost nodes a map stays constant - no wrap-around - and a grid of one node along an axis is all
    ones along it.  Every pixel's weights sum to 1 (a partition of unity; within 1e-15)."""
    S, rows, cols = int(S), int(rows), int(cols)
    if S < 1 or rows < 1 or cols < 1:
        raise ValueError(f"grid_blend_weights: S, rows and cols must be positive, got {S}, {rows}, {cols}")

    def hats(n):
        """[n, S]: hat i is 1 at node i and falls to 0 at its neighbours; clamped outside the first / last node"""
        if n == 1:
            return np.ones((1, S))
        nodes = (np.arange(n) + 0.5) * S / n
        t = np.clip((np.arange(S) + 0.5 - nodes[0]) / (nodes[1] - nodes[0]), 0.0, n - 1.0)  # position in node units
        lo = np.minimum(np.floor(t).astype(np.int64), n - 2)  # the pixel's cell: at most two hats are non-zero, 1 - f and f
        f = t - lo
        h = np.zeros((n, S))
        h[lo, np.arange(S)] = 1.0 - f
        h[lo + 1, np.arange(S)] += f
        return h

    hy, hx = hats(rows), hats(cols)
    return np.ascontiguousarray((hy[:, None, :, None] * hx[None, :, None, :]).reshape(rows * cols, S, S))


def parse_psf_grid(grid):
    """`psf_grid` as (rows, cols): a pair of positive integers, or the command line's "RxC" string"""
    try:
        if isinstance(grid, str):
            r, c = grid.lower().split("x")
            rows, cols = int(r), int(c)
        else:
            rows, cols = (int(v) for v in grid)
            if tuple(float(v) for v in grid) != (rows, cols):
                raise ValueError
    except (ValueError, TypeError):
        raise ValueError(f"varying_blur: psf_grid is (rows, cols) or the string 'RxC' with positive integers, got {grid!r}") from None
    if rows < 1 or cols < 1:
        raise ValueError(f"varying_blur: psf_grid is (rows, cols) or the string 'RxC' with positive integers, got {grid!r}")
    return rows, cols


@register_operator(name="varying_blur")
class VaryingBlurOperator(_ImageOperator):
    """Blur with a PSF that changes across the field, as the Nagy-O'Leary interpolation of K shift-invariant blurs:
        y = sum_k U_k .* (B_k x) + sigma_s n,   A = sum_k diag(U_k) B_k,   A^T = sum_k B_k^T diag(U_k),
    B_k the circular blur of `custom_blur` with PSF k (centre at index size // 2, rounded to float32, used as given) and U_k a
    per-pixel blend map.  1 <= K <= 16; the measurement keeps the image's size.
      kernels       K 2-D arrays (or a [K, kh, kw] array)
      kernel_path   a .npy with a [K, kh, kw] array (or one 2-D PSF: K = 1)
      blend         an array or tensor [K, S, S] (broadcast over the channels), [K, 3, S, S] or [3 K, S, S] (channel 3 k + c)
      blend_path    a .npy of the same
      psf_grid      (rows, cols) or "RxC" with rows * cols = K: the maps of `grid_blend_weights`, the PSFs row-major on the grid
    Exactly one of kernels / kernel_path and exactly one of blend / blend_path / psf_grid.  The maps must be finite and none may
    be all zero; a partition of unity is NOT enforced: any finite maps are a valid linear A (maps that do not sum to one change
    the local gain, negative entries are allowed).  `forward` and `transpose` are one A (fh_conv_blend); the solver's system is
    fh_problem.op = 14.  Every PSF has at most `Taps.MAX_TAPS` non-zeros and reaches at most 32 from its centre."""

    MAX_PSFS = 16

    def __init__(self, in_shape, sigma_s, device, kernels=None, kernel_path=None, blend=None, blend_path=None, psf_grid=None,
                 **kwargs):
        S = int(in_shape[-1])
        if (kernel_path is None or kernel_path == "") == (kernels is None):
            raise ValueError("varying_blur needs exactly one of kernels (K 2-D arrays) and kernel_path (a .npy file with a "
                             "[K, kh, kw] array)")
        psfs = _load_psfs("varying_blur", kernels, kernel_path, "PSF")
        K = len(psfs)
        if not 1 <= K <= self.MAX_PSFS:
            raise ValueError(f"varying_blur: {K} PSFs; the number of PSFs K is 1 .. {self.MAX_PSFS}")
        given = [blend is not None, not (blend_path is None or blend_path == ""), not (psf_grid is None or psf_grid == "")]
        if sum(given) != 1:
            raise ValueError("varying_blur needs exactly one of blend (an array [K, S, S], [K, 3, S, S] or [3 K, S, S]), "
                             "blend_path (a .npy file of the same) and psf_grid ((rows, cols) or 'RxC')")
        if given[2]:
            rows, cols = parse_psf_grid(psf_grid)
            if rows * cols != K:
                raise ValueError(f"varying_blur: psf_grid {rows} x {cols} holds {rows * cols} nodes for {K} PSFs; rows * cols must be K")
            maps = grid_blend_weights(S, rows, cols)
        else:
            maps = _load_array("varying_blur", "the blend maps", blend, blend_path)
        if tuple(maps.shape) == (K, S, S):
            maps = np.broadcast_to(maps[:, None], (K, 3, S, S))
        elif tuple(maps.shape) in ((K, 3, S, S), (3 * K, S, S)):
            maps = maps.reshape(K, 3, S, S)
        else:
            raise ValueError(f"varying_blur: the blend maps must have shape [{K}, {S}, {S}], [{K}, 3, {S}, {S}] or [{3 * K}, {S}, {S}] "
                             f"for {K} PSFs on a {S} x {S} image, got {tuple(maps.shape)}")
        if not np.isfinite(maps).all():
            raise ValueError("varying_blur: the blend maps have a non-finite entry")
        for i in range(K):
            if not maps[i].any():
                raise ValueError(f"varying_blur: the blend map of PSF {i} is all zero (drop the PSF instead)")
        self.device = torch.device(device)
        self._set_frames(psfs, "varying_blur", "PSF {}")
        ft = self.frame_taps
        refused = _plan_refusal("fh_conv_blend_plan", S, K, ft.max_taps, ft.halo, 3)
        if refused:
            raise ValueError(f"varying_blur: no kernel runs these tap lists (at most {ft.max_taps} taps per PSF reaching "
                             f"({ft.hy}, {ft.hx})) on a {S} x {S} image (adjoint = {refused[0]}, code {refused[1]})")
        self.blend = torch.from_numpy(np.ascontiguousarray(maps)).to(self.device)  # float64 [K, 3, S, S]
        self.sigma_s = torch.Tensor([sigma_s]).to(self.device)
        self.in_shape = in_shape
        self.out_shape = in_shape

    def apply(self, x, adjoint=False, ctx=None):
        """A (or A^T) of an NCHW tensor [N,3,S,S] -> [N,3,S,S]; float64"""
        S = self.in_shape[-1]
        x64, N, ctx = self._images(x, (3, S, S), ctx)
        return ctx.blur_blend(x64, torch.empty_like(x64), self.frame_taps, self.blend, 3 * N, adjoint)


def poisson_gaussian_sigma(y, gain, read_sigma):
    """Plug-in noise map of a Poisson-Gaussian sensor, sigma = 2 sqrt(gain clip((y + 1) / 2, 0, 1) + read_sigma^2): `y` in the
    [-1, 1] units of the measurements (array or tensor), `gain` and `read_sigma` in intensity units of [0, 1]; the factor 2 maps
    the standard deviation back to [-1, 1].  Evaluated on the measurement itself, it is what a user with real data would pass
    as `noise_map`."""
    gain, read_sigma = float(gain), float(read_sigma)
    if not (np.isfinite(gain) and np.isfinite(read_sigma) and gain >= 0 and read_sigma >= 0 and gain + read_sigma > 0):
        raise ValueError(f"poisson_gaussian_sigma: gain and read_sigma are finite and >= 0, and not both 0; got {gain}, {read_sigma}")
    if torch.is_tensor(y):
        return 2.0 * torch.sqrt(gain * ((y + 1.0) / 2.0).clamp(0.0, 1.0) + read_sigma ** 2)
    return 2.0 * np.sqrt(gain * np.clip((np.asarray(y, dtype=np.float64) + 1.0) / 2.0, 0.0, 1.0) + read_sigma ** 2)


class _NoiseMap:
    """What `weighted_blur` and `weighted_sr` add to their parents: a per-pixel noise level, y = A0 x + n with
    n_i ~ N(0, sigma_i^2) independent, sigma_i in (0, inf], inf = pixel not measured.
      noise_map       array / tensor [n,n], [3,n,n] or [1,3,n,n] at the measurement's side n, in the [-1, 1] units of y; entries
                      > 0 or +inf, not all inf
      noise_map_path  a .npy of the same shapes (instead of `noise_map`)
    Finite entries are clipped from below like the scalar noise level (`_sigma_y2`: 0.001, decimating operators 0.01).
    `noise_map` is float64 [1,3,n,n] on the device, `weights` = 1 / noise_map (0 where inf) what the solver whitens with
    (fh_problem.op 8 .. 11), `mask` = weights > 0.  `sigma_s` is accepted and stored like the parent's, but the solver does not
    read it for these operators.  The adjoint stays unweighted - `transpose` and `forward_adjoint` are A0^T (mask * v) - so DPS
    and DiffPIR treat the operator as they treat `masked_blur`."""
    _NOISE_FLOOR = 0.001

    def _set_noise_map(self, n, noise_map, noise_map_path):
        name = self.name
        noise_map_path = noise_map_path or None
        if (noise_map is None) == (noise_map_path is None):
            raise ValueError(f"{name} needs exactly one of noise_map (an array) and noise_map_path (a .npy file)")
        a = _load_array(name, "the noise map", noise_map, noise_map_path, _image_shapes(n))
        self._set_noise_levels(np.ones((3, n, n)) * a.reshape((1, n, n) if a.ndim == 2 else (3, n, n)))

    def _set_noise_levels(self, a, sites=None):
        """`noise_map`, `weights` and `mask`, float64 [1, C, n, n], from a [C, n, n] array of standard deviations after the
        checks and the floor; `sites` (boolean, the same shape): the entries that are sampled at all, inf elsewhere"""
        name = self.name
        if np.isnan(a).any():
            raise ValueError(f"{name}: the noise map has a NaN entry")
        if not (a > 0).all():
            raise ValueError(f"{name}: the noise map has an entry <= 0 (entries are standard deviations > 0, or +inf for a "
                             "pixel that was not measured)")
        if sites is not None:
            a = np.where(sites, a, np.inf)
        if np.isinf(a).all():
            raise ValueError(f"{name}: the noise map is all inf - no pixel is measured")
        s = np.where(np.isinf(a), a, np.maximum(a, self._NOISE_FLOOR))[None]
        w = np.where(np.isinf(s), 0.0, 1.0 / s)
        self.noise_map = torch.from_numpy(np.ascontiguousarray(s)).to(self.device)
        self.weights = torch.from_numpy(np.ascontiguousarray(w)).to(self.device)
        self.mask = (self.weights > 0).to(F64)

    def _noise(self, y, noiseless):
        # one draw at the measurement shape (the parent's RNG consumption), scaled per pixel; unmeasured pixels read 0
        keep = self.mask.to(y.dtype)
        if not noiseless:
            sig = torch.where(self.mask > 0, self.noise_map, torch.zeros_like(self.noise_map)).to(y.dtype)
            y = y + sig * torch.randn_like(y)
        return y * keep


@register_operator(name="weighted_blur")
class WeightedBlurOperator(_NoiseMap, CustomBlurOperator):
    """`custom_blur` (same PSF arguments, checks and kernels) with a per-pixel noise map at the image's side, see `_NoiseMap`.
    With the 1 x 1 PSF [[1]] it is heteroscedastic denoising."""

    def __init__(self, in_shape, sigma_s, device, kernel_path=None, kernel=None, noise_map=None, noise_map_path=None, **kwargs):
        CustomBlurOperator.__init__(self, in_shape, sigma_s, device, kernel_path=kernel_path, kernel=kernel)
        self._set_noise_map(int(in_shape[-1]), noise_map, noise_map_path)


@register_operator(name="weighted_sr")
class WeightedSROperator(_NoiseMap, CustomSROperator):
    """`custom_sr` (same PSF and factor arguments, checks and routes) with a per-pixel noise map at the LOW-resolution side
    S / scale_factor, see `_NoiseMap`."""
    _NOISE_FLOOR = 0.01

    def __init__(self, in_shape, sigma_s, device, scale_factor=None, kernel_path=None, kernel=None, noise_map=None,
                 noise_map_path=None, **kwargs):
        CustomSROperator.__init__(self, in_shape, sigma_s, device, scale_factor=scale_factor, kernel_path=kernel_path,
                                  kernel=kernel)
        self._set_noise_map(int(in_shape[-1]) // self.scale_factor, noise_map, noise_map_path)


BAYER_PATTERNS = ("rggb", "bggr", "grbg", "gbrg")


def bayer_sites(n, pattern):
    """Boolean [3, n, n] array of a Bayer mosaic (True = the site samples that channel; exactly one channel per site).  The
    four letters of `pattern` are the 2 x 2 cell read row-major - (even row, even column), (even, odd), (odd, even),
    (odd, odd) - with channels r = 0, g = 1, b = 2."""
    if not isinstance(pattern, str) or pattern.lower() not in BAYER_PATTERNS:
        raise ValueError(f"bayer_sites: the pattern is one of {', '.join(BAYER_PATTERNS)}, got {pattern!r}")
    n = int(n)
    sites = np.zeros((3, n, n), dtype=bool)
    for i, letter in enumerate(pattern.lower()):
        sites["rgb".index(letter), i // 2::2, i % 2::2] = True
    return sites


def parse_frame_sigmas(sigmas):
    """`frame_sigmas` as a float64 array: a sequence of numbers, or the command line's "a,b,c" string ("inf" drops a frame)"""
    if isinstance(sigmas, str):
        try:
            sigmas = [float(v) for v in sigmas.split(",") if v.strip()]
        except ValueError:
            raise ValueError(f"weighted_burst_sr: frame_sigmas is 'a,b,c,...' with numbers, got {sigmas!r}") from None
    return np.asarray(sigmas, dtype=np.float64).ravel()


@register_operator(name="weighted_burst_sr")
class WeightedBurstSROperator(_NoiseMap, BurstSROperator):
    """`burst_sr` (same PSF, shift and factor arguments, checks and kernels) with a per-pixel noise level on every frame,
    y_k = (B_k x)[..., ::s, ::s] + n_k with n ~ N(0, diag(sigma^2)), sigma in (0, inf], inf = not measured - see `_NoiseMap`, here
    at the burst's shape: `noise_map`, `weights` and `mask` are float64 [1, 3 K, So, So], frame-major like the measurement
    (channel 3 k + c).  Exactly one noise source:
      noise_map       array / tensor [So,So] or [3,So,So] (the same for every frame), [K,3,So,So], [3K,So,So] or [1,3K,So,So]
      noise_map_path  a .npy of the same shapes
      frame_sigmas    K numbers (or the string "a,b,c"), one level per frame; inf drops a frame
    `mosaic` = "rggb" / "bggr" / "grbg" / "gbrg" (`bayer_sites`, the same pattern for every frame) sets the entries of the
    channels a site does not sample to inf on top of that source: joint demosaicing and super-resolution from raw frames.
    The solver's system is fh_problem.op = 13; the adjoint stays unweighted, `transpose` = `forward_adjoint` = A^T (mask * v)."""
    _NOISE_FLOOR = 0.01

    def __init__(self, in_shape, sigma_s, device, scale_factor=None, kernels=None, kernel_path=None, frame_shifts=None,
                 noise_map=None, noise_map_path=None, frame_sigmas=None, mosaic=None, **kwargs):
        BurstSROperator.__init__(self, in_shape, sigma_s, device, scale_factor=scale_factor, kernels=kernels,
                                 kernel_path=kernel_path, frame_shifts=frame_shifts)
        name, K, n = self.name, self.nframes, self.out_shape[-1]
        noise_map_path = noise_map_path or None
        if isinstance(frame_sigmas, str) and frame_sigmas == "":
            frame_sigmas = None
        if sum(v is not None for v in (noise_map, noise_map_path, frame_sigmas)) != 1:
            raise ValueError(f"{name} needs exactly one of noise_map (an array), noise_map_path (a .npy file) and frame_sigmas "
                             "(one noise level per frame)")
        if mosaic is not None and not (isinstance(mosaic, str) and mosaic == ""):
            if not isinstance(mosaic, str) or mosaic.lower() not in BAYER_PATTERNS:
                raise ValueError(f"{name}: mosaic is None or one of {', '.join(BAYER_PATTERNS)}, got {mosaic!r}")
            mosaic = mosaic.lower()
        else:
            mosaic = None
        if frame_sigmas is not None:
            fs = parse_frame_sigmas(frame_sigmas)
            if fs.size != K:
                raise ValueError(f"{name}: {fs.size} frame_sigmas for {K} frames; give one noise level per frame")
            a = np.repeat(fs, 3)[:, None, None] * np.ones((3 * K, n, n))
        else:
            shapes = ((n, n), (3, n, n), (K, 3, n, n), (3 * K, n, n), (1, 3 * K, n, n))
            a = _load_array(name, "the noise map", noise_map, noise_map_path, shapes)
            if a.ndim == 2 or a.shape == (3, n, n):  # one map for every frame ((3, n, n) is also (3 K, n, n) at K = 1: the same)
                a = np.broadcast_to(a.reshape((1, 1, n, n) if a.ndim == 2 else (1, 3, n, n)), (K, 3, n, n))
        self.mosaic = mosaic
        self._set_noise_levels(np.ascontiguousarray(a).reshape(3 * K, n, n),
                               None if mosaic is None else np.tile(bayer_sites(n, mosaic), (K, 1, 1)))


def folded_dct_hartley_bases(S, use_dct=True):
    """The bases of `fourier_sampling` (fh_problem.op = 15), float64 (Hc, P), C-contiguous [S][S]:
        Hc[u][n] = (cos + sin)(2 pi u n / S) / sqrt(S)      symmetric, Hc Hc = I;
        P        = C_dct Hc  (use_dct)  or  Hc              what folds into the solver's dense passes.
    The 2-D discrete Hartley transform H x = Re F x - Im F x (F orthonormal) is R(Hc x Hc) with the butterfly R of
    fh_hartley_fix, so dct2(H u) = P R(u) P^T and H (idct2 v) = R(P^T v P).  Built in extended precision like
    `dct_basis_longdouble` - the angle reduced with the integer (u n) mod S before it meets 2 pi / S - and rounded once."""
    S = int(S)
    if S < 2 or S % 2:
        raise ValueError(f"folded_dct_hartley_bases: the side must be even and >= 2, got {S}")
    ld = np.longdouble
    k = (np.arange(S, dtype=np.int64)[:, None] * np.arange(S, dtype=np.int64)[None, :]) % S
    ang = k.astype(ld) * (2 * np.arccos(ld(-1)) / ld(S))
    Hc = (np.cos(ang) + np.sin(ang)) / np.sqrt(ld(S))
    P = dct_basis_longdouble(S) @ Hc if use_dct else Hc
    f = lambda M: np.ascontiguousarray(M.astype(np.float64))
    return f(Hc), f(P)


def _reflect(a):
    """a[..., (-u) % S, (-v) % S]: the point reflection of an FFT-ordered grid about DC"""
    return np.roll(np.flip(a, axis=(-2, -1)), 1, axis=(-2, -1))


KSPACE_PATTERNS = ("cartesian", "radial")


def kspace_mask(S, pattern="cartesian", acceleration=4.0, center_fraction=0.08, seed=0):
    """A 0/1 sampling mask on the [S, S] frequency grid in FFT order (DC at [0, 0], -u = (S - u) % S), float64.
      cartesian  whole lines along the second axis (u fixed): the centre band |u| <= h with 2 h + 1 the odd count nearest to
                 center_fraction * S, plus lines outside it drawn at random in +-u pairs until the sampled fraction is
                 1 / acceleration + center_fraction to within one line (all lines when that asks for more than there are)
      radial     ceil(S / acceleration) straight spokes through DC at evenly spaced angles with one random offset;
                 `center_fraction` is not read
    Both are symmetric under the point reflection k -> -k by construction (a real image's sample at k is its sample at -k),
    sample DC, and are deterministic in `seed`."""
    S = int(S)
    if S < 2 or S % 2:
        raise ValueError(f"kspace_mask: the side must be even and >= 2, got {S}")
    if pattern not in KSPACE_PATTERNS:
        raise ValueError(f"kspace_mask: the pattern is one of {', '.join(KSPACE_PATTERNS)}, got {pattern!r}")
    try:
        acc, cf = float(acceleration), float(center_fraction)
    except (TypeError, ValueError):
        raise ValueError(f"kspace_mask: acceleration and center_fraction are numbers, got {acceleration!r}, {center_fraction!r}") from None
    if not (np.isfinite(acc) and acc >= 1.0):
        raise ValueError(f"kspace_mask: acceleration is a finite number >= 1, got {acceleration!r}")
    if not (np.isfinite(cf) and 0.0 <= cf < 1.0):
        raise ValueError(f"kspace_mask: center_fraction is in [0, 1), got {center_fraction!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError(f"kspace_mask: seed is a non-negative integer, got {seed!r}")
    rng = np.random.default_rng(int(seed))
    m = np.zeros((S, S))
    if pattern == "cartesian":
        h = min(max(int(round((cf * S - 1.0) / 2.0)), 0), S // 2 - 1)
        lines = np.zeros(S, dtype=bool)
        lines[np.minimum(np.arange(S), S - np.arange(S)) <= h] = True  # DC and the pairs +-1 .. +-h
        pool = np.arange(h + 1, S // 2)  # the proper pairs (u, S - u) outside the band; S / 2 is its own reflection
        pairs = int(round((S * (1.0 / acc + cf) - (2 * h + 1)) / 2.0))
        if pairs >= pool.size:
            lines[:] = True
        elif pairs > 0:
            u = rng.choice(pool, size=pairs, replace=False)
            lines[u] = True
            lines[S - u] = True
        m[lines, :] = 1.0
        return m
    n = int(np.ceil(S / acc))
    theta = np.pi * (np.arange(n) + rng.random()) / n
    t = np.arange(0.0, S / 2 + 0.25, 0.5)  # half a spoke; the other half is its reflection
    u = np.rint(t[None, :] * np.cos(theta)[:, None]).astype(np.int64).ravel()
    v = np.rint(t[None, :] * np.sin(theta)[:, None]).astype(np.int64).ravel()
    m[u % S, v % S] = 1.0
    m[(-u) % S, (-v) % S] = 1.0
    return m


def _kspace_sigma(sigma, S, what):
    s = np.asarray(sigma, dtype=np.float64)
    if s.ndim == 0:
        s = np.full((S, S), float(s))
    if s.shape != (S, S) or np.isnan(s).any() or not (s > 0).all():
        raise ValueError(f"{what}: sigma is a number > 0 or an [{S}, {S}] map of such (inf = not measured)")
    return s


def kspace_to_hartley(F, mask, sigma):
    """Complex k-space samples -> the Hartley-domain measurement of `fourier_sampling`.
      F      complex [..., S, S], orthonormal DFT samples in FFT order; read only where `mask` is 1
      mask   0/1 [S, S]: which samples were taken (need not be symmetric)
      sigma  the noise level PER COMPONENT (real and imaginary part each), a number or an [S, S] map
    Returns (y, mask_sym, noise_map): y real [..., S, S] with y[k] = Re F~[k] - Im F~[k] (0 off the mask), mask_sym the mask OR
    its point reflection, noise_map float64 [S, S] (inf off the mask).  F~ is the Hermitian completion: (H[k], H[-k]) is the
    rotation of (Re F[k], Im F[k]) scaled by sqrt 2, so
      only one of k, -k measured   the conjugate is filled in; both Hartley entries get sqrt(2) sigma
      both measured                they are averaged, (F[k] + conj F[-k]) / 2; the entries get sqrt((s_k^2 + s_-k^2) / 2) = sigma
      k = -k (self-conjugate)      the imaginary part is dropped; the entry gets sigma"""
    F = np.asarray(F)
    S = F.shape[-1]
    if F.ndim < 2 or F.shape[-2] != S or S % 2:
        raise ValueError(f"kspace_to_hartley: F must be [..., S, S] with S even, got shape {tuple(F.shape)}")
    m = np.asarray(mask, dtype=np.float64)
    if m.shape != (S, S) or not np.isin(m, (0.0, 1.0)).all():
        raise ValueError(f"kspace_to_hartley: the mask must be a 0/1 array of shape ({S}, {S})")
    s = _kspace_sigma(sigma, S, "kspace_to_hartley")
    m = m * np.isfinite(s)
    if not m.any():
        raise ValueError("kspace_to_hartley: no sample is measured")
    mr, sr = _reflect(m), _reflect(np.where(m > 0, s, 0.0))
    s = np.where(m > 0, s, 0.0)
    Fm = np.where(m > 0, F.astype(np.complex128), 0.0)
    Fr = np.conj(_reflect(Fm))  # conj F[-k], 0 where -k was not measured
    cnt = m + mr
    Ft = (Fm + Fr) / np.maximum(cnt, 1.0)
    idx = np.arange(S)
    selfc = ((idx[:, None] * 2) % S == 0) & ((idx[None, :] * 2) % S == 0)
    var = np.where(cnt == 2, (s ** 2 + sr ** 2) / 2.0, 2.0 * (s ** 2 + sr ** 2))  # one measured: 2 sigma^2 (the other term is 0)
    var = np.where(selfc, s ** 2, var)
    msym = (cnt > 0).astype(np.float64)
    y = np.where(msym > 0, Ft.real - Ft.imag, 0.0)
    return y, msym, np.where(msym > 0, np.sqrt(var), np.inf)


def hartley_to_kspace(y, mask=None):
    """The inverse of `kspace_to_hartley`: F[k] = (H[k] + H[-k]) / 2 + i (H[-k] - H[k]) / 2, complex128 [..., S, S] (times `mask`,
    the symmetric 0/1 mask, when one is given)."""
    y = np.asarray(y, dtype=np.float64)
    yr = _reflect(y)
    F = 0.5 * (y + yr) + 0.5j * (yr - y)
    return F if mask is None else F * np.asarray(mask, dtype=np.float64)


_HARTLEY_CACHE = {}


@register_operator(name="fourier_sampling")
class FourierSamplingOperator(_NoiseMap, _ImageOperator):
    """Undersampled Fourier-domain measurement, y = M (H x + n): H the orthonormal 2-D discrete Hartley transform
    H x = Re F x - Im F x per channel - real, symmetric, self-inverse, and an exact re-expression of k-space data (a sample at k
    with iid complex noise is the two Hartley samples at k and -k with iid noise; `kspace_to_hartley` converts) - and M a 0/1
    sampling mask on the [S, S] frequency grid in FFT order (DC at [0, 0]).  Covers Cartesian and radial k-space undersampling
    and aperture-synthesis uv coverage with one weight per visibility.  Exactly one mask source:
      mask       array / tensor [S,S], [3,S,S] or [1,3,S,S], entries exactly 0 or 1
      mask_path  a .npy of the same shapes
      pattern    "cartesian" or "radial": `kspace_mask(S, pattern, acceleration, center_fraction, seed)`
    The mask is made symmetric by OR with its point reflection m[-u][-v]: for a real image a sample at k IS a sample at -k (its
    conjugate), so both Hartley entries are known.  An all-zero mask is refused.  Optional `noise_map` / `noise_map_path`: the
    per-entry noise level on the same grid, `_NoiseMap`'s rules (entries > 0 or +inf, floor 0.001); entries off the mask count as
    inf.  `weights` is always present - the mask, or 1 / noise_map (0 off the mask or where inf) - and is what the solver
    whitens with (fh_problem.op = 15; sigma_y2 = clip(sigma_s, 0.001)^2 without a map, 1 with one).
    `forward` = mask * (H x + n), `transpose` = `forward_adjoint` = H (mask * v)."""

    def __init__(self, in_shape, sigma_s, device, mask=None, mask_path=None, pattern=None, acceleration=4.0, center_fraction=0.08,
                 seed=0, noise_map=None, noise_map_path=None, **kwargs):
        name = self.name
        S = int(in_shape[-1])
        if S < 2 or S % 2 or int(in_shape[-2]) != S:
            raise ValueError(f"{name}: the image must be square with an even side, got {tuple(in_shape)}")
        mask_path, pattern, noise_map_path = mask_path or None, pattern or None, noise_map_path or None
        if sum(v is not None for v in (mask, mask_path, pattern)) != 1:
            raise ValueError(f"{name} needs exactly one of mask (an array), mask_path (a .npy file) and pattern "
                             f"({' / '.join(KSPACE_PATTERNS)}, with acceleration, center_fraction, seed)")
        if pattern is not None:
            a = kspace_mask(S, pattern, acceleration, center_fraction, seed)
        else:
            a = _load_array(name, "the mask", mask, mask_path, _image_shapes(S))
        if not np.isin(a, (0.0, 1.0)).all():
            raise ValueError(f"{name}: the mask has an entry other than 0 and 1 (per-entry noise levels go in noise_map)")
        m = np.ones((1, 3, S, S)) * a.reshape((1, 1, S, S) if a.ndim == 2 else (1, 3, S, S))
        m = np.maximum(m, _reflect(m))
        if not m.any():
            raise ValueError(f"{name}: the mask is all zero - no frequency is measured")
        self.device = torch.device(device)
        self.sigma_s = torch.Tensor([sigma_s]).to(self.device)
        self.in_shape = in_shape
        self.out_shape = tuple(in_shape)
        self.mask = torch.from_numpy(np.ascontiguousarray(m)).to(self.device)  # float64 [1,3,S,S]
        if noise_map is None and noise_map_path is None:
            self.noise_map = None
            self.weights = self.mask
        else:
            self._set_noise_map(S, noise_map, noise_map_path)  # noise_map, weights, mask = weights > 0 of the map alone
            w = self.weights * torch.from_numpy(m).to(self.device)
            if not bool((w > 0).any()):
                raise ValueError(f"{name}: no frequency is both on the mask and finite in the noise map")
            self.noise_map = torch.where(w > 0, self.noise_map, torch.full_like(self.noise_map, float("inf")))
            self.weights = w.contiguous()
            self.mask = (w > 0).to(F64)

    def _noise(self, y, noiseless):
        if self.noise_map is not None:
            return _NoiseMap._noise(self, y, noiseless)
        return LinearOperator._noise(self, y, noiseless) * self.mask.to(y.dtype)

    def hartley_basis(self):
        """Hc of `folded_dct_hartley_bases` on the device, built once per (side, device)"""
        return self.folded_hartley_bases(False)[0]

    def folded_hartley_bases(self, use_dct, device=None):
        """device copies (P, P^T) of `folded_dct_hartley_bases` - fold_fwd_* and fold_inv_* of fh_problem.op = 15"""
        S, dev = int(self.in_shape[-1]), torch.device(device if device is not None else self.device)
        key = (S, bool(use_dct), str(dev))
        if key not in _HARTLEY_CACHE:
            P = folded_dct_hartley_bases(S, use_dct)[1]
            _HARTLEY_CACHE[key] = (torch.from_numpy(P).to(dev), torch.from_numpy(np.ascontiguousarray(P.T)).to(dev))
        return _HARTLEY_CACHE[key]

    def apply(self, x, adjoint=False, ctx=None):
        """H x of an NCHW tensor [N,3,S,S]; float64.  H is its own adjoint: `adjoint` is ignored."""
        S = self.in_shape[-1]
        x64, _N, ctx = self._images(x, (3, S, S), ctx)
        return ctx.hartley2d(x64, torch.empty_like(x64), self.hartley_basis())


def _cubic(x):
    ax = np.abs(x)
    return ((1.5 * ax ** 3 - 2.5 * ax ** 2 + 1) * (ax <= 1)
            + (-0.5 * ax ** 3 + 2.5 * ax ** 2 - 4 * ax + 2) * ((1 < ax) & (ax <= 2)))


def resize_matrix(n_in, scale):
    """[n_out, n_in] float32 matrix of the antialiased cubic Resizer along one axis (resizer.py:103-160)."""
    n_out = int(np.ceil(n_in * scale))
    width = 4.0 / scale
    centre = (np.arange(1, n_out + 1) - (n_out - n_in * scale) / 2) / scale + 0.5 * (1 - 1 / scale)
    first = np.floor(centre - width / 2)
    pos = (first[:, None] + np.arange(np.ceil(width) + 2) - 1).astype(np.int64)
    wgt = scale * _cubic(scale * (centre[:, None] - pos - 1))
    norm = wgt.sum(1, keepdims=True)
    norm[norm == 0] = 1.0
    wgt = (wgt / norm).astype(np.float32)
    fold = np.concatenate((np.arange(n_in), np.arange(n_in - 1, -1, -1)))
    pos = fold[np.mod(pos, 2 * n_in)]
    R = np.zeros((n_out, n_in), dtype=np.float32)
    np.add.at(R, (np.repeat(np.arange(n_out), pos.shape[1]), pos.reshape(-1)), wgt.reshape(-1))
    return torch.from_numpy(R)


@register_operator(name="super_resolution")
class SuperResolutionOperator(LinearOperator):  # measurements.py:87-123
    decimates = True

    def __init__(self, in_shape, scale_factor, sigma_s, device, **kwargs):
        self.device = torch.device(device)
        self.scale_factor = int(scale_factor)
        self.sigma_s = torch.Tensor([sigma_s]).to(self.device)
        kernels = scipy.io.loadmat(os.path.join(KERNEL_DIR, "kernels_bicubicx234.mat"))["kernels"]
        k_index = self.scale_factor - 2 if self.scale_factor < 5 else 2
        self.kernel = kernels[0, k_index].astype(np.float64)
        self.taps = Taps(self.kernel, self.device)
        self.in_shape = in_shape
        self.out_shape = (1, 3, int(in_shape[-2] / self.scale_factor), int(in_shape[-1] / self.scale_factor))
        self._R = resize_matrix(in_shape[-1], 1.0 / self.scale_factor).to(self.device)

    def forward(self, data, flatten=False, noiseless=False):
        # the *measurement* is the antialiased bicubic Resizer (one-off per image, outside the solver loop);
        # the solver's A is blur(25x25 bicubic PSF) + decimation
        R = self._R.to(data.dtype)
        y = torch.einsum("oh,nchw->ncow", R, data.to(self.device))
        y = torch.einsum("pw,ncow->ncop", R, y)
        y = self._noise(y, noiseless)
        self._last_y = y
        if flatten:
            return y, y.reshape(y.shape[0], -1)
        return y

    def forward_adjoint(self, v):
        """exact adjoint of the noiseless `forward` (the antialiased bicubic Resizer), for DPS; `transpose` is the solver's A^T"""
        R = self._R.to(v.dtype)
        return torch.einsum("oh,pw,ncop->nchw", R, R, v.to(self.device))

    def get_kernel(self):
        return self.taps.kernel.view(1, 1, *self.taps.kernel.shape).to(self.device)


@register_operator(name="inpainting")
class InpaintingOperator(LinearOperator):  # measurements.py:204-246
    def __init__(self, device, sigma_s, mask_opt, mask=None, **kwargs):
        self.device = torch.device(device)
        self.sigma_s = torch.Tensor([sigma_s]).to(self.device)
        self.in_shape = (1, 3, mask_opt["image_size"], mask_opt["image_size"])
        self.mask = self.generate_mask(mask_opt) if mask is None else mask.to(self.device)

    def apply(self, x, adjoint=False, ctx=None):
        """mask * x in float64 (A = A^T, no kernel: the solver forms this family's right-hand side itself)"""
        return x.detach().to(device=self.device, dtype=F64) * self.mask.to(F64)

    def forward(self, data, flatten=False, noiseless=False):
        y = self._noise(data.clone(), noiseless) * self.mask.to(data.dtype)
        if flatten:
            idx = torch.where(self.mask > 0)
            return y, y[..., idx[-3], idx[-2], idx[-1]]
        return y

    def forward_adjoint(self, v):
        return v * self.mask.to(v.dtype)

    def transpose(self, data, flatten=False):
        y = data.clone()
        if flatten:
            idx = torch.where(self.mask > 0)
            x = torch.zeros(y.shape[0], *self.in_shape[-3:], device=self.device)
            x[..., idx[-3], idx[-2], idx[-1]] = y
            return x
        return y

    def generate_mask(self, mask_opt):
        img = torch.randn(*self.in_shape).to(self.device)  # consumes the global torch RNG like the reference (:244)
        return MaskGenerator(**mask_opt)(img)


def _channel_weights(channel_weights):
    w = (1.0 / 3.0,) * 3 if channel_weights is None else channel_weights
    try:
        w = tuple(float(v) for v in w)
    except (TypeError, ValueError):
        raise ValueError(f"channel_weights must be three finite numbers, got {channel_weights!r}") from None
    if len(w) != 3 or not all(np.isfinite(v) for v in w):
        raise ValueError(f"channel_weights must be three finite numbers, got {channel_weights!r}")
    return w


@register_operator(name="colorization")
class ColorizationOperator(LinearOperator):  # measurements.py:74-84 (A = mean over the colour channels)
    """y = sum_c w_c x_c + noise, one measurement plane per image.  `channel_weights` defaults to (1/3, 1/3, 1/3), the
    reference's `mean(dim=1)`; the weights are shared by every image of a lock-step batch.  Forward and adjoint run in
    float64 through fh_channel_mix."""
    keeps_last_y = False

    def __init__(self, in_shape, sigma_s, device, channel_weights=None, **kwargs):
        self.device = torch.device(device)
        self.sigma_s = torch.Tensor([sigma_s]).to(self.device)
        self.in_shape = in_shape
        self.out_shape = (1, 1, in_shape[-2], in_shape[-1])
        self.channel_weights = _channel_weights(channel_weights)
        self._w = None  # the three weights on the device, created on first use

    @property
    def weights(self):
        if self._w is None:
            self._w = torch.tensor(self.channel_weights, dtype=F64, device=self.device)
        return self._w

    def apply(self, x, adjoint=False, ctx=None):
        """float64 channel mix of an NCHW tensor ([N,3,S,S] -> [N,1,S,S], or its adjoint); returns float64."""
        S = self.in_shape[-1]
        x64 = x.detach().to(device=self.device, dtype=F64).reshape(-1, 1 if adjoint else 3, S, S).contiguous()
        out = torch.empty(x64.shape[0], 3 if adjoint else 1, S, S, dtype=F64, device=self.device)
        return (self._ctx() if ctx is None else ctx).channel_mix(x64, out, self.weights, adjoint)

    _mix = apply


@register_operator(name="noise")
class DenoiseOperator(LinearOperator):  # measurements.py:56-72 (A = I)
    """y = x + sigma_s * randn.  Deviation from the reference: its class takes no `noiseless` argument and adds no noise
    at all, so its own sampler (which calls `forward(x, noiseless=...)`) cannot run it; here `forward` has the signature
    of the other operators and adds the measurement noise.  The solvers treat it as inpainting with an all-ones mask."""

    def __init__(self, in_shape, sigma_s, device, **kwargs):
        self.device = torch.device(device)
        self.sigma_s = torch.Tensor([sigma_s]).to(self.device)
        self.in_shape = in_shape
        self.out_shape = tuple(in_shape)
        self.mask = torch.ones(1, *in_shape[-3:], device=self.device)

    apply = InpaintingOperator.apply  # (the all-ones mask)

    def forward(self, data, flatten=False, noiseless=False):
        y = self._noise(data.clone(), noiseless)
        if flatten:
            return y, y.reshape(y.shape[0], -1)
        return y

    def transpose(self, data, flatten=False):
        y = data.clone()
        if flatten:
            return y.reshape(y.shape[0], *self.in_shape[-3:])
        return y

    def forward_adjoint(self, v):
        return v


class MaskGenerator:  # measurements.py:248-318 (random / box / extreme; global numpy RNG, as the reference)
    def __init__(self, mask_type, mask_len_range=None, mask_prob_range=None, image_size=256, margin=(16, 16)):
        assert mask_type in ["box", "random", "both", "extreme"]
        self.mask_type, self.mask_len_range, self.mask_prob_range = mask_type, mask_len_range, mask_prob_range
        self.image_size, self.margin = image_size, margin

    def __call__(self, img):
        if self.mask_type == "random":
            return self._random(img)
        mask = self._box(img)
        return 1.0 - mask if self.mask_type == "extreme" else mask

    def _random(self, img):
        n = self.image_size ** 2
        prob = np.random.uniform(*self.mask_prob_range)
        keep = torch.ones(n)
        keep[np.random.choice(n, int(n * prob), replace=False)] = 0
        return keep.view(1, 1, self.image_size, self.image_size).expand(img.shape[0], img.shape[1], -1, -1) \
                   .contiguous().to(img.device)

    def _box(self, img):
        lo, hi = int(self.mask_len_range[0]), int(self.mask_len_range[1])
        h, w = np.random.randint(lo, hi), np.random.randint(lo, hi)
        mh, mw = self.margin
        t = np.random.randint(mh, self.image_size - mh - h)
        l = np.random.randint(mw, self.image_size - mw - w)
        mask = torch.ones_like(img)
        mask[..., t:t + h, l:l + w] = 0
        return mask
