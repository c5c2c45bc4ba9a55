"""The kernels between the UNet's convolutions and GroupNorms, per entry point: fh_resample2x, fh_concat_channels,
fh_layout_nchw_nhwc, fh_add_f32 and fh_absmax_f32 (csrc/fh_unet.hip).  free-hunch_amd/unet_hip.py launches them; the other
GPU tests reach them only through whole-network comparisons at batch 1 or 2.

What the shapes are for.  k_resample, k_concat, k_add_f32, k_nchw_to_nhwc and k_nhwc_to_nchw are grid-stride loops whose grid
is capped at 4096 blocks of 256 threads: beyond 1,048,576 work items a thread takes a second trip, which the full-size
network does at batch 4 and 8 and no network test does - one shape per kernel here has more items than that.  The small
shapes have one pixel, one row, odd extents and C / 4 that is no power of two.  fh_layout_nchw_nhwc promises zero padding
channels one way and ignores them the other way: the output starts as NaN, and the ignored input channels hold NaN.
fh_absmax_f32 has a float4 body and a scalar tail: sizes with n % 4 != 0 and the maximum in either.

Every output is a `Guarded32` (tests/test_attention_paths_gpu.py): NaN before the call, sentinels behind it."""
import pytest
import torch
import torch.nn.functional as F

from test_attention_paths_gpu import Guarded32, U

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
ONE_TRIP = 4096 * 256  # work items a capped grid covers in its first trip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _lib():
    from free_hunch_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------- a. fh_resample2x
def _resample(dev, x, shape, mode):
    """fh_resample2x of x into a guarded buffer; shape = (N, Hs, Ws, C), the SMALL side"""
    L, lib = _lib()
    N, Hs, Ws, C = shape
    big, small = (N, 2 * Hs, 2 * Ws, C), (N, Hs, Ws, C)
    assert tuple(x.shape) == (big if mode in (0, 3) else small)
    g = Guarded32(small if mode in (0, 3) else big, dev)
    L.check(lib.fh_resample2x(x.data_ptr(), g.ptr(), N, Hs, Ws, C, mode, L.stream()), "resample")
    return g.check(("resample", shape, mode))


def _pool64(x):
    """2 x 2 average pool of NHWC x in float64"""
    return F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)


def _up(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def _check_resample(dev, shape, mode):
    N, Hs, Ws, C = shape
    if mode in (0, 3):  # big -> small: three float32 additions (and an exact power-of-two factor)
        x = torch.randn(N, 2 * Hs, 2 * Ws, C, device=dev)
        out = _resample(dev, x, shape, mode)
        f = 0.25 if mode == 0 else 1.0
        ref = 4 * f * _pool64(x)
        bound = 3 * U * f * 4 * _pool64(x.abs())  # 3 2^-24 f (|a| + |b| + |c| + |d|)
        d = (out.double() - ref).abs()
        assert bool((d <= bound).all()), (shape, mode, float((d / bound.clamp_min(1e-300)).max()))
    else:  # small -> big: a copy, a copy times 0.25, or zero insertion - exact
        x = torch.randn(N, Hs, Ws, C, device=dev)
        out = _resample(dev, x, shape, mode)
        if mode == 4:
            ref = torch.zeros(N, 2 * Hs, 2 * Ws, C, device=dev)
            ref[:, ::2, ::2] = x
        else:
            ref = _up(x * 0.25 if mode == 1 else x)
        assert torch.equal(out, ref), (shape, mode)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 1, 9, 4), (3, 5, 7, 36)])
def test_resample_modes_at_small_shapes(dev, shape, mode):
    """All five modes against F.avg_pool2d / repeat_interleave in float64.  Modes 1, 2 and 4 are exact (mode 4 has to write its
    zeros: the output starts as NaN); modes 0 and 3 within 3 2^-24 f (|a| + |b| + |c| + |d|) elementwise, f = 0.25 or 1."""
    _check_resample(dev, shape, mode)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_resample_second_grid_stride_trip(dev, mode):
    """More than 4096 x 256 float4 items, as the full-size network at batch 4 or 8: (2, 96, 88, 64) small -> big and
    (2, 96, 88, 256) big -> small, both 1,081,344 items."""
    shape = (2, 96, 88, 256) if mode in (0, 3) else (2, 96, 88, 64)
    N, Hs, Ws, C = shape
    assert N * Hs * Ws * (C // 4) * (1 if mode in (0, 3) else 4) > ONE_TRIP
    _check_resample(dev, shape, mode)


@pytest.mark.parametrize("shape", [(2, 1, 9, 4), (3, 5, 7, 36)])
def test_resample_adjoint_pairs(dev, shape):
    """<mode0(x), y> = <x, mode1(y)> and <mode2(y), x> = <y, mode3(x)> in float64, within 1e-6 |x| |y|"""
    N, Hs, Ws, C = shape
    x = torch.randn(N, 2 * Hs, 2 * Ws, C, device=dev)
    y = torch.randn(N, Hs, Ws, C, device=dev)
    tol = 1e-6 * float(x.double().norm() * y.double().norm())
    dot = lambda a, b: float((a.double() * b.double()).sum())  # noqa: E731
    assert abs(dot(_resample(dev, x, shape, 0), y) - dot(x, _resample(dev, y, shape, 1))) <= tol
    assert abs(dot(_resample(dev, y, shape, 2), x) - dot(y, _resample(dev, x, shape, 3))) <= tol


def test_resample_refuses_bad_arguments(dev):
    L, lib = _lib()
    x = torch.zeros(1, 4, 4, 8, device=dev)
    g = Guarded32((1, 4, 4, 8), dev)
    assert lib.fh_resample2x(x.data_ptr(), g.ptr(), 1, 2, 2, 6, 0, L.stream()) == L.FH_EINVAL  # C % 4 != 0
    assert lib.fh_resample2x(x.data_ptr(), g.ptr(), 1, 2, 2, 8, 5, L.stream()) == L.FH_EINVAL  # mode 5
    torch.cuda.synchronize()
    assert bool(torch.isnan(g.out).all())


# ---------------------------------------------------------------- b. fh_concat_channels
@pytest.mark.parametrize("P,Ca,Cb", [(1, 4, 4), (35, 4, 100), (35, 96, 32), (70000, 32, 32)])
def test_concat_and_split_channels(dev, P, Ca, Cb):
    """split = 0 equals torch.cat bit for bit; split = 1 into guarded a, b equals the slices bit for bit and leaves `out` as
    it was.  (70000, 32, 32): 1,120,000 float4 items, a second grid-stride trip."""
    L, lib = _lib()
    assert (P * (Ca + Cb) // 4 > ONE_TRIP) == (P == 70000)
    a, b = torch.randn(P, Ca, device=dev), torch.randn(P, Cb, device=dev)
    out = Guarded32((P, Ca + Cb), dev)
    L.check(lib.fh_concat_channels(a.data_ptr(), b.data_ptr(), out.ptr(), P, Ca, Cb, 0, L.stream()), "concat")
    cat = torch.cat([a, b], dim=1)
    assert torch.equal(out.check(("concat", P, Ca, Cb)), cat)
    ga, gb = Guarded32((P, Ca), dev), Guarded32((P, Cb), dev)
    L.check(lib.fh_concat_channels(ga.ptr(), gb.ptr(), out.ptr(), P, Ca, Cb, 1, L.stream()), "split")
    assert torch.equal(ga.check("split a"), a) and torch.equal(gb.check("split b"), b)
    assert torch.equal(out.check("split source"), cat)


def test_concat_refuses_channels_off_the_float4_grid(dev):
    L, lib = _lib()
    a, b = torch.zeros(3, 6, device=dev), torch.zeros(3, 4, device=dev)
    out = Guarded32((3, 10), dev)
    assert lib.fh_concat_channels(a.data_ptr(), b.data_ptr(), out.ptr(), 3, 6, 4, 0, L.stream()) == L.FH_EINVAL
    assert lib.fh_concat_channels(b.data_ptr(), a.data_ptr(), out.ptr(), 3, 4, 6, 0, L.stream()) == L.FH_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.out).all())


# ---------------------------------------------------------------- c. fh_layout_nchw_nhwc
@pytest.mark.parametrize("N,C,P,Cp", [(1, 3, 1, 32), (2, 3, 35, 32), (2, 6, 35, 6), (1, 5, 7, 8), (2, 3, 20000, 32)])
def test_layout_to_nhwc_zeroes_the_padding_channels(dev, N, C, P, Cp):
    """[N][C][P] -> [N][P][Cp]: the real channels equal the permute bit for bit, channels C .. Cp - 1 are exactly 0 (the
    output starts as NaN).  (2, 3, 20000, 32): 1,280,000 elements, a second grid-stride trip."""
    L, lib = _lib()
    x = torch.randn(N, C, P, device=dev)
    out = Guarded32((N, P, Cp), dev)
    L.check(lib.fh_layout_nchw_nhwc(x.data_ptr(), out.ptr(), N, C, P, Cp, 1, L.stream()), "layout")
    y = out.check(("to nhwc", N, C, P, Cp))
    assert torch.equal(y[..., :C], x.permute(0, 2, 1))
    assert bool((y[..., C:] == 0).all())


@pytest.mark.parametrize("N,C,P,Cp", [(1, 3, 1, 32), (2, 3, 35, 32), (2, 6, 35, 6), (1, 5, 7, 8), (2, 3, 20000, 32),
                                      (2, 6, 90000, 8)])
def test_layout_to_nchw_ignores_the_padding_channels(dev, N, C, P, Cp):
    """[N][P][Cp] -> [N][C][P] from a buffer whose padding channels hold NaN: no NaN comes out, and the result equals the
    permute bit for bit.  This direction loops over N C P elements: (2, 6, 90000, 8) is its second-trip shape."""
    L, lib = _lib()
    assert (N * C * P > ONE_TRIP) == (P == 90000)
    x = torch.full((N, P, Cp), float("nan"), device=dev)
    x[..., :C] = torch.randn(N, P, C, device=dev)
    out = Guarded32((N, C, P), dev)
    L.check(lib.fh_layout_nchw_nhwc(x.data_ptr(), out.ptr(), N, C, P, Cp, 0, L.stream()), "layout")
    assert torch.equal(out.check(("to nchw", N, C, P, Cp)), x[..., :C].permute(0, 2, 1))


def test_layout_refuses_fewer_padded_channels_than_channels(dev):
    L, lib = _lib()
    x = torch.zeros(1, 8, 5, device=dev)
    out = Guarded32((1, 5, 8), dev)
    for to_nhwc in (0, 1):
        assert lib.fh_layout_nchw_nhwc(x.data_ptr(), out.ptr(), 1, 8, 5, 4, to_nhwc, L.stream()) == L.FH_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.out).all())


# ---------------------------------------------------------------- d. fh_add_f32
@pytest.mark.parametrize("n", [4, 1028, 4_200_000])
def test_add_equals_torch(dev, n):
    """a + b bit for bit; n = 4,200,000 is 1,050,000 float4 items, a second grid-stride trip"""
    L, lib = _lib()
    a, b = torch.randn(n, device=dev), torch.randn(n, device=dev)
    out = Guarded32((n,), dev)
    L.check(lib.fh_add_f32(a.data_ptr(), b.data_ptr(), out.ptr(), n, L.stream()), "add")
    assert torch.equal(out.check(("add", n)), a + b)


def test_add_refuses_sizes_off_the_float4_grid(dev):
    L, lib = _lib()
    a = torch.zeros(8, device=dev)
    out = Guarded32((8,), dev)
    assert lib.fh_add_f32(a.data_ptr(), a.data_ptr(), out.ptr(), 6, L.stream()) == L.FH_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.out).all())


# ---------------------------------------------------------------- e. fh_absmax_f32
AMAX_SLOTS = 16  # FH_AMAX_SLOTS of include/fh_hip.h


def _absmax(dev, x, nan_expected=False):
    L, lib = _lib()
    slots = Guarded32((AMAX_SLOTS,), dev, init=torch.zeros(AMAX_SLOTS))  # (the caller zeroes the slots)
    L.check(lib.fh_absmax_f32(x.data_ptr(), x.numel(), slots.ptr(), L.stream()), "absmax")
    what = ("absmax", x.numel())
    return (slots.check_tail(what) if nan_expected else slots.check(what)).max()


# 2,621,443: more float4s than the 2048 x 256 threads of the kernel's capped grid, a second trip of its body loop
@pytest.mark.parametrize("n", [1, 3, 5, 1027, 1_048_579, 2_621_443])
def test_absmax_body_and_scalar_tail(dev, n):
    """max over the FH_AMAX_SLOTS slots == x.abs().max() exactly, with the maximum in the last element (the scalar tail: no n
    here is a multiple of 4), negative, and in the float4 body (its last float4, where there is one); a NaN in the tail
    makes the result NaN ("a NaN anywhere wins")."""
    x0 = torch.randn(n, device=dev).clamp_(-4, 4)
    assert n % 4 != 0
    body_last = (n // 4) * 4 - 1 if n >= 4 else 0
    for at, v in ((n - 1, 1000.0), (n - 1, -1000.0), (body_last, 77.0), (body_last, -77.0), (n // 2, -50.0), (None, None)):
        x = x0.clone()
        if at is not None:
            x[at] = v
        got = _absmax(dev, x)
        assert float(got) == float(x.abs().max()) > 0, (n, at, v)
        if at is not None:
            assert float(got) == abs(v)
    x = x0.clone()
    x[n - 1] = float("nan")
    assert bool(torch.isnan(_absmax(dev, x, nan_expected=True))), "a NaN in the tail is lost"
    if n >= 4:
        x = x0.clone()
        x[1] = float("nan")
        assert bool(torch.isnan(_absmax(dev, x, nan_expected=True))), "a NaN in the body is lost"
