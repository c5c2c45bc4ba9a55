"""Host-side check (no GPU) of the predicate that routes a GroupNorm to the one-launch kernels,
fh_groupnorm_small_supported(P, C), and of its agreement with the two entry points it guards."""
import ctypes as C
import re
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    return _lib, _lib.load()


def _const(name):
    with open(os.path.join(ROOT, "free-hunch_amd", "csrc", "fh_unet.hip")) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


def _limits():
    """(L, pixel limit) as the source states them: elements and pixels of one (image, group) slice"""
    return _const("kGnSmallLimit"), _const("kGnSmallMaxPixels")


def test_predicate_takes_no_batch_size():
    """(P, C) only: a two-group run and a one-group run must pick the same kernel per image"""
    _, lib = _lib()
    assert list(lib.fh_groupnorm_small_supported.argtypes) == [C.c_int, C.c_int]


def test_predicate_channel_rules():
    _, lib = _lib()
    assert lib.fh_groupnorm_small_supported(64, 96) == 0  # cg = 3: no whole float4 per group
    assert lib.fh_groupnorm_small_supported(64, 48) == 0  # not 32 groups
    assert lib.fh_groupnorm_small_supported(64, 64) == 0  # cg = 2
    assert lib.fh_groupnorm_small_supported(0, 128) == 0
    for P, Cc in ((64, 512), (64, 1024), (256, 768), (1024, 256)):
        assert lib.fh_groupnorm_small_supported(P, Cc) == 1, (P, Cc)


def test_predicate_limit_is_sharp():
    _, lib = _lib()
    lim, maxpix = _limits()
    for Cc in (128, 256, 384, 512, 768, 1024, 1536, 2048):
        cg = Cc // 32
        # (third limit of include/fh_hip.h, where cg / 4 does not divide the threads: items per thread x pixel lanes)
        pmax = min(lim // cg, maxpix, _const("kGnSmallMaxIpt") * (_const("kGnSmallThreads") // (cg // 4)))
        assert lib.fh_groupnorm_small_supported(pmax, Cc) == 1, (pmax, Cc)
        assert lib.fh_groupnorm_small_supported(pmax + 1, Cc) == 0, (pmax + 1, Cc)


def test_entry_points_refuse_what_the_predicate_refuses():
    """FH_EINVAL from both, before any pointer is touched (all pointers null here), wherever the predicate is 0"""
    L, lib = _lib()
    lim, maxpix = _limits()
    for P, Cc in ((64, 96), (64, 48), (maxpix + 1, 128), (lim // 64 + 1, 2048), (4096, 512), (0, 128)):
        assert lib.fh_groupnorm_small_supported(P, Cc) == 0
        assert lib.fh_groupnorm_fwd_small(None, None, None, None, None, 0, None, None, 1, P, Cc, 1, None) == L.FH_EINVAL
        assert lib.fh_groupnorm_bwd_small(None, None, None, None, None, None, None, None, 0, None, None, None, None, 0, 1, P,
                                          Cc, 1, None) == L.FH_EINVAL
    # ... and null operands are refused where the predicate is 1
    assert lib.fh_groupnorm_small_supported(64, 512) == 1
    assert lib.fh_groupnorm_fwd_small(None, None, None, None, None, 0, None, None, 1, 64, 512, 1, None) == L.FH_EINVAL
    assert lib.fh_groupnorm_bwd_small(None, None, None, None, None, None, None, None, 0, None, None, None, None, 0, 1, 64,
                                      512, 1, None) == L.FH_EINVAL
