"""The GroupNorm-backward entry points that are compositions of the others, on the GPU, bit for bit (float32 tensors
compared with torch.equal): fh_groupnorm_bwd is fh_groupnorm_bwd_sums followed by fh_groupnorm_bwd_apply_ex, and
fh_groupnorm_bwd_apply is fh_groupnorm_bwd_apply_ex with the same operands.  Also: the statistics pass stays within the
scratch that fh_groupnorm_scratch_doubles asks for."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, P, C): 32-pixel chunks with a 6-pixel tail; 24 channel quads (240 of the 256 threads live); 320 channel quads (the
# strided channel loop)
SHAPES = [(2, 70, 32), (3, 1000, 96), (1, 70, 1280)]
GUARD = 64  # doubles: one workgroup's block of partials


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_composed_entry_points_bitwise(shape, act, ss):
    from free_hunch_amd import _lib as L
    lib, dev, st = L.load(), torch.device("cuda:0"), L.stream()
    N, P, C = shape
    g = torch.Generator().manual_seed(N * 1000003 + P * 1009 + C + 2 * act + ss)
    x = (torch.randn(N, P, C, generator=g) * 2 + 0.5).to(dev)
    dy, acc = torch.randn(N, P, C, generator=g).to(dev), torch.randn(N, P, C, generator=g).to(dev)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
    e = torch.randn(N, 2 * C, generator=g).to(dev)  # scale | shift: the two halves of one [N, 2C] tensor
    sc, sh = (e[:, :C], e[:, C:]) if ss else (None, None)
    gp = (gamma.data_ptr(), beta.data_ptr(), _ptr(sc), _ptr(sh), 2 * C)
    xp, dyp = x.data_ptr(), dy.data_ptr()

    # the statistics pass inside exactly the scratch the library asks for, a block of NaNs behind it
    n = lib.fh_groupnorm_scratch_doubles(N, P)
    assert n > 0 and n % 64 == 0
    scratch = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    stats = torch.empty(N, 32, 2, device=dev)
    L.check(lib.fh_groupnorm_stats(xp, stats.data_ptr(), scratch.data_ptr(), N, P, C, st), "stats")
    assert bool(scratch[n:].isnan().all()) and bool(stats.isfinite().all())
    sp = stats.data_ptr()

    def new_dx(accumulate):
        return acc.clone() if accumulate else torch.full((N, P, C), float("nan"), device=dev)

    # the pieces: sums, then the extended apply
    sums = torch.empty(N, 32, 2, device=dev)
    L.check(lib.fh_groupnorm_bwd_sums(xp, dyp, sp, *gp, sums.data_ptr(), scratch.data_ptr(), N, P, C, act, st), "bwd_sums")
    assert bool(scratch[n:].isnan().all())
    pieces = {}
    for accumulate in (0, 1):
        dx = new_dx(accumulate)
        L.check(lib.fh_groupnorm_bwd_apply_ex(xp, dyp, sp, sums.data_ptr(), *gp, dx.data_ptr() if accumulate else None, None,
                                              dx.data_ptr(), None, 0, N, P, C, act, None, st), "bwd_apply_ex")
        assert bool(dx.isfinite().all())
        pieces[accumulate] = dx

    for accumulate in (0, 1):
        # fh_groupnorm_bwd = sums + apply
        dx, sums1 = new_dx(accumulate), torch.empty(N, 32, 2, device=dev)
        L.check(lib.fh_groupnorm_bwd(xp, dyp, sp, *gp, sums1.data_ptr(), scratch.data_ptr(), dx.data_ptr(), N, P, C, act,
                                     accumulate, st), "bwd")
        assert torch.equal(sums1, sums), accumulate
        assert torch.equal(dx, pieces[accumulate]), accumulate
        assert bool(scratch[n:].isnan().all())
        # fh_groupnorm_bwd_apply = the extended apply with the same operands
        dx = new_dx(accumulate)
        L.check(lib.fh_groupnorm_bwd_apply(xp, dyp, sp, sums.data_ptr(), *gp, dx.data_ptr(), N, P, C, act, accumulate, st),
                "bwd_apply")
        assert torch.equal(dx, pieces[accumulate]), accumulate
