"""GroupNorm passes at the UNet's large shapes: time and effective bandwidth of fh_groupnorm_stats / _apply / _bwd.
`bench_gn.py small`: the one-launch kernels (fh_groupnorm_fwd_small / _bwd_small) against the three launches they replace, at
the small-level shapes of FFHQ-256 and ImageNet-256 and batch 4 / 8 - the table of profiles/gn_small.md that fixes the limit
of fh_groupnorm_small_supported (the pixel limit is opened to 4096 through FH_GN_SMALL_MAX_PIXELS for this run, so that
the 64^2 shapes it excludes are in the table).  Shapes the kernels cannot hold are refused by the library and print as "-"."""
import os, sys, ctypes as C
if len(sys.argv) > 1 and sys.argv[1] == "small":
    os.environ.setdefault("FH_GN_SMALL_MAX_PIXELS", "4096")  # the table also holds the shapes beyond the pixel limit
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT)
import torch
from free_hunch_amd import _lib
lib = _lib.load()
dev = torch.device("cuda:0")

def timed(f, iters=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3

def queued(f, iters=50):
    """GPU time per call of f with the launches queued behind a long kernel, so that the host's launch cost is not in it"""
    blocker = torch.randn(8192, 8192, device=dev)
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    blocker @ blocker
    e0.record()
    for _ in range(iters): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us

def small_table():
    shapes = ((4096, 128), (4096, 256), (1024, 256), (1024, 512), (1024, 768), (1024, 1024), (256, 256), (256, 512), (256, 768),
              (256, 1024), (256, 1536), (256, 2048), (64, 512), (64, 1024), (64, 2048))
    print("| P | C | slice (elements) | N | fwd 3 launches (us) | fwd 1 launch (us) | bwd 3 launches (us) | bwd 1 launch (us) |")
    print("|---|---|---|---|---|---|---|---|")
    st = _lib.stream()
    for (P, Cc) in shapes:
        for N in (4, 8):
            x, dy, add2 = (torch.randn(N, P, Cc, device=dev) for _ in range(3))
            y, dx = torch.empty_like(x), torch.randn(N, P, Cc, device=dev)
            gamma, beta, e = torch.randn(Cc, device=dev), torch.randn(Cc, device=dev), 0.1 * torch.randn(N, 2 * Cc, device=dev)
            gp = (gamma.data_ptr(), beta.data_ptr(), e.data_ptr(), e[:, Cc:].data_ptr(), 2 * Cc)
            stats, sums = torch.empty(N, 32, 2, device=dev), torch.empty(N, 32, 2, device=dev)
            scratch = torch.empty(lib.fh_groupnorm_scratch_doubles(N, P), dtype=torch.float64, device=dev)
            def fwd3():
                lib.fh_groupnorm_stats(x.data_ptr(), stats.data_ptr(), scratch.data_ptr(), N, P, Cc, st)
                lib.fh_groupnorm_apply(x.data_ptr(), stats.data_ptr(), *gp, y.data_ptr(), N, P, Cc, 1, st)
            def bwd3():  # in-place accumulate + a second addend: the heaviest form the tape uses
                lib.fh_groupnorm_bwd_sums(x.data_ptr(), dy.data_ptr(), stats.data_ptr(), *gp, sums.data_ptr(), scratch.data_ptr(), N, P, Cc, 1, st)
                lib.fh_groupnorm_bwd_apply_ex(x.data_ptr(), dy.data_ptr(), stats.data_ptr(), sums.data_ptr(), *gp, dx.data_ptr(), add2.data_ptr(), dx.data_ptr(), None, 0, N, P, Cc, 1, None, st)
            fwd1 = lambda: lib.fh_groupnorm_fwd_small(x.data_ptr(), *gp, y.data_ptr(), stats.data_ptr(), N, P, Cc, 1, st)
            bwd1 = lambda: lib.fh_groupnorm_bwd_small(x.data_ptr(), dy.data_ptr(), stats.data_ptr(), None, *gp, dx.data_ptr(), add2.data_ptr(), dx.data_ptr(), None, 0, N, P, Cc, 1, st)
            ok = fwd1() == 0
            t = [queued(fwd3), queued(fwd1) if ok else None, queued(bwd3), queued(bwd1) if ok else None]
            print(f"| {P} | {Cc} | {P * Cc // 32} | {N} | " + " | ".join("-" if v is None else f"{v:.1f}" for v in t) + " |", flush=True)

if len(sys.argv) > 1 and sys.argv[1] == "small":
    small_table()
    sys.exit(0)

for (N, HW, Cc) in ((8, 256 * 256, 128), (8, 256 * 256, 256), (8, 128 * 128, 256), (8, 64 * 64, 512)):
    x = torch.randn(N, HW, Cc, device=dev)
    dy = torch.randn(N, HW, Cc, device=dev)
    y = torch.empty_like(x); dx = torch.empty_like(x)
    gamma, beta = torch.randn(Cc, device=dev), torch.randn(Cc, device=dev)
    stats = torch.empty(N, 32, 2, device=dev); sums = torch.empty(N, 32, 2, device=dev)
    scratch = torch.empty(lib.fh_groupnorm_scratch_doubles(N, HW), dtype=torch.float64, device=dev)
    st = _lib.stream()
    tb = x.numel() * 4
    t = timed(lambda: lib.fh_groupnorm_stats(x.data_ptr(), stats.data_ptr(), scratch.data_ptr(), N, HW, Cc, st))
    print(f"N={N} P={HW} C={Cc} ({tb/2**20:.0f} MiB): stats {t*1e6:7.1f} us {tb/t/1e12:5.2f} TB/s", end="")
    t = timed(lambda: lib.fh_groupnorm_apply(x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, None, 0, y.data_ptr(), N, HW, Cc, 1, st))
    print(f" | apply {t*1e6:7.1f} us {2*tb/t/1e12:5.2f} TB/s", end="")
    t = timed(lambda: lib.fh_groupnorm_bwd(x.data_ptr(), dy.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, None, 0, sums.data_ptr(), scratch.data_ptr(), dx.data_ptr(), N, HW, Cc, 1, 0, st))
    print(f" | bwd (partial + stream) {t*1e6:7.1f} us {5*tb/t/1e12:5.2f} TB/s")
