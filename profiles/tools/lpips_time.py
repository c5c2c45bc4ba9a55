"""Time of LPIPS(...)(a, b) for 8 pairs at 256 x 256 (device events around a synchronise, after a warm-up call) and of
the five tap kernels alone against their algorithmic bytes (two float32 reads of the tap tensor).
    python profiles/tools/lpips_time.py [--once]     (--once: one call only, for a rocprofv3 --kernel-trace --stats run)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    import __graft_entry__ as g
    g.build()
    from bench import smooth_images
    from free_hunch_amd import lpips
    dev = torch.device("cuda", 0)
    model = lpips.LPIPS(lpips.seeded_weights(0), dev)
    a = smooth_images(8, 256, 7)
    b = (a.float() + 8 * torch.randn(a.shape, generator=torch.Generator().manual_seed(3))).round().clamp(0, 255).to(torch.uint8)
    a, b = a.to(dev), b.to(dev)
    d = model(a, b)  # warm-up
    torch.cuda.synchronize()
    if "--once" in sys.argv:
        model(a, b)
        torch.cuda.synchronize()
        return
    print(f"LPIPS 8 pairs 256x256: {timed(lambda: model(a, b), 5):.3f} ms per call; d = {d.cpu().tolist()}")
    side = 256
    for t, c in enumerate(lpips.TAP_CHANNELS):
        feat = torch.randn(16, side, side, c, device=dev)
        model.tap(feat, model.lins[t])
        ms = timed(lambda: model.tap(feat, model.lins[t]), 20)
        gb = feat.numel() * 4 / 1e9
        print(f"tap {t}: [16,{side},{side},{c}] {gb * 1e3:.1f} MB in {ms * 1e3:.1f} us = {gb / (ms * 1e-3):.0f} GB/s")
        side //= 2


if __name__ == "__main__":
    main()
