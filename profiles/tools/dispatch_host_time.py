"""Host time of the UNet dispatch alone (no GPU): forward + input-VJP of trace A of tests/golden/unet_calls.json on CPU
tensors against a stub library that records nothing, launches nothing and answers the host queries from the fixture's
table - what is left is the Python of free-hunch_amd/unet_hip.py plus the allocator, the per-launch host work the
lock-step sampler is bound by.

    python profiles/tools/dispatch_host_time.py PARENT_CHECKOUT [CHANGE_CHECKOUT] [--passes 20] [--warmup 5]

One worker process per checkout plus a second one of the parent; the workers take turns, one pass each, so drift of the
machine hits all alike.  Prints the median per worker and the parent's spread against itself.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLD = os.path.join(ROOT, "tests", "golden")


class _Stub:
    def __init__(self, answers):
        self._answers = answers

    def __getattr__(self, name):
        table = self._answers.get(name)
        fn = (lambda *a: 0) if table is None else (lambda *a: table[a])
        self.__dict__[name] = fn
        return fn


def worker(root):
    sys.path[:0] = [root, GOLD]
    import torch
    import make_unet_calls as muc
    from free_hunch_amd import _lib, unet, unet_hip
    with open(os.path.join(GOLD, "unet_calls.json")) as f:
        queries = muc.unpack(json.load(f))[0]
    answers = {}
    for (name, args), r in queries.items():
        answers.setdefault(name, {})[args] = r
    stub = _Stub(answers)
    _lib.load, _lib.stream = (lambda: stub), (lambda: None)
    cfg_args, n, dtype, unet_hip.CONV_MODE = muc.TRACES["A"]
    cfg = unet.UNetConfig(*cfg_args)
    model = unet.UNetModel(cfg, dtype=dtype)
    model.load_state_dict(unet.seeded_state(cfg, 0))
    x = torch.zeros(n, cfg.in_channels, cfg.image_size, cfg.image_size, requires_grad=True)
    t = torch.full((n,), 3)
    print("ready", flush=True)
    for _line in sys.stdin:
        t0 = time.perf_counter()
        y = model(x, t)
        torch.autograd.grad(y, x, torch.ones_like(y))
        print(time.perf_counter() - t0, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("change", nargs="?", default=ROOT)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.parent))
    names = ["parent", "change", "parent again"]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", r], stdin=subprocess.PIPE,
                              stdout=subprocess.PIPE, text=True) for r in (a.parent, a.change, a.parent)]
    times = [[] for _ in procs]
    try:
        for p in procs:
            assert p.stdout.readline().strip() == "ready"
        for i in range(a.warmup + a.passes):
            for p, ts in zip(procs, times):
                p.stdin.write("go\n")
                p.stdin.flush()
                s = float(p.stdout.readline())
                if i >= a.warmup:
                    ts.append(s)
    finally:
        for p in procs:
            p.stdin.close()
            p.wait()
    med = [statistics.median(ts) * 1e3 for ts in times]
    for name, m, ts in zip(names, med, times):
        print(f"{name:13s} median {m:8.2f} ms   min {min(ts) * 1e3:8.2f}   max {max(ts) * 1e3:8.2f}   ({len(ts)} passes)")
    print(f"parent against itself: {abs(med[0] - med[2]):.2f} ms;  change - parent: {med[1] - med[0]:+.2f} ms "
          f"({(med[1] / med[0] - 1) * 100:+.2f} %)")


if __name__ == "__main__":
    main()
