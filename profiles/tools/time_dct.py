"""GPU time of one fh_dct2d call (two symmetric passes) at S = 256 by plane count and direction: 200 calls between two events,
queued behind a long kernel so that the host's launch cost is not in the figure; best of 5.  `python profiles/tools/time_dct.py`"""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from free_hunch_amd import _lib
dev = torch.device("cuda:0"); S = 256
ctx = _lib.Context.get(S, 24, 0, slot=9000)
x = torch.randn(24, S, S, dtype=torch.float64, device=dev)
big = torch.randn(8192, 8192, device=dev)
for planes in (4, 8, 12, 15, 24):
    xin = x[:planes].contiguous(); out = torch.empty_like(xin)
    for inv in (False, True):
        for _ in range(20): ctx.dct2d(xin, out, inverse=inv)
        torch.cuda.synchronize()
        best = 1e9
        for rep in range(5):
            big @ big
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200): ctx.dct2d(xin, out, inverse=inv)
            e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3 / 200)
        print("dct2d planes %2d inv %d: %.2f us per 2-pass call" % (planes, inv, best), flush=True)
