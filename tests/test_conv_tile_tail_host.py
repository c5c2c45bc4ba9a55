"""Host-side check that the 16-byte epilogue of the exact-split 256-pixel convolution tiles leaves the launch plan alone (no
GPU): fh_conv2d_x6_plan, fh_conv2d_x6_gn_chunks and fh_conv2d_x6_norm_supported answer for the 256-pixel rows of
tests/golden/conv_plan.json what the table records, with the switch FH_CONV_TILE_TAIL=0 (read once per process) and without
it - the grid numbers the tiles and the group-sum partials, so it must not depend on the form of the epilogue."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    return _lib.load()


def plan_answers():
    """for every row of the golden table whose launch plans 256-pixel tiles: (row key, plan[0..7], chunks, norm_supported)"""
    lib = _lib()
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan.json")) as f:
        rows = json.load(f)["rows"]
    buf, out = (ctypes.c_int32 * 8)(), []
    for N, H, W, Ci, Co, k, stride, ks, chunks, _chunks1, norm in rows:
        pad = k // 2
        assert lib.fh_conv2d_x6_plan(ks, N, H, W, Ci, Co, k, k, pad, stride, buf) == 0
        if buf[1] != 256:
            continue
        got = (lib.fh_conv2d_x6_gn_chunks(ks, N, H, W, Ci, Co, k, k, pad, stride),
               lib.fh_conv2d_x6_norm_supported(N, H, W, Ci, Co))
        out.append([[N, H, W, Ci, Co, k, stride, ks], list(buf), list(got), [chunks, norm]])
    return out


def test_plan_queries_unchanged_for_256_pixel_rows():
    rows = plan_answers()
    assert len(rows) >= 50
    for (N, H, W, Ci, Co, k, stride, ks), plan, got, want in rows:
        assert got == want, ((N, H, W, Ci, Co), got, want)
        assert (k, stride, ks) == (3, 1, 1)
        # row-reuse family, 256 x 128 tile by LDS-DMA, and the grid that numbers the tiles and the group-sum partials
        assert plan[0] == 1 and plan[2] == 128 and plan[4] == 1 and plan[3] == min(W, 256)
        assert plan[5:] == [N * H * W // 256, -(-Co // 128), 1]
        if got[0]:
            assert got[0] == (H * W // 256) * plan[6]
    assert os.environ.get("FH_CONV_TILE_TAIL") is None, "the switch is read once per process: run the tests without it"
    src = ("import sys, json; sys.path[:0] = [%r, %r]\nimport test_conv_tile_tail_host as t\n"
           "print('RESULT ' + json.dumps(t.plan_answers()))" % (ROOT, os.path.join(ROOT, "tests")))
    off = subprocess.run([sys.executable, "-c", src], check=True, env=dict(os.environ, FH_CONV_TILE_TAIL="0"), timeout=300,
                         stdout=subprocess.PIPE, text=True).stdout
    off = json.loads([ln for ln in off.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert off == rows
