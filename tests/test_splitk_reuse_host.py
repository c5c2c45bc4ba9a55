"""Host-side check of the split-K routing of the split-bf16 convolution (no GPU): fh_conv2d_x6_plan, asked for every row of
tests/golden/conv_plan.json, sends a split-K launch to the row-reuse kernel exactly where the predicate of include/fh_hip.h
holds, with tiles that are whole row segments of one image and the grid of the generic launch; FH_CONV_SPLITK_REUSE=0
(read once per process, hence a child process) plans the generic kernel for every split-K launch and changes nothing else."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, REUSE, REUSE_SPLIT = 0, 1, 2


def _rows():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan.json")) as f:
        return json.load(f)["rows"]


def plans(lib, rows):
    """[family, bm, bn, segw, gl, grid x, y, z] per row, at the row's own split-K factor"""
    out = []
    buf = (ctypes.c_int32 * 8)()
    for N, H, W, Ci, Co, k, stride, ks, _c, _c1, _n in rows:
        assert lib.fh_conv2d_x6_plan(ks, N, H, W, Ci, Co, k, k, k // 2, stride, buf) == 0
        out.append(list(buf))
    return out


def _out_pixels(N, H, W, k, stride):
    pad = k // 2
    return N * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1)


def eligible(N, H, W, Ci, Co, k, stride, ks):
    """the predicate: a split-K launch on 128 x 128 tiles (the 64-pixel-tile plans stay generic) of a 3 x 3 / stride 1 /
    pad 1 layer whose 128-pixel tiles are whole row segments of one image"""
    tiles128 = -(-_out_pixels(N, H, W, k, stride) // 128) * -(-Co // 128)
    if not (ks > 1 and Co > 64 and tiles128 * ks >= 256):
        return False
    if not (k == 3 and stride == 1 and (H * W) % 128 == 0):
        return False
    return W % 128 == 0 or (W, H % 2) == (64, 0) or (W, H % 4) == (32, 0) or (W, H % 8) == (16, 0)


_CHILD = r"""
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import __graft_entry__ as g
g.build()
from free_hunch_amd import _lib
import test_splitk_reuse_host as t
json.dump(t.plans(_lib.load(), t._rows()), sys.stdout)
"""


@pytest.fixture(scope="module")
def both():
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    assert os.environ.get("FH_CONV_SPLITK_REUSE") is None, "the switch is read once per process: run the tests without it"
    rows = _rows()
    src = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    off = subprocess.run([sys.executable, "-c", src], check=True, env=dict(os.environ, FH_CONV_SPLITK_REUSE="0"), timeout=300,
                         stdout=subprocess.PIPE).stdout
    return rows, plans(_lib.load(), rows), json.loads(off)


def test_split_launches_take_row_reuse_exactly_where_the_predicate_holds(both):
    rows, on, _off = both
    seen = set()
    assert sum(r[7] > 1 for r in rows) >= 100
    for r, p in zip(rows, on):
        N, H, W, Ci, Co, k, stride, ks = r[:8]
        if ks == 1:
            assert p[0] != REUSE_SPLIT, (r, p)
            continue
        family, bm, bn, segw, gl, gx, gy, gz = p
        assert gz == ks, (r, p)
        assert (family == REUSE_SPLIT) == eligible(N, H, W, Ci, Co, k, stride, ks), (r, p)
        assert family != REUSE, (r, p)
        assert (gx, gy) == (-(-_out_pixels(N, H, W, k, stride) // bm), -(-Co // bn)), (r, p)
        if family == REUSE_SPLIT:
            assert (bm, bn, gl) == (128, 128, 0) and segw in (128, 64, 32, 16), (r, p)
            assert segw * (bm // segw) == bm, (r, p)
            assert (H * W) % bm == 0, (r, p)  # no tile straddles two images
            assert W % segw == 0 and (segw == 128 or segw == W) and H % (bm // segw) == 0, (r, p)  # whole row segments
            seen.add(segw)
        else:
            assert (segw, gl) == (0, 0), (r, p)
    assert seen == {128, 64, 32, 16}, seen


def test_switch_off_plans_the_generic_kernel_and_leaves_the_rest(both):
    rows, on, off = both
    assert len(on) == len(off) == len(rows)
    for r, p, q in zip(rows, on, off):
        if r[7] == 1:
            assert p == q, (r, p, q)
        else:
            assert q[0] == GENERIC and q[3:5] == [0, 0], (r, q)
            assert q[1:3] == p[1:3] and q[5:] == p[5:], (r, p, q)  # same tile, same grid


def test_what_the_python_side_asks_is_unchanged_on_rerouted_layers(both):
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    lib = _lib.load()
    rows, on, _off = both
    n = 0
    for r, p in zip(rows, on):
        if p[0] != REUSE_SPLIT:
            continue
        N, H, W, Ci, Co, k, stride, ks, chunks, _c1, norm = r
        assert lib.fh_conv2d_splitk(N, H, W, Ci, Co, k, k) == ks
        assert chunks == 0 and lib.fh_conv2d_x6_gn_chunks(ks, N, H, W, Ci, Co, k, k, 1, 1) == 0
        assert lib.fh_conv2d_x6_norm_supported(N, H, W, Ci, Co) == norm
        n += 1
    assert n >= 20


def test_query_rejects_bad_arguments():
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int32 * 8)()
    assert lib.fh_conv2d_x6_plan(2, 1, 16, 16, 64, 128, 3, 3, 1, 1, None) == -1
    assert lib.fh_conv2d_x6_plan(0, 1, 16, 16, 64, 128, 3, 3, 1, 1, buf) == -1
    assert lib.fh_conv2d_x6_plan(2, 1, 16, 16, 48, 128, 3, 3, 1, 1, buf) == -1
