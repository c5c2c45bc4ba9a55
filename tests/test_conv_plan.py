"""Host-side check of the split-bf16 convolution's launch plan (no GPU): the three questions the Python side asks the
library before a launch - split-K factor, number of group-sum block partials, whether the fused GroupNorm input applies -
answered for every layer of the two public architectures (forward and input-gradient, batch 1 ... 16), the shapes
tests/test_hip_unet.py parametrises and the thirteen VGG layers of LPIPS, against tests/golden/conv_plan.json (written by
tests/golden/make_conv_plan.py from the library as it stood before the tile choice was folded into one plan function)."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    return _lib.load()


def _table():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan.json")) as f:
        t = json.load(f)
    assert t["columns"] == ["N", "H", "W", "Cin", "Cout", "k", "stride", "ksplit", "gn_chunks", "gn_chunks_ksplit1",
                            "norm_supported"]
    return t["rows"]


def test_library_reproduces_the_plan_table():
    lib, rows = _lib(), _table()
    assert len(rows) >= 900
    for N, H, W, Ci, Co, k, stride, ks, chunks, chunks1, norm in rows:
        pad = k // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        got = (lib.fh_conv2d_splitk(N, Ho, Wo, Ci, Co, k, k),
               lib.fh_conv2d_x6_gn_chunks(ks, N, H, W, Ci, Co, k, k, pad, stride),
               lib.fh_conv2d_x6_gn_chunks(1, N, H, W, Ci, Co, k, k, pad, stride),
               lib.fh_conv2d_x6_norm_supported(N, H, W, Ci, Co))
        assert got == (ks, chunks, chunks1, norm), ((N, H, W, Ci, Co, k, stride), got, (ks, chunks, chunks1, norm))


def test_plan_table_anchor_values():
    """(N, H = W, C = Cin = Cout, 3 x 3) -> (ksplit, chunks, norm_supported) as measured on the library before the refactor"""
    rows = {tuple(r[:7]): (r[7], r[8], r[10]) for r in _table()}
    for (N, S, C_), want in {(8, 256, 128): (1, 256, 1), (8, 128, 256): (1, 128, 1), (8, 64, 256): (1, 32, 1),
                             (4, 64, 512): (1, 64, 1), (1, 128, 256): (2, 0, 0), (8, 32, 512): (2, 0, 0)}.items():
        assert rows[(N, S, S, C_, C_, 3, 1)] == want, (N, S, C_)


def test_group_sum_chunks_are_whole_tiles_of_one_image():
    """What the epilogue's reader relies on: a positive chunk count is (Ho Wo / bm) x ceil(Cout / 128) for a tile height
    bm in {64, 128, 256} that divides the image - checked on the built library, for both split-K columns of the table."""
    lib, seen = _lib(), set()
    for N, H, W, Ci, Co, k, stride, ks, _c, _c1, _n in _table():
        pad = k // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        for z in {ks, 1}:
            chunks = lib.fh_conv2d_x6_gn_chunks(z, N, H, W, Ci, Co, k, k, pad, stride)
            if chunks <= 0:
                continue
            nb = -(-Co // 128)
            fits = [bm for bm in (64, 128, 256) if (Ho * Wo) % bm == 0 and chunks == (Ho * Wo // bm) * nb]
            assert len(fits) == 1, ((N, H, W, Ci, Co, k, stride, z), chunks, fits)
            assert z == 1 and Co > 64 and Co % 32 == 0
            seen.add(fits[0])
    assert seen == {64, 128, 256}
