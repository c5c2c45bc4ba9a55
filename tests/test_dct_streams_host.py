"""Host-side check of the symmetric DCT pass's launch plan (`fh_dct_sym_plan`, no GPU): the grid stays within the 256 CUs,
two plane streams per workgroup are planned exactly when there are more (plane, tile) tasks than CUs, the streams cover
every plane once with at most 8 planes each, the LDS fits the 160 KiB of a CU, and a one-stream plan is the launch the
kernel had before it learned the second stream (its formula restated here)."""
import ctypes as C

import pytest

SIDES = (128, 256)
PLANES = (1, 3, 4, 8, 9, 12, 13, 15, 24, 48)


def _plan(S, planes):
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    lib = _lib.load()
    gx, gy, gz, ns, lds = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    rc = lib.fh_dct_sym_plan(S, planes, C.byref(gx), C.byref(gy), C.byref(gz), C.byref(ns), C.byref(lds))
    assert rc == 0, rc
    return gx.value, gy.value, gz.value, ns.value, lds.value


@pytest.mark.parametrize("S", SIDES)
@pytest.mark.parametrize("planes", PLANES)
def test_plan(S, planes, monkeypatch):
    monkeypatch.delenv("FH_DCT_STREAMS", raising=False)  # (read once per process: a set switch would show as ns == 1 below)
    gx, gy, gz, ns, lds = _plan(S, planes)
    assert (gx, gy) == (S // 32, S // 64) and gz >= 1
    assert gx * gy * gz <= 256
    assert ns in (1, 2) and (ns == 2) == (planes * gx * gy > 256)
    streams = gz * ns
    seen = []
    for s in range(streams):
        mine = list(range(s, planes, streams))
        assert len(mine) <= 8, (s, mine)
        seen += mine
    assert sorted(seen) == list(range(planes))
    assert lds <= 163840
    if ns == 1:
        want_gz = min(max(256 // (gx * gy), -(-planes // 8), 1), planes)
        assert (gz, lds) == (want_gz, (2 * 32 * (S // 2 + 2) + 2 * 2 * 32 * 66) * 8)


def test_plan_anchor_values():
    """The shapes the bench runs at S = 256: 12 planes (a 4-image group) are 192 workgroups of two one-plane streams, 24 planes
    (the 8-image group) 256 workgroups whose 16 streams carry two planes and one; a single plane keeps one stream."""
    assert _plan(256, 12)[:4] == (8, 4, 6, 2)
    assert _plan(256, 24)[:4] == (8, 4, 8, 2)
    assert _plan(256, 1)[:4] == (8, 4, 1, 1) and _plan(256, 8)[:4] == (8, 4, 8, 1)


def test_plan_rejects_bad_arguments():
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    lib = _lib.load()
    v, w = C.c_int(), C.c_int64()
    assert lib.fh_dct_sym_plan(96, 3, C.byref(v), C.byref(v), C.byref(v), C.byref(v), C.byref(w)) != 0
    assert lib.fh_dct_sym_plan(256, 0, C.byref(v), C.byref(v), C.byref(v), C.byref(v), C.byref(w)) != 0
    assert lib.fh_dct_sym_plan(256, 3, None, C.byref(v), C.byref(v), C.byref(v), C.byref(w)) != 0
