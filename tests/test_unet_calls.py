"""Host-side record of the UNet dispatch (no GPU): the forward pass and input-VJP of five small configurations are run on
CPU tensors against a recording stand-in for the library, and every call - entry point, integer / float arguments, which
pointers coincide, the byte size of every buffer the dispatch allocated, the fields of the epilogue struct, the host
queries and their order - must equal tests/golden/unet_calls.json, which tests/golden/make_unet_calls.py wrote from the
dispatch as it stood before its convolution and GroupNorm routes were folded into one path each."""
import json
import os

import pytest

import make_unet_calls as muc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = """fh_conv2d_nhwc fh_conv2d_x6_nhwc_gn fh_conv2d_x6_norm_nhwc_gn fh_conv3x3_thin_nhwc fh_conv3x3_wino_nhwc
    fh_groupnorm_stats fh_groupnorm_apply fh_groupnorm_finalize fh_groupnorm_table fh_groupnorm_bwd_table
    fh_groupnorm_bwd_sums fh_groupnorm_bwd_apply_ex fh_groupnorm_fwd_small fh_groupnorm_bwd_small fh_absmax_f32
    fh_attention_fwd fh_attention_bwd fh_bgemm_f32 fh_softmax_rows fh_softmax_bwd_rows fh_resample2x fh_concat_channels
    fh_add_f32 fh_layout_nchw_nhwc""".split()


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "unet_calls.json")) as f:
        doc = json.load(f)
    assert "commit" in doc["about"]
    assert {k: (tuple(tuple(x) if isinstance(x, list) else x for x in v["config"]), v["N"], v["dtype"], v["CONV_MODE"])
            for k, v in doc["configs"].items()} == muc.TRACES
    return muc.unpack(doc)


def test_fixture_covers_every_route(fixture):
    queries, traces = fixture
    assert set(traces) == {"A", "A4", "B", "Aw", "Af"}
    launched = {row[0] for calls in traces.values() for row in calls}
    assert not [e for e in ENTRY_POINTS if e not in launched]
    splitk = {r for (n, _a), r in queries.items() if n == "fh_conv2d_splitk"}
    assert 1 in splitk and max(splitk) > 1
    chunks = {r for (n, _a), r in queries.items() if n == "fh_conv2d_x6_gn_chunks"}
    assert 0 in chunks and max(chunks) > 0
    # GroupNorm backward, both entry points: x dy stats sums gamma beta scale shift ss | acc_src add2 dx dx2 csplit ... (amax2)
    bwd = [(t, row[1:]) for t, calls in traces.items() for row in calls
           if row[0] in ("fh_groupnorm_bwd_apply_ex", "fh_groupnorm_bwd_small")]
    assert any(a[12] is not None for _t, a in bwd), "split (dx2)"
    assert any(a[10] is not None for _t, a in bwd), "add2"
    assert any(a[9] is not None and a[11].split(":")[0] == "p9" for _t, a in bwd), "acc_src is dx"
    assert any(len(a) == 20 and a[18] is not None for t, a in bwd if t == "A4"), "amax2"


def test_dispatch_reproduces_the_recorded_calls(fixture, monkeypatch):
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib, unet, unet_hip
    want_q, want = fixture
    got_q, got = muc.record(unet, unet_hip, _lib, monkeypatch.setattr)
    got_q, got = muc.unpack(json.loads(json.dumps(muc.pack(got_q, got, ""))))  # (tuples -> lists, as the fixture went)
    assert got_q == want_q
    for name in want:
        for i, (a, b) in enumerate(zip(got[name], want[name])):
            assert a == b, (name, i, a, b)
        assert len(got[name]) == len(want[name]), name
