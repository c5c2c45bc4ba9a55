"""Host-side check of fh_conv_circ's launch plan (no GPU): fh_conv_circ_plan - status, kernel, grid, block, dynamic LDS
bytes - against tests/golden/conv_circ_plan.json, which tests/golden/make_conv_circ_plan.py recorded from the launch code
as it stood before the dispatch was folded into conv_plan (see the table's "about")."""
import ctypes as C
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESIZE = -1, -2
LDS_LIMIT = {"k_conv_dec": 100 * 1024, "k_conv_up": 100 * 1024}  # the two kernels with an opt-in; every other: 64 KiB


def _lib():
    import __graft_entry__ as g
    g.build()
    from free_hunch_amd import _lib
    return _lib.load()


def _table():
    with open(os.path.join(ROOT, "tests", "golden", "conv_circ_plan.json")) as f:
        t = json.load(f)
    assert t["columns"] == ["S", "stride", "adjoint", "planes", "halo", "ntaps", "status", "kernel", "grid_x", "grid_y",
                            "grid_z", "block", "lds_bytes"]
    assert t["kernels"] == ["k_conv1d<0>", "k_conv1d<1>", "k_conv_tile8", "k_conv_tile", "k_conv_dec", "k_conv_up",
                            "k_conv_direct"]
    return t


def _plan(lib, S, ntaps, halo, planes, stride, adjoint):
    out = (C.c_int32 * 6)()
    rc = lib.fh_conv_circ_plan(S, ntaps, halo, planes, stride, adjoint, out)
    return rc, list(out)


def test_library_reproduces_the_plan_table():
    lib, rows = _lib(), _table()["rows"]
    assert len(rows) >= 900
    for S, stride, adjoint, planes, halo, ntaps, status, *want in rows:
        rc, got = _plan(lib, S, ntaps, halo, planes, stride, adjoint)
        assert (rc, got) == (status, want), ((S, stride, adjoint, planes, halo, ntaps), (rc, got), (status, want))


def test_table_reaches_every_kernel_and_both_errors():
    t = _table()
    ok = [r for r in t["rows"] if r[6] == 0]
    assert {r[7] for r in ok} == set(range(7))
    assert {r[6] for r in t["rows"]} == {0, EINVAL, ESIZE}
    assert all(r[7:] == [0] * 6 for r in t["rows"] if r[6] != 0)
    # the four encodings of the halo code all occur among the accepted rows
    assert any(0 <= r[4] <= 32 for r in ok) and any(-100 <= r[4] < 0 for r in ok)
    assert any(r[4] <= -101 for r in ok) and any(r[4] >= 1000 for r in ok)


def test_accepted_plans_fit_the_lds_their_kernel_runs_under():
    """A condition, not a measurement: 64 KiB of dynamic LDS without an opt-in, 100 KiB for k_conv_dec / k_conv_up -
    on the table and on what the built library answers for the same rows."""
    lib, t = _lib(), _table()
    for S, stride, adjoint, planes, halo, ntaps, status, kernel, _gx, _gy, _gz, block, lds in t["rows"]:
        if status != 0:
            continue
        rc, got = _plan(lib, S, ntaps, halo, planes, stride, adjoint)
        limit = LDS_LIMIT.get(t["kernels"][kernel], 64 * 1024)
        assert block == 256 and 0 <= lds <= limit and rc == 0 and 0 <= got[5] <= limit, (S, stride, adjoint, halo, ntaps, lds)
        assert (lds == 0) == (t["kernels"][kernel] == "k_conv_direct")


def test_gpu_test_shapes_reach_the_kernels_they_name():
    """Which kernel the cases of test_conv_circ_matches_a_direct_sum (tests/test_edge_cases.py) reach, forward / adjoint."""
    import numpy as np
    lib, names = _lib(), _table()["kernels"]
    from free_hunch_amd.measurements import _TapList
    import torch
    for (S, stride, kh, kw, density), want in {
            (64, 1, 9, 5, 0.5): ("k_conv_tile8", "k_conv_tile8"), (96, 1, 31, 7, 0.3): ("k_conv_tile8", "k_conv_tile8"),
            (256, 1, 61, 17, 0.2): ("k_conv_tile8", "k_conv_tile8"), (64, 1, 61, 61, 0.1): ("k_conv_tile", "k_conv_tile"),
            (64, 2, 7, 7, 1.0): ("k_conv_dec", "k_conv_up"), (96, 3, 11, 9, 1.0): ("k_conv_dec", "k_conv_up"),
            (64, 4, 25, 25, 1.0): ("k_conv_dec", "k_conv_up"), (256, 4, 25, 25, 1.0): ("k_conv_dec", "k_conv_up"),
            (48, 4, 25, 25, 1.0): ("k_conv_direct", "k_conv_tile"), (64, 1, 25, 1, 1.0): ("k_conv1d<0>", "k_conv1d<0>"),
            (96, 1, 1, 61, 0.5): ("k_conv1d<1>", "k_conv1d<1>"), (64, 2, 9, 1, 1.0): ("k_conv_direct", "k_conv_tile")}.items():
        halo = _TapList(np.ones((kh, kw)), torch.device("cpu")).halo
        got = []
        for adjoint in (0, 1):
            rc, out = _plan(lib, S, max(2, int(kh * kw * density)), halo, 3, stride, adjoint)  # (about the random sets' sizes)
            assert rc == 0
            got.append(names[out[0]])
        assert tuple(got) == want, ((S, stride, kh, kw, density), got, want)


# the cases test_conv_circ_matches_a_direct_sum adds at sides that are no multiple of 16: (forward, adjoint) kernel
RAGGED = {
    (100, 1, 9, 5, 0.5): ("k_conv_tile8", "k_conv_tile8"), (250, 1, 31, 7, 0.3): ("k_conv_tile8", "k_conv_tile8"),
    (100, 1, 61, 61, 0.1): ("k_conv_tile", "k_conv_tile"), (6, 1, 5, 5, 1.0): ("k_conv_tile8", "k_conv_tile8"),
    (20, 1, 61, 17, 0.2): ("k_conv_tile8", "k_conv_tile8"), (100, 1, 25, 1, 1.0): ("k_conv1d<0>", "k_conv1d<0>"),
    (250, 1, 1, 61, 0.5): ("k_conv1d<1>", "k_conv1d<1>"), (100, 2, 7, 7, 1.0): ("k_conv_direct", "k_conv_tile"),
    (100, 4, 25, 25, 1.0): ("k_conv_direct", "k_conv_tile"), (40, 4, 25, 25, 1.0): ("k_conv_direct", "k_conv_tile"),
    (60, 3, 11, 9, 1.0): ("k_conv_direct", "k_conv_tile"), (20, 1, 61, 1, 1.0): ("k_conv1d<0>", "k_conv1d<0>"),
    (6, 1, 1, 5, 1.0): ("k_conv1d<1>", "k_conv1d<1>"),
}


# the tap lists the operator systems of tests/test_ragged_ops_gpu.py run at ragged sides, as the operators build them:
# (S, taps, halo code, stride) -> (forward, adjoint) kernel.  With a mask or weights (ops 5, 8) conv_launch takes the
# masked variant of the same kernel at stride 1 (k_conv1d_masked, k_conv_tile8_masked) and finishes k_conv_tile and every
# decimating pass (op 10) with k_mask.
RAGGED_OPS = {
    (100, 25, -13, 1): ("k_conv1d<0>", "k_conv1d<0>"), (100, 25, -113, 1): ("k_conv1d<1>", "k_conv1d<1>"),  # shipped Gaussian,
    (250, 25, -13, 1): ("k_conv1d<0>", "k_conv1d<0>"), (250, 25, -113, 1): ("k_conv1d<1>", "k_conv1d<1>"),  # identity prior
    (100, 217, 2864, 1): ("k_conv_tile8", "k_conv_tile8"),   # shipped motion PSF: reach (29, 8)
    (100, 374, 2950, 1): ("k_conv_tile", "k_conv_tile"),     # 61 x 61 sparse PSF: reach (30, 30)
    (100, 49, 1260, 4): ("k_conv_direct", "k_conv_tile"), (36, 49, 1260, 3): ("k_conv_direct", "k_conv_tile"),     # 9 x 9 disk
    (100, 317, 1650, 4): ("k_conv_direct", "k_conv_tile"), (36, 317, 1650, 3): ("k_conv_direct", "k_conv_tile"),   # 21 x 21 disk
    (100, 117, 1262, 4): ("k_conv_direct", "k_conv_tile"), (250, 117, 1262, 2): ("k_conv_direct", "k_conv_tile"),  # 9 x 13 binomial
    (20, 117, 1262, 2): ("k_conv_direct", "k_conv_tile"), (36, 117, 1262, 4): ("k_conv_direct", "k_conv_tile"),    # (identity prior)
    (100, 49, 1390, 4): ("k_conv_direct", "k_conv_tile"), (100, 49, 1195, 4): ("k_conv_direct", "k_conv_tile"),    # burst frames:
    (60, 49, 1325, 3): ("k_conv_direct", "k_conv_tile"), (60, 49, 1195, 3): ("k_conv_direct", "k_conv_tile"),      # K = s^2, K = 1
}
RAGGED_WINDOWS = [(40, 7), (100, 20)]  # (S, reach) of the dense disks: k_conv_window / k_conv_window_masked
RAGGED_RECT = [(20, 10), (36, 9), (40, 10), (100, 25), (100, 20), (250, 125), (250, 25), (36, 12)]  # (S, So) of ops 7 / 11
RAGGED_FRAMES = [(100, 16, 49, 1390, 4), (100, 1, 49, 1195, 4), (60, 9, 49, 1325, 3), (60, 1, 49, 1195, 3)]  # S, K, taps, halo, s


def test_ragged_shapes_reach_the_kernels_they_name():
    """The same for the cases at sides that are no multiple of 16, with the grid each launch gets: whole tiles plus one
    partial tile per direction.  k_conv_dec needs So % 16 == 0 and k_conv_up S % (16 s) == 0, hence S % 16 == 0: no ragged
    side reaches them, and every decimating case here is on k_conv_direct / k_conv_tile with zero insertion."""
    import numpy as np
    lib, names = _lib(), _table()["kernels"]
    from free_hunch_amd.measurements import _TapList
    import torch
    tile = {"k_conv1d<0>": (64, 32), "k_conv1d<1>": (32, 64), "k_conv_tile8": (32, 64), "k_conv_tile": (32, 16)}  # (x, y) outputs
    cases = [((S, max(2, int(kh * kw * density)), _TapList(np.ones((kh, kw)), torch.device("cpu")).halo, stride), want)
             for (S, stride, kh, kw, density), want in RAGGED.items()] + list(RAGGED_OPS.items())
    for which in (cases[:len(RAGGED)], cases[len(RAGGED):]):  # each of the two sets reaches every kernel a ragged side can
        reached = set()
        for (S, ntaps, halo, stride), want in which:
            assert S % 16 != 0
            got = []
            for adjoint in (0, 1):
                rc, out = _plan(lib, S, ntaps, halo, 3, stride, adjoint)
                assert rc == 0, (S, ntaps, halo, stride, adjoint, rc)
                name = names[out[0]]
                got.append(name)
                if name == "k_conv_direct":
                    So = S // stride
                    assert out[1:5] == [-(-3 * So * So // 256), 1, 1, 256] and out[5] == 0
                else:
                    tx, ty = tile[name]
                    assert out[1:5] == [-(-S // tx), -(-S // ty), 3, 256] and 0 < out[5] <= 64 * 1024, (S, ntaps, halo, stride, out)
            assert tuple(got) == want, ((S, ntaps, halo, stride), got, want)
            reached.update(got)
        assert reached == {"k_conv1d<0>", "k_conv1d<1>", "k_conv_tile8", "k_conv_tile", "k_conv_direct"}


def test_no_ragged_side_reaches_the_tiled_sr_pair():
    """k_conv_dec / k_conv_up tile the low-resolution image in blocks of 16: over every even side that is no multiple of 16
    and every stride that divides it, with the 9 x 9 disk of the op 2 / op 10 cases, the plan never names them - their
    system-level GPU cases stay the 64- and 96-pixel ones (test_all_ones_weights_equal_the_unweighted_twin_bitwise,
    test_weighted_sr_amm_vs_oracle), which this test pins to the pair."""
    lib, names = _lib(), _table()["kernels"]
    for S in range(2, 257, 2):
        for stride in (2, 3, 4):
            if S % stride:
                continue
            got = []
            for adjoint in (0, 1):
                rc, out = _plan(lib, S, 49, 1260, 3, stride, adjoint)
                assert rc == 0, (S, stride, adjoint)
                got.append(names[out[0]])
            if S % 16 != 0:
                assert got == ["k_conv_direct", "k_conv_tile"], (S, stride, got)
            elif (S, stride) in ((64, 4), (64, 2), (96, 3)):
                assert got == ["k_conv_dec", "k_conv_up"], (S, stride, got)


def test_ragged_operator_cases_keep_their_window_rect_and_frame_plans():
    """fh_conv_window_plan, fh_dct_rect_plan and fh_conv_frames_plan for the shapes of tests/test_ragged_ops_gpu.py: partial
    tiles in both directions, and burst SR on the chain route (no ragged side is fused) whose launches are the k_conv_direct /
    k_conv_tile plans of RAGGED_OPS."""
    lib = _lib()
    for S, h in RAGGED_WINDOWS:
        out = (C.c_int32 * 5)()
        assert lib.fh_conv_window_plan(S, h, h, 3, out) == 0
        assert list(out)[:4] == [-(-S // 32), -(-S // 64), 3, 256] and 0 < out[4] <= (96 * 129 + 65 * 80) * 8, (S, h, list(out))
        assert S % 32 != 0 and S % 64 != 0
    for S, So in RAGGED_RECT:
        assert S % 16 != 0 and S % So == 0
        for inverse in (0, 1):
            out = (C.c_int32 * 10)()
            assert lib.fh_dct_rect_plan(S, So, 3, inverse, out) == 0
            ko, r_a, r_b = (So, S, So) if inverse else (S, So, S)
            assert out[1] == out[6] == -(-ko // 32) and out[0] == -(-r_a // 32) and out[5] == -(-r_b // 32), (S, So, list(out))
            assert out[3] == out[8] == 256 and 0 < out[4] <= 140 * 1024 and 0 < out[9] <= 140 * 1024
    for S, K, taps, halo, s in RAGGED_FRAMES:
        for adjoint in (0, 1):
            out, one = (C.c_int32 * 6)(), (C.c_int32 * 6)()
            assert lib.fh_conv_frames_plan(S, K, taps, halo, 3, s, adjoint, out) == 0
            assert lib.fh_conv_circ_plan(S, taps, halo, 3, s, adjoint, one) == 0
            assert out[0] == 0 and list(out)[1:4] == list(one)[1:4] and out[5] == one[5], (S, K, adjoint, list(out), list(one))
            assert (S, taps, halo, s) in RAGGED_OPS


def test_plan_query_rejects_what_no_context_or_call_accepts():
    lib = _lib()
    for args in ((0, 9, 4, 3, 1, 0), (63, 9, 4, 3, 1, 0), (258, 9, 4, 3, 1, 0), (64, 0, 4, 3, 1, 0), (64, 9, 4, 0, 1, 0),
                 (64, 9, 4, 3, 0, 0), (64, 9, 33, 3, 1, 0), (64, 9, 999, 3, 1, 0), (64, 9, -134, 3, 1, 0),
                 (64, 9, 1000 + 64 * 33, 3, 1, 0), (64, 9, 1000 + 33, 3, 1, 0)):
        assert _plan(lib, *args) == (EINVAL, [0] * 6), args
    assert lib.fh_conv_circ_plan(64, 9, 4, 3, 1, 0, None) == EINVAL
