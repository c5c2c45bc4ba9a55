"""Writes tests/golden/conv_circ_plan.json: what fh_conv_circ_plan of a built library answers - status, kernel, grid,
block and dynamic LDS bytes - over a sweep of image sizes, strides, directions, plane counts, halo codes and tap counts.
No device is needed.  tests/test_conv_circ_plan.py holds every later build to the committed table.

    python tests/golden/make_conv_circ_plan.py [--lib LIBFH_HIP_SO] [--out FILE]

The sweep is every 37th row of the full product below (37 is coprime to every dimension's size, so each value of each
dimension is met many times); the maker asserts that, and the test asserts that all seven kernels and both error codes
occur in it.
"""
import argparse
import ctypes as C
import itertools
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (32, 48, 64, 96, 128, 256)
EXTENTS = (0, 1, 4, 12, 16, 30, 32, 33)
KERNELS = ["k_conv1d<0>", "k_conv1d<1>", "k_conv_tile8", "k_conv_tile", "k_conv_dec", "k_conv_up", "k_conv_direct"]
COLUMNS = ["S", "stride", "adjoint", "planes", "halo", "ntaps", "status", "kernel", "grid_x", "grid_y", "grid_z", "block",
           "lds_bytes"]
STEP = 37


def strides(S):
    """every stride in 1..4 that divides S, one small stride that does not, and 5"""
    return [s for s in (1, 2, 3, 4) if S % s == 0] + [next(s for s in (3, 7) if S % s)] + [5]


def halo_codes():
    """(halo code, full tap count of the extent) in the four encodings of fh_conv_circ"""
    out = [(h, (2 * h + 1) ** 2) for h in EXTENTS]                                          # h = max(|dy|, |dx|)
    out += [(-(h + 1), 2 * h + 1) for h in EXTENTS]                                         # column list
    out += [(-(h + 101), 2 * h + 1) for h in EXTENTS]                                       # row list
    out += [(1000 + 64 * hy + hx, (2 * hy + 1) * (2 * hx + 1)) for hy in EXTENTS for hx in EXTENTS]  # both extents
    return out


def sweep():
    full = []
    for S in SIZES:
        for stride, adjoint, planes, (halo, ext) in itertools.product(strides(S), (0, 1), (3, 24), halo_codes()):
            full += [(S, stride, adjoint, planes, halo, n) for n in (1, min(ext, 1024), 1025)]
    keys = list(dict.fromkeys(full))[::STEP]  # (extent 0 gives ntaps 1 twice)
    for col, want in ((0, set(SIZES)), (1, {1, 2, 3, 4, 5, 7}), (2, {0, 1}), (3, {3, 24}), (4, {h for h, _ in halo_codes()})):
        assert {k[col] for k in keys} == want, (col, want - {k[col] for k in keys})
    return keys


def rows(lib):
    fn = lib.fh_conv_circ_plan
    fn.argtypes, fn.restype = [C.c_int] * 6 + [C.POINTER(C.c_int32)], C.c_int
    table = []
    for S, stride, adjoint, planes, halo, ntaps in sweep():
        out = (C.c_int32 * 6)()
        rc = fn(S, ntaps, halo, planes, stride, adjoint, out)
        table.append([S, stride, adjoint, planes, halo, ntaps, rc] + list(out))
    return table


HOW = ("status = what fh_conv_circ returns (0, -1 = FH_EINVAL, -2 = FH_ESIZE); kernel = index into `kernels`; error rows "
       "carry zeros.  This table was recorded from the launch code as it stood BEFORE the dispatch was folded into "
       "conv_plan: in a copy of that commit the seven hipLaunchKernelGGL calls of conv_launch were made to write (kernel, "
       "grid, block, LDS bytes) instead of launching, nothing else was changed, and this script was pointed at that build.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "free-hunch_amd", "libfh_hip.so"))
    ap.add_argument("--out", default=os.path.join(HERE, "conv_circ_plan.json"))
    a = ap.parse_args()
    table = rows(C.CDLL(os.path.abspath(a.lib)))
    with open(a.out, "w") as f:
        f.write('{"about": %s,\n "kernels": %s,\n "columns": %s,\n "rows": [\n'
                % (json.dumps(HOW), json.dumps(KERNELS), json.dumps(COLUMNS)))
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in table))
        f.write("\n ]}\n")
    print(f"{len(table)} rows -> {a.out}")


if __name__ == "__main__":
    main()
