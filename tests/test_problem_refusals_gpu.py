"""What fh_amm and fh_cg_solve refuse, per operator code: the smallest valid fh_problem of every op 0 .. 15, then one mutated
field at a time, with the exact return code of both entry points and an output that a refusal must leave untouched.

The expected codes are the library's recorded answers, not what include/fh_hip.h says they ought to be: the table pins the
host dispatch of fh_kernels.hip so that it can be reorganised without moving a refusal.  "A" rows are mutations the library
accepts (a field the op ignores, or a problem that is still well-formed): only rc == 0 is asserted there.

The problems are built directly on _lib.FhProblem; the plugin's operator tables are not involved.  Nothing here provokes a
fault: every case is a host-side refusal or a valid tiny problem, and every buffer is sized for the largest layout any accepted
mutation makes the kernels address (a stride of 1 on the decimating tap list, for instance)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
S, SO, K = 16, 8, 2  # image side, measurement side at stride 2, frames / PSFs of ops 12 .. 14
N = 3 * S * S  # the longest measurement vector of any case below
SENTINEL = -12345.678
SLACK = 8  # doubles behind every vector, so that a pointer 8 bytes off still has N doubles

# one mutation per column, in this order (the rows of EXPECT below)
MUTATIONS = ("mask", "stride", "fold", "tap2_dx", "tap2_w", "ntaps2", "halo", "halo2", "fold_sym", "use_dct", "op16", "op-1")
# R: both entry points return FH_EINVAL and leave out / x untouched;  A: both return 0;  -: not applied
# (op 0 reads its mask as the operator itself and no check looks at it: a null one would not be refused)
EXPECT = {
    0: "- A A A A A A A A A R R",
    1: "A A R A A A R A A A R R",
    2: "A A A A A A R A A A R R",
    3: "A R A A A A A A A A R R",
    4: "A R R R R R R A A A R R",
    5: "R R R A A A R A A A R R",
    6: "R R R R R R R A A A R R",
    7: "R R R A A A A A R A R R",
    8: "R R R A A A R A A A R R",
    9: "R R R R R R R A A A R R",
    10: "R R A A A A R A A A R R",
    11: "R R R A A A A A R A R R",
    12: "R R R R R R R R R A R R",
    13: "R R R R R R R R R A R R",
    14: "R R R R A R R R R R R R",
    15: "R R R R R R R R R R R R",
}
DECIMATING = (2, 7, 10, 11, 12, 13)
TAP_LIST = (1, 2, 5, 8, 10)
WINDOW = (4, 6, 9)
FOLDED = (7, 11, 15)
WITH_MASK = (0, 5, 6, 8, 9, 10, 11, 13, 15)  # the valid problem brings a mask / weights


@pytest.fixture(scope="module")
def bufs():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    b = {
        "ones": torch.ones(N + SLACK, dtype=F64, device=dev),  # D, r, masks, weights, and every "set" pointer
        "zeros": torch.zeros(N + SLACK, dtype=F64, device=dev),  # B, M (no factor columns: never read)
        "dy": torch.tensor([-1, -1, -1, 0, 0, 0, 1, 1, 1] * K, dtype=torch.int32, device=dev),
        "dx": torch.tensor([-1, 0, 1] * 3 * K, dtype=torch.int32, device=dev),
        "w": torch.full((9 * K,), 1.0 / 9.0, dtype=F64, device=dev),
        "off": torch.tensor([0, 9, 18], dtype=torch.int32, device=dev),
        "cw": torch.tensor([0.299, 0.587, 0.114], dtype=F64, device=dev),
        "blend": torch.full((K * N,), 1.0 / K, dtype=F64, device=dev),
        "basis": torch.full((S * S,), 0.05, dtype=F64, device=dev),  # constant: equal to its transpose at any shape
        "u": torch.rand(N + SLACK, generator=g, dtype=F64).to(dev),
        "sentinel": torch.full((N + SLACK,), SENTINEL, dtype=F64, device=dev),
    }
    b["out"] = b["sentinel"].clone()
    return b


def _valid(op, b):
    """the smallest valid fh_problem of `op`: a 3 x 3 PSF, stride 2 where the op decimates, K frames, no factor columns"""
    from free_hunch_amd import _lib
    p = _lib.FhProblem()
    p.op, p.use_dct, p.planes, p.stride = op, 1, 3, 2 if op in DECIMATING else 1
    p.d, p.sigma_y2, p.m, p.ldm = N, 0.01, 0, 64
    p.D, p.r, p.B, p.M = b["ones"].data_ptr(), b["ones"].data_ptr(), b["zeros"].data_ptr(), b["zeros"].data_ptr()
    if op in WITH_MASK:
        p.mask = b["ones"].data_ptr()
    if op in TAP_LIST:
        p.ntaps, p.halo = 9, 1
        p.tap_dy, p.tap_dx, p.tap_w = b["dy"].data_ptr(), b["dx"].data_ptr(), b["w"].data_ptr()
    elif op == 3:
        p.ntaps, p.tap_w = 3, b["cw"].data_ptr()
    elif op in WINDOW:
        p.ntaps, p.halo, p.tap_w = 9, 64 * 1 + 1, b["w"].data_ptr()
    elif op in FOLDED:
        p.fold_fwd_w = p.fold_fwd_h = p.fold_inv_w = p.fold_inv_h = b["basis"].data_ptr()
    elif op in (12, 13, 14):
        p.ntaps, p.halo, p.ntaps2, p.halo2 = 9 * K, 1000 + 64 * 1 + 1, K, 9
        p.tap_dy, p.tap_dx, p.tap_w, p.tap2_dy = b["dy"].data_ptr(), b["dx"].data_ptr(), b["w"].data_ptr(), b["off"].data_ptr()
        if op == 14:
            p.tap2_w = b["blend"].data_ptr()
    return p


def _mutate(p, name, b):
    spare = b["ones"].data_ptr()
    if name == "mask":
        p.mask = None if p.mask else spare
    elif name == "stride":
        p.stride = 3 - p.stride
    elif name == "fold":
        p.fold_fwd_w = None if p.fold_fwd_w else spare
    elif name == "tap2_dx":
        p.tap2_dx = b["dx"].data_ptr()
    elif name == "tap2_w":
        p.tap2_w = b["blend"].data_ptr()
    elif name == "ntaps2":
        p.ntaps2 = -1
    elif name in ("halo", "halo2"):
        setattr(p, name, -200)
    elif name == "fold_sym":
        p.fold_sym = 1
    elif name == "use_dct":
        p.use_dct = 2
    else:
        p.op = {"op16": 16, "op-1": -1}[name]


class _Calls:
    def __init__(self, b):
        from free_hunch_amd import _lib
        self._lib, self.b = _lib, b
        self.ctx = _lib.Context.get(S, 3, 0, slot=977)
        self.lib = self.ctx.lib

    def amm(self, p, u_off=0, out_off=0, out_is_u=False):
        out = self.b["out"].data_ptr() + out_off
        u = out if out_is_u else self.b["u"].data_ptr() + u_off
        return self.lib.fh_amm(self.ctx.h, C.byref(p), u, out, self._lib.stream())

    def solve(self, p, b_off=0, x_off=0):
        info = self._lib.FhCgInfo()
        return self.lib.fh_cg_solve(self.ctx.h, C.byref(p), self.b["u"].data_ptr() + b_off, self.b["out"].data_ptr() + x_off,
                                    1e-3, 0.0, 8, C.byref(info), self._lib.stream())

    def refused(self, call, what):
        """`call` returns FH_EINVAL and leaves the sentinel-filled output as it was, bit for bit"""
        self.b["out"].copy_(self.b["sentinel"])
        rc = call()
        torch.cuda.synchronize()
        print(what, "rc =", rc)
        assert rc == self._lib.FH_EINVAL, (what, rc)
        assert torch.equal(self.b["out"], self.b["sentinel"]), (what, "a refused call wrote to its output")

    def accepted(self, call, what):
        rc = call()
        torch.cuda.synchronize()
        print(what, "rc =", rc)
        assert rc == 0, (what, rc)


def test_table_is_complete():
    assert sorted(EXPECT) == list(range(16))
    for op, row in EXPECT.items():
        cells = row.split()
        assert len(cells) == len(MUTATIONS) and set(cells) <= set("RA-"), op
        assert "R" in cells, (op, "a row without a refusal checks nothing")
        assert cells.count("-") == (1 if op == 0 else 0), op


@pytest.mark.parametrize("op", range(16))
def test_refusals(op, bufs):
    c = _Calls(bufs)
    c.accepted(lambda: c.amm(_valid(op, bufs)), (op, "valid", "fh_amm"))
    c.accepted(lambda: c.solve(_valid(op, bufs)), (op, "valid", "fh_cg_solve"))
    for name, cell in zip(MUTATIONS, EXPECT[op].split()):
        if cell == "-":
            continue
        p = _valid(op, bufs)
        _mutate(p, name, bufs)
        check = c.refused if cell == "R" else c.accepted
        check(lambda: c.amm(p), (op, name, "fh_amm"))
        check(lambda: c.solve(p), (op, name, "fh_cg_solve"))
    if op in (3, 15):  # 16-byte accesses: every operand 8 bytes off is refused, by both entry points
        p = _valid(op, bufs)
        c.refused(lambda: c.amm(p, u_off=8), (op, "u + 8 bytes", "fh_amm"))
        c.refused(lambda: c.amm(p, out_off=8), (op, "out + 8 bytes", "fh_amm"))
        c.refused(lambda: c.solve(p, b_off=8), (op, "b + 8 bytes", "fh_cg_solve"))
        c.refused(lambda: c.solve(p, x_off=8), (op, "x + 8 bytes", "fh_cg_solve"))
    if op == 15:  # the tail butterfly reads u while it writes out
        c.refused(lambda: c.amm(_valid(op, bufs), out_is_u=True), (op, "out == u", "fh_amm"))
