"""The UNet's attention per entry point: the three-kernel path (fh_bgemm_f32 + fh_softmax_rows / fh_softmax_bwd_rows) as
HipOps._attn_core_fwd / _attn_core_bwd launch it, fh_bgemm_f32 on windows of larger buffers, the two softmax kernels on their
own, and the fused kernels at inputs where the online softmax has to rescale by many orders of magnitude.

The three-kernel path is the path of every head width other than 32 and 64 (fh_attention_supported) and of FH_ATTN_FUSED=0.
Its operands are slices of the interleaved [N][T][3C] qkv buffer (leading dimension 3C > K, two stride levels: image, head)
and its backward GEMMs write INTO slices of dqkv, so a store outside its slice would be overwritten by the next GEMM and
never seen at network level.

Reference everywhere: `_attention_float64` (tests/test_hip_unet.py) and torch.autograd.grad in float64 on the CPU.  Every
output handed to the library is a `Guarded32`: NaN before the call, 4096 sentinel floats behind it in the same allocation that
must be unchanged after it, no NaN left where the entry point promises to write and - for strided outputs - nothing but NaN
outside that window.  Measured errors: profiles/attention_paths.md."""
import math
import types

import numpy as np
import pytest
import torch

from test_hip_unet import _attention_float64

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TAIL = 4096
SENTINEL = -7.25e30
U = 2.0 ** -24  # unit roundoff of float32
BAR = 5e-6      # the project's bound for fp32 attention against float64 (test_fused_attention_vs_float64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _lib():
    from free_hunch_amd import _lib as L
    return L, L.load()


class Guarded32:
    """A float32 output buffer of `shape` filled with NaN, with TAIL sentinel floats behind it in the same allocation."""

    def __init__(self, shape, dev, init=None):
        n = int(np.prod(shape))
        self.full = torch.full((n + TAIL,), float("nan"), dtype=F32, device=dev)
        self.full[n:] = SENTINEL
        self.out = self.full[:n].view(*shape)
        if init is not None:
            self.out.copy_(init)

    def ptr(self):
        return self.out.data_ptr()

    def check_tail(self, what):
        torch.cuda.synchronize()
        assert bool((self.full[-TAIL:] == SENTINEL).all()), (what, "wrote past the end of its output")
        return self.out

    def check(self, what, window=None):
        """`window` (bool, the buffer's shape): the elements the call promised to write; None = all of them"""
        self.check_tail(what)
        nan = torch.isnan(self.out)
        if window is None:
            assert not bool(nan.any()), (what, "left outputs unwritten")
        else:
            assert not bool((nan & window).any()), (what, "left outputs unwritten")
            assert bool((nan | window).all()), (what, "wrote outside its window")
        return self.out


class _GuardedAllocs:
    """The name `torch` inside unet_hip for the duration of a test: every tensor the dispatch allocates is a Guarded32."""

    def __init__(self):
        self.made = []

    def empty(self, *shape, dtype=F32, device=None):
        assert dtype == F32
        self.made.append(Guarded32(shape, device))
        return self.made[-1].out

    def empty_like(self, t):
        return self.empty(*t.shape, dtype=t.dtype, device=t.device)

    def __getattr__(self, name):
        return getattr(torch, name)

    def check(self, what):
        for i, g in enumerate(self.made):
            g.check((what, "allocation", i, tuple(g.out.shape)))


def err(a, b, scale):
    """max |a - b| relative to max |scale| (the float64 reference), in float64"""
    return float((a.double().cpu() - b.double().cpu()).abs().max() / scale.double().abs().max().clamp_min(1e-30))


def _qkv_heads(qkv, heads, new_order):
    """(q, k, v) as [N * heads][T][ch], split as `_attention_float64` splits them"""
    N, T, C3 = qkv.shape
    C = C3 // 3
    ch = C // heads
    if new_order:
        parts = [t.reshape(N, T, heads, ch) for t in qkv.split(C, dim=2)]
    else:
        parts = list(qkv.reshape(N, T, heads, 3 * ch).split(ch, dim=3))
    return [t.permute(0, 2, 1, 3).reshape(N * heads, T, ch) for t in parts]


def _logits(qkv, heads, new_order):
    """q k^T / sqrt(ch) in nats, [N * heads][T][T], and v"""
    q, k, v = _qkv_heads(qkv, heads, new_order)
    return torch.einsum("btc,bsc->bts", q, k) / math.sqrt(q.shape[-1]), v


def _reference(qkv, dout, heads, new_order):
    """float64 on the CPU: (output, d/dqkv of <output, dout>, softmax weights [N * heads][T][T], logits)"""
    q64 = qkv.double().cpu().requires_grad_()
    ref = _attention_float64(q64, heads, new_order)
    (gref,) = torch.autograd.grad((ref * dout.double().cpu()).sum(), q64)
    ref = ref.detach()
    with torch.no_grad():
        z, v = _logits(q64, heads, new_order)
        w = torch.softmax(z, dim=-1)
        N, T, C = ref.shape
        mine = torch.einsum("bts,bsc->btc", w, v).reshape(N, heads, T, C // heads).permute(0, 2, 1, 3).reshape(N, T, C)
        assert float((mine - ref).abs().max()) < 1e-12 * float(ref.abs().max()), "the weights are not the reference's"
    return ref, gref, w, z


def _ops(new_order):
    from free_hunch_amd import unet_hip
    return unet_hip, unet_hip.HipOps(types.SimpleNamespace(use_new_attention_order=bool(new_order)), {})


def _inputs(shape, dev, scale=1.5):
    N, T, C, heads, new_order = shape
    g = torch.Generator().manual_seed(sum(shape) + 3)
    qkv = (torch.randn(N, T, 3 * C, generator=g) * scale).to(dev)
    dout = torch.randn(N, T, C, generator=g).to(dev)
    return qkv, dout


def _run_core(monkeypatch, shape, qkv, dout, fused):
    """forward and backward through the dispatch's own attention core, every allocation guarded -> (A, saved, dqkv)"""
    N, T, C, heads, new_order = shape
    unet_hip, ops = _ops(new_order)
    monkeypatch.setenv("FH_ATTN_FUSED", "1" if fused else "0")
    allocs = _GuardedAllocs()
    monkeypatch.setattr(unet_hip, "torch", allocs)
    A, saved = ops._attn_core_fwd(qkv, N, T, C, heads)
    assert isinstance(saved, tuple) == fused
    dqkv = ops._attn_core_bwd(qkv, saved, dout, N, T, C, heads)
    allocs.check(("attention core", shape, "fused" if fused else "three kernels"))
    assert tuple(A.shape) == (N, T, C) and tuple(dqkv.shape) == (N, T, 3 * C)
    assert any(g.out.data_ptr() == dqkv.data_ptr() for g in allocs.made)
    return A, saved, dqkv


# ---------------------------------------------------------------- a. the three-kernel path against float64
# (N, T, C, heads): head widths 12 (K one partial chunk, no multiple of 8; T = 36 under one 64-row tile), 16 (the width of
# the recorded SMALL_A call; M and N tails at T = 100), 48, 128, and the recorded shape with N > 1 (both stride levels vary)
THREE_KERNEL = [(2, 36, 96, 8), (1, 100, 64, 4), (2, 64, 96, 2), (1, 256, 256, 2), (3, 256, 64, 4)]


@pytest.mark.parametrize("new_order", [0, 1])
@pytest.mark.parametrize("shape", THREE_KERNEL)
def test_three_kernel_attention_vs_float64(dev, monkeypatch, shape, new_order):
    """HipOps._attn_core_fwd / _attn_core_bwd with FH_ATTN_FUSED=0 - six fh_bgemm_f32 launches on slices of qkv / dqkv plus the
    two softmax kernels, with the dispatch's own strides - against float64: output, dqkv and the materialised weights S
    within 5e-6 of scale, the bound test_fused_attention_vs_float64 holds the fused kernels to.  dqkv (like every tensor
    the core allocates) starts as NaN in a guarded buffer: every element is written; a second run gives the same bits."""
    shape = shape + (new_order,)
    N, T, C, heads, _ = shape
    qkv, dout = _inputs(shape, dev)
    ref, gref, w, _z = _reference(qkv, dout, heads, new_order)
    A, S, dqkv = _run_core(monkeypatch, shape, qkv, dout, fused=False)
    e = err(A, ref, ref), err(S, w, w), err(dqkv, gref, gref)
    print(f"three-kernel attention {shape}: out {e[0]:.2e} S {e[1]:.2e} dqkv {e[2]:.2e}", flush=True)
    assert tuple(S.shape) == (N * heads, T, T)
    assert e[0] < BAR and e[1] < BAR and e[2] < BAR
    A2, S2, dqkv2 = _run_core(monkeypatch, shape, qkv, dout, fused=False)
    assert torch.equal(A2, A) and torch.equal(S2, S) and torch.equal(dqkv2, dqkv)


# ---------------------------------------------------------------- b. the two paths agree
@pytest.mark.parametrize("shape", [(2, 64, 64, 2, 0), (1, 256, 128, 2, 1), (3, 96, 128, 4, 1)])
def test_fused_and_three_kernel_attention_agree(dev, monkeypatch, shape):
    """The fused core and the three-kernel core on the same qkv and dout: each within 5e-6 of float64, hence within 1e-5 of
    each other (the sum of the two bars: derived, not measured)."""
    N, T, C, heads, new_order = shape
    assert _lib()[1].fh_attention_supported(T, C, heads) == 1
    qkv, dout = _inputs(shape, dev)
    ref, gref, _w, _z = _reference(qkv, dout, heads, new_order)
    Af, _, df = _run_core(monkeypatch, shape, qkv, dout, fused=True)
    At, _, dt = _run_core(monkeypatch, shape, qkv, dout, fused=False)
    e = err(Af, ref, ref), err(df, gref, gref), err(At, ref, ref), err(dt, gref, gref), err(Af, At, ref), err(df, dt, gref)
    print(f"attention paths {shape}: fused out {e[0]:.2e} dqkv {e[1]:.2e}; three-kernel out {e[2]:.2e} dqkv {e[3]:.2e}; "
          f"between them out {e[4]:.2e} dqkv {e[5]:.2e}", flush=True)
    assert max(e[:4]) < BAR
    assert e[4] < 2 * BAR and e[5] < 2 * BAR


# ---------------------------------------------------------------- c. fh_bgemm_f32 with gaps and two stride levels
class _Window:
    """`batch` matrices [rows][cols] inside a larger NaN buffer: leading dimension cols + pad, second-level stride s1 between
    the `inner` matrices of a group, first-level stride s0 between groups, all different; nothing but the windows is finite."""

    def __init__(self, rows, cols, pad, batch, inner, dev, values=None):
        self.ld = cols + pad
        self.s1 = rows * self.ld + 7
        self.s0 = inner * self.s1 + 13
        self.off = 5
        b = torch.arange(batch)
        start = self.off + (b // inner) * self.s0 + (b % inner) * self.s1
        self.idx = (start[:, None, None] + torch.arange(rows)[None, :, None] * self.ld + torch.arange(cols)[None, None, :]).to(dev)
        n = int(self.idx.max()) + 1 + 11
        self.buf = Guarded32((n,), dev)
        self.inside = torch.zeros(n, dtype=torch.bool, device=dev)
        self.inside[self.idx.flatten()] = True
        assert int(self.inside.sum()) == self.idx.numel(), "windows overlap"
        if values is not None:
            self.buf.out[self.idx.flatten()] = values.flatten().to(dev)

    def ptr(self):
        return self.buf.ptr() + 4 * self.off

    def read(self):
        return self.buf.out[self.idx]


@pytest.mark.parametrize("mnk", [(36, 36, 12), (65, 1, 33), (1, 65, 31), (100, 70, 50), (256, 16, 256)])
def test_bgemm_windows_and_two_level_strides(dev, mnk):
    """fh_bgemm_f32 as the attention dispatch uses it: batch 6 with inner = 3 and two different strides per operand, every
    operand a window of a larger buffer whose other elements are NaN (leading dimension = extent + 20: a read outside the
    window poisons the result), C a window with ldc = N + 12 of a guarded NaN buffer whose gap columns must stay NaN.
    Bound (the standard dot-product bound, both sides in float64 from the same float32 inputs; a dropped or duplicated term
    exceeds it by orders of magnitude):  |C - ref| <= (K + 2) 2^-24 |alpha| sum_k |a_k| |b_k|  elementwise."""
    L, lib = _lib()
    M, N, K = mnk
    batch, inner, alpha = 6, 3, 0.25
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    A = torch.randn(batch, M, K, generator=g)
    B = torch.randn(batch, N, K, generator=g)
    ref = alpha * torch.bmm(A.double(), B.double().transpose(1, 2))
    bound = (K + 2) * U * abs(alpha) * torch.bmm(A.double().abs(), B.double().abs().transpose(1, 2))
    for ta in (0, 1):
        for tb in (0, 1):
            Am, Bm = (A.transpose(1, 2) if ta else A), (B.transpose(1, 2) if tb else B)
            wa = _Window(Am.shape[1], Am.shape[2], 20, batch, inner, dev, Am)
            wb = _Window(Bm.shape[1], Bm.shape[2], 20, batch, inner, dev, Bm)
            wc = _Window(M, N, 12, batch, inner, dev)
            L.check(lib.fh_bgemm_f32(wa.ptr(), wb.ptr(), wc.ptr(), M, N, K, wa.ld, wb.ld, wc.ld, ta, tb, batch, inner, wa.s0,
                                     wa.s1, wb.s0, wb.s1, wc.s0, wc.s1, alpha, L.stream()), "bgemm")
            wc.buf.check(("bgemm", mnk, ta, tb), window=wc.inside)
            d = (wc.read().double().cpu() - ref).abs()
            worst = float((d / bound).max())
            print(f"bgemm {mnk} transA {ta} transB {tb}: max |C - ref| / bound = {worst:.3f}", flush=True)
            assert bool((d <= bound).all()), (mnk, ta, tb, worst)


# ---------------------------------------------------------------- d. the softmax kernels on their own
def _rows(kind, rows, T, g):
    """the row contents of the softmax tests, float32 [rows][T]"""
    if kind == "randn":
        return 3 * torch.randn(rows, T, generator=g)
    if kind == "constant":  # another constant per row
        return (torch.arange(rows, dtype=F32)[:, None] * 7.5 - 3.25).expand(rows, T).contiguous()
    if kind == "span":  # -80 .. 80 in a shuffled order: the small weights underflow, nothing overflows
        lin = torch.linspace(-80, 80, T) if T > 1 else torch.tensor([80.0])
        return torch.stack([lin[torch.randperm(T, generator=g)] for _ in range(rows)])
    assert kind == "spike"  # one +30 above unit noise; the last row has it in its last element
    x = torch.randn(rows, T, generator=g)
    at = torch.randint(0, T, (rows,), generator=g)
    at[-1] = T - 1
    x[torch.arange(rows), at] += 30
    return x


@pytest.mark.parametrize("kind", ["randn", "constant", "span", "spike"])
@pytest.mark.parametrize("rows,T", [(3, 1), (5, 7), (4, 255), (4, 256), (4, 257), (2, 1000), (2, 4096)])
def test_softmax_rows_forward_and_backward(dev, rows, T, kind):
    """fh_softmax_rows (in place) against torch.softmax in float64: max error 5e-6 (weights are <= 1: the attention bar; the
    kernel's arithmetic gives below 1e-7, printed), row sums within 1e-6 of 1, nothing non-finite, a constant row uniform to
    1 ulp.  fh_softmax_bwd_rows (in place on dp) with p = the float64 softmax rounded to float32 and dp = randn against
    p (dp - sum p dp) in float64: 5e-6 max|dp|.  T = 1 and T < 64: lanes without an element carry -inf into the maximum;
    T = 257: a second trip for one thread only.  Guarded buffers: the row after the last is untouched."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(1000 * rows + T)
    x = _rows(kind, rows, T, g)
    ref = torch.softmax(x.double(), dim=-1)
    s = Guarded32((rows, T), dev, init=x.to(dev))
    L.check(lib.fh_softmax_rows(s.ptr(), rows, T, L.stream()), "softmax")
    p = s.check(("softmax", rows, T, kind)).cpu()
    assert bool(torch.isfinite(p).all())
    e_f = float((p.double() - ref).abs().max())
    e_s = float((p.double().sum(-1) - 1).abs().max())
    assert e_f <= BAR
    assert e_s <= 1e-6
    if kind == "constant":
        assert bool((p == p[:, :1]).all()), "a constant row is not uniform"
        assert abs(float(p[0, 0]) - 1.0 / T) <= float(np.spacing(np.float32(1.0 / T)))
    p32 = ref.float()
    dp = torch.randn(rows, T, generator=g)
    want = p32.double() * (dp.double() - (p32.double() * dp.double()).sum(-1, keepdim=True))
    d = Guarded32((rows, T), dev, init=dp.to(dev))
    L.check(lib.fh_softmax_bwd_rows(p32.to(dev).data_ptr(), d.ptr(), rows, T, L.stream()), "softmax bwd")
    e_b = float((d.check(("softmax bwd", rows, T, kind)).cpu().double() - want).abs().max()) / float(dp.abs().max())
    print(f"softmax rows={rows} T={T} {kind}: forward {e_f:.2e} row sums {e_s:.2e} backward {e_b:.2e}", flush=True)
    assert e_b <= BAR


def test_softmax_rows_refuse_empty_and_null(dev):
    L, lib = _lib()
    s = Guarded32((4, 8), dev, init=torch.zeros(4, 8))
    p = torch.zeros(4, 8, device=dev)
    st = L.stream()
    assert lib.fh_softmax_rows(s.ptr(), 0, 8, st) == L.FH_EINVAL
    assert lib.fh_softmax_rows(s.ptr(), 4, 0, st) == L.FH_EINVAL
    assert lib.fh_softmax_rows(None, 4, 8, st) == L.FH_EINVAL
    assert lib.fh_softmax_bwd_rows(p.data_ptr(), s.ptr(), 0, 8, st) == L.FH_EINVAL
    assert lib.fh_softmax_bwd_rows(p.data_ptr(), s.ptr(), 4, 0, st) == L.FH_EINVAL
    assert lib.fh_softmax_bwd_rows(None, s.ptr(), 4, 8, st) == L.FH_EINVAL
    assert lib.fh_softmax_bwd_rows(p.data_ptr(), None, 4, 8, st) == L.FH_EINVAL
    assert bool((s.check("refused calls") == 0).all())


# ---------------------------------------------------------------- e. the fused kernels at the softmax's hard inputs
def _planted(shape, where, dev):
    """randn qkv with, per head, a unit vector u: 8 u added to every query and key j* replaced by 40 u, so that every row's
    largest logit, by >= 20 nats, sits at j* = the first, a middle or the last key tile"""
    N, T, C, heads, new_order = shape
    ch = C // heads
    j = {"first": 0, "middle": T // 2 + 5, "last": T - 1}[where]
    g = torch.Generator().manual_seed(sum(shape) + j)
    qkv = torch.randn(N, T, 3 * C, generator=g)
    dout = torch.randn(N, T, C, generator=g)
    for h in range(heads):
        u = torch.randn(ch, generator=g)
        u /= u.norm()
        q0, k0 = (h * ch, C + h * ch) if new_order else (3 * h * ch, 3 * h * ch + ch)
        qkv[:, :, q0:q0 + ch] += 8 * u
        qkv[:, j, k0:k0 + ch] = 40 * u
    return qkv.to(dev), dout.to(dev), j  # (float32 from here on: the reference is built from the rounded values)


HARD = [((1, 256, 128, 2, 0), "first"), ((1, 256, 128, 2, 0), "middle"), ((1, 256, 128, 2, 0), "last"),
        ((1, 1024, 64, 2, 1), "first"), ((1, 1024, 64, 2, 1), "middle"), ((1, 1024, 64, 2, 1), "last"),
        ((1, 256, 192, 3, 0), "wide")]
ERR32_FACTOR = 3  # a different summation order and v_exp_f32 against the float32 CPU evaluation


@pytest.mark.parametrize("shape,case", HARD)
def test_fused_attention_at_hard_softmax_inputs(dev, shape, case):
    """fh_attention_fwd / fh_attention_bwd where the online softmax rescales by alpha = exp2(m - mn) over a wide margin: a
    planted key that wins every row by >= 20 nats from the first, a middle or the last key tile (asserted on the float64
    reference), and 4 randn (logit std ~ 16 nats).  Bound for output, dqkv and dsum: max(5e-6, 3 err32) of scale, err32 the
    error of a float32 CPU evaluation of the same reference formula against float64 - at the wide-range input the reference's
    own float32 arithmetic errs by about the plain bar, which would then test rounding luck; at the planted inputs err32 is
    negligible and the bar is the plain 5e-6.  lse = the float64 log-sum-exp in log2 units within 1e-5 max(1, |lse|)."""
    L, lib = _lib()
    N, T, C, heads, new_order = shape
    assert lib.fh_attention_supported(T, C, heads) == 1
    if case == "wide":
        qkv, dout = _inputs(shape, dev, scale=4.0)
    else:
        qkv, dout, j = _planted(shape, case, dev)
    ref, gref, _w, z = _reference(qkv, dout, heads, new_order)
    if case != "wide":
        top = z.topk(2, dim=-1)
        assert bool((top.indices[..., 0] == j).all()), "the planted key does not win every row"
        gap = float((top.values[..., 0] - top.values[..., 1]).min())
        print(f"planted key {j} of {T}: gap {gap:.1f} .. {float((top.values[..., 0] - top.values[..., 1]).max()):.1f} nats, "
              f"largest logit {float(z.max()):.1f}", flush=True)
        assert gap >= 20
    else:
        print(f"wide range: logit std {float(z.std()):.1f} max {float(z.max()):.1f} nats", flush=True)
    dsum_ref = (ref * dout.double().cpu()).reshape(N, T, heads, C // heads).sum(-1).transpose(1, 2).reshape(N * heads, T)
    lse_ref = torch.logsumexp(z, dim=-1) / math.log(2.0)
    # the same formula in float32 on the CPU
    q32 = qkv.cpu().requires_grad_()
    out32 = _attention_float64(q32, heads, new_order)
    (g32,) = torch.autograd.grad((out32 * dout.cpu()).sum(), q32)
    out32 = out32.detach()
    dsum32 = (out32 * dout.cpu()).reshape(N, T, heads, C // heads).sum(-1).transpose(1, 2).reshape(N * heads, T)
    e32 = {"out": err(out32, ref, ref), "dqkv": err(g32, gref, gref), "dsum": err(dsum32, dsum_ref, dsum_ref)}

    out, lse = Guarded32((N, T, C), dev), Guarded32((N * heads, T), dev)
    dsum, dqkv = Guarded32((N * heads, T), dev), Guarded32((N, T, 3 * C), dev)
    st = L.stream()
    L.check(lib.fh_attention_fwd(qkv.data_ptr(), out.ptr(), lse.ptr(), N, T, C, heads, new_order, st), "attn fwd")
    out.check("attention out"), lse.check("attention lse")
    L.check(lib.fh_attention_bwd(qkv.data_ptr(), out.ptr(), dout.data_ptr(), lse.ptr(), dsum.ptr(), dqkv.ptr(), N, T, C,
                                 heads, new_order, st), "attn bwd")
    dsum.check("attention dsum"), dqkv.check("attention dqkv")
    e = {"out": err(out.out, ref, ref), "dqkv": err(dqkv.out, gref, gref), "dsum": err(dsum.out, dsum_ref, dsum_ref)}
    e_lse = float(((lse.out.double().cpu() - lse_ref).abs() / lse_ref.abs().clamp_min(1.0)).max())
    for k in e:
        print(f"fused attention {shape} {case} {k}: err32 {e32[k]:.2e} device {e[k]:.2e} bar {max(BAR, ERR32_FACTOR * e32[k]):.2e}",
              flush=True)
    print(f"fused attention {shape} {case} lse: device {e_lse:.2e} (|lse| up to {float(lse_ref.abs().max()):.1f})", flush=True)
    for k in e:
        assert e[k] <= max(BAR, ERR32_FACTOR * e32[k]), (k, e[k], e32[k])
    assert e_lse <= 1e-5
