"""The one-launch GroupNorm kernels (fh_groupnorm_fwd_small / fh_groupnorm_bwd_small) on the GPU: against float64 torch,
against the three-launch path (partial -> finalize -> stream) on the same inputs, and inside a small UNet whose every
GroupNorm takes them (FH_GN_SMALL on and off against the torch backend, and batch independence bit for bit)."""
import collections
import os
import re

import pytest
import torch
import torch.nn.functional as F

import inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _largest():
    """(P, C) of the largest slice the predicate accepts, from the two limits the source states: the element limit at the
    pixel limit (the test checks that the built predicate agrees)"""
    with open(os.path.join(ROOT, "free-hunch_amd", "csrc", "fh_unet.hip")) as f:
        src = f.read()
    lim = int(re.search(r"constexpr int kGnSmallLimit = (\d+);", src).group(1))
    P = int(re.search(r"constexpr int kGnSmallMaxPixels = (\d+);", src).group(1))
    return P, lim * 32 // P


# (N, P, C): two images at cg = 16; cg = 24 (six float4 per pixel: 85 pixel lanes, two threads idle); odd P, no multiple
# of any lane count; cg = 4 (one float4 per pixel, two pixels per thread); the largest accepted slice (16 per thread)
SHAPES = [(2, 64, 512), (1, 256, 768), (3, 117, 256), (2, 1024, 128), (1, *_largest())]
UNEQUAL = {768: 512}  # csplit of the unequal split (768 = 512 + 256); elsewhere 3 C / 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lib():
    from free_hunch_amd import _lib as L
    return L, L.load()


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def ulps(a, b):
    """largest |a - b| in units of the float32 spacing at max(|a|, |b|)"""
    m = torch.maximum(a.abs(), b.abs())
    spacing = (torch.nextafter(m, torch.full_like(m, float("inf"))) - m).double()
    return float(((a.double() - b.double()).abs() / spacing).max())


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_small_kernels_vs_float64_and_three_launch_path(dev, shape, act, ss):
    L, lib = _lib()
    N, P, C = shape
    assert lib.fh_groupnorm_small_supported(P, C) == 1
    if (P, C) == _largest():
        assert lib.fh_groupnorm_small_supported(P + 1, C) == 0 and lib.fh_groupnorm_small_supported(P, C + 128) == 0
    g = torch.Generator().manual_seed(N * 1000003 + P * 1009 + C + 2 * act + ss)
    x = (torch.randn(N, P, C, generator=g) * 2 + 0.5).to(dev)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
    e = torch.randn(N, 2 * C, generator=g).to(dev)  # scale | shift: the two halves of one [N, 2C] tensor
    dy = torch.randn(N, P, C, generator=g).to(dev)
    acc, add2 = torch.randn(N, P, C, generator=g).to(dev), torch.randn(N, P, C, generator=g).to(dev)
    sc, sh = (e[:, :C], e[:, C:]) if ss else (None, None)
    gp = (gamma.data_ptr(), beta.data_ptr(), _ptr(sc), _ptr(sh), 2 * C)
    st = L.stream()

    # float64 torch
    xd = x.double().permute(0, 2, 1).reshape(N, C, P, 1).requires_grad_()
    t = F.group_norm(xd, 32, gamma.double(), beta.double(), eps=1e-5)
    if ss:
        t = t * (1 + e[:, :C, None, None].double()) + e[:, C:, None, None].double()
    ref = F.silu(t) if act else t
    (gref,) = torch.autograd.grad((ref * dy.double().permute(0, 2, 1).reshape(N, C, P, 1)).sum(), xd)
    ref = ref.detach().reshape(N, C, P).permute(0, 2, 1)
    gref = gref.reshape(N, C, P).permute(0, 2, 1)

    # forward: one launch against stats + apply
    y, stats = torch.empty_like(x), torch.empty(N, 32, 2, device=dev)
    L.check(lib.fh_groupnorm_fwd_small(x.data_ptr(), *gp, y.data_ptr(), stats.data_ptr(), N, P, C, act, st), "fwd_small")
    y3, stats3 = torch.empty_like(x), torch.empty(N, 32, 2, device=dev)
    scratch = torch.empty(lib.fh_groupnorm_scratch_doubles(N, P), dtype=torch.float64, device=dev)
    L.check(lib.fh_groupnorm_stats(x.data_ptr(), stats3.data_ptr(), scratch.data_ptr(), N, P, C, st), "stats")
    L.check(lib.fh_groupnorm_apply(x.data_ptr(), stats3.data_ptr(), *gp, y3.data_ptr(), N, P, C, act, st), "apply")
    print(f"{shape} act={act} ss={ss} fwd: rel64 {rel(y, ref):.2e} stats ulps {ulps(stats, stats3):.2f} rel3 {rel(y, y3):.2e}")
    assert rel(y, ref) < 2e-5
    assert ulps(stats, stats3) <= 1.0
    assert rel(y, y3) < 1e-6

    # backward: both paths read the statistics of the three-launch path, every extra of the tape in turn
    sums3 = torch.empty(N, 32, 2, device=dev)
    L.check(lib.fh_groupnorm_bwd_sums(x.data_ptr(), dy.data_ptr(), stats3.data_ptr(), *gp, sums3.data_ptr(),
                                      scratch.data_ptr(), N, P, C, act, st), "bwd_sums")
    half, uneq = C // 2, UNEQUAL.get(C, 3 * C // 4)
    for what, a_src, a2, csplit in (("plain", None, None, 0), ("in_place", "dx", None, 0), ("acc_src+add2", acc, add2, 0),
                                    ("add2", None, add2, 0), ("split_half", acc, None, half), ("split_unequal", None, add2, uneq)):
        want = gref + (0 if a_src is None else acc.double()) + (0 if a2 is None else add2.double())
        outs = []
        for small in (True, False):
            if csplit:
                dx = torch.full((N, P, csplit), float("nan"), device=dev)
                dx2 = torch.full((N, P, C - csplit), float("nan"), device=dev)
            else:
                dx, dx2 = (acc.clone() if isinstance(a_src, str) else torch.full((N, P, C), float("nan"), device=dev)), None
            src = dx if isinstance(a_src, str) else a_src
            if small:
                sums = torch.empty(N, 32, 2, device=dev)
                L.check(lib.fh_groupnorm_bwd_small(x.data_ptr(), dy.data_ptr(), stats3.data_ptr(), sums.data_ptr(), *gp,
                                                   _ptr(src), _ptr(a2), dx.data_ptr(), _ptr(dx2), csplit, N, P, C, act, st),
                        "bwd_small")
            else:
                L.check(lib.fh_groupnorm_bwd_apply_ex(x.data_ptr(), dy.data_ptr(), stats3.data_ptr(), sums3.data_ptr(), *gp,
                                                      _ptr(src), _ptr(a2), dx.data_ptr(), _ptr(dx2), csplit, N, P, C, act,
                                                      None, st), "bwd_apply_ex")
            outs.append(dx if dx2 is None else torch.cat([dx, dx2], 2))
        r64, u, r3 = rel(outs[0], want), ulps(sums, sums3), rel(outs[0], outs[1])
        print(f"{shape} act={act} ss={ss} bwd {what}: rel64 {r64:.2e} sums ulps {u:.2f} rel3 {r3:.2e}")
        assert r64 < 5e-5, what
        assert u <= 1.0, what
        assert r3 < 1e-6, what
    # the optional sums output may be left out
    dx = torch.empty_like(x)
    L.check(lib.fh_groupnorm_bwd_small(x.data_ptr(), dy.data_ptr(), stats3.data_ptr(), None, *gp, None, None, dx.data_ptr(),
                                       None, 0, N, P, C, act, st), "bwd_small(no sums)")
    assert rel(dx, gref) < 5e-5


# ---- network level: 128 base channels at 32^2, two levels (128 @ 32^2: cg = 4; 256 @ 16^2 with attention: cg = 8), one block
def _nets(dev):
    from free_hunch_amd import unet as hu
    cfg = hu.UNetConfig(image_size=32, num_channels=128, num_res_blocks=1, channel_mult=(1, 2), learn_sigma=True,
                        attention_resolutions="2", num_heads=4, num_head_channels=64, use_scale_shift_norm=True,
                        resblock_updown=True, use_new_attention_order=False)
    sd = hu.seeded_state(cfg, 11)
    nets = []
    for backend in ("hip", "torch"):
        m = hu.UNetModel(cfg, backend=backend)
        m.load_state_dict(sd)
        nets.append(m.to(dev).eval())
    return nets


def _fwd_vjp(m, x, t, cot):
    xi = x.clone().requires_grad_()
    y = m(xi, t)
    (gx,) = torch.autograd.grad((y * cot).sum(), xi)
    return y.detach(), gx


@pytest.fixture
def gn_small_env():
    old = os.environ.get("FH_GN_SMALL")
    yield
    if old is None:
        os.environ.pop("FH_GN_SMALL", None)
    else:
        os.environ["FH_GN_SMALL"] = old


def test_network_with_and_without_the_small_path(dev, gn_small_env):
    hip, ref = _nets(dev)
    x = (inputs.randn((2, 3, 32, 32), 3, torch.float32) * 0.7).to(dev)
    t = torch.tensor([500, 500], device=dev)
    cot = inputs.randn((2, hip.cfg.out_channels, 32, 32), 4, torch.float32).to(dev)
    want = _fwd_vjp(ref, x, t, cot)

    class Counting:
        """the library with a count of the entry points looked up through it (HipOps looks one up per call)"""
        def __init__(self, lib):
            self.lib, self.calls = lib, collections.Counter()

        def __getattr__(self, name):
            self.calls[name] += 1
            return getattr(self.lib, name)

    ops = hip._backend_ops()
    err, calls = {}, {}
    for flag in ("1", "0"):
        os.environ["FH_GN_SMALL"] = flag
        ops.lib = Counting(ops.lib)
        try:
            got = _fwd_vjp(hip, x, t, cot)
        finally:
            calls[flag], ops.lib = ops.lib.calls, ops.lib.lib
        err[flag] = (rel(got[0], want[0]), rel(got[1], want[1]))
    # the switch switches: every GroupNorm of this network is small, so with the path on each one whose producer left no
    # group sums takes one launch - no statistics pass and no sums pass is left - and with it off neither entry point runs.
    # (The two paths usually agree bit for bit - the double sums round to the same float - so the outputs cannot tell.)
    on, off = calls["1"], calls["0"]
    print("GroupNorm calls, small path on:", {k: v for k, v in on.items() if "groupnorm" in k},
          "off:", {k: v for k, v in off.items() if "groupnorm" in k})
    assert on["fh_groupnorm_fwd_small"] > 0 and on["fh_groupnorm_bwd_small"] > 0
    assert on["fh_groupnorm_stats"] == 0 and on["fh_groupnorm_bwd_sums"] == 0
    assert on["fh_groupnorm_fwd_small"] + on["fh_groupnorm_apply"] == off["fh_groupnorm_apply"]
    assert on["fh_groupnorm_bwd_small"] + on["fh_groupnorm_bwd_apply_ex"] == off["fh_groupnorm_bwd_apply_ex"]
    assert off["fh_groupnorm_fwd_small"] == 0 and off["fh_groupnorm_bwd_small"] == 0
    assert off["fh_groupnorm_stats"] == on["fh_groupnorm_fwd_small"] and off["fh_groupnorm_bwd_sums"] == on["fh_groupnorm_bwd_small"]
    print("rel to the torch backend (y, dx): small path", err["1"], "three launches", err["0"])
    for k, bound in ((0, 2e-4), (1, 5e-4)):
        assert err["1"][k] < bound and err["0"][k] < bound
        assert err["1"][k] <= 1.1 * err["0"][k]

    # batch independence, new path on: the kernel choice and the arithmetic do not depend on N
    os.environ["FH_GN_SMALL"] = "1"
    both = _fwd_vjp(hip, x, t, cot)
    for b in range(2):
        one = _fwd_vjp(hip, x[b:b + 1], t[b:b + 1], cot[b:b + 1])
        assert torch.equal(one[0], both[0][b:b + 1]) and torch.equal(one[1], both[1][b:b + 1]), b
