"""Two plane streams per workgroup in the symmetric DCT pass (`k_dct_sym<.., NS = 2>`, planned by `fh_dct_sym_plan` when a
launch has more (plane, tile) tasks than CUs: from 9 planes on at S = 256, never at S = 128 within a context's plane limit).
Every plane keeps its chain of accumulations, so everything here is bitwise:

* plain passes: each plane of a 9 / 12 / 15 / 24-plane call equals that plane transformed alone (a 1-plane call is the
  one-stream launch); 15 planes leave the two halves of the last workgroup with unequal plane lists, 9 is the smallest
  paired count;
* through the batched CG (epilogue operands, done flags, the p.Ap partials): the solves of this process equal the same
  solves of a child process with FH_DCT_STREAMS=1 (the one-stream launch at every size; read once per process) - iteration
  counts identical, solutions `torch.equal` - at m = 0, at m = 4 after scripted updates, and with one image on a tolerance
  it meets at once while the others run on, so that its planes leave their streams and the halves' trip counts differ;
* the paired launch twice on the same input gives the same bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inputs
from test_timed_path import DATA, _solver_case

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 256
PAIRED = (9, 12, 15, 24)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _ns(planes):
    from free_hunch_amd import _lib
    v = [C.c_int() for _ in range(4)]
    lds = C.c_int64()
    assert _lib.load().fh_dct_sym_plan(S, planes, *[C.byref(x) for x in v], C.byref(lds)) == 0
    return v[3].value


# ---------------------------------------------------------------- plain passes
@pytest.fixture(scope="module")
def planes24(dev):
    """24 seeded planes and, per direction, every plane transformed alone (computed once, never written again)"""
    from free_hunch_amd import _lib
    ctx = _lib.Context.get(S, 24, 0, slot=7100)
    x = inputs.randn((24, S, S), 7101).to(dev)
    alone = {inv: torch.cat([ctx.dct2d(x[p:p + 1].contiguous(), inverse=inv) for p in range(24)]) for inv in (False, True)}
    return ctx, x, alone


@pytest.mark.parametrize("planes", PAIRED)
@pytest.mark.parametrize("inverse", [False, True])
def test_paired_pass_equals_each_plane_alone(planes24, planes, inverse):
    ctx, x, alone = planes24
    assert _ns(1) == 1 and _ns(planes) == 2  # the single-plane call is the one-stream launch, this one the paired launch
    out = ctx.dct2d(x[:planes].contiguous(), inverse=inverse)
    for p in range(planes):
        assert torch.equal(out[p], alone[inverse][p]), (planes, inverse, p)
    assert float(out.abs().max()) > 1.0  # (not a buffer of zeros)


@pytest.mark.parametrize("planes", [12, 15])
def test_paired_pass_is_repeatable(planes24, planes):
    ctx, x, _ = planes24
    for inverse in (False, True):
        xin = x[:planes].contiguous()
        a = ctx.dct2d(xin, inverse=inverse)
        b = ctx.dct2d(xin, inverse=inverse)
        assert torch.equal(a, b), (planes, inverse)


# ---------------------------------------------------------------- through the batched CG
MAXITER = 40
EARLY = 1  # the image whose tolerance is met in the first iterations (planes 3 .. 5: streams of the first halves)


def _covs_m4(nimg, dev):
    """covariance models with 4 factor columns: two scripted time + space updates each (the pattern of the Heun calls)"""
    from free_hunch_amd import covariance as hc
    covs = []
    for b in range(nimg):
        cov = hc.CovarianceHessianBFGSDCT(DATA, 80.0 ** 2, 3 * S * S, device=dev, use_precalculated_info=True, ctx_slot=b)
        for what, a in inputs.script(7200 + b, (1, 3, S, S), 2, 80.0):
            if what == "time":
                cov.update_time_step(a["x"].to(dev), a["sigma"], a["sigma_next"], a["score"].to(dev))
            else:
                cov.update_space_step(a["m0"].to(dev), a["m1"].to(dev), a["sigma"], a["x"].to(dev), a["xn"].to(dev))
        covs.append(cov)
    assert {c.famC.m for c in covs} == {4}
    return covs


def _cg(op, covs, b_vec, rtols, dev):
    """fh_cg_solve_batched as solve_customcuda_batched calls it for a blur, with a tolerance per image and MAXITER"""
    from free_hunch_amd import _lib
    from free_hunch_amd.conditioning_mechanisms import _problem, _sigma_y2
    B = len(covs)
    ctx = _lib.Context.get(S, 3 * B, 0, slot=7300 + B)
    ctx.set_exclusive(True)
    prob, keep = _problem(op, covs[0], _sigma_y2(op))
    per = _lib.FhBatch()
    per.nimg = B
    for b, cov in enumerate(covs):
        per.D[b], per.r[b], per.B[b], per.M[b] = (cov.C.D.data_ptr(), cov.C.r.data_ptr(), cov.famC.B.data_ptr(),
                                                  cov.C.M_dev.data_ptr())
    sol = torch.empty_like(b_vec)
    infos = (_lib.FhCgInfo * B)()
    _lib.check(ctx.lib.fh_cg_solve_batched(ctx.h, C.byref(prob), C.byref(per), b_vec.data_ptr(), sol.data_ptr(),
                                           (C.c_double * B)(*rtols), 0.0, MAXITER, infos, _lib.stream()), "fh_cg_solve_batched")
    torch.cuda.synchronize()
    del keep
    return sol, [i.niter for i in infos]


def solver_cases(dev):
    """{case: (solution, iteration counts)} for 4 and 5 images (12 planes: one plane per stream; 15: uneven halves)"""
    from free_hunch_amd.conditioning_mechanisms import solve_customcuda_batched
    out = {}
    for nimg in (4, 5):
        ops, covs, ys, xs = _solver_case(S, "gaussian_blur", dev, nimg)
        infos = []  # m = 0 through the sampler's entry point: sigma_t = 80 is its loosest tolerance (rtol 1)
        mat = solve_customcuda_batched(ops, ys, xs, covs, 1.0, 80.0, infos, exclusive=True)
        out[f"m0_entry_{nimg}"] = (mat, [i["niter"] for i in infos])
        b_vec = torch.stack([inputs.randn((3 * S * S,), 7400 + b).to(dev) for b in range(nimg)])
        tight = [1e-30] * nimg  # never met: MAXITER iterations
        # (the residual of these cond ~ 1e6 systems first rises: 0.9 |b| is not met in 40 iterations, 1e6 |b| after the first)
        mixed = [1e6 if b == EARLY else 1e-30 for b in range(nimg)]
        out[f"m0_{nimg}"] = _cg(ops[0], covs, b_vec, tight, dev)
        out[f"m0_early_{nimg}"] = _cg(ops[0], covs, b_vec, mixed, dev)
        covs4 = _covs_m4(nimg, dev)
        out[f"m4_{nimg}"] = _cg(ops[0], covs4, b_vec, tight, dev)
        out[f"m4_early_{nimg}"] = _cg(ops[0], covs4, b_vec, mixed, dev)
    return out


_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}, {gold!r}]
import test_dct_streams_gpu as t
assert t._ns(12) == 1  # FH_DCT_STREAMS=1: one stream per workgroup at every size
res = t.solver_cases(torch.device("cuda:0"))
np.savez(sys.argv[1], **{{k: v[0].cpu().numpy() for k, v in res.items()}}, **{{k + "_niter": np.array(v[1]) for k, v in res.items()}})
"""


@pytest.fixture(scope="module")
def both(dev, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("streams") / "one_stream.npz")
    src = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), gold=os.path.join(ROOT, "tests", "golden"))
    subprocess.run([sys.executable, "-c", src, path], check=True, env=dict(os.environ, FH_DCT_STREAMS="1"), timeout=300)
    assert _ns(12) == 2 and _ns(15) == 2
    return solver_cases(dev), np.load(path)


@pytest.mark.parametrize("nimg", [4, 5])
@pytest.mark.parametrize("case", ["m0_entry", "m0", "m4", "m0_early", "m4_early"])
def test_batched_cg_paired_equals_one_stream(both, case, nimg):
    here, ref = both
    key = f"{case}_{nimg}"
    sol, niter = here[key]
    print(key, "iterations", niter, flush=True)
    assert niter == [int(n) for n in ref[key + "_niter"]], (key, niter, list(ref[key + "_niter"]))
    assert torch.equal(sol.cpu(), torch.from_numpy(ref[key])), key
    assert bool(torch.isfinite(sol).all()) and float(sol.abs().max()) > 0
    if case.endswith("early"):  # the early image really left mid-solve, the others ran on
        assert niter[EARLY] < MAXITER and all(n == MAXITER for b, n in enumerate(niter) if b != EARLY), niter
    elif case != "m0_entry":
        assert niter == [MAXITER] * nimg, niter
