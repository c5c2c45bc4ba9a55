"""The two solve entry points against each other and against the operators' public methods, for every configuration of
test_solver_systems_host.py at 32 x 32 (decimating operators x 2: 16 x 16 measurements): two images with different data - and
different masks or noise maps where the operator has them - solved one by one (`solve_customcuda`) and together
(`solve_customcuda_batched`) take the same iterations and give the same `mat`, and `mat` IS the CG solution pushed through the
operator's public `transpose` (after the weights where the system is whitened), bit for bit.  `solve_all` is also what
profiles/tools/solve_dump.py records."""
import pytest
import torch

from test_solver_systems_host import CONFIGS, make

pytestmark = pytest.mark.gpu
F64 = torch.float64
S = 32
RTOL = 1e-8
SIGMA_T = 80.0  # rtol_func(80, RTOL) = RTOL: the batched solve takes its tolerance from the schedule only


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _randn(shape, seed, dev):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64).to(dev)


def solve_all(config, dev, nimg):
    """`nimg` images of a configuration solved one by one and in one batch: per image the operator, (mat, CG solution u,
    iterations) of the single solve, and the batch's (mat [nimg,3,S,S], iterations)"""
    from free_hunch_amd import conditioning_mechanisms as cm
    from free_hunch_amd.covariance import ScalarCovariance
    rtol = cm.rtol_func(SIGMA_T, RTOL)
    ops, covs, ys, xs, singles = [], [], [], [], []
    for i in range(nimg):
        op = make(config, S=S, device=dev, seed=i, sr_factor=2)
        op.ctx_slot = i
        x = _randn((1, 3, S, S), 500 + i, dev)
        y = op.forward(x, noiseless=True).to(F64)
        ys.append(y + 0.05 * _randn(tuple(y.shape), 600 + i, dev))
        xs.append(0.3 * x)
        ops.append(op)
        covs.append(ScalarCovariance(0.5 + 0.25 * i, 3 * S * S, dev, ctx_slot=i))
    for i in range(nimg):
        info = []
        mat = cm.solve_customcuda(ops[i], ys[i], xs[i], covs[i], RTOL, SIGMA_T, info, rtol=rtol)
        singles.append((mat, cm.solve_customcuda.last_solution, info[0]["niter"]))
    infos = []
    mats = cm.solve_customcuda_batched(ops, ys, xs, covs, RTOL, SIGMA_T, infos)
    return ops, singles, (mats, [i["niter"] for i in infos])


@pytest.mark.parametrize("config", list(CONFIGS))
def test_single_and_batched_solves_agree(dev, config):
    from free_hunch_amd import conditioning_mechanisms as cm
    assert cm.rtol_func(SIGMA_T, RTOL) == pytest.approx(RTOL, rel=1e-12)
    ops, singles, (mats, niters) = solve_all(config, dev, 2)
    row_weights = [getattr(op, "weights", None) for op in ops]
    if hasattr(ops[0], "mask") and ops[0].name != "noise":
        assert not torch.equal(ops[0].mask, ops[1].mask) or "border" in config  # each image its own mask or noise map
    assert tuple(mats.shape) == (2, 3, S, S) and mats.dtype == F64
    for i, (op, (mat, u, niter)) in enumerate(zip(ops, singles)):
        assert 0 < niter < 2000 and niters[i] == niter, (config, i, niters, niter)
        err, scale = float((mats[i:i + 1] - mat).abs().max()), max(1.0, float(mat.abs().max()))
        print(f"{config} image {i}: {niter} iterations, |batched - single| = {err:.3e}, max|single| = {scale:.3e}", flush=True)
        assert err <= 1e-12 * scale
        # mat = A^T [W] u through the public adjoint: inpainting and denoising return u itself
        whitened = op.name.startswith("weighted") or op.name == "fourier_sampling"
        back = op.transpose(row_weights[i] * u if whitened else u)
        assert back.dtype == F64 and torch.equal(back, mat), (config, i, float((back - mat).abs().max()))
