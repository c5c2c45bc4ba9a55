"""Dump what the two solve entry points compute, for a bitwise A/B of two checkouts.

    python profiles/tools/solve_dump.py OUT.pt          # in each checkout, one process per run
    python profiles/tools/solve_dump.py --compare A.pt B.pt

For every configuration of tests/test_solver_paths_gpu.py it records the right-hand side b, the CG solution u, mat and the
iteration count of three single solves, and b, u, mat and the iteration counts of one batched solve of the same three images.
b and u never leave the solves, so the tool catches them on the way in: it wraps the two C entry points and reads the
right-hand side and the solution at the pointers they are given (the tensors are found among those `torch.empty_like` saw)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]


def record(out):
    from free_hunch_amd import _lib
    import test_solver_paths_gpu as sp
    lib, seen, calls = _lib.load(), [], []
    empty_like = torch.empty_like

    def watching(t, *a, **k):
        new = empty_like(t, *a, **k)
        seen.extend([t, new])
        return new

    def wrap(name, b_at, sol_at):
        fn = getattr(lib, name)

        def call(*args):
            by_ptr = {t.data_ptr(): t for t in seen}
            b = by_ptr[args[b_at]].clone()
            rc = fn(*args)
            calls.append((b, by_ptr[args[sol_at]]))
            return rc
        setattr(lib, name, call)

    torch.empty_like = watching
    wrap("fh_cg_solve", 2, 3)
    wrap("fh_cg_solve_batched", 3, 4)
    dev, dump = torch.device("cuda:0"), {}
    for config in sp.CONFIGS:
        del seen[:], calls[:]
        _ops, singles, (mats, niters) = sp.solve_all(config, dev, 3)
        assert len(calls) == 4, (config, len(calls))
        for i, (mat, u, niter) in enumerate(singles):
            assert u.data_ptr() == calls[i][1].data_ptr()
            dump[f"{config}/single{i}"] = {"b": calls[i][0].cpu(), "u": u.cpu(), "mat": mat.cpu(), "niter": niter}
        dump[f"{config}/batched"] = {"b": calls[3][0].cpu(), "u": calls[3][1].cpu(), "mat": mats.cpu(), "niter": niters}
        print(f"{config}: iterations {[s[2] for s in singles]} / {niters}", flush=True)
    torch.save(dump, out)
    print(f"wrote {len(dump)} entries to {out}")


def compare(path_a, path_b):
    a, b = torch.load(path_a, weights_only=True), torch.load(path_b, weights_only=True)
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    tensors = scalars = differ = 0
    for key in a:
        for field in ("b", "u", "mat"):
            tensors += 1
            if not torch.equal(a[key][field], b[key][field]):
                differ += 1
                print(f"DIFFERS {key} {field}: max |a - b| = {float((a[key][field] - b[key][field]).abs().max()):.3e}")
        na, nb = a[key]["niter"], b[key]["niter"]
        scalars += len(na) if isinstance(na, list) else 1
        if na != nb:
            differ += 1
            print(f"DIFFERS {key} niter: {na} / {nb}")
    print(f"compared {tensors} tensors and {scalars} iteration counts: {differ} differ")
    return differ


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    record(sys.argv[1])
