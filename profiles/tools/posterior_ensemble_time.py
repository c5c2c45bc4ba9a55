"""Measurements of profiles/posterior_ensemble.md.

    python profiles/tools/posterior_ensemble_time.py kernel          # fh_ensemble_stats at 3 x 256 x 256
    python profiles/tools/posterior_ensemble_time.py sampler [steps] # one ensemble of 8 against 8 independent images

kernel : K = 4, 16, 64 members, N = 1, 8 ensembles, with a truth.  After 20 warm-up calls, 9 windows of CALLS calls each between
         two device events; per window the time of one call, and over the windows median, min and max.  Bytes are what the
         definition needs, counted from the shapes: N n (8 K + 1) in (samples once, truth), 5 N n out (mean_u8, std).
sampler: the batches the CLI runs, through the functions it calls (ensemble.build_batch, ensemble.sample_batch), on one loaded
         network: A = --posterior_samples=8 on one image (one lock-step batch of 8 members, two groups), B = 8 images without the
         flag (sampler.py is the parent commit's, untouched).  One warm-up of each, then A and B alternate REPS times; host clock
         around a batch that ends in a device synchronise."""
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CALLS, WINDOWS, REPS = 200, 9, 5


def kernel():
    from free_hunch_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n = 3 * 256 * 256
    print(f"fh_ensemble_stats, n = {n}: per call over {WINDOWS} windows of {CALLS} calls")
    for K in (4, 16, 64):
        for N in (1, 8):
            g = torch.Generator(device=dev).manual_seed(K * 100 + N)
            x = 1.15 * torch.randn((N, K, n), generator=g, dtype=torch.float64, device=dev)
            truth = torch.randint(0, 256, (N, n), generator=g, dtype=torch.uint8, device=dev)
            mean_u8 = torch.empty((N, n), dtype=torch.uint8, device=dev)
            std = torch.empty((N, n), dtype=torch.float32, device=dev)
            scratch = torch.empty(lib.fh_ensemble_scratch_doubles(N, n), dtype=torch.float64, device=dev)
            out = torch.empty((N, 4), dtype=torch.float64, device=dev)
            st = _lib.stream()

            def call():
                _lib.check(lib.fh_ensemble_stats(x.data_ptr(), truth.data_ptr(), N, K, n, mean_u8.data_ptr(), std.data_ptr(),
                                                 scratch.data_ptr(), out.data_ptr(), st), "fh_ensemble_stats")

            for _ in range(20):
                call()
            torch.cuda.synchronize()
            per_call = []
            for _ in range(WINDOWS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(CALLS):
                    call()
                b.record()
                b.synchronize()
                per_call.append(a.elapsed_time(b) * 1e-3 / CALLS)
            med = statistics.median(per_call)
            nbytes = N * n * (8 * K + 1) + 5 * N * n
            print(f"K = {K:2d}  N = {N}: median {med * 1e6:8.1f} us  (min {min(per_call) * 1e6:.1f}, max {max(per_call) * 1e6:.1f})  "
                  f"{nbytes / 1e6:7.1f} MB  {nbytes / med / 1e9:7.1f} GB/s", flush=True)


def sampler(steps):
    import PIL.Image
    from bench import smooth_images
    from free_hunch_amd import ensemble as ens, unet as hu
    from free_hunch_amd.config import load_config
    from free_hunch_amd.pipeline import list_images
    from free_hunch_amd.precond import iDDPMLinearPrecond
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    tmp = tempfile.mkdtemp()
    for i, im in enumerate(smooth_images(8, 256, 7)):
        PIL.Image.fromarray(im.permute(1, 2, 0).numpy(), "RGB").save(os.path.join(tmp, f"img{i:08d}.png"))
    o = load_config([f"--outdir={tmp}", f"--dataset_path={tmp}", "--synthetic_weights=ffhq", f"--num_steps={steps}",
                     "--max_batch_size=8", "--operator_name=gaussian_blur", "--solver=heun",
                     "--conditioning_mechanism=online_covariance", "--image_base_covariance=dct_diagonal"])
    cfg = hu.FFHQ256
    model = hu.UNetModel(cfg, backend=o.unet_backend, dtype=o.unet_dtype)
    model.load_state_dict(hu.seeded_state(cfg, 0))
    net = iDDPMLinearPrecond(model.to(dev).eval(), cfg.image_size, 3).to(dev)
    files = list_images(tmp)
    # the options generate_conditional.py forwards
    kw = dict(conditioning_mechanism=o.conditioning_mechanism, cond_scaling=o.cond_scaling, clip_x0_mean=o.clip_x0_mean,
              pigdm_posthoc_scaling=o.pigdm_posthoc_scaling, max_vector_count=o.max_vector_count,
              dataset_path=os.path.join(ROOT, "free-hunch_amd", "data"), image_base_covariance=o.image_base_covariance,
              pca_component_count=o.pca_component_count, denoiser_mean_error_threshold=o.denoiser_mean_error_threshold,
              use_analytical_score_time_update=o.use_analytical_score_time_update, project_to_diagonal=o.project_to_diagonal,
              space_step_update_threshold=o.space_step_update_threshold,
              space_step_update_lower_threshold=o.space_step_update_lower_threshold, max_rtol=o.max_rtol,
              do_space_updates=o.do_space_updates, use_analytic_var_at_end=o.use_analytic_var_at_end, solver_type=o.solver_type,
              use_rtol_func=o.use_rtol_func, diffpir_lambda=o.diffpir_lambda, recon_mse_path=None,
              num_steps=o.num_steps, sigma_min=o.sigma_min, sigma_max=o.sigma_max, rho=o.rho, solver=o.solver,
              discretization=o.discretization, schedule=o.schedule, scaling=o.scaling,
              S_churn=o.S_churn, S_min=o.S_min, S_max=o.S_max, S_noise=o.S_noise)
    batches = {"ensemble of 8 (one image)": ens.list_units([0], [0], 8), "8 independent images": ens.list_units(range(8), [0], 1)}

    def run(chunk):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops, ys, noise, imgs, _ = ens.build_batch(o, files, chunk, cfg.image_size, dev)
        t1 = time.perf_counter()
        x = ens.sample_batch(net, ops, ys, noise, **dict(kw))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if chunk[-1][2] > 0:
            ens.ensemble_stats(x, imgs[0].to(dev))
            torch.cuda.synchronize()
        return t1 - t0, t2 - t1, time.perf_counter() - t2

    for chunk in batches.values():
        run(chunk)
    times = {k: [] for k in batches}
    for _ in range(REPS):
        for k, chunk in batches.items():
            times[k].append(run(chunk))
    print(f"gaussian_blur, Heun-{steps}, dct_diagonal, batch 8, two groups; {REPS} alternating repetitions after one warm-up each")
    for k, ts in times.items():
        tot = [sum(t) for t in ts]
        print(f"{k:28s}: {8 / statistics.median(tot):.3f} images/s  (batch median {statistics.median(tot):.3f} s, min {min(tot):.3f}, "
              f"max {max(tot):.3f}; medians: build {statistics.median(t[0] for t in ts):.3f} s, sample "
              f"{statistics.median(t[1] for t in ts):.3f} s, statistics {statistics.median(t[2] for t in ts) * 1e3:.2f} ms)", flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["kernel"]:
        kernel()
    elif sys.argv[1:2] == ["sampler"]:
        sampler(int(sys.argv[2]) if len(sys.argv) > 2 else 30)
    else:
        raise SystemExit(__doc__)
