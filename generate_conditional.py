#!/usr/bin/env python3
"""Free Hunch conditional generation on MI355X - the CLI of the reference (generate_conditional.py:434-598):

    python generate_conditional.py --outdir=DIR [--key=value ...]
    torchrun --nproc-per-node 8 generate_conditional.py --outdir=DIR ...

Same flags (free-hunch_amd/config.py), same outputs: DIR/images/{idx:06d}_{seed:06d}.png, cond_images/,
forward_images/, results.txt.  Differences by design: images are sharded i -> rank i mod world with no per-image
barrier, each rank runs `max_batch_size` images in lock-step, outputs are exchanged with one all_gather at the end,
RNG is keyed by (seed, image index).  PSNR, SSIM and LPIPS are computed on the device; LPIPS needs the two published weight
files, which are not shipped: `--lpips_vgg_path=vgg16-397923af.pth --lpips_lin_path=weights/v0.1/vgg.pth` adds the `LPIPS:`
line to results.txt, without them the run reports PSNR and SSIM only.
`--synthetic_weights=ffhq|imagenet` runs with seeded random weights when no checkpoint is present.
`--posterior_samples=K` draws K samples of the SAME measurement per (image, seed): posterior_samples/, posterior_mean/,
posterior_std/ and the calibration lines of results.txt (free-hunch_amd/ensemble.py); images/ keeps member 0."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main(argv=None):
    from free_hunch_amd import ensemble as ens, unet as hu
    from free_hunch_amd.config import load_config
    from free_hunch_amd.pipeline import gather_images, list_images, load_image_u8, lpips_u8, metrics_u8, shard_indices
    from free_hunch_amd.precond import iDDPMLinearPrecond
    from free_hunch_amd.sampler import StandardRGBEncoder

    o = load_config(argv)
    # LPIPS weights are read before anything else happens: a wrong path must not cost a sampling run
    lpips_state = None
    if o.lpips_vgg_path:
        from free_hunch_amd import lpips as fh_lpips
        lpips_state = fh_lpips.load_weights(o.lpips_vgg_path, o.lpips_lin_path)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    from free_hunch_amd.conditioning_mechanisms import choose_conditioning_mechanism
    choose_conditioning_mechanism(o.conditioning_mechanism)  # raises for unknown / unsupported names up front
    if o.iddpm_preconditioning != "linear":
        raise NotImplementedError("cosine preconditioning is incompatible with the plugin API in the reference too")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl")
    os.makedirs(o.outdir, exist_ok=True)

    if o.synthetic_weights:
        cfg = {"ffhq": hu.FFHQ256, "imagenet": hu.IMAGENET256}[o.synthetic_weights]
        model = hu.UNetModel(cfg, backend=o.unet_backend, dtype=o.unet_dtype)
        model.load_state_dict(hu.seeded_state(cfg, 0))
    else:
        model, cfg = hu.load_model(o.openai_state_dict_path, o.openai_setup_path, backend=o.unet_backend,
                                   dtype=None if o.unet_dtype == "fp32" else o.unet_dtype)
    net = iDDPMLinearPrecond(model.to(device).eval(), cfg.image_size, 3).to(device)
    # the metric's network is packed now, not after sampling: a failure here must not cost the run
    lpips_model = None if lpips_state is None else fh_lpips.LPIPS(lpips_state, device)
    S = cfg.image_size

    files = list_images(o.dataset_path)[: o.total_images]
    if not files:
        raise SystemExit(f"no images under {o.dataset_path}")
    total = len(files)
    mine = shard_indices(total, rank, world)
    enc = StandardRGBEncoder()
    data_dir = o.dataset_path if os.path.exists(os.path.join(o.dataset_path, "dct_variance.pt")) else \
        os.path.join(ROOT, "free-hunch_amd", "data")
    if rank == 0 and o.image_base_covariance == "dct_diagonal":
        shipped = "" if data_dir == o.dataset_path else \
            " (shipped ImageNet prior: python -m free_hunch_amd.frequency_analysis --data DIR builds the dataset's own)"
        print(f"dct_variance: {os.path.join(data_dir, 'dct_variance.pt')}{shipped}", flush=True)
    # the dataset's own denoiser-error table when it has one, else the shipped ImageNet table (recon_mse_path=None)
    recon_path = os.path.join(o.dataset_path, "recon_mse.pt")
    recon_path = recon_path if os.path.exists(recon_path) else None
    reads_recon = o.conditioning_mechanism == "peng_analytic" or \
        (o.conditioning_mechanism == "online_covariance" and o.use_analytic_var_at_end)
    if rank == 0 and reads_recon:
        from free_hunch_amd.recon_mse import SHIPPED
        shipped = "" if recon_path else \
            " (shipped ImageNet table: python -m free_hunch_amd.recon_mse --data DIR builds the dataset's own)"
        print(f"recon_mse: {recon_path or SHIPPED}{shipped}", flush=True)
    # every option the reference forwards to its sampler / plugin (generate_conditional.py:121-130, 495)
    kw = dict(conditioning_mechanism=o.conditioning_mechanism, cond_scaling=o.cond_scaling, clip_x0_mean=o.clip_x0_mean,
              pigdm_posthoc_scaling=o.pigdm_posthoc_scaling, max_vector_count=o.max_vector_count, dataset_path=data_dir,
              image_base_covariance=o.image_base_covariance, pca_component_count=o.pca_component_count,
              denoiser_mean_error_threshold=o.denoiser_mean_error_threshold,
              use_analytical_score_time_update=o.use_analytical_score_time_update,
              project_to_diagonal=o.project_to_diagonal, space_step_update_threshold=o.space_step_update_threshold,
              space_step_update_lower_threshold=o.space_step_update_lower_threshold, max_rtol=o.max_rtol,
              do_space_updates=o.do_space_updates, use_analytic_var_at_end=o.use_analytic_var_at_end,
              solver_type=o.solver_type, use_rtol_func=o.use_rtol_func, diffpir_lambda=o.diffpir_lambda,
              recon_mse_path=recon_path)
    loop = dict(num_steps=o.num_steps, sigma_min=o.sigma_min, sigma_max=o.sigma_max, rho=o.rho, solver=o.solver,
                discretization=o.discretization, schedule=o.schedule, scaling=o.scaling)
    churn = dict(S_churn=o.S_churn, S_min=o.S_min, S_max=o.S_max, S_noise=o.S_noise)
    # the lock-step sampler covers the deterministic loop; stochastic churn runs image by image like the reference
    # (ensemble.sample_batch chooses).  one unit = (image, seed): the reference repeats every image once per seed
    # (generate_conditional.py:378-390); with --posterior_samples=K a unit has K adjacent members that share its measurement
    K = o.posterior_samples
    outs, conds, fwds = [], [], []
    units = ens.list_units(mine, o.seeds, K)
    stem = lambda i, sd: f"{i:06d}_{sd:06d}"
    import PIL.Image
    save_rgb = lambda u8, *path: PIL.Image.fromarray(u8.permute(1, 2, 0).cpu().numpy(), "RGB").save(os.path.join(o.outdir, *path))
    if K > 1:
        for sub in ("posterior_samples", "posterior_mean", "posterior_std"):
            os.makedirs(os.path.join(o.outdir, sub), exist_ok=True)
    members, means, calib, carry = [], [], [], None  # the open unit's samples; per finished unit: mean image, calibration sums
    for s in range(0, len(units), max(1, o.max_batch_size)):
        chunk = units[s: s + max(1, o.max_batch_size)]
        ops, ys, noise, imgs, carry = ens.build_batch(o, files, chunk, S, device, carry)
        x = ens.sample_batch(net, ops, ys, noise, churn_seeds=[ens.member_seed(ens.unit_key(i, sd), k) for i, sd, k in chunk],
                             **loop, **churn, **kw)
        first = [b for b, u in enumerate(chunk) if u[2] == 0]  # member 0 is the run without the flag: images/, the metrics
        if first:
            outs.append(enc.decode(x[first]))
            conds.append(torch.stack([imgs[b] for b in first]).to(device))
        if o.operator_name == "fourier_sampling":  # a frequency grid is no picture: the zero-filled reconstruction A0^T y
            fwds += [enc.decode(ops[b].transpose(ys[b])) for b in first]
        else:
            fwds += [enc.decode(ys[b]) for b in first]
        for b, (i, sd, k) in enumerate(chunk) if K > 1 else ():
            # the samples stay on this rank: PNG per member, and the unit's statistics once its last member is in
            save_rgb(enc.decode(x[b]), "posterior_samples", f"{stem(i, sd)}_{k:03d}.png")
            members.append(x[b])
            if k == K - 1:
                st = ens.ensemble_stats(torch.stack(members), imgs[b].to(device))
                members = []
                means.append(st.mean_u8)
                calib.append(torch.stack([st.spread2, st.skill2, st.cover1, st.cover2]))
                save_rgb(st.mean_u8, "posterior_mean", stem(i, sd) + ".png")
                np.save(os.path.join(o.outdir, "posterior_std", stem(i, sd) + ".npy"), st.std.cpu().numpy())
                save_rgb((4.0 * st.std).round().clamp(max=255).to(torch.uint8), "posterior_std", stem(i, sd) + ".png")
        print(f"[rank {rank}] (image, seed) {[u[:2] for u in chunk] if K == 1 else chunk} done", flush=True)
    local_out = torch.cat(outs) if outs else torch.zeros((0, 3, S, S), dtype=torch.uint8, device=device)
    local_cond = torch.cat(conds) if conds else torch.zeros((0, 3, S, S), dtype=torch.uint8, device=device)
    ns = len(o.seeds)
    unit_ids = [i * ns + o.seeds.index(sd) for i, sd, k in units if k == 0]  # global position of (image, seed)
    # metrics as in generate_conditional.py:539-569: per image on the device (fh_metrics_u8); the partial sums travel in the
    # header of the ONE all_gather that collects the images (the reference: a barrier per image + three all_reduces)
    sums = torch.zeros(3 if lpips_state is None else 4, dtype=torch.float64, device=device)
    if local_out.shape[0]:
        ps, ss = metrics_u8(local_out, local_cond)
        parts = [ps.sum(), ss.sum(), torch.tensor(float(local_out.shape[0]), dtype=torch.float64, device=device)]
        if lpips_state is not None:  # fourth header element: the rank-local LPIPS sum
            parts.append(lpips_u8(local_out, local_cond, lpips_model).sum())
        sums = torch.stack(parts)
    nbase = sums.numel()
    if K > 1:
        # the ensembles' sums ride in the same header: the samples themselves do not travel.  Per rank: PSNR and SSIM (and LPIPS)
        # of the mean images, then spread^2, skill^2 and the two covered fractions, each summed over this rank's units
        post = torch.zeros(nbase + 3, dtype=torch.float64, device=device)
        if means:
            mean_imgs = torch.stack(means)
            ps, ss = metrics_u8(mean_imgs, local_cond)
            parts = [ps.sum(), ss.sum()]
            if lpips_state is not None:
                parts.append(lpips_u8(mean_imgs, local_cond, lpips_model).sum())
            post = torch.cat([torch.stack(parts), torch.stack(calib).sum(0)])
        sums = torch.cat([sums, post])
    all_out, sums = gather_images(local_out, unit_ids, total * ns, device, partial_sums=sums)  # the single exchange of the run
    psnr_mean, ssim_mean = float(sums[0] / sums[2]), float(sums[1] / sums[2])
    lpips_line = lpips_print = ""
    if lpips_state is not None:
        lpips_mean = float(sums[3] / sums[2])
        lpips_line, lpips_print = f"LPIPS: {lpips_mean:.4f}\n", f", LPIPS {lpips_mean:.4f}"
    post_lines = ""
    if K > 1:
        pm = [float(v / sums[2]) for v in sums[nbase:]]  # means over the units
        spread2, skill2, cover1, cover2 = pm[-4:]
        ratio = ((1 + 1 / K) * spread2 / skill2) ** 0.5 if skill2 > 0 else float("inf")
        post_lines = (f"posterior_samples: {K}\nPSNR(mean): {pm[0]:.4f}\nSSIM(mean): {pm[1]:.4f}\n"
                      + (f"LPIPS(mean): {pm[2]:.4f}\n" if lpips_state is not None else "")
                      + f"spread: {spread2 ** 0.5:.4f}\nskill: {skill2 ** 0.5:.4f}\nspread/skill: {ratio:.4f}\n"
                      f"coverage(1 sigma): {cover1:.4f}\ncoverage(2 sigma): {cover2:.4f}\n")
    name = lambda u: f"{u // ns:06d}_{o.seeds[u % ns]:06d}.png"
    for sub in ("images", "cond_images", "forward_images"):
        os.makedirs(os.path.join(o.outdir, sub), exist_ok=True)
    if rank == 0:
        for u in range(total * ns):
            PIL.Image.fromarray(all_out[u].permute(1, 2, 0).cpu().numpy(), "RGB").save(
                os.path.join(o.outdir, "images", name(u)))
            if u % ns == 0:  # the ground-truth images are not exchanged: rank 0 reads them from the dataset itself
                PIL.Image.fromarray(load_image_u8(files[u // ns], S).permute(1, 2, 0).numpy(), "RGB").save(
                    os.path.join(o.outdir, "cond_images", name(u)))
        with open(os.path.join(o.outdir, "results.txt"), "w") as f:
            f.write(f"PSNR: {psnr_mean:.4f}\nSSIM: {ssim_mean:.4f}\n{lpips_line}images: {total * ns}\n{post_lines}")
        print(f"PSNR {psnr_mean:.3f} dB, SSIM {ssim_mean:.4f}{lpips_print} over {total * ns} images -> {o.outdir}", flush=True)
        if K > 1:
            print(f"posterior ensembles of {K}: PSNR(mean) {pm[0]:.3f} dB, spread/skill {ratio:.3f}, coverage "
                  f"{cover1:.3f} / {cover2:.3f} at 1 / 2 sigma", flush=True)
    for j, u in enumerate(unit_ids):  # forward (measurement) images are written by the owning rank
        if fwds[j].shape[-1] == S and fwds[j].shape[1] == 1:  # a one-channel measurement (colorization): 8-bit grayscale
            PIL.Image.fromarray(fwds[j][0, 0].cpu().numpy(), "L").save(os.path.join(o.outdir, "forward_images", name(u)))
        elif fwds[j].shape[-1] == S:
            PIL.Image.fromarray(fwds[j][0].permute(1, 2, 0).cpu().numpy(), "RGB").save(
                os.path.join(o.outdir, "forward_images", name(u)))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
