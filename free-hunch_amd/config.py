"""Flag system of the CLI (reference: config_utils.py:72-114 + config/config.yaml): `--outdir=DIR` plus any number of
`--key=value` overrides, coerced by the schema below.

Schema and defaults are the reference's `config/config.yaml:1-124`, key for key (so a bare run selects `dps` with the
`identity` base covariance and `max_batch_size=2`, exactly like the reference); keys the Free Hunch path does not read
(`net`, `gnet`, `subdirs`, `class_idx`, `guidance`, `ref_stats_name`, `save_videos`, ...) are accepted and carried
along.  A key outside the schema is kept as the string it was given, as `validate_and_convert` does (config_utils.py:
66-68).  Keys marked NEW are this build's additions."""
from __future__ import annotations

import sys
from types import SimpleNamespace

# name -> (type, default)      types: str / int / float / bool / "ints" (List[int])
SCHEMA = {
    "net": (str, None), "gnet": (str, None), "outdir": (str, None), "subdirs": (bool, False), "seeds": ("ints", [0]),
    "class_idx": (int, None), "total_images": (int, 10), "max_batch_size": (int, 2), "device": (str, "cuda"),
    "num_steps": (int, 50), "sigma_min": (float, 0.002), "sigma_max": (float, 80.0), "rho": (float, 7.0),
    "guidance": (float, None), "S_churn": (float, 0.0), "S_min": (float, 0.0), "S_max": (float, float("inf")),
    "S_noise": (float, 1.0), "solver": (str, "heun"), "discretization": (str, "edm"), "schedule": (str, "linear"),
    "scaling": (str, "none"), "architecture": (str, "openai"),
    "openai_state_dict_path": (str, "models/256x256_diffusion_uncond.pt"),
    "openai_setup_path": (str, "models/256x256_diffusion_uncond_setup.txt"),
    "iddpm_preconditioning": (str, "linear"), "conditional": (bool, True),
    "dataset_name": (str, "training.dataset.ImageFolderDataset"), "dataset": (str, "imagenet"),
    "data_subset": (str, "val"), "dataset_path": (str, "data/imagenet/"), "ref_stats_name": (str, "fid_ref.pkl"),
    "operator_name": (str, "gaussian_blur"), "kernel_size": (int, 61), "intensity": (float, 1.0),
    "noise_name": (str, "gaussian"), "noise_sigma": (float, 0.1), "cond_scaling": (float, 1.0),
    "save_videos": (bool, False), "conditioning_mechanism": (str, "dps"), "clip_x0_mean": (bool, False),
    "pigdm_posthoc_scaling": (bool, False), "max_vector_count": (int, 100000),
    "image_base_covariance": (str, "identity"), "pca_component_count": (int, 10),
    "denoiser_mean_error_threshold": (float, 0.2), "use_analytical_score_time_update": (bool, True),
    "project_to_diagonal": (bool, False), "space_step_update_threshold": (float, 10.0),
    "space_step_update_lower_threshold": (float, 1.0), "scale_factor": (int, 2), "do_space_updates": (bool, True),
    "num_other_images_to_save": (int, 200), "max_rtol": (float, 1.0), "use_analytic_var_at_end": (bool, False),
    "inpainting_type": (str, "random"), "inpainting_prob_lower": (float, 0.1), "inpainting_prob_upper": (float, 0.3),
    "solver_type": (str, "customcuda"), "use_rtol_func": (bool, False), "diffpir_lambda": (float, 10.0),
    "use_ddnm_kernel_params": (bool, False), "save_other_images": (bool, False),
    # NEW: seeded random weights of that architecture when no checkpoint is present ("ffhq" | "imagenet")
    "synthetic_weights": (str, ""),
    # NEW: "hip" (libfh_hip.so kernels) | "torch" (PyTorch-ROCm ops, for A/B runs)
    "unet_backend": (str, "hip"),
    # NEW: "fp32" | "bf16" | "fp16" - reduced-precision UNet torso (the reference's use_fp16 flag lives in the
    # checkpoint's setup file, training/openai_fp16_util.py:15-32); a non-parity speed mode
    "unet_dtype": (str, "fp32"),
    # NEW: the two weight files of LPIPS-VGG (torchvision's vgg16-397923af.pth, lpips' weights/v0.1/vgg.pth); both empty =
    # no LPIPS line in results.txt
    "lpips_vgg_path": (str, ""), "lpips_lin_path": (str, ""),
    # NEW: the PSF of --operator_name=custom_blur, a 2-D .npy (used as given, not normalised; up to 65 x 65); also the PSF of
    # --operator_name=masked_blur and of --operator_name=custom_sr (blur, then every --scale_factor-th sample: 2 .. 16)
    "kernel_path": (str, ""),
    # NEW: the validity mask of --operator_name=masked_blur (y = M (B x + n), the PSF from --kernel_path): a 0/1 .npy of shape
    # [S,S], [3,S,S] or [1,3,S,S], and / or a border of N dropped pixels on every side (-1: the PSF's reach); the two multiply
    "mask_path": (str, ""), "mask_border": (int, 0),
    # NEW: the per-pixel noise level of --operator_name=weighted_blur / weighted_sr (the PSF from --kernel_path, the factor from
    # --scale_factor): either --noise_map_path, a .npy of standard deviations in the [-1, 1] units of the measurement ([n,n],
    # [3,n,n] or [1,3,n,n] at the measurement's side; +inf = pixel not measured), or a Poisson-Gaussian sensor --noise_gain=G
    # --noise_read_sigma=R in intensity units of [0, 1] (measurements.poisson_gaussian_sigma): the run then synthesises the
    # measurement with that noise and hands the solver the map estimated from the measurement
    "noise_map_path": (str, ""), "noise_gain": (float, None), "noise_read_sigma": (float, None),
    # NEW: --operator_name=burst_sr, K low-resolution frames of one scene (K <= --scale_factor^2, factor 2 .. 4): --kernel_path holds
    # a [K, kh, kw] array of per-frame PSFs, or one 2-D PSF that --frame_shifts="dy,dx;dy,dx;..." (K pairs, high-resolution pixels,
    # fractions allowed) displaces per frame; with K PSFs the K shifts apply one each
    "frame_shifts": (str, ""),
    # NEW: --operator_name=weighted_burst_sr, burst_sr (same --kernel_path, --scale_factor, --frame_shifts) with a noise level per
    # pixel of every frame: one of --noise_map_path (a .npy [So,So] / [3,So,So] for every frame, or [K,3,So,So] / [3K,So,So] /
    # [1,3K,So,So]), --frame_sigmas="a,b,c,..." (one level per frame, inf drops a frame) and the sensor pair --noise_gain /
    # --noise_read_sigma; --mosaic=rggb | bggr | grbg | gbrg makes every frame a raw Bayer frame (one channel per site)
    "frame_sigmas": (str, ""), "mosaic": (str, ""),
    # NEW: --operator_name=varying_blur, a PSF that changes across the field: --kernel_path holds a [K, kh, kw] array of PSFs
    # (K <= 16) and exactly one of --blend_path (a .npy of blend maps [K,S,S], [K,3,S,S] or [3K,S,S]) and --psf_grid=RxC (the
    # PSFs on an R x C grid, R * C = K, blended bilinearly between the cell centres: measurements.grid_blend_weights)
    "blend_path": (str, ""), "psf_grid": (str, ""),
    # NEW: --operator_name=fourier_sampling, undersampled k-space measured in the Hartley domain: the sampling mask is either
    # --mask_path (a 0/1 .npy [S,S], [3,S,S] or [1,3,S,S] in FFT order, DC at [0,0]; OR-ed with its point reflection) or
    # --kspace_pattern=cartesian|radial with --kspace_acceleration=R (and --kspace_center_fraction, --kspace_seed:
    # measurements.kspace_mask); --noise_map_path optionally gives the noise level per frequency (inf = not measured)
    "kspace_pattern": (str, ""), "kspace_acceleration": (float, None), "kspace_center_fraction": (float, None),
    "kspace_seed": (int, None),
    # NEW: K posterior samples per (image, seed) unit, 1 .. 64 (free_hunch_amd/ensemble.py): the K members share the operator's
    # random content and ONE measurement and differ in their initial noise alone.  K >= 2 adds posterior_samples/, posterior_mean/
    # (the MMSE estimate), posterior_std/ (.npy in 8-bit units, .png at 4 x) and the calibration lines of results.txt; images/
    # keeps member 0, which is the run without the flag
    "posterior_samples": (int, 1),
}


def _coerce(kind, text):
    if kind is bool:
        return text.strip().lower() in ("true", "yes", "1", "on")
    if kind == "ints":
        return [int(v.strip()) for v in text.split(",") if v.strip() != ""]
    if kind is int:
        return int(float(text))  # the README passes --scale_factor=4.0
    return kind(text)


def load_config(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    cfg = {k: d for k, (_t, d) in SCHEMA.items()}
    for arg in argv:
        if not arg.startswith("--") or "=" not in arg:
            raise SystemExit(f"expected --key=value, got '{arg}'")
        key, value = arg[2:].split("=", 1)
        cfg[key] = _coerce(SCHEMA[key][0], value) if key in SCHEMA else value
    if cfg["outdir"] is None:
        raise SystemExit("--outdir=DIR is required")
    if not 1 <= cfg["posterior_samples"] <= 64:
        raise SystemExit(f"--posterior_samples is the number of samples per measurement, 1 .. 64; got {cfg['posterior_samples']}")
    if bool(cfg["lpips_vgg_path"]) != bool(cfg["lpips_lin_path"]):
        raise SystemExit("--lpips_vgg_path and --lpips_lin_path go together: LPIPS needs both weight files")
    if cfg["operator_name"] == "custom_blur" and not cfg["kernel_path"]:
        raise SystemExit("--operator_name=custom_blur needs --kernel_path=FILE.npy (the PSF, a 2-D array)")
    if cfg["operator_name"] == "masked_blur":
        if not cfg["kernel_path"]:
            raise SystemExit("--operator_name=masked_blur needs --kernel_path=FILE.npy (the PSF, a 2-D array)")
        if not cfg["mask_path"] and cfg["mask_border"] == 0:
            raise SystemExit("--operator_name=masked_blur needs a mask: --mask_path=FILE.npy and / or --mask_border=N (without a "
                             "mask use --operator_name=custom_blur)")
    if cfg["operator_name"] == "custom_sr" and not cfg["kernel_path"]:
        raise SystemExit("--operator_name=custom_sr needs --kernel_path=FILE.npy (the PSF, a 2-D array) beside --scale_factor")
    if cfg["operator_name"] in ("burst_sr", "weighted_burst_sr") and not cfg["kernel_path"]:
        raise SystemExit(f"--operator_name={cfg['operator_name']} needs --kernel_path=FILE.npy (a [K, kh, kw] array of per-frame PSFs, or one 2-D "
                         "PSF beside --frame_shifts) beside --scale_factor")
    if cfg["operator_name"] == "varying_blur":
        if not cfg["kernel_path"]:
            raise SystemExit("--operator_name=varying_blur needs --kernel_path=FILE.npy (a [K, kh, kw] array of PSFs)")
        if bool(cfg["blend_path"]) == bool(cfg["psf_grid"]):
            raise SystemExit("--operator_name=varying_blur needs its blend maps: exactly one of --blend_path=FILE.npy and "
                             "--psf_grid=RxC")
    elif cfg["blend_path"] or cfg["psf_grid"]:
        raise SystemExit(f"--blend_path and --psf_grid belong to --operator_name=varying_blur; operator "
                         f"'{cfg['operator_name']}' does not read them")
    kspace = [k for k in ("kspace_pattern", "kspace_acceleration", "kspace_center_fraction", "kspace_seed")
              if cfg[k] not in ("", None)]
    if cfg["operator_name"] == "fourier_sampling":
        if bool(cfg["mask_path"]) == bool(cfg["kspace_pattern"]):
            raise SystemExit("--operator_name=fourier_sampling needs its sampling mask: exactly one of --mask_path=FILE.npy and "
                             "--kspace_pattern=cartesian|radial (with --kspace_acceleration=R)")
        if cfg["kspace_pattern"] and cfg["kspace_pattern"] not in ("cartesian", "radial"):
            raise SystemExit(f"--kspace_pattern is cartesian or radial, got '{cfg['kspace_pattern']}'")
        if cfg["kspace_pattern"] and cfg["kspace_acceleration"] is None:
            raise SystemExit("--kspace_pattern needs --kspace_acceleration=R (R >= 1: the undersampling factor)")
        if cfg["mask_path"] and kspace:
            raise SystemExit("--kspace_acceleration, --kspace_center_fraction and --kspace_seed go with --kspace_pattern, not with "
                             "--mask_path")
        if cfg["mask_border"] != 0:
            raise SystemExit("--mask_border belongs to --operator_name=masked_blur; operator 'fourier_sampling' does not read it")
        if cfg["noise_gain"] is not None or cfg["noise_read_sigma"] is not None:
            raise SystemExit("--noise_gain and --noise_read_sigma belong to --operator_name=weighted_blur / weighted_sr / "
                             "weighted_burst_sr; operator 'fourier_sampling' reads --noise_map_path only")
    elif kspace:
        raise SystemExit(f"--kspace_pattern, --kspace_acceleration, --kspace_center_fraction and --kspace_seed belong to "
                         f"--operator_name=fourier_sampling; operator '{cfg['operator_name']}' does not read them")
    if cfg["frame_shifts"] and cfg["operator_name"] not in ("burst_sr", "weighted_burst_sr"):
        raise SystemExit(f"--frame_shifts belongs to --operator_name=burst_sr (and weighted_burst_sr); operator "
                         f"'{cfg['operator_name']}' does not read it")
    if (cfg["frame_sigmas"] or cfg["mosaic"]) and cfg["operator_name"] != "weighted_burst_sr":
        raise SystemExit(f"--frame_sigmas and --mosaic belong to --operator_name=weighted_burst_sr; operator "
                         f"'{cfg['operator_name']}' does not read them")
    weighted = cfg["operator_name"] in ("weighted_blur", "weighted_sr")
    sensor = cfg["noise_gain"] is not None or cfg["noise_read_sigma"] is not None
    if cfg["operator_name"] == "weighted_burst_sr":
        if sensor and (cfg["noise_gain"] is None or cfg["noise_read_sigma"] is None):
            raise SystemExit("--noise_gain and --noise_read_sigma go together: the Poisson-Gaussian noise map needs both")
        if bool(cfg["noise_map_path"]) + bool(cfg["frame_sigmas"]) + sensor != 1:
            raise SystemExit("--operator_name=weighted_burst_sr needs a noise map: exactly one of --noise_map_path=FILE.npy, "
                             "--frame_sigmas=\"a,b,c,...\" and --noise_gain=G --noise_read_sigma=R")
    elif weighted:
        if not cfg["kernel_path"]:
            raise SystemExit(f"--operator_name={cfg['operator_name']} needs --kernel_path=FILE.npy (the PSF, a 2-D array)")
        if sensor and (cfg["noise_gain"] is None or cfg["noise_read_sigma"] is None):
            raise SystemExit("--noise_gain and --noise_read_sigma go together: the Poisson-Gaussian noise map needs both")
        if bool(cfg["noise_map_path"]) == sensor:
            raise SystemExit(f"--operator_name={cfg['operator_name']} needs a noise map: either --noise_map_path=FILE.npy or "
                             "--noise_gain=G --noise_read_sigma=R, not both")
    elif (cfg["noise_map_path"] or sensor) and cfg["operator_name"] != "fourier_sampling":
        raise SystemExit(f"--noise_map_path, --noise_gain and --noise_read_sigma belong to --operator_name=weighted_blur / "
                         f"weighted_sr / weighted_burst_sr (--noise_map_path also to fourier_sampling); operator "
                         f"'{cfg['operator_name']}' does not read them")
    if cfg["operator_name"] not in ("masked_blur", "fourier_sampling") and (cfg["mask_path"] or cfg["mask_border"] != 0):
        raise SystemExit(f"--mask_path and --mask_border belong to --operator_name=masked_blur (--mask_path also to "
                         f"fourier_sampling); operator '{cfg['operator_name']}' does not read them")
    if cfg["kernel_path"] and cfg["operator_name"] not in ("custom_blur", "masked_blur", "custom_sr", "weighted_blur",
                                                           "weighted_sr", "burst_sr", "weighted_burst_sr", "varying_blur"):
        raise SystemExit(f"--kernel_path is the PSF of --operator_name=custom_blur / masked_blur / custom_sr / weighted_blur / "
                         f"weighted_sr / burst_sr / weighted_burst_sr / varying_blur; operator "
                         f"'{cfg['operator_name']}' does not read it")
    return SimpleNamespace(**cfg)
