"""MI355X-native drop-in for the hot path of the reference's ``ElasticDiffusion`` class
(/root/reference/elastic_diffusion.py:110-1130, "ED:n" below; ControlNet variant "EDC:n" =
elastic_diffusion_w_controlnet.py): same constructor and ``generate_image`` surface, same RNG stream as the
reference's CPU path, but one image is a *program* (a generator, ``_program``) whose timestep is

    host   : pick-index draws (torch CPU generator, ED:501-544) + pad-strip reseed replay (ED:359)   -- no device sync
    HIP    : ed_assemble_rows       -> ONE model-input batch: K CFG pairs + V views (all d x d); ed_assemble_rows_x when the UNet
                                       is a 9-channel inpainting model (mask + masked-image latent behind every row's latent)
    yield  : ONE UNet forward for the whole batch (hipGraph replay; rows optionally sharded over ranks and all-gathered
             over RCCL; with several images in flight the rows of all pending calls are fused, per-row timesteps)
    HIP    : ed_phase_epilogue      -> unpad, fill, scatter, CFG + DDIM [, RRG] in one launch
    HIP    : [RePaint] ed_undo_step, then the same phase with K = 1 and guidance/3

instead of the reference's R+1 sequential batch-2 UNet calls, V/view_batch_size view calls and ~hundreds of eager
tensor ops with host syncs per step.  The resampling steps can be batched because their inputs depend only on the RNG,
never on each other's UNet outputs (ED:661-681): the sequential semantics live only in the overwrite order of the
fill, which the epilogue's per-pixel last-covering-step table reproduces.  (``FUSED_GLUE = False`` runs the same steps
through the separate entry points ed_pick_assemble ... ed_rrg_update.)

There is no CPU path in this module: without the HIP library and a ROCm device it raises.
"""
import math
import time

import numpy as np
import torch
import torch.nn as nn

from . import geometry, host_rng, ops
from .graphs import GraphedForward
from .schedule import SAMPLERS, CosineScheduler, DDIMSchedule, DPMSolverSchedule, LCMSchedule, check_eta
from .sharding import RowSharder


# Fused latent-space glue: ed_assemble_rows before the model call and ed_phase_epilogue (+ RRG) after it -- 2 launches
# per phase instead of 6-7.  False = the separate entry points (kept for A/B and for the per-kernel parity tests).
FUSED_GLUE = True

# Timesteps per pad-strip VAE call (see _strip_frames: a fixed call shape on every rank count)
STRIP_CHUNK = 5


def _identity_progress(it):
    return it


def _default_progress(it):
    """``progress=tqdm`` is the reference's default (ED:963); the identity when tqdm is not importable."""
    try:
        from tqdm import tqdm
    except ImportError:
        return it
    return tqdm(it)


def _make_grid(imgs, nrow=8, padding=2):
    """torchvision.utils.make_grid for a (N,C,H,W) batch with its defaults (what ED:1124 calls): a single image is
    returned as is; otherwise ``min(nrow, N)`` images per row, each cell offset by ``padding`` px of zeros (one shared
    2-px line between neighbours, a 2-px border top/left and bottom/right)."""
    N, C, H, W = imgs.shape
    if N == 1:
        return imgs[0]
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    h, w = H + padding, W + padding
    grid = imgs.new_zeros(C, h * ymaps + padding, w * xmaps + padding)
    for k in range(N):
        y, x = divmod(k, xmaps)
        grid[:, y * h + padding:y * h + padding + H, x * w + padding:x * w + padding + W] = imgs[k]
    return grid


def _on_own_device(fn):
    """Run a pipeline entry point with the pipeline's device current: hipGraph capture, side streams, events and the
    torch ops of the model all follow the calling thread's current device, and the reference accepts any device
    (``ElasticDiffusion(torch.device('cuda:1'))`` in a process whose current device is 0)."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        if self.device.index is None or self.device.index == torch.cuda.current_device():
            return fn(self, *a, **k)
        with torch.cuda.device(self.device):
            return fn(self, *a, **k)

    return wrapper


def check_img2img_arguments(num_inference_steps, init_image=None, strength=1.0, mask_image=None):
    """The argument rules of ``init_image`` / ``strength`` / ``mask_image``, pure host code that runs
    before anything is launched -> ``t_start``, the index of the first timestep the loop executes (0 = the whole schedule).
    ValueError: ``strength`` outside (0, 1] or leaving no step, ``strength != 1`` or a mask without an init image."""
    t_start = DDIMSchedule.img2img_window(num_inference_steps, strength)
    if init_image is None:
        if float(strength) != 1.0:
            raise ValueError(f"strength={strength!r} needs init_image (without one every image starts from pure noise)")
        if mask_image is not None:
            raise ValueError("mask_image needs init_image (the picture whose kept region it marks)")
    return t_start


MASK_MODES = ("binary", "graded")

# Input channels of an inpainting UNet: noisy latent (4) | latent mask (1) | masked-image latent (4)
INPAINT_IN_CHANNELS = 9


def scheduler_kind(scheduler):
    """The ``sampler`` name a scheduler object answers to ("euler_a" is spelled ``DDIMSchedule(eta=1)`` and answers to both)."""
    if isinstance(scheduler, LCMSchedule):
        return "lcm"
    if isinstance(scheduler, DPMSolverSchedule):
        return "dpmsolver++sde" if scheduler.algorithm_type == "sde-dpmsolver++" else "dpmsolver++"
    return "ddim"


def check_sampler_arguments(sampler=None, solver_order=2, scheduler=None, eta=0.0):
    """ValueError for a ``sampler`` / ``solver_order`` / ``eta`` ElasticDiffusion cannot honour (before anything is built):
    ``sampler`` is None (= "ddim" without a ``scheduler``, the scheduler's own kind with one) or one of ``schedule.SAMPLERS``; with
    a ``scheduler`` object it has to name that object's kind.  ``eta`` lies in [0, 1] and belongs to "ddim" alone ("euler_a" is
    its eta = 1 by name; a ``scheduler`` object carries its own)."""
    if sampler is not None and sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    if solver_order not in (1, 2):
        raise ValueError(f"solver_order must be 1 or 2, got {solver_order!r}")
    eta = check_eta(eta)
    if eta != 0.0 and (sampler or "ddim") != "ddim":
        raise ValueError(f"eta={eta!r} belongs to sampler='ddim', got sampler={sampler!r}")
    if eta != 0.0 and scheduler is not None:
        raise ValueError("eta is given together with a scheduler object: pass DDIMSchedule(eta=...) instead")
    if scheduler is not None and sampler is not None:
        kind = scheduler_kind(scheduler)
        if sampler == "euler_a" and kind == "ddim" and scheduler.eta == 1.0:
            kind = "euler_a"
        if kind != sampler:
            raise ValueError(f"sampler={sampler!r} but the scheduler object given is a {type(scheduler).__name__} ({kind!r})")


def check_regions_sampler(regions, scheduler):
    """ValueError for ``regions`` under a stochastic sampler, before anything launches: the regional epilogue has no noise variant
    (DESIGN.md section 29.6)."""
    if regions is None:
        return
    if getattr(scheduler, "eta", 0.0) != 0.0 or scheduler_kind(scheduler) in ("dpmsolver++sde", "lcm"):
        raise ValueError("regions are not supported with a stochastic sampler (DDIM with eta > 0, euler_a, dpmsolver++sde, lcm): "
                         "the regional epilogue has no noise variant")


def make_scheduler(base, sampler=None, solver_order=2, eta=0.0):
    """The scheduler of ``sampler`` with the settings of ``base`` (a DDIMSchedule read from a snapshot / the defaults)."""
    cfg = vars(base.config)
    if sampler == "dpmsolver++":  # the same schedule settings, the multistep update
        return DPMSolverSchedule(**cfg, solver_order=solver_order)
    if sampler == "dpmsolver++sde":  # ... and its stochastic form (section 29)
        return DPMSolverSchedule(**cfg, solver_order=solver_order, algorithm_type="sde-dpmsolver++")
    if sampler == "lcm":
        return LCMSchedule(**cfg)
    if sampler == "euler_a" or eta != 0.0:
        return DDIMSchedule(**cfg, eta=1.0 if sampler == "euler_a" else eta)
    return base


def check_inpaint_unet_arguments(in_channels, init_image=None, mask_image=None, mask_mode="binary", controlnet=False,
                                 latent_size=None):
    """The argument rules of a 9-channel inpainting UNet, pure host code that runs before anything is
    launched -> is this the 9-channel path?  ValueError: ``in_channels`` other than 4 or 9; with 9, a run without both
    ``init_image`` and ``mask_image``, ``mask_mode="graded"``, a ControlNet, or pictures that are not 8-bit (the hole is blanked in
    the init picture's bytes through the pixel mask: a float ``init_image`` or a mask at latent resolution carries neither)."""
    if in_channels == 4:
        return False
    if in_channels != INPAINT_IN_CHANNELS:
        raise ValueError(f"unet.config.in_channels must be 4 or {INPAINT_IN_CHANNELS} (an inpainting UNet), got {in_channels!r}")
    if controlnet:
        raise ValueError("a 9-channel inpainting UNet with a ControlNet is not supported")
    if init_image is None or mask_image is None:
        raise ValueError("a 9-channel inpainting UNet needs both init_image and mask_image (its extra input channels are the "
                         "mask and the encoding of the picture with the hole blanked)")
    if mask_mode == "graded":
        raise ValueError('mask_mode="graded" is not supported with a 9-channel inpainting UNet (there is no blend to release)')
    at_latent_size = (isinstance(mask_image, torch.Tensor) and mask_image.dtype in (torch.bool, torch.uint8)
                      and latent_size is not None and tuple(mask_image.shape) == tuple(latent_size))
    if not _is_8bit_picture(init_image, 3) or not _is_8bit_picture(mask_image, 1) or at_latent_size:
        raise ValueError("a 9-channel inpainting UNet needs an 8-bit init_image (RGB PIL image, uint8 [H,W,3]) and an 8-bit "
                         "picture mask_image (L PIL image, uint8 [H,W]) at pixel resolution")
    return True


def control_keep(n_steps, start, end):
    """diffusers 0.21.4's ``controlnet_keep`` for ``n_steps`` executed timesteps and per-net windows ``start`` / ``end`` (lists of N
    floats): keep[i][n] = 1.0 - float(i / T < start[n] or (i + 1) / T > end[n]), in Python floats exactly so."""
    return [[1.0 - float(i / n_steps < s or (i + 1) / n_steps > e) for s, e in zip(start, end)] for i in range(n_steps)]


def check_control_arguments(n_nets, nets_listed, scale, start=0.0, end=1.0, condition_image=None):
    """The argument rules of Multi-ControlNet and guidance windows (diffusers 0.21.4's ``check_inputs``), pure
    host code -> None for today's single-net path (one net that was not given as a list, a scalar scale, the default window), else
    (scales, starts, ends), three lists of ``n_nets`` floats.  ValueError: list lengths other than the number of nets, more than
    ``ops.CONTROL_MAX_NETS`` nets, a window outside 0 <= start < end <= 1, a list of condition images without a list of as many nets."""
    if isinstance(condition_image, (list, tuple)) and (not nets_listed or len(condition_image) != n_nets):
        raise ValueError(f"{len(condition_image)} condition images for " +
                         (f"{n_nets} ControlNets" if nets_listed else "a ControlNet that was not given as a list (controlnet=[...])"))
    listed = [isinstance(v, (list, tuple)) for v in (scale, start, end)]
    if not nets_listed and not any(listed) and float(start) == 0.0 and float(end) == 1.0:
        return None
    if n_nets < 1:
        raise ValueError("controlnet_conditioning_scale lists / control_guidance_start / control_guidance_end need a ControlNet")
    if n_nets > ops.CONTROL_MAX_NETS:
        raise ValueError(f"at most {ops.CONTROL_MAX_NETS} ControlNets, got {n_nets}")
    out = []
    for name, v, is_list in zip(("controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end"),
                                (scale, start, end), listed):
        if is_list and len(v) != n_nets:
            raise ValueError(f"{name} lists {len(v)} values for {n_nets} ControlNet{'s' if n_nets != 1 else ''}")
        out.append([float(x) for x in v] if is_list else [float(v)] * n_nets)
    for s0, e0 in zip(out[1], out[2]):
        if not 0.0 <= s0 < e0 <= 1.0:  # (NaN fails every comparison)
            raise ValueError(f"control guidance window must satisfy 0 <= start < end <= 1, got start {s0}, end {e0}")
    return tuple(out)


SCORE_PCA_KEYS = ("pca_cls_dir", "pca_uncond")  # the reference script's file names (pca_diffusion_scores.py:181, 196)


def check_score_pca_arguments(score_pca, channels):
    """``score_pca`` projects 4-channel scores onto three components: a latent of another channel count
    (``channels``: the model's OUTPUT channels, what the class direction and the unconditional score have) is refused."""
    if score_pca and channels != 4:
        raise ValueError(f"score_pca maps a 4-channel score onto its first three principal components; this model's scores have "
                         f"{channels} channels")
    return bool(score_pca)


def check_ip_adapter_arguments(loaded, has_image_encoder, ip_adapter_image=None, ip_adapter_image_embeds=None,
                               ip_adapter_negative_image_embeds=None):
    """The argument rules of ``ip_adapter_image`` / ``ip_adapter_image_embeds``, pure host code that runs
    before anything is launched -> does this run carry an image prompt?  ValueError: an adapter is loaded and no image is given
    (or both forms are), an image is given without an adapter, ``ip_adapter_image`` without an image encoder.
    ``loaded`` / ``has_image_encoder`` may be lists, one entry per loaded adapter -- its kind ("base" | "plus") and whether it has an
    encoder: the rules of several adapters and of Plus adapters (section 32; ``check_ip_adapters_arguments``)."""
    if not isinstance(loaded, (list, tuple)):
        loaded, has_image_encoder = (["base"], [bool(has_image_encoder)]) if loaded else ([], [])
    if len(loaded) > 1 or "plus" in loaded or (loaded and ip_adapter_negative_image_embeds is not None):
        return check_ip_adapters_arguments(list(loaded), list(has_image_encoder), ip_adapter_image, ip_adapter_image_embeds,
                                           ip_adapter_negative_image_embeds)
    loaded, has_image_encoder = bool(loaded), bool(loaded and has_image_encoder[0])   # one base adapter: the rules as they were
    if isinstance(ip_adapter_image, (list, tuple)) and len(ip_adapter_image) == 1:
        ip_adapter_image = ip_adapter_image[0]
    if isinstance(ip_adapter_image_embeds, (list, tuple)) and len(ip_adapter_image_embeds) == 1:
        ip_adapter_image_embeds = ip_adapter_image_embeds[0]
    given = (ip_adapter_image is not None) + (ip_adapter_image_embeds is not None)
    if not loaded:
        if given or ip_adapter_negative_image_embeds is not None:
            raise ValueError("ip_adapter_image / ip_adapter_image_embeds given but no IP-Adapter is loaded (load_ip_adapter)")
        return False
    if given != 1:
        raise ValueError("an IP-Adapter is loaded: every image needs exactly one of ip_adapter_image / ip_adapter_image_embeds "
                         f"({'both' if given else 'neither'} given); unload_ip_adapter() goes back to text-only generation")
    if ip_adapter_image is not None:
        if not has_image_encoder:
            raise ValueError("ip_adapter_image needs the image_encoder given to load_ip_adapter (a CLIP vision model); without one "
                             "pass ip_adapter_image_embeds")
        if not _is_8bit_picture(ip_adapter_image, 3):
            raise ValueError("ip_adapter_image must be an RGB PIL image or a uint8 [H,W,3] array / tensor, got "
                             f"{type(ip_adapter_image).__name__}")
    elif not isinstance(ip_adapter_image_embeds, torch.Tensor) or ip_adapter_image_embeds.dim() != 2:
        raise ValueError("ip_adapter_image_embeds must be a [1 or B, clip_dim] tensor, got "
                         f"{tuple(getattr(ip_adapter_image_embeds, 'shape', ())) or type(ip_adapter_image_embeds).__name__}")
    return True


def ip_adapter_entries(value, count, what):
    """``value`` of a run keyword as a list with one entry per loaded adapter: a list / tuple of ``count`` entries, or a bare value
    where one adapter is loaded"""
    if isinstance(value, (list, tuple)):
        if len(value) != count:
            raise ValueError(f"{what} has {len(value)} entries but {count} IP-Adapter(s) are loaded: one entry per adapter, in load order")
        return list(value)
    if count != 1:
        raise ValueError(f"{count} IP-Adapters are loaded: {what} must be a list with one entry per adapter, in load order")
    return [value]


def check_ip_adapters_arguments(kinds, has_encoder, ip_adapter_image=None, ip_adapter_image_embeds=None,
                                ip_adapter_negative_image_embeds=None):
    """``check_ip_adapter_arguments`` for several adapters and for Plus adapters: ``kinds`` = "base" | "plus"
    per loaded adapter, ``has_encoder`` alike.  Exactly one of the two forms, as a list with one entry per adapter (a bare value with
    one adapter); a picture needs that adapter's encoder; embeddings are [1 or B, clip_dim] for a base adapter and [1 or B, S,
    embed_dim] (the CLIP vision model's penultimate hidden states) for a Plus adapter; a Plus adapter given as embeddings needs its
    unconditional embeddings too (``ip_adapter_negative_image_embeds``, same list form; an entry may be None for a base adapter,
    whose unconditional tokens are the projection of zeros)."""
    A = len(kinds)
    given = (ip_adapter_image is not None) + (ip_adapter_image_embeds is not None)
    if given != 1:
        raise ValueError(f"{A} IP-Adapter(s) are loaded: every image needs exactly one of ip_adapter_image / ip_adapter_image_embeds "
                         f"({'both' if given else 'neither'} given); unload_ip_adapter() goes back to text-only generation")
    if ip_adapter_image is not None:
        if ip_adapter_negative_image_embeds is not None:
            raise ValueError("ip_adapter_negative_image_embeds goes with ip_adapter_image_embeds: with ip_adapter_image the unconditional "
                             "tokens come from the image encoder")
        for a, img in enumerate(ip_adapter_entries(ip_adapter_image, A, "ip_adapter_image")):
            if not has_encoder[a]:
                raise ValueError(f"ip_adapter_image needs the image_encoder given to load_ip_adapter (adapter {a} has none); without "
                                 "one pass ip_adapter_image_embeds")
            if not _is_8bit_picture(img, 3):
                raise ValueError(f"ip_adapter_image[{a}] must be an RGB PIL image or a uint8 [H,W,3] array / tensor, got {type(img).__name__}")
        return True
    embeds = ip_adapter_entries(ip_adapter_image_embeds, A, "ip_adapter_image_embeds")
    neg = ([None] * A if ip_adapter_negative_image_embeds is None
           else ip_adapter_entries(ip_adapter_negative_image_embeds, A, "ip_adapter_negative_image_embeds"))
    for a, (kind, e, n) in enumerate(zip(kinds, embeds, neg)):
        rank, shape = (3, "[1 or B, S, embed_dim]") if kind == "plus" else (2, "[1 or B, clip_dim]")
        for name, t in (("ip_adapter_image_embeds", e), ("ip_adapter_negative_image_embeds", n)):
            if t is None and name == "ip_adapter_negative_image_embeds":
                continue
            if not isinstance(t, torch.Tensor) or t.dim() != rank:
                raise ValueError(f"{name}[{a}] must be a {shape} tensor for a {kind} adapter, got "
                                 f"{tuple(getattr(t, 'shape', ())) or type(t).__name__}")
        if kind == "plus" and n is None:
            raise ValueError(f"adapter {a} is a Plus adapter given as embeddings: its unconditional image tokens are the Resampler of the "
                             "encoder's output for an all-zero picture, which only the caller has -- pass "
                             "ip_adapter_negative_image_embeds (same list form)")
        if n is not None and tuple(n.shape[1:]) != tuple(e.shape[1:]):
            raise ValueError(f"ip_adapter_negative_image_embeds[{a}] is {tuple(n.shape)}, ip_adapter_image_embeds[{a}] {tuple(e.shape)}")
    return True


def read_ip_adapter(source):
    """-> (flat state dict, name) of an IP-Adapter: a ``*.safetensors`` file with flat ``image_proj.*`` / ``ip_adapter.*`` keys, a
    ``*.bin`` / ``*.pt`` file holding the nested ``{"image_proj": {...}, "ip_adapter": {...}}`` form (read with
    ``torch.load(weights_only=True)``), or a state dict in either form."""
    import os
    from .models import flatten_ip_adapter_state
    if isinstance(source, dict):
        return flatten_ip_adapter_state(source), "ip_adapter"
    path = os.fspath(source)
    name = os.path.splitext(os.path.basename(path))[0]
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return flatten_ip_adapter_state(load_file(path, device="cpu")), name
    if path.endswith((".bin", ".pt", ".pth")):
        return flatten_ip_adapter_state(torch.load(path, map_location="cpu", weights_only=True)), name
    raise ValueError(f"IP-Adapter file must be *.safetensors, *.bin or *.pt, got {path!r}")


def _is_8bit_picture(image, channels):
    """is ``image`` what ``_u8_image`` takes as an 8-bit picture: a PIL image or a uint8 array / tensor [H,W,channels]?"""
    if hasattr(image, "convert"):
        return True
    if not isinstance(image, (np.ndarray, torch.Tensor)) or image.dtype not in (np.uint8, torch.uint8):
        return False
    return (image.ndim == 3 and image.shape[2] == channels) or (image.ndim == 2 and channels == 1)


def check_soft_inpaint_arguments(init_image=None, mask_image=None, mask_blur=0.0, mask_mode="binary", composite=False,
                                 output_type="pil", grid=False, latent_size=None):
    """The argument rules of ``mask_blur`` / ``mask_mode`` / ``composite``, pure host code that runs
    before anything is launched -> ``mask_blur`` as a float.  ValueError: a radius that is not finite, negative or above
    ``ops.MASK_BLUR_MAX``; an unknown mode; any of the three without ``mask_image``; ``mask_blur`` or ``composite`` with a mask
    that is a tensor at latent resolution (``latent_size`` = (Hl, Wl)) and not an 8-bit picture; ``composite`` without an
    8-bit ``init_image``, with another ``output_type`` than "pil" or with ``grid``."""
    try:
        blur = float(mask_blur)
    except (TypeError, ValueError):
        raise ValueError(f"mask_blur must be a number in [0, {ops.MASK_BLUR_MAX:g}], got {mask_blur!r}") from None
    if not 0.0 <= blur <= ops.MASK_BLUR_MAX:  # also refuses NaN
        raise ValueError(f"mask_blur must be finite and in [0, {ops.MASK_BLUR_MAX:g}], got {mask_blur!r}")
    if mask_mode not in MASK_MODES:
        raise ValueError(f"mask_mode must be one of {MASK_MODES}, got {mask_mode!r}")
    if mask_image is None:
        for name, on in (("mask_blur", blur > 0), ("mask_mode", mask_mode != "binary"), ("composite", composite)):
            if on:
                raise ValueError(f"{name} needs mask_image")
        return blur
    at_latent_size = (isinstance(mask_image, torch.Tensor) and mask_image.dtype in (torch.bool, torch.uint8)
                      and latent_size is not None and tuple(mask_image.shape) == tuple(latent_size))
    picture = _is_8bit_picture(mask_image, 1) and not at_latent_size
    if blur > 0 and not picture:
        raise ValueError("mask_blur needs an 8-bit picture mask (L PIL image, uint8 [H,W]), not a tensor at latent resolution")
    if composite:
        if not picture:
            raise ValueError("composite needs an 8-bit picture mask (L PIL image, uint8 [H,W]): it is the alpha of the paste")
        if not _is_8bit_picture(init_image, 3):
            raise ValueError("composite needs an 8-bit init_image (RGB PIL image, uint8 [H,W,3]), the picture that is pasted over")
        if output_type != "pil":
            raise ValueError(f"composite needs output_type='pil', got {output_type!r}")
        if grid:
            raise ValueError("composite needs grid=False: one composited image per prompt")
    return blur


MAX_REGIONS = 7  # + the base prompt = ops.MAX_REGION_ROWS conditional rows per resampling step


def check_region_arguments(regions, height, width, scale=8, region_blur=0.0, in_channels=4):
    """The argument rules of ``regions`` / ``region_blur`` (regional prompts), pure host code that runs before
    anything is launched -> (None, 0.0) without regions, else ([(prompt, mask, weight), ...], region_blur as a float) with every
    weight a float and every mask one of: ("box", (x0, y0, x1, y1)) in pixels, ("pixel", picture) an 8-bit picture (L PIL image,
    uint8 [H,W] / [H,W,1]) of height x width, ("latent", uint8 array / tensor) of (height // scale, width // scale).
    ValueError: not 1..7 regions; an entry that is not (prompt, mask) or (prompt, mask, weight); a prompt that is not a string; a
    weight that is not a finite float > 0; a mask of any other size or kind; a box that is empty or leaves the picture; a blur
    radius that is not in [0, ops.MASK_BLUR_MAX]; ``region_blur`` without regions; a 9-channel inpainting UNet."""
    try:
        blur = float(region_blur)
    except (TypeError, ValueError):
        raise ValueError(f"region_blur must be a number in [0, {ops.MASK_BLUR_MAX:g}], got {region_blur!r}") from None
    if not 0.0 <= blur <= ops.MASK_BLUR_MAX:  # also refuses NaN
        raise ValueError(f"region_blur must be finite and in [0, {ops.MASK_BLUR_MAX:g}], got {region_blur!r}")
    if regions is None:
        if blur > 0:
            raise ValueError("region_blur needs regions")
        return None, 0.0
    if in_channels != 4:
        raise ValueError("regions are not supported with a 9-channel inpainting UNet (its mask and masked-image rows are out of "
                         "scope for regional prompts)")
    regions = list(regions)
    if not 1 <= len(regions) <= MAX_REGIONS:
        raise ValueError(f"regions must hold 1 to {MAX_REGIONS} (prompt, mask[, weight]) entries, got {len(regions)}")
    Hl, Wl = height // scale, width // scale
    out = []
    for k, entry in enumerate(regions):
        if not isinstance(entry, (tuple, list)) or len(entry) not in (2, 3):
            raise ValueError(f"regions[{k}] must be (prompt, mask) or (prompt, mask, weight), got {entry!r}")
        prompt, mask = entry[0], entry[1]
        if not isinstance(prompt, str):
            raise ValueError(f"regions[{k}]: the prompt must be a string (it applies to every sample), got {type(prompt).__name__}")
        try:
            weight = float(entry[2]) if len(entry) == 3 else 1.0
        except (TypeError, ValueError):
            raise ValueError(f"regions[{k}]: weight must be a float > 0, got {entry[2]!r}") from None
        if not 0.0 < weight < float("inf"):
            raise ValueError(f"regions[{k}]: weight must be a finite float > 0, got {entry[2]!r}")
        if isinstance(mask, (tuple, list)):
            if len(mask) != 4 or not all(isinstance(v, (int, np.integer)) for v in mask):
                raise ValueError(f"regions[{k}]: a box must be four ints (x0, y0, x1, y1) in pixels, got {mask!r}")
            x0, y0, x1, y1 = (int(v) for v in mask)
            if not (0 <= x0 < x1 <= width and 0 <= y0 < y1 <= height):
                raise ValueError(f"regions[{k}]: box {tuple(mask)} must satisfy 0 <= x0 < x1 <= {width} and 0 <= y0 < y1 <= {height}")
            out.append((prompt, ("box", (x0, y0, x1, y1)), weight))
            continue
        if hasattr(mask, "convert"):
            size = (mask.size[1], mask.size[0])
        elif isinstance(mask, (np.ndarray, torch.Tensor)) and mask.dtype in (np.uint8, torch.uint8) and \
                (mask.ndim == 2 or (mask.ndim == 3 and mask.shape[2] == 1)):
            size = tuple(int(v) for v in mask.shape[:2])
        else:
            raise ValueError(f"regions[{k}]: the mask must be an L PIL image, a uint8 [H,W] array / tensor or a box (x0, y0, x1, y1), "
                             f"got {type(mask).__name__} {getattr(mask, 'dtype', '')}")
        if size == (height, width):
            out.append((prompt, ("pixel", mask), weight))
        elif size == (Hl, Wl) and not hasattr(mask, "convert"):
            out.append((prompt, ("latent", mask), weight))
        else:
            raise ValueError(f"regions[{k}]: the mask is {size}; it must be the picture's {(height, width)} or, as a uint8 array / "
                             f"tensor, the latent's {(Hl, Wl)}")
    return out, blur


def check_ip_adapter_mask_arguments(n_adapters, ip_adapter_masks, height, width, scale=8):
    """The argument rules of ``ip_adapter_masks`` (IP-Adapter attention masks), pure host code that runs before
    anything is launched -> None without masks, else one entry per loaded adapter: None (no mask: all ones) or what
    ``check_region_arguments`` makes of a region's mask -- ("box", (x0, y0, x1, y1)), ("pixel", picture), ("latent", array) -- read
    through that function, so the accepted forms are ``regions``' forms.
    ValueError: masks without a loaded adapter; a count other than the adapters'; a size that is neither the picture's nor the
    latent's; a box that is empty or leaves the picture; any other kind of mask."""
    if ip_adapter_masks is None:
        return None
    if not n_adapters:
        raise ValueError("ip_adapter_masks given but no IP-Adapter is loaded")
    if not isinstance(ip_adapter_masks, (list, tuple)) or len(ip_adapter_masks) != n_adapters:
        n = len(ip_adapter_masks) if isinstance(ip_adapter_masks, (list, tuple)) else 1
        raise ValueError(f"ip_adapter_masks must be a list with one entry per adapter (a mask or None): {n_adapters} adapter(s) "
                         f"loaded, {n} mask(s) given")
    out = []
    for k, mask in enumerate(ip_adapter_masks):
        if mask is None:
            out.append(None)
            continue
        try:
            out.append(check_region_arguments([("", mask)], height, width, scale)[0][0][1])
        except ValueError as e:
            raise ValueError(str(e).replace("regions[0]", f"ip_adapter_masks[{k}]")) from None
    return out


class _Plan:
    """Per-call geometry: host plans (geometry.py) + their int32 device tables + the pick sampler."""


class _Rescale:
    """Guidance rescale of ONE image in flight (``guidance_rescale`` > 0): the factor and its device buffers -- the
    per-sample std ratios the moments kernels write and the epilogue / DDIM / RRG kernels read (never the host), and the
    partials workspace.  Allocated once per image; every phase reuses them (launches are ordered on one stream).
    ``ratio_low`` (B floats) and the reduced-resolution part of the workspace (a few KB) are allocated whether or not RRG ever
    becomes active in the run: cheaper than deciding it per timestep."""

    def __init__(self, gr, B, n_full, n_low, device):
        self.gr = gr
        self.ratio = torch.empty(B, device=device, dtype=torch.float32)
        self.ratio_low = torch.empty(B, device=device, dtype=torch.float32)
        self.ws = ops.guidance_moments_workspace(B, n_full, n_low, device)


class _ModelCall:
    """One request of a denoising program to the model boundary: ``rows`` [n,C,d,d] in the model dtype at timestep
    ``t`` (0-d device tensor) with per-row text / pooled / ControlNet-condition rows.  Programs are generators that
    yield these and receive the model output rows (see ``_phase_steps``): the driver decides whether a call runs on its
    own (one image in flight) or fused with the calls of other images (``generate_latents_interleaved``)."""
    __slots__ = ("rows", "t", "text", "pooled", "cond", "direct", "ctl", "ipm")

    def __init__(self, rows, t, text, pooled, cond=None, direct=False, ctl=None, ipm=None):
        self.rows, self.t, self.text, self.pooled, self.cond, self.direct = rows, t, text, pooled, cond, direct
        # Multi-ControlNet (section 31): (indices of the nets this call runs, f32 [n, len(indices)] per-row weights); ``cond``
        # then holds those nets' condition rows stacked along the channels
        self.ctl = ctl
        # IP-Adapter attention masks (section 33): (f32 [n, A, S] per-row masks of ``ops.ip_mask_rows``, PH, PW) or None
        self.ipm = ipm


class _HostRng:
    """The host generator state of ONE image in flight (torch CPU generator + numpy MT19937).  The reference runs
    images one after the other on the global generators; with several images interleaved, each program must see
    exactly the stream it would have seen alone, so the globals are swapped in and out around every turn."""

    def __init__(self, seed):
        outer = (torch.get_rng_state(), np.random.get_state())
        # CPU generator + numpy only: ``torch.manual_seed`` would also re-seed every device generator, which this
        # path never draws from, and the caller's device RNG state is not ours to change
        torch.default_generator.manual_seed(int(seed))
        np.random.seed(seed)
        self.state = (torch.get_rng_state(), np.random.get_state())
        torch.set_rng_state(outer[0])
        np.random.set_state(outer[1])

    def __enter__(self):
        self.outer = (torch.get_rng_state(), np.random.get_state())
        torch.set_rng_state(self.state[0])
        np.random.set_state(self.state[1])

    def __exit__(self, *exc):
        self.state = (torch.get_rng_state(), np.random.get_state())
        torch.set_rng_state(self.outer[0])
        np.random.set_state(self.outer[1])


class _Stager:
    """Pinned host staging ring: host RNG results are written into pinned memory and uploaded with an async copy;
    a slot is reused only after its copy event has completed, so the host may run ahead of the GPU."""

    def __init__(self, depth=4):
        self.depth = depth
        self.rings = {}
        self.slot_of = {}
        self.waited = 0.0  # seconds the host spent blocked because it was a full ring ahead of the GPU

    def host(self, shape, dtype):
        key = (tuple(shape), dtype)
        ring = self.rings.setdefault(key, {"slots": [], "next": 0})
        k = ring["next"] % self.depth
        ring["next"] += 1
        if k >= len(ring["slots"]):
            buf = torch.empty(shape, dtype=dtype, pin_memory=True)
            ring["slots"].append([buf, None])
            self.slot_of[buf.data_ptr()] = ring["slots"][-1]
        slot = ring["slots"][k]
        if slot[1] is not None:
            w0 = time.perf_counter()
            slot[1].synchronize()  # the async upload that last used this slot must have finished
            self.waited += time.perf_counter() - w0
            slot[1] = None
        return slot[0]

    def upload(self, host_buf, device):
        dev = torch.empty(host_buf.shape, dtype=host_buf.dtype, device=device)
        dev.copy_(host_buf, non_blocking=True)
        with torch.cuda.device(device):  # the copy ran on ``device``'s current stream: record the event there
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
        self.slot_of[host_buf.data_ptr()][1] = ev
        return dev


class ElasticDiffusion(nn.Module):
    """Constructor signature of ED:111-115 plus keyword-only injection points (no pretrained weights, ``diffusers`` or
    network exist in the build environment): ``unet``, ``vae``, ``scheduler``, ``text_encoder`` (callable
    ``prompts -> (embeds, pooled)``), ``controlnet``, ``process_group``.  ``max_prompt_chunks`` / ``prompt_weighting`` are handed
    to ``text.load_clip`` when the CLIP encoders come from ``weights`` (prompts of up to that many 75-token chunks instead of
    truncation, A1111's ``(word:1.3)`` syntax; both off by default).

    ``sampler`` / ``solver_order`` (keyword-only): ``"dpmsolver++"`` samples with DPM-Solver++(2M) at order
    ``solver_order`` (1 or 2) on the same timestep grid instead of DDIM -- the update is a variant of the same step launches, reading
    the previous timestep's x0; passing ``scheduler=DPMSolverSchedule(...)`` does the same.  None / ``"ddim"``: the loop as it was.

    The stochastic samplers: ``sampler="ddim"`` with ``eta`` in (0, 1], ``"euler_a"`` (= DDIM at eta = 1, the
    ancestral step on this timestep grid), ``"dpmsolver++sde"`` (SDE-DPM-Solver++(2M)) and ``"lcm"`` (the scheduler an LCM-LoRA is
    sampled with) add ``c_n * noise`` to the same update in the same launches; the noise is one latent-sized host draw per phase, in
    the order a stochastic scheduler would draw inside the reference.  ``regions`` are refused with them."""

    def __init__(self, device, sd_version="2.0", verbose=False, log_freq=5, view_batch_size=1, low_vram=False, *,
                 unet=None, vae=None, scheduler=None, text_encoder=None, controlnet=None, process_group=None,
                 model_dtype=None, weights=None, cache_backgrounds=False, use_graphs=True, residual_fp32=None,
                 max_prompt_chunks=1, prompt_weighting=False, sampler=None, solver_order=2, eta=0.0):
        super().__init__()
        check_sampler_arguments(sampler, solver_order, scheduler, eta)
        device = torch.device(device)
        if device.type == "cuda" and device.index is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("elasticdiffusion_official_amd runs the hot path in HIP kernels on an MI355X; "
                               f"device={device} is not a ROCm device and there is no CPU fallback "
                               "(the CPU restatement lives in oracle/ and is test infrastructure only)")
        from . import _hip
        _hip.lib()  # fail here, loudly, if the extension is missing
        self.device = device
        self.sd_version = sd_version
        self.verbose = verbose
        self.log_freq = log_freq
        self.view_batch_size = view_batch_size
        self.low_vram = low_vram
        self.torch_dtype = torch.float32  # latent-space state is always fp32 (ED:121 uses fp16 only for low_vram)
        xl = sd_version.startswith("XL")
        if unet is None or vae is None:
            from .models import build_models
            built_unet, built_vae = build_models(sd_version, device=device, dtype=model_dtype, weights=weights)
            unet = unet if unet is not None else built_unet
            vae = vae if vae is not None else built_vae
        self.unet = self._model_layout(unet.to(device))
        # Precision mode of a 16-bit UNet (round 6).  residual_fp32 = True: the residual stream in fp32 under the 16-bit branches
        # (models._stream32) -- the mode that meets north_star's 1e-3 where plain fp16 does not.  None (default) = by MEASUREMENT, per model
        # family (bench.py's live fp32 leg): the SDXL workloads' plain-fp16 latents end 7.2e-4 ... 9.1e-4 from the
        # fp32 loop's, SD 1.x's 1.09-1.12e-3 -- so the SD 1.x / 2.x family runs the stream mode (9.7e-4, +4.3 % time) and SDXL plain fp16.
        from .models import UNet2DConditionModel as _OwnUNet
        p0 = next(iter(self.unet.parameters()), None) if isinstance(self.unet, torch.nn.Module) else None
        is16 = p0 is not None and p0.dtype in (torch.float16, torch.bfloat16)
        if residual_fp32 is None:
            residual_fp32 = not xl
        self.residual_fp32 = bool(residual_fp32) and is16 and isinstance(self.unet, _OwnUNet)
        if isinstance(self.unet, _OwnUNet):
            self.unet.residual_fp32 = self.residual_fp32
        self.vae = vae.to(device)
        if isinstance(self.vae, torch.nn.Module) and self.device.type == "cuda":
            from .models import prepare_vae_split
            prepare_vae_split(self.vae)     # split fp16 weights of the fp32 VAE's MFMA convolutions, built at load time
        # a LIST of ControlNets (even of one) takes the multi path of DESIGN.md section 31; ``self.controlnet`` stays the first net
        self.controlnets_listed = isinstance(controlnet, (list, tuple))
        nets = list(controlnet) if self.controlnets_listed else ([] if controlnet is None else [controlnet])
        self.controlnets = [self._model_layout(cn.to(device)) for cn in nets]
        self.controlnet = self.controlnets[0] if self.controlnets else None
        self._check_controlnets()
        if scheduler is None:
            scheduler = DDIMSchedule.from_config_dir(weights) if weights else DDIMSchedule()  # ED:153
            scheduler = make_scheduler(scheduler, sampler, solver_order, float(eta))
        self.scheduler = scheduler
        if text_encoder is None and weights:
            # real UNet/VAE weights with synthetic prompt embeddings would be prompt-independent garbage: a snapshot
            # must carry its CLIP encoders (ED:145-151); a failure to load them is an error, not a silent fallback
            from .text import load_clip
            text_encoder = load_clip(weights, xl, device, max_prompt_chunks=max_prompt_chunks, prompt_weighting=prompt_weighting)
        self.text_encoder = text_encoder
        self.model_size = 128 if xl else 64  # d_H, d_W of ED:398-400
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1)  # ED:156
        self.sharder = RowSharder(process_group)
        # The noised-background frames depend only on (pad geometry, timestep schedule, VAE): with cache_backgrounds
        # they are computed for the first image of a size and reused (the reference's own TODO, ED:340).  Off by
        # default so that every image pays for its own frames.
        self.cache_backgrounds = cache_backgrounds
        self._frame_cache = {}
        # one hipGraph per model batch shape (graphs.py); falls back to eager launches if a capture fails
        self._runner = GraphedForward(self._forward_rows, enabled=use_graphs, prepare=self._text_kv)
        self._time_ids = torch.zeros(1, 6, dtype=torch.float32, device=device)  # persistent: captured by the graphs
        self.set_view_config()
        self.default_size = None
        self._stager = _Stager()
        self.host_s = {"picks": 0.0, "phase_total": 0.0, "noise": 0.0, "stager_wait": 0.0}  # reset per image by _setup_run
        self.last_latents = None
        self.last_init_latents = None  # z0 of the last image started with ``init_image`` (its encoded, scaled latent)
        self.last_init_pixels = None   # uint8 [height,width,3]: the (resized) 8-bit init picture of the last such image, on the device
        self.last_pixel_mask = None    # uint8 [height,width]: its (resized, blurred) 8-bit picture mask, on the device
        self.last_masked_image_latents = None  # zm of the last image on a 9-channel UNet (the blanked picture's scaled latent)
        self.last_score_pca = None     # the PCA maps of the last ``generate_latents(score_pca=True)``, else None
        self.last_region_weights = None  # f32 [n + 1,Hl,Wl] of the last run with ``regions`` (plane 0 the base prompt's), else None

    def _check_controlnets(self):
        """All nets of a Multi-ControlNet share one parameter dtype and the UNet's 4-channel family (latent channels, context width)"""
        nets = self.controlnets
        if not self.controlnets_listed:  # (a single net is taken as it always was)
            return
        if not 1 <= len(nets) <= ops.CONTROL_MAX_NETS:
            raise ValueError(f"controlnet lists {len(nets)} nets: 1 .. {ops.CONTROL_MAX_NETS} are supported")
        def sig(m):
            p = next(m.parameters(), None) if isinstance(m, torch.nn.Module) else None
            c = getattr(m, "config", None)
            return (None if p is None else p.dtype, getattr(c, "in_channels", None), getattr(c, "cross_attention_dim", None),
                    getattr(c, "block_out_channels", None))
        if len(nets) > 1:
            sigs = [sig(m) for m in nets]
            if any(g != sigs[0] for g in sigs[1:]):
                raise ValueError(f"the ControlNets of one pipeline must share dtype and model family, got {sigs}")
        for m in nets:
            c, u = getattr(m, "config", None), getattr(self.unet, "config", None)
            for name in ("cross_attention_dim", "block_out_channels"):
                a, b = getattr(c, name, None), getattr(u, name, None)
                if a is not None and b is not None and (tuple(a) if isinstance(a, (list, tuple)) else a) != \
                        (tuple(b) if isinstance(b, (list, tuple)) else b):
                    raise ValueError(f"a ControlNet's {name} {a} does not match the UNet's {b}")
            if getattr(c, "in_channels", 4) != 4:
                raise ValueError(f"a ControlNet takes the 4 latent channels, got in_channels {c.in_channels}")

    @staticmethod
    def _model_layout(module):
        """16-bit UNet / ControlNet weights in the memory format the forward runs in (models.CHANNELS_LAST), so that no
        convolution has to re-lay-out its filter on every call; idempotent, and a no-op for fp32 / injected stand-ins."""
        from . import models
        p = next(module.parameters(), None)
        if models.CHANNELS_LAST and p is not None and p.dtype in (torch.bfloat16, torch.float16):
            module = module.to(memory_format=torch.channels_last)
        return module

    def _mark(self, name):
        """Phase markers (HIP events on the current stream; read only by ``phase_times`` after a sync)."""
        if name == "start":
            self._marks = []
        with torch.cuda.device(self.device):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(self.device))
        self._marks.append((name, ev))

    def phase_times(self):
        """-> {phase: ms} of the last generate_image call (synchronises)."""
        torch.cuda.synchronize(self.device)
        m = self._marks
        return {b[0]: a[1].elapsed_time(b[1]) for a, b in zip(m[:-1], m[1:])}

    # ---- small API surface the reference's callers use (APP:35-39, ED:159-171, 943-950) -----------------
    def set_view_config(self, patch_size=None):
        s = self.unet.config.sample_size
        w = patch_size if patch_size is not None else s // 2
        self.view_config = {"window_size": w, "stride": w, "context_size": s - w}

    def seed_everything(self, seed, seed_np=True):
        host_rng.seed_everything(seed, seed_np)

    def get_downsample_size(self, H, W):
        return geometry.reduced_size(H, W, self.sd_version, self.vae_scale_factor)

    def get_views(self, panorama_height, panorama_width, h_ws=64, w_ws=64, stride=32, **kwargs):
        s = self.vae_scale_factor
        if panorama_height % s or panorama_width % s:
            raise ValueError(f"height {panorama_height} and Width {panorama_width} must be divisable by {s}")
        rows = geometry.axis_windows(panorama_height // s, h_ws, stride)
        cols = geometry.axis_windows(panorama_width // s, w_ws, stride)
        return [(r[0], r[1], c[0], c[1]) for r in rows for c in cols]

    @property
    def model_dtype(self):
        return next(self.unet.parameters()).dtype

    # ---- LoRA adapters, merged into the weights ----------------------------------
    def _lora_state(self):
        """The adapter state, made on first use: a pipeline that never loads an adapter allocates and launches nothing for it."""
        st = self.__dict__.get("_lora")
        if st is None:
            from . import lora, models
            encs = list(getattr(self.text_encoder, "encoders", None) or [])
            targets = {"unet": self.unet, "text_encoder": encs[0] if encs else None,
                       "text_encoder_2": encs[1] if len(encs) > 1 else None}
            cfg = None
            if isinstance(self.unet, models.UNet2DConditionModel):
                try:  # block structure only (layers per block, attention placement): the same at full and reduced width
                    cfg = models.unet_config(models.family(self.sd_version))
                except ValueError:
                    cfg = None
            st = self.__dict__["_lora"] = lora.LoraState(targets, self.device, cfg)
        return st

    def _lora_change(self, fn):
        """Run one change of adapter state.  The merge kernel writes the weights through raw pointers, so afterwards the captured
        graphs (a replay reads derived weight copies at fixed addresses and runs no Python) are dropped and the hoisted
        cross-attention k|v re-projected; the derived-weight caches of the written models are dropped by ``LoraState.merge``."""
        if self.__dict__.get("_live_jobs"):
            raise RuntimeError("LoRA state cannot change while generate_latents_interleaved has images in flight")
        with torch.cuda.device(self.device):
            out = fn(self._lora_state())
        self._runner.entries.clear()
        self._runner.new_image()
        return out

    @torch.no_grad()
    def load_lora(self, source, scale=1.0, name=None, text_encoder=True):
        """Merge a LoRA adapter (a ``*.safetensors`` file or a state dict; diffusers / PEFT, legacy diffusers and kohya key
        spellings, kohya SDXL files in SGM block names) into the UNet and -- with ``text.ClipTextEncoder`` encoders -- the CLIP
        weights, at ``scale``.  Every key must name a Linear / Conv2d weight of fitting shape or nothing is applied.
        ``text_encoder=False`` drops the text-encoder keys.  Several adapters add up, each weight rounded once from its pristine
        copy.  ControlNet weights are never touched.  Returns the adapter's name (default: the file's base name)."""
        return self._lora_change(lambda st: st.load(source, scale, name, text_encoder))[0]

    @torch.no_grad()
    def set_lora_scale(self, scale, name=None):
        """New scale for the adapter ``name`` (None: all of them): one table rewrite and one merge launch per touched model.
        Scale 0 gives the original weights back bit for bit."""
        self._lora_change(lambda st: st.set_scale(scale, name))

    @torch.no_grad()
    def unload_lora(self, name=None):
        """Remove the adapter ``name`` (None: all): the weights are re-merged from their pristine copies, which are freed for
        every tensor no remaining adapter touches."""
        if not self.loras:
            if name is not None:
                raise KeyError(f"no LoRA adapter named {name!r}; none is loaded")
            return
        self._lora_change(lambda st: st.unload(name))

    @property
    def loras(self):
        """[(name, scale, tensors touched)] in load order"""
        st = self.__dict__.get("_lora")
        return [] if st is None else st.listing()

    # ---- IP-Adapter image prompts ------------------------------------------------
    def _ip_change(self, fn):
        """One change of IP-Adapter state: the context grows or shrinks by the image tokens and the scale is a kernel argument a
        captured graph holds by value, so the graphs are dropped and the hoisted k|v re-projected, as ``_lora_change`` does."""
        if self.__dict__.get("_live_jobs"):
            raise RuntimeError("IP-Adapter state cannot change while generate_latents_interleaved has images in flight")
        with torch.cuda.device(self.device):
            out = fn()
        self._runner.entries.clear()
        self._runner.new_image()
        return out

    @staticmethod
    def _image_encoder_callable(image_encoder, device, plus=False):
        """``image_encoder`` of ``load_ip_adapter`` -> callable pixel_values [1,3,S,S] fp32 -> [1, clip_dim] embeddings (or None).
        ``plus``: a Plus adapter reads the vision model's penultimate hidden states [1, S, embed_dim] instead (section 32); a
        callable returns whatever its adapter needs."""
        if image_encoder is None:
            return None
        if isinstance(image_encoder, (str, bytes)) or hasattr(image_encoder, "__fspath__"):
            from transformers import CLIPVisionModelWithProjection    # the encoder stays a library model
            image_encoder = CLIPVisionModelWithProjection.from_pretrained(image_encoder, local_files_only=True)
        if isinstance(image_encoder, nn.Module) and hasattr(image_encoder, "config") and hasattr(image_encoder.config, "projection_dim"):
            model = image_encoder.to(device).eval()
            dt = next(model.parameters()).dtype
            if plus:
                return lambda pixels: model(pixel_values=pixels.to(dt), output_hidden_states=True).hidden_states[-2]
            return lambda pixels: model(pixel_values=pixels.to(dt)).image_embeds
        if not callable(image_encoder):
            raise ValueError("image_encoder must be a callable pixel_values -> embeds, a transformers.CLIPVisionModelWithProjection "
                             f"or a local directory of one, got {type(image_encoder).__name__}")
        return image_encoder

    def _ip_list(self):
        """the loaded adapters' pipeline-side state, in load order: [{"name", "encoder", "kind"}]"""
        st = self.__dict__.get("_ips")
        if st is None:      # (a pipeline that only ever carried the single-adapter state)
            one = self.__dict__.get("_ip")
            return [dict(one, kind=one.get("kind", "base"))] if one else []
        return st

    def _ip_set(self, entries):
        self._ips = list(entries)
        self._ip = self._ips[0] if self._ips else None

    @torch.no_grad()
    def load_ip_adapter(self, source, scale=1.0, image_encoder=None, *, add=False):
        """Install an IP-Adapter (``read_ip_adapter``'s sources) into the UNet's cross attentions at ``scale``: a base adapter or a
        Plus adapter (Resampler image projection).  Every key must fit or nothing is installed
        (``UNet2DConditionModel.install_ip_adapter``).  ``image_encoder``: what turns ``ip_adapter_image`` into what the adapter
        reads -- a callable pixel_values -> embeddings (base: [1, clip_dim]; Plus: the penultimate hidden states [1, S, embed_dim]),
        a ``transformers.CLIPVisionModelWithProjection`` or a local directory of one; without it only ``ip_adapter_image_embeds``
        can be given.  ``add=False`` replaces whatever is installed; ``add=True`` appends behind it, up to four adapters -- their
        image tokens follow the text tokens in load order and every run keyword takes one entry per adapter.  Returns its name."""
        if not hasattr(self.unet, "install_ip_adapter"):
            raise ValueError(f"this pipeline's UNet ({type(self.unet).__name__}) cannot carry an IP-Adapter")
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"IP-Adapter scale must be finite, got {scale}")
        state, name = read_ip_adapter(source)
        kind = "plus" if "image_proj.latents" in state else "base"
        enc = self._image_encoder_callable(image_encoder, self.device, plus=kind == "plus")
        held = self._ip_list() if add else []

        def change():
            self.unet.install_ip_adapter(state, add=bool(add and held))
            if held:
                self.unet.ip_scales = self.unet.ip_scales[:-1] + [scale]
            else:
                self.unet.ip_scale = scale
            self.unet = self._model_layout(self.unet)
            self._ip_set(held + [{"name": name, "encoder": enc, "kind": kind}])
        self._ip_change(change)
        return name

    def set_ip_adapter_scale(self, scale, name=None):
        """New weight(s) of the image prompt(s): a float (for the adapter ``name``, or for every adapter) or a list of one float per
        adapter.  0 = the text-only result, bit for bit where a fused kernel runs.  With two or more adapters the weights are
        device data every attention reads when it runs: the captured graphs stay and replay with the new weights.  With one
        adapter the scale is a kernel argument, and the graphs are captured again, as before."""
        ips = self._ip_list()
        if not ips:
            raise ValueError("no IP-Adapter is loaded")
        if isinstance(scale, (list, tuple)):
            if name is not None or len(scale) != len(ips):
                raise ValueError(f"{len(ips)} IP-Adapter(s) are loaded: a list of scales has one float per adapter (and no name), got "
                                 f"{len(scale)}")
            scales = [float(s) for s in scale]
        elif name is None:
            scales = [float(scale)] * len(ips)
        else:
            names = [st["name"] for st in ips]
            if name not in names:
                raise ValueError(f"no IP-Adapter named {name!r} is loaded (loaded: {names})")
            scales = list(self.unet.ip_scales)
            scales[names.index(name)] = float(scale)
        if not all(math.isfinite(s) for s in scales):
            raise ValueError(f"IP-Adapter scales must be finite, got {scales}")
        if len(ips) == 1:
            def change():
                self.unet.ip_scale = scales[0]
            self._ip_change(change)
            return
        if self.__dict__.get("_live_jobs"):
            raise RuntimeError("IP-Adapter state cannot change while generate_latents_interleaved has images in flight")
        with torch.cuda.device(self.device):
            self.unet.ip_scales = scales       # one copy into the device weights; every captured graph reads them when it replays

    def unload_ip_adapter(self, name=None):
        """remove the adapter ``name`` (the others keep their order and scales) or, without a name, all of them"""
        ips = self._ip_list()
        if not ips:
            return
        if name is not None:
            names = [st["name"] for st in ips]
            if name not in names:
                raise ValueError(f"no IP-Adapter named {name!r} is loaded (loaded: {names})")
            keep = [st for k, st in enumerate(ips) if k != names.index(name)]
        else:
            keep = []

        def change():
            if name is None or not keep:
                self.unet.remove_ip_adapter()
            else:
                self.unet.remove_ip_adapter(names.index(name))
            self._ip_set(keep)
        self._ip_change(change)

    @property
    def ip_adapter(self):
        """None | (name, scale, image tokens) of the first adapter"""
        ips = self._ip_list()
        if not ips:
            return None
        if len(ips) == 1:
            return (ips[0]["name"], self.unet.ip_scale, self.unet.ip_tokens)
        kind, tokens, scale = self.unet.ip_adapters[0]
        return (ips[0]["name"], scale, tokens)

    @property
    def ip_adapters(self):
        """[(name, scale, image tokens, "base" | "plus")] in load order"""
        ips = self._ip_list()
        if not ips or not hasattr(self.unet, "ip_adapters"):
            return []
        return [(st["name"], scale, tokens, kind) for st, (kind, tokens, scale) in zip(ips, self.unet.ip_adapters)]

    def _check_ip_adapter(self, ip_adapter_image=None, ip_adapter_image_embeds=None, ip_adapter_negative_image_embeds=None):
        ips = self._ip_list()
        return check_ip_adapter_arguments([st["kind"] for st in ips], [st["encoder"] is not None for st in ips], ip_adapter_image,
                                          ip_adapter_image_embeds, ip_adapter_negative_image_embeds)

    def _clip_pixels(self, image, size=224):
        """``ip_adapter_image`` -> CLIPImageProcessor's pixel_values [1,3,size,size] fp32, on the device: one upload, Pillow's
        bicubic resize of the shortest edge to ``size`` (``ops.resize_u8``), then centre crop and normalise in one launch."""
        u8 = self._u8_image(image, 3, "ip_adapter_image")
        if isinstance(u8, np.ndarray):
            u8 = torch.from_numpy(np.ascontiguousarray(u8))
        u8 = u8.to(self.device).contiguous()
        H, W = int(u8.shape[0]), int(u8.shape[1])
        new = ops.clip_resize_size(H, W, size)
        if not all(1 <= n <= ops.RESIZE_MAX_DIM for n in (H, W) + new):
            raise ValueError(f"ip_adapter_image: cannot resize {(H, W)} to {new} (sides up to {ops.RESIZE_MAX_DIM})")
        if new != (H, W):
            u8 = ops.resize_u8(u8, new, "bicubic")
        return ops.u8_to_clip_input(u8, size)

    def _ip_tokens(self, B, ip_adapter_image=None, ip_adapter_image_embeds=None, ip_adapter_negative_image_embeds=None):
        """-> (unconditional, conditional) image tokens [B, sum Ni, cross_dim], the adapters' tokens side by side in load order.
        Base adapter: the projection of a zero embedding (or of the negative embeddings given) and of the picture's.  Plus adapter:
        the Resampler of the encoder's output for an all-zero picture (or of the negative embeddings) and of the picture's."""
        ips = self._ip_list()
        A = len(ips)
        if ip_adapter_image is not None:
            images, embeds, neg = ip_adapter_entries(ip_adapter_image, A, "ip_adapter_image"), [None] * A, [None] * A
        else:
            images, embeds = [None] * A, ip_adapter_entries(ip_adapter_image_embeds, A, "ip_adapter_image_embeds")
            neg = ([None] * A if ip_adapter_negative_image_embeds is None
                   else ip_adapter_entries(ip_adapter_negative_image_embeds, A, "ip_adapter_negative_image_embeds"))
        uns, cos = [], []
        for a, st in enumerate(ips):
            rank, width = self.unet.ip_embed_shape(a)
            e, n = embeds[a], neg[a]
            if images[a] is not None:
                pixels = self._clip_pixels(images[a])
                e = st["encoder"](pixels)
                if st["kind"] == "plus":
                    n = st["encoder"](torch.zeros_like(pixels))    # the published pipeline's unconditional image: all-zero pixel values
            e = torch.as_tensor(e).to(self.device)
            if e.dim() != rank or e.shape[0] not in (1, B) or e.shape[-1] != width:
                want = f"[1 or {B}, {width}]" if rank == 2 else f"[1 or {B}, S, {width}]"
                raise ValueError(f"image embeddings must be {want}, got {tuple(e.shape)}")
            e = e.expand(B, *e.shape[1:])
            if n is None:
                n = torch.zeros_like(e)
            else:
                n = torch.as_tensor(n).to(self.device)
                if n.dim() != rank or n.shape[0] not in (1, B) or n.shape[1:] != e.shape[1:]:
                    raise ValueError(f"negative image embeddings must match the image embeddings {tuple(e.shape)}, got {tuple(n.shape)}")
                n = n.expand(B, *n.shape[1:])
            uns.append(self.unet.ip_image_tokens(n, a))
            cos.append(self.unet.ip_image_tokens(e, a))
        return (uns[0], cos[0]) if A == 1 else (torch.cat(uns, dim=1), torch.cat(cos, dim=1))

    @torch.no_grad()
    def get_text_embeds(self, prompt, min_chunks=None):
        """ED:254-265.  With no CLIP weights available the default is a deterministic synthetic embedding per prompt
        string (shape-compatible: (B,77,cross_attention_dim) and the pooled (B,projection_dim)); the synthetic embeddings are
        always 77 tokens, whatever the prompt's length.  ``min_chunks``: at least this many 77-token chunks from an encoder
        that encodes long prompts in chunks (one with a ``chunks`` method, text.ClipTextEncoder); any other injected callable
        is called as ``text_encoder(prompt)``."""
        if self.text_encoder is not None:
            if min_chunks is not None and hasattr(self.text_encoder, "chunks"):
                e, p = self.text_encoder(prompt, min_chunks=min_chunks)
            else:
                e, p = self.text_encoder(prompt)
            return e.to(self.device), p.to(self.device)
        cfg = self.unet.config
        D = getattr(cfg, "cross_attention_dim", 768)
        P = getattr(cfg, "pooled_projection_dim", None)
        embeds, pooled = [], []
        for s in ([prompt] if isinstance(prompt, str) else prompt):
            g = torch.Generator().manual_seed(host_rng.strip_seed("prompt", 0, 0, 0, s))
            e = torch.randn(1, 77, D, generator=g)
            embeds.append(e)
            pooled.append(torch.randn(1, P, generator=g) if P else e)
        return torch.cat(embeds).to(self.device), torch.cat(pooled).to(self.device)

    # ---- per-image setup ---------------------------------------------------------------------------
    def _dev_i32(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    def _plan(self, height, width):
        s = self.vae_scale_factor
        if height % s or width % s:
            raise ValueError(f"height {height} and Width {width} must be divisable by {s}")  # ED:200-201
        Hl, Wl = height // s, width // s
        h, w = self.get_downsample_size(height, width)
        vc = self.view_config
        P = _Plan()
        P.Hl, P.Wl, P.h, P.w = Hl, Wl, h, w
        P.pick = geometry.PickPlan(Hl, Wl, h, w)
        P.views = geometry.ViewPlan(Hl, Wl, vc["window_size"], vc["stride"], vc["context_size"])
        P.gpad = geometry.PadPlan(h, w, self.model_size)
        P.vpad = geometry.PadPlan(P.views.Sh, P.views.Sw, self.model_size)
        P.one_batch = (P.gpad.PH, P.gpad.PW) == (P.vpad.PH, P.vpad.PW)
        d = self._dev_i32
        P.src_row, P.src_col = d(P.pick.src_row), d(P.pick.src_col)
        P.inv_row, P.inv_col = d(P.pick.inv_row), d(P.pick.inv_col)
        P.up_row, P.up_col = d(P.pick.up_row), d(P.pick.up_col)
        P.down_row, P.down_col = d(P.pick.down_row), d(P.pick.down_col)
        P.win_y0, P.win_x0 = d(P.views.win_y0), d(P.views.win_x0)
        rb, rs, cb, cs = P.views.cover_tables(P.vpad.top, P.vpad.left)
        P.row_blk, P.row_src, P.col_blk, P.col_src = d(rb), d(rs), d(cb), d(cs)
        P.sampler = host_rng.PickSampler(P.pick.N)
        return P

    def _strip_chunk(self, Hs, Ws, T):
        """Timesteps per pad-strip VAE call: ~16 MiB of fp32 pixels, at most STRIP_CHUNK."""
        s = self.vae_scale_factor
        return max(1, min(T, STRIP_CHUNK, (16 << 20) // max(1, 3 * Hs * s * Ws * s * 4)))

    def _strip_group(self, Hs, Ws, chunk, n_units):
        """Units (of ``chunk`` timesteps) per VAE call when the strips are encoded narrowed (models.VAE_NARROW_CONSTANT), else 0.  A narrowed
        call is several times smaller than the full one, and a single unit would leave the convolutions of the last level with a
        fraction of a round of tiles; so a rank puts as many of its units into one call as fit _strip_chunk's pixel budget counted in
        NARROWED pixels, spread evenly over its calls.  The figure depends on the pool and the rank count alone, so every call of a
        rank count has one batch (the last call repeats a unit) and MIOpen sees one shape per rank count."""
        plan = getattr(self.vae, "constant_plan", None)
        if plan is None or not hasattr(self.vae, "encode_constant"):
            return 0
        s = self.vae_scale_factor
        py, px = plan(Hs * s, Ws * s)
        if py is None and px is None:
            return 0
        Hn, Wn = (Hs if py is None else py.keep), (Ws if px is None else px.keep)
        fit = max(1, (16 << 20) // max(1, chunk * 3 * Hn * s * Wn * s * 4))
        per_rank = -(-n_units // (self.sharder.world_size if self.sharder.exchange else 1))
        return -(-per_rank // -(-per_rank // fit))

    def strip_pools(self, pad, T):
        """-> {(Hs, Ws, chunk): [strip indices]}: the strips of one PadPlan whose encodes share a call shape.  Each pool is
        ONE sharded unit list, i.e. one ``sharder.run`` (one exchange when sharded) per pool and image."""
        pools = {}
        for k, (dim, side_id, Hs, Ws, y0, x0) in enumerate(pad.strips):
            pools.setdefault((Hs, Ws, self._strip_chunk(Hs, Ws, T)), []).append(k)
        return pools

    @torch.no_grad()
    def _strip_frames(self, pad, timesteps, C):
        """All noised-background frames [T,C,PH,PW] of one PadPlan (ED:327-391), computed once per image instead of
        2 VAE encodes per global UNet call (the reference's TODO at ED:340).  Contents depend only on
        (dim, side, size, t); the draws come from md5-seeded private generators (host_rng.strip_draws).
        (Overlapping these encodes with the loop on a side stream was measured in round 2 -- 12.73 vs 12.79 s per image,
        the UNet already saturates the chip -- and removed.)"""
        T = len(timesteps)
        if not pad.padded:
            return None
        key = (pad.h, pad.w, pad.d, C, tuple(int(t) for t in timesteps))
        if self.cache_backgrounds and key in self._frame_cache:
            return self._frame_cache[key]
        dev = self.device
        frames = torch.zeros(T, C, pad.PH, pad.PW, device=dev, dtype=torch.float32)
        sf = self.vae.config.scaling_factor
        s = self.vae_scale_factor
        vae_dtype = next(self.vae.parameters()).dtype
        coef_host = torch.tensor([self.scheduler.add_noise_coefficients(t) for t in timesteps], dtype=torch.float32)
        plans = []
        for (dim, side_id, Hs, Ws, y0, x0) in pad.strips:
            draws = [host_rng.strip_draws(dim, side_id, Hs, Ws, t, C) for t in timesteps]
            # The unit of work is one VAE call over ``chunk`` consecutive timesteps, and EVERY call has exactly that
            # batch (the last chunk repeats the final timestep): the convolution shapes MIOpen sees are then the same on
            # 1, 2, 4 or 8 ranks -- for a shape its find-db has no record of, MIOpen runs a full find on first use (30-130 s
            # per process), which is what round 2's per-rank timestep split (25 -> 21+4 / 13,12 / 7,6 per call) would have
            # paid on the first real multi-GPU run.  ~16 MiB of fp32 pixels per call, at most STRIP_CHUNK timesteps so that a 50-step
            # schedule still splits into >= 10 units for 8 ranks.
            chunk = self._strip_chunk(Hs, Ws, T)
            plans.append((Hs, Ws, y0, x0, chunk, torch.cat([dr[0] for dr in draws]), torch.cat([dr[1] for dr in draws]),
                          torch.cat([dr[2] for dr in draws])))
        coef = coef_host.to(dev)
        # Strips of the same size (the two strips of a padded axis, unless the pad is odd) form ONE pool of units: 2 x 10
        # units on 8 ranks split 3,3,3,3,2,2,2,2 instead of 2 x (2,2,1,1,1,1,1,1) -- 15 % of the encodes on the busiest rank
        # instead of 20 % -- and one exchange per pool instead of one per strip.
        pools = self.strip_pools(pad, T)
        for (Hs, Ws, chunk), members in pools.items():
            n_units = -(-T // chunk)
            # draws of the pool's strips back to back: row p*T + t = strip p of the pool at timestep index t
            colour = torch.cat([plans[k][5] for k in members]).to(dev)
            post = torch.cat([plans[k][6] for k in members]).to(dev)
            fwd = torch.cat([plans[k][7] for k in members]).to(dev)
            # unit (p, u) covers timesteps u*chunk .. u*chunk+chunk-1 of strip p, clamped to T-1 (repeats dropped below)
            t_idx = torch.arange(n_units * chunk, device=dev).clamp_(max=T - 1).view(n_units, chunk)
            sel_all = torch.cat([t_idx + p * T for p in range(len(members))])          # [P * n_units, chunk] draw rows
            t_all = t_idx.repeat(len(members), 1)                                      # ... and their timestep indices

            group = self._strip_group(Hs, Ws, chunk, sel_all.shape[0])

            def encode(sel_rows, _a, _b, _c, t_rows):
                """Noised strips of the units ``sel_rows`` [n, chunk] (units are sharded over ranks like model rows)."""
                outs = []
                if group:
                    # narrowed encodes, ``group`` units per VAE call (the last call is filled up with its final unit); the posterior and
                    # the forward noise are applied to the expanded moments, per element as below
                    n = sel_rows.shape[0]
                    for a in range(0, n, group):
                        pick = torch.arange(a, a + group, device=sel_rows.device).clamp_(max=n - 1)
                        sel, tt = sel_rows[pick].reshape(-1), t_rows[pick].reshape(-1)
                        dist = self.vae.encode_constant(colour[sel].to(vae_dtype), Hs * s, Ws * s).latent_dist
                        enc = (dist.mean.float() + dist.std.float() * post[sel]) * sf
                        cf = coef[tt]
                        out = cf[:, 0].view(-1, 1, 1, 1) * enc + cf[:, 1].view(-1, 1, 1, 1) * fwd[sel]
                        outs.append(out.view(group, chunk, *out.shape[1:])[:min(group, n - a)])
                    return torch.cat(outs)
                for sel, tt in zip(sel_rows, t_rows):
                    img = colour[sel][:, :, None, None].expand(chunk, 3, Hs * s, Ws * s).contiguous().to(vae_dtype)
                    dist = self.vae.encode(img).latent_dist
                    enc = (dist.mean.float() + dist.std.float() * post[sel]) * sf
                    cf = coef[tt]
                    outs.append(cf[:, 0].view(-1, 1, 1, 1) * enc + cf[:, 1].view(-1, 1, 1, 1) * fwd[sel])
                return torch.stack(outs)

            strips = self.sharder.run(encode, sel_all, None, None, None, t_all, out_like=((chunk, C, Hs, Ws), torch.float32))
            strips = strips.reshape(len(members), n_units * chunk, C, Hs, Ws)
            for p, k in enumerate(members):
                y0, x0 = plans[k][2], plans[k][3]
                frames[:, :, y0:y0 + Hs, x0:x0 + Ws] = strips[p, :T]
        if self.cache_backgrounds:
            self._frame_cache[key] = frames
        return frames

    def _embed_rows(self, K, V, un, co, pun, pco):
        """Text rows for one fused model batch: K x [uncond(B), cond(B)] then V x uncond(B)  (ED:436-438, 846-847).  With regional
        prompts ``co`` / ``pco`` are lists of the P conditional embeddings (base prompt first): K x [uncond, cond_0 .. cond_{P-1}]."""
        dt = self.model_dtype
        cos, pcos = (list(co), list(pco)) if isinstance(co, (list, tuple)) else ([co], [pco])
        text = torch.cat([un, *cos] * K + [un] * V).to(dt).contiguous()
        pooled = torch.cat([pun, *pcos] * K + [pun] * V).to(dt).contiguous()
        return text, pooled

    # ---- model boundary ----------------------------------------------------------------------------
    # The cross-attention k / v of the text rows are the same in every forward of an image: computed once per image and batch
    # shape, outside the hipGraph (models.UNet2DConditionModel.cross_attention_kv; 70 projections per SDXL forward otherwise)
    TEXT_KV_ONCE = True

    def _text_kv(self, txt, into=None):
        """GraphedForward's ``prepare``: {"unet": {...}, "controlnet": {...}} of precomputed cross-attention k|v tensors for
        the text rows ``txt``, or None for models that do not offer it (injected stand-ins) / when switched off."""
        if not self.TEXT_KV_ONCE or not hasattr(self.unet, "cross_attention_kv"):
            return None
        out = {} if into is None else into
        # a part that is missing from ``into`` (a ControlNet attached after this batch shape was captured) is allocated here;
        # the captured graph cannot read it, but the runner's entries are dropped when the ControlNet changes (set_controlnet)
        out["unet"] = self.unet.cross_attention_kv(txt, out.get("unet"))
        if self.controlnet is not None and hasattr(self.controlnet, "cross_attention_kv"):
            out["controlnet"] = self.controlnet.cross_attention_kv(self._text_part(txt), out.get("controlnet"))
            if len(self.controlnets) > 1:  # prepared per net, open or closed at this step (section 31)
                more = out.get("controlnets_more") or [None] * (len(self.controlnets) - 1)
                out["controlnets_more"] = [cn.cross_attention_kv(self._text_part(txt), m) for cn, m in zip(self.controlnets[1:], more)]
        return out

    def _text_part(self, txt):
        """The rows a ControlNet is handed: the text tokens alone -- an IP-Adapter's image tokens are the UNet's (section 24)"""
        ni = getattr(self.unet, "ip_tokens", 0)
        return txt[:, :txt.shape[1] - ni].contiguous() if ni else txt

    def _forward_rows(self, x, t_dev, txt, pl, cond, text_kv=None, ctl=None, ipm=None):
        """ED:413-426 / EDC:476-518 for an arbitrary batch of d x d rows (this is what a hipGraph captures).  ``ctl`` = (active
        net indices, w f32 [rows, len(active)]): the Multi-ControlNet path -- ``cond`` holds the active
        nets' condition rows stacked along the channels, every active net returns its raw residuals and ONE
        ``ops.control_residuals`` launch hands sum_n w[:, n] * r_n to the UNet.  ``ipm`` = (m f32 [rows, A, S], PH, PW): the rows'
        IP-Adapter attention masks (section 33), handed to the UNet alone -- a ControlNet still sees text only."""
        kw, ckw = {}, {}
        if ipm is not None:
            kw["ip_masks"] = ipm
        if self.sd_version.startswith("XL"):
            ids = self._time_ids.to(txt.dtype).expand(x.shape[0], -1)
            kw["added_cond_kwargs"] = {"text_embeds": pl, "time_ids": ids}
        if text_kv is not None:
            kw["cross_kv"] = text_kv["unet"]
            ckw["cross_kv"] = text_kv.get("controlnet")
        if cond is not None and ctl is not None:
            from . import models
            active, w = ctl
            cn_kw = {k: v for k, v in kw.items() if k not in ("cross_kv", "ip_masks")}
            downs, mids = [], []
            for k, n in enumerate(active):
                cn, nkw = self.controlnets[n], {}
                if text_kv is not None and text_kv.get("controlnet") is not None:
                    nkw["cross_kv"] = text_kv["controlnet"] if n == 0 else text_kv["controlnets_more"][n - 1]
                if isinstance(cn, models.ControlNetModel):
                    nkw["raw_residuals"] = True
                c = cond if len(active) == 1 else cond[:, 3 * k:3 * k + 3].contiguous()
                down, mid = cn(x, t_dev, encoder_hidden_states=self._text_part(txt), controlnet_cond=c, conditioning_scale=1.0,
                               guess_mode=False, return_dict=False, **cn_kw, **nkw)
                downs.append(list(down))
                mids.append(mid)
            if isinstance(self.unet, models.UNet2DConditionModel):
                kw["control_residuals"] = (downs, mids, w)
            else:  # a stand-in UNet takes the sums through the keywords it knows: the same launch without skips
                sums = ops.control_residuals(None, [d + [m] for d, m in zip(downs, mids)], w)
                kw["down_block_additional_residuals"], kw["mid_block_additional_residual"] = sums[:-1], sums[-1]
        elif cond is not None:
            cn_kw = {k: v for k, v in kw.items() if k not in ("cross_kv", "ip_masks")}
            down, mid = self.controlnet(x, t_dev, encoder_hidden_states=self._text_part(txt), controlnet_cond=cond,
                                        conditioning_scale=self._cn_scale, guess_mode=False, return_dict=False, **cn_kw, **ckw)
            kw["down_block_additional_residuals"], kw["mid_block_additional_residual"] = down, mid
        return self.unet(x, t_dev, encoder_hidden_states=txt, **kw)["sample"].contiguous()

    def _run_model(self, x_rows, t_dev, text, pooled, cond_rows=None, fresh_side=False, ctl=None, ipm=None):
        """Rows are sharded across ranks (sharding.py); each rank's share runs as one (graph-replayed) forward.
        ``t_dev``: 0-d timestep shared by all rows, or one timestep per row (fused batches of several images).  ``ctl``
        (``_ModelCall.ctl``): its per-row weights shard with the rows, like a per-row timestep.  ``ipm`` (``_ModelCall.ipm``): the
        per-row mask buffer shards the same way."""
        if ipm is not None:
            per_row, active = t_dev.dim() != 0, None if ctl is None else ctl[0]

            def fn(x, txt, pl, cond, *more):
                more = list(more)
                t = more.pop(0) if per_row else t_dev
                c = None if active is None else (active, more.pop(0))
                return self._runner(x, t, txt, pl, cond, fresh_side, ctl=c, ipm=(more.pop(0), ipm[1], ipm[2]))
            return self.sharder.run(fn, x_rows, text, pooled, cond_rows, *((t_dev,) if per_row else ()),
                                    *(() if ctl is None else (ctl[1],)), ipm[0])
        if ctl is not None:
            active, per_row = ctl[0], t_dev.dim() != 0

            def fn(x, txt, pl, cond, *more):
                return self._runner(x, more[0] if per_row else t_dev, txt, pl, cond, fresh_side, ctl=(active, more[-1]))
            return self.sharder.run(fn, x_rows, text, pooled, cond_rows, *((t_dev,) if per_row else ()), ctl[1])
        if t_dev.dim() == 0:
            return self.sharder.run(lambda x, txt, pl, cond: self._runner(x, t_dev, txt, pl, cond, fresh_side),
                                    x_rows, text, pooled, cond_rows)
        return self.sharder.run(lambda x, txt, pl, cond, t: self._runner(x, t, txt, pl, cond, fresh_side),
                                x_rows, text, pooled, cond_rows, t_dev)

    # ---- one estimation phase (ED:1016-1035 or ED:1043-1056) ---------------------------------------
    def _phase_steps(self, P, x, ti, K, g, drop_p, emb, cond=None, direct=True, rrg_w=None, rrg_norm=0.0, frames=None,
                     rescale=None, extras=None, multistep=None, keep_scores=False, region_w=None, step_noise=None, ctl=None,
                     ip_masks=None):
        """Generator: pre-model glue -> ``yield _ModelCall`` (receives the model output rows) -> post-model glue;
        returns (prev, x0, info).  ``direct``: assemble straight into the hipGraph's static input (one image in flight,
        one rank); otherwise into a scratch batch the driver concatenates / the sharder slices.  ``rrg_w``: this is the
        last phase of a timestep with Reduced-Resolution Guidance active -- with FUSED_GLUE the epilogue then also
        produces info["x_next"] = prev + RRG term (ED:1061-1078).  ``rescale`` (a ``_Rescale``): the guided model output is
        std-rescaled before the DDIM update -- one moments reduction over the same rows, then the rescale-aware kernels;
        with ``rrg_w`` the reduced-resolution pair gets its own ratio (info["ratio_low"]).  ``extras`` = (extra [B,E,Hl,Wl],
        pad_value [E]) on a 9-channel inpainting UNet: the model rows carry C + E channels, the extra ones registered to each row's
        latent (``ops.assemble_rows_x``); everything after the model call is unchanged.  ``multistep`` (``_multistep_args``): the
        DPM-Solver++(2M) update of this timestep in the DDIM one's place, in the same launch; None launches what it always did.
        ``keep_scores``: info["direction"] / info["local"] are kept as ``verbose`` keeps them (the inputs of the score PCA maps).
        ``region_w`` (f32 [P,Hl,Wl]; regional prompts): a step holds 1 + P rows per sample and the class direction
        is the per-pixel weighted sum of the P directions -- ``ops.assemble_rows_n`` and the regional epilogue in the places of the
        plain launches; None launches what it always did.  ``step_noise`` (the step's c_n, section 29; None for a step that is not
        stochastic): the phase's latent-sized normal draw is made with the other host draws -- after the picks and the strip
        reseeds, where the reference's ``scheduler.step`` would draw -- and added by the step's own launch; with ``rrg_w`` the
        reduced-resolution step's draw, whose result the reference discards, only advances the generator.  ``ip_masks`` (f32
        [B,A,Hl,Wl]; IP-Adapter attention masks, section 33): one ``ops.ip_mask_rows`` launch beside the assemble launch forms the
        per-row masks of this model call from the same picks and windows, and the ``_ModelCall`` carries them; None launches what it
        always did."""
        ms_kw = {} if multistep is None else dict(multistep=multistep)
        B, C = x.shape[:2]
        CR = C if extras is None else C + extras[0].shape[1]  # channels of a model INPUT row
        dev, mdt = self.device, self.model_dtype
        copies = 2 if region_w is None else 1 + region_w.shape[0]  # rows per resampling step and sample
        assert region_w is None or extras is None
        n_g, n_v = copies * K * B, P.views.V * B
        # host draws first (they never wait for the GPU)
        h0 = time.perf_counter()
        idx_host = self._stager.host((K, P.pick.N), torch.uint8)
        stamp_host = self._stager.host((P.pick.N, 4), torch.int8)
        P.sampler.draw(K, drop_p, lambda: host_rng.replay_strip_reseeds(len(P.gpad.strips)), out=idx_host, stamp=stamp_host)
        self.host_s["picks"] += time.perf_counter() - h0
        stamp = self._stager.upload(stamp_host, dev)
        idx = self._stager.upload(idx_host, dev)
        # view batches as the reference forms them: only their pad-strip reseeds are observable (ED:830, 359)
        if P.vpad.strips:
            for _ in range(math.ceil(P.views.V / self.view_batch_size)):
                host_rng.replay_strip_reseeds(len(P.vpad.strips))
        if step_noise is not None:
            assert region_w is None
            ms_kw["noise"] = (step_noise, self._draw_step_noise(x.shape, None if rrg_w is None else (B, C, P.h, P.w)))
        gframes, vframes = frames if frames is not None else (self._gframes, self._vframes)
        gframe = None if gframes is None else gframes[ti]
        vframe = None if vframes is None else vframes[ti]
        low = torch.empty(K, B, C, P.h, P.w, device=dev, dtype=torch.float32)
        direct = direct and P.one_batch and self.sharder.world_size == 1
        if P.one_batch:
            shape = (n_g + n_v, CR, P.gpad.PH, P.gpad.PW)
            ipm_kw = {}
            if ip_masks is not None and direct:   # (the key of the static input: the buffer's shape, known before it is filled)
                S_m = ops.ip_mask_layout(P.gpad.PH, P.gpad.PW)[1]
                ipm_kw = dict(ipm=(torch.empty(n_g + n_v, ip_masks.shape[1], S_m, device="meta"), P.gpad.PH, P.gpad.PW))
            rows = (self._runner.input_rows(shape, mdt, dev, None if cond is None else cond[K], *emb[K],
                                            ctl=None if ctl is None else ctl[K], **ipm_kw) if direct
                    else torch.empty(shape, device=dev, dtype=mdt))
            g_rows, v_rows = rows[:n_g], rows[n_g:]
        else:
            g_rows = torch.empty(n_g, CR, P.gpad.PH, P.gpad.PW, device=dev, dtype=mdt)
            v_rows = torch.empty(n_v, CR, P.vpad.PH, P.vpad.PW, device=dev, dtype=mdt)
        if region_w is not None:
            if FUSED_GLUE:
                ops.assemble_rows_n(x, idx, P.src_row, P.src_col, g_rows, P.h, P.w, P.gpad.top, P.gpad.left, gframe, low,
                                    v_rows, P.win_y0, P.win_x0, P.views.Sh, P.views.Sw, P.vpad.top, P.vpad.left, vframe, copies)
            else:  # the pair rows as always, then every cond row a copy of the pair's
                pair = torch.empty(2 * K * B, C, P.gpad.PH, P.gpad.PW, device=dev, dtype=mdt)
                ops.pick_assemble(x, idx, P.src_row, P.src_col, pair, P.h, P.w, P.gpad.top, P.gpad.left, gframe, low)
                ops.gather_views(x, v_rows, P.win_y0, P.win_x0, P.views.Sh, P.views.Sw, P.vpad.top, P.vpad.left, vframe)
                g_rows.view(K, copies, B, C, P.gpad.PH, P.gpad.PW)[:] = pair.view(K, 2, B, C, P.gpad.PH, P.gpad.PW)[:, :1]
        elif extras is not None:
            if FUSED_GLUE:
                ops.assemble_rows_x(x, idx, P.src_row, P.src_col, g_rows, P.h, P.w, P.gpad.top, P.gpad.left, gframe, low,
                                    v_rows, P.win_y0, P.win_x0, P.views.Sh, P.views.Sw, P.vpad.top, P.vpad.left, vframe, *extras)
            else:
                self._assemble_unfused_x(P, x, idx, K, g_rows, v_rows, gframe, vframe, low, *extras)
        elif FUSED_GLUE:
            ops.assemble_rows(x, idx, P.src_row, P.src_col, g_rows, P.h, P.w, P.gpad.top, P.gpad.left, gframe, low,
                              v_rows, P.win_y0, P.win_x0, P.views.Sh, P.views.Sw, P.vpad.top, P.vpad.left, vframe)
        else:
            ops.pick_assemble(x, idx, P.src_row, P.src_col, g_rows, P.h, P.w, P.gpad.top, P.gpad.left, gframe, low)
            ops.gather_views(x, v_rows, P.win_y0, P.win_x0, P.views.Sh, P.views.Sw, P.vpad.top, P.vpad.left, vframe)
        ipm = ipm_g = ipm_v = None
        if ip_masks is not None:   # the rows' masks: the gather of the assemble launch applied to the masks, four levels, one launch
            pick_a = (idx, P.src_row, P.src_col, P.h, P.w, P.gpad.top, P.gpad.left)
            view_a = (P.win_y0, P.win_x0, P.views.Sh, P.views.Sw, P.vpad.top, P.vpad.left)
            if P.one_batch:
                ipm = (ops.ip_mask_rows(ip_masks, *pick_a, *view_a, P.gpad.PH, P.gpad.PW, copies), P.gpad.PH, P.gpad.PW)
            else:
                ipm_g = (ops.ip_mask_rows(ip_masks, *pick_a, None, None, 0, 0, 0, 0, P.gpad.PH, P.gpad.PW, copies), P.gpad.PH, P.gpad.PW)
                ipm_v = (ops.ip_mask_rows(ip_masks, None, None, None, 0, 0, 0, 0, *view_a, P.vpad.PH, P.vpad.PW, copies),
                         P.vpad.PH, P.vpad.PW)
        text, pooled = emb[K]
        t_dev = self._t_dev[ti]
        self.host_s["phase_total"] += time.perf_counter() - h0
        if P.one_batch:
            out = yield _ModelCall(rows, t_dev, text, pooled, None if cond is None else cond[K], direct,
                                   None if ctl is None else ctl[K], ipm)
            g_out, v_out = out[:n_g], out[n_g:]
        else:
            g_out = yield _ModelCall(g_rows, t_dev, text[:n_g].contiguous(), pooled[:n_g].contiguous(),
                                     None if cond is None else cond[K][0], ctl=None if ctl is None else ctl[K][0], ipm=ipm_g)
            g_out = g_out.clone()  # the two calls may share one graph output buffer when their shapes coincide
            v_out = yield _ModelCall(v_rows, t_dev, text[n_g:].contiguous(), pooled[n_g:].contiguous(),
                                     None if cond is None else cond[K][1], ctl=None if ctl is None else ctl[K][1], ipm=ipm_v)
        h0 = time.perf_counter()
        uncond_last = torch.empty(B, C, P.h, P.w, device=dev, dtype=torch.float32)
        low_dir = torch.empty(B, C, P.h, P.w, device=dev, dtype=torch.float32)
        prev, x0 = torch.empty_like(x), torch.empty_like(x)
        x_next, direction, local = None, None, None
        pt = self.scheduler.config.prediction_type
        ratio_low = rescale.ratio_low if rescale is not None and rrg_w is not None else None
        if FUSED_GLUE:
            keep = self.verbose or keep_scores  # the full-resolution direction / local score are only by-products for the image logs
            direction = torch.empty_like(x) if keep else None
            local = torch.empty_like(x) if keep else None
            x_next = torch.empty_like(x) if rrg_w is not None else None
            pick_t = (P.inv_row, P.inv_col, P.up_row, P.up_col, P.down_row, P.down_col)
            view_t = (P.row_blk, P.row_src, P.col_blk, P.col_src)
            rs_kw = {}
            rg_kw = {} if region_w is None else dict(region_w=region_w)
            if rescale is not None:
                ops.phase_moments(g_out, v_out, x.shape, stamp, pick_t, view_t, P.views.n_col_blocks,
                                  (P.gpad.top, P.gpad.left), K, P.h, P.w, np.float32(g), rescale.ratio, rescale.ws,
                                  ratio_low=ratio_low, **rg_kw)
                rs_kw = dict(ratio=rescale.ratio, ratio_low=ratio_low, guidance_rescale=rescale.gr)
            ops.phase_epilogue(g_out, v_out, x, stamp, pick_t, view_t, P.views.n_col_blocks,
                               (P.gpad.top, P.gpad.left), K, P.h, P.w, np.float32(g), self._step_coef[ti], prev, x0,
                               low_dir=low_dir, uncond_last=uncond_last, direction=direction, local=local, x_next=x_next,
                               low_latent=low[K - 1] if rrg_w is not None else None, rrg_norm=rrg_norm,
                               rrg_weight=0.0 if rrg_w is None else np.float32(rrg_w), prediction_type=pt, **rs_kw, **ms_kw,
                               **rg_kw)
        else:
            dirs = torch.empty(K, B, C, P.h, P.w, device=dev, dtype=torch.float32)
            direction = torch.empty_like(x)
            if region_w is None:
                ops.unpad_direction(g_out, dirs, uncond_last, P.gpad.top, P.gpad.left)
                ops.fill_directions(dirs, stamp, P.inv_row, P.inv_col, P.up_row, P.up_col, P.down_row, P.down_col, direction,
                                    low_dir)
            else:  # the separate kernels once per region on its (uncond, cond_p) pair rows, then the weighted sums
                n_p = copies - 1
                g6 = g_out.view(K, copies, B, C, P.gpad.PH, P.gpad.PW)
                full = torch.empty(n_p, *x.shape, device=dev, dtype=torch.float32)
                lows = torch.empty(n_p, B, C, P.h, P.w, device=dev, dtype=torch.float32)
                for p in range(n_p):
                    pair = g6[:, [0, 1 + p]].reshape(2 * K * B, C, P.gpad.PH, P.gpad.PW).contiguous()
                    ops.unpad_direction(pair, dirs, uncond_last, P.gpad.top, P.gpad.left)
                    ops.fill_directions(dirs, stamp, P.inv_row, P.inv_col, P.up_row, P.up_col, P.down_row, P.down_col, full[p],
                                        lows[p])
                ops.region_blend(full, region_w, direction)
                w_low = region_w[:, P.down_row.long()][:, :, P.down_col.long()].contiguous()  # low_dir samples (down_row, down_col)
                ops.region_blend(lows, w_low, low_dir)
            local = torch.empty_like(x)
            ops.scatter_centres(v_out, local, P.views.n_col_blocks, P.row_blk, P.row_src, P.col_blk, P.col_src)
            rs_kw = {}
            if rescale is not None:
                ops.guidance_moments(local, direction, np.float32(g), rescale.ratio, rescale.ws)
                if ratio_low is not None:  # the pair ops.rrg_update forms (in _program)
                    ops.guidance_moments(uncond_last, low_dir, np.float32(g), ratio_low, rescale.ws)
                rs_kw = dict(ratio=rescale.ratio, guidance_rescale=rescale.gr)
            ops.cfg_ddim_step(local, direction, x, prev, x0, np.float32(g), *self._step_coef[ti], prediction_type=pt, **rs_kw,
                              **ms_kw)
        self.host_s["phase_total"] += time.perf_counter() - h0
        info = {"low_latent": low[K - 1], "uncond_score": uncond_last, "low_direction": low_dir,
                "direction": direction, "local": local, "init_low": low[0], "x_next": x_next, "ratio_low": ratio_low}
        return prev, x0, info

    def _draw_step_noise(self, shape, discarded=None):
        """The noise of one stochastic step (section 29): ``torch.randn(shape)`` on the host generator, staged through pinned memory
        like ``_undo``'s; then, for ``discarded`` (the reduced-resolution step inside RRG), a draw of that shape whose values nobody
        reads -- no staging, no upload."""
        h0 = time.perf_counter()
        host = self._stager.host(tuple(shape), torch.float32)
        self.host_s["stager_wait"] += time.perf_counter() - h0
        host_rng.draw_noise_into(host[None])
        if discarded is not None:
            host_rng.skip_noise(discarded)
        self.host_s["noise"] += time.perf_counter() - h0
        return self._stager.upload(host, self.device)

    def _step_noise(self, t):
        """``step_noise`` of ``_phase_steps`` at timestep ``t``: the schedule's noise coefficient, None where the step is not
        stochastic (c_n == 0.0: nothing is drawn and the deterministic kernels run)."""
        c_n = self.scheduler.noise_coefficient(t)
        return c_n if c_n != 0.0 else None

    def _multistep_args(self, t, hist, is_last):
        """The ``multistep`` argument of the step kernels at timestep ``t``: None under a DDIM scheduler; under a
        ``DPMSolverSchedule`` (c_x, b, half_b, r_inv, x0_hist) with ``hist`` = (x0 of the previous timestep, that timestep) or None,
        the history passed only where the schedule makes the step second order."""
        if not isinstance(self.scheduler, DPMSolverSchedule):
            return None
        coef = self.scheduler.multistep_coefficients(t, None if hist is None else hist[1], is_last)
        return coef[2:] + (hist[0] if coef[5] != 0.0 else None,)

    def _drive(self, program):
        """Run one program alone: every model call is its own (graph-replayed, row-sharded) forward."""
        try:
            call = next(program)
            while True:
                call = program.send(self._run_model(call.rows, call.t, call.text, call.pooled, call.cond, ctl=call.ctl,
                                                    ipm=call.ipm))
        except StopIteration as stop:
            return stop.value

    def _undo(self, x, ti_next):
        """ED:692-704; noise drawn on the host generator in the reference's order, staged through pinned memory."""
        n_sub = self._undo_coef.shape[1]
        h0 = time.perf_counter()
        host = self._stager.host((n_sub,) + tuple(x.shape), torch.float32)
        self.host_s["stager_wait"] += time.perf_counter() - h0
        host_rng.draw_noise_into(host)
        self.host_s["noise"] += time.perf_counter() - h0
        noise = self._stager.upload(host, self.device)
        out = torch.empty_like(x)
        ops.undo_step(x, noise, self._undo_coef[ti_next], out)
        return out

    # ---- ControlNet condition rows (EDC:457-461, 932-949) -- constant over the whole image ------------
    def _control_rows(self, S, condition_image, B, ckw):
        """Multi-ControlNet (section 31): ``_condition_rows`` per net, then -> ``at(step)``: (cond, ctl) of the executed step --
        cond = {K: the rows of the nets open at that step stacked along the channels}, ctl = {K: (their indices, per-row weights
        f32 [rows, n_open])}; (None, None) when every net is closed (the step is a plain UNet forward).  Steps with equal
        weights share their tensors."""
        imgs = list(condition_image) if isinstance(condition_image, (list, tuple)) else [condition_image]
        N = len(self.controlnets)
        if len(imgs) != N:
            raise ValueError(f"{len(imgs)} condition image{'s' if len(imgs) != 1 else ''} for {N} ControlNet{'s' if N != 1 else ''}")
        per_net = [self._condition_rows(S.P, im, B, S.Ks, **ckw) for im in imgs]
        cache = {}

        def build(weights):
            active = tuple(n for n, v in enumerate(weights) if v != 0)
            if not active:
                return None, None
            wv = torch.tensor([[float(weights[n]) for n in active]], dtype=torch.float32).to(self.device)
            cond, ctl = {}, {}
            for K in S.Ks:
                parts = [per_net[n][K] for n in active]
                if S.P.one_batch:
                    cond[K] = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1).contiguous()
                    ctl[K] = (active, wv.expand(cond[K].shape[0], -1).contiguous())
                else:
                    cond[K] = tuple(parts[0][j] if len(parts) == 1 else torch.cat([q[j] for q in parts], dim=1).contiguous()
                                    for j in (0, 1))
                    ctl[K] = tuple((active, wv.expand(c.shape[0], -1).contiguous()) for c in cond[K])
            return cond, ctl

        def at(step):
            weights = S.control[step]
            if weights not in cache:
                cache[weights] = build(weights)
            return cache[weights]
        return at

    def _condition_rows(self, P, cond_img, B, Ks, copies=2):
        s = self.vae_scale_factor
        cond_img = cond_img.to(self.device, torch.float32).contiguous()
        assert cond_img.shape[0] == 1 and tuple(cond_img.shape[-2:]) == (P.h * s, P.w * s), \
            "condition image must be (1,3,8h,8w) at the reduced resolution (EDC:1183-1193)"
        mdt = next(self.controlnet.parameters()).dtype
        # global rows: zero pad in pixel space
        gp = P.gpad
        rows_g = np.full((1, gp.PH * s), -1, dtype=np.int32)
        cols_g = np.full((1, gp.PW * s), -1, dtype=np.int32)
        rows_g[0, gp.top * s:(gp.top + P.h) * s] = np.arange(P.h * s)
        cols_g[0, gp.left * s:(gp.left + P.w) * s] = np.arange(P.w * s)
        g_img = torch.empty(1, 3, gp.PH * s, gp.PW * s, device=self.device, dtype=mdt)
        ops.gather2d(cond_img, g_img, self._dev_i32([0]), self._dev_i32(rows_g), self._dev_i32(cols_g))
        # view rows: nearest upsample to full resolution (index map), crop per view at pixel scale, zero pad
        up_r = geometry.nearest_index_map(P.h * s, P.Hl * s)
        up_c = geometry.nearest_index_map(P.w * s, P.Wl * s)
        vp, V = P.vpad, P.views.V
        n = (self.view_config["context_size"] * 8) // 2
        rows_v = np.full((V, vp.PH * s), -1, dtype=np.int32)
        cols_v = np.full((V, vp.PW * s), -1, dtype=np.int32)
        for v, (h0, h1, w0, w1) in enumerate(P.views.views):
            bt, at = geometry.axis_context(h0 * 8, h1 * 8, P.Hl * s, n)
            bl, al = geometry.axis_context(w0 * 8, w1 * 8, P.Wl * s, n)
            rr = up_r[h0 * 8 - bt: h1 * 8 + at]
            cc = up_c[w0 * 8 - bl: w1 * 8 + al]
            rows_v[v, vp.top * s: vp.top * s + len(rr)] = rr
            cols_v[v, vp.left * s: vp.left * s + len(cc)] = cc
        v_img = torch.empty(V, 3, vp.PH * s, vp.PW * s, device=self.device, dtype=mdt)
        ops.gather2d(cond_img, v_img, self._dev_i32([0] * V), self._dev_i32(rows_v), self._dev_i32(cols_v))
        out = {}
        for K in Ks:
            g_part = g_img.expand(copies * K * B, -1, -1, -1)
            v_part = v_img.repeat_interleave(B, dim=0)
            out[K] = torch.cat([g_part, v_part]).contiguous() if P.one_batch else (g_part.contiguous(), v_part.contiguous())
        return out

    # ---- image-to-image / inpainting inputs ------------------------------------
    def _u8_image(self, image, channels, what):
        """A PIL image or a uint8 array / tensor [H,W,channels] ([H,W] too for one channel) -> contiguous uint8 numpy array or
        tensor of exactly that rank-3 shape, else None (not an 8-bit picture)."""
        if hasattr(image, "convert"):
            mode = "RGB" if channels == 3 else "L"
            image = np.array(image if image.mode == mode else image.convert(mode))
        if not isinstance(image, (np.ndarray, torch.Tensor)) or image.dtype not in (np.uint8, torch.uint8):
            return None
        if image.ndim == 2 and channels == 1:
            image = image[:, :, None]
        if image.ndim != 3 or image.shape[2] != channels:
            raise ValueError(f"{what}: an 8-bit picture must be [H,W,{channels}], got {tuple(image.shape)}")
        return image

    def _init_pixels(self, image, height, width):
        """``init_image`` -> (the VAE encoder's input (1|B,3,height,width) in [-1, 1] in the VAE's dtype, the (H, W) of an 8-bit
        source that was resized or None).  An 8-bit picture of another size is resized with Pillow's Lanczos filter on the
        device (``ops.resize_u8``: ``VaeImageProcessor``'s default, Pillow's bytes) and converted by ``ops.u8_to_vae_input``."""
        vdt = next(self.vae.parameters()).dtype
        u8 = self._u8_image(image, 3, "init_image")
        if u8 is None:
            if not isinstance(image, torch.Tensor) or not image.is_floating_point():
                raise ValueError("init_image must be an RGB PIL image, a uint8 [H,W,3] array / tensor or a float tensor "
                                 f"(1|B,3,height,width) in [0,1], got {type(image).__name__}")
            t = image[None] if image.dim() == 3 else image
            if t.dim() != 4 or tuple(t.shape[1:]) != (3, height, width):
                raise ValueError(f"a float init_image must already be (1|B,3,{height},{width}), got {tuple(image.shape)}")
            self.last_init_pixels = None
            return (2.0 * t.to(self.device, torch.float32) - 1.0).to(vdt).contiguous(), None
        if isinstance(u8, np.ndarray):
            u8 = torch.from_numpy(np.ascontiguousarray(u8))
        u8 = u8.to(self.device).contiguous()
        src = tuple(u8.shape[:2])
        if src != (height, width):
            if not all(1 <= n <= ops.RESIZE_MAX_DIM for n in src + (height, width)):
                raise ValueError(f"init_image: cannot resize {src} to {(height, width)} (sides up to {ops.RESIZE_MAX_DIM})")
            u8 = ops.resize_u8(u8, (height, width), "lanczos")
        self.last_init_pixels = u8
        return ops.u8_to_vae_input(u8, vdt), (src if src != (height, width) else None)

    def _latent_mask(self, mask, height, width, resized_from=None, mask_blur=0.0, graded=False, raw=None):
        """``mask_image`` -> uint8 (Hl, Wl) on the device, 1 = repaint, 0 = keep; with ``graded`` the level map instead, the
        sampled byte itself (a uint8 tensor at latent resolution is the level map, a bool one 0 / 255).  The 8-bit picture mask
        at height x width, blurred by ``ops.gaussian_blur_u8`` when ``mask_blur`` > 0 (Pillow's ``GaussianBlur`` bytes), is
        what gets sampled, and stays on the device as ``last_pixel_mask``.  A bool / uint8 tensor that is already
        (Hl, Wl) is taken as the latent mask (non-zero = repaint); an 8-bit picture (L PIL image, uint8 [H,W] / [H,W,1]) of
        height x width is sampled at the top-left pixel of every latent cell and compared with 128 (torch's nearest
        ``interpolate`` of the mask binarised at 0.5).  A picture that has the size ``resized_from`` of an init image that
        was resized is first resized on the HOST with PIL's NEAREST filter -- a rare path, one pass over the mask's bytes.
        ``raw``: a list that receives the picture mask at height x width BEFORE the blur (what a 9-channel UNet's masked image is
        blanked through)."""
        s = self.vae_scale_factor
        Hl, Wl = height // s, width // s
        self.last_pixel_mask = None
        if isinstance(mask, torch.Tensor) and mask.dtype in (torch.bool, torch.uint8) and tuple(mask.shape) == (Hl, Wl):
            if mask_blur > 0:
                raise ValueError("mask_blur needs an 8-bit picture mask, not a tensor at latent resolution")
            mask = mask.to(self.device).contiguous()
            return ops.mask_levels_to_latent(mask, 1) if graded else ops.mask_to_latent(mask, 1)
        u8 = self._u8_image(mask, 1, "mask_image")
        if u8 is None:
            raise ValueError("mask_image must be an L PIL image, a uint8 [H,W] / [H,W,1] array / tensor of the image's size, or a "
                             f"bool / uint8 tensor ({Hl},{Wl}); got {type(mask).__name__} {getattr(mask, 'dtype', '')}")
        size = tuple(u8.shape[:2])
        if size != (height, width):
            if resized_from is None or size != tuple(resized_from):
                raise ValueError(f"mask_image is {size}; it must be {(height, width)}"
                                 + ("" if resized_from is None else f" or the init image's {tuple(resized_from)}"))
            from PIL import Image
            host = u8.cpu().numpy() if isinstance(u8, torch.Tensor) else u8
            u8 = np.array(Image.fromarray(np.ascontiguousarray(host[:, :, 0])).resize((width, height), resample=Image.NEAREST))
        if isinstance(u8, np.ndarray):
            u8 = torch.from_numpy(np.ascontiguousarray(u8))
        u8 = u8.to(self.device).contiguous()
        u8 = u8.view(u8.shape[0], u8.shape[1])       # [H,W,1] from ``_u8_image``, [H,W] from the host resize
        if raw is not None:
            raw.append(u8)
        if mask_blur > 0:
            u8 = ops.gaussian_blur_u8(u8, mask_blur)
        self.last_pixel_mask = u8
        return ops.mask_levels_to_latent(u8, s) if graded else ops.mask_to_latent(u8, s)

    def _img2img_start(self, S, B, init_image, mask_image, mask_blur=0.0, graded=False):
        """The initial latent of an image-to-image run: encode, sample the posterior, noise to the first executed timestep.
        Host RNG order: posterior noise, then the initial noise, both (B,C,Hl,Wl) fp32.  -> (x, z0, noise, latent mask | None)
        On a 9-channel UNet (``S.inpaint9``) the unblurred picture mask is kept as ``self._raw_pixel_mask`` for
        ``_inpaint9_extras``, which draws next."""
        P = S.P
        raw = [] if getattr(S, "inpaint9", False) else None
        s = self.vae_scale_factor
        pix, resized_from = self._init_pixels(init_image, P.Hl * s, P.Wl * s)
        if pix.shape[0] not in (1, B):
            raise ValueError(f"init_image holds {pix.shape[0]} images for {B} prompts (1 or {B})")
        mask = None
        self.last_pixel_mask = None
        if mask_image is not None:
            mask = self._latent_mask(mask_image, P.Hl * s, P.Wl * s, resized_from, mask_blur, graded, raw)
        self._raw_pixel_mask = raw[0] if raw else None
        dist = self.vae.encode(pix).latent_dist
        shape = (B, S.C, P.Hl, P.Wl)
        if tuple(dist.mean.shape[1:]) != shape[1:]:
            raise ValueError(f"the VAE encodes the init image to {tuple(dist.mean.shape)}, the loop runs on {shape}")
        mean, std = (t.expand(shape).contiguous() for t in (dist.mean, dist.std))
        h0 = time.perf_counter()
        eps_host = self._stager.host(shape, torch.float32)
        eps_host.normal_()
        x_host = self._stager.host(shape, torch.float32)
        x_host.normal_()
        self.host_s["noise"] += time.perf_counter() - h0
        eps = self._stager.upload(eps_host, self.device)
        noise = self._stager.upload(x_host, self.device)
        a, b = self.scheduler.add_noise_coefficients(self._timesteps[S.t_start])
        z0, x = ops.img2img_init(mean, std, eps, noise, self.vae.config.scaling_factor, a, b)
        return x, z0, noise, mask

    def _inpaint9_extras(self, S, B, mask):
        """The five extra input channels of a 9-channel inpainting UNet -> (extra f32 [B,5,Hl,Wl],
        pad_value f32 [5]): the latent mask as 0.0 / 1.0 (1 = repaint; after ``mask_blur``) and zm, the scaled posterior sample
        of the init picture with the hole blanked through the UNBLURRED pixel mask.  One host draw (1,C,Hl,Wl), taken after
        ``_img2img_start``'s two, broadcast over the prompts.  Once per image: two launches and one VAE encode."""
        P = S.P
        vdt = next(self.vae.parameters()).dtype
        masked = ops.u8_to_vae_input_masked(self.last_init_pixels, self._raw_pixel_mask, vdt, 128)
        self._raw_pixel_mask = None
        dist = self.vae.encode(masked).latent_dist
        shape = (1, S.C, P.Hl, P.Wl)
        if tuple(dist.mean.shape) != shape:
            raise ValueError(f"the VAE encodes the masked image to {tuple(dist.mean.shape)}, the loop runs on {shape}")
        h0 = time.perf_counter()
        eps_host = self._stager.host(shape, torch.float32)
        eps_host.normal_()
        self.host_s["noise"] += time.perf_counter() - h0
        eps = self._stager.upload(eps_host, self.device)
        # ed_img2img_init's z0 output alone is (mean + std * eps) * sf, the restatement's expression; its x output is not used
        zm, _ = ops.img2img_init(dist.mean.contiguous(), dist.std.contiguous(), eps, eps, self.vae.config.scaling_factor, 1.0, 0.0)
        self.last_masked_image_latents = zm
        extra = torch.cat([mask.to(torch.float32).view(1, 1, P.Hl, P.Wl).expand(B, -1, -1, -1), zm.expand(B, -1, -1, -1)], dim=1)
        pad_value = torch.tensor([1.0] + [0.0] * S.C, dtype=torch.float32).to(self.device)
        return extra.contiguous(), pad_value

    def _assemble_unfused_x(self, P, x, idx, K, g_rows, v_rows, gframe, vframe, low, extra, pad_value):
        """``FUSED_GLUE`` off on a 9-channel UNet: the latent channels through ed_pick_assemble / ed_gather_views as always, the
        extra channels by torch indexing from the same tables -- bit-equal to ``ops.assemble_rows_x`` (a gather and one rounding)."""
        B, C = x.shape[:2]
        E = extra.shape[1]
        mdt = g_rows.dtype
        g4 = torch.empty(g_rows.shape[0], C, P.gpad.PH, P.gpad.PW, device=x.device, dtype=mdt)
        v4 = torch.empty(v_rows.shape[0], C, P.vpad.PH, P.vpad.PW, device=x.device, dtype=mdt)
        ops.pick_assemble(x, idx, P.src_row, P.src_col, g4, P.h, P.w, P.gpad.top, P.gpad.left, gframe, low)
        ops.gather_views(x, v4, P.win_y0, P.win_x0, P.views.Sh, P.views.Sw, P.vpad.top, P.vpad.left, vframe)
        pad = pad_value.to(mdt).view(1, E, 1, 1)
        g_rows[:, :C], v_rows[:, :C] = g4, v4
        g_rows[:, C:], v_rows[:, C:] = pad, pad
        q = idx.view(K, P.h, P.w).long()
        sy = P.src_row.long()[2 * torch.arange(P.h, device=x.device).view(1, -1, 1) + (q >> 1)]     # [K,h,w]
        sx = P.src_col.long()[2 * torch.arange(P.w, device=x.device).view(1, 1, -1) + (q & 1)]
        picked = extra[:, :, sy, sx].permute(2, 0, 1, 3, 4).to(mdt)                                  # [K,B,E,h,w]
        top, left = P.gpad.top, P.gpad.left
        g_rows.view(K, 2, B, C + E, P.gpad.PH, P.gpad.PW)[:, :, :, C:, top:top + P.h, left:left + P.w] = picked[:, None]
        top, left, Sh, Sw = P.vpad.top, P.vpad.left, P.views.Sh, P.views.Sw
        vr = v_rows.view(P.views.V, B, C + E, P.vpad.PH, P.vpad.PW)
        for v, (y0, x0) in enumerate(zip(P.views.win_y0, P.views.win_x0)):
            vr[v, :, C:, top:top + Sh, left:left + Sw] = extra[:, :, int(y0):int(y0) + Sh, int(x0):int(x0) + Sw].to(mdt)

    def _blend_known(self, S, x, mask, z0, noise, j, graded=False):
        """x <- where(mask, x, known(j)) in place: the kept region of the init image at the noise level of timestep index ``j``
        (the SAME initial noise at every step), the clean z0 after the last one.  ``graded``: ``mask`` is the level map and a
        pixel is held iff its level <= thr(j) = (255 * (T - j)) // T -- level 0 at every j, level 255
        never, one in between until the remaining fraction of the schedule drops to level / 255.  One launch either way."""
        if graded:
            thr = (255 * (S.T - j)) // S.T
            if j >= S.T:
                return ops.inpaint_blend_level(x, mask, thr, z0, None, 1.0, 0.0, clean=True)
            a, b = self.scheduler.add_noise_coefficients(self._timesteps[j])
            return ops.inpaint_blend_level(x, mask, thr, z0, noise, a, b)
        if j >= S.T:
            return ops.inpaint_blend(x, mask, z0, None, 1.0, 0.0, clean=True)
        a, b = self.scheduler.add_noise_coefficients(self._timesteps[j])
        return ops.inpaint_blend(x, mask, z0, noise, a, b)

    def _score_channels(self):
        """channels of the latent, and so of the class direction and the local score (``_setup_run``'s S.C)"""
        cfg = self.unet.config
        return getattr(cfg, "out_channels", 4) if cfg.in_channels == INPAINT_IN_CHANNELS else cfg.in_channels

    def _check_inpaint9(self, height, width, init_image=None, mask_image=None, mask_mode="binary"):
        """``check_inpaint_unet_arguments`` for this pipeline's UNet and ControlNet at a run's size"""
        s = self.vae_scale_factor
        return check_inpaint_unet_arguments(self.unet.config.in_channels, init_image, mask_image, mask_mode,
                                            self.controlnet is not None, (height // s, width // s))

    # ---- the loop (ED:953-1078) --------------------------------------------------------------------
    def _setup_run(self, height, width, num_inference_steps, guidance_scale, resampling_steps, new_p, rrg_stop_t,
                   rrg_init_weight, rrg_scherduler_cls, cosine_scale, repaint_sampling, controlnet_conditioning_scale,
                   guidance_rescale=0.0, strength=1.0, control_guidance_start=0.0, control_guidance_end=1.0):
        """Everything of one ``generate_image`` call that does not depend on the prompt, the seed or the condition
        image: geometry tables, schedules, the noised pad-background frames.  Shared by all images in flight."""
        inpaint9 = self.unet.config.in_channels == INPAINT_IN_CHANNELS  # (the callers checked the arguments: _check_inpaint9)
        ops.rescale_coefficients(guidance_rescale)  # ValueError outside [0, 1], before anything is launched
        control = check_control_arguments(len(self.controlnets), self.controlnets_listed, controlnet_conditioning_scale,
                                          control_guidance_start, control_guidance_end)  # ValueError likewise
        t_start = DDIMSchedule.img2img_window(num_inference_steps, strength)  # ValueError likewise
        self._mark("start")
        self.host_s = {"picks": 0.0, "phase_total": 0.0, "noise": 0.0, "stager_wait": 0.0}
        self._stager.waited = 0.0
        S = _Plan()
        S.P = P = self._plan(height, width)
        self.default_size = (4 * height, 4 * width)  # ED:969
        n_rrg = num_inference_steps - int(num_inference_steps * rrg_stop_t)
        if rrg_scherduler_cls is CosineScheduler or getattr(rrg_scherduler_cls, "__name__", "") == "CosineScheduler":
            S.rrg = rrg_scherduler_cls(steps=n_rrg, cosine_scale=cosine_scale, factor=rrg_init_weight)
        else:
            S.rrg = rrg_scherduler_cls(steps=n_rrg, start_val=rrg_init_weight, stop_val=0)
        # the latent has the model's OUTPUT channels everywhere; only the input rows of a 9-channel inpainting UNet are wider
        S.inpaint9 = inpaint9
        S.C = C = getattr(self.unet.config, "out_channels", 4) if inpaint9 else self.unet.config.in_channels
        dev = self.device
        ts = self.scheduler.set_timesteps(num_inference_steps)
        S.T = len(ts)
        S.t_start = t_start  # first executed timestep index (image-to-image ``strength``); 0 = the whole schedule
        self._timesteps = list(ts)
        self._t_dev = ts.to(dev)
        self._step_coef = [self.scheduler.step_coefficients(t) for t in ts]
        S.R = R = int(resampling_steps)
        if not 0 <= R <= host_rng.MAX_RESAMPLING_STEPS:
            raise ValueError(f"resampling_steps must be in [0, {host_rng.MAX_RESAMPLING_STEPS}] (the per-pixel "
                             f"last-covering-step table is int8), got {resampling_steps}")
        S.repaint = bool(repaint_sampling) and R > 0
        if S.repaint:
            # undo_step is only ever entered with timesteps[i+1] (ED:1040): row 0 is a placeholder
            rows = [self.scheduler.undo_coefficients(t) for t in ts[1:]]
            self._undo_coef = torch.stack(rows[:1] + rows).to(dev) if rows else None
        d0, d1 = self.default_size
        self._time_ids.copy_(torch.tensor([[d0, d1, 0, 0, d0, d1]], dtype=torch.float32))  # ED:232-246, 414-418
        self._gframes = self._strip_frames(P.gpad, self._timesteps, C)
        self._vframes = self._strip_frames(P.vpad, self._timesteps, C)
        self._mark("setup_done")
        S.Ks = sorted({R + 1, 1} if S.repaint else {R + 1})
        S.control = None
        if control is not None:
            # Multi-ControlNet / guidance windows (section 31): per executed timestep the weights scale[n] * keep[i][n]; they are
            # device data of the graphs (``GraphedForward``'s static ``w``), so no change of scale or window re-captures anything
            keep = control_keep(S.T - t_start, control[1], control[2])
            S.control = [tuple(np.float32(sc * k) for sc, k in zip(control[0], row)) for row in keep]
        else:
            if getattr(self, "_cn_scale", controlnet_conditioning_scale) != controlnet_conditioning_scale:
                self._runner.entries.clear()  # the scale is a constant inside captured graphs
            self._cn_scale = controlnet_conditioning_scale
        S.guidance, S.drop_p = guidance_scale, 1 - new_p
        S.guidance_rescale = float(guidance_rescale)  # 0 = plain CFG: the loop launches what it always launched
        S.norm = np.float32(2.0 / (C * P.Hl * P.Wl))
        return S

    def _region_weights(self, S, regions, region_blur):
        """The per-pixel weights of a run's regions (``check_region_arguments``' list) -> f32 [n + 1,Hl,Wl] on the device.  A box is
        drawn as a 255 rectangle at pixel size; a pixel-size mask is feathered by ``ops.gaussian_blur_u8`` when ``region_blur`` > 0
        and reduced to the latent grid by ``ops.resize_u8`` (Pillow's BILINEAR bytes); a latent-size mask is used as is.  Then one
        ``ops.region_weights`` launch.  Nothing syncs and nothing is drawn."""
        P, s, dev = S.P, self.vae_scale_factor, self.device
        H, W = P.Hl * s, P.Wl * s
        masks = torch.empty(len(regions), P.Hl, P.Wl, dtype=torch.uint8, device=dev)
        for k, (_, (kind, m), _) in enumerate(regions):
            masks[k] = self._latent_size_mask(S, kind, m, region_blur, "region mask")
        return ops.region_weights(masks, [w for _, _, w in regions])

    def _latent_size_mask(self, S, kind, m, blur, what):
        """one mask of ``check_region_arguments``' kinds -> uint8 [Hl,Wl] on the device (see ``_region_weights``)"""
        P, s, dev = S.P, self.vae_scale_factor, self.device
        H, W = P.Hl * s, P.Wl * s
        if kind == "latent":
            t = torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m
            return t.to(dev).reshape(P.Hl, P.Wl)
        if kind == "box":
            u8 = torch.zeros(H, W, dtype=torch.uint8, device=dev)
            u8[m[1]:m[3], m[0]:m[2]] = 255
        else:
            u8 = self._u8_image(m, 1, what)
            if isinstance(u8, np.ndarray):
                u8 = torch.from_numpy(np.ascontiguousarray(u8))
            u8 = u8.to(dev).contiguous().view(H, W)
        if blur > 0:
            u8 = ops.gaussian_blur_u8(u8, blur)
        return ops.resize_u8(u8, (P.Hl, P.Wl), "bilinear")

    def _ip_masks(self, S, entries, B):
        """``check_ip_adapter_mask_arguments``' entries -> f32 [B,A,Hl,Wl] on the device, fp32(u8) / 255 rounded once, all ones for
        an adapter without a mask: uploaded and reduced to the latent grid once per image, through ``regions``' path (section 33)."""
        P = S.P
        u8 = torch.full((len(entries), P.Hl, P.Wl), 255, dtype=torch.uint8, device=self.device)
        for a, e in enumerate(entries):
            if e is not None:
                u8[a] = self._latent_size_mask(S, e[0], e[1], 0.0, "ip_adapter_masks")
        if hasattr(self.unet, "ip_mask_weights"):   # the device weights of the masked path exist before any capture (a single adapter included)
            self.unet.ip_mask_weights()
        # fp32(u8) / 255 through a 256-entry table divided on the host: a device division by a Python scalar is a multiplication by
        # its reciprocal, two roundings
        lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(self.device)
        return lut[u8.long()][None].expand(B, -1, -1, -1).contiguous()

    def _prompt_chunks(self, prompts, negative_prompts):
        """Chunk count the encoder needs for these prompts and negative prompts together, or None for an encoder that does not
        chunk (an injected callable without ``chunks``, the synthetic embeddings)."""
        enc = self.text_encoder
        if enc is None or not hasattr(enc, "chunks"):
            return None
        return max(enc.chunks(prompts), enc.chunks(negative_prompts))

    def _program(self, S, prompts, negative_prompts, condition_image=None, trace=None, progress=_identity_progress,
                 direct=True, frames=None, init_image=None, mask_image=None, mask_blur=0.0, mask_mode="binary",
                 min_chunks=None, ip_adapter_image=None, ip_adapter_image_embeds=None, score_maps=None, regions=None,
                 region_blur=0.0, ip_adapter_negative_image_embeds=None, ip_adapter_masks=None):
        """Generator: the denoising loop of ONE image (ED:981-1078), yielding ``_ModelCall``s; returns the final latent.
        All host RNG draws happen inside, in the reference's order.  ``init_image`` / ``mask_image``: image-to-image and
        inpainting -- the loop starts at timestep index ``S.t_start`` from the noised encoding of the
        image, and with a mask the kept region is put back at the next noise level after every step.  ``mask_blur`` /
        ``mask_mode``: the mask feathered on the device and, in "graded" mode, read as a per-pixel release time (section 19).
        ``score_maps`` (a dict; section 26): filled with {"pca_cls_dir": {i: bytes}, "pca_uncond": {i: bytes}}, the PCA maps
        (uint8 [B, Hl, Wl, 3], on the device) of the class direction and the local score of the FIRST phase of every timestep
        index i with i % log_freq == 0.  ``regions`` / ``region_blur`` (``check_region_arguments``' list; section 28): regional
        prompts -- ``prompts`` is the base prompt, every region adds one conditional row per resampling step and sample, and the
        class direction is their per-pixel weighted sum.  No draw depends on them."""
        P = S.P
        if isinstance(prompts, str):
            prompts = [prompts]
        if isinstance(negative_prompts, str):
            negative_prompts = [negative_prompts] * len(prompts)
        # prompt and negative prompt share one token count: the larger chunk count of the two (and of ``min_chunks``)
        n = self._prompt_chunks(prompts, negative_prompts)
        if n is not None:
            if regions:  # ... and of the region prompts: all are rows of one model batch
                n = max(n, self.text_encoder.chunks([q for q, _, _ in regions]))
            n = max(n, int(min_chunks or 1))
        un, pun = self.get_text_embeds(negative_prompts, n)
        co, pco = self.get_text_embeds(prompts, n)
        if un.shape[1] != co.shape[1]:
            raise ValueError(f"text_encoder returned {co.shape[1]} tokens for the prompts and {un.shape[1]} for the negative "
                             "prompts: the two are rows of one model batch and must have the same token count")
        B = len(prompts)
        cos, pcos = [co], [pco]
        for q, _, _ in regions or ():  # a region's prompt applies to every sample
            cq, pq = self.get_text_embeds([q] * B, n)
            if cq.shape[1] != co.shape[1]:
                raise ValueError(f"text_encoder returned {cq.shape[1]} tokens for a region prompt and {co.shape[1]} for the prompts")
            cos.append(cq)
            pcos.append(pq)
        if ip_adapter_image is not None or ip_adapter_image_embeds is not None:
            # image prompt: the context of every row is [text tokens | image tokens] -- conditional rows carry the picture's tokens,
            # unconditional rows (the V view rows among them, through _embed_rows) the projection of a zero embedding
            neg = {} if ip_adapter_negative_image_embeds is None else dict(ip_adapter_negative_image_embeds=ip_adapter_negative_image_embeds)
            iun, ico = self._ip_tokens(B, ip_adapter_image, ip_adapter_image_embeds, **neg)   # (the call as it always was without the keyword)
            un = torch.cat([un, iun.to(un.dtype)], dim=1)
            cos = [torch.cat([c, ico.to(c.dtype)], dim=1) for c in cos]  # the image tokens ride on every conditional row
            co = cos[0]
        # initial latent from the host generator (ED:998-1000)
        z0 = noise0 = mask = None
        graded = mask_mode == "graded"
        if init_image is None:
            x_host = self._stager.host((B, S.C, P.Hl, P.Wl), torch.float32)
            x_host.normal_()
            x = self._stager.upload(x_host, self.device)
            self.last_init_pixels = self.last_pixel_mask = None
        else:
            x, z0, noise0, mask = self._img2img_start(S, B, init_image, mask_image, mask_blur, graded)
        self.last_init_latents = z0
        extras = None
        if S.inpaint9:  # the model conditions on the mask and the blanked picture: nothing is pasted back (diffusers' num_channels_unet == 9)
            extras = self._inpaint9_extras(S, B, mask)
            mask = None
        region_w = None
        if regions:
            region_w = self._region_weights(S, regions, region_blur)
            emb = {K: self._embed_rows(K, P.views.V, un, cos, pun, pcos) for K in S.Ks}
        else:
            emb = {K: self._embed_rows(K, P.views.V, un, co, pun, pco) for K in S.Ks}
        self.last_region_weights = region_w
        rg_kw = {} if region_w is None else dict(region_w=region_w)
        if ip_adapter_masks is not None:   # ``check_ip_adapter_mask_arguments``' entries: every model call carries its rows' masks
            rg_kw["ip_masks"] = self._ip_masks(S, ip_adapter_masks, B)
        cond = control_at = None
        if condition_image is not None:
            if self.controlnet is None:
                raise ValueError("condition_image given but no controlnet was supplied")
            ckw = {} if region_w is None else dict(copies=1 + len(cos))
            check_control_arguments(len(self.controlnets), self.controlnets_listed, 1.0, condition_image=condition_image)
            if S.control is None:
                cond = self._condition_rows(P, condition_image, B, S.Ks, **ckw)
            else:
                control_at = self._control_rows(S, condition_image, B, ckw)
        elif S.control is not None:
            raise ValueError("controlnet_conditioning_scale lists and guidance windows need condition_image")
        logs = {"x0": [], "rrg_x0": [], "init_low": None, "embeds": (un, co, pun, pco)} if self.verbose else None
        self._logs = logs
        rescale = None
        if S.guidance_rescale:
            rescale = _Rescale(S.guidance_rescale, B, S.C * P.Hl * P.Wl, S.C * P.h * P.w, self.device)
        # DPM-Solver++(2M) history, per image: (x0 of the last full-resolution phase of the previous timestep index, its timestep).
        # The two buffers alternate by themselves: every phase writes a fresh x0, and the one before the last is released here.
        hist = None
        pca_ws = None
        if score_maps is not None:
            score_maps.update({key: {} for key in SCORE_PCA_KEYS})
            pca_ws = ops.score_pca_workspace(B, P.Hl * P.Wl, self.device)
        for i, t in enumerate(progress(self._timesteps[S.t_start:]), start=S.t_start):  # absolute index; t_start = 0 without strength
            ms = self._multistep_args(t, hist, i == S.T - 1)  # both phases of a timestep step from the same history
            nz = self._step_noise(t)  # every phase of a stochastic timestep draws its own noise
            w_i = S.rrg(i)
            rrg_w = w_i if w_i > 10 else None  # ED:1061-1062
            two_phase = S.repaint and i < S.T - 1
            mapped = score_maps is not None and i % self.log_freq == 0
            if control_at is not None:  # every phase of timestep i runs the nets open at i, with its weights
                cond, ctl = control_at(i - S.t_start)
                rg_kw["ctl"] = ctl
            prev, x0, info = yield from self._phase_steps(P, x, i, S.R + 1, S.guidance, S.drop_p, emb, cond, direct,
                                                          None if two_phase else rrg_w, S.norm, frames, rescale, extras, ms,
                                                          keep_scores=mapped, step_noise=nz, **rg_kw)
            if mapped:  # PCA:165-196 on the R + 1-pass direction estimate and the per-view score, before the RePaint phase
                score_maps["pca_cls_dir"][i] = ops.score_pca(info["direction"], normalize=True, workspace=pca_ws)
                score_maps["pca_uncond"][i] = ops.score_pca(info["local"], workspace=pca_ws)
            if logs is not None and logs["init_low"] is None:
                # ED:1023-1024: taken right after the FIRST direction estimate, i.e. before the RePaint phase replaces
                # ``info`` with the one of the undone sample (ED:1043)
                logs["init_low"] = info["init_low"].clone()
            cfg = S.guidance
            if two_phase:  # ED:1038-1056
                if mask is not None:  # the re-noised latent carries the known region into the second phase
                    self._blend_known(S, prev, mask, z0, noise0, i + 1, graded)
                x = self._undo(prev, i + 1)
                cfg = S.guidance / 3
                prev, x0, info = yield from self._phase_steps(P, x, i, 1, cfg, S.drop_p, emb, cond, direct, rrg_w, S.norm,
                                                              frames, rescale, extras, ms, step_noise=nz, **rg_kw)
            hist = (x0, t)
            if logs is not None:  # verbose image logs (ED:1058-1059, 1073-1076)
                if i % self.log_freq == 0:
                    logs["x0"].append(x0.clone())
                    if rrg_w is not None:  # the reduced-resolution x0 the guidance pulls towards (ED:909-921)
                        sb, sa = self._step_coef[i][0], self._step_coef[i][1]
                        out = info["uncond_score"] + np.float32(cfg) * info["low_direction"]
                        if info["ratio_low"] is not None:  # the rescaled prediction the RRG term was formed from
                            gr, omgr = ops.rescale_coefficients(S.guidance_rescale)
                            out = gr * (out * info["ratio_low"].view(-1, 1, 1, 1)) + omgr * out
                        if self.scheduler.config.prediction_type == "v_prediction":
                            logs["rrg_x0"].append(np.float32(sa) * info["low_latent"] - np.float32(sb) * out)
                        else:
                            logs["rrg_x0"].append((info["low_latent"] - np.float32(sb) * out) / np.float32(sa))
            if info["x_next"] is not None:  # RRG already applied inside the fused epilogue
                x = info["x_next"]
            elif rrg_w is not None:  # ED:1061-1078
                sb, sa = self._step_coef[i][0], self._step_coef[i][1]
                nxt = torch.empty_like(prev)
                ops.rrg_update(prev, x0, info["low_latent"], info["uncond_score"], info["low_direction"], P.up_row,
                               P.up_col, nxt, np.float32(cfg), sb, sa, S.norm, np.float32(w_i),
                               prediction_type=self.scheduler.config.prediction_type, ratio_low=info["ratio_low"],
                               guidance_rescale=S.guidance_rescale if info["ratio_low"] is not None else 0.0)
                x = nxt
            else:
                x = prev
            if mask is not None:
                self._blend_known(S, x, mask, z0, noise0, i + 1, graded)
            if trace is not None:
                trace.append(x.clone())
        return x

    @_on_own_device
    @torch.no_grad()
    def generate_latents(self, prompts, negative_prompts="", height=768, width=768, num_inference_steps=50,
                         guidance_scale=10.0, resampling_steps=20, new_p=0.3, rrg_stop_t=0.2, rrg_init_weight=1000,
                         rrg_scherduler_cls=CosineScheduler, cosine_scale=3.0, repaint_sampling=True,
                         progress=_identity_progress, condition_image=None, controlnet_conditioning_scale=1.0,
                         trace=None, guidance_rescale=0.0, init_image=None, strength=1.0, mask_image=None, *, mask_blur=0.0,
                         mask_mode="binary", min_chunks=None, ip_adapter_image=None, ip_adapter_image_embeds=None,
                         ip_adapter_negative_image_embeds=None, score_pca=False, regions=None, region_blur=0.0, control_guidance_start=0.0, control_guidance_end=1.0,
                         ip_adapter_masks=None):
        """``ip_adapter_masks`` (keyword-only): one entry per loaded IP-Adapter -- None, an L PIL image / uint8
        array at picture or latent size, or a box (x0, y0, x1, y1) in pixels, the forms of a region's mask -- that confines the
        adapter's image prompt to a part of the picture: at every cross attention adapter a's term is multiplied per query row by
        its mask, followed through the picks and view windows of each model row and averaged 2 x 2 per UNet level.
        ``condition_image`` / ``controlnet_conditioning_scale`` / ``control_guidance_start`` / ``control_guidance_end``
        (diffusers 0.21.4's Multi-ControlNet keywords): with a pipeline built on a LIST of N ControlNets,
        ``condition_image`` is a list of N conditions and the other three are floats (applied to every net) or lists of N; net n
        acts with weight ``scale[n]`` on the executed timesteps i with start[n] <= i / T and (i + 1) / T <= end[n] and is not run on
        the others.  A single net given as such, with a scalar scale and the default window, runs the path it always ran.

        ``guidance_rescale`` in [0, 1] (diffusers' keyword; 0 = off): the std rescale of the guided model output of
        arXiv 2305.08891 section 3.4, what zero-terminal-SNR / v-prediction checkpoints are meant to be sampled with
        (DESIGN.md section 17).

        ``init_image`` / ``strength`` / ``mask_image`` (diffusers' image-to-image and 4-channel
        inpainting semantics): start from the VAE encoding of ``init_image`` -- an RGB PIL image or uint8 [H,W,3] array /
        tensor (Lanczos-resized to height x width on the device when it has another size), or a float tensor
        (1|B,3,height,width) in [0,1] -- noised to the first of the last ``int(steps * strength)`` timesteps, which are the ones
        that run.  ``mask_image`` (L PIL image / uint8 [H,W] of the image's size, or a bool / uint8 tensor at latent
        resolution; white = repaint, black = keep; a mask of the size of an init image that gets resized is resized on the host
        with PIL's NEAREST, a rare path): after every step the kept region is replaced by the init latent at the next
        noise level, so it ends as ``last_init_latents`` bit for bit.  Absent, the loop is what it always was.

        ``mask_blur`` / ``mask_mode`` (keyword-only): ``mask_blur`` > 0 feathers an 8-bit picture mask at
        the run's size with ``PIL.ImageFilter.GaussianBlur(mask_blur)``'s bytes, on the device.  ``mask_mode="binary"`` then
        thresholds the (blurred) bytes at 128 as before; ``"graded"`` reads the byte L sampled for a latent pixel as a release
        time: the pixel is held to the init image while L <= (255 * (T - j)) // T at target timestep index j, so black is kept
        bit for bit, white is never held, and a grey one is free from the original at the noise level where the remaining
        fraction of the schedule drops to L / 255.  No new RNG draws, one blend launch per phase in either mode.  The pixel
        mask and the 8-bit init picture stay on the device as ``last_pixel_mask`` / ``last_init_pixels``.

        ``min_chunks`` (keyword-only): encode prompt and negative prompt to at least this many 77-token
        chunks (a chunking ``text_encoder`` only) -- what a job of ``generate_latents_interleaved`` is encoded with.

        A UNet with 9 input channels (an inpainting checkpoint) needs an 8-bit ``init_image`` and picture
        ``mask_image``: every model row is ``cat([latent, mask, masked-image latent])`` with the extras sampled where the row's
        latent was (``ops.assemble_rows_x``), one more host draw is made for the masked-image latent
        (``last_masked_image_latents``), and the kept region is NOT pasted back in latent space.

        ``ip_adapter_image`` / ``ip_adapter_image_embeds`` (keyword-only): the image prompt of a loaded
        IP-Adapter (``load_ip_adapter``), exactly one of the two -- an RGB PIL image / uint8 [H,W,3] array or tensor (uploaded
        once; CLIP's resize, crop and normalise run on the device, then the ``image_encoder``), or its CLIP image embeddings
        [1 or B, clip_dim].

        ``score_pca`` (keyword-only): the reference's diagnostic pictures (pca_diffusion_scores.py) for this
        loop.  At every timestep index i with i % log_freq == 0 the class direction (normalised as there) and the local
        unconditional score of the timestep's first phase are projected onto their first three principal components and scaled to
        bytes on the device (``ops.score_pca``; nothing syncs); ``last_score_pca`` = {"pca_cls_dir": {i: uint8 [B, Hl, Wl, 3]},
        "pca_uncond": {...}} afterwards.  It only reads: latents and host RNG stream are those of the run without it.

        ``regions`` / ``region_blur`` (keyword-only): regional prompts.  ``regions`` = 1 to 7 entries
        ``(prompt, mask)`` or ``(prompt, mask, weight)``; a mask is an L PIL image / uint8 [H,W] at the picture's size (reduced to the
        latent grid on the device with Pillow's BILINEAR bytes, after a Gaussian blur of radius ``region_blur`` when that is > 0), a
        uint8 array / tensor already at the latent's size (used as is), or a box ``(x0, y0, x1, y1)`` in pixels; ``weight`` > 0
        (default 1) scales the region where regions overlap.  ``prompts`` is the base prompt: it fills what the regions leave
        uncovered.  One negative prompt is shared by all rows.  Every region adds one conditional model row per resampling step and
        sample; the host RNG stream is that of the run without regions.  ``last_region_weights`` holds the [n + 1,Hl,Wl] weights
        (plane 0 the base prompt's) of the last run, or None."""
        regions, region_blur = check_region_arguments(regions, height, width, self.vae_scale_factor, region_blur,
                                                      self.unet.config.in_channels)
        check_regions_sampler(regions, getattr(self, "scheduler", None))
        self._check_ip_adapter(ip_adapter_image, ip_adapter_image_embeds, ip_adapter_negative_image_embeds)
        ip_adapter_masks = check_ip_adapter_mask_arguments(len(self._ip_list()), ip_adapter_masks, height, width, self.vae_scale_factor)
        check_img2img_arguments(num_inference_steps, init_image, strength, mask_image)
        score_pca = check_score_pca_arguments(score_pca, self._score_channels())
        mask_blur = check_soft_inpaint_arguments(init_image, mask_image, mask_blur, mask_mode,
                                                 latent_size=(height // self.vae_scale_factor, width // self.vae_scale_factor))
        self._check_inpaint9(height, width, init_image, mask_image, mask_mode)
        S = self._setup_run(height, width, num_inference_steps, guidance_scale, resampling_steps, new_p, rrg_stop_t,
                            rrg_init_weight, rrg_scherduler_cls, cosine_scale, repaint_sampling,
                            controlnet_conditioning_scale, guidance_rescale, strength, control_guidance_start, control_guidance_end)
        self._runner.new_image()
        maps = {} if score_pca else None
        x = self._drive(self._program(S, prompts, negative_prompts, condition_image, trace, progress, direct=True,
                                      init_image=init_image, mask_image=mask_image, mask_blur=mask_blur, mask_mode=mask_mode,
                                      min_chunks=min_chunks, ip_adapter_image=ip_adapter_image,
                                      ip_adapter_image_embeds=ip_adapter_image_embeds, ip_adapter_negative_image_embeds=ip_adapter_negative_image_embeds, score_maps=maps, regions=regions,
                                      region_blur=region_blur, ip_adapter_masks=ip_adapter_masks))
        self.last_score_pca = maps
        self.last_latents = x
        self.host_s["blocked_ahead_of_gpu"] = self._stager.waited
        self._mark("loop_done")
        return x

    @_on_own_device
    @torch.no_grad()
    def generate_latents_interleaved(self, jobs, in_flight=2, height=768, width=768, num_inference_steps=50,
                                     guidance_scale=10.0, resampling_steps=20, new_p=0.3, rrg_stop_t=0.2,
                                     rrg_init_weight=1000, rrg_scherduler_cls=CosineScheduler, cosine_scale=3.0,
                                     repaint_sampling=True, controlnet_conditioning_scale=1.0, on_done=None,
                                     guidance_rescale=0.0, strength=1.0, control_guidance_start=0.0, control_guidance_end=1.0):
        """Several images of the SAME size / settings in flight at once (new; the reference has nothing like it).

        ``jobs`` = list of dicts {prompts, negative_prompts="", seed, condition_image=None, init_image=None,
        mask_image=None, mask_blur=0.0, mask_mode="binary", ip_adapter_image=None, ip_adapter_image_embeds=None, score_pca=False,
        regions=None, region_blur=0.0, ip_adapter_masks=None}
        (``score_pca``: that job's maps, as ``generate_latents`` makes them, in ``job_score_pca[index]``); ``strength`` is a setting of the call like the other schedule parameters, and jobs with and without
        an init image may mix (at ``strength`` 1: below it every job needs one; on a 9-channel inpainting UNet every job carries
        both ``init_image`` and ``mask_image``).  Each job is one
        ``_program`` with its own host RNG stream (``_HostRng``: exactly the stream ``seed_everything(seed)`` +
        ``generate_latents`` would consume, so every image's latents are those of running it alone, up to the model's
        own batch-shape dependent rounding).  Per tick, the pending model calls of all live programs -- e.g. the 20-row
        phase A batch of one image and the 6-row RePaint batch of another -- are concatenated into ONE forward, which
        is then row-sharded over the ranks like any other batch.  Why: with N ranks a lone image leaves 20/N and 6/N rows
        per rank, where the UNet runs at a fraction of its batch-20 rate; m images in flight multiply the rows per
        forward by ~m while the exchange stays one all-gather per tick.  Returns the final latents in job order
        (``on_done(index, latent)`` is called as each finishes, e.g. to decode it).

        Prompt length: the rows of all jobs share one text tensor, so with a chunking ``text_encoder`` every job is encoded to
        n chunks, n = the largest chunk count over the prompts and negative prompts of ALL jobs of the call: a job equals the
        same job run alone through ``generate_latents(..., min_chunks=n)``."""
        carrying = [job.get("ip_adapter_image") is not None or job.get("ip_adapter_image_embeds") is not None for job in jobs]
        if any(carrying) and not all(carrying):
            raise ValueError("either every job of a call carries an image prompt (ip_adapter_image / ip_adapter_image_embeds) or "
                             "none does: the rows of all jobs share one context width")
        for job in jobs:
            self._check_ip_adapter(job.get("ip_adapter_image"), job.get("ip_adapter_image_embeds"),
                                   job.get("ip_adapter_negative_image_embeds"))
        job_ip_masks = [check_ip_adapter_mask_arguments(len(self._ip_list()), job.get("ip_adapter_masks"), height, width,
                                                        self.vae_scale_factor) for job in jobs]
        n_chunks = None
        job_regions = [check_region_arguments(job.get("regions"), height, width, self.vae_scale_factor, job.get("region_blur", 0.0),
                                              self.unet.config.in_channels) for job in jobs]
        for rg, _ in job_regions:
            check_regions_sampler(rg, getattr(self, "scheduler", None))
        for job, (rg, _) in zip(jobs, job_regions):
            n = self._prompt_chunks(job["prompts"], job.get("negative_prompts", ""))
            if n is not None:
                n_chunks = max(n_chunks or 1, n, *([self.text_encoder.chunks([q for q, _, _ in rg])] if rg else []))
        for job in jobs:
            check_img2img_arguments(num_inference_steps, job.get("init_image"), strength, job.get("mask_image"))
            check_score_pca_arguments(job.get("score_pca", False), self._score_channels())
            if job.get("composite"):
                raise ValueError("composite is a keyword of generate_image: a job of generate_latents_interleaved returns latents")
            check_soft_inpaint_arguments(job.get("init_image"), job.get("mask_image"), job.get("mask_blur", 0.0),
                                         job.get("mask_mode", "binary"),
                                         latent_size=(height // self.vae_scale_factor, width // self.vae_scale_factor))
            self._check_inpaint9(height, width, job.get("init_image"), job.get("mask_image"), job.get("mask_mode", "binary"))
        S = self._setup_run(height, width, num_inference_steps, guidance_scale, resampling_steps, new_p, rrg_stop_t,
                            rrg_init_weight, rrg_scherduler_cls, cosine_scale, repaint_sampling,
                            controlnet_conditioning_scale, guidance_rescale, strength, control_guidance_start, control_guidance_end)
        self._runner.new_image()
        results = [None] * len(jobs)
        queue = list(range(len(jobs)))
        live = []  # [job index, program, rng, pending call]

        started = [0]

        def start(j):
            job = jobs[j]
            rng = _HostRng(job["seed"])
            # Every image pays for its own noised pad-background frames, exactly as when it runs alone (they depend only
            # on geometry and schedule, so the first job takes the ones _setup_run just made and each later job
            # recomputes identical ones); cache_backgrounds=True is the explicit opt-in to share them (ADVICE r2:
            # otherwise the N-GPU bench line amortises 100 VAE encodes the 1-GPU line pays per image)
            with torch.cuda.device(self.device):  # a job's clock starts BEFORE its pad-strip encodes
                ev0 = torch.cuda.Event(enable_timing=True)
                ev0.record(torch.cuda.current_stream(self.device))
            self.job_events[j] = [ev0, None]
            frames = None
            if started[0] and not self.cache_backgrounds:
                frames = (self._strip_frames(S.P.gpad, self._timesteps, S.C), self._strip_frames(S.P.vpad, self._timesteps, S.C))
            started[0] += 1
            if job.get("score_pca"):
                self.job_score_pca[j] = {}
            prog = self._program(S, job["prompts"], job.get("negative_prompts", ""), job.get("condition_image"),
                                 direct=False, frames=frames, init_image=job.get("init_image"),
                                 mask_image=job.get("mask_image"), mask_blur=float(job.get("mask_blur", 0.0)),
                                 mask_mode=job.get("mask_mode", "binary"), min_chunks=n_chunks,
                                 ip_adapter_image=job.get("ip_adapter_image"),
                                 ip_adapter_image_embeds=job.get("ip_adapter_image_embeds"),
                                 ip_adapter_negative_image_embeds=job.get("ip_adapter_negative_image_embeds"),
                                 score_maps=self.job_score_pca.get(j),
                                 regions=job_regions[j][0], region_blur=job_regions[j][1], ip_adapter_masks=job_ip_masks[j])
            with rng:
                call = next(prog)
            live.append([j, prog, rng, call])

        self.job_score_pca = {}  # job index -> its PCA maps, for the jobs that carry ``score_pca``
        self.job_events = {}  # job -> [start event, end event] on this device's stream (``job_latencies``)
        self._live_jobs = live  # a change of LoRA state is refused while this list is non-empty (``_lora_change``)
        try:
            while queue and len(live) < max(1, in_flight):
                start(queue.pop(0))
            self.ticks = 0
            while live:
                # one fused forward per group of shape-compatible pending calls (normally exactly one group)
                groups = {}
                for ent in live:
                    c = ent[3]
                    # (Multi-ControlNet: calls fuse when the same nets are open; their per-row weights ride along)
                    groups.setdefault((tuple(c.rows.shape[1:]), c.cond is None, tuple(c.text.shape[1:]),
                                       None if c.ctl is None else c.ctl[0]), []).append(ent)
                for ents in groups.values():
                    calls = [e[3] for e in ents]
                    sizes = [c.rows.shape[0] for c in calls]
                    if len(calls) == 1:
                        c = calls[0]
                        outs = [self._run_model(c.rows, c.t, c.text, c.pooled, c.cond, fresh_side=True, ctl=c.ctl, ipm=c.ipm)]
                    else:
                        rows = torch.cat([c.rows for c in calls])
                        t = torch.cat([c.t.reshape(1).expand(n) for c, n in zip(calls, sizes)])
                        text = torch.cat([c.text for c in calls])
                        pooled = torch.cat([c.pooled for c in calls])
                        cond = None if calls[0].cond is None else torch.cat([c.cond for c in calls])
                        ctl = None if calls[0].ctl is None else (calls[0].ctl[0], torch.cat([c.ctl[1] for c in calls]))
                        ipm = None
                        if any(c.ipm is not None for c in calls):   # a job without masks contributes all-ones rows
                            like = next(c.ipm for c in calls if c.ipm is not None)
                            ipm = (torch.cat([c.ipm[0] if c.ipm is not None else like[0].new_ones((n,) + tuple(like[0].shape[1:]))
                                              for c, n in zip(calls, sizes)]), like[1], like[2])
                        outs = self._run_model(rows, t, text, pooled, cond, fresh_side=True, ctl=ctl, ipm=ipm).split(sizes)
                    self.ticks += 1
                    for ent, out in zip(ents, outs):
                        j, prog, rng = ent[0], ent[1], ent[2]
                        try:
                            with rng:
                                ent[3] = prog.send(out)
                        except StopIteration as stop:
                            results[j] = stop.value
                            live.remove(ent)
                            if on_done is not None:
                                on_done(j, stop.value)
                            with torch.cuda.device(self.device):
                                ev1 = torch.cuda.Event(enable_timing=True)
                                ev1.record(torch.cuda.current_stream(self.device))
                            self.job_events[j][1] = ev1
                            if queue:
                                start(queue.pop(0))
        finally:
            self._live_jobs = None
        self.last_latents = results[-1] if results else None
        self.host_s["blocked_ahead_of_gpu"] = self._stager.waited
        self._mark("loop_done")
        return results

    def job_latencies(self, jobs=None):
        """-> seconds from the start of each job of the last ``generate_latents_interleaved`` call (its first pad-strip
        encode; the first job's frames are made by the shared setup just before) to the end of its ``on_done`` (decode), in
        job order; synchronises.  ``jobs``: only these job indices (a rank that did not decode a job has no decode inside
        that job's interval).  With m images in flight the throughput is ~m images per latency: bench.py reports both so a
        throughput-scaling line cannot be read as a per-image speed-up."""
        torch.cuda.synchronize(self.device)
        return [1e-3 * a.elapsed_time(b) for j, (a, b) in sorted(self.job_events.items())
                if b is not None and (jobs is None or j in jobs)]

    @_on_own_device
    @torch.no_grad()
    def generate(self, latent, text_embeds, add_text_embeds, guidance_scale=7.5, guidance_rescale=0.0, score_pca=False, *,
                 regions=None):
        """ED:761-796: plain CFG + DDIM generation of ``latent`` (B,C,h,w; the reference calls it on the initial
        reduced-resolution latent for its ``verbose`` image log) over the scheduler's current timesteps.
        ``text_embeds`` / ``add_text_embeds`` = cat([uncond, cond]) like the reference's.  A latent smaller than the
        model's native size is padded with the noised-background frames (ED:404-411).
        ``guidance_rescale`` > 0: the reference's rescale_noise_cfg (ED:800-811) on uncond + g * (cond - uncond) with
        noise_pred_text = cond, its std ratio computed on the device.
        ``score_pca``: this loop is the script's own (PCA:151-204); every log_freq steps the PCA maps of
        cond - uncond (normalised as there) and of uncond are added to the info dict, {"pca_cls_dir": {i: uint8 [B,h,w,3] on the
        device}, "pca_uncond": {...}}.
        -> (PIL image of the first sample, {"inter_x0": [pred_original_sample every log_freq steps]})"""
        if regions is not None:
            raise ValueError("regions are not supported by generate(), the base-resolution loop: it has no resampling rows to carry "
                             "them; use generate_image / generate_latents")
        ops.rescale_coefficients(guidance_rescale)
        if self.unet.config.in_channels != 4:
            raise ValueError("generate() drives a 4-channel UNet: a bare latent has no mask or masked-image rows")
        dev, mdt = self.device, self.model_dtype
        x = latent.to(dev, torch.float32).contiguous()
        B, C, h, w = x.shape
        maps = {key: {} for key in SCORE_PCA_KEYS} if check_score_pca_arguments(score_pca, C) else {}
        pca_ws = ops.score_pca_workspace(B, h * w, dev) if maps else None
        if self.scheduler.timesteps is None:
            raise RuntimeError("generate(): call scheduler.set_timesteps / generate_image first (ED:776 iterates them)")
        ts = list(self.scheduler.timesteps)
        pad = geometry.PadPlan(h, w, self.model_size)
        frames = self._strip_frames(pad, ts, C)
        xl = self.sd_version.startswith("XL")
        text = text_embeds.to(dev, mdt).contiguous()
        pooled = add_text_embeds.to(dev, mdt).contiguous() if xl else text
        if self.default_size is None:
            self.default_size = (4 * h * self.vae_scale_factor, 4 * w * self.vae_scale_factor)
        d0, d1 = self.default_size
        self._time_ids.copy_(torch.tensor([[d0, d1, 0, 0, d0, d1]], dtype=torch.float32))
        self._runner.new_image()
        inter = []
        rs_kw = {}
        if guidance_rescale:
            ws = ops.guidance_moments_workspace(B, C * h * w, 0, dev)
            rs_kw = dict(ratio=torch.empty(B, device=dev, dtype=torch.float32), guidance_rescale=guidance_rescale)
        hist = None  # DPM-Solver++(2M): the previous iteration's (x0, timestep)
        for i, t in enumerate(ts):
            if pad.padded:  # the reference re-seeds the global generators once per pad strip (ED:359)
                host_rng.replay_strip_reseeds(len(pad.strips))
            rows = torch.empty(2 * B, C, pad.PH, pad.PW, device=dev, dtype=mdt)
            if frames is not None:
                rows.copy_(frames[i].to(mdt).expand(2 * B, -1, -1, -1))
            rows[:, :, pad.top:pad.top + h, pad.left:pad.left + w] = torch.cat([x, x]).to(mdt)
            out = self._run_model(rows, torch.as_tensor(t, device=dev), text, pooled)
            out = out[:, :, pad.top:pad.top + h, pad.left:pad.left + w].float()
            uncond, cnd = out[:B].contiguous(), out[B:].contiguous()
            prev, x0 = torch.empty_like(x), torch.empty_like(x)
            direction = (cnd - uncond).contiguous()
            if maps and i % self.log_freq == 0:
                maps["pca_cls_dir"][i] = ops.score_pca(direction, normalize=True, workspace=pca_ws)
                maps["pca_uncond"][i] = ops.score_pca(uncond, workspace=pca_ws)
            if rs_kw:
                ops.guidance_moments(uncond, direction, np.float32(guidance_scale), rs_kw["ratio"], ws, text=cnd)
            ms = self._multistep_args(t, hist, i == len(ts) - 1)
            nz = self._step_noise(t)  # a stochastic step draws where the reference calls scheduler.step (ED:776)
            ops.cfg_ddim_step(uncond, direction, x, prev, x0, np.float32(guidance_scale),
                              *self.scheduler.step_coefficients(t),
                              prediction_type=self.scheduler.config.prediction_type, **rs_kw,
                              **({} if ms is None else dict(multistep=ms)),
                              **({} if nz is None else dict(noise=(nz, self._draw_step_noise(x.shape)))))
            hist = (x0, t)
            x = prev
            if i % self.log_freq == 0:
                inter.append(x0.cpu())
        return self._to_pil(self.decode_latents(x))[0], {"inter_x0": inter, **maps}

    @staticmethod
    def _to_pil(imgs):
        from PIL import Image
        arr = imgs.mul(255).byte().permute(0, 2, 3, 1).cpu().numpy()  # what ToPILImage does for float CHW (ED:1125)
        return [Image.fromarray(a) for a in arr]

    def _image_log(self, decode_fn, guidance_scale, guidance_rescale=0.0):
        """ED:1092-1118: the ``verbose`` image log of the last single-image run (grids via make_grid's defaults)."""
        logs, image_log = getattr(self, "_logs", None), {}
        if not logs:
            return image_log

        def grid_of(latents):
            dec = torch.cat([decode_fn(z[k:k + 1]) for z in latents for k in range(len(z))])
            return self._to_pil(_make_grid(dec.clamp(0, 1))[None])[0]

        if logs["init_low"] is not None and self.unet.config.in_channels == 4:  # (no plain-CFG global image on an inpainting UNet)
            un, co, pun, pco = logs["embeds"]
            image_log["global_img"], info = self.generate(logs["init_low"], torch.cat([un, co]), torch.cat([pun, pco]),
                                                          guidance_scale=guidance_scale, guidance_rescale=guidance_rescale)
            if info["inter_x0"]:
                image_log["global_img_inter_x0_imgs"] = grid_of([z.to(self.device) for z in info["inter_x0"]])
        if logs["x0"]:
            image_log["intermediate_x0_imgs"] = grid_of(logs["x0"])
        image_log["intermediate_cascade_x0_imgs"] = {}
        if logs["rrg_x0"]:
            image_log["intermediate_cascade_x0_imgs"]["rrg"] = grid_of(logs["rrg_x0"])
        return image_log

    # ---- decode (ED:267-310) -----------------------------------------------------------------------
    @_on_own_device
    @torch.no_grad()
    def decode_latents(self, latents):
        vdt = next(self.vae.parameters()).dtype
        img = self.vae.decode((latents / self.vae.config.scaling_factor).to(vdt)).sample
        return (img.float() / 2 + 0.5).clamp(0, 1)

    @_on_own_device
    @torch.no_grad()
    def tiled_decode(self, latents, tile_batch=8):
        """ED:275-310 with the tiles gathered in one launch, decoded ``tile_batch`` at a time (and sharded over ranks),
        and accumulated + normalised in one launch."""
        B, C, Hl, Wl = latents.shape
        s = self.vae_scale_factor
        tp = geometry.TilePlan(Hl, Wl, self.unet.config.sample_size, s, low_vram=self.low_vram)
        vdt = next(self.vae.parameters()).dtype
        tiles = torch.empty(tp.T * B, C, tp.Ts, tp.Ts, device=self.device, dtype=vdt)
        ops.tile_gather_pad(latents.contiguous(), tiles, self._dev_i32(tp.tile_y0), self._dev_i32(tp.tile_x0),
                            self.vae.config.scaling_factor)

        def dec(rows, *_):
            outs = [self.vae.decode(rows[a:a + tile_batch]).sample for a in range(0, rows.shape[0], tile_batch)]
            return torch.cat(outs).contiguous()

        decoded = self.sharder.run(dec, tiles, None, None, None, out_like=((3, tp.Ts * s, tp.Ts * s), vdt))
        image = torch.empty(B, decoded.shape[1], Hl * s, Wl * s, device=self.device, dtype=torch.float32)
        rt, rs, ct, cs = tp.pixel_tables()
        ops.tile_accumulate_normalise(decoded, image, tp.n_col_tiles, self._dev_i32(rt), self._dev_i32(rs),
                                      self._dev_i32(ct), self._dev_i32(cs))
        return image

    @_on_own_device
    @torch.no_grad()
    def generate_image(self, prompts, negative_prompts="", height=768, width=768, num_inference_steps=50,
                       guidance_scale=10.0, resampling_steps=20, new_p=0.3, rrg_stop_t=0.2, rrg_init_weight=1000,
                       rrg_scherduler_cls=CosineScheduler, cosine_scale=3.0, repaint_sampling=True,
                       progress=_default_progress, tiled_decoder=False, grid=False, guidance_rescale=0.0, *,
                       condition_image=None, controlnet_conditioning_scale=1.0, output_type="pil", init_image=None,
                       strength=1.0, mask_image=None, mask_blur=0.0, mask_mode="binary", composite=False,
                       ip_adapter_image=None, ip_adapter_image_embeds=None, ip_adapter_negative_image_embeds=None, score_pca=False,
                       regions=None, region_blur=0.0,
                       control_guidance_start=0.0, control_guidance_end=1.0, ip_adapter_masks=None):
        """ED:953-965 signature (ControlNet keywords of EDC:1120-1134 are keyword-only here), then ``guidance_rescale``
        (diffusers' keyword) and, keyword-only, ``init_image`` / ``strength`` / ``mask_image`` / ``mask_blur`` / ``mask_mode``
        (see ``generate_latents``) and ``composite``: paste every decoded picture over the 8-bit init picture through the
        (blurred) pixel mask, ``PIL.Image.composite``'s bytes, in the launch that converts the floats to 8 bit
        (``ops.composite_u8``) -- where the mask is 0 the result IS the init picture.
        ``ip_adapter_image`` / ``ip_adapter_image_embeds``: the image prompt of a loaded IP-Adapter (see ``generate_latents``).
        ``score_pca``: the PCA maps of ``generate_latents``, the first sample's enlarged by the VAE factor with Pillow's BILINEAR bytes
        on the device, in ``image_log`` as {"pca_cls_dir": {i: PIL}, "pca_uncond": {i: PIL}} (the script's pictures and names).
        ``regions`` / ``region_blur``: regional prompts (see ``generate_latents``).
        ``ip_adapter_masks``: one attention mask per loaded IP-Adapter (see ``generate_latents``).
        Returns ``(images, image_log)``; images are PIL by default, a float tensor with ``output_type='pt'``."""
        check_region_arguments(regions, height, width, self.vae_scale_factor, region_blur, self.unet.config.in_channels)
        check_regions_sampler(regions, getattr(self, "scheduler", None))
        self._check_ip_adapter(ip_adapter_image, ip_adapter_image_embeds, ip_adapter_negative_image_embeds)
        check_ip_adapter_mask_arguments(len(self._ip_list()), ip_adapter_masks, height, width, self.vae_scale_factor)
        check_img2img_arguments(num_inference_steps, init_image, strength, mask_image)
        check_soft_inpaint_arguments(init_image, mask_image, mask_blur, mask_mode, composite, output_type, grid,
                                     latent_size=(height // self.vae_scale_factor, width // self.vae_scale_factor))
        self._check_inpaint9(height, width, init_image, mask_image, mask_mode)
        z = self.generate_latents(prompts, negative_prompts, height, width, num_inference_steps, guidance_scale,
                                  resampling_steps, new_p, rrg_stop_t, rrg_init_weight, rrg_scherduler_cls,
                                  cosine_scale, repaint_sampling, progress, condition_image,
                                  controlnet_conditioning_scale, guidance_rescale=guidance_rescale, init_image=init_image,
                                  strength=strength, mask_image=mask_image, mask_blur=mask_blur, mask_mode=mask_mode,
                                  ip_adapter_image=ip_adapter_image, ip_adapter_image_embeds=ip_adapter_image_embeds, ip_adapter_negative_image_embeds=ip_adapter_negative_image_embeds,
                                  score_pca=score_pca, regions=regions, region_blur=region_blur,
                                  control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end,
                                  ip_adapter_masks=ip_adapter_masks)
        dec = self.tiled_decode if tiled_decoder else self.decode_latents
        image_log = self._image_log(dec, guidance_scale, guidance_rescale) if self.verbose else {}  # ED:1092-1118 (before the final decode)
        if score_pca:
            image_log.update(self._score_pca_log(self.last_score_pca))
        imgs = torch.cat([dec(z[i:i + 1]) for i in range(len(z))])  # decode_bs = 1 (ED:1090, 1121)
        self._mark("decode_done")
        if grid:
            imgs = _make_grid(imgs)[None]  # ED:1124: torchvision make_grid(imgs, nrow=8, padding=2, pad_value=0)
        if output_type == "pt":
            return imgs, image_log
        if composite:
            return self._composite_pil(imgs), image_log
        return self._to_pil(imgs), image_log

    def _score_pca_log(self, maps):
        """PCA:180: the first sample's maps enlarged by the VAE factor (``T.Resize`` on a PIL image = ``Image.resize(BILINEAR)``)"""
        from PIL import Image
        s = self.vae_scale_factor
        log = {}
        for key, by_step in maps.items():
            log[key] = {}
            for i, m in by_step.items():
                big = ops.resize_u8(m[0], (m.shape[1] * s, m.shape[2] * s), filter="bilinear")
                log[key][i] = Image.fromarray(big.cpu().numpy())
        return log

    def _composite_pil(self, imgs):
        """decoded (B,3,H,W) floats in [0,1] -> PIL images: each pasted over ``last_init_pixels`` through ``last_pixel_mask``"""
        from PIL import Image
        init, mask = self.last_init_pixels, self.last_pixel_mask
        if init is None or mask is None or tuple(init.shape[:2]) != tuple(imgs.shape[2:]):
            raise ValueError(f"composite: the decoded picture is {tuple(imgs.shape[2:])}, the init picture "
                             f"{None if init is None else tuple(init.shape[:2])}")
        imgs = imgs.float().contiguous()
        return [Image.fromarray(ops.composite_u8(imgs[i:i + 1], init, mask).cpu().numpy()) for i in range(len(imgs))]

    @_on_own_device
    def outpaint_canvas(self, image, left, top, right, bottom):
        """The canvas of an outpainting run: ``image`` (what ``init_image`` accepts in 8-bit form: an RGB PIL image or a uint8
        [H,W,3] array / tensor) grown by the four borders with its edge replicated -> (canvas uint8 [H',W',3], mask uint8
        [H',W'], 255 on the new border and 0 over the original), both on the device, ready to pass as ``init_image`` /
        ``mask_image``.  One launch (``ops.canvas_pad_u8``)."""
        u8 = self._u8_image(image, 3, "image")
        if u8 is None:
            raise ValueError(f"outpaint_canvas takes an RGB PIL image or a uint8 [H,W,3] array / tensor, got {type(image).__name__}")
        pads = (left, top, right, bottom)
        if any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) or p < 0 for p in pads):
            raise ValueError(f"outpaint_canvas: the borders must be integers >= 0, got {pads!r}")
        if isinstance(u8, np.ndarray):
            u8 = torch.from_numpy(np.ascontiguousarray(u8))
        H, W = int(u8.shape[0]), int(u8.shape[1])
        if H < 1 or W < 1 or H + top + bottom > ops.RESIZE_MAX_DIM or W + left + right > ops.RESIZE_MAX_DIM:
            raise ValueError(f"outpaint_canvas: {H} x {W} grown by {pads} leaves the sides 1..{ops.RESIZE_MAX_DIM}")
        return ops.canvas_pad_u8(u8.to(self.device).contiguous(), *(int(p) for p in pads))


class ElasticDiffusionControlNet(ElasticDiffusion):
    """Drop-in for the ControlNet variant (/root/reference/elastic_diffusion_w_controlnet.py:118-196, 1119-1322):
    ``controlnet_model`` is the third positional constructor argument and ``condition_image`` /
    ``controlnet_conditioning_scale`` sit where the reference has them in ``generate_image``.

    ``generate_image(condition_image=...)`` takes the already pre-processed condition (float tensor (1,3,8h,8w) in [0,1]
    at the reduced resolution, EDC:1183-1193; a PIL image / numpy array of that size is converted).  A raw photo goes
    through ``prepare_condition_image`` (the reference command line's three lines, EDC:1391-1393; its resize is Pillow's
    bicubic, computed on the device by csrc/resize_kernels.hip) or, already resized, through ``process_condition_image``
    (EDC:1102-1117) first:

    * ``'canny'`` is ``cv2.Canny(img, 100, 200)`` replicated to three channels, computed on the device by the HIP
      kernels of csrc/canny_kernels.hip (``ops.canny``; the algorithm is written out in DESIGN.md);
    * ``'depth'`` calls the ``depth_estimator=`` callable given to the constructor (the reference builds a HF
      ``pipeline('depth-estimation')`` there, EDC:186); without one it raises ``NotImplementedError``.
    """

    def __init__(self, device, sd_version="2.0", controlnet_model="canny", verbose=False, log_freq=5,
                 view_batch_size=1, low_vram=False, *, controlnet=None, depth_estimator=None, **kw):
        kinds = list(controlnet_model) if isinstance(controlnet_model, (list, tuple)) else None
        if kinds is not None and not 1 <= len(kinds) <= ops.CONTROL_MAX_NETS:
            raise ValueError(f"controlnet_model lists {len(kinds)} kinds: 1 .. {ops.CONTROL_MAX_NETS} ControlNets are supported")
        if kinds is not None and controlnet is not None and (not isinstance(controlnet, (list, tuple)) or len(controlnet) != len(kinds)):
            raise ValueError(f"controlnet_model lists {len(kinds)} kinds: controlnet must list as many nets")
        if kinds is None and isinstance(controlnet, (list, tuple)):
            raise ValueError("a list of ControlNets needs controlnet_model to list their kinds, e.g. ['canny', 'depth']")
        if controlnet is None:
            from .models import build_models
            dev = torch.device(device)
            unet, vae, controlnet = build_models(sd_version, device=dev, dtype=kw.get("model_dtype"), controlnet=True,
                                                 weights=kw.get("weights"))
            kw.setdefault("unet", unet)
            kw.setdefault("vae", vae)
            if kinds is not None:  # one net per kind: the snapshot's subfolders controlnet, controlnet_1, ... (seeds 2, 3, ... without)
                from .models import build_controlnet
                controlnet = [controlnet] + [build_controlnet(sd_version, dev, kw.get("model_dtype"), kw.get("weights"), k)
                                             for k in range(1, len(kinds))]
        super().__init__(device, sd_version, verbose, log_freq, view_batch_size, low_vram, controlnet=controlnet, **kw)
        self.controlnet_model = controlnet_model
        self.depth_estimator = depth_estimator

    def process_condition_image(self, condition_image, controlnet_model, *, output_type="pil"):
        """EDC:1102-1117: a PIL image (or HWC uint8 array) at the reduced resolution -> the ControlNet condition, a PIL RGB
        image with three identical channels.  ``output_type="pt"`` (extra) returns the fp32 (1,3,H,W) condition tensor on
        the pipeline's device instead, without the PIL round trip."""
        if isinstance(controlnet_model, (list, tuple)):  # kind by kind (Multi-ControlNet)
            imgs = list(condition_image) if isinstance(condition_image, (list, tuple)) else [condition_image] * len(controlnet_model)
            if len(imgs) != len(controlnet_model):
                raise ValueError(f"{len(imgs)} condition images for {len(controlnet_model)} ControlNet kinds")
            return [self.process_condition_image(im, k, output_type=output_type) for im, k in zip(imgs, controlnet_model)]
        if isinstance(condition_image, (list, tuple)):
            raise ValueError("a list of condition images needs a list of ControlNet kinds")
        assert controlnet_model in ["canny", "depth"], f"processing for ControlNet: {controlnet_model} is not implemented"
        if output_type not in ("pil", "pt"):
            raise ValueError(f"output_type must be 'pil' or 'pt', got {output_type!r}")
        from PIL import Image
        if controlnet_model == "canny":
            if isinstance(condition_image, torch.Tensor):           # uint8 [H,W,C] / [H,W] already on the device (ops.canny checks it)
                img = condition_image
            else:
                if hasattr(condition_image, "convert") and condition_image.mode not in ("L", "RGB"):
                    condition_image = condition_image.convert("RGB")
                arr = np.array(condition_image)
                if arr.dtype != np.uint8 or arr.ndim not in (2, 3):
                    raise TypeError(f"canny needs an 8-bit image (PIL, or uint8 [H,W,C] / [H,W] array), got {arr.dtype} {arr.shape}")
                img = torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
            if output_type == "pt":
                return ops.canny(img, 100, 200, out="cond")
            return Image.fromarray(ops.canny(img, 100, 200, out="u8").cpu().numpy())
        if self.depth_estimator is None:
            raise NotImplementedError(
                "depth extraction needs a depth estimator: construct with depth_estimator=<callable>, called as "
                "depth_estimator(image)['depth'] -> single-channel image, e.g. transformers.pipeline('depth-estimation') "
                "as the reference does (EDC:186, 1112)")
        depth = np.array(self.depth_estimator(condition_image)["depth"])[:, :, None]
        depth_image = Image.fromarray(np.concatenate([depth, depth, depth], axis=2))
        if output_type == "pt":
            return self._to_condition_tensor(depth_image, depth_image.size[1], depth_image.size[0]).to(self.device)
        return depth_image

    def _device_image(self, image):
        """The source bytes of an image the resize kernels take -- an L / RGB PIL image, a uint8 [H,W,C] (C = 1 or 3) / [H,W] array
        or such a tensor -- as a uint8 tensor on the pipeline's device (one upload), else None: every other input (RGBA / LA are
        resampled premultiplied by Pillow, P / 1 with the nearest filter, ...) stays on the host path."""
        if hasattr(image, "convert"):
            if image.mode not in ("L", "RGB"):
                return None
            image = np.array(image)
        if not isinstance(image, (np.ndarray, torch.Tensor)) or image.dtype not in (np.uint8, torch.uint8):
            return None
        if not (image.ndim == 2 or (image.ndim == 3 and image.shape[2] in (1, 3))):
            return None
        if not all(1 <= n <= ops.RESIZE_MAX_DIM for n in image.shape[:2]):
            return None
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image))
        return image.to(self.device).contiguous()

    def prepare_condition_image(self, image, height, width, *, output_type="pil"):
        """EDC:1391-1393, what the reference command line does with ``--condition_image``: resize the photo to the reduced
        resolution of a ``height`` x ``width`` run (PIL's default filter: bicubic), RGB, then ``process_condition_image``.

        An L / RGB PIL image, a uint8 [H,W,C] / [H,W] array or such a tensor is uploaded once and resized on the device
        (``ops.resize_u8``: Pillow's bytes exactly); the Canny detector takes the resized tensor where it is, and
        ``output_type="pt"`` (extra) returns the fp32 (1,3,H,W) condition tensor without a host image in between.  The depth
        estimator is a host callable and still receives a PIL image.  Any other PIL mode is resized by PIL on the host."""
        if output_type not in ("pil", "pt"):
            raise ValueError(f"output_type must be 'pil' or 'pt', got {output_type!r}")
        if isinstance(self.controlnet_model, (list, tuple)):  # a list of photos (or one photo for every net) -> a list, kind by kind
            kinds = list(self.controlnet_model)
            imgs = list(image) if isinstance(image, (list, tuple)) else [image] * len(kinds)
            if len(imgs) != len(kinds):
                raise ValueError(f"{len(imgs)} condition images for {len(kinds)} ControlNets")
            out = []
            for im, kind in zip(imgs, kinds):
                self.controlnet_model = kind
                try:
                    out.append(self.prepare_condition_image(im, height, width, output_type=output_type))
                finally:
                    self.controlnet_model = kinds
            return out
        if isinstance(image, (list, tuple)):
            raise ValueError("a list of condition images needs a list of ControlNets")
        ds = self.get_downsample_size(height, width)
        h_px, w_px = ds[0] * self.vae_scale_factor, ds[1] * self.vae_scale_factor
        dev = self._device_image(image) if max(h_px, w_px) <= ops.RESIZE_MAX_DIM else None
        if dev is None:
            image = image.resize((w_px, h_px)).convert("RGB")
        else:
            image = ops.resize_u8(dev, (h_px, w_px), "bicubic")
            if self.controlnet_model != "canny":
                from PIL import Image
                arr = image.cpu().numpy()
                image = Image.fromarray(arr[:, :, 0] if arr.ndim == 3 and arr.shape[2] == 1 else arr).convert("RGB")
        return self.process_condition_image(image, self.controlnet_model, output_type=output_type)

    def _to_condition_tensor(self, image, h_px, w_px):
        if isinstance(image, torch.Tensor):
            t = image.float()
            t = t[None] if t.dim() == 3 else t
        else:  # PIL image or HWC uint8 array -> what VaeImageProcessor.preprocess(do_normalize=False) yields:
            # RGB, Lanczos resize to the requested size, [0,1] floats (EDC:173-175, 1017)
            size = (image.size[1], image.size[0]) if hasattr(image, "convert") else tuple(np.shape(image)[:2])
            rgb_array = isinstance(image, np.ndarray) and image.ndim == 3 and image.shape[2] == 3
            if size != (h_px, w_px) and max(h_px, w_px) <= ops.RESIZE_MAX_DIM and (hasattr(image, "convert") or rgb_array):
                dev = self._device_image(image)
                if dev is not None:   # Lanczos on the device, written straight as the condition tensor (L: the channel replicated)
                    return ops.resize_u8(dev, (h_px, w_px), "lanczos", out="cond")
            if hasattr(image, "convert"):
                image = image.convert("RGB")
                if image.size != (w_px, h_px):
                    from PIL import Image
                    image = image.resize((w_px, h_px), resample=Image.LANCZOS)
            arr = np.asarray(image)
            t = torch.from_numpy(np.ascontiguousarray(arr)).float().div(255.0).permute(2, 0, 1)[None]
        if tuple(t.shape[-2:]) != (h_px, w_px):
            t = torch.nn.functional.interpolate(t, size=(h_px, w_px), mode="bilinear", align_corners=False)
        return t

    @torch.no_grad()
    def generate_image(self, prompts, negative_prompts="", condition_image=None, height=768, width=768,
                       num_inference_steps=50, guidance_scale=10.0, controlnet_conditioning_scale=1.0,
                       resampling_steps=20, new_p=0.3, rrg_stop_t=0.2, rrg_init_weight=1000,
                       rrg_scherduler_cls=CosineScheduler, cosine_scale=3.0, repaint_sampling=True,
                       progress=_default_progress, tiled_decoder=False, grid=False, guidance_rescale=0.0, *,
                       output_type="pil", init_image=None, strength=1.0, mask_image=None, mask_blur=0.0, mask_mode="binary",
                       composite=False, ip_adapter_image=None, ip_adapter_image_embeds=None, ip_adapter_negative_image_embeds=None,
                       score_pca=False, regions=None,
                       region_blur=0.0, control_guidance_start=0.0, control_guidance_end=1.0, ip_adapter_masks=None):
        check_region_arguments(regions, height, width, self.vae_scale_factor, region_blur, self.unet.config.in_channels)
        check_regions_sampler(regions, getattr(self, "scheduler", None))
        self._check_ip_adapter(ip_adapter_image, ip_adapter_image_embeds, ip_adapter_negative_image_embeds)
        check_img2img_arguments(num_inference_steps, init_image, strength, mask_image)
        check_soft_inpaint_arguments(init_image, mask_image, mask_blur, mask_mode, composite, output_type, grid,
                                     latent_size=(height // self.vae_scale_factor, width // self.vae_scale_factor))
        self._check_inpaint9(height, width, init_image, mask_image, mask_mode)
        if condition_image is None:
            raise ValueError("condition_image is required (EDC:1183-1193)")
        h, w = self.get_downsample_size(height, width)
        s = self.vae_scale_factor
        check_control_arguments(len(self.controlnets), self.controlnets_listed, controlnet_conditioning_scale,
                                control_guidance_start, control_guidance_end, condition_image)
        if isinstance(condition_image, (list, tuple)):
            cond = [self._to_condition_tensor(c, h * s, w * s) for c in condition_image]
        else:
            cond = self._to_condition_tensor(condition_image, h * s, w * s)
        return super().generate_image(prompts, negative_prompts, height, width, num_inference_steps, guidance_scale,
                                      resampling_steps, new_p, rrg_stop_t, rrg_init_weight, rrg_scherduler_cls,
                                      cosine_scale, repaint_sampling, progress, tiled_decoder, grid, guidance_rescale,
                                      condition_image=cond, controlnet_conditioning_scale=controlnet_conditioning_scale,
                                      output_type=output_type, init_image=init_image, strength=strength,
                                      mask_image=mask_image, mask_blur=mask_blur, mask_mode=mask_mode, composite=composite,
                                      ip_adapter_image=ip_adapter_image, ip_adapter_image_embeds=ip_adapter_image_embeds, ip_adapter_negative_image_embeds=ip_adapter_negative_image_embeds,
                                      score_pca=score_pca, regions=regions, region_blur=region_blur,
                                      control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end,
                                      ip_adapter_masks=ip_adapter_masks)
