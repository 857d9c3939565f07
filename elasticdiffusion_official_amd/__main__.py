"""Command line of the hot path, mirroring the reference's ``__main__`` blocks (elastic_diffusion.py:1134-1210,
elastic_diffusion_w_controlnet.py:1342-1433): same flags and defaults, PNGs + args.txt under
``<outdir>/<exp>/<timestamp>_<seed>/``.

    python -m elasticdiffusion_official_amd --prompt "..." --H 1024 --W 2048 --sd_version XL1.0 [--weights DIR]

Differences: needs a ROCm device (no CPU fallback); ``--weights DIR`` points at a local HF snapshot (unet/, vae/,
text_encoder*/ ...); without it the architecture is randomly initialised and the text embeddings are synthetic
(this build image has neither checkpoints nor network).  Boolean flags take true/false (the reference's
``type=bool`` treats every non-empty string as True).  ``--condition_image FILE`` selects the ControlNet pipeline and is
the already extracted condition by default; ``--process_condition true`` treats it as a raw photo like the reference's
flag of the same name (resize to the reduced resolution, canny on the device / injected depth estimator) and saves the
extracted condition as ``condition.png``.  ``--condition_image``, ``--controlnet_model`` and
``--controlnet_conditioning_scale`` may be repeated, once per ControlNet, with ``--control_guidance_start`` /
``--control_guidance_end`` giving each net its window of the steps; the conditions are then saved as ``condition_{n}.png``.  ``--prediction_type``, ``--timestep_spacing`` and
``--rescale_betas_zero_snr`` override what the snapshot's ``scheduler/scheduler_config.json`` says (or the SD defaults
without ``--weights``); the reference takes these from the hub config only.  ``--guidance_rescale`` is diffusers' keyword of
that name (0 = off), what such checkpoints are meant to be sampled with.  ``--sampler dpmsolver++`` (``--solver_order`` 1 / 2) samples with
DPM-Solver++(2M) instead of DDIM on the same timestep grid; ``--eta`` (DDIM), ``--sampler euler_a`` /
``dpmsolver++sde`` / ``lcm`` are the stochastic samplers of section 29 (one host noise draw per phase).  ``--init_image FILE`` with ``--strength`` (and
``--mask_image FILE``: white = repaint, black = keep) is image-to-image / inpainting with diffusers' semantics; the picture is
resized to H x W with Pillow's Lanczos filter, a mask of the picture's size with NEAREST.  ``--mask_blur R`` feathers the mask with
Pillow's ``GaussianBlur(R)`` on the device, ``--mask_mode graded`` reads the grey levels as release times, ``--composite`` pastes
the result over the init picture through the mask, and ``--outpaint L,T,R,B`` grows ``--init_image`` by that many pixels per side
(edge replicated) and repaints the new border; it takes the place of ``--mask_image``.  ``--max_prompt_chunks N`` encodes a prompt of
more than 75 tokens in up to N 75-token chunks instead of truncating it and ``--prompt_weighting true`` reads ``(word:1.3)`` / ``[word]``
as A1111's emphasis syntax; both act on the CLIP encoders of ``--weights`` (the synthetic embeddings are always 77 tokens).
``--sd_version 1.5-inpaint`` / ``2.0-inpaint`` / ``XL1.0-inpaint`` builds the 9-channel inpainting UNet of the family (what the
inpainting checkpoints carry; a ``--weights`` snapshot with a 9-channel ``conv_in`` selects it by itself): it needs ``--init_image``
and a mask, and conditions on the mask and the blanked picture instead of pasting the kept region back.
``--lora PATH[:SCALE]`` (repeatable) merges a LoRA adapter file into the weights after the models are built, in the order given
(DESIGN.md section 23); SCALE defaults to 1.
``--ip_adapter PATH[:SCALE]`` installs a base IP-Adapter and takes the image prompt either as a picture,
``--ip_adapter_image FILE`` with ``--image_encoder DIR`` (a local CLIPVisionModelWithProjection), or as CLIP image embeddings,
``--ip_adapter_embeds FILE`` (``.pt`` / ``.npy``).  All four flags are repeatable (up to four adapters, base or Plus; DESIGN.md
section 32) and matched by position; a Plus adapter given as embeddings also needs ``--ip_adapter_negative_embeds FILE``.
``--score_pca true`` saves the reference's diagnostic pictures (pca_diffusion_scores.py) every ``--log_freq``
steps under the script's own names, ``pca_cls_dir_{i}.png`` / ``pca_uncond_{i}.png``.
``--region_prompt TEXT`` with ``--region_mask FILE|x0,y0,x1,y1[:WEIGHT]`` (both repeatable, paired in order) are regional prompts
(DESIGN.md section 28): ``--prompt`` stays the base prompt that fills what the regions leave uncovered, a mask is a picture at
H x W (white = the region) or a box in pixels, WEIGHT > 0 (default 1) decides overlaps, and ``--region_blur R`` feathers the masks.
"""
import argparse
import os
import time
from datetime import datetime

import numpy as np
import torch


def _bool(v):
    return str(v).lower() in ("1", "true", "yes", "y", "t")


class _Repeat(argparse.Action):
    """A flag that may be given several times: once, the option is its string, as it always was; from the second on, a list."""

    def __call__(self, parser, namespace, value, option_string=None):
        held = getattr(namespace, self.dest, None)
        setattr(namespace, self.dest, value if held is None else (held if isinstance(held, list) else [held]) + [value])


def _listed(value):
    return [] if value is None else (list(value) if isinstance(value, list) else [value])


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m elasticdiffusion_official_amd")
    ap.add_argument("--prompt", type=str, default="A realistic portrait of a young black woman. she has a Christmas red "
                    "hat and a red scarf. Her eyes are light brown like they're almost caramel color. Her attire, simple yet dignified.")
    ap.add_argument("--negative", type=str, default="blurry, ugly, duplicate, no details, deformed")
    ap.add_argument("--sd_version", type=str, default="XL1.0", help="1.4, 1.5, 2.0, 2.1, XL1.0; 1.5-inpaint, 2.0-inpaint, "
                    "XL1.0-inpaint: the 9-channel inpainting UNet of that family (needs --init_image and --mask_image / "
                    "--outpaint); a --weights snapshot with a 9-channel conv_in selects it by itself")
    ap.add_argument("--H", type=int, default=2048)
    ap.add_argument("--W", type=int, default=2048)
    ap.add_argument("--low_vram", type=_bool, default=False)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--num_sampled", type=int, default=1)
    ap.add_argument("--guidance_scale", type=float, default=10.0)
    ap.add_argument("--cosine_scale", type=float, default=10.0)
    ap.add_argument("--rrg_scale", type=float, default=4000)
    ap.add_argument("--resampling_steps", type=int, default=10)
    ap.add_argument("--new_p", type=float, default=0.3)
    ap.add_argument("--rrg_stop_t", type=float, default=0.2)
    ap.add_argument("--view_batch_size", type=int, default=16)
    ap.add_argument("--outdir", type=str, default="results_log/")
    ap.add_argument("--make_grid", type=_bool, default=False)
    ap.add_argument("--repaint_sampling", type=_bool, default=True)
    ap.add_argument("--tiled_decoder", type=_bool, default=False)
    ap.add_argument("--exp", type=str, default="ElasticDiffusion")
    ap.add_argument("--tag", type=str, default="")
    ap.add_argument("--log_freq", type=int, default=5)
    ap.add_argument("--verbose", type=_bool, default=False)
    ap.add_argument("--weights", type=str, default=None, help="local HF snapshot directory (optional)")
    ap.add_argument("--condition_image", type=str, action="append", default=None, help="condition image => ControlNet path "
                    "(pre-processed unless --process_condition true); repeat it, with --controlnet_model, once per ControlNet")
    ap.add_argument("--process_condition", type=_bool, default=False, help="true: --condition_image is a raw photo; resize it "
                    "and extract the canny / depth condition from it as the reference command line does (EDC:1390-1393)")
    ap.add_argument("--controlnet_conditioning_scale", type=float, action="append", default=None,
                    help="default 0.2; once for all ControlNets or once per ControlNet")
    ap.add_argument("--controlnet_model", type=str, action="append", default=None, help="default depth; once per --condition_image")
    ap.add_argument("--control_guidance_start", type=float, action="append", default=None,
                    help="fraction of the executed steps at which a ControlNet starts to act (default 0); once or once per ControlNet")
    ap.add_argument("--control_guidance_end", type=float, action="append", default=None,
                    help="fraction of the executed steps after which a ControlNet is released (default 1); once or once per ControlNet")
    ap.add_argument("--prediction_type", type=str, default=None, choices=["epsilon", "v_prediction"],
                    help="what the UNet predicts; default: the snapshot's scheduler_config.json, else epsilon")
    ap.add_argument("--timestep_spacing", type=str, default=None, choices=["leading", "linspace", "trailing"],
                    help="default: the snapshot's scheduler_config.json, else leading")
    ap.add_argument("--rescale_betas_zero_snr", type=_bool, default=None,
                    help="zero terminal SNR betas; default: the snapshot's scheduler_config.json, else false")
    ap.add_argument("--guidance_rescale", type=float, default=0.0,
                    help="std rescale of the guided prediction in [0, 1] (arXiv 2305.08891 section 3.4; diffusers' "
                    "guidance_rescale), for zero-terminal-SNR / v-prediction checkpoints; 0 = off")
    ap.add_argument("--sampler", type=str, default="ddim", choices=["ddim", "euler_a", "dpmsolver++", "dpmsolver++sde", "lcm"],
                    help="ddim: the reference's first-order sampler; dpmsolver++: DPM-Solver++(2M), the multistep solver meant "
                    "for 20-25 step images (no extra model call per step); euler_a: the ancestral step (DDIM at eta = 1) on "
                    "the same timestep grid; dpmsolver++sde: SDE-DPM-Solver++(2M); lcm: the scheduler of an LCM-LoRA (4-8 steps)")
    ap.add_argument("--solver_order", type=int, default=2, choices=[1, 2], help="order of --sampler dpmsolver++ / dpmsolver++sde")
    ap.add_argument("--eta", type=float, default=0.0, help="eta of --sampler ddim in [0, 1]: 0 = deterministic (default), 1 = the "
                    "ancestral step; every stochastic step draws one latent-sized noise sample on the host")
    ap.add_argument("--init_image", type=str, default=None, help="start from this picture instead of pure noise "
                    "(image-to-image; resized to H x W)")
    ap.add_argument("--strength", type=float, default=1.0, help="fraction of the schedule an --init_image run executes, in "
                    "(0, 1] (diffusers' strength); 1 = all of it")
    ap.add_argument("--mask_image", type=str, default=None, help="inpainting mask for --init_image: white = repaint, black = keep")
    ap.add_argument("--mask_blur", type=float, default=0.0, help="feather the mask: Gaussian radius in pixels at H x W "
                    "(PIL.ImageFilter.GaussianBlur); 0 = off")
    ap.add_argument("--mask_mode", type=str, default="binary", choices=["binary", "graded"], help="binary: the (blurred) mask "
                    "thresholded at 128; graded: its grey level is the fraction of the schedule a pixel is free for")
    ap.add_argument("--composite", action="store_true", help="paste the result over the init picture through the (blurred) mask")
    ap.add_argument("--outpaint", type=str, default=None, metavar="L,T,R,B", help="grow --init_image by this many pixels on the "
                    "left, top, right and bottom (edge replicated) and repaint the new border; exclusive with --mask_image")
    ap.add_argument("--max_prompt_chunks", type=int, default=1, help="encode prompts of up to this many 75-token chunks "
                    "(concatenated on the token axis) instead of truncating at 75 tokens; 1 = the reference's truncation")
    ap.add_argument("--prompt_weighting", type=_bool, default=False, help="true: (word), [word], (word:1.3) scale the "
                    "embeddings of their tokens (A1111 syntax); false: brackets are literal text")
    ap.add_argument("--lora", action="append", default=[], metavar="PATH[:SCALE]", help="merge this LoRA adapter "
                    "(*.safetensors; diffusers, PEFT or kohya keys) into the UNet / CLIP weights at SCALE (default 1); repeatable, "
                    "applied in the order given")
    ap.add_argument("--ip_adapter", action=_Repeat, default=None, metavar="PATH[:SCALE]", help="install this IP-Adapter, base or "
                    "Plus (*.safetensors, *.bin, *.pt) at SCALE (default 1); needs --ip_adapter_image or --ip_adapter_embeds.  "
                    "Repeatable, up to 4: the image flags are then given once per adapter and matched by position")
    ap.add_argument("--ip_adapter_image", action=_Repeat, default=None, help="the image prompt (a picture; needs --image_encoder)")
    ap.add_argument("--ip_adapter_embeds", action=_Repeat, default=None, help="the image prompt as CLIP image embeddings "
                    "[1, clip_dim] (Plus: penultimate hidden states [1, S, embed_dim]): a .pt (torch.save of a tensor) or .npy file")
    ap.add_argument("--ip_adapter_negative_embeds", action=_Repeat, default=None, help="the unconditional embeddings a Plus adapter "
                    "given as --ip_adapter_embeds needs (.pt / .npy; 'none' at the position of a base adapter)")
    ap.add_argument("--ip_adapter_mask", action="append", default=[], metavar="FILE|x0,y0,x1,y1", help="where an adapter's image "
                    "prompt applies: a mask picture at H x W (white = applies), a box in pixels, or 'none'; repeatable, matched by "
                    "position with --ip_adapter (DESIGN.md section 33)")
    ap.add_argument("--image_encoder", action=_Repeat, default=None, help="local directory of a transformers "
                    "CLIPVisionModelWithProjection, for --ip_adapter_image (one for all adapters, or one per adapter)")
    ap.add_argument("--score_pca", type=_bool, default=False, help="true: every --log_freq steps, save the PCA maps of the class "
                    "direction and of the local unconditional score as pca_cls_dir_{i}.png / pca_uncond_{i}.png")
    ap.add_argument("--region_prompt", action="append", default=[], metavar="TEXT", help="prompt of one region (repeatable, up to 7); "
                    "pairs with the --region_mask at the same position, --prompt stays the base prompt")
    ap.add_argument("--region_mask", action="append", default=[], metavar="FILE|x0,y0,x1,y1[:WEIGHT]", help="where a region "
                    "applies: a mask picture at H x W (white = the region) or a box in pixels; WEIGHT > 0 (default 1) scales the "
                    "region where regions overlap")
    ap.add_argument("--region_blur", type=float, default=0.0, help="feather the region masks: Gaussian radius in pixels at H x W; "
                    "0 = off")
    return ap


def _region_mask_arg(text):
    """``FILE|x0,y0,x1,y1[:WEIGHT]`` -> (a path or a 4-tuple of ints, weight)"""
    spec, weight = _lora_arg(text)
    parts = spec.split(",")
    if len(parts) == 4:
        try:
            return tuple(int(v) for v in parts), weight
        except ValueError:
            pass
    return spec, weight


def parse_regions(opt, open_image=None):
    """The ``regions`` list of ``generate_image`` from --region_prompt / --region_mask, or None without them; SystemExit on unequal
    counts or a mask file that does not exist.  ``open_image(path)`` -> the mask picture (default: Pillow, converted to "L")."""
    if len(opt.region_prompt) != len(opt.region_mask):
        raise SystemExit(f"--region_prompt and --region_mask pair in order: got {len(opt.region_prompt)} prompts and "
                         f"{len(opt.region_mask)} masks")
    if not opt.region_prompt:
        if opt.region_blur:
            raise SystemExit("--region_blur needs --region_prompt / --region_mask")
        return None
    if open_image is None:
        from PIL import Image
        open_image = lambda path: Image.open(path).convert("L")  # noqa: E731
    regions = []
    for prompt, text in zip(opt.region_prompt, opt.region_mask):
        mask, weight = _region_mask_arg(text)
        if isinstance(mask, str):
            if not os.path.isfile(mask):
                raise SystemExit(f"--region_mask: no such file {mask!r} (a box is x0,y0,x1,y1)")
            mask = open_image(mask)
        regions.append((prompt, mask, weight))
    return regions


def parse_ip_adapter_masks(opt, n_adapters, open_image=None):
    """The ``ip_adapter_masks`` list of ``generate_image`` from --ip_adapter_mask, or None without the flag; SystemExit on a count
    other than --ip_adapter's or a mask file that does not exist.  ``open_image`` as in ``parse_regions``."""
    if not opt.ip_adapter_mask:
        return None
    if len(opt.ip_adapter_mask) != n_adapters:
        raise SystemExit(f"--ip_adapter_mask is matched by position with --ip_adapter ('none' for an adapter without a mask): got "
                         f"{len(opt.ip_adapter_mask)} masks for {n_adapters} adapters")
    if open_image is None:
        from PIL import Image
        open_image = lambda path: Image.open(path).convert("L")  # noqa: E731
    masks = []
    for text in opt.ip_adapter_mask:
        parts = text.split(",")
        if text.lower() == "none":
            masks.append(None)
        elif len(parts) == 4 and all(p.strip().lstrip("-").isdigit() for p in parts):
            masks.append(tuple(int(p) for p in parts))
        elif not os.path.isfile(text):
            raise SystemExit(f"--ip_adapter_mask: no such file {text!r} (a box is x0,y0,x1,y1)")
        else:
            masks.append(open_image(text))
    return masks


def _load_embeds(path):
    if path.endswith(".npy"):
        return torch.from_numpy(np.load(path, allow_pickle=False)).float()
    if path.endswith(".pt"):
        return torch.load(path, map_location="cpu", weights_only=True).float()
    raise SystemExit(f"--ip_adapter_embeds takes a .pt or .npy file, got {path!r}")


def _lora_arg(text):
    """``PATH[:SCALE]`` -> (path, scale); a trailing ``:x`` counts as the scale only when x reads as a number"""
    path, sep, tail = text.rpartition(":")
    if sep and path:
        try:
            return path, float(tail)
        except ValueError:
            pass
    return text, 1.0


INPAINT_VERSIONS = ("1.5-inpaint", "2.0-inpaint", "XL1.0-inpaint")


def _outpaint_borders(text):
    try:
        pads = tuple(int(v) for v in text.split(","))
    except ValueError:
        pads = ()
    if len(pads) != 4 or min(pads) < 0 or max(pads) == 0:
        raise SystemExit(f"--outpaint takes four integers >= 0, not all zero: L,T,R,B (got {text!r})")
    return pads


def _control_flags(opt):
    """The repeatable ControlNet flags after parsing: one occurrence (or none) leaves the scalar it always was; several
    --condition_image make the Multi-ControlNet run -> the number of ControlNets (0 without one)."""
    n = len(opt.condition_image or ())
    for name, default in (("controlnet_model", "depth"), ("controlnet_conditioning_scale", 0.2), ("control_guidance_start", 0.0),
                          ("control_guidance_end", 1.0)):
        v = getattr(opt, name)
        if v is None:
            v = [default]
        if len(v) not in (1, n) or (name == "controlnet_model" and n > 1 and len(v) != n):
            raise SystemExit(f"--{name}: given {len(v)} times for {n} --condition_image")
        setattr(opt, name, v[0] if len(v) == 1 and (n <= 1 or name != "controlnet_model") else v)
    if n <= 1:
        opt.condition_image = opt.condition_image[0] if n else None
    return n


def main(argv=None):
    opt = build_parser().parse_args(argv)
    n_control = _control_flags(opt)
    if not 0.0 <= opt.guidance_rescale <= 1.0:
        raise SystemExit(f"--guidance_rescale must be in [0, 1], got {opt.guidance_rescale}")
    if opt.max_prompt_chunks < 1:
        raise SystemExit(f"--max_prompt_chunks must be >= 1, got {opt.max_prompt_chunks}")
    from .pipeline import check_img2img_arguments, check_region_arguments
    regions = parse_regions(opt)
    try:
        check_region_arguments(regions, opt.H, opt.W, 8, opt.region_blur, 9 if opt.sd_version.endswith("-inpaint") else 4)
    except ValueError as e:
        raise SystemExit(f"--region_prompt / --region_mask / --region_blur: {e}")
    loras = [_lora_arg(v) for v in opt.lora]
    for path, _ in loras:
        if not os.path.isfile(path):
            raise SystemExit(f"--lora: no such file {path!r}")
    ip = None
    if opt.ip_adapter is not None:
        ip = [_lora_arg(v) for v in _listed(opt.ip_adapter)]
        images, embeds, negs = _listed(opt.ip_adapter_image), _listed(opt.ip_adapter_embeds), _listed(opt.ip_adapter_negative_embeds)
        encoders = _listed(opt.image_encoder)
        if bool(images) == bool(embeds):
            raise SystemExit("--ip_adapter needs exactly one of --ip_adapter_image / --ip_adapter_embeds")
        if len(ip) > 4:
            raise SystemExit(f"--ip_adapter: up to 4 adapters, got {len(ip)}")
        if len(images or embeds) != len(ip):
            raise SystemExit(f"{len(ip)} --ip_adapter flags need as many --ip_adapter_image or --ip_adapter_embeds flags, matched by "
                             f"position; got {len(images or embeds)}")
        if images and not encoders:
            raise SystemExit("--ip_adapter_image needs --image_encoder (a local CLIPVisionModelWithProjection directory)")
        if len(encoders) not in (0, 1, len(ip)):
            raise SystemExit(f"--image_encoder: one for all adapters or one per adapter, got {len(encoders)} for {len(ip)}")
        if negs and (images or len(negs) != len(ip)):
            raise SystemExit("--ip_adapter_negative_embeds goes with --ip_adapter_embeds, once per adapter ('none' for a base adapter)")
        for flag, paths in (("--ip_adapter", [p for p, _ in ip]), ("--ip_adapter_image", images), ("--ip_adapter_embeds", embeds),
                            ("--ip_adapter_negative_embeds", [p for p in negs if p.lower() != "none"])):
            for path in paths:
                if not os.path.isfile(path):
                    raise SystemExit(f"{flag}: no such file {path!r}")
        for d in encoders:
            if not os.path.isdir(d):
                raise SystemExit(f"--image_encoder: no such directory {d!r}")
    elif opt.ip_adapter_image or opt.ip_adapter_embeds or opt.image_encoder or opt.ip_adapter_negative_embeds:
        raise SystemExit("--ip_adapter_image / --ip_adapter_embeds / --image_encoder need --ip_adapter")
    ip_masks = parse_ip_adapter_masks(opt, len(ip or ()))
    if ip_masks is not None:
        from .pipeline import check_ip_adapter_mask_arguments
        try:
            check_ip_adapter_mask_arguments(len(ip), ip_masks, opt.H, opt.W)
        except ValueError as e:
            raise SystemExit(f"--ip_adapter_mask: {e}")
    pads = None
    if opt.outpaint is not None:
        if opt.mask_image or not opt.init_image:
            raise SystemExit("--outpaint needs --init_image and takes the place of --mask_image")
        pads = _outpaint_borders(opt.outpaint)
    has_mask = opt.mask_image or pads
    from .pipeline import check_soft_inpaint_arguments
    if opt.sd_version.endswith("-inpaint"):
        if opt.sd_version not in INPAINT_VERSIONS:
            raise SystemExit(f"--sd_version: the inpainting variants are {', '.join(INPAINT_VERSIONS)}, got {opt.sd_version!r}")
        if not opt.init_image or not has_mask:
            raise SystemExit(f"--sd_version {opt.sd_version} needs --init_image and --mask_image (or --outpaint)")
        if opt.mask_mode == "graded" or opt.condition_image:
            raise SystemExit(f"--sd_version {opt.sd_version} takes neither --mask_mode graded nor --condition_image")
    try:
        check_img2img_arguments(opt.steps, opt.init_image, opt.strength, has_mask or None)
        # the files are opened later: 8-bit pictures stand in for them, so that every rule is checked before a model is built
        check_soft_inpaint_arguments(np.zeros((1, 1, 3), np.uint8) if opt.init_image else None,
                                     np.zeros((1, 1), np.uint8) if has_mask else None, opt.mask_blur, opt.mask_mode,
                                     opt.composite, grid=opt.make_grid)
    except ValueError as e:
        raise SystemExit(f"--init_image / --strength / --mask_image / --mask_blur / --mask_mode / --composite: {e}")

    from . import ElasticDiffusion, ElasticDiffusionControlNet
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: this package has no CPU path (the reference's CPU path lives in oracle/)")
    device = torch.device("cuda")
    kw = {}
    if opt.weights:
        from .text import load_clip
        kw["weights"] = opt.weights
        kw["text_encoder"] = load_clip(opt.weights, opt.sd_version.startswith("XL"), device,
                                       max_prompt_chunks=opt.max_prompt_chunks, prompt_weighting=opt.prompt_weighting)
    sched = dict(prediction_type=opt.prediction_type, timestep_spacing=opt.timestep_spacing,
                 rescale_betas_zero_snr=opt.rescale_betas_zero_snr)
    if any(v is not None for v in sched.values()):  # a given flag overrides the snapshot's value / the default
        from .pipeline import check_sampler_arguments, make_scheduler
        from .schedule import DDIMSchedule
        check_sampler_arguments(opt.sampler, opt.solver_order, None, opt.eta)
        kw["scheduler"] = make_scheduler(DDIMSchedule.from_config_dir(opt.weights, **sched), opt.sampler, opt.solver_order, opt.eta)
    elif opt.sampler != "ddim" or opt.eta != 0.0:
        kw.update(sampler=opt.sampler, solver_order=opt.solver_order, eta=opt.eta)
    extra = {}
    if opt.condition_image:
        from PIL import Image
        sd = ElasticDiffusionControlNet(device, opt.sd_version, opt.controlnet_model, verbose=opt.verbose,
                                        log_freq=opt.log_freq, view_batch_size=opt.view_batch_size,
                                        low_vram=opt.low_vram, **kw)
        condition_image = [Image.open(f) for f in opt.condition_image] if n_control > 1 else Image.open(opt.condition_image)
        if opt.process_condition:
            condition_image = sd.prepare_condition_image(condition_image, opt.H, opt.W)
        extra = dict(condition_image=condition_image, controlnet_conditioning_scale=opt.controlnet_conditioning_scale)
        if opt.control_guidance_start != 0.0 or opt.control_guidance_end != 1.0:
            extra.update(control_guidance_start=opt.control_guidance_start, control_guidance_end=opt.control_guidance_end)
    else:
        sd = ElasticDiffusion(device, opt.sd_version, verbose=opt.verbose, log_freq=opt.log_freq,
                              view_batch_size=opt.view_batch_size, low_vram=opt.low_vram, **kw)
    for path, scale in loras:
        name = sd.load_lora(path, scale)
        print(f"LoRA {name!r} merged at scale {scale:g}: {sd.loras[-1][2]} tensors")
    if ip is not None:
        for a, (path, scale) in enumerate(ip):
            enc = None if not encoders else encoders[a if len(encoders) > 1 else 0]
            name = sd.load_ip_adapter(path, scale, image_encoder=enc, add=a > 0)
            print(f"IP-Adapter {name!r} installed at scale {scale:g}: {sd.ip_adapters[-1][2]} image tokens ({sd.ip_adapters[-1][3]})")
        one = len(ip) == 1    # one adapter: the bare value, as always
        if images:
            from PIL import Image
            pics = [Image.open(f).convert("RGB") for f in images]
            extra["ip_adapter_image"] = pics[0] if one else pics
        else:
            loaded = [_load_embeds(f) for f in embeds]
            extra["ip_adapter_image_embeds"] = loaded[0] if one else loaded
            if negs:
                neg = [None if f.lower() == "none" else _load_embeds(f) for f in negs]
                extra["ip_adapter_negative_image_embeds"] = neg[0] if one else neg
        if ip_masks is not None:
            extra["ip_adapter_masks"] = ip_masks
    if opt.init_image:
        from PIL import Image
        extra["init_image"], extra["strength"] = Image.open(opt.init_image).convert("RGB"), opt.strength
        if opt.mask_image:
            extra["mask_image"] = Image.open(opt.mask_image).convert("L")
        if pads:
            extra["init_image"], extra["mask_image"] = sd.outpaint_canvas(extra["init_image"], *pads)
        extra.update(mask_blur=opt.mask_blur, mask_mode=opt.mask_mode, composite=opt.composite)
    if opt.score_pca:
        extra["score_pca"] = True
    if regions:
        extra.update(regions=regions, region_blur=opt.region_blur)
    sd.seed_everything(opt.seed)
    t0 = time.time()
    imgs, image_log = sd.generate_image(prompts=[opt.prompt] * opt.num_sampled, negative_prompts=opt.negative,
                                        height=opt.H, width=opt.W, num_inference_steps=opt.steps, grid=opt.make_grid,
                                        guidance_scale=opt.guidance_scale, resampling_steps=opt.resampling_steps,
                                        new_p=opt.new_p, cosine_scale=opt.cosine_scale, rrg_init_weight=opt.rrg_scale,
                                        rrg_stop_t=opt.rrg_stop_t, repaint_sampling=opt.repaint_sampling,
                                        tiled_decoder=opt.tiled_decoder, guidance_rescale=opt.guidance_rescale, **extra)
    torch.cuda.synchronize()
    print(f"Time taken: {time.time() - t0:.2f} seconds")
    if opt.verbose:  # the reference prints its TimeIt table here (ED:1191-1192); ours: GPU phases + host-side time
        for name, ms in sd.phase_times().items():
            print(f"  {name:<14s} {ms / 1e3:9.3f} s (GPU, HIP events)")
        for name, sec in sd.host_s.items():
            print(f"  host:{name:<20s} {sec:9.3f} s")
    save_dir = os.path.join(opt.outdir, opt.exp, f"{datetime.now().strftime('%Y-%m-%d %H:%M:%S')}_{opt.seed}")
    os.makedirs(save_dir, exist_ok=True)
    for i, img in enumerate(imgs):
        img.save(f"{save_dir}/{i}.png")
    if opt.condition_image and opt.process_condition:
        if n_control > 1:
            for n, img in enumerate(extra["condition_image"]):
                img.save(f"{save_dir}/condition_{n}.png")
        else:
            extra["condition_image"].save(f"{save_dir}/condition.png")  # the extracted condition, next to the images
    for key, logged in image_log.items():  # ED:1201-1205: the verbose image log next to the images
        if isinstance(logged, dict):
            for label, img in logged.items():
                img.save(f"{save_dir}/{key}_{label}.png")
        else:
            logged.save(f"{save_dir}/{key}.png")
    with open(f"{save_dir}/args.txt", "w") as f:
        f.write("\n".join(f"{k}: {v}" for k, v in vars(opt).items()))
    print(f"saved {len(imgs)} image(s) to {save_dir}")
    return save_dir


if __name__ == "__main__":
    main()
