"""CPU restatement of DESIGN.md section 23 (LoRA adapters merged into the weights), independent of the package:

  * ``merged_fp64`` / ``magnitude``: the merged weight in fp64 and the magnitude its fp32 error bound is stated against;
  * ``coefficient``: c = f32(scale) * (f32(alpha) / f32(r));
  * ``sgm_name``: this file's own map from a module path of the UNet to the SGM (original LDM) block name kohya's SDXL files use;
  * writers of every key spelling: each takes [(root, module path, up, down, alpha | None)] and returns a state dict for
    ``safetensors.torch.save_file``.

Factors are stated on the NCHW weight: up [N, r] (or [N, r, 1, 1]), down [r, Cin] / [r, Cin, kh, kw].
"""
import numpy as np
import torch


def coefficient(scale, alpha, r):
    a = np.float32(r) if alpha is None else np.float32(alpha)
    return np.float32(np.float32(scale) * np.float32(a / np.float32(r)))


def _mats(weight_shape, up, down):
    """(up [N, r], down [r, K]) in fp64, K in NCHW (logical) order"""
    N = weight_shape[0]
    r = up.shape[1]
    return up.reshape(N, r).double(), down.reshape(r, -1).double()


def merged_fp64(base, adapters):
    """base: the weight in its logical shape ([N, K] or [N, Cin, kh, kw]); adapters: [(up, down, c)] -> fp64 tensor of base's shape:
    f64(base) + sum_j c_j * up_j @ down_j"""
    out = base.double().reshape(base.shape[0], -1).clone()
    for up, down, c in adapters:
        u, d = _mats(base.shape, up, down)
        out += float(c) * (u @ d)
    return out.reshape(base.shape)


def magnitude(base, adapters):
    """|base| + sum_j |c_j| * (|up_j| @ |down_j|), fp64, base's shape"""
    out = base.double().abs().reshape(base.shape[0], -1).clone()
    for up, down, c in adapters:
        u, d = _mats(base.shape, up, down)
        out += abs(float(c)) * (u.abs() @ d.abs())
    return out.reshape(base.shape)


def fp32_bound(base, adapters):
    """Elementwise bound on |W_fp32 - merged_fp64|: (r_max + J + 2) * 2^-24 * magnitude -- r products summed in fp32 (each step one
    rounding), J scaled terms summed, one add to the base, with a unit of slack; the standard forward bound of recursive sums."""
    r_max = max([a[0].shape[1] for a in adapters], default=0)
    return (r_max + len(adapters) + 2) * 2.0 ** -24 * magnitude(base, adapters)


# ---- SGM block names ---------------------------------------------------------------------------------------------------------
def sgm_name(path, cfg):
    """Module path of this repo's UNet -> kohya's flattened SGM name (without the ``lora_unet_`` prefix), from the configuration's
    ``layers_per_block`` / ``attn`` / number of blocks.  Written from the layout of the original UNet: ``input_blocks`` = conv_in,
    then per down block its layers and (all but the last block) a downsampler; ``middle_block`` = resnet, transformer, resnet;
    ``output_blocks`` = per up block layers_per_block + 1 layers, the upsampler appended to the block's last layer."""
    L, attn, n = cfg["layers_per_block"], list(cfg["attn"]), len(cfg["block_out_channels"])
    p = path.split(".")
    res = {"conv1": "in_layers_2", "conv2": "out_layers_3", "time_emb_proj": "emb_layers_1", "conv_shortcut": "skip_connection"}
    top = {"conv_in": "input_blocks_0_0", "conv_out": "out_2", "time_embedding.linear_1": "time_embed_0",
           "time_embedding.linear_2": "time_embed_2", "add_embedding.linear_1": "label_emb_0_0", "add_embedding.linear_2": "label_emb_0_2"}
    if path in top:
        return top[path]
    if p[0] == "down_blocks":
        b = int(p[1])
        first = 1 + b * (L + 1)                    # every earlier block has L layers and one downsampler
        if p[2] == "downsamplers":
            return f"input_blocks_{first + L}_0_op"
        i = first + int(p[3])
        if p[2] == "resnets":
            return f"input_blocks_{i}_0_{res[p[4]]}"
        return f"input_blocks_{i}_1_{'_'.join(p[4:])}"
    if p[0] == "mid_block":
        if p[1] == "resnets":
            return f"middle_block_{2 * int(p[2])}_{res[p[3]]}"
        return f"middle_block_1_{'_'.join(p[3:])}"
    if p[0] == "up_blocks":
        b = int(p[1])
        has_attn = attn[::-1][b]
        if p[2] == "upsamplers":
            return f"output_blocks_{b * (L + 1) + L}_{2 if has_attn else 1}_conv"
        i = b * (L + 1) + int(p[3])
        if p[2] == "resnets":
            return f"output_blocks_{i}_0_{res[p[4]]}"
        return f"output_blocks_{i}_1_{'_'.join(p[4:])}"
    raise KeyError(path)


# ---- writers -----------------------------------------------------------------------------------------------------------------
def _alpha(sd, key, alpha):
    if alpha is not None:
        sd[key] = torch.tensor(float(alpha))


def write_peft(entries):
    """diffusers / PEFT: <root>.<module>.lora_A.weight (down) / .lora_B.weight (up) [/ .alpha]"""
    sd = {}
    for root, path, up, down, alpha in entries:
        sd[f"{root}.{path}.lora_A.weight"], sd[f"{root}.{path}.lora_B.weight"] = down.contiguous(), up.contiguous()
        _alpha(sd, f"{root}.{path}.alpha", alpha)
    return sd


def write_legacy(entries):
    """diffusers legacy: <root>.<module>.lora.down.weight / .lora.up.weight; text encoders: ....lora_linear_layer.down.weight"""
    sd = {}
    for root, path, up, down, alpha in entries:
        mid = "lora" if root == "unet" else "lora_linear_layer"
        sd[f"{root}.{path}.{mid}.down.weight"], sd[f"{root}.{path}.{mid}.up.weight"] = down.contiguous(), up.contiguous()
        _alpha(sd, f"{root}.{path}.alpha", alpha)
    return sd


def processor_key(path):
    """<attn>.to_q -> <attn>.processor.to_q_lora ; <attn>.to_out.0 -> <attn>.processor.to_out_lora ; None for other modules"""
    for proj, name in ((".to_q", "to_q_lora"), (".to_k", "to_k_lora"), (".to_v", "to_v_lora"), (".to_out.0", "to_out_lora")):
        if path.endswith(proj):
            return f"{path[:-len(proj)]}.processor.{name}"
    return None


def write_processor(entries):
    """diffusers legacy attention-processor form (attention projections only)"""
    sd = {}
    for root, path, up, down, alpha in entries:
        key = processor_key(path)
        assert root == "unet" and key is not None, path
        sd[f"unet.{key}.down.weight"], sd[f"unet.{key}.up.weight"] = down.contiguous(), up.contiguous()
    return sd


KOHYA_PREFIX = {"unet": "lora_unet_", "text_encoder": "lora_te_", "text_encoder_2": "lora_te2_"}


def write_kohya(entries, xl=False, sgm_cfg=None):
    """kohya: lora_unet_<flattened path>.lora_down.weight / .lora_up.weight / .alpha; ``xl``: text encoders as lora_te1_ / lora_te2_;
    ``sgm_cfg``: spell the UNet's modules in SGM block names of that configuration"""
    sd = {}
    for root, path, up, down, alpha in entries:
        prefix = "lora_te1_" if (xl and root == "text_encoder") else KOHYA_PREFIX[root]
        flat = sgm_name(path, sgm_cfg) if (sgm_cfg is not None and root == "unet") else path.replace(".", "_")
        sd[f"{prefix}{flat}.lora_down.weight"], sd[f"{prefix}{flat}.lora_up.weight"] = down.contiguous(), up.contiguous()
        _alpha(sd, f"{prefix}{flat}.alpha", alpha)
    return sd


def random_factors(weight_shape, r, seed, dtype=torch.float32, conv_up_4d=True):
    """(up, down) for a weight of that logical shape: up [N, r] ([N, r, 1, 1] for a convolution), down [r, *weight_shape[1:]]"""
    g = torch.Generator().manual_seed(seed)
    N = weight_shape[0]
    up = torch.randn(N, r, generator=g) * 0.3
    down = torch.randn(r, *weight_shape[1:], generator=g) * 0.3
    if len(weight_shape) == 4 and conv_up_4d:
        up = up.reshape(N, r, 1, 1)
    return up.to(dtype), down.to(dtype)
