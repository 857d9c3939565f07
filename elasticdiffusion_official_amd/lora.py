"""LoRA adapters, merged into the weights.

An adapter file names low-rank pairs (``up`` [N, r], ``down`` [r, K]) for some of the Linear / Conv2d weights of the UNet and the
CLIP text encoders.  They are added into those weights ONCE -- diffusers' ``fuse_lora`` form -- so the forward, its kernels, its
dispatch rules and its captured graphs stay exactly what they are:

    W = rn( f32(base) + sum_j c_j * up_j @ down_j ),     c_j = f32(scale_j) * (f32(alpha_j) / f32(r_j)),  alpha_j = r_j without one

always from a kept copy of the untouched weight (one rounding; scale 0 or unloading gives the original bits back), by ONE
``ed_lora_merge`` launch per model over a descriptor table of all its touched tensors.

  ``read_lora``   file or state dict -> [LoraTarget(root, path, up, down, alpha)], every key consumed or an error; the key
                  spellings of diffusers / PEFT, legacy diffusers (incl. attention-processor names), kohya, and kohya SDXL in SGM
                  block names (``sgm_blocks`` maps those from ``models.unet_config``, not from a table of one architecture)
  ``plan``        validation of the targets against the modules (CPU / meta tensors suffice): shapes, ranks, memory order
  ``LoraState``   what a pipeline holds: pristine bases, fp32 factors on the device, the table, the merge
"""
import os
import re
from collections import namedtuple

import numpy as np
import torch

ROOTS = ("unet", "text_encoder", "text_encoder_2")

LoraTarget = namedtuple("LoraTarget", "root path up down alpha")

_UNSUPPORTED = ("dora_scale", "hada_", "lokr_", "lora_mid", "lora_magnitude_vector")
_KOHYA_ROOTS = (("lora_unet_", "unet"), ("lora_te1_", "text_encoder"), ("lora_te2_", "text_encoder_2"), ("lora_te_", "text_encoder"))
_DOTTED_SUFFIXES = ((".lora_A.weight", "down"), (".lora_B.weight", "up"), (".lora.down.weight", "down"), (".lora.up.weight", "up"),
                    (".lora_linear_layer.down.weight", "down"), (".lora_linear_layer.up.weight", "up"), (".alpha", "alpha"))
_PROCESSOR = re.compile(r"^(.*)\.processor\.(to_q|to_k|to_v|to_out)_lora\.(down|up)\.weight$")
_SGM_RESNET = {"in_layers_2": "conv1", "out_layers_3": "conv2", "emb_layers_1": "time_emb_proj", "skip_connection": "conv_shortcut"}
_SGM_TOP = {"time_embed_0": "time_embedding.linear_1", "time_embed_2": "time_embedding.linear_2",
            "label_emb_0_0": "add_embedding.linear_1", "label_emb_0_2": "add_embedding.linear_2",
            "input_blocks_0_0": "conv_in", "out_2": "conv_out"}


# ---- names ---------------------------------------------------------------------------------------------------------------
def lora_modules(module):
    """{module path: module} of what an adapter may target: the Linear and Conv2d layers"""
    return {n: m for n, m in module.named_modules() if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d))}


def flat_names(module):
    """{path with '.' -> '_': path} over ``lora_modules`` -- how kohya spells a module.  Two paths that flatten to the same string
    are an error, not a guess."""
    out = {}
    for name in lora_modules(module):
        flat = name.replace(".", "_")
        if flat in out:
            raise RuntimeError(f"LoRA: module paths {out[flat]!r} and {name!r} both flatten to {flat!r}")
        out[flat] = name
    return out


def sgm_blocks(cfg):
    """{(section, index, sub): (kind, module path)} of a UNet configuration (``models.unet_config``) in the block numbering of the
    original (SGM / LDM) UNet: ``input_blocks`` counts conv_in, then every layer of every down block and the downsampler after it;
    ``output_blocks`` every layer of every up block, whose last sub-module is the upsampler.  kind: resnet | attention | down | up."""
    layers, attn = int(cfg["layers_per_block"]), tuple(cfg["attn"])
    n = len(cfg["block_out_channels"])
    out = {}
    idx = 1
    for b in range(n):
        for l in range(layers):
            out[("input_blocks", idx, 0)] = ("resnet", f"down_blocks.{b}.resnets.{l}")
            if attn[b]:
                out[("input_blocks", idx, 1)] = ("attention", f"down_blocks.{b}.attentions.{l}")
            idx += 1
        if b < n - 1:
            out[("input_blocks", idx, 0)] = ("down", f"down_blocks.{b}.downsamplers.0.conv")
            idx += 1
    out[("middle_block", 0, None)] = ("resnet", "mid_block.resnets.0")
    out[("middle_block", 1, None)] = ("attention", "mid_block.attentions.0")
    out[("middle_block", 2, None)] = ("resnet", "mid_block.resnets.1")
    idx = 0
    rattn = attn[::-1]
    for b in range(n):
        for l in range(layers + 1):
            out[("output_blocks", idx, 0)] = ("resnet", f"up_blocks.{b}.resnets.{l}")
            if rattn[b]:
                out[("output_blocks", idx, 1)] = ("attention", f"up_blocks.{b}.attentions.{l}")
            if l == layers and b < n - 1:
                out[("output_blocks", idx, 2 if rattn[b] else 1)] = ("up", f"up_blocks.{b}.upsamplers.0.conv")
            idx += 1
    return out


_SGM_NAME = re.compile(r"^(?:(input_blocks|output_blocks)_(\d+)_(\d+)|(middle_block)_(\d+))_(.+)$")


def sgm_to_flat(name, cfg):
    """A kohya name in SGM block names -> the flattened name of this repo's module, or None when ``name`` is not SGM-spelled.
    A block the configuration does not have, or an inner name its kind does not have, raises."""
    if name in _SGM_TOP:
        return _SGM_TOP[name].replace(".", "_")
    m = _SGM_NAME.match(name)
    if m is None:
        return None
    if m.group(1):
        key, rest = (m.group(1), int(m.group(2)), int(m.group(3))), m.group(6)
    else:
        key, rest = ("middle_block", int(m.group(5)), None), m.group(6)
    hit = sgm_blocks(cfg).get(key)
    if hit is None:
        raise RuntimeError(f"LoRA: {name!r} names a block this UNet does not have")
    kind, path = hit
    flat = path.replace(".", "_")
    if kind == "resnet":
        if rest not in _SGM_RESNET:
            raise RuntimeError(f"LoRA: {name!r}: no such layer in a residual block")
        return f"{flat}_{_SGM_RESNET[rest]}"
    if kind in ("down", "up"):
        if rest != ("op" if kind == "down" else "conv"):
            raise RuntimeError(f"LoRA: {name!r}: no such layer in a {kind}sampler")
        return flat
    return f"{flat}_{rest}"   # attention: proj_in, proj_out, transformer_blocks_i_... are spelled as here


# ---- files -----------------------------------------------------------------------------------------------------------------
def _load(source):
    if isinstance(source, dict):
        return dict(source), "<state dict>"
    from safetensors.torch import load_file
    return load_file(os.fspath(source)), os.fspath(source)


def parse_keys(state_dict):
    """-> {(root, spelling, name): {"up": t, "down": t, "alpha": t}}; spelling is "dotted" (a module path) or "flat" (kohya).  Every
    key lands in a group or the call raises; the variants that are not plain LoRA raise NotImplementedError naming the key."""
    groups, unknown = {}, []
    for key, t in state_dict.items():
        if any(u in key for u in _UNSUPPORTED):
            raise NotImplementedError(f"LoRA key {key!r}: DoRA / LoHa / LoKr / Tucker (lora_mid) adapters are not supported")
        if key.endswith((".diff", ".diff_b", ".w_norm", ".b_norm", ".bias")):
            raise NotImplementedError(f"LoRA key {key!r}: bias and normalisation-layer differences are not supported")
        slot = None
        for prefix, root in _KOHYA_ROOTS:
            if key.startswith(prefix):
                name, _, suffix = key[len(prefix):].partition(".")
                part = {"lora_down.weight": "down", "lora_up.weight": "up", "alpha": "alpha"}.get(suffix)
                if part is not None and name:
                    slot = ((root, "flat", name), part)
                break
        else:
            root = next((r for r in sorted(ROOTS, key=len, reverse=True) if key.startswith(r + ".")), None)
            if root is not None:
                rest = key[len(root) + 1:]
                m = _PROCESSOR.match(rest)
                if m is not None:
                    proj = "to_out.0" if m.group(2) == "to_out" else m.group(2)
                    slot = ((root, "dotted", f"{m.group(1)}.{proj}"), m.group(3))
                else:
                    for suffix, part in _DOTTED_SUFFIXES:
                        if rest.endswith(suffix) and len(rest) > len(suffix):
                            slot = ((root, "dotted", rest[:-len(suffix)]), part)
                            break
        if slot is None:
            unknown.append(key)
            continue
        group = groups.setdefault(slot[0], {})
        if slot[1] in group:
            raise RuntimeError(f"LoRA key {key!r}: a second spelling of a tensor the file already carries")
        group[slot[1]] = t
    if unknown:
        raise RuntimeError(f"LoRA: {len(unknown)} keys are not in a known spelling, e.g. {unknown[:3]}")
    return groups


def resolve(root, spelling, name, names, flats, unet_cfg=None):
    """Module path of one target.  ``names`` = ``lora_modules(target)``, ``flats`` = ``flat_names(target)``."""
    sep = "." if spelling == "dotted" else "_"
    tries = [name]
    if root == "unet":
        if spelling == "flat" and unet_cfg is not None:
            tries = [sgm_to_flat(name, unet_cfg) or name]
    else:
        # adapter files spell the HF CLIP modules with the ``text_model`` wrapper; transformers versions differ in whether the
        # model class keeps that level, so a name is looked up as written, then without / with it
        wrapper = "text_model" + sep
        tries.append(name[len(wrapper):] if name.startswith(wrapper) else wrapper + name)
    for n in tries:
        if spelling == "dotted" and n in names:
            return n
        if spelling == "flat" and n in flats:
            return flats[n]
    raise RuntimeError(f"LoRA: {root} has no Linear / Conv2d module {'spelled ' if spelling == 'flat' else ''}{name!r}")


def read_lora(source, targets, unet_cfg=None, text_encoder=True):
    """-> [LoraTarget] in the order of the source's keys.  ``source``: a ``*.safetensors`` path or a state dict; ``targets``: {root: module} for the roots
    that exist (a key of a root that is absent raises -- with ``text_encoder=False`` the text-encoder keys are dropped instead);
    ``unet_cfg``: the UNet's ``models.unet_config`` (resolves kohya names in SGM block spelling)."""
    sd, where = _load(source)
    groups = parse_keys(sd)
    tables = {}
    out, seen = [], {}
    for (root, spelling, name), g in groups.items():
        if root != "unet" and not text_encoder:
            continue
        if root not in targets or targets[root] is None:
            raise RuntimeError(f"{where}: keys for {root} (e.g. {name!r}) but this pipeline has no such model to merge them into"
                               + ("; pass text_encoder=False to drop them" if root != "unet" else ""))
        if root not in tables:
            tables[root] = (lora_modules(targets[root]), flat_names(targets[root]))
        path = resolve(root, spelling, name, *tables[root], unet_cfg=unet_cfg)
        if "up" not in g or "down" not in g:
            raise RuntimeError(f"{where}: {root}.{path} has {sorted(g)} but needs both up and down")
        if (root, path) in seen:
            raise RuntimeError(f"{where}: {name!r} and {seen[(root, path)]!r} both name {root}.{path}")
        seen[(root, path)] = name
        alpha = g.get("alpha")
        out.append(LoraTarget(root, path, g["up"], g["down"], None if alpha is None else float(alpha)))
    return out


# ---- validation and layout ---------------------------------------------------------------------------------------------------
def _trim(shape):
    shape = list(shape)
    while len(shape) > 1 and shape[-1] == 1:
        shape.pop()
    return shape


def weight_order(w):
    """"contiguous" | "channels_last": the physical order of a weight that is dense as [N, K]; anything else raises."""
    if w.is_contiguous():
        return "contiguous"
    if w.dim() == 4 and w.is_contiguous(memory_format=torch.channels_last):
        return "channels_last"
    raise RuntimeError(f"weight of shape {tuple(w.shape)} and strides {tuple(w.stride())} is dense in neither contiguous nor "
                       "channels-last order")


def coefficient(scale, alpha, r):
    """c = f32(scale) * (f32(alpha) / f32(r)), alpha = r when the file carries none"""
    alpha = np.float32(r if alpha is None else alpha)
    return np.float32(scale) * (alpha / np.float32(r))


def factors(t, weight):
    """(up [N, r], down [r, K]) of one target as fp32 matrices, ``down`` re-laid into the weight's physical K order; raises on a rank
    or shape mismatch.  The up-cast from a 16-bit file is exact."""
    N = weight.shape[0]
    where = f"{t.root}.{t.path}"
    if t.up.dim() < 2 or t.down.dim() < 2 or _trim(t.up.shape) != _trim(t.up.shape[:2]) or t.up.shape[1] < 1:
        raise RuntimeError(f"LoRA {where}: up has shape {tuple(t.up.shape)}, expected [{N}, r] (or [{N}, r, 1, 1])")
    r = int(t.up.shape[1])
    if t.down.shape[0] != r:
        raise RuntimeError(f"LoRA {where}: rank mismatch, up {tuple(t.up.shape)} against down {tuple(t.down.shape)}")
    # the factor's trailing extents are the weight's; extents of 1 may be written or left out (a Linear's [r, in, 1, 1], a 1x1 conv's [r, C])
    if t.up.shape[0] != N or _trim(t.down.shape) != _trim([r] + list(weight.shape[1:])):
        raise RuntimeError(f"LoRA {where}: up {tuple(t.up.shape)} / down {tuple(t.down.shape)} do not fit the weight "
                           f"{tuple(weight.shape)}")
    if weight.numel() >= 2 ** 31:
        raise RuntimeError(f"LoRA {where}: the weight has {weight.numel()} elements; the merge kernel indexes below 2^31")
    try:
        order = weight_order(weight)
    except RuntimeError as e:
        raise RuntimeError(f"LoRA {where}: {e}") from None
    up = t.up.reshape(N, r).to(torch.float32)
    down = t.down.reshape(r, *weight.shape[1:]).to(torch.float32)
    if order == "channels_last":
        down = down.permute(0, 2, 3, 1)
    return up.contiguous(), down.reshape(r, -1).contiguous()


def plan(targets_read, targets):
    """[(LoraTarget, weight Parameter, up [N, r] f32, down [r, K] f32)] for every target, on the factors' own device (the host):
    everything that can be refused is refused here, before the first byte of a weight is written."""
    out = []
    mods = {root: lora_modules(m) for root, m in targets.items() if m is not None}
    for t in targets_read:
        w = mods[t.root][t.path].weight
        if w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise RuntimeError(f"LoRA {t.root}.{t.path}: weights of dtype {w.dtype} cannot be merged")
        up, down = factors(t, w)
        out.append((t, w, up, down))
    return out


# ---- state of one pipeline ---------------------------------------------------------------------------------------------------
class LoraTable:
    """The descriptor table of one ``ed_lora_merge`` launch (layout: include/elastic_hip.h): ``host`` int64 on the CPU, ``dev`` its
    copy on the device (None until ``upload``), and the counts the entry point takes."""

    TILE_N, TILE_K = 64, 128

    def __init__(self, tensors):
        """tensors: [(base, dst, [(up, down, c), ...])] -- base / dst dense tensors of one dtype and shape, up [N, r] / down [r, K] fp32
        on the device, c a float; N = base.shape[0], K = the rest of base in its physical order."""
        from .ops import _DTYPE
        words, arecs, tile = [], [], 0
        self.keep = []
        for base, dst, adapters in tensors:
            N = int(base.shape[0])
            K = base.numel() // N
            words += [base.data_ptr(), dst.data_ptr(), N, K, _DTYPE.get(dst.dtype, -1), len(arecs) // 4,
                      len(arecs) // 4 + len(adapters), tile]
            tile += -(-N // self.TILE_N) * -(-K // self.TILE_K)
            for up, down, c in adapters:
                arecs += [up.data_ptr(), down.data_ptr(), int(up.shape[1]), int(np.float32(c).view(np.uint32))]
            self.keep.append((base, dst, adapters))
        self.n_tensors, self.n_adapters, self.n_tiles = len(tensors), len(arecs) // 4, tile
        self.host = torch.tensor(words + arecs, dtype=torch.int64)
        self.dev = None
        self.flops = sum(2.0 * b.numel() * int(u.shape[1]) for b, _, ads in tensors for u, _, _ in ads)
        self.nbytes = sum(2.0 * b.numel() * b.element_size() for b, _, _ in tensors)

    def upload(self, device):
        self.dev = self.host.to(device)   # the one host-to-device copy of a change of LoRA state
        return self


class LoraState:
    """Adapters of one pipeline: ``targets`` {root: module}.  Pristine copies exist only for touched tensors, on the device, and
    go when the last adapter touching a tensor is unloaded."""

    def __init__(self, targets, device, unet_cfg=None):
        self.targets, self.device, self.unet_cfg = targets, device, unet_cfg
        self.adapters = []   # load order: {"name", "scale", "items": [(root, weight, up, down, alpha, r)]}
        self.bases = {}      # id(weight) -> (root, weight, pristine clone)

    def listing(self):
        return [(a["name"], a["scale"], len(a["items"])) for a in self.adapters]

    def _pick(self, name):
        if name is None:
            return list(self.adapters)
        hit = [a for a in self.adapters if a["name"] == name]
        if not hit:
            raise KeyError(f"no LoRA adapter named {name!r}; loaded: {[a['name'] for a in self.adapters]}")
        return hit

    def load(self, source, scale=1.0, name=None, text_encoder=True):
        if name is None:
            name = os.path.splitext(os.path.basename(os.fspath(source)))[0] if not isinstance(source, dict) else f"lora{len(self.adapters)}"
        if any(a["name"] == name for a in self.adapters):
            raise ValueError(f"a LoRA adapter named {name!r} is already loaded")
        scale = float(scale)
        if not np.isfinite(np.float32(scale)):
            raise ValueError(f"LoRA scale must be finite, got {scale}")
        read = read_lora(source, self.targets, self.unet_cfg, text_encoder)
        planned = plan(read, self.targets)            # every refusal happens above this line
        items, fresh = [], []
        for t, w, up, down in planned:
            if id(w) not in self.bases:
                self.bases[id(w)] = (t.root, w, w.detach().clone(memory_format=torch.preserve_format))
                fresh.append(id(w))
            items.append((t.root, w, up.to(self.device), down.to(self.device), t.alpha, int(up.shape[1])))
        self.adapters.append({"name": name, "scale": scale, "items": items})
        try:
            return name, self.merge({t.root for t in read})
        except Exception:
            # the launch was refused (no device, a table the entry point rejects): nothing was written, so nothing stays loaded
            self.adapters.pop()
            for k in fresh:
                del self.bases[k]
            raise

    def set_scale(self, scale, name=None):
        scale = float(scale)
        if not np.isfinite(np.float32(scale)):
            raise ValueError(f"LoRA scale must be finite, got {scale}")
        roots = set()
        for a in self._pick(name):
            a["scale"] = scale
            roots |= {it[0] for it in a["items"]}
        return self.merge(roots)

    def unload(self, name=None):
        gone = self._pick(name)
        roots = {it[0] for a in gone for it in a["items"]}
        self.adapters = [a for a in self.adapters if not any(a is g for g in gone)]
        written = self.merge(roots)                  # tensors no adapter touches any more are restored by the copy path
        live = {id(it[1]) for a in self.adapters for it in a["items"]}
        for k in [k for k in self.bases if k not in live]:
            del self.bases[k]
        return written

    def table(self, root):
        """The table of one model: every tensor with a pristine copy, each with its active adapters (c != 0) in load order."""
        rows = {key: (base, w.detach(), []) for key, (r, w, base) in self.bases.items() if r == root}
        for a in self.adapters:
            for it in a["items"]:
                if it[0] == root:
                    c = coefficient(a["scale"], it[4], it[5])
                    if c != 0:
                        rows[id(it[1])][2].append((it[2], it[3], float(c)))
        return LoraTable(list(rows.values())) if rows else None

    def merge(self, roots):
        """One launch per model in ``roots`` with touched tensors; returns the roots whose weights were written, after dropping the
        derived-weight caches of those models (the kernel writes through a raw pointer: no Parameter's version moves)."""
        from . import ops
        written = []
        for root in ROOTS:
            if root not in roots:
                continue
            table = self.table(root)
            if table is None:
                continue
            ops.lora_merge(table.upload(self.device))
            for m in self.targets[root].modules():
                m.__dict__.pop("_derived", None)
            written.append(root)
        return written
