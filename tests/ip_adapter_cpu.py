"""torch-CPU restatement of ``ed_u8_to_clip_input``'s operation sequence (test infrastructure, never shipped).

Held to two bars: bit equality with the kernel on the GPU (tests/test_ip_adapter_gpu.py) and 1e-6 absolute against
``transformers.CLIPImageProcessor()`` on the CPU (tests/test_ip_adapter.py).  Values reach 2.7, where an fp32 ulp is 2.4e-7: the
second bar is four ulps of op-order freedom and nothing more.
"""
import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def resize_size(H, W, size=224):
    """transformers' shortest-edge rule: the short side becomes ``size``, the long side int(size * long / short)"""
    short, long = (H, W) if H <= W else (W, H)
    new_long = int(size * long / short)
    return (size, new_long) if H <= W else (new_long, size)


def pil_resize(u8, size=224):
    """uint8 [H,W,3] array -> Pillow's bicubic resize to ``resize_size`` (the bytes ``ops.resize_u8`` reproduces on the device)"""
    from PIL import Image
    H, W = u8.shape[:2]
    h, w = resize_size(H, W, size)
    return np.asarray(Image.fromarray(u8).resize((w, h), resample=Image.BICUBIC))


def u8_to_clip_input(u8, size=224, mean=CLIP_MEAN, std=CLIP_STD):
    """uint8 [H,W,3] tensor (both sides >= size) -> fp32 [1,3,size,size], the kernel's operations in its order:
    centre crop at ((H - size) // 2, (W - size) // 2); x = fp32(fp64(v) * (1 / 255)); (x - mean_c) / std_c in fp32."""
    u8 = torch.as_tensor(u8)
    H, W = u8.shape[:2]
    y0, x0 = (H - size) // 2, (W - size) // 2
    crop = u8[y0:y0 + size, x0:x0 + size].permute(2, 0, 1)
    x = (crop.to(torch.float64) * (1.0 / 255.0)).to(torch.float32)
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    return ((x - m) / s)[None].contiguous()
