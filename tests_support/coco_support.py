"""What the COCO CLIP-score evaluator's host tests, GPU tests and tools/clip_vith_bench.py share: seeded weights for a CLIP tower's
manifest, a deterministic test image, and Pillow's resize-then-crop as the reference of clip_preprocess_any."""
import numpy as np
import torch
from PIL import Image

from safe_denoiser_amd import clip_vision as V


def device_state_dict(m, seed):
    """Seeded weights of a tower's manifest (vision or projected text), generated on the GPU and held at the tower's storage
    precision."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for name, shape in m.state_dict_shapes().items():
        if name.endswith("class_embedding"):
            sd[name] = 0.3 * torch.randn(shape, generator=g, device="cuda").to(m.dtype).float()
        elif len(shape) == 1:
            norm = "norm" in name
            base = 1.0 if (norm and name.endswith("weight")) else 0.0
            sd[name] = base + (0.2 if norm else 0.1) * (torch.rand(shape, generator=g, device="cuda") - 0.5)
        elif "embedding" in name and "patch" not in name:
            sd[name] = (0.3 * torch.randn(shape, generator=g, device="cuda")).to(m.dtype)
        else:
            fan_in = int(np.prod(shape[1:]))
            amp = (3.0 / fan_in) ** 0.5 * (2.0 if ".q_proj." in name else 1.0)
            sd[name] = ((torch.rand(shape, generator=g, device="cuda") * 2 - 1) * amp).to(m.dtype)
    return sd


def sample_image(h, w, seed):
    """uint8 [h, w, 3]: smooth gradients (so that a shifted crop or a wrong tap shows) under seeded noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    smooth = np.stack([127 + 127 * np.sin(x / 7.0), 255.0 * y / h, 127 + 127 * np.cos((x + y) / 11.0)], -1)
    return np.clip(smooth + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def pillow_crop(img, size, crop):
    """Pillow's bicubic resize of the shortest side to `size`, then the centre crop by the named library's rule."""
    h, w = img.shape[:2]
    rh, rw = V.resized_shape(h, w, size)
    top, left = V.crop_offset(rh, size, crop), V.crop_offset(rw, size, crop)
    full = np.asarray(Image.fromarray(img).resize((rw, rh), Image.BICUBIC))
    return np.ascontiguousarray(full[top:top + size, left:left + size])
