"""The Inception-v3 pool3 tower of FID and KID: `InceptionV3([3])(batch)[0]` of pytorch-fid as the reference vendors it
(evaluations/utils/inception.py:16-163 -- torchvision's Inception3 trunk with the FID patches of :197-341 -- built by
evaluations/utils/fid.py:203-215), executed by libsdn (sdn_inception_create / sdn_inception_forward): pixels in [0, 1] -> f32
[B, 2048].  Neither torchvision nor torchmetrics is needed.

fp32 storage only, exact f32 products on the f32-input matrix cores (sdn_gemm_f32): pytorch-fid runs fp32 and FID is quoted to
two decimals.  Every BasicConv2d (conv without bias, BatchNorm eps 1e-3, ReLU) is one GEMM with a bias + ReLU epilogue: the norm is
folded into the weight and a bias HERE, when packing, in float64 and rounded to f32 once (`fold_conv_bn`).

    tower = InceptionV3.from_pretrained("pt_inception-2015-12-05-6726825d.pth")       # a LOCAL file; nothing is downloaded
    feats = tower(images)                    # uint8 [B, H, W, 3] or float [B, 3, H, W] in [0, 1]  ->  f32 [B, 2048]
    feats = tower.get_activations(pil_images, batch_size=50)                          # the reference's get_activations

Not verified here: the real checkpoint is not on the machine this was written on; parity is measured on synthetic weights against
a float64 restatement of the trunk (tests_support/inception_oracle.py).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._model import EngineModel
from .clip_vision import resize_rect_u8

BN_EPS = 1e-3                                                      # torchvision's BasicConv2d: BatchNorm2d(eps=0.001)
FEATURES = 2048


def fold_conv_bn(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """BatchNorm folded into its convolution, in float64: (w * s[:, None, None, None], beta - mean * s) with
    s = gamma / sqrt(var + eps).  w [O, I, kh, kw]; the rest [O].  Returns float64 tensors (round them once)."""
    f64 = lambda t: t.detach().to(torch.float64)
    s = f64(gamma) / torch.sqrt(f64(var) + eps)
    return f64(w) * s[:, None, None, None], f64(beta) - f64(mean) * s


def resize_bilinear(x: torch.Tensor, size, scale: float = 1.0, shift: float = 0.0) -> torch.Tensor:
    """sdn_resize_bilinear_f32: scale * F.interpolate(x, size, mode="bilinear", align_corners=False) + shift of an f32 GPU tensor
    [B, 3, H, W], as an NHWC tensor [B, size[0], size[1], 3].  No antialiasing (not Pillow's resample)."""
    _lib.require_gpu()
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_cuda:
        raise _lib.SdnError(f"x must be an f32 GPU tensor [B, 3, H, W], got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    oh, ow = (int(v) for v in size)
    out = torch.empty((x.shape[0], oh, ow, 3), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().sdn_resize_bilinear_f32(x.data_ptr(), x.shape[0], x.shape[2], x.shape[3], oh, ow, float(scale), float(shift),
                                                  out.data_ptr(), _lib.stream_ptr()), "sdn_resize_bilinear_f32")
    return out


class InceptionV3(EngineModel):
    CHUNK = 32                 # images per plan invocation: the largest patch matrix is then 0.89 GB, every operand below 2 GiB

    def __init__(self, resize_input: bool = True, normalize_input: bool = True, image_size: int = 299):
        """pytorch-fid's arguments.  resize_input: inputs of any size are resized to image_size x image_size on the engine
        (F.interpolate bilinear, align_corners=False); without it inputs must already be image_size x image_size.  normalize_input:
        the trunk sees 2 x - 1.  image_size: 299 for FID; the trunk is fully convolutional and runs on any square side >= 75."""
        self.dtype, self.precision = torch.float32, "fp32"
        self.resize_input, self.normalize_input = bool(resize_input), bool(normalize_input)
        self.config = SimpleNamespace(image_size=int(image_size), resize_input=self.resize_input, normalize_input=self.normalize_input,
                                      features=FEATURES)
        self._create("sdn_inception_create", _lib.InceptionConfig(image_size=int(image_size), normalize_input=int(self.normalize_input),
                                                                  dtype=2))
        info = _lib.InceptionConv()
        self.convs = []
        for i in range(_lib.lib().sdn_inception_conv_count(self._h)):
            _lib.check(_lib.lib().sdn_inception_conv_info(self._h, i, C.byref(info)), "sdn_inception_conv_info")
            self.convs.append(dict(name=info.name.decode(), **{k: getattr(info, k) for k in ("cin", "cout", "kh", "kw", "stride", "pad_h",
                                                                                            "pad_w", "kpad", "n_padded")}))
        self._conv_by_key = {c["name"] + ".conv.weight": c for c in self.convs}

    # ---- packing: the BatchNorm fold ---------------------------------------------------------------------------------------
    def _source_shape(self, p: dict) -> tuple:
        c = self._conv_by_key.get(p["name"])
        return (c["cout"], c["cin"], c["kh"], c["kw"]) if c else (p["rows"],)

    def _pack(self, sd: dict, device) -> torch.Tensor:
        """Extra keys (fc.*, AuxLogits.*, *.num_batches_tracked) are ignored.  Per BasicConv2d the `conv.weight` region receives the
        folded weight [cout][kpad] in (ky, kx, c) column order and the `bn.bias` region the folded bias; `bn.weight`,
        `bn.running_mean` and `bn.running_var` are stored as given (no kernel reads them)."""
        missing = [p["name"] for p in self.manifest if p["name"] not in sd]
        if missing:
            raise KeyError(f"state_dict lacks {len(missing)} keys, e.g. {missing[:3]}")
        for p in self.manifest:
            if tuple(sd[p["name"]].shape) != self._source_shape(p):
                raise _lib.SdnError(f"{p['name']}: expected shape {self._source_shape(p)}, got {tuple(sd[p['name']].shape)}")
        by_name = {p["name"]: p for p in self.manifest}
        buf = torch.zeros(self.weight_bytes, dtype=torch.uint8, device=device)
        for c in self.convs:
            n = c["name"]
            w, b = fold_conv_bn(sd[n + ".conv.weight"], sd[n + ".bn.weight"], sd[n + ".bn.bias"], sd[n + ".bn.running_mean"],
                                sd[n + ".bn.running_var"])
            w = w.permute(0, 2, 3, 1).reshape(c["cout"], -1).to(torch.float32)                 # the one rounding
            w = torch.nn.functional.pad(w, (0, c["kpad"] - w.shape[1]))
            self._store(buf, by_name[n + ".conv.weight"], w.to(device))
            self._store(buf, by_name[n + ".bn.bias"], b.to(torch.float32).to(device))
            for k in (".bn.weight", ".bn.running_mean", ".bn.running_var"):
                self._store(buf, by_name[n + k], sd[n + k].detach().to(torch.float32).to(device))
        return buf

    def synthetic_state_dict(self, seed: int = 1234) -> dict:
        """Random weights of this architecture: conv weights U(+-sqrt(6 / fan_in)) (variance-preserving under ReLU), BatchNorm gains
        in 1 +- 0.1, biases and running means in +-0.1, running variances in [0.5, 1.5]."""
        g = torch.Generator().manual_seed(seed)
        sd = {}
        for name, shape in self.state_dict_shapes().items():
            r = torch.rand(shape, generator=g)
            if len(shape) == 4:
                sd[name] = (2 * r - 1) * (6.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
            elif name.endswith("running_var"):
                sd[name] = 0.5 + r
            else:
                sd[name] = (1.0 if name.endswith("bn.weight") else 0.0) + 0.2 * (r - 0.5)
        return sd

    def load_synthetic_on_device(self, seed: int = 1234, device="cuda"):
        return self.load_state_dict(self.synthetic_state_dict(seed), device)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda", **kwargs):
        """A LOCAL `.pth` (pytorch-fid's pt_inception-2015-12-05 state_dict) or `.safetensors` file with the same keys."""
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path)
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        m = cls(**kwargs)
        m.load_state_dict(sd, device)
        return m

    # ---- forward -------------------------------------------------------------------------------------------------------------
    def forward(self, images: torch.Tensor) -> torch.Tensor:
        """f32 [B, 2048] of uint8 [B, H, W, 3] (ToTensor's u8 / 255 is applied) or float [B, 3, H, W] in [0, 1]."""
        _lib.require_gpu()
        if self._weights is None:
            raise _lib.SdnError("no weights loaded: call load_state_dict() first")
        dev = self._weights.device
        x = images
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise _lib.SdnError("images must be a uint8 [B, H, W, 3] or float [B, 3, H, W] tensor")
        if x.dtype == torch.uint8:
            if x.shape[-1] != 3:
                raise _lib.SdnError(f"uint8 images must be [B, H, W, 3], got {tuple(x.shape)}")
            x = x.to(dev).permute(0, 3, 1, 2).to(torch.float32) / 255.0          # transforms.ToTensor
        elif not x.is_floating_point() or x.shape[1] != 3:
            raise _lib.SdnError(f"float images must be [B, 3, H, W], got {x.dtype} {tuple(x.shape)}")
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        b, h, w = x.shape[0], x.shape[2], x.shape[3]
        s = self.config.image_size
        if not self.resize_input and (h, w) != (s, s):
            raise _lib.SdnError(f"resize_input=False takes {s} x {s} images, got {h} x {w}")
        out = torch.empty((b, FEATURES), dtype=torch.float32, device=dev)
        for lo in range(0, b, self.CHUNK):                          # consecutive chunks on the same stream
            nb = min(self.CHUNK, b - lo)
            ws = self._workspace(nb, dev)
            _lib.check(_lib.lib().sdn_inception_forward(self._h, _lib.dptr(self._weights), x[lo:lo + nb].data_ptr(), out[lo:lo + nb].data_ptr(),
                                                        nb, h, w, 1 if self.resize_input else 0, _lib.dptr(ws), ws.numel(), _lib.stream_ptr()),
                       "sdn_inception_forward")
        return out

    __call__ = forward

    def get_activations(self, images, batch_size: int = 50, size=(256, 256)) -> torch.Tensor:
        """evaluations/utils/fid.py:71-129 on the engine: every image through `Resize((256, 256))` (Pillow's bilinear resample on the
        uint8 image: sdn_image_resize_rect_u8, bit for bit), ToTensor and the tower.  images: a list of PIL images (any sizes) or a
        uint8 tensor [B, H, W, 3].  size = (299, 299) is KID's transform (base_image.py:99-101).  Returns f32 [N, 2048] on the device
        (the reference returns float64 numpy of the same values)."""
        _lib.require_gpu()
        dev = self._weights.device if self._weights is not None else "cuda"
        if isinstance(images, torch.Tensor):
            groups = [images[lo:lo + batch_size] for lo in range(0, images.shape[0], max(int(batch_size), 1))]
        else:
            groups, run = [], []
            for im in list(images):                                  # runs of equally sized images, at most batch_size long
                a = np.asarray(im.convert("RGB"), dtype=np.uint8)
                if run and (run[-1].shape != a.shape or len(run) >= batch_size):
                    groups.append(torch.from_numpy(np.stack(run)))
                    run = []
                run.append(a)
            if run:
                groups.append(torch.from_numpy(np.stack(run)))
        feats = [self.forward(resize_rect_u8(g.to(dev), size, "bilinear")) for g in groups]
        return torch.cat(feats) if feats else torch.empty((0, FEATURES), dtype=torch.float32, device=dev)
