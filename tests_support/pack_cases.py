"""The eight engine handles at the smallest configurations the host tests construct, for tests/test_pack_digests.py and
tests/golden/make_pack_digests.py: how each is built, the prefixed / aliased key forms its packer accepts, and the digests taken
of it (packed bytes, manifest, source shapes; on the GPU the manifest regions of the synthetic device weights)."""
import hashlib

import torch

from safe_denoiser_amd import checkpoint
from tests_support import clip_proj_oracle, clip_vision_oracle, t5_oracle

SEED = 1234
SMALL_UNET = dict(text_len=5, block_out_channels=(64, 64), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), layers_per_block=1,
                  attention_head_dim=1, cross_attention_dim=64, sample_size=8, norm_num_groups=32)
SMALL_MMDIT = dict(text_len=45, sample_size=16, num_layers=3, num_attention_heads=4, joint_attention_dim=128, pooled_projection_dim=64,
                   pos_embed_max_size=24)
SMALL_VAE = dict(block_out_channels=(64, 128), layers_per_block=1, sample_size=16)
SMALL_VAE_NOQUANT = dict(SMALL_VAE, latent_channels=16, use_quant_conv=False, use_post_quant_conv=False)
SMALL_CLIP = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                  max_position_embeddings=77)


def _unet(**kw):
    from safe_denoiser_amd.unet import UNet2DConditionModel
    return UNet2DConditionModel(**SMALL_UNET, **kw)


def _mmdit():
    from safe_denoiser_amd.mmdit import SD3Transformer2DModel
    return SD3Transformer2DModel(**SMALL_MMDIT)


def _vae(role="decoder", cfg=SMALL_VAE):
    from safe_denoiser_amd.vae import AutoencoderKL
    return AutoencoderKL(_role=role, **cfg)


def _clip():
    from safe_denoiser_amd.clip import CLIPTextModel
    return CLIPTextModel(precision="bf16x3", **SMALL_CLIP)


def _clip_proj():
    from safe_denoiser_amd.clip import CLIPTextModelWithProjection
    cfg = clip_proj_oracle.load_golden()["b/cfg"]                       # the fixture's gelu arm
    assert cfg["hidden_act"] == "gelu"
    return CLIPTextModelWithProjection(dtype=torch.float16, clip_skip=1, **checkpoint.clip_projection_kwargs(cfg))


def _t5():
    from safe_denoiser_amd.t5 import T5EncoderModel
    return T5EncoderModel(**dict(t5_oracle.load_golden()["cfg"]))


def _vision():
    from safe_denoiser_amd.clip_vision import CLIPVisionModelWithProjection
    return CLIPVisionModelWithProjection(**checkpoint.clip_vision_kwargs(clip_vision_oracle.load_golden()["cfg"]))


def _extra(sd):
    """No alias exists for these keys: what the packer accepts beyond the plain dict is keys it does not know."""
    return dict(sd, **{"not.a.parameter": torch.zeros(1)})


def _prefixed(prefix, keep=()):
    return lambda sd: {(k if k in keep else prefix + k): v for k, v in sd.items()}


_DEPRECATED = (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn"))


def _vae_on_disk(sd):
    """The SD-v1.4 checkpoint's form: deprecated attention names, their linears stored as 1x1 convs."""
    out = {}
    for k, v in sd.items():
        if "attentions" in k:
            for new, old in _DEPRECATED:
                k = k.replace("." + new + ".", "." + old + ".")
            if k.endswith("weight") and v.dim() == 2:
                v = v.reshape(*v.shape, 1, 1)
        out[k] = v
    return out


def _t5_shared(sd):
    out = {"encoder." + k: v for k, v in sd.items() if k != "embed_tokens.weight"}
    out["shared.weight"] = sd["embed_tokens.weight"]
    return out


# name -> (factory, alias form of a canonical state_dict)
CASES = {
    "unet_bf16": (_unet, _extra),
    "unet_fp32": (lambda: _unet(dtype=torch.float32), _extra),
    "unet_bf16x3": (lambda: _unet(precision="bf16x3"), _extra),
    "mmdit": (_mmdit, _extra),
    "vae_decoder": (_vae, _vae_on_disk),
    "vae_encoder": (lambda: _vae("encoder"), _vae_on_disk),
    "vae_decoder_noquant": (lambda: _vae(cfg=SMALL_VAE_NOQUANT), _vae_on_disk),
    "clip": (_clip, _prefixed("text_model.")),
    "clip_proj": (_clip_proj, _prefixed("text_model.", keep=("text_projection.weight",))),
    "t5": (_t5, _t5_shared),
    "vision": (_vision, _prefixed("vision_model.", keep=("visual_projection.weight",))),
}


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def manifest_digest(m) -> str:
    return hashlib.sha256(repr([(p["name"], p["kind"], p["rows"], p["cols"], p["offset"]) for p in m.manifest]).encode()).hexdigest()


def shapes_digest(m) -> str:
    return hashlib.sha256(repr([(k, tuple(v)) for k, v in m.state_dict_shapes().items()]).encode()).hexdigest()


def region_bytes(m, p: dict) -> int:
    """Packed size of one manifest entry: f32 vectors, matrices in the storage type."""
    return p["rows"] * 4 if p["cols"] == 0 else p["rows"] * p["cols"] * torch.empty((), dtype=m.dtype).element_size()


P_GLU_VALUE, P_GLU_GATE = 7, 8


def regions(m, buf: torch.Tensor) -> list:
    """The bytes of every manifest entry of a packed buffer (engine-derived regions and padding are left out).  The two halves of a
    T5 gated weight interleave in blocks of 16 rows from the value entry's offset on: that pair is taken as one region."""
    out = []
    for p in m.manifest:
        if p["kind"] != P_GLU_GATE:
            out.append(buf[p["offset"]:p["offset"] + region_bytes(m, p) * (2 if p["kind"] == P_GLU_VALUE else 1)])
    return out


def regions_digest(m, buf: torch.Tensor) -> str:
    return sha(torch.cat([r.cpu() for r in regions(m, buf)]))
