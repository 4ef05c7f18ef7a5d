"""Local checkpoint directories: the on-disk format on the input side of the engine.

The reference enters through `DDPMScheduler.from_pretrained(model_id, subfolder="scheduler")` and
`pipeline_func.from_pretrained(model_id, scheduler=scheduler, torch_dtype=weight_dtype, revision="fp16")`
(run_nudity.py:104-122).  There is no network here, so `model_id` must be a LOCAL directory in the diffusers layout:
    unet/config.json             unet/diffusion_pytorch_model.safetensors | .fp16.safetensors | .bin
    vae/config.json              vae/diffusion_pytorch_model.*
    text_encoder/config.json     text_encoder/model.safetensors | pytorch_model.bin
    tokenizer/{vocab.json,merges.txt,...}      (handed to transformers.CLIPTokenizer when the files are there)
    scheduler/scheduler_config.json
and, for the SD-v3 family (run_nudity_sdv3.py:64-72; SD3SafeDenoiserPipeline.from_pretrained):
    transformer/config.json      transformer/diffusion_pytorch_model.* (or shards + *.safetensors.index.json)
    text_encoder{,_2,_3}/        tokenizer{,_2,_3}/
Host logic only (files -> dicts); the engine classes upload the tensors.  Configuration values the engine's plans do not
implement are rejected loudly instead of being ignored.
"""
from __future__ import annotations

import json
import os
from typing import Optional

_WEIGHT_NAMES = ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.fp16.safetensors", "model.safetensors",
                 "model.fp16.safetensors", "diffusion_pytorch_model.bin", "diffusion_pytorch_model.fp16.bin", "pytorch_model.bin",
                 "pytorch_model.fp16.bin")


def read_config(component_dir: str, name: str = "config.json") -> dict:
    path = os.path.join(component_dir, name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: not found (expected a diffusers-layout checkpoint directory)")
    with open(path) as f:
        return json.load(f)


def find_weights(component_dir: str, variant: Optional[str] = None) -> str:
    names = _WEIGHT_NAMES
    if variant:                                                       # e.g. "fp16": prefer the matching files
        names = tuple(n for n in names if f".{variant}." in n) + tuple(n for n in names if f".{variant}." not in n)
    for n in names:
        p = os.path.join(component_dir, n)
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(f"no weight file in {component_dir} (looked for {', '.join(names)})")


def find_index(component_dir: str, variant: Optional[str] = None) -> Optional[str]:
    """The shard index of a component whose weights are split over several safetensors files; None for a single file."""
    names = ("model.safetensors.index.json", "diffusion_pytorch_model.safetensors.index.json")
    if variant:
        names = tuple(n.replace(".index.json", f".index.{variant}.json") for n in names) + names
    for n in names:
        p = os.path.join(component_dir, n)
        if os.path.isfile(p):
            return p
    return None


def load_weights(component_dir: str, variant: Optional[str] = None) -> dict:
    """diffusers-keyed state_dict of one component, as CPU tensors.  A sharded component (`*.safetensors.index.json` with a
    `weight_map`, as SD-v3's two-shard text_encoder_3) is read shard by shard into one dict."""
    index = find_index(component_dir, variant)
    if index is not None:
        from safetensors.torch import load_file
        with open(index) as f:
            weight_map = json.load(f).get("weight_map")
        if not isinstance(weight_map, dict) or not weight_map:
            raise ValueError(f"{index}: no weight_map")
        sd = {}
        for shard in sorted(set(weight_map.values())):
            sp = os.path.join(component_dir, shard)
            if not os.path.isfile(sp):
                raise FileNotFoundError(f"{sp}: shard named by {os.path.basename(index)} is missing")
            part = load_file(sp, device="cpu")
            sd.update({k: v for k, v in part.items() if weight_map.get(k) == shard})
        missing = [k for k in weight_map if k not in sd]
        if missing:
            raise KeyError(f"{index}: {len(missing)} tensors of the weight_map are in no shard, e.g. {missing[:3]}")
        return sd
    path = find_weights(component_dir, variant)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    import torch
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd


def _require(cfg: dict, what: str, **expected):
    for k, v in expected.items():
        if k in cfg and cfg[k] != v and not (isinstance(v, tuple) and cfg[k] in v):
            raise NotImplementedError(f"{what}: config value {k} = {cfg[k]!r} is not implemented by the engine's plan (needs {v!r})")


def unet_kwargs(cfg: dict) -> dict:
    """UNet2DConditionModel(**kwargs) from unet/config.json (the SD-v1.x family)."""
    _require(cfg, "unet", act_fn="silu", use_linear_projection=False, center_input_sample=False, flip_sin_to_cos=True,
             freq_shift=0, downsample_padding=1, mid_block_scale_factor=1, norm_eps=1e-5, dual_cross_attention=False,
             only_cross_attention=False, class_embed_type=None, upcast_attention=False, resnet_time_scale_shift="default",
             mid_block_type="UNetMidBlock2DCrossAttn", time_embedding_type="positional", addition_embed_type=None)
    down = tuple(cfg.get("down_block_types", ()))
    if any(t not in ("CrossAttnDownBlock2D", "DownBlock2D") for t in down):
        raise NotImplementedError(f"unet: down_block_types {down} are not implemented")
    up = tuple(cfg.get("up_block_types", ()))
    if up and tuple("CrossAttnUpBlock2D" if "CrossAttn" in t else "UpBlock2D" for t in reversed(down)) != up:
        raise NotImplementedError(f"unet: up_block_types {up} do not mirror down_block_types {down}")
    ahd = cfg.get("attention_head_dim", 8)
    if not isinstance(ahd, int):
        raise NotImplementedError("unet: per-level attention_head_dim is not implemented")
    keys = ("in_channels", "out_channels", "sample_size", "block_out_channels", "down_block_types", "layers_per_block",
            "attention_head_dim", "cross_attention_dim", "norm_num_groups")
    out = {k: (tuple(cfg[k]) if isinstance(cfg[k], list) else cfg[k]) for k in keys if k in cfg}
    return out


def mmdit_kwargs(cfg: dict, sd35: bool = False, max_width: int = 2048) -> dict:
    """SD3Transformer2DModel(**kwargs) from transformer/config.json (the SD-v3 family; SD3-medium's file).  Without `sd35` the plan
    has no q/k RMS norm and no second attention per block (the SD-3.5 additions); with it, qk_norm = "rms_norm" and a list of
    dual_attention_layers are accepted and returned (SD-3.5-medium's file).  Either way the text projection is as wide as the
    blocks, and that width is at most `max_width`: 2048 unless the caller passes the engine's mmdit.MAX_WIDTH = 2560, which admits
    SD-3.5-large (2432 wide); a width above 2048 must be a multiple of 128 (the wide LayerNorm forms' rule)."""
    dual = cfg.get("dual_attention_layers") or ()
    if not sd35:
        _require(cfg, "transformer", qk_norm=None)
        if dual:
            raise NotImplementedError(f"transformer: config value dual_attention_layers = {cfg['dual_attention_layers']!r} is not "
                                      "implemented by the engine's plan (needs ())")
    else:
        _require(cfg, "transformer", qk_norm=(None, "rms_norm"))
        layers = cfg.get("num_layers", 24)
        if not all(isinstance(i, int) and 0 <= i < layers for i in dual):
            raise NotImplementedError(f"transformer: config value dual_attention_layers = {cfg['dual_attention_layers']!r} is not "
                                      f"implemented by the engine's plan (needs block indices below num_layers = {layers})")
    arch = cfg.get("_class_name")
    if arch is not None and arch != "SD3Transformer2DModel":
        raise NotImplementedError(f"transformer: _class_name = {arch!r} is not implemented (needs 'SD3Transformer2DModel')")
    heads, hd = cfg.get("num_attention_heads", 24), cfg.get("attention_head_dim", 64)
    if "caption_projection_dim" in cfg and cfg["caption_projection_dim"] != heads * hd:
        raise NotImplementedError(f"transformer: config value caption_projection_dim = {cfg['caption_projection_dim']!r} is not "
                                  f"implemented by the engine's plan (needs num_attention_heads * attention_head_dim = {heads * hd})")
    keys = ("in_channels", "out_channels", "sample_size", "patch_size", "num_layers", "num_attention_heads", "attention_head_dim",
            "joint_attention_dim", "pooled_projection_dim", "pos_embed_max_size")
    out = {k: cfg[k] for k in keys if k in cfg}
    if sd35:
        if heads * hd > max_width:
            raise NotImplementedError(f"transformer: width num_attention_heads * attention_head_dim = {heads} * {hd} = {heads * hd} is "
                                      f"not implemented by the engine's plan (needs at most {max_width}; SD-3.5-large is 2432 wide)")
        if heads * hd > 2048 and (heads * hd) % 128:
            raise NotImplementedError(f"transformer: width num_attention_heads * attention_head_dim = {heads} * {hd} = {heads * hd} is "
                                      "not implemented by the engine's plan (a width above 2048 must be a multiple of 128)")
        out.update(qk_norm=cfg.get("qk_norm"), dual_attention_layers=tuple(dual))
    return out


def vae_kwargs(cfg: dict) -> dict:
    _require(cfg, "vae", act_fn="silu")
    keys = ("in_channels", "out_channels", "latent_channels", "block_out_channels", "layers_per_block", "norm_num_groups",
            "sample_size", "scaling_factor", "shift_factor", "use_quant_conv", "use_post_quant_conv")
    out = {k: (tuple(cfg[k]) if isinstance(cfg[k], list) else cfg[k]) for k in keys if k in cfg and cfg[k] is not None}
    return out


def clip_kwargs(cfg: dict) -> dict:
    _require(cfg, "text_encoder", hidden_act="quick_gelu")
    keys = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings")
    return {k: cfg[k] for k in keys if k in cfg}


def clip_projection_kwargs(cfg: dict) -> dict:
    """CLIPTextModelWithProjection(**kwargs) from text_encoder/config.json or text_encoder_2/config.json (SD-v3)."""
    act = cfg.get("hidden_act")
    if act not in ("quick_gelu", "gelu"):
        raise NotImplementedError(f"text_encoder: hidden_act = {act!r} is not implemented by the engine's plan (needs 'quick_gelu' "
                                  "or 'gelu')")
    arch = cfg.get("architectures")
    if arch is not None and list(arch) != ["CLIPTextModelWithProjection"]:
        raise NotImplementedError(f"text_encoder: only architectures = ['CLIPTextModelWithProjection'] is implemented, got {arch!r}")
    for k in ("projection_dim", "eos_token_id"):
        if not isinstance(cfg.get(k), int):
            raise NotImplementedError(f"text_encoder: config value {k} = {cfg.get(k)!r} is not implemented by the engine's plan (needs an integer)")
    heads, hidden = cfg.get("num_attention_heads"), cfg.get("hidden_size")
    if heads is not None and hidden is not None and hidden != 64 * heads:
        raise NotImplementedError(f"text_encoder: hidden_size = {hidden} with {heads} heads is not implemented by the engine's plan "
                                  "(needs heads of 64)")
    _require(cfg, "text_encoder", layer_norm_eps=1e-5, attention_dropout=0.0)
    keys = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings",
            "hidden_act", "projection_dim", "eos_token_id")
    return {k: cfg[k] for k in keys if k in cfg}


def clip_vision_kwargs(cfg: dict) -> dict:
    """CLIPVisionModelWithProjection(**kwargs) from the config.json of a transformers CLIPVisionModelWithProjection, or of a whole
    CLIPModel (its `vision_config`, with the top-level `projection_dim`)."""
    arch = cfg.get("architectures")
    if arch is not None and list(arch) not in (["CLIPVisionModelWithProjection"], ["CLIPModel"]):
        raise NotImplementedError(f"vision tower: only architectures = ['CLIPVisionModelWithProjection'] or ['CLIPModel'] are implemented, "
                                  f"got {arch!r}")
    if isinstance(cfg.get("vision_config"), dict):
        cfg = {**cfg["vision_config"], **({"projection_dim": cfg["projection_dim"]} if "projection_dim" in cfg else {})}
    act = cfg.get("hidden_act")
    if act not in ("quick_gelu", "gelu"):
        raise NotImplementedError(f"vision tower: hidden_act = {act!r} is not implemented by the engine's plan (needs 'quick_gelu' or 'gelu')")
    for k in ("image_size", "patch_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "projection_dim"):
        if not isinstance(cfg.get(k), int):
            raise NotImplementedError(f"vision tower: config value {k} = {cfg.get(k)!r} is not implemented by the engine's plan (needs an integer)")
    if cfg["hidden_size"] not in (64 * cfg["num_attention_heads"], 80 * cfg["num_attention_heads"]):
        raise NotImplementedError(f"vision tower: hidden_size = {cfg['hidden_size']} with {cfg['num_attention_heads']} heads is not "
                                  "implemented by the engine's plan (needs heads of 64 or 80)")
    _require(cfg, "vision tower", layer_norm_eps=1e-5, attention_dropout=0.0, num_channels=3)
    keys = ("image_size", "patch_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "projection_dim",
            "hidden_act")
    return {k: cfg[k] for k in keys}


def clip_model_text_kwargs(cfg: dict) -> dict:
    """CLIPTextModelWithProjection(**kwargs) from the config.json of a whole transformers CLIPModel: its `text_config` with the
    top-level `projection_dim`.  (clip_projection_kwargs stays the reader of a stand-alone text_encoder/config.json.)"""
    arch = cfg.get("architectures")
    if arch is not None and list(arch) != ["CLIPModel"]:
        raise NotImplementedError(f"CLIPModel text tower: only architectures = ['CLIPModel'] is implemented, got {arch!r}")
    if not isinstance(cfg.get("text_config"), dict):
        raise NotImplementedError("CLIPModel text tower: config.json has no text_config")
    t = dict(cfg["text_config"])
    if "projection_dim" in cfg:
        t["projection_dim"] = cfg["projection_dim"]
    t.pop("architectures", None)
    t["architectures"] = ["CLIPTextModelWithProjection"]            # the text half of a CLIPModel is that model's arithmetic
    return clip_projection_kwargs(t)


def t5_kwargs(cfg: dict) -> dict:
    """T5EncoderModel(**kwargs) from text_encoder_3/config.json (T5-v1.1 family, encoder-only use)."""
    if cfg.get("feed_forward_proj") != "gated-gelu":
        raise NotImplementedError(f"text_encoder_3: feed_forward_proj = {cfg.get('feed_forward_proj')!r} is not implemented by the "
                                  "engine's plan (needs 'gated-gelu')")
    if cfg.get("d_kv") != 64:
        raise NotImplementedError(f"text_encoder_3: d_kv = {cfg.get('d_kv')!r} is not implemented by the engine's plan (needs 64)")
    arch = cfg.get("architectures")
    if cfg.get("is_decoder") or (arch is not None and list(arch) != ["T5EncoderModel"]):
        raise NotImplementedError(f"text_encoder_3: only the encoder-only use (architectures = ['T5EncoderModel']) is implemented, "
                                  f"got architectures = {arch!r}, is_decoder = {cfg.get('is_decoder')!r}")
    _require(cfg, "text_encoder_3", dense_act_fn="gelu_new", is_gated_act=True)
    keys = ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets",
            "relative_attention_max_distance", "layer_norm_epsilon")
    return {k: cfg[k] for k in keys if k in cfg}


def load_tokenizer(model_dir: str, subfolder: str = "tokenizer"):
    """transformers.CLIPTokenizer from `tokenizer/` (SD-v3: also `tokenizer_2/`) when its vocabulary files exist, or
    transformers.T5TokenizerFast from a folder that holds a sentencepiece model instead (SD-v3's `tokenizer_3/`); None otherwise
    (pass tokenizer=...)."""
    d = os.path.join(model_dir, subfolder)
    if os.path.isfile(os.path.join(d, "vocab.json")) and os.path.isfile(os.path.join(d, "merges.txt")):
        from transformers import CLIPTokenizer
        return CLIPTokenizer.from_pretrained(d)
    if os.path.isfile(os.path.join(d, "spiece.model")):
        from transformers import T5TokenizerFast
        return T5TokenizerFast.from_pretrained(d)
    return None
