"""Host side of an SD-v3 job (no GPU): transformer/config.json -> SD3Transformer2DModel kwargs, the flow scheduler from
scheduler/scheduler_config.json, the SD-v3 drivers' two-phase parsers, their erase ids, and the repellency arguments for a scheduler
that has no beta table (run_nudity_sdv3.py:34-39,252-262,433-525)."""
import json
from types import SimpleNamespace

import pytest
import torch

from safe_denoiser_amd import checkpoint, driver
from safe_denoiser_amd.schedulers import DDPMScheduler, FlowMatchEulerDiscreteScheduler

# transformer/config.json of stabilityai/stable-diffusion-3-medium-diffusers, as published
SD3_MEDIUM_JSON = {"_class_name": "SD3Transformer2DModel", "_diffusers_version": "0.29.0.dev0", "attention_head_dim": 64,
                   "caption_projection_dim": 1536, "in_channels": 16, "joint_attention_dim": 4096, "num_attention_heads": 24,
                   "num_layers": 24, "out_channels": 16, "patch_size": 2, "pooled_projection_dim": 2048, "pos_embed_max_size": 192,
                   "sample_size": 128}
SD3_SCHEDULER_JSON = {"_class_name": "FlowMatchEulerDiscreteScheduler", "_diffusers_version": "0.29.0.dev0",
                      "num_train_timesteps": 1000, "shift": 3.0}


def test_mmdit_kwargs_maps_the_sd3_medium_file(tmp_path):
    (tmp_path / "transformer").mkdir()
    (tmp_path / "transformer" / "config.json").write_text(json.dumps(SD3_MEDIUM_JSON))
    kw = checkpoint.mmdit_kwargs(checkpoint.read_config(str(tmp_path / "transformer")))
    assert kw == dict(in_channels=16, out_channels=16, sample_size=128, patch_size=2, num_layers=24, num_attention_heads=24,
                      attention_head_dim=64, joint_attention_dim=4096, pooled_projection_dim=2048, pos_embed_max_size=192)
    # keys the later SD-3.5 files carry, at the values this plan implements, change nothing
    assert checkpoint.mmdit_kwargs(dict(SD3_MEDIUM_JSON, qk_norm=None, dual_attention_layers=[])) == kw


@pytest.mark.parametrize("key,value", [("qk_norm", "rms_norm"), ("dual_attention_layers", [0]), ("caption_projection_dim", 1024)])
def test_mmdit_kwargs_refuses_what_the_plan_does_not_implement(key, value):
    with pytest.raises(NotImplementedError, match=key):
        checkpoint.mmdit_kwargs(dict(SD3_MEDIUM_JSON, **{key: value}))


@pytest.mark.parametrize("shift", [3.0, 1.0])
def test_flow_scheduler_from_pretrained_follows_the_files_shift(tmp_path, shift):
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(SD3_SCHEDULER_JSON, shift=shift)))
    got = FlowMatchEulerDiscreteScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    want = FlowMatchEulerDiscreteScheduler(num_train_timesteps=1000, shift=shift)
    assert got.config.shift == shift and got.config.num_train_timesteps == 1000
    got.set_timesteps(4)
    want.set_timesteps(4)
    assert torch.equal(got.sigmas, want.sigmas) and torch.equal(got.timesteps, want.timesteps) and got.sigmas.shape == (5,)
    other = FlowMatchEulerDiscreteScheduler(shift=4.0 - shift)
    other.set_timesteps(4)
    assert not torch.equal(got.sigmas, other.sigmas)


def test_flow_scheduler_from_pretrained_refusals(tmp_path):
    (tmp_path / "scheduler").mkdir()
    path = tmp_path / "scheduler" / "scheduler_config.json"
    path.write_text(json.dumps(dict(SD3_SCHEDULER_JSON, use_dynamic_shifting=True)))
    with pytest.raises(NotImplementedError, match="use_dynamic_shifting"):
        FlowMatchEulerDiscreteScheduler.from_pretrained(str(tmp_path))
    path.write_text(json.dumps(dict(SD3_SCHEDULER_JSON, _class_name="PNDMScheduler")))
    with pytest.raises(NotImplementedError, match="PNDMScheduler"):
        FlowMatchEulerDiscreteScheduler.from_pretrained(str(tmp_path))
    path.write_text(json.dumps(dict(SD3_SCHEDULER_JSON, use_dynamic_shifting=False)))
    assert FlowMatchEulerDiscreteScheduler.from_pretrained(str(tmp_path)).config.shift == 3.0
    with pytest.raises(FileNotFoundError):
        FlowMatchEulerDiscreteScheduler.from_pretrained(str(tmp_path), subfolder="no_such_folder")


def test_parse_sd3_args_layers(tmp_path):
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({}))
    a = driver.parse_sd3_args(["--config", str(cfg)])
    assert a.guidance_scale == 3.5 and a.category == "all" and a.erase_id == "std" and a.image_length == 512
    assert driver.parse_args(["--config", str(cfg)]).guidance_scale == 7.5                  # the SD-v1.4 parser keeps its default
    # the JSON supplies defaults; the category comes from its key "nudity", not "category"
    cfg.write_text(json.dumps({"nudity": "nudity", "category": "all", "guidance_scale": 5.0, "erase_id": "safree_neg_prompt_rep_time",
                               "save_dir": "./out", "num_inference_steps": 28}))
    a = driver.parse_sd3_args(["--config", str(cfg)])
    assert (a.category, a.guidance_scale, a.erase_id, a.save_dir, a.num_inference_steps) == \
        ("nudity", 5.0, "safree_neg_prompt_rep_time", "./out", 28)
    # the command line overrides the JSON
    a = driver.parse_sd3_args(["--config", str(cfg), "--guidance_scale", "2.5", "--category", "all", "--erase_id", "std", "--save-dir", "x"])
    assert (a.category, a.guidance_scale, a.erase_id, a.save_dir, a.num_inference_steps) == ("all", 2.5, "std", "x", 28)
    with pytest.raises(SystemExit):
        driver.parse_sd3_args(["--config", str(cfg), "--category", "coco"])


def test_parse_sd3_coco_args(tmp_path):
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"nudity": "nudity"}))
    a = driver.parse_sd3_coco_args(["--config", str(cfg)])
    assert a.guidance_scale == 3.5 and a.category == "coco"
    assert driver.parse_coco_args(["--config", str(cfg)]).guidance_scale == 7.5
    cfg.write_text(json.dumps({"category": "coco_open_clip", "guidance_scale": 4.0}))
    a = driver.parse_sd3_coco_args(["--config", str(cfg), "--guidance_scale", "6"])
    assert a.guidance_scale == 6.0 and a.category == "coco_open_clip"


def test_sd3_erase_ids_are_the_references_three():
    assert set(driver.SD3_ERASE_IDS) == {"std", "safree_neg_prompt", "safree_neg_prompt_rep_time"}
    assert driver.SD3_ERASE_IDS == {"std": (False, False), "safree_neg_prompt": (True, False),
                                    "safree_neg_prompt_rep_time": (True, True)}


def test_repellency_kwargs_for_a_scheduler_without_betas():
    task = {"repellency": {"method": "kernel_fast", "n_embed": 4, "guidance_scale": 7.5, "params": {"scale": 0.03, "proj_ref_path": "p.pt"}}}
    flow = FlowMatchEulerDiscreteScheduler()
    kw = driver.repellency_kwargs(task, 28, flow)
    assert kw == dict(name="kernel_fast", num_timesteps=28, max_idx=None, beta_min=None, beta_max=None, n_embed=4, scheduler=flow,
                      scale=0.03, proj_ref_path="p.pt")
    ddpm = DDPMScheduler()
    kw = driver.repellency_kwargs(task, 50, ddpm)
    assert kw == dict(name="kernel_fast", num_timesteps=50, max_idx=1000, beta_min=0.00085, beta_max=0.012, n_embed=4, scheduler=ddpm,
                      scale=0.03, proj_ref_path="p.pt")


def test_run_job_refuses_an_sd14_only_erase_id_on_an_sd3_pipeline(tmp_path):
    pipe = SimpleNamespace(family="sd3")
    args = SimpleNamespace(erase_id="sld_rep_time")
    with pytest.raises(KeyError, match="sld_rep_time"):
        driver.run_job(args, pipe)
