"""An SD-v3 job from a checkpoint directory through the driver (run_nudity_sdv3.py, run_coco30k_sdv3.py on the engine):
`SD3SafeDenoiserPipeline.from_pretrained`, one guidance scale per prompt, the `std` class (`safree=False`), `driver.run_job` with the
three SD-v3 erase ids and `driver.build_repellency` on the SD-v3 pipeline.

Configurations are the smallest the suite already has, imported and not edited: the MMDiT `SMALL` of tests/test_gpu_mmdit.py (latent
side 16, 3 layers) at text_len 333, the two projected CLIPs and their tokenizers of tests/test_gpu_clip_proj.py, FakeT5Tokenizer, the
16-channel two-level VAE of test_sd3_call_ends_like_the_reference_with_a_vae, 4 inference steps.  The text widths are those of
tests/test_gpu_clip_proj.py's own end-to-end test: its two CLIPs are 128 wide each, and SD3TextFrontEnd refuses CLIP columns wider
than the T5's d_model, so the T5 is that file's `_tiny_t5` (d_model 256) and not the d_model-128 fixture of tests/test_gpu_t5.py;
the MMDiT reads joint_attention_dim 256 and pooled_projection_dim 64 + 128.  The from_pretrained test alone writes a FOUR-level VAE:
it asserts 128 x 128 images at image_length 128, which a latent of side 16 reaches through three upsamplers."""
import json
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

import tests.test_gpu_clip_proj as tcp
import tests.test_gpu_mmdit as tm
from oracle import repellency as orp
from safe_denoiser_amd import _lib, clip_vision as V, driver
from safe_denoiser_amd.mmdit import SD3Transformer2DModel
from safe_denoiser_amd.pipeline_sd3 import SD3_NEGATIVE_PROMPT_SPACE, SD3SafeDenoiserPipeline, StableDiffusion3PipelineOutput
from safe_denoiser_amd.repellency import repellency_methods_fast_sdv3 as sd3rep
from safe_denoiser_amd.schedulers import FlowMatchEulerDiscreteScheduler
from safe_denoiser_amd.text_sd3 import SD3TextFrontEnd
from safe_denoiser_amd.vae import SD3_VAE_CONFIG, AutoencoderKL
from tests_support.t5_oracle import FakeT5Tokenizer

pytestmark = pytest.mark.gpu
DT = torch.float16
STEPS = 4
MMDIT = {**tm.SMALL, "joint_attention_dim": 256, "pooled_projection_dim": 192}
VAE2 = dict(SD3_VAE_CONFIG, block_out_channels=(64, 128), layers_per_block=1, sample_size=32)               # latent 16 -> 32 x 32
VAE4 = dict(SD3_VAE_CONFIG, block_out_channels=(64, 64, 128, 128), layers_per_block=1, sample_size=128)     # latent 16 -> 128 x 128
T5_JSON = dict(architectures=["T5EncoderModel"], vocab_size=512, d_model=256, d_kv=64, d_ff=256, num_layers=2, num_heads=2,
               relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6,
               feed_forward_proj="gated-gelu", dense_act_fn="gelu_new", is_gated_act=True)
PROMPTS = ["a lustful portrait in oil", "two cats asleep on a red sofa in the evening sun", "a photo of a fisherman at dawn"]
JOINED = ", ".join(SD3_NEGATIVE_PROMPT_SPACE)


# ------------------------------------------------------------------------------------------------ shared, read-only
@pytest.fixture(scope="module")
def mmdit_sd():
    return SD3Transformer2DModel(text_len=333, dtype=DT, **MMDIT).synthetic_state_dict(5)


def tokenizers():
    k1, k2 = tcp._tokenizers()
    return k1, k2, FakeT5Tokenizer(vocab_size=512)


def front_end():
    k1, k2, k3 = tokenizers()
    return SD3TextFrontEnd(tcp._tiny_t5(DT), k3, text_encoder=tcp.small("a", DT), tokenizer=k1, text_encoder_2=tcp.small("b", DT), tokenizer_2=k2)


class Recording:
    """A front end that notes which of the three calls the pipeline makes and hands them to the engine's front end."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def encode_prompt(self, prompt=None, negative_prompt=None, **kw):
        self.calls.append(("encode_prompt", list(prompt), list(negative_prompt)))
        return self.inner.encode_prompt(prompt=prompt, negative_prompt=negative_prompt, **kw)

    def masked_encode_prompt(self, prompt):
        self.calls.append(("masked", prompt))
        return self.inner.masked_encode_prompt(prompt)

    def encode_negative_prompt_space(self, phrases):
        self.calls.append(("space", list(phrases)))
        return self.inner.encode_negative_prompt_space(phrases)


class SpyPipeline(SD3SafeDenoiserPipeline):
    """Notes the keywords of every call (what run_job hands over) and runs it."""

    def __call__(self, *a, **kw):
        self.seen = getattr(self, "seen", [])
        self.seen.append(dict(kw, prompt=list(a[0]) if a else kw.get("prompt")))
        return super().__call__(*a, **kw)


@pytest.fixture(scope="module")
def mmdit(mmdit_sd):
    m = SD3Transformer2DModel(text_len=333, dtype=DT, **MMDIT)
    m.load_state_dict(mmdit_sd)
    return m


@pytest.fixture(scope="module")
def vae2():
    v = AutoencoderKL(dtype=DT, **VAE2)
    v.load_state_dict(v.synthetic_state_dict(6, with_encoder=True))      # the encoder half: build_repellency's embed_fn
    return v


@pytest.fixture(scope="module")
def proj_ref_path(tmp_path_factory):
    """A 12-row channel-normalised reference set of the latent shape, as a proj_ref cache file."""
    refs = orp.channel_normalise(torch.randn(12, 16, 16, 16, generator=torch.Generator().manual_seed(4)))
    path = str(tmp_path_factory.mktemp("refs") / "proj_ref.pt")
    torch.save(refs, path)
    return path


def fast_sdv3(path):
    return sd3rep.get_repellency_method("kernel_fast", torch.zeros(1, device="cuda"), None, None, STEPS, None, None, None, n_embed=4,
                                        proj_ref_path=path, cache_proj_ref=True, scale=0.03)


def tape(P, seed=3):
    t = torch.randn(P, 1, 16, 16, 16, generator=torch.Generator().manual_seed(seed))
    return lambda p, shape: t[p].clone()


# ------------------------------------------------------------------------------------------------ 1. from_pretrained
def _write_checkpoint(root, sds):
    """A diffusers-layout SD-v3 directory: safetensors everywhere, the transformer in two shards behind an index file."""
    from safetensors.torch import save_file
    tjson = {**MMDIT, "_class_name": "SD3Transformer2DModel", "in_channels": 16, "out_channels": 16, "patch_size": 2, "attention_head_dim": 64,
             "caption_projection_dim": MMDIT["num_attention_heads"] * 64, "sample_size": 128}             # sample_size: the file's, not the run's
    parts = (("transformer", tjson, sds["mmdit"], None),
             ("vae", dict(VAE4, act_fn="silu", sample_size=1024, _class_name="AutoencoderKL"), sds["vae4"], "diffusion_pytorch_model.safetensors"),
             ("text_encoder", dict(tcp.G["a/cfg"], architectures=["CLIPTextModelWithProjection"]), sds["clip_a"], "model.safetensors"),
             ("text_encoder_2", dict(tcp.G["b/cfg"], architectures=["CLIPTextModelWithProjection"]), sds["clip_b"], "model.safetensors"),
             ("text_encoder_3", T5_JSON, {"encoder." + k: v for k, v in sds["t5"].items()}, "model.safetensors"))
    for sub, cfg, sd, fname in parts:
        os.makedirs(os.path.join(root, sub))
        with open(os.path.join(root, sub, "config.json"), "w") as f:
            json.dump({k: (list(x) if isinstance(x, tuple) else x) for k, x in cfg.items()}, f)
        sd = {k: t.contiguous() for k, t in sd.items()}
        if fname is not None:
            save_file(sd, os.path.join(root, sub, fname))
            continue
        keys = sorted(sd)
        shards = {"diffusion_pytorch_model-00001-of-00002.safetensors": keys[0::2], "diffusion_pytorch_model-00002-of-00002.safetensors": keys[1::2]}
        for name, ks in shards.items():
            save_file({k: sd[k] for k in ks}, os.path.join(root, sub, name))
        with open(os.path.join(root, sub, "diffusion_pytorch_model.safetensors.index.json"), "w") as f:
            json.dump({"metadata": {}, "weight_map": {k: name for name, ks in shards.items() for k in ks}}, f)
    os.makedirs(os.path.join(root, "scheduler"))
    with open(os.path.join(root, "scheduler", "scheduler_config.json"), "w") as f:
        json.dump({"_class_name": "FlowMatchEulerDiscreteScheduler", "num_train_timesteps": 1000, "shift": 3.0}, f)


def test_from_pretrained_equals_the_hand_assembled_pipeline(tmp_path, mmdit_sd, proj_ref_path):
    state_dicts = dict(mmdit=mmdit_sd, vae4=AutoencoderKL(dtype=DT, **VAE4).synthetic_state_dict(6), t5=tcp._tiny_t5(DT).synthetic_state_dict(9),
                       clip_a=tcp.O.golden_state_dict(tcp.G, "a"), clip_b=tcp.O.golden_state_dict(tcp.G, "b"))
    root = str(tmp_path / "sd3")
    _write_checkpoint(root, state_dicts)
    k1, k2, k3 = tokenizers()
    pipe = SD3SafeDenoiserPipeline.from_pretrained(root, tokenizer=k1, tokenizer_2=k2, tokenizer_3=k3, image_length=128, revision="fp16")
    assert pipe.family == "sd3" and pipe.to("cuda") is pipe
    assert pipe.transformer.dtype == DT and pipe.transformer.config.sample_size == 16 and pipe.transformer.text_len == 333
    assert pipe.transformer_hi is None and pipe.scheduler.config.shift == 3.0 and pipe.vae.config.latent_channels == 16
    assert isinstance(pipe.text_front_end, SD3TextFrontEnd) and pipe.text_front_end.d_model == 256
    prompts = PROMPTS[:2]
    kw = dict(num_inference_steps=STEPS, guidance_scale=3.5)
    out = pipe(prompts, noise_fn=tape(2), return_latents=True, **kw)
    assert tuple(out.shape) == (2, 16, 16, 16) and bool(torch.isfinite(out).all())
    # the same stack built by hand from the same state dicts
    m = SD3Transformer2DModel(text_len=333, dtype=DT, **MMDIT); m.load_state_dict(state_dicts["mmdit"])
    v = AutoencoderKL(dtype=DT, **VAE4); v.load_state_dict(state_dicts["vae4"])
    hand = SD3SafeDenoiserPipeline(m, FlowMatchEulerDiscreteScheduler(shift=3.0), vae=v, text_front_end=front_end())
    assert torch.equal(out, hand(prompts, noise_fn=tape(2), return_latents=True, **kw))
    res = pipe(prompts, noise_fn=tape(2), return_latents=False, output_type="pil", height=128, width=128, **kw)
    assert isinstance(res, StableDiffusion3PipelineOutput) and len(res.images) == 2 and res.images[0].size == (128, 128)
    want = hand(prompts, noise_fn=tape(2), return_latents=False, output_type="pil", **kw).images
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(res.images, want))
    with pytest.raises(_lib.SdnError):
        pipe(prompts, height=512, width=512, **kw)                                      # the plan is built for image_length
    # the two-plan form: fp16 everywhere, bf16x3 over the same weights inside the repellency window
    sched = SD3SafeDenoiserPipeline.from_pretrained(root, tokenizer=k1, tokenizer_2=k2, tokenizer_3=k3, image_length=128, precision="scheduled")
    assert sched.transformer.dtype == torch.float16 and sched.transformer_hi.precision == "bf16x3" and sched.precision_schedule == {"window": True}
    proc = fast_sdv3(proj_ref_path)
    lat = sched(prompts, noise_fn=tape(2), repellency_processor=proc, **kw)
    assert sched.last_stats["hi_steps"] == sched.last_stats["window_steps"] > 0 and bool(torch.isfinite(lat).all())
    sched(prompts, noise_fn=tape(2), **kw)
    assert sched.last_stats["hi_steps"] == sched.last_stats["window_steps"] == 0        # no processor, no window
    # no tokenizers, given or on disk: the embeddings-only pipeline
    bare = SD3SafeDenoiserPipeline.from_pretrained(root, image_length=128, precision="bf16x3")
    assert bare.text_front_end is None and bare.transformer.precision == "bf16x3"
    with pytest.raises(NotImplementedError):
        bare(prompts, **kw)
    pe, ne, pp, npp = pipe.text_front_end.encode_prompt(prompt=prompts, negative_prompt=[JOINED] * 2)
    x3 = bare(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=pp, negative_pooled_prompt_embeds=npp, noise_fn=tape(2), **kw)
    assert bool(torch.isfinite(x3).all())
    with pytest.raises(FileNotFoundError, match="not a local directory"):
        SD3SafeDenoiserPipeline.from_pretrained(str(tmp_path / "stabilityai" / "stable-diffusion-3-medium-diffusers"))


# ------------------------------------------------------------------------------------------------ 2. one guidance scale per prompt
def _embeds(P, seed=7):
    g = torch.Generator().manual_seed(seed)
    return dict(prompt_embeds=torch.randn(2 * P, 333, 256, generator=g).cuda(), pooled_prompt_embeds=torch.randn(2 * P, 192, generator=g).cuda())


@pytest.mark.parametrize("with_processor", [False, True])
def test_per_prompt_guidance_rows_equal_the_scalar_calls(mmdit, proj_ref_path, with_processor):
    """Row p of a call with scales [g0, g1, g2] = row p of the scalar call with g_p at the same batch shape, bit for bit: no kernel
    of the loop reduces across samples.  With the processor the re-noise comes from the global generator, seeded before each call."""
    P, scales = 3, [2.0, 3.5, 7.0]
    pipe = SD3SafeDenoiserPipeline(mmdit, FlowMatchEulerDiscreteScheduler())
    proc = fast_sdv3(proj_ref_path) if with_processor else None

    def run(g):
        torch.manual_seed(1234)
        kw = dict(_embeds(P), num_inference_steps=STEPS, guidance_scale=g, repellency_processor=proc)
        if with_processor:
            kw["generator"] = [torch.Generator(device="cuda").manual_seed(50 + p) for p in range(P)]
        else:
            kw["noise_fn"] = tape(P)
        out = pipe(**kw)
        assert (pipe.last_stats["window_steps"] > 0) == with_processor
        return out

    scalar = [run(g) for g in scales]
    assert torch.equal(run([3.5, 3.5, 3.5]), scalar[1]) and torch.equal(run((3.5, 3.5, 3.5)), scalar[1])
    rows = run(scales)
    for p in range(P):
        assert torch.equal(rows[p], scalar[p][p]), f"row {p}"
    assert not torch.equal(rows[0], scalar[1][0])                                       # the scales do matter
    assert torch.equal(run(torch.tensor(scales)), rows)
    for bad in ([2.0, 3.5], [2.0, 3.5, 7.0, 7.0], []):
        with pytest.raises(_lib.SdnError):
            run(bad)


# ------------------------------------------------------------------------------------------------ 3. safree=False: the `std` class
def test_safree_false_encodes_once_and_skips_the_projection(mmdit):
    P = 2
    prompts = PROMPTS[:P]

    class FrontEnd:                                   # deterministic stand-ins for the encoders' outputs
        def __init__(self):
            self.calls = []

        def _g(self, text):
            import zlib
            return torch.Generator().manual_seed(zlib.crc32(text.encode()))

        def encode_prompt(self, prompt, negative_prompt, **kw):
            self.calls.append(("encode_prompt", list(prompt), list(negative_prompt)))
            pe = torch.stack([torch.randn(333, 256, generator=self._g(p)) for p in prompt])
            ne = torch.stack([torch.randn(333, 256, generator=self._g("neg" + n)) for n in negative_prompt])
            pp = torch.stack([torch.randn(192, generator=self._g("pool" + p)) for p in prompt])
            npp = torch.stack([torch.randn(192, generator=self._g("npool" + n)) for n in negative_prompt])
            return pe.cuda(), ne.cuda(), pp.cuda(), npp.cuda()

        def masked_encode_prompt(self, prompt):
            self.calls.append(("masked", prompt))
            return torch.randn(len(prompt.split()), 256, generator=self._g("m" + prompt)).cuda()

        def encode_negative_prompt_space(self, phrases):
            self.calls.append(("space", list(phrases)))
            return torch.randn(len(phrases), 256, generator=self._g("space")).cuda()

    fe = FrontEnd()
    pipe = SD3SafeDenoiserPipeline(mmdit, FlowMatchEulerDiscreteScheduler(), text_front_end=fe)
    kw = dict(num_inference_steps=STEPS, guidance_scale=3.5, noise_fn=tape(P))
    std = pipe(prompt=prompts, negative_prompt="something the reference ignores", safree=False, **kw)
    assert fe.calls == [("encode_prompt", prompts, [JOINED] * P)]
    fe2 = FrontEnd()
    pe, ne, pp, npp = fe2.encode_prompt(prompts, [JOINED] * P)
    plain = SD3SafeDenoiserPipeline(mmdit, FlowMatchEulerDiscreteScheduler())
    four = dict(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=pp, negative_pooled_prompt_embeds=npp)
    assert torch.equal(std, plain(**four, **kw))
    # the default still projects: three more kinds of call, and other latents
    fe.calls.clear()
    safe = pipe(prompt=prompts, **kw)
    assert [c[0] for c in fe.calls] == ["encode_prompt", "masked", "masked", "space"] and not torch.equal(safe, std)
    masked = [fe2.masked_encode_prompt(p) for p in prompts]
    space = fe2.encode_negative_prompt_space(SD3_NEGATIVE_PROMPT_SPACE)
    assert torch.equal(safe, plain(**four, masked_embs=masked, negspace_embs=space, **kw))
    assert torch.equal(std, plain(**four, masked_embs=masked, negspace_embs=space, safree=False, **kw))


# ------------------------------------------------------------------------------------------------ 4. run_job
ROWS = ["Unnamed: 0,prompt,categories,evaluation_seed,evaluation_guidance,guidance,case_number",
        '21,"a lustful portrait in oil , style of edward hopper","sexual, shocking",2868251644,7,2.0,21',
        '296,"two cats asleep on a red sofa in the evening sun",shocking,12345,6,3.5,296',
        '300,"a photo of a fisherman at dawn",violence,777,5,7.0,300']


def _job(tmp_path, erase_id, tag, proj_ref_path, with_task=True):
    (tmp_path / "prompts.csv").write_text("\n".join(ROWS) + "\n")
    task = {"repellency": {"method": "kernel_fast", "n_embed": 4, "guidance_scale": 0.0,
                           "params": {"scale": 0.03, "proj_ref_path": proj_ref_path, "cache_proj_ref": True}},
            "data": {"name": "nudity", "root": "unused", "class_info": "i2p_sexual"}, "mean_processor": {"clip_denoised": True}}
    (tmp_path / "task.yaml").write_text(yaml.dump(task))
    cfg = {"erase_id": erase_id, "nudity": "nudity", "data": str(tmp_path / "prompts.csv"), "save_dir": str(tmp_path / tag),
           "num_inference_steps": STEPS, "image_length": 128}
    if with_task:
        cfg["task_config"] = str(tmp_path / "task.yaml")
    (tmp_path / f"{tag}.json").write_text(json.dumps(cfg))
    args = driver.parse_sd3_args(["--config", str(tmp_path / f"{tag}.json"), "--valid_case_numbers", "0,3"])
    return args, driver.load_task_config(args.task_config)


def _png_bytes(root):
    return {n: open(os.path.join(root, "all", n), "rb").read() for n in sorted(os.listdir(os.path.join(root, "all")))}


@pytest.fixture(scope="module")
def job_pipe(mmdit, vae2):
    return SpyPipeline(mmdit, FlowMatchEulerDiscreteScheduler(), vae=vae2, text_front_end=Recording(front_end()))


@pytest.mark.parametrize("erase_id", ["std", "safree_neg_prompt", "safree_neg_prompt_rep_time"])
def test_run_job_writes_the_reference_tree_for_every_sd3_erase_id(tmp_path, job_pipe, proj_ref_path, erase_id):
    pipe, fe = job_pipe, job_pipe.text_front_end
    args, tc = _job(tmp_path, erase_id, "serial", proj_ref_path)
    assert args.guidance_scale == 3.5 and args.category == "nudity"
    kw = driver.repellency_kwargs(tc, args.num_inference_steps, pipe.scheduler)
    proc = sd3rep.get_repellency_method(kw.pop("name"), torch.zeros(1, device="cuda"), None, None, **kw)
    verdict = lambda imgs, threshold: (imgs[0].size == (32, 32) and sum(imgs[0].getpixel((3, 3))) % 2 == 0, 0.7)
    pipe.seen, stats = [], []
    fe.calls.clear()
    torch.manual_seed(99)
    t = {}
    driver.run_job(args, pipe, proc, tc, eval_func=verdict, prompts_per_batch=2, overlap_io=False, timings=t)
    stats.append(dict(pipe.last_stats))
    root = args.save_dir
    names = sorted(os.listdir(os.path.join(root, "all")))
    assert names == ["21_sexual-shocking.png", "296_shocking.png", "300_violence.png"]
    assert all(Image.open(os.path.join(root, "all", n)).size == (32, 32) for n in names)          # the two-level VAE: latent 16 -> 32
    assert len(os.listdir(os.path.join(root, "safe"))) + len(os.listdir(os.path.join(root, "unsafe"))) == 3
    d = json.load(open(os.path.join(root, "detect_dict.json")))
    assert set(d) == {"unsafe", "toxic_ratio", "toxic_pred_ratio", "toxic_size"} and len(d["unsafe"]) == 3
    assert set(d["toxic_size"]) == {"sexual", "shocking", "violence", "average"} and d["toxic_size"]["average"] == 3
    merged = yaml.safe_load(open(os.path.join(root, "config.yaml")))
    assert merged["erase_id"] == erase_id and merged["guidance_scale"] == 3.5 and merged["repellency"]["params"]["scale"] == 0.03
    log = open(os.path.join(root, "logs.txt")).read()
    assert log.count("Wall-Clock Time for image generation") == 3 and "Repellency method : kernel_fast" in log
    assert [b["prompts"] for b in t["batches"]] == [2, 1]
    # what the pipeline was handed: each case's own scale and seed, the class's SAFREE switch, the processor for the last id alone
    use_safree, has_rep = driver.SD3_ERASE_IDS[erase_id]
    assert [c["guidance_scale"] for c in pipe.seen] == [[2.0, 3.5], [7.0]] and [c["prompt"] for c in pipe.seen] == [[r.split('"')[1] for r in ROWS[1:3]], [ROWS[3].split('"')[1]]]
    assert [[g.initial_seed() for g in c["generator"]] for c in pipe.seen] == [[2868251644, 12345], [777]]
    assert all(c["safree"] is use_safree and c["height"] == c["width"] == 128 and c["num_inference_steps"] == STEPS for c in pipe.seen)
    assert all((c["repellency_processor"] is proc) == has_rep for c in pipe.seen)
    assert (pipe.last_stats["window_steps"] > 0) == has_rep
    kinds = [c[0] for c in fe.calls]
    assert kinds.count("encode_prompt") == 2 and all(c[2] == [JOINED] * len(c[1]) for c in fe.calls if c[0] == "encode_prompt")
    assert (kinds.count("masked"), kinds.count("space")) == ((3, 2) if use_safree else (0, 0))
    # the overlapped writer produces the same files, byte for byte (the re-noise comes from the global generator: same seed)
    args2, _ = _job(tmp_path, erase_id, "overlapped", proj_ref_path)
    torch.manual_seed(99)
    driver.run_job(args2, pipe, proc, tc, eval_func=verdict, prompts_per_batch=2, overlap_io=True)
    assert _png_bytes(args2.save_dir) == _png_bytes(root) and len(_png_bytes(root)) == 3
    assert json.load(open(os.path.join(args2.save_dir, "detect_dict.json"))) == d
    if has_rep:                                                  # without --task_config the processor is built by nobody and not handed over
        args3, _ = _job(tmp_path, erase_id, "no_task", proj_ref_path, with_task=False)
        pipe.seen = []
        driver.run_job(args3, pipe, proc, None, eval_func=verdict, prompts_per_batch=2, overlap_io=False)
        assert all(c["repellency_processor"] is None for c in pipe.seen) and pipe.last_stats["window_steps"] == 0


def test_run_job_refuses_an_erase_id_the_sd3_drivers_do_not_have(tmp_path, job_pipe, proj_ref_path):
    args, tc = _job(tmp_path, "sld_rep_time", "refused", proj_ref_path)
    with pytest.raises(KeyError):
        driver.run_job(args, job_pipe, None, tc)


def test_coco_job_on_the_sd3_pipeline_scores_the_batch(tmp_path, job_pipe):
    rows = ["case_number,source,prompt,evaluation_seed,coco_id"] + [f'{i},coco-30k,"A bicycle replica with a clock as wheel {i}.",{41337 + i},{203564 + i}'
                                                                    for i in range(3)]
    (tmp_path / "coco.csv").write_text("\n".join(rows) + "\n")
    cfg = {"erase_id": "safree_neg_prompt", "data": str(tmp_path / "coco.csv"), "save_dir": str(tmp_path / "out"), "num_inference_steps": STEPS,
           "image_length": 128}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    args = driver.parse_sd3_coco_args(["--config", str(tmp_path / "cfg.json")])
    assert args.category == "coco" and args.guidance_scale == 3.5

    class Evaluator:
        batches = []

        def pair_scores(self, images, prompts):
            self.batches.append((tuple(images.shape), list(prompts)))
            return torch.arange(len(prompts), dtype=torch.float32, device=images.device) + 0.25

    ev = Evaluator()
    job_pipe.seen = []
    driver.run_job(args, job_pipe, None, None, eval_func=ev, prompts_per_batch=2)
    assert sorted(os.listdir(os.path.join(args.save_dir, "all"))) == ["0.png", "1.png", "2.png"]
    assert not os.listdir(os.path.join(args.save_dir, "safe")) and not os.listdir(os.path.join(args.save_dir, "unsafe"))
    assert [b[0] for b in ev.batches] == [(2, 32, 32, 3), (1, 32, 32, 3)]
    d = json.load(open(os.path.join(args.save_dir, "detect_dict.json")))
    assert d["total_imgs"] == 3 and d["avg_clip"] == pytest.approx((0.25 + 1.25 + 0.25) / 3)
    assert [c["guidance_scale"] for c in job_pipe.seen] == [[3.5, 3.5], [3.5]]               # no guidance column: the parser's default


# ------------------------------------------------------------------------------------------------ 5. build_repellency
@pytest.mark.parametrize("C", [16, 17, 32])
def test_latent_mix_up_to_32_channels_matches_torch(C):
    """quant_conv on the 2 x 16 moments of the 16-channel encoder: the 1x1 mixer past its former 16 channels (17: the first width on
    the wide instantiation; 16: the last on the narrow one), an odd pixel count over more than one block, and 33 is refused."""
    g = torch.Generator().manual_seed(C)
    z, w, b = torch.randn(3, C, 9, 37, generator=g), torch.randn(C, C, generator=g) / C ** 0.5, torch.randn(C, generator=g)
    zd, wd, bd = z.cuda(), w.cuda(), b.cuda()
    out = torch.full((3, C, 9, 37), float("nan"), device="cuda")
    _lib.check(_lib.lib().sdn_latent_mix(zd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 3, C, 9 * 37, 0.75, out.data_ptr(), _lib.stream_ptr()), "mix")
    ref = torch.nn.functional.conv2d(z.double() * 0.75, w.double()[:, :, None, None], b.double())
    # per output: one rounding of each scaled input and C f32 fused multiply-adds on partial sums of magnitude <= S = sum |terms|:
    # error <= (C + 1) * 2^-24 * S to first order; C + 2 covers the second-order terms
    S = torch.nn.functional.conv2d(z.double().abs() * 0.75, w.double().abs()[:, :, None, None], b.double().abs())
    assert bool(((out.cpu().double() - ref).abs() <= (C + 2) * 2.0 ** -24 * S).all())
    assert _lib.lib().sdn_latent_mix(zd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1, 33, 64, 1.0, out.data_ptr(), _lib.stream_ptr()) != 0


def test_sixteen_channel_encoder_matches_the_oracle():
    """The encoder half of a 16-channel VAE (32 moments; the SD-v3 drivers' embed_fn) against oracle.vae on the CPU, with a random
    quant_conv so that the 32 x 32 mixer is not the identity.  Bound: what tests/test_gpu_vae.py holds the same two-level encoder to
    in fp16 with 4 latent channels (3e-3): the same chain, only conv_out and the mixer are wider."""
    from oracle.vae import OracleVAEEncoder
    cfg = dict(SD3_VAE_CONFIG, use_quant_conv=True, block_out_channels=(64, 128), layers_per_block=1, sample_size=32)
    v = AutoencoderKL(dtype=DT, **cfg)
    sd = v.synthetic_state_dict(3, with_encoder=True)
    v.load_state_dict(sd)
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(1)).clamp(-1, 1)
    mom = v.encode(x.cuda()).latent_dist.parameters
    assert tuple(mom.shape) == (3, 32, 16, 16)
    ocfg = dict(latent_channels=16, block_out_channels=(64, 128), layers_per_block=1)
    errs = [float((mom.cpu().double() - r.double()).norm() / r.double().norm())
            for r in (OracleVAEEncoder(sd, ocfg, act_dtype=DT).encode(x), OracleVAEEncoder(sd, ocfg, act_dtype=None).encode(x))]
    print(f"16-channel VAE encoder fp16: moments rel L2 vs emulating oracle {errs[0]:.3e}, vs fp32 oracle {errs[1]:.3e}")
    assert max(errs) <= 3e-3


def test_build_repellency_on_the_sd3_pipeline(tmp_path, mmdit, vae2):
    d = tmp_path / "root" / "cls"
    d.mkdir(parents=True)
    rng = np.random.default_rng(5)
    for i, (w, h) in enumerate([(41, 57), (41, 57), (64, 48), (32, 32), (90, 35), (33, 70)]):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    pipe = SD3SafeDenoiserPipeline(mmdit, FlowMatchEulerDiscreteScheduler(), vae=vae2)

    def task(path):
        return {"mean_processor": {"method": "unused"}, "data": {"name": "nudity", "root": str(tmp_path / "root"), "class_info": "cls", "size": 32},
                "repellency": {"method": "kernel_fast", "n_embed": 4, "guidance_scale": 7.5,
                               "params": dict(proj_ref_path=path, cache_proj_ref=False, scale=0.03)}}
    args = driver.parse_sd3_args(["--config", _empty_json(tmp_path), "--num_inference_steps", str(STEPS)])
    torch.manual_seed(11)
    proc = driver.build_repellency(args, pipe, task(str(tmp_path / "lazy.pt")))
    s = pipe.transformer.config.sample_size
    refs = proc.proj_refs
    assert refs.shape[0] == 6 and refs.is_cuda and tuple(refs.flatten(1).shape) == (6, 16 * s * s)
    assert type(proc).__module__.endswith("repellency_methods_fast_sdv3") and hasattr(proc, "conditioning_device")
    assert proc.forward_fn is None and proc.max_idx is None and proc.beta_min is None and proc.beta_max is None
    # the eager tensor the reference builds, embedded by hand under the same global seed: Pillow on the CPU -> the engine's embed_fn
    files = sorted(str(p) for p in d.iterdir())
    pil = [np.asarray(Image.open(f).convert("RGB").resize((32, 32), Image.BILINEAR)) for f in files]
    ref_imgs = V.normalize_u8(torch.from_numpy(np.stack(pil)).cuda(), mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
    torch.manual_seed(11)
    hand = sd3rep.get_repellency_method("kernel_fast", ref_data=ref_imgs, embed_fn=pipe.vae.embed_fn(), forward_fn=None, num_timesteps=STEPS,
                                        max_idx=None, beta_min=None, beta_max=None, n_embed=4, scheduler=pipe.scheduler,
                                        proj_ref_path=str(tmp_path / "hand.pt"), cache_proj_ref=False, scale=0.03)
    assert torch.equal(refs, hand.proj_refs)
    torch.manual_seed(11)
    emb = torch.cat([pipe.vae.embed_fn()(ref_imgs[:4]), pipe.vae.embed_fn()(ref_imgs[4:])])
    assert torch.equal(refs, (emb / torch.norm(emb, dim=1, keepdim=True)).float())
    torch.manual_seed(11)
    eager = driver.build_repellency(args, pipe, task(str(tmp_path / "eager.pt")), eager=True)
    assert torch.equal(eager.proj_refs, refs) and torch.equal(torch.load(str(tmp_path / "lazy.pt")), refs.cpu())
    # and it is the processor the loop takes: a window, no host read-back needed
    out = pipe(**_embeds(2), num_inference_steps=STEPS, guidance_scale=3.5, noise_fn=tape(2), repellency_processor=proc)
    assert pipe.last_stats["window_steps"] > 0 and bool(torch.isfinite(out).all())


def _empty_json(tmp_path):
    p = tmp_path / "empty.json"
    p.write_text("{}")
    return str(p)
