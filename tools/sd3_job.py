#!/usr/bin/env python3
"""An SD-v3 job as a measurement (not the bench line): SD3-medium with synthetic weights, the three text encoders at full size with
synthetic weights (T5-XXL, CLIP-L, bigG) behind the stand-in tokenizers, the 16-channel VAE, and a synthetic fast_sdv3 reference
set of REFS rows, through driver.run_job at 512 x 512 -- prompt strings in, PNG files out, as run_nudity_sdv3.py.

    python tools/sd3_job.py [--prompts 32] [--per-batch 16] [--steps 28] [--refs 515] [--erase-id safree_neg_prompt_rep_time]
                            [--bench-sd3 tools/bench_sd3.py] [--out profiles/sd3_job.json]

Writes images/sec of the job, its split into front end / loop / decode / host I/O, and the commit.  The split: the front end's
three calls and the VAE decode are timed around a stream synchronisation each (which the job itself does not have, so the split's
parts are upper bounds and the job is timed in a run of its own without them); loop = the batches' GPU time minus those two;
host I/O = the writer thread's busy time, overlapped with the next batch.  `--bench-sd3 PATH`: runs that tools/bench_sd3.py (the
loop alone, from embeddings, same side / batch / steps / reference rows) as a child process FIRST and records its figure and the
ratio job / loop-only.  There are no real checkpoints or tokenizer vocabularies here: every number is for synthetic weights and
whitespace tokenizers, whose prompts are about as long in tokens as they are in words."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from safe_denoiser_amd import driver  # noqa: E402
from safe_denoiser_amd.clip import SD3_CLIP_G_CONFIG, SD3_CLIP_L_CONFIG, CLIPTextModelWithProjection  # noqa: E402
from safe_denoiser_amd.mmdit import SD3Transformer2DModel  # noqa: E402
from safe_denoiser_amd.pipeline_sd3 import SD3SafeDenoiserPipeline  # noqa: E402
from safe_denoiser_amd.repellency import repellency_methods_fast_sdv3 as sd3rep  # noqa: E402
from safe_denoiser_amd.schedulers import FlowMatchEulerDiscreteScheduler  # noqa: E402
from safe_denoiser_amd.t5 import T5EncoderModel  # noqa: E402
from safe_denoiser_amd.text_sd3 import SD3TextFrontEnd  # noqa: E402
from safe_denoiser_amd.vae import SD3_VAE_CONFIG, AutoencoderKL  # noqa: E402
from tests_support.fake_tokenizer import FakeCLIPTokenizer  # noqa: E402
from tests_support.t5_oracle import FakeT5Tokenizer  # noqa: E402

WORDS = ("a painting of the sea at dawn with two fishing boats and a lighthouse in heavy fog , oil on canvas , muted colours , "
         "highly detailed brush strokes in the style of the dutch masters").split()


def git_head():
    head = os.environ.get("SDN_GIT_HEAD")
    if not head:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, timeout=10).stdout.strip() or None
        except Exception:
            head = None
    return head


class TimedFrontEnd:
    """The front end's three calls, each between two stream synchronisations."""

    def __init__(self, inner):
        self.inner, self.seconds, self.masked_rows = inner, 0.0, 0

    def _timed(self, fn, *a, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        torch.cuda.synchronize()
        self.seconds += time.perf_counter() - t0
        return out

    def encode_prompt(self, **kw):
        return self._timed(self.inner.encode_prompt, **kw)

    def masked_encode_prompt(self, prompt):
        out = self._timed(self.inner.masked_encode_prompt, prompt)
        self.masked_rows += out.shape[0]
        return out

    def encode_negative_prompt_space(self, phrases):
        return self._timed(self.inner.encode_negative_prompt_space, phrases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--per-batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=28)
    ap.add_argument("--refs", type=int, default=515)
    ap.add_argument("--erase-id", default="safree_neg_prompt_rep_time", choices=sorted(driver.SD3_ERASE_IDS))
    ap.add_argument("--bench-sd3", default=None, help="a tools/bench_sd3.py to run first, as a child process, for the loop-only figure")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sd3_job.json"))
    a = ap.parse_args()
    side, dt = 64, torch.float16
    report = {"commit": git_head(), "commit_note": "HEAD of the tree the tool ran in; changes on top of it do not show here",
              "image": "512x512", "prompts": a.prompts, "prompts_per_batch": a.per_batch, "steps": a.steps,
              "reference_rows": a.refs, "erase_id": a.erase_id, "dtype": "float16",
              "weights": "synthetic (no checkpoint exists here); tokenizers: whitespace stand-ins"}
    if a.bench_sd3:
        env = dict(os.environ, SIDE=str(side), P=str(a.per_batch), STEPS=str(a.steps), REFS=str(a.refs))
        out = subprocess.run([sys.executable, a.bench_sd3], env=env, capture_output=True, text=True, timeout=900)
        line = (out.stdout.strip().splitlines() or [""])[-1]
        m = re.search(r"([0-9.]+) images/sec", line)
        if out.returncode != 0 or not m:
            raise SystemExit(f"{a.bench_sd3} failed ({out.returncode}): {out.stdout[-400:]} {out.stderr[-400:]}")
        report["loop_only"] = {"tool": "tools/bench_sd3.py", "images_per_s": float(m.group(1)), "line": line}

    work = tempfile.mkdtemp(prefix="sd3_job_")
    tr = SD3Transformer2DModel(text_len=333, dtype=dt, sample_size=side)
    tr.load_synthetic_on_device(3)
    vae = AutoencoderKL(dtype=dt, **dict(SD3_VAE_CONFIG, sample_size=side * 8))
    vae.load_synthetic_on_device(5)
    t5 = T5EncoderModel(dtype=dt).load_synthetic_on_device(7)
    e1 = CLIPTextModelWithProjection(dtype=dt, hidden_act="quick_gelu", projection_dim=768, **SD3_CLIP_L_CONFIG).load_synthetic_on_device(8)
    e2 = CLIPTextModelWithProjection(dtype=dt, hidden_act="gelu", projection_dim=1280, **SD3_CLIP_G_CONFIG).load_synthetic_on_device(9)
    fe = TimedFrontEnd(SD3TextFrontEnd(t5, FakeT5Tokenizer(), text_encoder=e1, tokenizer=FakeCLIPTokenizer(), text_encoder_2=e2,
                                       tokenizer_2=FakeCLIPTokenizer()))
    pipe = SD3SafeDenoiserPipeline(tr, FlowMatchEulerDiscreteScheduler(), vae=vae, text_front_end=fe)
    decode_s = [0.0]
    decode = vae.decode_latents_uint8

    def timed_decode(lat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = decode(lat)
        torch.cuda.synchronize()
        decode_s[0] += time.perf_counter() - t0
        return out

    g = torch.Generator(device="cuda").manual_seed(1)
    refs = torch.randn(a.refs, 16, side, side, generator=g, device="cuda")
    refs = (refs / refs.norm(dim=1, keepdim=True)).cpu()
    ref_path = os.path.join(work, "proj_ref.pt")
    torch.save(refs, ref_path)
    del refs
    task = {"mean_processor": {}, "data": {"name": "synthetic"},
            "repellency": {"method": "kernel_fast", "n_embed": 4, "guidance_scale": 0.0,
                           "params": {"scale": 0.03, "proj_ref_path": ref_path, "cache_proj_ref": True}}}
    import yaml
    with open(os.path.join(work, "task.yaml"), "w") as f:
        yaml.dump(task, f)
    rows = ["case_number,prompt,categories,evaluation_seed,guidance"]
    for i in range(a.prompts):                                      # 8 to 23 words, three guidance scales
        words = [WORDS[(i * 7 + k) % len(WORDS)] for k in range(8 + i % 16)]
        rows.append(f'{i},"{" ".join(words)}",sexual,{1000 + i},{(2.5, 3.5, 7.0)[i % 3]}')
    with open(os.path.join(work, "prompts.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")

    def job(tag):
        cfg = {"erase_id": a.erase_id, "nudity": "nudity", "data": os.path.join(work, "prompts.csv"), "save_dir": os.path.join(work, tag),
               "num_inference_steps": a.steps, "image_length": side * 8, "task_config": os.path.join(work, "task.yaml")}
        with open(os.path.join(work, f"{tag}.json"), "w") as f:
            json.dump(cfg, f)
        args = driver.parse_sd3_args(["--config", os.path.join(work, f"{tag}.json")])
        tc = driver.load_task_config(args.task_config)
        kw = driver.repellency_kwargs(tc, args.num_inference_steps, pipe.scheduler)
        proc = sd3rep.get_repellency_method(kw.pop("name"), torch.zeros(1, device="cuda"), None, None, **kw)
        t = {}
        torch.manual_seed(0)
        fe.seconds, fe.masked_rows, decode_s[0] = 0.0, 0, 0.0
        driver.run_job(args, pipe, proc, tc, eval_func=None, prompts_per_batch=a.per_batch, timings=t)
        return t

    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):                 # the job's own log lines (they are in logs.txt as well)
        job("warm")
        plain = job("plain")                                        # the figure: no synchronisation the job does not have
        vae.decode_latents_uint8 = timed_decode
        split = job("split")
        vae.decode_latents_uint8 = decode
    n_png = len(os.listdir(os.path.join(work, "plain", "all")))
    gpu_s = sum(b["gpu_s"] for b in split["batches"])
    report["job"] = {"images_per_s": a.prompts / plain["total_s"], "total_s": plain["total_s"],
                     "batches_gpu_s": sum(b["gpu_s"] for b in plain["batches"]), "host_io_s": plain["host_io_s"], "png_files": n_png,
                     "window_steps": pipe.last_stats["window_steps"]}
    report["split_run"] = {"total_s": split["total_s"], "front_end_s": fe.seconds, "loop_s": gpu_s - fe.seconds - decode_s[0],
                           "decode_s": decode_s[0], "host_io_s_overlapped": split["host_io_s"], "masked_t5_rows": fe.masked_rows,
                           "note": "front end and decode timed between stream synchronisations; loop = batches' GPU time minus the two"}
    if "loop_only" in report:
        report["job_over_loop_only"] = report["job"]["images_per_s"] / report["loop_only"]["images_per_s"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
