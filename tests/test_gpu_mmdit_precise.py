"""SD-v3 MMDiT precision plans (sdn_mmdit_config.dtype 2 = fp32 on the f32-input matrix cores, 3 = bf16x3 contractions on f32
storage): the new f32 operators (adaLN LayerNorm, patchify, two-stream joint attention), the whole network against the pure-fp32
oracle (small configuration on the CPU oracle, full SD3-medium on the oracle's torch ops evaluated on the GPU), the flow loop with
fast_sdv3 repellency in fp32 latents, and the SD-v3 pipeline's precision schedule.
Bounds: the value measured on MI355X (quoted next to each) times 2, never looser than the ceilings the plans are specified to
meet (operators 1e-6 / float64, bf16x3 network 1e-4 per forward, loops 1e-4 small / 1e-3 full size)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import safe_denoiser_amd as sda
from oracle.mmdit import OracleMMDiT
from safe_denoiser_amd import _lib
from safe_denoiser_amd.mmdit import SD3Transformer2DModel

pytestmark = pytest.mark.gpu

SMALL = dict(sample_size=16, num_layers=3, num_attention_heads=4, joint_attention_dim=128, pooled_projection_dim=64,
             pos_embed_max_size=24)
SMALL_O = dict(sample_size=16, num_layers=3, num_heads=4, joint_dim=128, pooled_dim=64, pos_embed_max_size=24)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.fixture
def no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = old


# ---- operators ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [256, 1536])
def test_layernorm_mod_f32_matches_torch_fp32(Cc):
    g = torch.Generator().manual_seed(1)
    B, rows = 3, 37
    x = torch.randn(B * rows, Cc, generator=g) * 2 + 0.3
    mod = torch.randn(B, 3 * Cc, generator=g) * 0.3
    xg, mg = x.cuda(), mod.cuda()
    out = torch.empty_like(xg)
    _lib.check(sda.lib().sdn_layernorm_mod_f32(xg.data_ptr(), B * rows, Cc, 1e-6, mg[:, Cc:].data_ptr(), mg.data_ptr(), 3 * Cc, rows,
                                               out.data_ptr(), _lib.stream_ptr()), "sdn_layernorm_mod_f32")
    ref = F.layer_norm(x, (Cc,), eps=1e-6).reshape(B, rows, Cc) * (1 + mod[:, None, Cc:2 * Cc]) + mod[:, None, :Cc]
    r = rel_l2(out, ref.reshape(-1, Cc))
    print(f"sdn_layernorm_mod_f32 C={Cc}: rel L2 vs torch fp32 {r:.2e}")
    assert r <= 2e-7                                          # measured 5.9e-8 (C = 256) / 5.7e-8 (C = 1536)


def test_patchify_f32_is_the_torch_reshuffle():
    g = torch.Generator().manual_seed(2)
    for (b, c, s) in ((2, 16, 8), (3, 16, 64)):
        lat = torch.randn(b, c, s, s, generator=g)
        lg = lat.cuda()
        pt = torch.empty(b * (s // 2) ** 2, c * 4, device="cuda")
        _lib.check(sda.lib().sdn_patchify_f32(lg.data_ptr(), b, c, s, s, 2, pt.data_ptr(), _lib.stream_ptr()), "sdn_patchify_f32")
        ref = F.unfold(lat, kernel_size=2, stride=2).transpose(1, 2).reshape(-1, c * 4)          # column order (c, py, px)
        assert torch.equal(pt.cpu(), ref)


def _joint(mode, q1, q2, Cc, Hh, n1, n2):
    B = q1.shape[0]
    o1 = torch.empty(B, n1, Cc, device="cuda"); o2 = torch.empty(B, n2, Cc, device="cuda")
    s2 = _lib.AttnSegment2(q2.data_ptr(), q2[..., Cc:].data_ptr(), q2[..., 2 * Cc:].data_ptr(), o2.data_ptr(), n1,
                           3 * Cc, 3 * Cc, 3 * Cc, Cc)
    _lib.check(sda.lib().sdn_joint_attention_f32(mode, q1.data_ptr(), q1[..., Cc:].data_ptr(), q1[..., 2 * Cc:].data_ptr(),
                                                 o1.data_ptr(), C.byref(s2), B, Hh, n1 + n2, 64, 3 * Cc, 3 * Cc, 3 * Cc, Cc,
                                                 64 ** -0.5, _lib.stream_ptr()), "sdn_joint_attention_f32")
    return o1, o2


@pytest.mark.parametrize("n1,n2", [(64, 45), (100, 7), (1024, 333)])
def test_joint_attention_f32_both_modes(n1, n2):
    """Two token streams in separate buffers (query sets and K / V tiles straddle n1 for 100 + 7 and 1024 + 333): float64 torch on the
    concatenation, and the bits of the single-stream kernel run over the materialised concatenation."""
    g = torch.Generator().manual_seed(3)
    B, Hh, d = 2, 4, 64
    Cc = Hh * d
    qkv1 = torch.randn(B, n1, 3 * Cc, generator=g); qkv2 = torch.randn(B, n2, 3 * Cc, generator=g)
    cat = torch.cat([qkv1, qkv2], 1).double()
    sp = lambda t: t.reshape(B, n1 + n2, Hh, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sp(cat[..., :Cc]), sp(cat[..., Cc:2 * Cc]), sp(cat[..., 2 * Cc:]))
    ref = ref.transpose(1, 2).reshape(B, n1 + n2, Cc)
    g1, g2 = qkv1.cuda(), qkv2.cuda()
    gc = torch.cat([g1, g2], 1).contiguous()
    # measured: mode 0 (exact f32 products) 3.1e-7 ... 7.5e-7, mode 1 (bf16x3) 5.7e-6 ... 6.4e-6
    for mode, single, bound in ((0, sda.lib().sdn_attention_f32, 1.5e-6), (1, sda.lib().sdn_attention_x3, 1.3e-5)):
        o1, o2 = _joint(mode, g1, g2, Cc, Hh, n1, n2)
        oc = torch.empty(B, n1 + n2, Cc, device="cuda")
        _lib.check(single(gc.data_ptr(), gc[..., Cc:].data_ptr(), gc[..., 2 * Cc:].data_ptr(), oc.data_ptr(), B, Hh, n1 + n2, n1 + n2, 64,
                          3 * Cc, 3 * Cc, 3 * Cc, Cc, 64 ** -0.5, _lib.stream_ptr()), "single-stream attention")
        torch.cuda.synchronize()
        r1, r2 = rel_l2(o1, ref[:, :n1]), rel_l2(o2, ref[:, n1:])
        print(f"joint attention f32 mode {mode} ({n1} + {n2}): rel L2 vs float64 {r1:.2e} / {r2:.2e}")
        assert r1 <= bound and r2 <= bound
        assert torch.equal(o1, oc[:, :n1]) and torch.equal(o2, oc[:, n1:])


# ---- small network --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_sd():
    return SD3Transformer2DModel(text_len=45, **SMALL).synthetic_state_dict(5)


def _small(precision, sd):
    m = SD3Transformer2DModel(text_len=45, precision=precision, **SMALL) if precision else \
        SD3Transformer2DModel(text_len=45, dtype=torch.float16, **SMALL)
    m.load_state_dict(sd)
    return m


def test_small_precise_mmdit_matches_the_fp32_oracle(small_sd):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 16, 16, 16, generator=g); e = torch.randn(2, 45, 128, generator=g); pl = torch.randn(2, 64, generator=g)
    ref = OracleMMDiT(small_sd, SMALL_O, act_dtype=None)(x, 812.0, e, pl)
    res = {}
    for precision in (None, "fp32", "bf16x3"):
        m = _small(precision, small_sd)
        y = m(x.cuda(), timestep=torch.tensor([812.0, 812.0]).cuda(), encoder_hidden_states=e.cuda(), pooled_projections=pl.cuda())[0]
        torch.cuda.synchronize()
        assert y.dtype == torch.float32 and torch.isfinite(y).all()
        res[precision or "fp16"] = rel_l2(y, ref)
    print(f"small mmdit vs the pure-fp32 oracle: fp16 {res['fp16']:.2e}, fp32 {res['fp32']:.2e}, bf16x3 {res['bf16x3']:.2e}")
    assert res["fp32"] <= 1.2e-6 and res["bf16x3"] <= 1.2e-5            # measured 6.0e-7 / 5.95e-6 (fp16: 6.9e-4)
    assert 10 * res["fp32"] <= res["fp16"] and 10 * res["bf16x3"] <= res["fp16"]


@pytest.mark.parametrize("precision,cap", [("fp32", 3), ("bf16x3", 5)])
def test_precise_batch_above_the_plan_limit_runs_as_row_blocks(small_sd, precision, cap):
    """7 samples with the plan limit lowered: row blocks (2+2+2+1, or 4+3) give the single forward's bits.  (bf16x3 with blocks of at
    least two samples: its GEMMs take the exact f32 tile below 64 rows, and one sample's 45 text rows are below that.)"""
    m = _small(precision, small_sd)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(7, 16, 16, 16, generator=g).cuda(); e = m.prepare_text(torch.randn(7, 45, 128, generator=g).cuda())
    pl = torch.randn(7, 64, generator=g).cuda()
    assert e.dtype == torch.float32
    ref, y = torch.empty(7, 16, 16, 16, device="cuda"), torch.empty(7, 16, 16, 16, device="cuda")
    m.forward_into(x, 812.0, e, pl, ref)
    m.max_samples = lambda: cap
    m.forward_into(x, 812.0, e, pl, y)
    assert torch.equal(y, ref)


# ---- loops ----------------------------------------------------------------------------------------------------------------------
class Tapes:
    def __init__(self, P, steps, side, dev=None):
        gg = torch.Generator().manual_seed(11)
        self.data = [torch.randn(steps + 2, 1, 16, side, side, generator=gg) for _ in range(P)]
        self.cur, self.dev = [0] * P, dev

    def __call__(self, p, shape):
        z = self.data[p][self.cur[p]].clone()
        self.cur[p] += 1
        return z if self.dev is None else z.to(self.dev)


def _processor(tmp_path, refs):
    from safe_denoiser_amd.repellency import repellency_methods_fast_sdv3 as sd3rep
    path = str(tmp_path / "pr.pt"); torch.save(refs, path)
    return sd3rep.get_repellency_method("kernel_fast", torch.zeros(1, device="cuda"), None, None, 50, 1000, 0.00085, 0.012, n_embed=4,
                                        proj_ref_path=path, cache_proj_ref=True, scale=0.03)


def test_small_loop_bf16x3_fp32_latents_matches_the_fp32_oracle(tmp_path, small_sd):
    from oracle import repellency as orp
    from oracle import schedulers as osch
    from oracle.mmdit import sd3_denoise_one
    from safe_denoiser_amd.pipeline_sd3 import SD3SafeDenoiserPipeline
    from safe_denoiser_amd.schedulers import FlowMatchEulerDiscreteScheduler
    m = _small("bf16x3", small_sd)
    g = torch.Generator().manual_seed(7)
    P, steps = 2, 12
    emb = torch.randn(2 * P, 45, 128, generator=g); pooled = torch.randn(2 * P, 64, generator=g)
    refs = orp.channel_normalise(torch.randn(10, 16, 16, 16, generator=g))
    proc = _processor(tmp_path, refs)
    net = OracleMMDiT(small_sd, SMALL_O, act_dtype=None)
    t_o = Tapes(P, steps, 16)
    ref = []
    for p in range(P):
        lat, st = sd3_denoise_one(net, osch.FlowMatchEuler(), torch.stack([emb[p], emb[P + p]]), torch.stack([pooled[p], pooled[P + p]]),
                                  p, t_o, num_inference_steps=steps, repel=dict(proj_refs=refs, scale=0.03), latents_dtype=torch.float32)
        ref.append(lat)
    t_p = Tapes(P, steps, 16)
    pipe = SD3SafeDenoiserPipeline(m, FlowMatchEulerDiscreteScheduler())
    out = pipe(prompt_embeds=emb.cuda(), pooled_prompt_embeds=pooled.cuda(), num_inference_steps=steps, repellency_processor=proc,
               noise_fn=t_p, latents_dtype=torch.float32)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32
    assert t_p.cur == t_o.cur and pipe.last_stats["window_steps"] == st["window_steps"] > 0
    errs = [rel_l2(out[p:p + 1], ref[p]) for p in range(P)]
    print(f"small sd3 loop, bf16x3 + fp32 latents ({st['window_steps']} window steps): rel L2 vs the fp32 oracle {['%.2e' % e for e in errs]}")
    assert max(errs) <= 1.7e-5                                            # measured 8.4e-6 / 8.2e-6


def test_sd3_precision_schedule(tmp_path, small_sd):
    """"all" = the bf16x3 transformer alone, bit for bit; "none" = the fp16 transformer alone; {"window": True} runs exactly the
    repellency-window steps (780 <= t <= 1000) on transformer_hi, each plan reading text / pooled in its own dtype."""
    from oracle import repellency as orp
    from safe_denoiser_amd.pipeline_sd3 import SD3SafeDenoiserPipeline
    from safe_denoiser_amd.schedulers import FlowMatchEulerDiscreteScheduler
    lo_net, hi_net = _small(None, small_sd), _small("bf16x3", small_sd)
    g = torch.Generator().manual_seed(8)
    P, steps = 2, 12
    emb = torch.randn(2 * P, 45, 128, generator=g).cuda(); pooled = torch.randn(2 * P, 64, generator=g).cuda()
    proc = _processor(tmp_path, orp.channel_normalise(torch.randn(10, 16, 16, 16, generator=g)))

    def run(net, hi=None, sched=None, ldt=torch.float32):
        pipe = SD3SafeDenoiserPipeline(net, FlowMatchEulerDiscreteScheduler(), transformer_hi=hi, precision_schedule=sched)
        out = pipe(prompt_embeds=emb, pooled_prompt_embeds=pooled, num_inference_steps=steps, repellency_processor=proc,
                   noise_fn=Tapes(P, steps, 16), latents_dtype=ldt)
        return out, pipe.last_stats

    a, st_a = run(lo_net, hi_net, "all")
    b, _ = run(hi_net)
    assert st_a["hi_steps"] == steps and torch.equal(a, b)
    a, st_a = run(lo_net, hi_net, "none", torch.float16)
    b, _ = run(lo_net, ldt=torch.float16)
    assert st_a["hi_steps"] == 0 and torch.equal(a, b)
    seen = []
    fwd = hi_net.forward_into
    hi_net.forward_into = lambda sample, t, *rest: (seen.append(t), fwd(sample, t, *rest))[1]
    try:
        w, st_w = run(lo_net, hi_net, {"window": True})
    finally:
        del hi_net.forward_into
    assert 0 < st_w["window_steps"] < steps and st_w["hi_steps"] == st_w["window_steps"] == len(seen)
    assert all(780 <= t <= 1000 for t in seen)
    print(f"precision schedule {{'window': True}}: {len(seen)} of {steps} steps on the bf16x3 plan (t = {seen})")
    assert torch.isfinite(w).all()


# ---- full SD3-medium ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd3_medium_x3():
    """Full SD3-medium (~2 B parameters, synthetic weights seed 3) on the bf16x3 plan + its state dict, built once for this module."""
    m = SD3Transformer2DModel(sample_size=64, precision="bf16x3")
    sd = m.synthetic_state_dict(3)
    m.load_state_dict(sd)
    return m, sd


def test_full_sd3_medium_bf16x3_matches_the_fp32_oracle(sd3_medium_x3, no_tf32):
    """SD3-medium at 512 x 512 (1024 image + 333 text tokens), two samples, against the pure-fp32 oracle's torch ops on the GPU."""
    m, sd = sd3_medium_x3
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 16, 64, 64, generator=g).cuda(); e = torch.randn(2, 333, 4096, generator=g).cuda()
    pl = torch.randn(2, 2048, generator=g).cuda()
    y = m(x, timestep=812.0, encoder_hidden_states=e, pooled_projections=pl)[0]
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    net = OracleMMDiT(sd, None, act_dtype=None, device="cuda")
    r = rel_l2(y, net(x, 812.0, e, pl))
    del net
    torch.cuda.empty_cache()
    print(f"full SD3-medium MMDiT bf16x3, B = 2: rel L2 vs the pure-fp32 oracle {r:.3e}")
    assert r <= 1.4e-5                                                    # measured 6.6e-6


def test_full_sd3_medium_10_step_loop_bf16x3_fp32_latents(tmp_path, sd3_medium_x3, no_tf32):
    """BASELINE config 4 at full size with the precise transformer: 512 x 512, guidance 3.5, 10 flow-Euler steps (the first 5 in the
    repellency window, M = 64 references), 2 prompts batched vs the per-prompt pure-fp32 oracle loop on the same noise tapes, fp32
    latents on both sides.  The fp16 plan misses the project's 1e-3 here (2.4e-3 bound, tests/test_gpu_mmdit.py)."""
    from oracle import repellency as orp
    from oracle import schedulers as osch
    from oracle.mmdit import sd3_denoise_one
    from safe_denoiser_amd.pipeline_sd3 import SD3SafeDenoiserPipeline
    from safe_denoiser_amd.schedulers import FlowMatchEulerDiscreteScheduler
    m, sd = sd3_medium_x3
    g = torch.Generator().manual_seed(21)
    P, steps = 2, 10
    emb = torch.randn(2 * P, 333, 4096, generator=g); pooled = torch.randn(2 * P, 2048, generator=g)
    refs = orp.channel_normalise(torch.randn(64, 16, 64, 64, generator=g))
    proc = _processor(tmp_path, refs)
    t_p = Tapes(P, steps, 64)
    pipe = SD3SafeDenoiserPipeline(m, FlowMatchEulerDiscreteScheduler())
    out = pipe(prompt_embeds=emb.cuda(), pooled_prompt_embeds=pooled.cuda(), num_inference_steps=steps, guidance_scale=3.5,
               repellency_processor=proc, noise_fn=t_p, latents_dtype=torch.float32).float().cpu()
    net = OracleMMDiT(sd, None, act_dtype=None, device="cuda")
    t_o = Tapes(P, steps, 64, "cuda")
    ref = []
    for p in range(P):
        lat, st = sd3_denoise_one(net, osch.FlowMatchEuler(), torch.stack([emb[p], emb[P + p]]).cuda(),
                                  torch.stack([pooled[p], pooled[P + p]]).cuda(), p, t_o, num_inference_steps=steps, guidance_scale=3.5,
                                  repel=dict(proj_refs=refs.cuda(), scale=0.03), latents_dtype=torch.float32)
        ref.append(lat.cpu())
    del net
    torch.cuda.empty_cache()
    assert t_p.cur == t_o.cur and pipe.last_stats["window_steps"] == st["window_steps"] > 0
    errs = [rel_l2(out[p:p + 1], ref[p]) for p in range(P)]
    print(f"full SD3-medium, 10-step loop, bf16x3 + fp32 latents ({st['window_steps']} window steps): rel L2 vs the pure-fp32 oracle "
          f"{['%.2e' % e for e in errs]}")
    assert max(errs) <= 1.3e-5                                            # measured 6.3e-6 / 6.5e-6
