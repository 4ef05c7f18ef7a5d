"""Projected CLIP text encoders (SD-v3 text_encoder / text_encoder_2) on the GPU: libsdn's plan against the transformers fixture,
the new operators alone (erf-GELU GEMM epilogue against float64, the end-token row kernel against torch), exact properties
(causality, pooling positions, strided outputs), full-size parity against the torch oracle on the GPU, and the SD-v3 pipeline
driven from prompt strings with all three encoders on the engine.  Measured distances go to profiles/clip_proj_parity.json."""
import ctypes as C
import json
import math
import os

import pytest
import torch

import safe_denoiser_amd as sda
from safe_denoiser_amd import _lib, checkpoint
from safe_denoiser_amd.clip import CLIPTextModelWithProjection
from safe_denoiser_amd.text_sd3 import SD3TextFrontEnd
from tests_support import clip_proj_oracle as O
from tests_support import exact as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "clip_proj_parity.json")
G = O.load_golden()
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
F32_BOUND = {"fp32": 2e-5, "bf16x3": 5e-5}          # the bounds tests/test_gpu_clip.py holds the same plan to
ACT = {"quick_gelu": 4, "gelu": 7}


def record(key, value, bound):
    data = {}
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            data = json.load(f)
    data[key] = {"measured": value, "bound": bound}
    with open(PARITY, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def small(arm, dtype=torch.bfloat16, precision=None, clip_skip=None):
    m = CLIPTextModelWithProjection(dtype=dtype, precision=precision, clip_skip=clip_skip, **checkpoint.clip_projection_kwargs(G[f"{arm}/cfg"]))
    m.load_state_dict(O.golden_state_dict(G, arm))
    return m


def gold(arm, name):
    return torch.from_numpy(G[f"{arm}/{name}"])


# ---------------------------------------------------------------------------------------------- 1. engine vs fixture
@pytest.mark.parametrize("arm", O.ARMS)
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_engine_matches_the_transformers_fixture(tag, arm):
    """Bound = 2 x the distance of transformers' own run at that storage width from its fp32 run (recorded in the fixture)."""
    m = small(arm, DT[tag])
    out = m(gold(arm, "ids"), output_hidden_states=True)
    h, e = out.hidden_states[-2], out[0]
    assert e is out.text_embeds and h.dtype == e.dtype == DT[tag]
    assert tuple(h.shape) == tuple(gold(arm, "h2").shape) and tuple(e.shape) == tuple(gold(arm, "text_embeds").shape)
    assert torch.isfinite(h.float()).all() and torch.isfinite(e.float()).all()
    for q, got in (("h2", h), ("text_embeds", e)):
        err, bound = O.rel_l2(got.float(), gold(arm, q)), 2.0 * float(G[f"{arm}/err_{tag}_{q}"])
        print(f"clip proj {tag} arm {arm} {q}: rel L2 {err:.3e} (transformers at this width {bound / 2:.3e}, bound {bound:.3e})")
        record(f"fixture/{tag}/{arm}/{q}", err, bound)
        assert err <= bound
    with pytest.raises(sda.SdnError, match=r"hidden_states\[-2\]"):
        out.hidden_states[-1]
    with pytest.raises(sda.SdnError):
        out.hidden_states[-3]


@pytest.mark.parametrize("arm", O.ARMS)
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_fp32_storage_modes_match_the_fixture(precision, arm):
    m = small(arm, precision=precision)
    out = m(gold(arm, "ids"), output_hidden_states=True)
    assert out.hidden_states[-2].dtype == torch.float32 and out.text_embeds.dtype == torch.float32
    for q, got in (("h2", out.hidden_states[-2]), ("text_embeds", out.text_embeds)):
        err = O.rel_l2(got, gold(arm, q))
        print(f"clip proj {precision} arm {arm} {q}: rel L2 {err:.3e} (bound {F32_BOUND[precision]:.1e})")
        record(f"fixture/{precision}/{arm}/{q}", err, F32_BOUND[precision])
        assert err <= F32_BOUND[precision]


@pytest.mark.parametrize("arm", O.ARMS)
def test_clip_skip_one_returns_hidden_states_minus_three(arm):
    m = small(arm, precision="fp32", clip_skip=1)
    out = m(gold(arm, "ids"), output_hidden_states=True)
    got = out.hidden_states[-(1 + 2)]                              # the reference's own indexing, :386
    assert O.rel_l2(got, gold(arm, "h3")) <= F32_BOUND["fp32"]
    assert O.rel_l2(got, gold(arm, "h2")) > 0.05                   # ... and it is another layer's output
    assert O.rel_l2(out.text_embeds, gold(arm, "text_embeds")) <= F32_BOUND["fp32"]      # the pooled vector does not move with the tap
    with pytest.raises(sda.SdnError, match=r"hidden_states\[-3\]"):
        out.hidden_states[-2]


@pytest.mark.parametrize("arm", O.ARMS)
def test_tapped_state_is_not_final_normed_and_last_layer_tap(arm):
    sd = O.golden_state_dict(G, arm)
    h = small(arm, precision="fp32")(gold(arm, "ids")).hidden_states[-2].cpu()
    assert O.rel_l2(h, O.final_norm(sd, gold(arm, "h2"))) > 0.2    # far above any bound of this file
    cfg = G[f"{arm}/cfg"]
    ref = O.clip_text_with_projection(sd, gold(arm, "ids"), num_heads=cfg["num_attention_heads"], hidden_act=cfg["hidden_act"],
                                      eos_token_id=cfg["eos_token_id"])
    # hidden_tap = 1 (the un-normed output of the last layer) through the C interface
    c = _lib.ClipProjConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                            num_layers=cfg["num_hidden_layers"], num_heads=cfg["num_attention_heads"], max_position_embeddings=77, dtype=2,
                            projection_dim=cfg["projection_dim"], act=ACT[cfg["hidden_act"]], eos_token_id=cfg["eos_token_id"], hidden_tap=1)
    hnd = C.c_void_p()
    lib = sda.lib()
    assert lib.sdn_clip_proj_create(C.byref(c), C.byref(hnd)) == 0
    try:
        w = small(arm, precision="fp32")._weights                   # same manifest whatever the tap
        ids = gold(arm, "ids").to(torch.int32).cuda()
        b = ids.shape[0]
        hid = torch.empty(b, 77, cfg["hidden_size"], device="cuda")
        emb = torch.empty(b, cfg["projection_dim"], device="cuda")
        ws = torch.empty(lib.sdn_unet_workspace_bytes(hnd, b), dtype=torch.uint8, device="cuda")
        assert lib.sdn_clip_proj_forward(hnd, w.data_ptr(), ids.data_ptr(), hid.data_ptr(), 77 * cfg["hidden_size"], cfg["hidden_size"],
                                         emb.data_ptr(), cfg["projection_dim"], b, ws.data_ptr(), ws.numel(), _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert O.rel_l2(hid, ref.hidden_states[-1]) <= F32_BOUND["fp32"]
    finally:
        lib.sdn_unet_destroy(hnd)


@pytest.mark.parametrize("arm", O.ARMS)
def test_pooling_positions_are_the_fixtures(arm):
    """The legacy-rule model (arm a) and the first-match model (arm b) pool where transformers pooled; on arm b the other rule
    would pool elsewhere, and text_embeds then differs grossly."""
    cfg = G[f"{arm}/cfg"]
    ids = gold(arm, "ids").to(torch.int32).cuda()
    b = ids.shape[0]
    x = torch.randn(b, 77, 128, device="cuda")
    gam, bet = torch.ones(128, device="cuda"), torch.zeros(128, device="cuda")
    out, pos = torch.empty(b, 128, device="cuda"), torch.full((b,), -1, dtype=torch.int32, device="cuda")
    assert sda.lib().sdn_clip_eos_rows(2, ids.data_ptr(), x.data_ptr(), gam.data_ptr(), bet.data_ptr(), b, 77, 128, cfg["vocab_size"],
                                       cfg["eos_token_id"], 1e-5, out.data_ptr(), pos.data_ptr(), _lib.stream_ptr()) == 0
    assert pos.cpu().tolist() == G[f"{arm}/positions"].tolist()
    if arm == "b":
        wrong = CLIPTextModelWithProjection(precision="fp32", **{**checkpoint.clip_projection_kwargs(cfg), "eos_token_id": 2})
        wrong.load_state_dict(O.golden_state_dict(G, arm))
        assert O.rel_l2(wrong(gold(arm, "ids")).text_embeds, gold(arm, "text_embeds")) > 0.1


@pytest.mark.parametrize("arm,tag", [("a", "bf16"), ("b", "f16")])
def test_causality_is_bit_exact(arm, tag):
    m = small(arm, DT[tag])
    ids = gold(arm, "ids")
    a = m(ids).hidden_states[-2]
    ids2 = ids.clone(); ids2[:, 40:] = 7
    b = m(ids2).hidden_states[-2]
    torch.testing.assert_close(b[:, :40], a[:, :40], rtol=0, atol=0)
    assert float((b[:, 40:].float() - a[:, 40:].float()).abs().max()) > 1e-2


# ---------------------------------------------------------------------------------------------- 2. the erf-GELU epilogue alone
def _gelu_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 1.5 / math.sqrt(K)
    bias = 0.5 * torch.randn(N, generator=g)
    return a, w, bias


def _exact(a, w, bias):
    """float64 on the GPU: (pre-activation, its magnitude S)."""
    A, W, b = a.double().cuda(), w.double().cuda(), bias.double().cuda()
    return (A @ W.t() + b).cpu(), (A.abs() @ W.abs().t() + b.abs()).cpu()


@pytest.mark.parametrize("M", [3149, 200])                        # 13 x 16 tiles of 256 x 320 with a ragged last row block; one small ragged M
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_gelu_gemm_16_bit_against_float64(tag, M):
    """SDN_ACT_GELU on sdn_gemm_bf16 / sdn_gemm_f16 at bigG's feed-forward shape (1280 -> 5120): the criterion of
    tests/test_gpu_gemm_exact.py (tests_support/exact.py) with the exact erf GELU and the documented error of the epilogue's
    gelu_erf, 2.6e-5 absolute (csrc/sdn_gemm_common.h)."""
    dt, N, K = DT[tag], 5120, 1280
    a, w, bias = _gelu_case(M, N, K, M)
    a, w = a.to(dt), w.to(dt)
    buf, view = X.guarded_like((M, N), dt, "cuda")
    ag, wg, bg = X.with_nan_tail(a.cuda(), 8), w.cuda(), bias.cuda()
    d = _lib.GemmDesc(M=M, N=N, K=K, act=7)
    fn = sda.lib().sdn_gemm_bf16 if tag == "bf16" else sda.lib().sdn_gemm_f16
    assert fn(C.byref(d), ag.data_ptr(), None, wg.data_ptr(), bg.data_ptr(), None, None, None, view.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    rec = (C.c_int * 10)()
    sda.lib().sdn_debug_gemm_last_launch(rec, 10)
    assert X.launch_key(list(rec)) == (("dma", 10, 4, 2, 0) if M > 3000 else ("dma", 2, 2, 2, 0)), list(rec)
    pre, s = _exact(a, w, bias)
    s = s + X.subnormal_term(a.double(), w.double(), dt) / X.ACC
    y = X.gelu64(pre)
    st = X.analyse(view.cpu(), y, X.GELU_D * s, e_epi=torch.full_like(y, X.GEGLU_ABS))
    print(f"erf-GELU {tag} [{M},{N},{K}]: max ulp {st['max_ulp']:.3f}, max err / bound {st['max_err_over_tol']:.3f}")
    assert X.failures(st, exact_fn=False, direction=False) == []
    assert X.sentinels_intact(buf, view) == 0


ACC_X3 = 2.0 ** -15     # bf16x3 products per unit of S: each operand is hi + lo to 2^-17 (2 x 2^-17 for the pair) and the dropped lo x lo
                        # term is below 2^-18 (|lo| <= 2^-9 |x|): under 2^-15 with the f32 accumulation's 2^-20 on top


@pytest.mark.parametrize("M", [333, 200])
@pytest.mark.parametrize("mode", ["f32", "x3"])
def test_gelu_gemm_f32_storage_against_float64(mode, M):
    """The same epilogue code of sdn_gemm_f32 / sdn_gemm_x3 (erff): f32 operands and output.  E_epi = 2^-20 |x|, the budget
    tests_support/exact.py gives an exactly evaluated activation."""
    N, K = 5120, 1280
    a, w, bias = _gelu_case(M, N, K, 7 * M)
    buf, view = X.guarded_like((M, N), torch.float32, "cuda")
    ag, wg, bg = X.with_nan_tail(a.cuda(), 8), w.cuda(), bias.cuda()
    d = _lib.GemmDesc(M=M, N=N, K=K, act=7)
    fn = sda.lib().sdn_gemm_f32 if mode == "f32" else sda.lib().sdn_gemm_x3
    assert fn(C.byref(d), ag.data_ptr(), None, wg.data_ptr(), bg.data_ptr(), None, None, None, view.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    pre, s = _exact(a, w, bias)
    if mode == "x3":
        s = s * (ACC_X3 / X.ACC)
    st = X.analyse(view.cpu(), X.gelu64(pre), X.GELU_D * s, e_epi=X.ACT_REL * pre.abs(), dtype=torch.float32)
    print(f"erf-GELU {mode} [{M},{N},{K}]: max err / bound {st['max_err_over_tol']:.3f}, err / S {st['err_over_s']:.3e}")
    assert X.failures(st, exact_fn=False, direction=False) == []
    assert X.sentinels_intact(buf, view) == 0


# ---------------------------------------------------------------------------------------------- 3. the end-token row kernel alone
@pytest.mark.parametrize("eos", [2, 100])
@pytest.mark.parametrize("tag", ["bf16", "f16", "f32"])
def test_eos_rows_against_torch(tag, eos):
    dt = DT.get(tag, torch.float32)
    B, n, Cw, vocab = 9, 77, 1280, 128
    g = torch.Generator().manual_seed(5 + eos)
    ids = torch.randint(3, 100, (B, n), generator=g, dtype=torch.int32)
    ids[:, 0] = 126
    end = 127 if eos == 2 else eos
    for b in range(B):
        for p in torch.randint(1, n, (3,), generator=g).tolist():   # several copies of the end token: the first one pools
            ids[b, p] = end
    ids[0, :] = torch.randint(3, 99, (n,), generator=g, dtype=torch.int32)       # no end token at all
    ids[1, 5], ids[1, 9] = 4000, -7                                 # outside the vocabulary: clamped to 127 / 0 before the rule
    ids[2, n - 1] = end; ids[2, 1:n - 1] = 50                       # the last position
    x = (torch.randn(B, n, Cw, generator=g) * 2 + 0.5).to(dt)
    gam, bet = 0.5 + torch.rand(Cw, generator=g), 0.3 * torch.randn(Cw, generator=g)
    xb, view = X.guarded_like((B, Cw), dt, "cuda")
    pos = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ig, xg, gg, bg = ids.cuda(), x.cuda(), gam.cuda(), bet.cuda()
    code = {"bf16": 0, "f16": 1, "f32": 2}[tag]
    assert sda.lib().sdn_clip_eos_rows(code, ig.data_ptr(), xg.data_ptr(), gg.data_ptr(), bg.data_ptr(), B, n, Cw, vocab, eos, 1e-5,
                                       view.data_ptr(), pos.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    want = O.pool_positions(ids.clamp(0, vocab - 1), eos)
    assert pos.cpu().tolist() == want.tolist()
    assert want[0] == (0 if eos != 2 else int(ids[0].argmax())) and want[2] == n - 1 and (want[1] == 5 if eos == 2 else True)
    rows = x[torch.arange(B), want.long()].double()
    ref = torch.nn.functional.layer_norm(rows, (Cw,), gam.double(), bet.double(), 1e-5)
    err = (view.cpu().double() - ref).abs()
    # one storage rounding of the result + the f32 arithmetic (mean, variance and the affine map: a few 2^-24 of the operands)
    tol = 0.5 * X.ulp(ref, dt) + 2.0 ** -20 * (ref.abs() + bet.double().abs() + 1.0)
    assert bool((err <= tol).all()), float((err / tol).max())
    assert X.sentinels_intact(xb, view) == 0


# ---------------------------------------------------------------------------------------------- 4. strided outputs
@pytest.mark.parametrize("tag", ["bf16", "f16", "f32"])
def test_strided_outputs_equal_cat_and_pad(tag):
    """Both fixture encoders writing column slices of one [B, 333, 4096] and one [B, 2048] buffer = the contiguous calls followed
    by cat and pad, bit for bit; what lies outside the slices is untouched (zero where it was zero)."""
    kw = dict(precision="fp32") if tag == "f32" else dict(dtype=DT[tag])
    dt = DT.get(tag, torch.float32)
    ea, eb = small("a", **kw), small("b", **kw)
    ids_a, ids_b = gold("a", "ids"), gold("b", "ids")
    B = ids_a.shape[0]
    oa, ob = ea(ids_a), eb(ids_b)
    want_h = torch.nn.functional.pad(torch.cat([oa.hidden_states[-2], ob.hidden_states[-2]], dim=-1), (0, 4096 - 256))
    want_e = torch.nn.functional.pad(torch.cat([oa.text_embeds, ob.text_embeds], dim=-1), (0, 2048 - 192))
    hb, hview = X.guarded_like((B, 333, 4096), dt, "cuda")
    eb_, eview = X.guarded_like((B, 2048), dt, "cuda")
    hview.zero_(); eview.zero_()
    ea.forward_into(ids_a, hview[:, :77, :128], eview[:, :64])
    eb.forward_into(ids_b, hview[:, :77, 128:256], eview[:, 64:192])
    torch.cuda.synchronize()
    assert torch.equal(hview[:, :77], want_h) and torch.equal(eview, want_e)
    assert torch.all(hview[:, 77:] == 0) and torch.all(hview[:, :77, 256:] == 0) and torch.all(eview[:, 192:] == 0)
    assert X.sentinels_intact(hb, hview) == 0 and X.sentinels_intact(eb_, eview) == 0
    with pytest.raises(sda.SdnError):
        ea.forward_into(ids_a, hview[:, :77, :64], eview[:, :64])                 # wrong width
    with pytest.raises(sda.SdnError):
        off = 2 if tag == "f32" else 4                                            # 8 bytes into a row
        ea.forward_into(ids_a, hview[:, :77, off:off + 128], eview[:, :64])       # a slice that starts off a 16-byte boundary


def test_output_strides_do_not_outlive_their_forward():
    """One handle writes into padded slices (row strides 256 / 192 of sentinel-filled buffers), then into contiguous tensors: the second
    call writes exactly the contiguous layout and equals a fresh handle's result, and the first call's padding keeps its sentinels."""
    m, fresh = small("a", DT["f16"]), small("a", DT["f16"])
    ids = gold("a", "ids")[:2]
    want = fresh(ids)
    hb, hview = X.guarded_like((2, 80, 256), DT["f16"], "cuda")
    eb, eview = X.guarded_like((2, 192), DT["f16"], "cuda")
    hview.fill_(-7.0); eview.fill_(-7.0)
    m.forward_into(ids, hview[:, :77, :128], eview[:, :64])
    hc, hcv = X.guarded_like((2, 77, 128), DT["f16"], "cuda")
    ec, ecv = X.guarded_like((2, 64), DT["f16"], "cuda")
    m.forward_into(ids, hcv, ecv)
    torch.cuda.synchronize()
    assert torch.equal(hcv, want.hidden_states[-2]) and torch.equal(ecv, want.text_embeds)
    assert X.sentinels_intact(hc, hcv) == 0 and X.sentinels_intact(ec, ecv) == 0
    assert torch.equal(hview[:, :77, :128], want.hidden_states[-2]) and torch.equal(eview[:, :64], want.text_embeds)
    assert torch.all(hview[:, 77:] == -7.0) and torch.all(hview[:, :77, 128:] == -7.0) and torch.all(eview[:, 64:] == -7.0)
    assert X.sentinels_intact(hb, hview) == 0 and X.sentinels_intact(eb, eview) == 0


# ---------------------------------------------------------------------------------------------- 5. full size
def device_state_dict(m, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for name, shape in m.state_dict_shapes().items():
        if len(shape) == 1:
            norm = "layer_norm" in name
            base = 1.0 if (norm and name.endswith("weight")) else 0.0
            sd[name] = base + (0.2 if norm else 0.1) * (torch.rand(shape, generator=g, device="cuda") - 0.5)
        elif "embedding" in name:
            sd[name] = (0.3 * torch.randn(shape, generator=g, device="cuda")).to(m.dtype)
        else:
            amp = (3.0 / shape[1]) ** 0.5 * (2.0 if ".q_proj." in name else 1.0)
            sd[name] = ((torch.rand(shape, generator=g, device="cuda") * 2 - 1) * amp).to(m.dtype)
    return sd


@pytest.mark.parametrize("tag", ["f16", "bf16"])
@pytest.mark.parametrize("name,cfg", [("big_g", O.CLIP_G_CONFIG), ("clip_l", O.CLIP_L_CONFIG)])
def test_full_size_against_the_oracle_on_the_gpu(name, cfg, tag):
    """bigG at 32 layers and CLIP-L at 12, synthetic weights, 8 sequences.  Reference: the tests_support oracle in fp32 on the same
    16-bit weights; bound: 2 x the distance of the SAME oracle evaluated by torch in that 16-bit dtype (the reference's own loss)."""
    dt = DT[tag]
    m = CLIPTextModelWithProjection(dtype=dt, **checkpoint.clip_projection_kwargs(cfg))
    sd = device_state_dict(m, 11)
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(1, 49000, (8, 77), generator=g); ids[:, 0] = 49406
    for b, n in enumerate((9, 30, 76, 3, 50, 17, 64, 1)):
        ids[b, n:] = 49407
    ids = ids.cuda()
    kw = dict(num_heads=cfg["num_attention_heads"], hidden_act=cfg["hidden_act"], eos_token_id=cfg["eos_token_id"])
    with torch.no_grad():
        ref = O.clip_text_with_projection({k: v.float() for k, v in sd.items()}, ids, **kw)
        low = O.clip_text_with_projection({k: v.to(dt) for k, v in sd.items()}, ids, **kw)
        out = m(ids)
    assert tuple(out.hidden_states[-2].shape) == (8, 77, cfg["hidden_size"]) and tuple(out[0].shape) == (8, cfg["projection_dim"])
    for q, got, r, l in (("h2", out.hidden_states[-2], ref.hidden_states[-2], low.hidden_states[-2]),
                         ("text_embeds", out.text_embeds, ref.text_embeds, low.text_embeds)):
        assert torch.isfinite(got.float()).all()
        err, bound = O.rel_l2(got.float(), r), 2.0 * O.rel_l2(l.float(), r)
        print(f"{name} {tag} {q}: rel L2 vs fp32 oracle {err:.3e} (torch at this width {bound / 2:.3e}, bound {bound:.3e})")
        record(f"full_size/{name}/{tag}/{q}", err, bound)
        assert err <= bound


# ---------------------------------------------------------------------------------------------- 6. end to end
def _tiny_t5(dtype):
    from safe_denoiser_amd.t5 import T5EncoderModel
    t5 = T5EncoderModel(dtype=dtype, vocab_size=512, d_model=256, d_kv=64, d_ff=256, num_layers=2, num_heads=2)
    t5.load_state_dict(t5.synthetic_state_dict(9))
    return t5


def _tokenizers():
    a, b = G["a/cfg"], G["b/cfg"]
    return (O.FakeCLIPTokenizer(a["vocab_size"], bos_token_id=a["bos_token_id"], eos_token_id=127, pad_token_id=a["pad_token_id"]),
            O.FakeCLIPTokenizer(b["vocab_size"], bos_token_id=b["bos_token_id"], eos_token_id=b["eos_token_id"], pad_token_id=b["pad_token_id"]))


def test_sd3_pipeline_from_prompt_strings_with_all_three_encoders_on_the_engine():
    from safe_denoiser_amd.mmdit import SD3Transformer2DModel
    from safe_denoiser_amd.pipeline_sd3 import SD3_NEGATIVE_PROMPT_SPACE, SD3SafeDenoiserPipeline
    from safe_denoiser_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from tests_support.t5_oracle import FakeT5Tokenizer
    import tests.test_gpu_mmdit as tm                      # its small MMDiT configuration, read and not edited
    dt = torch.float16
    t5, tok3 = _tiny_t5(dt), FakeT5Tokenizer(vocab_size=512)
    e1, e2 = small("a", dt), small("b", dt)
    k1, k2 = _tokenizers()
    fe = SD3TextFrontEnd(t5, tok3, text_encoder=e1, tokenizer=k1, text_encoder_2=e2, tokenizer_2=k2)
    # the small MMDiT, with the text widths of THIS stack: 128 + 128 CLIP columns <= d_model 256, pooled 64 + 128
    m = SD3Transformer2DModel(text_len=77 + 256, dtype=dt, **{**tm.SMALL, "joint_attention_dim": 256, "pooled_projection_dim": 192})
    m.load_state_dict(m.synthetic_state_dict(5))
    prompts = ["a lustful portrait in oil", "two cats asleep on a red sofa in the evening sun"]
    P = len(prompts)
    tape = torch.randn(P, 1, 16, 16, 16, generator=torch.Generator().manual_seed(3))
    kw = dict(num_inference_steps=4, guidance_scale=3.5, noise_fn=lambda p, shape: tape[p].clone())
    pipe = SD3SafeDenoiserPipeline(m, FlowMatchEulerDiscreteScheduler(), text_front_end=fe)
    out = pipe(prompt=prompts, **kw)
    stats = dict(pipe.last_stats)
    joined = ", ".join(SD3_NEGATIVE_PROMPT_SPACE)
    pe, ne, pp, npp = fe.encode_prompt(prompt=prompts, negative_prompt=[joined] * P)
    assert pe.shape == ne.shape == (P, 333, 256) and pp.shape == npp.shape == (P, 192) and pe.dtype == pp.dtype == dt
    # the four tensors = an assembly made from the encoders called by hand
    for texts, joint, pooled in ((prompts, pe, pp), ([joined] * P, ne, npp)):
        i1 = k1(texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        i2 = k2(texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        o1, o2 = e1(i1, output_hidden_states=True), e2(i2, output_hidden_states=True)
        clip = torch.cat([o1.hidden_states[-2], o2.hidden_states[-2]], dim=-1)
        t5_rows = t5(tok3(texts, padding="max_length", max_length=256, truncation=True).input_ids)[0]
        assert torch.equal(joint, torch.cat([torch.nn.functional.pad(clip, (0, 256 - clip.shape[-1])), t5_rows], dim=-2))
        assert torch.equal(pooled, torch.cat([o1[0], o2[0]], dim=-1))
    masked = [fe.masked_encode_prompt(p) for p in prompts]
    space = fe.encode_negative_prompt_space(SD3_NEGATIVE_PROMPT_SPACE)
    plain = SD3SafeDenoiserPipeline(m, FlowMatchEulerDiscreteScheduler())
    same = plain(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=pp, negative_pooled_prompt_embeds=npp,
                 masked_embs=masked, negspace_embs=space, **kw)
    assert torch.isfinite(out).all() and torch.equal(out, same)
    assert plain.last_stats == stats


def test_from_pretrained_on_a_written_directory(tmp_path):
    from safetensors.torch import save_file
    from tests_support.t5_oracle import FakeT5Tokenizer
    dt = torch.float16
    t5 = _tiny_t5(dt)
    t5_cfg = dict(architectures=["T5EncoderModel"], vocab_size=512, d_model=256, d_kv=64, d_ff=256, num_layers=2, num_heads=2,
                  relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6,
                  feed_forward_proj="gated-gelu", dense_act_fn="gelu_new", is_gated_act=True)
    t5_sd = {"encoder." + k: v.contiguous() for k, v in t5.synthetic_state_dict(9).items()}
    parts = (("text_encoder", dict(G["a/cfg"], architectures=["CLIPTextModelWithProjection"]), O.golden_state_dict(G, "a")),
             ("text_encoder_2", dict(G["b/cfg"], architectures=["CLIPTextModelWithProjection"]), O.golden_state_dict(G, "b")),
             ("text_encoder_3", t5_cfg, t5_sd))
    for sub, cfg, sd in parts:
        (tmp_path / sub).mkdir()
        (tmp_path / sub / "config.json").write_text(json.dumps(cfg))
        save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / sub / "model.safetensors"))
    k1, k2 = _tokenizers()
    tok3 = FakeT5Tokenizer(vocab_size=512)
    fe = SD3TextFrontEnd.from_pretrained(str(tmp_path), tokenizer=k1, tokenizer_2=k2, tokenizer_3=tok3, dtype=dt)
    assert fe.text_encoder.config.hidden_act == "quick_gelu" and fe.text_encoder_2.config.hidden_act == "gelu"
    assert fe.text_encoder_2.config.eos_token_id == 100 and fe.clip_embeds is None and fe.d_model == 256
    by_hand = SD3TextFrontEnd(t5, tok3, text_encoder=small("a", dt), tokenizer=k1, text_encoder_2=small("b", dt), tokenizer_2=k2)
    got, want = fe.encode_prompt(prompt=["a red fox", "snow"], negative_prompt=""), by_hand.encode_prompt(prompt=["a red fox", "snow"], negative_prompt="")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert got[0].shape == (2, 333, 256) and got[2].shape == (2, 192) and float(got[0][:, :77, :256].float().abs().mean()) > 0.05
    (tmp_path / "text_encoder_2" / "config.json").write_text(json.dumps(dict(G["b/cfg"], hidden_act="relu")))
    with pytest.raises(NotImplementedError):
        SD3TextFrontEnd.from_pretrained(str(tmp_path), tokenizer=k1, tokenizer_2=k2, tokenizer_3=tok3, dtype=dt)
