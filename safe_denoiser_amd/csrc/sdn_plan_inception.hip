// Launch planner, Inception-v3 pool3 tower (the FID / KID feature extractor): build_inception() and its C entry points.
#include "sdn_plan.h"

namespace sdn_plan {

// =================================================================================================
// `InceptionV3([3])(x)[0]` of pytorch-fid as the reference vendors it (evaluations/utils/inception.py:16-163): torchvision's
// Inception3 trunk (third party; its wiring is restated here) with the FID patches of inception.py:197-341.  BasicConv2d = conv
// without bias + BatchNorm(eps 1e-3) + ReLU; the loader folds the norm into the weight and a bias, so a BasicConv2d is ONE GEMM
// with a bias + ReLU epilogue over patch rows (or over the map itself: 1x1, stride 1, channels % 64 == 0), written into its
// channel slice of the block's concatenation.  fp32 storage, sdn_gemm_f32 throughout.
// =================================================================================================
static int up(int v, int m) { return (v + m - 1) / m * m; }

// `out` is the [rows, out.C] map the result is a channel slice of (columns c0 .. c0 + cout)
void Builder::inception_conv(const std::string& name, const Act& in, int cout, int kh, int kw, int stride, int ph, int pw, const Act& out,
                             int c0) {
  const int cin = in.C, kpad = up(kh * kw * cin, 64), npad = up(cout, 32);
  const int so = (in.side + 2 * ph - kh) / stride + 1;                     // maps are square and so are their outputs (1x7 pads (0, 3))
  const int64_t M = (int64_t)B * so * so;
  if (u->param_index.find(name + ".conv.weight") == u->param_index.end()) {
    sdn_inception_conv ci; memset(&ci, 0, sizeof(ci));
    snprintf(ci.name, sizeof(ci.name), "%s", name.c_str());
    ci.cin = cin; ci.cout = cout; ci.kh = kh; ci.kw = kw; ci.stride = stride; ci.pad_h = ph; ci.pad_w = pw; ci.kpad = kpad; ci.n_padded = npad;
    u->convs.push_back(ci);
  }
  Ref w = param(name + ".conv.weight", SDN_P_MAT, cout, kpad, npad);
  param(name + ".bn.weight", SDN_P_VEC_F32, cout, 0);
  Ref bias = param(name + ".bn.bias", SDN_P_VEC_F32, cout, 0, npad);        // the folded bias: the epilogue reads n_padded floats
  param(name + ".bn.running_mean", SDN_P_VEC_F32, cout, 0);
  param(name + ".bn.running_var", SDN_P_VEC_F32, cout, 0);
  if (so != out.side || c0 + cout > out.C || (c0 & 3) || so < 1) plan_bad = true;
  const bool direct = kh == 1 && kw == 1 && stride == 1 && cin % 64 == 0;
  Act pr; Ref a = R(in);
  if (!direct) {
    if (M * kpad * 4 >= ((int64_t)1 << 31)) plan_bad = true;                 // callers chunk the batch (include/sdn.h)
    pr = act(M, kpad, so * so, so);
    Op o; o.kind = OP_CONV_ROWS; o.a = R(in); o.out = R(pr); o.batch = B; o.hw = in.side; o.c1 = cin; o.c2 = kpad;
    o.kh = kh; o.kw = kw; o.sh = o.sw = stride; o.ph = ph; o.pw = pw; o.rows = M;
    o.bytes = 4.0 * ((double)B * in.side * in.side * cin + (double)M * kpad);
    snprintf(o.label, sizeof(o.label), "k_patch_rows_f32"); emit(o);
    a = R(pr);
  }
  Op o; o.kind = OP_GEMM; memset(&o.gd, 0, sizeof(o.gd));
  o.gd.M = (int)M; o.gd.N = npad; o.gd.K = kpad; o.gd.a_mode = SDN_A_PLAIN; o.gd.act = SDN_ACT_RELU; o.gd.out_kind = SDN_OUT_F32;
  o.gd.n_valid = cout; o.gd.ldc = out.C;
  o.a = a; o.w = w; o.bias = bias; o.out = Ref{SP_WS, out.off + (int64_t)c0 * 4};
  o.flops = 2.0 * (double)M * cout * (double)(kh * kw * cin);               // the convolution's own count: padding columns are not work
  o.bytes = 4.0 * ((double)M * kpad + (double)npad * kpad + (double)M * cout);
  snprintf(o.label, sizeof(o.label), "k_gemm_f32"); emit(o);
  if (pr.off >= 0) drop(pr);                                                // stream order: the next op may reuse it
}

Act Builder::inception_conv_new(const std::string& name, const Act& in, int cout, int kh, int kw, int stride, int ph, int pw) {
  const int so = (in.side + 2 * ph - kh) / stride + 1;
  Act out = act((int64_t)B * so * so, cout, so * so, so);
  inception_conv(name, in, cout, kh, kw, stride, ph, pw, out, 0);
  return out;
}

void Builder::inception_pool(int mode, const Act& in, int stride, int pad, const Act& out, int c0) {
  const int so = (in.side + 2 * pad - 3) / stride + 1;
  if (so != out.side || c0 + in.C > out.C || so < 1) plan_bad = true;
  Op o; o.kind = OP_POOL3; o.mod = mode; o.a = R(in); o.out = R(out); o.batch = B; o.hw = in.side; o.c1 = in.C; o.sh = stride; o.ph = pad;
  o.ldo = out.C; o.c2 = c0; o.rows = (int64_t)B * so * so;
  o.bytes = 4.0 * ((double)B * in.side * in.side * in.C + (double)o.rows * in.C);
  snprintf(o.label, sizeof(o.label), "k_pool3_f32"); emit(o);
}

void Builder::build_inception() {
  const sdn_inception_config& c = u->icfg;
  const int S = c.image_size;
  auto map = [&](int side, int C) { return act((int64_t)B * side * side, C, side * side, side); };
  auto pooled = [&](int mode, const Act& in, int stride, int pad) {
    Act t = map((in.side + 2 * pad - 3) / stride + 1, in.C);
    inception_pool(mode, in, stride, pad, t, 0);
    return t;
  };

  // resize (or layout change) + input scaling: NCHW pixels -> NHWC [B, S, S, 3]; o.scale x + o.eps
  Act x = map(S, 3);
  { Op o; o.kind = OP_RESIZE; o.a = Ref{SP_IN, 0}; o.out = R(x); o.batch = B; o.hw = S; o.scale = c.normalize_input ? 2.f : 1.f;
    o.eps = c.normalize_input ? -1.f : 0.f; o.rows = (int64_t)B * S * S; o.bytes = 2.0 * 12.0 * B * S * S;
    snprintf(o.label, sizeof(o.label), "k_resize_bilinear_f32"); emit(o); }

  // ---- stem: Conv2d_1a_3x3 .. Conv2d_4a_3x3 with the two max pools ----
  Act t = inception_conv_new("Conv2d_1a_3x3", x, 32, 3, 3, 2); drop(x);
  x = inception_conv_new("Conv2d_2a_3x3", t, 32, 3, 3); drop(t);
  t = inception_conv_new("Conv2d_2b_3x3", x, 64, 3, 3, 1, 1, 1); drop(x);
  x = pooled(SDN_POOL_MAX, t, 2, 0); drop(t);
  t = inception_conv_new("Conv2d_3b_1x1", x, 80); drop(x);
  x = inception_conv_new("Conv2d_4a_3x3", t, 192, 3, 3); drop(t);
  t = pooled(SDN_POOL_MAX, x, 2, 0); drop(x);
  x = t;

  // ---- Mixed_5b / 5c / 5d: InceptionA, pad-excluding average pool ----
  const int pool_features[3] = {32, 64, 64};
  for (int i = 0; i < 3; ++i) {
    const std::string p = std::string("Mixed_5") + "bcd"[i];
    Act y = map(x.side, 224 + pool_features[i]);
    inception_conv(p + ".branch1x1", x, 64, 1, 1, 1, 0, 0, y, 0);
    Act a = inception_conv_new(p + ".branch5x5_1", x, 48);
    inception_conv(p + ".branch5x5_2", a, 64, 5, 5, 1, 2, 2, y, 64); drop(a);
    a = inception_conv_new(p + ".branch3x3dbl_1", x, 64);
    Act b = inception_conv_new(p + ".branch3x3dbl_2", a, 96, 3, 3, 1, 1, 1); drop(a);
    inception_conv(p + ".branch3x3dbl_3", b, 96, 3, 3, 1, 1, 1, y, 128); drop(b);
    a = pooled(SDN_POOL_AVG_NOPAD, x, 1, 1);
    inception_conv(p + ".branch_pool", a, pool_features[i], 1, 1, 1, 0, 0, y, 224); drop(a);
    drop(x); x = y;
  }

  // ---- Mixed_6a: InceptionB (grid reduction) ----
  {
    const std::string p = "Mixed_6a";
    Act y = map((x.side - 3) / 2 + 1, 384 + 96 + x.C);
    inception_conv(p + ".branch3x3", x, 384, 3, 3, 2, 0, 0, y, 0);
    Act a = inception_conv_new(p + ".branch3x3dbl_1", x, 64);
    Act b = inception_conv_new(p + ".branch3x3dbl_2", a, 96, 3, 3, 1, 1, 1); drop(a);
    inception_conv(p + ".branch3x3dbl_3", b, 96, 3, 3, 2, 0, 0, y, 384); drop(b);
    inception_pool(SDN_POOL_MAX, x, 2, 0, y, 480);
    drop(x); x = y;
  }

  // ---- Mixed_6b .. 6e: InceptionC (factorised 7x7), pad-excluding average pool ----
  const int c7s[4] = {128, 160, 160, 192};
  for (int i = 0; i < 4; ++i) {
    const std::string p = std::string("Mixed_6") + "bcde"[i];
    const int c7 = c7s[i];
    Act y = map(x.side, 768);
    inception_conv(p + ".branch1x1", x, 192, 1, 1, 1, 0, 0, y, 0);
    Act a = inception_conv_new(p + ".branch7x7_1", x, c7);
    Act b = inception_conv_new(p + ".branch7x7_2", a, c7, 1, 7, 1, 0, 3); drop(a);
    inception_conv(p + ".branch7x7_3", b, 192, 7, 1, 1, 3, 0, y, 192); drop(b);
    a = inception_conv_new(p + ".branch7x7dbl_1", x, c7);
    b = inception_conv_new(p + ".branch7x7dbl_2", a, c7, 7, 1, 1, 3, 0); drop(a);
    a = inception_conv_new(p + ".branch7x7dbl_3", b, c7, 1, 7, 1, 0, 3); drop(b);
    b = inception_conv_new(p + ".branch7x7dbl_4", a, c7, 7, 1, 1, 3, 0); drop(a);
    inception_conv(p + ".branch7x7dbl_5", b, 192, 1, 7, 1, 0, 3, y, 384); drop(b);
    a = pooled(SDN_POOL_AVG_NOPAD, x, 1, 1);
    inception_conv(p + ".branch_pool", a, 192, 1, 1, 1, 0, 0, y, 576); drop(a);
    drop(x); x = y;
  }

  // ---- Mixed_7a: InceptionD (grid reduction) ----
  {
    const std::string p = "Mixed_7a";
    Act y = map((x.side - 3) / 2 + 1, 320 + 192 + x.C);
    Act a = inception_conv_new(p + ".branch3x3_1", x, 192);
    inception_conv(p + ".branch3x3_2", a, 320, 3, 3, 2, 0, 0, y, 0); drop(a);
    a = inception_conv_new(p + ".branch7x7x3_1", x, 192);
    Act b = inception_conv_new(p + ".branch7x7x3_2", a, 192, 1, 7, 1, 0, 3); drop(a);
    a = inception_conv_new(p + ".branch7x7x3_3", b, 192, 7, 1, 1, 3, 0); drop(b);
    inception_conv(p + ".branch7x7x3_4", a, 192, 3, 3, 2, 0, 0, y, 320); drop(a);
    inception_pool(SDN_POOL_MAX, x, 2, 0, y, 512);
    drop(x); x = y;
  }

  // ---- Mixed_7b (average pool) and Mixed_7c (MAX pool: inception.py:333-337): InceptionE ----
  for (int i = 0; i < 2; ++i) {
    const std::string p = std::string("Mixed_7") + "bc"[i];
    Act y = map(x.side, 2048);
    inception_conv(p + ".branch1x1", x, 320, 1, 1, 1, 0, 0, y, 0);
    Act a = inception_conv_new(p + ".branch3x3_1", x, 384);
    inception_conv(p + ".branch3x3_2a", a, 384, 1, 3, 1, 0, 1, y, 320);
    inception_conv(p + ".branch3x3_2b", a, 384, 3, 1, 1, 1, 0, y, 704); drop(a);
    a = inception_conv_new(p + ".branch3x3dbl_1", x, 448);
    Act b = inception_conv_new(p + ".branch3x3dbl_2", a, 384, 3, 3, 1, 1, 1); drop(a);
    inception_conv(p + ".branch3x3dbl_3a", b, 384, 1, 3, 1, 0, 1, y, 1088);
    inception_conv(p + ".branch3x3dbl_3b", b, 384, 3, 1, 1, 1, 0, y, 1472); drop(b);
    a = pooled(i == 0 ? SDN_POOL_AVG_NOPAD : SDN_POOL_MAX, x, 1, 1);
    inception_conv(p + ".branch_pool", a, 192, 1, 1, 1, 0, 0, y, 1856); drop(a);
    drop(x); x = y;
  }

  // ---- AdaptiveAvgPool2d(1) -> features [B, 2048] ----
  { Op o; o.kind = OP_SPATIAL_MEAN; o.a = R(x); o.out = Ref{SP_OUT, 0}; o.batch = B; o.hw = x.side * x.side; o.c1 = x.C; o.rows = B;
    o.bytes = 4.0 * ((double)B * o.hw * x.C + (double)B * x.C);
    snprintf(o.label, sizeof(o.label), "k_spatial_mean_f32"); emit(o); }
  drop(x);
  plan->ws_bytes = arena.peak;
}

}  // namespace sdn_plan

using namespace sdn_plan;

extern "C" int sdn_inception_create(const sdn_inception_config* cfg, sdn_unet** out) {
  if (!cfg || !out) return SDN_E_INVALID;
  // 75: the smallest side at which Mixed_7a still has an output pixel; dtype: fp32 storage only (FID is quoted to two decimals)
  if (cfg->image_size < 75 || cfg->image_size > 1024 || (cfg->normalize_input != 0 && cfg->normalize_input != 1) || cfg->dtype != 2)
    return SDN_E_INVALID;
  sdn_unet* u = new sdn_unet();
  memset(&u->cfg, 0, sizeof(u->cfg));
  u->icfg = *cfg;
  u->kind = INCEPTION;
  get_plan(u, 1);                                               // registers the parameter manifest (batch-independent)
  *out = u;
  return SDN_OK;
}

extern "C" int sdn_inception_conv_count(const sdn_unet* m) { return (m && m->kind == INCEPTION) ? (int)m->convs.size() : 0; }

extern "C" int sdn_inception_conv_info(const sdn_unet* m, int32_t index, sdn_inception_conv* info) {
  if (!m || m->kind != INCEPTION || !info || index < 0 || index >= (int)m->convs.size()) return SDN_E_INVALID;
  *info = m->convs[index];
  return SDN_OK;
}

extern "C" int sdn_inception_forward(sdn_unet* m, const void* weights, const float* pixels, float* features, int32_t batch, int32_t h,
                                     int32_t w, int32_t resize, void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || m->kind != INCEPTION || !pixels || !features) return SDN_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(pixels) & 3) || (reinterpret_cast<uintptr_t>(features) & 3)) return SDN_E_INVALID;   // (image n of a batch is welcome)
  if (h < 1 || w < 1 || h > 8192 || w > 8192 || (resize != 0 && resize != 1)) return SDN_E_INVALID;
  if (!resize && (h != m->icfg.image_size || w != m->icfg.image_size)) return SDN_E_INVALID;
  Call call(weights, workspace, workspace_bytes, batch, stream);
  call.in = pixels; call.out = features; call.in_h = h; call.in_w = w;
  return run_plan(m, call);
}
