// Internal (non-ABI) declarations shared between the translation units of libsdn.
#pragma once
#include "../../include/sdn.h"

int sdn_gemm_pick_nrep(int n_padded, int act);
// NREP actually launched for this shape (10 / 8 = the 256-row, 8-wave tile; 5 / 4 / 2 / 1 = the 128-row tile).
// epilogue_reads: the epilogue fetches a residual tile / row gates (keeps short k loops on the 2-blocks-per-CU tile).
int sdn_gemm_pick_tile(int M, int N, int K, int act, int epilogue_reads = 0);

// graph mode of the plan runner: the step's timestep lives in device memory so that a captured forward can be replayed
int sdn_temb_from_device(int dtype, const float* t_dev, int batch, int dim, void* out, void* stream);
int sdn_set_scalar(float* dst, float v, void* stream);

// k-loop slices the split-K form should use for this shape (1 = do not split)
int sdn_gemm_pick_split(int M, int N, int K, int act, int out_kind);

// fp32 precision mode (sdn_f32.hip): timestep features from a host scalar or from device memory (graph mode)
int sdn_temb_f32(float timestep, const float* t_dev, int batch, int dim, void* out, void* stream);

// Two linears with nothing but a residual between them, out = Wb (h + Wa f + ba) + bb, as one contraction over [f | h]:
// w_cat [C][K + C] = [Wb Wa | Wb] (16 bit, product formed in fp32 and rounded once), b_cat[C] = Wb ba + bb.
// wa [C][K], wb [C][C] in the plan's 16-bit dtype (0 = bf16, 1 = f16).  Prepare-time helper (sdn_unet_prepare).
int sdn_linear_pair_fold(int dtype, const void* wa, const void* wb, const float* ba, const float* bb, int C, int K, void* w_cat,
                         float* b_cat, void* stream);


// 3x3 convolutions the slab-ring kernel (sdn_conv.hip) takes over from the implicit-GEMM tile: shape part of the test
// (square side x side map, M = batch * side^2 output rows, N padded output channels).
int sdn_conv_slab_shape_ok(int M, int N, int Cin, int side, int stride, int upsample, int asym_pad, int out_kind, int n_valid);

// Upsampler convs (3x3 over a nearest-2x upsampled Hs x Ws map) that take the phase form (sdn_gemm_desc.upsample = 2): the
// 256-row tile that serves N (10 or 8), or 0 when the shape does not qualify -- Hs Ws a multiple of 256 (whole tiles per sample
// and phase), Ws >= 8, Cin a multiple of 64.  Depends on the architecture only, never on the batch.
int sdn_conv_up4_tile(int Hs, int Ws, int Cin, int N);

// Launch record of the normalisation family (host side, diagnostics only: sdn_debug_norm_last_launch), set by the launchers of
// sdn_norm.hip and sdn_f32.hip where the kernel is chosen.  kernel: 1 k_gn_stats + k_gn_finalize + k_gn_apply, 2 k_gn_finalize_cols
// + k_gn_apply, 3 k_layernorm, 4 k_layernorm (adaLN), 5 k_row_stats, 6 k_gn_rows_stats + k_gn_rows_apply, 7 k_groupnorm_f32,
// 8 k_groupnorm_f32_any, 9 k_layernorm_f32_regs, 10 k_layernorm_f32, 11 k_layernorm_mod_f32.  dtype: 0 bf16, 1 f16, 2 f32.
// Fields a kernel does not have are 0.
enum { SDN_NL_KERNEL, SDN_NL_DTYPE, SDN_NL_NQ, SDN_NL_R, SDN_NL_NCH, SDN_NL_CT, SDN_NL_NTILES, SDN_NL_ROWS_PER_TILE, SDN_NL_RPC,
       SDN_NL_NCHUNK, SDN_NL_STATS_SRC, SDN_NL_TRIPLE, SDN_NL_COUNT };
struct sdn_norm_launch { int kernel, dtype, nq, r, nch, ct, ntiles, rows_per_tile, rpc, nchunk, stats_src, triple; };
void record_norm_launch(const sdn_norm_launch& l);
