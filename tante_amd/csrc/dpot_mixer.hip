// DPOT's two kernels that no other path of the library serves (reference models/dpot.py): GroupNorm over (channels-in-group x all
// tokens) on channels-last rows, and the truncated-mode Fourier mixer AFNO2D.forward.
//
// ---- tante_groupnorm: torch.nn.GroupNorm(G, C) (dpot.py:138,147) on x (B, HW, C) fp32 ---------------------------------------------------
// Statistics per (b, g) run over HW x C/G elements.  The rows of a group are cut into S <= 64 slabs; launch 1 computes per slab the mean
// FIRST and then the centred sum of squares about that mean (never E[x^2] - mean^2); launch 2 combines the slabs' (n, mean, M2) in slab
// order with the pairwise update  mean += d n_i / n,  M2 += M2_i + d^2 n_old n_i / n  (exact for a partition), normalises and applies the
// affine.  Every sum has a fixed order: lanes by shuffle, waves in order, slabs in order; no atomics.
//
// ---- tante_dpot_filter: AFNO2D.forward (dpot.py:47-102) on x (B, H, W, C) fp32 ----------------------------------------------------------
// With k1 = min(modes, H), k2 = min(modes, W/2 + 1) only the kept corner of the spectrum is ever computed; everything outside it is zero
// (not the bias) and so contributes nothing to the inverse.
//
//   launch 1 (b, h, 64 channels)     P[l, h]  = sum_w T1[l, w] x[h, w]              l < k2    T1 = e^{-2 pi i l w / W} / sqrt(W)
//   launch 2 (b, l, 64 channels)     X[k, l]  = sum_h T2[k, h] P[l, h]              k < k1    T2 = e^{-2 pi i k h / H} / sqrt(H)
//   launch 3 (rows, 16 columns, g)   V = gelu(Re U) + i gelu(Im U),  U = X W1 + b1            complex, per channel block g
//   launch 4 (rows, 16 columns, g)   Y = V W2 + b2
//   launch 5 (b, l, 64 channels)     Z[h, l]  = sum_k T3[h, k] Y[k, l]                        T3 = e^{+2 pi i k h / H} / sqrt(H)
//   launch 6 (b, h, 64 channels)     out[h, w] = Re sum_l T4[w, l] Z[h, l] + x[h, w] (+ residual[h, w])
//                                                                                             T4 = c_l e^{+2 pi i l w / W} / sqrt(W)
//
// c_l = 1 for l = 0 and l = W/2 (W even), 2 otherwise: the complex-to-real weights; the table entries of those two columns are real, so
// their imaginary input drops out by itself.  Launch 1 is dft_r2c_rows_kernel and launch 6 dft_c2r_rows_kernel<DpotInvEpilogue> of
// dft_rows.hip.h, which also holds the table layout and the table product; launches 2 .. 5, GroupNorm's kernels and the plans live in
// dpot_mixer.hip.h, which the backward (dpot_mixer_bwd.hip) shares; this file holds the entry points.
//
// The block MLP reads w1 / w2 (2, nb, bs, bs) and b1 / b2 (2, nb, bs) as the state dict holds them and evaluates the four real products
// Re = Xr Wr - Xi Wi, Im = Xi Wr + Xr Wi.  Its rows are few (B k1 k2: 40 per sample at the reference's config) against 2 x nb x bs^2
// weights per layer, so its grid is cut by WEIGHT bytes: a workgroup owns 16 output columns of one channel block and all (up to 192) rows,
// its four waves split K, and the partial tiles meet in LDS in wave order.  Each weight element is read from memory once per 192 rows.
// The activations between launches 2 .. 5 live in a layout of this kernel's own, (g, row, [re | im], bsP) with bsP = bs rounded up to 16
// and the padding written as zeros, so a block size that is no multiple of 4 or 16 costs the MLP no bounds test on its row operand.
//
// Every product is v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation, in both compute modes.  A operand lane (i = l & 15,
// k = l >> 4), B operand lane (k = l >> 4, j = l & 15), result register r = row 4 (l >> 4) + r, column l & 15.  LDS is plain C++ between
// barriers: no hand-placed waits.
#include "dpot_mixer.hip.h"

extern "C" int tante_groupnorm_supported(int64_t B, int HW, int C, int G) { return gn_reason(B, HW, C, G) == nullptr ? 1 : 0; }

extern "C" int64_t tante_groupnorm_workspace_bytes(int64_t B, int HW, int C, int G) {
  if (gn_reason(B, HW, C, G)) return -1;
  return (int64_t)sizeof(float) * 2 * B * G * gn_plan(HW, C, G).S;
}

extern "C" int tante_groupnorm(const float* x, int64_t B, int HW, int C, int G, float eps, const float* gamma, const float* beta, void* y,
                               int y_dtype, void* work, int64_t work_bytes, void* stream) {
  if (const char* why = gn_reason(B, HW, C, G)) TANTE_FAIL(-2, "tante_groupnorm: %s (B %lld, tokens %d, C %d, groups %d)", why, (long long)B, HW, C, G);
  if (y_dtype != TANTE_F32 && y_dtype != TANTE_BF16) TANTE_FAIL(-1, "tante_groupnorm: output dtype must be fp32 or bf16");
  if (!x || !y) TANTE_FAIL(-1, "tante_groupnorm: null argument");
  if (B == 0) return 0;
  const int64_t need = tante_groupnorm_workspace_bytes(B, HW, C, G);
  if (!work || work_bytes < need) TANTE_FAIL(-1, "tante_groupnorm: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  const GnPlan p = gn_plan(HW, C, G);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * G), (unsigned)p.S);
  hipLaunchKernelGGL(gn_stats_kernel, grid, dim3(DP_THREADS), 0, s, x, (float*)work, HW, C, G, p.cg, p.R, p.S);
  TANTE_CHECK_LAUNCH();
  if (y_dtype == TANTE_BF16)
    hipLaunchKernelGGL(gn_apply_kernel<true>, grid, dim3(DP_THREADS), 0, s, x, (const float*)work, gamma, beta, y, HW, C, G, p.cg, p.R, p.S, eps);
  else
    hipLaunchKernelGGL(gn_apply_kernel<false>, grid, dim3(DP_THREADS), 0, s, x, (const float*)work, gamma, beta, y, HW, C, G, p.cg, p.R, p.S, eps);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_dpot_filter_supported(int64_t B, int H, int W, int C, int bs, int modes, int hidden_factor) {
  return dp_reason(B, H, W, C, bs, modes, hidden_factor) == nullptr ? 1 : 0;
}

extern "C" int64_t tante_dpot_twiddle_floats(int H, int W, int modes) {
  if (H < 1 || W < 1 || H > DP_MAX || W > DP_MAX || modes < 1) return -1;
  return dp_tables(H, W, modes).total;
}

extern "C" int64_t tante_dpot_filter_workspace_bytes(int64_t B, int H, int W, int C, int bs, int modes) {
  if (dp_reason(B, H, W, C, bs, modes, 1)) return -1;
  return (int64_t)sizeof(float) * dp_work(B, H, W, C, bs, modes).total;
}

extern "C" int tante_dpot_filter(const float* x, const float* residual, int64_t B, int H, int W, int C, int bs, int modes, int hidden_factor,
                                 const float* twiddles, const float* w1, const float* b1, const float* w2, const float* b2, float* out, void* work,
                                 int64_t work_bytes, void* stream) {
  if (const char* why = dp_reason(B, H, W, C, bs, modes, hidden_factor))
    TANTE_FAIL(-2, "tante_dpot_filter: %s (B %lld, grid %d x %d, C %d, block %d, modes %d, hidden_size_factor %d)", why, (long long)B, H, W, C, bs, modes,
               hidden_factor);
  if (!x || !twiddles || !w1 || !b1 || !w2 || !b2 || !out) TANTE_FAIL(-1, "tante_dpot_filter: null argument");
  if (x == out) TANTE_FAIL(-1, "tante_dpot_filter: out may alias residual, not x");
  if (B == 0) return 0;
  const DpWork k = dp_work(B, H, W, C, bs, modes);
  const int64_t need = (int64_t)sizeof(float) * k.total;
  if (!work || work_bytes < need) TANTE_FAIL(-1, "tante_dpot_filter: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  if ((uintptr_t)work % 16) TANTE_FAIL(-1, "tante_dpot_filter: the workspace must be 16-byte aligned");
  const DpTables t = dp_tables(H, W, modes);
  const int nb = C / bs, bsP = r16(bs);
  float* P = (float*)work;          // and Z
  float* X = P + k.spat;            // and Y
  float* V = X + k.blk;
  hipStream_t s = (hipStream_t)stream;
  const unsigned cch = (unsigned)((C + DFT_CH - 1) / DFT_CH), pch = (unsigned)((nb * bsP + DFT_CH - 1) / DFT_CH);
  const dim3 mlp_grid((unsigned)((k.Mtot + 16 * DP_MT - 1) / (16 * DP_MT)), (unsigned)(bsP / 16), (unsigned)nb);
  const long C1 = C, C2 = 2l * C;
  const DftRows fwd_w = {H * W * C1, W * C1, C1, t.k2 * H * C2, C2, H * C2, H};       // x rows (b, h) -> P[b][l][h]
  const DftRows inv_w = {H * t.k2 * C2, t.k2 * C2, C2, H * W * C1, W * C1, C1, H};    // Z[b][h] -> out rows (b, h)
  hipLaunchKernelGGL(dft_r2c_rows_kernel, dim3((unsigned)(B * H), cch), dim3(DFT_THREADS), 0, s, x, twiddles + t.re[0], twiddles + t.im[0], t.Kp[0], P,
                     fwd_w, W, t.k2, C);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dpot_fwd_h_kernel, dim3((unsigned)t.k2, pch, (unsigned)B), dim3(DP_THREADS), 0, s, (const float*)P, twiddles + t.re[1],
                     twiddles + t.im[1], t.Kp[1], X, H, C, bs, bsP, nb, t.k1, t.k2, k.Mtot);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dpot_mlp_kernel<true>, mlp_grid, dim3(DP_THREADS), 0, s, (const float*)X, w1, b1, V, k.Mtot, nb, bs, bsP);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dpot_mlp_kernel<false>, mlp_grid, dim3(DP_THREADS), 0, s, (const float*)V, w2, b2, X, k.Mtot, nb, bs, bsP);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dpot_inv_h_kernel, dim3((unsigned)t.k2, cch, (unsigned)B), dim3(DP_THREADS), 0, s, (const float*)X, twiddles + t.re[2],
                     twiddles + t.im[2], t.Kp[2], P, H, C, bs, bsP, t.k1, t.k2, k.Mtot);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dft_c2r_rows_kernel<DpotInvEpilogue>, dim3((unsigned)(B * H), cch), dim3(DFT_THREADS), 0, s, (const float*)P, twiddles + t.re[3],
                     twiddles + t.im[3], t.Kp[3], out, inv_w, t.k2, W, C, DpotInvEpilogue{x, residual});
  TANTE_CHECK_LAUNCH();
  return 0;
}
