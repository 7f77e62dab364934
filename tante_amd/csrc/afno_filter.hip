// AFNO spectral filter (reference models/afno.py:103-117 + the axis swap and first skip of Block.forward, l.151-160) on channels-last
// fp32 rows (b, H, W, C):
//
//   X = rfftn(x, dim=(2, 1), 'ortho')            half spectrum over axis 1 (k = 0..H/2), full transform over axis 2 (l = 0..W-1)
//   Y = softshrink(W2 . gelu_erf(W1 . X))        block-diagonal complex two-layer MLP over channel blocks of `bs`, no bias
//   o = irfftn(Y, s=(H, W), dim=(2, 1), 'ortho') the SIZES are swapped: axis 2 gets an H-point inverse of its first min(W, H) entries,
//                                                axis 1 a W-point complex-to-real inverse of its first min(H/2+1, W/2+1) entries
//   out[h, w] = o[w, h] + residual[h, w]         (the filter returns (b, W, H, C); Block.forward swaps the axes back)
//
// With Lc = min(H, W) and Kc = min(H/2 + 1, W/2 + 1), everything the inverse drops is never computed:
//
//   launch 1 (b, h, 64 channels)  P[l, h]  = sum_w  T1[l, w] x[h, w]             l < Lc   T1 = e^{-2 pi i l w / W} / sqrt(W)
//   launch 2 (b, l, channel block) X[k]    = sum_h  T2[k, h] P[l, h]              k < Kc   T2 = e^{-2 pi i k h / H} / sqrt(H)
//                                  Y[k]    = softshrink(gelu(X[k] W1) W2)         real-ified: [Re | Im] . [[Wr, Wi], [-Wi, Wr]]
//                                  G[w, l] = sum_k  T3[w, k] Y[k]                          T3 = c_k e^{+2 pi i k w / W} / sqrt(W)
//   launch 3 (b, w, 64 channels)  out[h, w] = Re sum_l T4[h, l] G[w, l] + residual[h, w]   T4 = e^{+2 pi i l h / H} / sqrt(H)
//
// Launch 1 is dft_r2c_rows_kernel and launch 3 dft_c2r_rows_kernel<AfnoInvEpilogue> of dft_rows.hip.h, which also holds the table layout and
// the table product; launch 2, afno_mix_kernel, is this file's.
//
// c_k = 1 for k = 0 and for k = W/2 (W even), 2 otherwise: the complex-to-real weights.  The imaginary parts of those two entries drop
// out by themselves, their table entries being real.
//
// Every product is v_mfma_f32_16x16x4_f32: exact fp32 products and fp32 accumulation in BOTH compute modes, as the reference keeps the
// filter in fp32 under autocast.  A operand lane (i = l & 15, k = l >> 4), B operand lane (k = l >> 4, j = l & 15), result register r =
// row 4 (l >> 4) + r, column l & 15.  LDS is plain C++ between barriers: no hand-placed waits.  No hipFFT on this path.
#include "afno_filter.hip.h"

namespace {

__device__ __forceinline__ float softshrink(float v, float lam) { return v > lam ? v - lam : (v < -lam ? v + lam : 0.0f); }

// ---- launch 2: transform along h, block MLP, soft threshold, inverse along k ---------------------------------------------------------
__global__ __launch_bounds__(AF_THREADS) void afno_mix_kernel(const float* __restrict__ P, const float* __restrict__ T2r, const float* __restrict__ T2i,
                                                              int ldt2, const float* __restrict__ T3r, const float* __restrict__ T3i, int ldt3,
                                                              const float* __restrict__ w1, const float* __restrict__ w2, float lam,
                                                              float* __restrict__ G, int H, int W, int C, int bs, int Lc, int Kc) {
  __shared__ float bufA[AF_ROWS_A * AF_LD];
  __shared__ float bufB[AF_ROWS_B * AF_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const int l = blockIdx.x, g = blockIdx.y;
  const long b = blockIdx.z;
  const int bsP = (bs + 15) & ~15, n2 = 2 * bsP, ld = n2 + 4;
  const int Hp = (H + 3) & ~3, Kc16 = (Kc + 15) & ~15, Kc4 = (Kc + 3) & ~3;
  // P[b][l][h][re | im][C] -> bufA[h][re block | im block]
  const float* Pl = P + ((b * Lc + l) * H) * 2 * (long)C + (long)g * bs;
  for (int idx = tid; idx < Hp * n2; idx += AF_THREADS) {
    const int h = idx / n2, j = idx % n2, ri = j / bsP, c = j % bsP;
    bufA[h * ld + j] = (h < H && c < bs) ? Pl[((long)h * 2 + ri) * C + c] : 0.0f;
  }
  __syncthreads();
  const int MT = Kc16 >> 4, NTc = bsP >> 4, NT2 = n2 >> 4;
  // X[k] = sum_h T2[k, h] P[h]  -> bufB[k][re | im]   (rows Kc..Kc16 are zero: the table's padding)
  for (int t = wave; t < MT * NTc; t += AF_THREADS / 64) {
    const int mt = t / NTc, nt = t % NTc;
    f32x4 dr = {0.f, 0.f, 0.f, 0.f}, di = {0.f, 0.f, 0.f, 0.f};
    table_tile<true, true>(T2r, T2i, ldt2, mt * 16, bufA, ld, nt * 16, bsP, Hp, dr, di);
    for (int r = 0; r < 4; ++r) {
      float* p = bufB + (mt * 16 + 4 * kk + r) * ld + nt * 16 + i;
      p[0] = dr[r];
      p[bsP] = di[r];
    }
  }
  __syncthreads();
  // the two real-ified layers: rows k, K = N = 2 bsP; A from LDS, B = this block's (2 bsP, 2 bsP) matrix from memory
  for (int layer = 0; layer < 2; ++layer) {
    const float* src = layer == 0 ? bufB : bufA;
    float* dst = layer == 0 ? bufA : bufB;
    const float* wm = (layer == 0 ? w1 : w2) + (long)g * n2 * n2;
    for (int nt = wave; nt < NT2; nt += AF_THREADS / 64) {      // a wave owns a 16-column strip: one weight fragment feeds every row tile
      f32x4 d[AF_ROWS_B / 16];
      for (int mt = 0; mt < AF_ROWS_B / 16; ++mt) d[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* a = src + i * ld + kk;
      const float* bw = wm + (long)kk * n2 + nt * 16 + i;
      for (int k = 0; k < n2; k += 4) {
        const float bv = bw[(long)k * n2];
#pragma unroll
        for (int mt = 0; mt < AF_ROWS_B / 16; ++mt)
          if (mt < MT) d[mt] = mfma4(a[mt * 16 * ld + k], bv, d[mt]);
      }
#pragma unroll
      for (int mt = 0; mt < AF_ROWS_B / 16; ++mt)
        if (mt < MT)
          for (int r = 0; r < 4; ++r) dst[(mt * 16 + 4 * kk + r) * ld + nt * 16 + i] = layer == 0 ? gelu_erf_f(d[mt][r]) : softshrink(d[mt][r], lam);
    }
    __syncthreads();
  }
  // G[w, l] = sum_k T3[w, k] Y[k]
  const int MTw = (W + 15) >> 4;
  for (int t = wave; t < MTw * NTc; t += AF_THREADS / 64) {
    const int mt = t / NTc, nt = t % NTc;
    f32x4 dr = {0.f, 0.f, 0.f, 0.f}, di = {0.f, 0.f, 0.f, 0.f};
    table_tile<true, true>(T3r, T3i, ldt3, mt * 16, bufB, ld, nt * 16, bsP, Kc4, dr, di);
    const int c = nt * 16 + i;
    for (int r = 0; r < 4; ++r) {
      const int w = mt * 16 + 4 * kk + r;
      if (w < W && c < bs) {
        float* p = G + (((b * W + w) * Lc + l) * 2) * (long)C + (long)g * bs + c;
        p[0] = dr[r];
        p[C] = di[r];
      }
    }
  }
}

// ---- launch 3's store: + residual, and + 0.0f without one (which is not the bare value where that is -0) --------------------------------
struct AfnoInvEpilogue {
  const float* resid;
  __device__ float operator()(float v, long o) const { return v + (resid ? resid[o] : 0.0f); }
};

}  // namespace

extern "C" int tante_afno_filter_supported(int64_t B, int H, int W, int C, int bs) { return af_reason(B, H, W, C, bs) == nullptr ? 1 : 0; }

extern "C" int64_t tante_afno_twiddle_floats(int H, int W) {
  if (H < 1 || W < 1 || H > AF_MAX || W > AF_MAX) return -1;
  return af_tables(H, W).total;
}

extern "C" int64_t tante_afno_filter_workspace_bytes(int64_t B, int H, int W, int C) {
  if (B < 0 || H < 1 || W < 1 || H > AF_MAX || W > AF_MAX || C < 1) return -1;
  const AfTables t = af_tables(H, W);
  return (int64_t)sizeof(float) * 2 * B * t.Lc * ((int64_t)H + W) * C;       // P (B, Lc, H, 2, C) then G (B, W, Lc, 2, C)
}

extern "C" int tante_afno_filter(const float* x, const float* residual, int64_t B, int H, int W, int C, int bs, const float* twiddles,
                                 const float* w1, const float* w2, float lambda, float* out, void* work, int64_t work_bytes, void* stream) {
  if (const char* why = af_reason(B, H, W, C, bs)) TANTE_FAIL(-2, "tante_afno_filter: %s (B %lld, grid %d x %d, C %d, block %d)", why, (long long)B, H, W, C, bs);
  if (!x || !twiddles || !w1 || !w2 || !out) TANTE_FAIL(-1, "tante_afno_filter: null argument");
  if (x == out) TANTE_FAIL(-1, "tante_afno_filter: out may alias residual, not x");
  if (B == 0) return 0;
  const int64_t need = tante_afno_filter_workspace_bytes(B, H, W, C);
  if (!work || work_bytes < need) TANTE_FAIL(-1, "tante_afno_filter: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  const AfTables t = af_tables(H, W);
  float* P = (float*)work;
  float* G = P + 2 * B * t.Lc * (int64_t)H * C;
  hipStream_t s = (hipStream_t)stream;
  const unsigned cch = (unsigned)((C + DFT_CH - 1) / DFT_CH);
  const long C1 = C, C2 = 2l * C;
  const DftRows fwd_w = {H * W * C1, W * C1, C1, t.Lc * H * C2, C2, H * C2, H};       // x rows (b, h) -> P[b][l][h]
  const DftRows inv_h = {W * t.Lc * C2, t.Lc * C2, C2, H * W * C1, C1, W * C1, W};    // G[b][w] -> the columns (b, w) of out
  hipLaunchKernelGGL(dft_r2c_rows_kernel, dim3((unsigned)(B * H), cch), dim3(DFT_THREADS), 0, s, x, twiddles + t.re[0], twiddles + t.im[0], t.Kp[0], P,
                     fwd_w, W, t.Lc, C);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(afno_mix_kernel, dim3((unsigned)t.Lc, (unsigned)(C / bs), (unsigned)B), dim3(AF_THREADS), 0, s, (const float*)P, twiddles + t.re[1],
                     twiddles + t.im[1], t.Kp[1], twiddles + t.re[2], twiddles + t.im[2], t.Kp[2], w1, w2, lambda, G, H, W, C, bs, t.Lc, t.Kc);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dft_c2r_rows_kernel<AfnoInvEpilogue>, dim3((unsigned)(B * W), cch), dim3(DFT_THREADS), 0, s, (const float*)G, twiddles + t.re[3],
                     twiddles + t.im[3], t.Kp[3], out, inv_h, t.Lc, H, C, AfnoInvEpilogue{residual});
  TANTE_CHECK_LAUNCH();
  return 0;
}
