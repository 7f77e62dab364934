// The two tile stages that tante_convnext_block, tante_dwconv_ln (convnext.hip) and tante_dwconv_ln_bwd (convnext_bwd.hip) share: the
// depthwise 7 x 7 of a tile through a staged halo, and LayerNorm over the true C per token row.  The backward RECOMPUTES the forward's
// pre-norm sums and statistics from x, so both sides must run the same code in the same order: it lives here once.
#pragma once
#include "common.hip.h"

namespace {

constexpr int CN_THREADS = 256;
constexpr int DL_MAXC = 1024;
constexpr int DL_TW = 8;                   // tante_dwconv_ln: 8 x 8 tokens up to C = 512, 4 x 8 beyond
constexpr int DL_CH = 32;

// ---- step 1: depthwise 7 x 7 + bias of a TH x TW tile (TW a multiple of 8) at (y0, x0) into rows[token * RS + c] ----------------------------
// taps[t * tap_s + c * ch_s], t = dy * 7 + dx.  halo: (TH + 6) (TW + 6) CH floats.  Ends with a barrier.
__device__ __forceinline__ void dw_stage(const float* __restrict__ ximg, int H, int W, int C, int y0, int x0, int TH, int TW,
                                         const float* __restrict__ taps, int tap_s, int ch_s, const float* __restrict__ bias, float* halo, int CH,
                                         float* rows, int RS) {
  const int tid = threadIdx.x;
  const int HH = TH + 6, HW = TW + 6;
  const int segs_x = TW / 8, segs = TH * segs_x;
  for (int c0 = 0; c0 < C; c0 += CH) {
    const int cn = (C - c0) < CH ? (C - c0) : CH;
    __syncthreads();                                            // the previous chunk's reads of the halo are done
    for (int i = tid; i < HH * HW * CH; i += CN_THREADS) {
      const int c = i % CH, p = i / CH;
      const int gy = y0 + p / HW - 3, gx = x0 + p % HW - 3;
      float v = 0.0f;
      if (c < cn && gy >= 0 && gy < H && gx >= 0 && gx < W) v = ximg[((long)gy * W + gx) * C + c0 + c];
      halo[i] = v;
    }
    __syncthreads();
    for (int u = tid; u < segs * CH; u += CN_THREADS) {
      const int c = u % CH, seg = u / CH;
      if (c >= cn) continue;
      const int ty = seg / segs_x, xs = (seg % segs_x) * 8;
      const float* tp = taps + (long)(c0 + c) * ch_s;
      float acc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
#pragma unroll
      for (int dy = 0; dy < 7; ++dy) {
        float r[14], w[7];
        const float* hp = halo + ((ty + dy) * HW + xs) * CH + c;
#pragma unroll
        for (int i = 0; i < 14; ++i) r[i] = hp[i * CH];
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) w[dx] = tp[(dy * 7 + dx) * tap_s];
#pragma unroll
        for (int dx = 0; dx < 7; ++dx)
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] = fmaf(r[i + dx], w[dx], acc[i]);
      }
      const float b = bias[c0 + c];
      float* rp = rows + (ty * TW + xs) * RS + c0 + c;
#pragma unroll
      for (int i = 0; i < 8; ++i) rp[i * RS] = acc[i] + b;
    }
  }
  __syncthreads();
}

// ---- step 2: LayerNorm of ntok token rows over the true C, in place; channels C .. KP - 1 become zero.  Ends with a barrier. ------------
// KEEP_RSTD (the backward): the token's 1 / sqrt(var + eps) is left in rstd_out[token] as well.
template <bool KEEP_RSTD = false>
__device__ __forceinline__ void ln_stage(float* rows, int RS, int ntok, int C, int KP, float eps, const float* __restrict__ gw,
                                         const float* __restrict__ gb, float* rstd_out = nullptr) {
  const int q = threadIdx.x & 3;
  for (int t0 = 0; t0 < ntok; t0 += CN_THREADS / 4) {
    const int t = t0 + (threadIdx.x >> 2);
    const bool on = t < ntok;
    float* r = rows + (on ? t : 0) * RS;
    float s = 0.0f;
    for (int c = q; c < C; c += 4) s += r[c];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    const float mean = s / (float)C;
    float v = 0.0f;
    for (int c = q; c < C; c += 4) {
      const float d = r[c] - mean;
      v = fmaf(d, d, v);
    }
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    const float rstd = 1.0f / sqrtf(v / (float)C + eps);
    if (on)
      for (int c = q; c < KP; c += 4) {
        float o = 0.0f;
        if (c < C) {
          o = (r[c] - mean) * rstd;
          if (gw) o = fmaf(o, gw[c], gb ? gb[c] : 0.0f);
        }
        r[c] = o;
      }
    if constexpr (KEEP_RSTD)
      if (on && q == 0) rstd_out[t] = rstd;
  }
  __syncthreads();
}

inline int dl_th(int C) { return C <= 512 ? 8 : 4; }
inline int dl_rs(int C) { return ((C + 3) / 4) * 4 + 4; }
inline int dl_lds(int C) { return 4 * (dl_th(C) * DL_TW * dl_rs(C) + (dl_th(C) + 6) * (DL_TW + 6) * DL_CH); }

inline const char* dl_reason(int64_t n_img, int H, int W, int C) {
  if (C < 1 || C > DL_MAXC) return "channels outside 1..1024";
  if (H < 1 || W < 1) return "an empty image";
  if (n_img < 0) return "a negative image count";
  const int64_t tiles = (int64_t)((W + DL_TW - 1) / DL_TW) * ((H + dl_th(C) - 1) / dl_th(C));
  if (tiles > 2147483647ll || n_img * tiles > 2147483647ll) return "more than 2^31 - 1 tiles per call";
  return nullptr;
}

}  // namespace
