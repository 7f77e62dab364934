// What the forward (dpot_mixer.hip) and the backward (dpot_mixer_bwd.hip) of DPOT's GroupNorm and truncated-mode mixer share beyond
// dft_rows.hip.h: the slab plan and statistics kernel of GroupNorm, the mixer's tables, workspace plan and shape predicates, and the
// kernels of launches 2 .. 5, which the backward runs again -- to recompute X and U with the forward's own statements, and against the
// adjoint tables.  The layouts and the lane maps are described at the head of dpot_mixer.hip.
#pragma once
#include "dft_rows.hip.h"

namespace {

constexpr int DP_MAX = DFT_MAX;            // grid points per axis
constexpr int DP_MAX_BS = 512;             // channels per block
constexpr int DP_THREADS = DFT_THREADS;    // four waves
constexpr int DP_MT = 12;                  // row tiles per workgroup of the MLP launches: 192 rows
constexpr int GN_MAX_HW = 4096;
constexpr int GN_SLABS = 64;               // slabs per group at most
constexpr int GN_SLAB_ELEMS = 4096;        // elements a slab aims for

// ================================================================ GroupNorm =============================================================
struct GnPlan {
  int cg, R, S;      // channels per group, rows per slab, slabs
};

GnPlan gn_plan(int HW, int C, int G) {
  GnPlan p;
  p.cg = C / G;
  int R = (GN_SLAB_ELEMS + p.cg - 1) / p.cg;
  const int Rmin = (HW + GN_SLABS - 1) / GN_SLABS;
  if (R < Rmin) R = Rmin;
  if (R > HW) R = HW;
  p.R = R;
  p.S = (HW + R - 1) / R;
  return p;
}

const char* gn_reason(int64_t B, int HW, int C, int G) {
  if (HW < 1 || HW > GN_MAX_HW) return "tokens per sample outside 1..4096";
  if (G < 1 || C < 1 || C % G) return "channels are not a whole number of groups";
  if (C > (1 << 24)) return "more than 2^24 channels";
  if (B < 0 || B * (int64_t)G > 2147483647ll) return "more than 2^31 - 1 (sample, group) pairs per call";
  return nullptr;
}

// the sum of v over the 256 threads, the same value in every thread: lanes by shuffle, then the four waves in order
__device__ __forceinline__ float gn_block_sum(float v, float* s) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s[0] + s[1]) + (s[2] + s[3]);
}

__global__ __launch_bounds__(DP_THREADS) void gn_stats_kernel(const float* __restrict__ x, float* __restrict__ part, int HW, int C, int G, int cg,
                                                              int R, int S) {
  __shared__ float red[4];
  const long bg = blockIdx.x;
  const int s = blockIdx.y;
  const long b = bg / G;
  const int g = (int)(bg % G);
  const int r0 = s * R;
  const int nr = (HW - r0) < R ? (HW - r0) : R;
  const int n = nr * cg;
  const float* base = x + (b * HW + r0) * (long)C + (long)g * cg;
  float a = 0.0f;
  for (int idx = threadIdx.x; idx < n; idx += DP_THREADS) a += base[(long)(idx / cg) * C + idx % cg];
  const float mean = gn_block_sum(a, red) / (float)n;
  float q = 0.0f;
  for (int idx = threadIdx.x; idx < n; idx += DP_THREADS) {
    const float d = base[(long)(idx / cg) * C + idx % cg] - mean;
    q += d * d;
  }
  const float m2 = gn_block_sum(q, red);
  if (threadIdx.x == 0) {
    part[(bg * S + s) * 2] = mean;
    part[(bg * S + s) * 2 + 1] = m2;
  }
}

template <bool BF16_OUT>
__global__ __launch_bounds__(DP_THREADS) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ part, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, void* __restrict__ y, int HW, int C, int G, int cg, int R,
                                                              int S, float eps) {
  const long bg = blockIdx.x;
  const int s = blockIdx.y;
  const long b = bg / G;
  const int g = (int)(bg % G);
  // every thread combines the group's slabs in slab order (S <= 64 pairs, the same addresses in every lane)
  float cnt = 0.0f, mean = 0.0f, m2 = 0.0f;
  for (int i = 0; i < S; ++i) {
    const int nri = (HW - i * R) < R ? (HW - i * R) : R;
    const float ni = (float)(nri * cg);
    const float mi = part[(bg * S + i) * 2], qi = part[(bg * S + i) * 2 + 1];
    const float d = mi - mean, nn = cnt + ni;
    mean += d * (ni / nn);
    m2 += qi + d * d * (cnt * (ni / nn));
    cnt = nn;
  }
  const float rstd = 1.0f / sqrtf(m2 / cnt + eps);
  const int r0 = s * R;
  const int nr = (HW - r0) < R ? (HW - r0) : R;
  const int n = nr * cg;
  const long off = (b * HW + r0) * (long)C + (long)g * cg;
  for (int idx = threadIdx.x; idx < n; idx += DP_THREADS) {
    const int c = idx % cg;
    const long o = off + (long)(idx / cg) * C + c;
    float v = (x[o] - mean) * rstd;
    if (gamma) v *= gamma[g * cg + c];
    if (beta) v += beta[g * cg + c];
    if (BF16_OUT)
      ((__bf16*)y)[o] = (__bf16)v;
    else
      ((float*)y)[o] = v;
  }
}

// ================================================================ the mixer ==============================================================
struct DpTables : DftTables {
  int k1, k2;
};

// T1 (k2, W), T2 (k1, H), T3 (H, k1), T4 (W, k2)
DpTables dp_tables(int H, int W, int modes) {
  const int k1 = modes < H ? modes : H, k2 = modes < (W / 2 + 1) ? modes : (W / 2 + 1);
  const int M[4] = {k2, k1, H, W}, K[4] = {W, H, k1, k2};
  return DpTables{dft_tables(M, K), k1, k2};
}

// ---- launch 2: the truncated forward transform along h, into the MLP's (g, row, [re | im], bsP) layout ------------------------------------
// a workgroup owns 64 PADDED channels pc = g bsP + q; q >= bs is the zero padding, which it writes
__global__ __launch_bounds__(DP_THREADS) void dpot_fwd_h_kernel(const float* __restrict__ P, const float* __restrict__ Tr, const float* __restrict__ Ti,
                                                                int ldt, float* __restrict__ X, int H, int C, int bs, int bsP, int nb, int k1, int k2,
                                                                long Mtot) {
  __shared__ float ps[DP_MAX * DFT_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const int l = blockIdx.x;
  const int pc0 = blockIdx.y * DFT_CH;
  const long b = blockIdx.z;
  const int npc = (nb * bsP - pc0) < DFT_CH ? (nb * bsP - pc0) : DFT_CH;       // a multiple of 16
  const int Hp = (H + 3) & ~3;
  const float* Pl = P + ((b * k2 + l) * H) * 2 * (long)C;
  for (int idx = tid; idx < Hp * 2 * DFT_CH; idx += DP_THREADS) {
    const int h = idx / (2 * DFT_CH), j = idx % (2 * DFT_CH), ri = j / DFT_CH, pc = pc0 + j % DFT_CH;
    const int g = pc / bsP, q = pc % bsP;
    ps[h * DFT_LD + j] = (h < H && g < nb && q < bs) ? Pl[((long)h * 2 + ri) * C + g * bs + q] : 0.0f;
  }
  __syncthreads();
  const int MT = (k1 + 15) >> 4, NT = npc >> 4;
  for (int t = wave; t < MT * NT; t += DP_THREADS / 64) {
    const int mt = t / NT, nt = t % NT;
    f32x4 dr = {0.f, 0.f, 0.f, 0.f}, di = {0.f, 0.f, 0.f, 0.f};
    table_tile<true, true>(Tr, Ti, ldt, mt * 16, ps, DFT_LD, nt * 16, DFT_CH, Hp, dr, di);
    const int pc = pc0 + nt * 16 + i, g = pc / bsP, q = pc % bsP;
    for (int r = 0; r < 4; ++r) {
      const int k = mt * 16 + 4 * kk + r;
      if (k < k1) {
        const long m = (b * k1 + k) * k2 + l;
        float* p = X + ((g * Mtot + m) * 2) * (long)bsP + q;
        p[0] = dr[r];
        p[bsP] = di[r];
      }
    }
  }
}

// ---- launches 3 and 4: one layer of the complex block MLP -----------------------------------------------------------------------------
// in / out (nb, Mtot, 2, bsP); w (2, nb, bs, bs) rows = input; bias (2, nb, bs).  K is walked 16 at a time: lane (i, kk) loads the four
// consecutive k = 16 s + 4 kk + j of its row with one 16-byte load and feeds them as steps j = 0..3, the weight lane (kk, i) loading the
// same four k -- a permutation of k inside the step that both operands share.
template <bool GELU>
__global__ __launch_bounds__(DP_THREADS) void dpot_mlp_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                              float* __restrict__ out, long Mtot, int nb, int bs, int bsP) {
  __shared__ f32x4 red[3 * 2 * 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const long m0 = (long)blockIdx.x * (16 * DP_MT);
  const int n0 = blockIdx.y * 16;
  const int g = blockIdx.z;
  const long left = Mtot - m0;
  const int MT = left >= 16 * DP_MT ? DP_MT : (int)((left + 15) >> 4);
  const float* A = in + ((long)g * Mtot) * 2 * bsP;
  const float* wr = w + ((long)g * bs) * bs;
  const float* wi = w + ((long)(nb + g) * bs) * bs;
  const int n = n0 + i;
  const bool nvalid = n < bs;
  f32x4 re[DP_MT], im[DP_MT];
#pragma unroll
  for (int mt = 0; mt < DP_MT; ++mt) re[mt] = im[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* arow[DP_MT];
#pragma unroll
  for (int mt = 0; mt < DP_MT; ++mt) {
    long row = m0 + mt * 16 + i;
    if (row > Mtot - 1) row = Mtot - 1;          // rows past the end repeat the last one; their results are not stored
    arow[mt] = A + row * 2 * bsP + 4 * kk;
  }
  for (int ks = wave; ks < (bsP >> 4); ks += DP_THREADS / 64) {
    const int kb = ks * 16 + 4 * kk;
    float br[4], bi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = nvalid && (kb + j) < bs;
      br[j] = ok ? wr[(long)(kb + j) * bs + n] : 0.0f;
      bi[j] = ok ? wi[(long)(kb + j) * bs + n] : 0.0f;
    }
#pragma unroll
    for (int mt = 0; mt < DP_MT; ++mt)
      if (mt < MT) {
        const f32x4 xr = *(const f32x4*)(arow[mt] + ks * 16);
        const f32x4 xi = *(const f32x4*)(arow[mt] + ks * 16 + bsP);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          re[mt] = mfma4(xr[j], br[j], re[mt]);
          im[mt] = mfma4(xi[j], br[j], im[mt]);
          re[mt] = mfma4(-xi[j], bi[j], re[mt]);
          im[mt] = mfma4(xr[j], bi[j], im[mt]);
        }
      }
  }
  const float b_re = nvalid ? bias[g * bs + n] : 0.0f;
  const float b_im = nvalid ? bias[(long)(nb + g) * bs + n] : 0.0f;
  float* O = out + ((long)g * Mtot) * 2 * bsP + n;
#pragma unroll
  for (int mt = 0; mt < DP_MT; ++mt)
    if (mt < MT) {           // MT is uniform over the workgroup: the barriers below are reached by all or by none
      if (wave > 0) {
        red[((wave - 1) * 2 + 0) * 64 + lane] = re[mt];
        red[((wave - 1) * 2 + 1) * 64 + lane] = im[mt];
      }
      __syncthreads();
      if (wave == 0) {
        f32x4 sr = re[mt], si = im[mt];
        for (int v = 0; v < 3; ++v) {
          sr += red[(v * 2 + 0) * 64 + lane];
          si += red[(v * 2 + 1) * 64 + lane];
        }
        for (int r = 0; r < 4; ++r) {
          const long row = m0 + mt * 16 + 4 * kk + r;
          if (row < Mtot) {
            float vr = sr[r] + b_re, vi = si[r] + b_im;
            if (GELU) vr = gelu_erf_f(vr), vi = gelu_erf_f(vi);
            O[row * 2 * bsP] = nvalid ? vr : 0.0f;
            O[row * 2 * bsP + bsP] = nvalid ? vi : 0.0f;
          }
        }
      }
      __syncthreads();
    }
}

// ---- launch 5: the H-point complex inverse over the k1 kept rows -------------------------------------------------------------------------
__global__ __launch_bounds__(DP_THREADS) void dpot_inv_h_kernel(const float* __restrict__ Y, const float* __restrict__ Tr, const float* __restrict__ Ti,
                                                                int ldt, float* __restrict__ Z, int H, int C, int bs, int bsP, int k1, int k2,
                                                                long Mtot) {
  __shared__ float ys[DP_MAX * DFT_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const int l = blockIdx.x;
  const int c0 = blockIdx.y * DFT_CH;
  const long b = blockIdx.z;
  const int nc = (C - c0) < DFT_CH ? (C - c0) : DFT_CH;
  const int Kp = (k1 + 3) & ~3;
  for (int idx = tid; idx < Kp * 2 * DFT_CH; idx += DP_THREADS) {
    const int k = idx / (2 * DFT_CH), j = idx % (2 * DFT_CH), ri = j / DFT_CH, c = j % DFT_CH;
    float v = 0.0f;
    if (k < k1 && c < nc) {
      const int g = (c0 + c) / bs, q = (c0 + c) % bs;
      const long m = (b * k1 + k) * k2 + l;
      v = Y[((g * Mtot + m) * 2 + ri) * (long)bsP + q];
    }
    ys[k * DFT_LD + j] = v;
  }
  __syncthreads();
  const int MT = (H + 15) >> 4, NT = (nc + 15) >> 4;
  for (int t = wave; t < MT * NT; t += DP_THREADS / 64) {
    const int mt = t / NT, nt = t % NT;
    f32x4 dr = {0.f, 0.f, 0.f, 0.f}, di = {0.f, 0.f, 0.f, 0.f};
    table_tile<true, true>(Tr, Ti, ldt, mt * 16, ys, DFT_LD, nt * 16, DFT_CH, Kp, dr, di);
    const int c = nt * 16 + i;
    for (int r = 0; r < 4; ++r) {
      const int h = mt * 16 + 4 * kk + r;
      if (h < H && c < nc) {
        float* p = Z + (((b * H + h) * k2 + l) * 2) * (long)C + c0 + c;
        p[0] = dr[r];
        p[C] = di[r];
      }
    }
  }
}

// ---- launch 6's store: the inner skip and the optional residual -------------------------------------------------------------------------
struct DpotInvEpilogue {
  const float* x;
  const float* resid;
  __device__ float operator()(float v, long o) const {
    const float f = v + x[o];                // the filter's own skip: its value without a residual
    return resid ? f + resid[o] : f;         // one more fp32 add of the finished value
  }
};

const char* dp_reason(int64_t B, int H, int W, int C, int bs, int modes, int hidden_factor) {
  if (H < 1 || W < 1 || H > DP_MAX || W > DP_MAX) return "token grid outside 1..64 points per axis";
  if (bs < 1 || bs > DP_MAX_BS) return "channel block size outside 1..512";
  if (C < 1 || C % bs) return "channels are not a whole number of blocks";
  if (C / bs > 65535) return "more than 65535 channel blocks";
  if (modes < 1) return "modes must be at least 1";
  if (hidden_factor != 1) return "hidden_size_factor other than 1";
  if (B < 0 || B > 65535) return "more than 65535 samples per call";
  return nullptr;
}

struct DpWork {          // float offsets into the workspace
  long Mtot, spat, blk, total;
};

DpWork dp_work(int64_t B, int H, int W, int C, int bs, int modes) {
  const DpTables t = dp_tables(H, W, modes);
  DpWork k;
  k.Mtot = (long)B * t.k1 * t.k2;
  k.spat = (2l * B * t.k2 * H * C + 3) & ~3l;                  // P (B, k2, H, 2, C), later Z (B, H, k2, 2, C)
  k.blk = (long)(C / bs) * k.Mtot * 2 * r16(bs);               // X then Y, and the hidden V: (nb, Mtot, 2, bsP) each
  k.total = k.spat + 2 * k.blk;
  return k;
}

}  // namespace
