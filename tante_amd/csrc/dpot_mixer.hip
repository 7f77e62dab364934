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
// dft_rows.hip.h, which also holds the table layout and the table product; launches 2 .. 5 are this file's.
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
