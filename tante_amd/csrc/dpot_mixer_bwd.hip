// Backward of DPOT's two kernels (dpot_mixer.hip): what torch.autograd derives for torch.nn.GroupNorm (reference models/dpot.py:138, 147,
// 160, 167) and for AFNO2D.forward (dpot.py:47-102), on channels-last rows.  No atomics anywhere in this file: every sum has a fixed
// order, so two runs give the same bits.
//
// ---- tante_groupnorm_bwd: x (B, HW, C) fp32, dy fp32 or bf16 -> dx fp32, dgamma, dbeta ----------------------------------------------------
// With xh = (x - mean) rstd and n = HW C/G, per (sample, group)
//
//   dx = rstd (gamma dy - mean(gamma dy) - xh mean(gamma dy xh)),     dgamma_c = sum dy xh,   dbeta_c = sum dy   over samples and tokens.
//
//   launch 1  gn_stats_kernel of the forward: per slab the mean first, then the centred sum of squares about it
//   launch 2  (b g, slab)   the slabs' statistics combined pairwise in slab order (the forward's statements); per channel of the slab
//                           sum dy xh and sum dy (row subsets per thread, then the subsets in order through LDS), stored per (b, slab, c);
//                           the group's two sums from those, gamma-weighted: lanes by shuffle, waves in order
//   launch 3  (b g, slab)   the group's two sums over the slabs in slab order, then dx
//   launch 4  (C / 256)     dgamma_c, dbeta_c: the (b, slab) partials in order, (+)= under `accumulate`
//
// ---- tante_dpot_filter_bwd: dout (B, H, W, C) fp32 -> dx, dw1, db1, dw2, db2 ----------------------------------------------------------------
// The forward is a chain of real-linear maps on [re | im] rows and one pointwise function,
//
//   P = T1 x   X = T2 P   U = X W1 + b1   V = gelu(Re U) + i gelu(Im U)   Y = V W2 + b2   Z = T3 Y   out = Re(T4 Z) + x (+ residual),
//
// and the backward runs it in reverse against the conjugate-transposed tables (from the host, packed like the forward's):
//
//   R1 .. R3  x -> P -> X -> U         the forward's launches 1 .. 3 with their own statements (launch 3 without the GELU: U, not V; the
//                                      forward keeps neither X nor U, and the rows are few)
//   B1 (b, h, 64 channels)             dZ[h, l] = sum_w conj(T4[w, l]) dout[h, w]               dft_r2c_rows_kernel, real in, complex out
//   B2 (b, l, 64 padded channels)      dY[k, l] = sum_h conj(T3[h, k]) dZ[h, l]                 dpot_fwd_h_kernel: into the block layout
//   B3 (rows, 16 columns, g)           dU = (dY conj(W2)^T) gelu'(U), real and imaginary part each by its own derivative
//   B4 (16 x 64 weights, g), twice     dW2 = conj(V)^T dY, db2 = sum dY;   dW1 = conj(X)^T dU, db1 = sum dU      V = gelu(U) on load
//   B5 (rows, 16 columns, g)           dX = dU conj(W1)^T
//   B6 (b, l, 64 channels)             dP[h, l] = sum_k conj(T2[k, h]) dX[k, l]                 dpot_inv_h_kernel
//   B7 (b, h, 64 channels)             dx[h, w] = Re sum_l conj(T1[l, w]) dP[h, l] + dout[h, w] dft_c2r_rows_kernel<DpotBwdEpilogue>:
//                                                                                                the inner skip's gradient rides the store
//
// The residual's gradient is dout itself and is the caller's.  B3 / B5 are dpot_mlp_kernel's loop against the transposed, conjugated
// weight: their grid is cut by weight bytes like the forward's.  B4 has 2 nb bs^2 outputs and B k1 k2 rows: a wave owns one 16 x 16 tile
// of one channel block's gradient and walks ALL rows in row order, four per MFMA step, so the sum over rows has one fixed order and
// needs no partials; the bias sums ride the same loads (lanes hold rows r = kk (mod 4), joined in kk order).  Every product is
// v_mfma_f32_16x16x4_f32, as in the forward; the zero padding up to bsP is written by every launch that fills the block layout.
#include "dpot_mixer.hip.h"

namespace {

// ================================================================ GroupNorm =============================================================
// the group's (mean, rstd) from the slabs' (mean, M2): gn_apply_kernel's statements
__device__ __forceinline__ void gn_combine(const float* __restrict__ part, long bg, int HW, int cg, int R, int S, float eps, float& mean_o, float& rstd_o) {
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
  mean_o = mean;
  rstd_o = 1.0f / sqrtf(m2 / cnt + eps);
}

// cw: the channels a pass covers, a power of two <= 256; the 256 / cw thread rows split the slab's rows
template <typename T>
__global__ __launch_bounds__(DP_THREADS) void gn_bwd_sums_kernel(const T* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ part,
                                                                 const float* __restrict__ gamma, float* __restrict__ sums, float* __restrict__ chan,
                                                                 int HW, int C, int G, int cg, int R, int S, int cw, float eps) {
  __shared__ float red[4];
  __shared__ float cs[2 * DP_THREADS];
  const long bg = blockIdx.x;
  const int s = blockIdx.y;
  const long b = bg / G;
  const int g = (int)(bg % G);
  float mean, rstd;
  gn_combine(part, bg, HW, cg, R, S, eps, mean, rstd);
  const int r0 = s * R;
  const int nr = (HW - r0) < R ? (HW - r0) : R;
  const long off = (b * HW + r0) * (long)C + (long)g * cg;
  const int cl = threadIdx.x % cw, rsub = threadIdx.x / cw, nsub = DP_THREADS / cw;
  float a1 = 0.0f, a2 = 0.0f;
  for (int c0 = 0; c0 < cg; c0 += cw) {
    const int c = c0 + cl;
    float sg = 0.0f, sb = 0.0f;
    if (c < cg) {
      for (int r = rsub; r < nr; r += nsub) {
        const long o = off + (long)r * C + c;
        const float d = (float)dy[o];
        sb += d;
        sg += d * ((x[o] - mean) * rstd);
      }
      const float gm = gamma ? gamma[g * cg + c] : 1.0f;
      a1 += gm * sb;
      a2 += gm * sg;
    }
    if (chan) {        // uniform over the workgroup
      cs[rsub * cw + cl] = sg;
      cs[DP_THREADS + rsub * cw + cl] = sb;
      __syncthreads();
      if (rsub == 0 && c < cg) {
        float tg = 0.0f, tb = 0.0f;
        for (int q = 0; q < nsub; ++q) {
          tg += cs[q * cw + cl];
          tb += cs[DP_THREADS + q * cw + cl];
        }
        float* p = chan + ((b * S + s) * (long)C + (long)g * cg + c) * 2;
        p[0] = tg;
        p[1] = tb;
      }
      __syncthreads();
    }
  }
  const float s1 = gn_block_sum(a1, red);
  const float s2 = gn_block_sum(a2, red);
  if (threadIdx.x == 0) {
    sums[(bg * S + s) * 2] = s1;
    sums[(bg * S + s) * 2 + 1] = s2;
  }
}

template <typename T>
__global__ __launch_bounds__(DP_THREADS) void gn_bwd_apply_kernel(const T* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ part,
                                                                  const float* __restrict__ sums, const float* __restrict__ gamma,
                                                                  float* __restrict__ dx, int HW, int C, int G, int cg, int R, int S, float eps) {
  const long bg = blockIdx.x;
  const int s = blockIdx.y;
  const long b = bg / G;
  const int g = (int)(bg % G);
  float mean, rstd;
  gn_combine(part, bg, HW, cg, R, S, eps, mean, rstd);
  float s1 = 0.0f, s2 = 0.0f;
  for (int i = 0; i < S; ++i) {       // slab order, the same addresses in every lane
    s1 += sums[(bg * S + i) * 2];
    s2 += sums[(bg * S + i) * 2 + 1];
  }
  const float inv_n = 1.0f / ((float)HW * (float)cg);
  const float m1 = s1 * inv_n, m2 = s2 * inv_n;
  const int r0 = s * R;
  const int nr = (HW - r0) < R ? (HW - r0) : R;
  const int n = nr * cg;
  const long off = (b * HW + r0) * (long)C + (long)g * cg;
  for (int idx = threadIdx.x; idx < n; idx += DP_THREADS) {
    const int c = idx % cg;
    const long o = off + (long)(idx / cg) * C + c;
    float d = (float)dy[o];
    if (gamma) d *= gamma[g * cg + c];
    const float xh = (x[o] - mean) * rstd;
    dx[o] = rstd * (d - m1 - xh * m2);
  }
}

__global__ __launch_bounds__(256) void gn_bwd_param_kernel(const float* __restrict__ chan, long n_part, int C, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int accumulate) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float tg = 0.0f, tb = 0.0f;
  for (long p = 0; p < n_part; ++p) {      // (sample, slab) order
    tg += chan[(p * C + c) * 2];
    tb += chan[(p * C + c) * 2 + 1];
  }
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + tg : tg;
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + tb : tb;
}

struct GnBwdWork {       // float offsets into the workspace
  long sums, chan, total;
};

GnBwdWork gn_bwd_work(int64_t B, int HW, int C, int G) {
  const long S = gn_plan(HW, C, G).S;
  GnBwdWork k;
  k.sums = 2 * B * G * S;               // behind the forward's statistics
  k.chan = 2 * k.sums;
  k.total = k.chan + 2 * B * S * C;
  return k;
}

template <typename T>
void gn_bwd_launch(const void* dy, const float* x, const float* gamma, float* dx, float* dgamma, float* dbeta, int accumulate, float* work, int64_t B,
                   int HW, int C, int G, float eps, hipStream_t s) {
  const GnPlan p = gn_plan(HW, C, G);
  const GnBwdWork k = gn_bwd_work(B, HW, C, G);
  const bool params = dgamma || dbeta;
  int cw = 1;
  while (cw < p.cg && cw < DP_THREADS) cw <<= 1;
  const dim3 grid((unsigned)(B * G), (unsigned)p.S);
  hipLaunchKernelGGL(gn_stats_kernel, grid, dim3(DP_THREADS), 0, s, x, work, HW, C, G, p.cg, p.R, p.S);
  hipLaunchKernelGGL(gn_bwd_sums_kernel<T>, grid, dim3(DP_THREADS), 0, s, (const T*)dy, x, (const float*)work, gamma, work + k.sums,
                     params ? work + k.chan : nullptr, HW, C, G, p.cg, p.R, p.S, cw, eps);
  hipLaunchKernelGGL(gn_bwd_apply_kernel<T>, grid, dim3(DP_THREADS), 0, s, (const T*)dy, x, (const float*)work, (const float*)(work + k.sums), gamma, dx,
                     HW, C, G, p.cg, p.R, p.S, eps);
  if (params)
    hipLaunchKernelGGL(gn_bwd_param_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const float*)(work + k.chan), (long)(B * p.S), C, dgamma,
                       dbeta, accumulate);
}

// ================================================================ the mixer ==============================================================
// the conjugate transposes, in the forward's order: T1^H (W, k2), T2^H (H, k1), T3^H (k1, H), T4^H (k2, W)
DpTables dp_tables_adj(int H, int W, int modes) {
  const int k1 = modes < H ? modes : H, k2 = modes < (W / 2 + 1) ? modes : (W / 2 + 1);
  const int M[4] = {W, H, k1, k2}, K[4] = {k2, k1, H, W};
  return DpTables{dft_tables(M, K), k1, k2};
}

// ---- B3 and B5: out = in conj(W)^T (gelu'(U) on the real and the imaginary part): dpot_mlp_kernel's loop, the weight lane (kk, i) reading
// w[n0 + i][k] where the forward reads w[k][n0 + i], its imaginary part negated ------------------------------------------------------------
template <bool DGELU>
__global__ __launch_bounds__(DP_THREADS) void dpot_mlp_bwd_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ U,
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
      br[j] = ok ? wr[(long)n * bs + kb + j] : 0.0f;
      bi[j] = ok ? -wi[(long)n * bs + kb + j] : 0.0f;
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
  const long base = ((long)g * Mtot) * 2 * bsP + n;
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
            const long o = base + row * 2 * bsP;
            float vr = sr[r], vi = si[r];
            if (DGELU && nvalid) {
              vr *= act_df(U[o], TANTE_ACT_GELU_ERF);
              vi *= act_df(U[o + bsP], TANTE_ACT_GELU_ERF);
            }
            out[o] = nvalid ? vr : 0.0f;
            out[o + bsP] = nvalid ? vi : 0.0f;
          }
        }
      }
      __syncthreads();
    }
}

// ---- B4: dW = conj(A)^T D over all rows, db = sum of D's rows; A, D (nb, Mtot, 2, bsP); dw (2, nb, bs, bs), db (2, nb, bs) ------------------
// grid (bsP / 16 weight rows, ceil(bsP / 64) groups of four 16-column tiles, nb): a wave owns one 16 x 16 tile.  No barrier in this kernel.
template <bool GELU_A>
__global__ __launch_bounds__(DP_THREADS) void dpot_wgrad_kernel(const float* __restrict__ A, const float* __restrict__ D, float* __restrict__ dw,
                                                                float* __restrict__ db, long Mtot, int nb, int bs, int bsP, int accumulate) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const int it = blockIdx.x, nt = blockIdx.y * (DP_THREADS / 64) + wave, g = blockIdx.z;
  if (nt >= (bsP >> 4)) return;
  const float* a = A + ((long)g * Mtot) * 2 * bsP + it * 16 + i;
  const float* d = D + ((long)g * Mtot) * 2 * bsP + nt * 16 + i;
  f32x4 wr = {0.f, 0.f, 0.f, 0.f}, wi = {0.f, 0.f, 0.f, 0.f};
  float sr = 0.0f, si = 0.0f;
  for (long m = 0; m < Mtot; m += 4) {
    const long row = m + kk;
    float ar = 0.0f, ai = 0.0f, br = 0.0f, bi = 0.0f;
    if (row < Mtot) {
      ar = a[row * 2 * bsP];
      ai = a[row * 2 * bsP + bsP];
      br = d[row * 2 * bsP];
      bi = d[row * 2 * bsP + bsP];
      if (GELU_A) ar = gelu_erf_f(ar), ai = gelu_erf_f(ai);      // V as the forward's launch 3 rounds it
    }
    wr = mfma4(ar, br, wr);
    wi = mfma4(ar, bi, wi);
    wr = mfma4(ai, bi, wr);
    wi = mfma4(-ai, br, wi);
    sr += br;
    si += bi;
  }
  const int col = nt * 16 + i;
  const long plane = (long)nb * bs * bs;
  for (int r = 0; r < 4; ++r) {
    const int row = it * 16 + 4 * kk + r;
    if (row < bs && col < bs) {
      float* p = dw + ((long)g * bs + row) * bs + col;
      p[0] = accumulate ? p[0] + wr[r] : wr[r];
      p[plane] = accumulate ? p[plane] + wi[r] : wi[r];
    }
  }
  if (it == 0) {       // uniform over the workgroup; the four row classes in kk order
    const float tr = ((__shfl(sr, i, 64) + __shfl(sr, 16 + i, 64)) + __shfl(sr, 32 + i, 64)) + __shfl(sr, 48 + i, 64);
    const float ti = ((__shfl(si, i, 64) + __shfl(si, 16 + i, 64)) + __shfl(si, 32 + i, 64)) + __shfl(si, 48 + i, 64);
    if (kk == 0 && col < bs) {
      float* p = db + (long)g * bs + col;
      const long bplane = (long)nb * bs;
      p[0] = accumulate ? p[0] + tr : tr;
      p[bplane] = accumulate ? p[bplane] + ti : ti;
    }
  }
}

// ---- B7's store: the gradient of the filter's own skip -------------------------------------------------------------------------------------
struct DpotBwdEpilogue {
  const float* dout;
  __device__ float operator()(float v, long o) const { return v + dout[o]; }
};

struct DpBwdWork {       // float offsets into the workspace
  long Mtot, spat, blk, total;
};

DpBwdWork dp_bwd_work(int64_t B, int H, int W, int C, int bs, int modes) {
  const DpWork f = dp_work(B, H, W, C, bs, modes);
  return DpBwdWork{f.Mtot, f.spat, f.blk, f.spat + 4 * f.blk};      // P / dZ / dP, then X, U, dY / dX, dU
}

}  // namespace

extern "C" int tante_groupnorm_bwd_supported(int64_t B, int HW, int C, int G) { return gn_reason(B, HW, C, G) == nullptr ? 1 : 0; }

extern "C" int64_t tante_groupnorm_bwd_workspace_bytes(int64_t B, int HW, int C, int G) {
  if (gn_reason(B, HW, C, G)) return -1;
  return (int64_t)sizeof(float) * gn_bwd_work(B, HW, C, G).total;
}

extern "C" int tante_groupnorm_bwd(const void* dy, int dy_dtype, const float* x, int64_t B, int HW, int C, int G, float eps, const float* gamma, float* dx,
                                   float* dgamma, float* dbeta, int accumulate, void* work, int64_t work_bytes, void* stream) {
  if (const char* why = gn_reason(B, HW, C, G))
    TANTE_FAIL(-2, "tante_groupnorm_bwd: %s (B %lld, tokens %d, C %d, groups %d)", why, (long long)B, HW, C, G);
  if (dy_dtype != TANTE_F32 && dy_dtype != TANTE_BF16) TANTE_FAIL(-1, "tante_groupnorm_bwd: dy must be fp32 or bf16");
  if (!dy || !x || !dx) TANTE_FAIL(-1, "tante_groupnorm_bwd: null argument");
  if ((const void*)dx == dy || dx == x) TANTE_FAIL(-1, "tante_groupnorm_bwd: dx may alias neither dy nor x");
  const int64_t need = tante_groupnorm_bwd_workspace_bytes(B, HW, C, G);
  if (B > 0 && (!work || work_bytes < need))
    TANTE_FAIL(-1, "tante_groupnorm_bwd: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {          // no rows: the parameter gradients are zero
    if (dgamma || dbeta) {
      hipLaunchKernelGGL(gn_bwd_param_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const float*)nullptr, 0l, C, dgamma, dbeta, accumulate);
      TANTE_CHECK_LAUNCH();
    }
    return 0;
  }
  if (dy_dtype == TANTE_BF16)
    gn_bwd_launch<__bf16>(dy, x, gamma, dx, dgamma, dbeta, accumulate, (float*)work, B, HW, C, G, eps, s);
  else
    gn_bwd_launch<float>(dy, x, gamma, dx, dgamma, dbeta, accumulate, (float*)work, B, HW, C, G, eps, s);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t tante_dpot_twiddle_bwd_floats(int H, int W, int modes) {
  if (H < 1 || W < 1 || H > DP_MAX || W > DP_MAX || modes < 1) return -1;
  return dp_tables_adj(H, W, modes).total;
}

extern "C" int64_t tante_dpot_filter_bwd_workspace_bytes(int64_t B, int H, int W, int C, int bs, int modes) {
  if (dp_reason(B, H, W, C, bs, modes, 1)) return -1;
  return (int64_t)sizeof(float) * dp_bwd_work(B, H, W, C, bs, modes).total;
}

extern "C" int tante_dpot_filter_bwd(const float* dout, const float* x, int64_t B, int H, int W, int C, int bs, int modes, const float* twiddles,
                                     const float* twiddles_bwd, const float* w1, const float* b1, const float* w2, float* dx, float* dw1, float* db1,
                                     float* dw2, float* db2, int accumulate, void* work, int64_t work_bytes, void* stream) {
  if (const char* why = dp_reason(B, H, W, C, bs, modes, 1))
    TANTE_FAIL(-2, "tante_dpot_filter_bwd: %s (B %lld, grid %d x %d, C %d, block %d, modes %d)", why, (long long)B, H, W, C, bs, modes);
  if (!dout || !x || !twiddles || !twiddles_bwd || !w1 || !b1 || !w2 || !dx || !dw1 || !db1 || !dw2 || !db2)
    TANTE_FAIL(-1, "tante_dpot_filter_bwd: null argument");
  if (dx == dout || dx == x) TANTE_FAIL(-1, "tante_dpot_filter_bwd: dx may alias neither dout nor x");
  const DpBwdWork k = dp_bwd_work(B, H, W, C, bs, modes);
  const int64_t need = (int64_t)sizeof(float) * k.total;
  if (B > 0 && (!work || work_bytes < need))
    TANTE_FAIL(-1, "tante_dpot_filter_bwd: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  if (B > 0 && (uintptr_t)work % 16) TANTE_FAIL(-1, "tante_dpot_filter_bwd: the workspace must be 16-byte aligned");
  const DpTables t = dp_tables(H, W, modes), a = dp_tables_adj(H, W, modes);
  const int nb = C / bs, bsP = r16(bs);
  float* P = (float*)work;          // then dZ, then dP
  float* X = P + k.spat;
  float* U = X + k.blk;
  float* D1 = U + k.blk;            // dY, then dX
  float* D2 = D1 + k.blk;           // dU
  hipStream_t s = (hipStream_t)stream;
  const unsigned cch = (unsigned)((C + DFT_CH - 1) / DFT_CH), pch = (unsigned)((nb * bsP + DFT_CH - 1) / DFT_CH);
  const dim3 mlp_grid((unsigned)((k.Mtot + 16 * DP_MT - 1) / (16 * DP_MT)), (unsigned)(bsP / 16), (unsigned)nb);
  const dim3 wg_grid((unsigned)(bsP / 16), (unsigned)((bsP / 16 + DP_THREADS / 64 - 1) / (DP_THREADS / 64)), (unsigned)nb);
  const long C1 = C, C2 = 2l * C;
  const DftRows rows_lh = {H * W * C1, W * C1, C1, t.k2 * H * C2, C2, H * C2, H};     // real rows (b, h) -> [b][l][h]: x -> P, dout -> dZ
  const DftRows rows_hl = {H * t.k2 * C2, t.k2 * C2, C2, H * W * C1, W * C1, C1, H};  // dP[b][h] -> dx rows (b, h)
  if (B > 0) {
    hipLaunchKernelGGL(dft_r2c_rows_kernel, dim3((unsigned)(B * H), cch), dim3(DFT_THREADS), 0, s, x, twiddles + t.re[0], twiddles + t.im[0], t.Kp[0], P,
                       rows_lh, W, t.k2, C);
    TANTE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dpot_fwd_h_kernel, dim3((unsigned)t.k2, pch, (unsigned)B), dim3(DP_THREADS), 0, s, (const float*)P, twiddles + t.re[1],
                       twiddles + t.im[1], t.Kp[1], X, H, C, bs, bsP, nb, t.k1, t.k2, k.Mtot);
    TANTE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dpot_mlp_kernel<false>, mlp_grid, dim3(DP_THREADS), 0, s, (const float*)X, w1, b1, U, k.Mtot, nb, bs, bsP);
    TANTE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dft_r2c_rows_kernel, dim3((unsigned)(B * H), cch), dim3(DFT_THREADS), 0, s, dout, twiddles_bwd + a.re[3], twiddles_bwd + a.im[3],
                       a.Kp[3], P, rows_lh, W, t.k2, C);
    TANTE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dpot_fwd_h_kernel, dim3((unsigned)t.k2, pch, (unsigned)B), dim3(DP_THREADS), 0, s, (const float*)P, twiddles_bwd + a.re[2],
                       twiddles_bwd + a.im[2], a.Kp[2], D1, H, C, bs, bsP, nb, t.k1, t.k2, k.Mtot);
    TANTE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dpot_mlp_bwd_kernel<true>, mlp_grid, dim3(DP_THREADS), 0, s, (const float*)D1, w2, (const float*)U, D2, k.Mtot, nb, bs, bsP);
    TANTE_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(dpot_wgrad_kernel<true>, wg_grid, dim3(DP_THREADS), 0, s, (const float*)U, (const float*)D1, dw2, db2, k.Mtot, nb, bs, bsP, accumulate);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dpot_wgrad_kernel<false>, wg_grid, dim3(DP_THREADS), 0, s, (const float*)X, (const float*)D2, dw1, db1, k.Mtot, nb, bs, bsP, accumulate);
  TANTE_CHECK_LAUNCH();
  if (B > 0) {
    hipLaunchKernelGGL(dpot_mlp_bwd_kernel<false>, mlp_grid, dim3(DP_THREADS), 0, s, (const float*)D2, w1, (const float*)nullptr, D1, k.Mtot, nb, bs, bsP);
    TANTE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dpot_inv_h_kernel, dim3((unsigned)t.k2, cch, (unsigned)B), dim3(DP_THREADS), 0, s, (const float*)D1, twiddles_bwd + a.re[1],
                       twiddles_bwd + a.im[1], a.Kp[1], P, H, C, bs, bsP, t.k1, t.k2, k.Mtot);
    TANTE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dft_c2r_rows_kernel<DpotBwdEpilogue>, dim3((unsigned)(B * H), cch), dim3(DFT_THREADS), 0, s, (const float*)P, twiddles_bwd + a.re[0],
                       twiddles_bwd + a.im[0], a.Kp[0], dx, rows_hl, t.k2, W, C, DpotBwdEpilogue{dout});
    TANTE_CHECK_LAUNCH();
  }
  return 0;
}
