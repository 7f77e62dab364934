// Backward of the AFNO spectral filter (afno_filter.hip): what torch.autograd derives for the reference's models/afno.py:103-117 with the
// axis swap and first skip of l.154-159, on channels-last fp32 rows.  The forward is a chain of real-linear maps on [re | im] rows and two
// pointwise functions,
//
//   P = T1 x   X = T2 P   U = X M1   V = gelu(U)   Yp = V M2   Y = softshrink(Yp)   G = T3 Y   out = Re(T4 G) + residual,
//
// and the backward is the same three-launch shape run in reverse against the conjugate-transposed tables (from the host, packed like the
// forward's: af_tables(H, W, true)), plus one small reduce:
//
//   launch B1 (b, w, 64 channels)   dG[w, l] = sum_h conj(T4[h, l]) dout[h, w]                       real in, complex out
//   launch B2 (b, l, channel block) dY[k]    = sum_w conj(T3[w, k]) dG[w, l]
//                                   X, U, V, Yp recomputed from the saved P with the forward's own instruction sequence: the
//                                   threshold decisions [|Yp| > lambda] are the forward's, bit for bit
//                                   dYp = dY [|Yp| > lambda]     dV = dYp M2^T     dU = dV gelu'(U)     dX = dU M1^T
//                                   dP[h]    = sum_k conj(T2[k, h]) dX[k]
//                                   dM2 = V^T dYp,  dM1 = X^T dU  folded to the parameter's (bs, bs, 2): dWr = TL + BR, dWi = TR - BL
//   launch B3 (b, h, 64 channels)   dx[h, w] = Re sum_l conj(T1[l, w]) dP[l, h]                      complex in, real out
//   reduce                          dw[e]    = sum over (b, l) of the partials, in a fixed order (eight interleaved running sums)
//
// B1 is dft_r2c_rows_kernel reading the strided columns of dout, B3 dft_c2r_rows_kernel<AfnoBwdEpilogue> (dft_rows.hip.h); B2,
// afno_bwd_mix_kernel, and the reduce are this file's.
//
// The weight gradients are summed over the B Lc workgroups of a channel block without atomics: every workgroup of B2 stores its folded
// partial to its own slot of the workspace and the reduce adds the slots in a fixed order, so two runs give the same bits.
//
// LDS of B2, dynamic (past the 64 KB static limit at the largest shapes), four tiles of Kc16 = Kc rounded up to 16 rows (<= 48) with
// stride ld = 2 bsP + 4 floats (<= 132):
//
//   D   dY, then dYp in place                          Kc16 rows
//   X   the recomputed spectrum                        Kc16 rows
//   U   the pre-activation, then dU in place           Kc16 rows    } R: before U and V exist, the dG tile (W rows) and then the P tile
//   V   gelu(U), then dX                               Kc16 rows    } (H rows) live here, max(2 Kc16, r4(max(H, W))) rows
//
// (2 Kc16 + rows of R) ld floats: 192 x 132 x 4 = 101376 bytes at a 64 x 64 grid with 64-channel blocks, 34816 at 32 x 32 with 32-channel blocks.
// Every product is v_mfma_f32_16x16x4_f32 as in the forward; LDS is plain C++ between barriers.
#include "afno_filter.hip.h"

namespace {

constexpr int AFB_LDS_MAX = 4 * AF_ROWS_B * AF_LD * (int)sizeof(float);     // 101376

inline int afb_rows_r(int H, int W, int Kc) {
  const int a = 2 * r16(Kc), b = r4(H > W ? H : W);
  return a > b ? a : b;
}

// (dWr + i dWi)[i][j] of one channel block from the real-ified product A^T B over `rows` rows, A = [Ar | Ai], B = [Br | Bi] in LDS:
// dWr = Ar^T Br + Ai^T Bi (top-left + bottom-right), dWi = Ar^T Bi - Ai^T Br (top-right - bottom-left); -> part (bs, bs, 2)
__device__ __forceinline__ void fold_wgrad(const float* A, const float* Bm, int ld, int bsP, int bs, int rows, float* __restrict__ part) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
  const int NTc = bsP >> 4;
  for (int t = wave; t < NTc * NTc; t += AF_THREADS / 64) {
    const int mt = t / NTc, nt = t % NTc;
    f32x4 wr = {0.f, 0.f, 0.f, 0.f}, wi = {0.f, 0.f, 0.f, 0.f};
    const float* a = A + kk * ld + mt * 16 + i;
    const float* bm = Bm + kk * ld + nt * 16 + i;
    for (int k = 0; k < rows; k += 4) {
      const float ar = a[k * ld], ai = a[k * ld + bsP], br = bm[k * ld], bi = bm[k * ld + bsP];
      wr = mfma4(ar, br, wr);
      wr = mfma4(ai, bi, wr);
      wi = mfma4(ar, bi, wi);
      wi = mfma4(-ai, br, wi);
    }
    const int col = nt * 16 + i;
    for (int r = 0; r < 4; ++r) {
      const int row = mt * 16 + 4 * kk + r;
      if (row < bs && col < bs) {
        float* p = part + ((long)row * bs + col) * 2;
        p[0] = wr[r];
        p[1] = wi[r];
      }
    }
  }
}

// ---- launch B2: adjoint of the inverse along k, the block MLP's backward, adjoint of the transform along h ----------------------------
__global__ __launch_bounds__(AF_THREADS) void afno_bwd_mix_kernel(
    const float* __restrict__ P, const float* __restrict__ dG, const float* __restrict__ T2r, const float* __restrict__ T2i, int ldt2,
    const float* __restrict__ A3r, const float* __restrict__ A3i, int lda3, const float* __restrict__ A2r, const float* __restrict__ A2i, int lda2,
    const float* __restrict__ w1, const float* __restrict__ w2, float lam, float* __restrict__ dP, float* __restrict__ part1,
    float* __restrict__ part2, uint8_t* __restrict__ keep, int H, int W, int C, int bs, int Lc, int Kc) {
  extern __shared__ __attribute__((aligned(16))) float af_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const int l = blockIdx.x, g = blockIdx.y;
  const long b = blockIdx.z;
  const int bsP = (bs + 15) & ~15, n2 = 2 * bsP, ld = n2 + 4;
  const int Hp = (H + 3) & ~3, Wp = (W + 3) & ~3, Kc16 = (Kc + 15) & ~15, Kc4 = (Kc + 3) & ~3;
  float* tD = af_lds;
  float* tX = tD + Kc16 * ld;
  float* tU = tX + Kc16 * ld;
  float* tV = tU + Kc16 * ld;
  float* tR = tU;
  const int MT = Kc16 >> 4, NTc = bsP >> 4, NT2 = n2 >> 4;
  // dG[b][w][l][re | im][C] -> R[w][re block | im block]
  const float* Gl = dG + ((b * W) * Lc + l) * 2 * (long)C + (long)g * bs;
  for (int idx = tid; idx < Wp * n2; idx += AF_THREADS) {
    const int w = idx / n2, j = idx % n2, ri = j / bsP, c = j % bsP;
    tR[w * ld + j] = (w < W && c < bs) ? Gl[(((long)w * Lc) * 2 + ri) * C + c] : 0.0f;
  }
  __syncthreads();
  // dY[k] = sum_w conj(T3[w, k]) dG[w]  -> D   (rows Kc..Kc16 are zero: the table's padding)
  for (int t = wave; t < MT * NTc; t += AF_THREADS / 64) {
    const int mt = t / NTc, nt = t % NTc;
    f32x4 dr = {0.f, 0.f, 0.f, 0.f}, di = {0.f, 0.f, 0.f, 0.f};
    table_tile<true, true>(A3r, A3i, lda3, mt * 16, tR, ld, nt * 16, bsP, Wp, dr, di);
    for (int r = 0; r < 4; ++r) {
      float* p = tD + (mt * 16 + 4 * kk + r) * ld + nt * 16 + i;
      p[0] = dr[r];
      p[bsP] = di[r];
    }
  }
  __syncthreads();
  // from here to Yp: afno_mix_kernel's statements, so that the recomputed values are the forward's
  const float* Pl = P + ((b * Lc + l) * H) * 2 * (long)C + (long)g * bs;
  for (int idx = tid; idx < Hp * n2; idx += AF_THREADS) {
    const int h = idx / n2, j = idx % n2, ri = j / bsP, c = j % bsP;
    tR[h * ld + j] = (h < H && c < bs) ? Pl[((long)h * 2 + ri) * C + c] : 0.0f;
  }
  __syncthreads();
  for (int t = wave; t < MT * NTc; t += AF_THREADS / 64) {
    const int mt = t / NTc, nt = t % NTc;
    f32x4 dr = {0.f, 0.f, 0.f, 0.f}, di = {0.f, 0.f, 0.f, 0.f};
    table_tile<true, true>(T2r, T2i, ldt2, mt * 16, tR, ld, nt * 16, bsP, Hp, dr, di);
    for (int r = 0; r < 4; ++r) {
      float* p = tX + (mt * 16 + 4 * kk + r) * ld + nt * 16 + i;
      p[0] = dr[r];
      p[bsP] = di[r];
    }
  }
  __syncthreads();
  const float* wm1 = w1 + (long)g * n2 * n2;
  const float* wm2 = w2 + (long)g * n2 * n2;
  for (int layer = 0; layer < 2; ++layer) {
    const float* src = layer == 0 ? tX : tV;
    const float* wm = layer == 0 ? wm1 : wm2;
    for (int nt = wave; nt < NT2; nt += AF_THREADS / 64) {
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
          for (int r = 0; r < 4; ++r) {
            const int row = mt * 16 + 4 * kk + r, col = nt * 16 + i, at = row * ld + col;
            if (layer == 0) {
              tU[at] = d[mt][r];
              tV[at] = gelu_erf_f(d[mt][r]);
            } else {      // Yp stays in the register: softshrink's own comparisons decide what passes
              const float yp = d[mt][r];
              const bool kept = yp > lam || yp < -lam;
              if (!kept) tD[at] = 0.0f;
              const int c = col % bsP;
              if (keep && row < Kc && c < bs) keep[((((b * Lc + l) * Kc + row) * 2 + col / bsP) * (long)C) + (long)g * bs + c] = kept ? 1 : 0;
            }
          }
    }
    __syncthreads();
  }
  const long slot = ((b * Lc + l) * (long)(C / bs) + g) * bs * bs * 2;
  // dM2 = V^T dYp;  dU = (dYp M2^T) gelu'(U) in place of U
  fold_wgrad(tV, tD, ld, bsP, bs, Kc16, part2 + slot);
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      __syncthreads();
      fold_wgrad(tX, tU, ld, bsP, bs, Kc16, part1 + slot);      // dM1 = X^T dU;  dX = dU M1^T -> V
    }
    const float* src = pass == 0 ? tD : tU;
    const float* wm = pass == 0 ? wm2 : wm1;
    for (int nt = wave; nt < NT2; nt += AF_THREADS / 64) {      // the layer loop against the transposed matrix: B[k][j] = M[j][k]
      f32x4 d[AF_ROWS_B / 16];
      for (int mt = 0; mt < AF_ROWS_B / 16; ++mt) d[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* a = src + i * ld + kk;
      const float* bw = wm + (long)(nt * 16 + i) * n2 + kk;
      for (int k = 0; k < n2; k += 4) {
        const float bv = bw[k];
#pragma unroll
        for (int mt = 0; mt < AF_ROWS_B / 16; ++mt)
          if (mt < MT) d[mt] = mfma4(a[mt * 16 * ld + k], bv, d[mt]);
      }
#pragma unroll
      for (int mt = 0; mt < AF_ROWS_B / 16; ++mt)
        if (mt < MT)
          for (int r = 0; r < 4; ++r) {
            const int at = (mt * 16 + 4 * kk + r) * ld + nt * 16 + i;
            if (pass == 0)
              tU[at] = d[mt][r] * act_df(tU[at], TANTE_ACT_GELU_ERF);
            else
              tV[at] = d[mt][r];
          }
    }
  }
  __syncthreads();
  // dP[h] = sum_k conj(T2[k, h]) dX[k]
  const int MTh = (H + 15) >> 4;
  for (int t = wave; t < MTh * NTc; t += AF_THREADS / 64) {
    const int mt = t / NTc, nt = t % NTc;
    f32x4 dr = {0.f, 0.f, 0.f, 0.f}, di = {0.f, 0.f, 0.f, 0.f};
    table_tile<true, true>(A2r, A2i, lda2, mt * 16, tV, ld, nt * 16, bsP, Kc4, dr, di);
    const int c = nt * 16 + i;
    for (int r = 0; r < 4; ++r) {
      const int h = mt * 16 + 4 * kk + r;
      if (h < H && c < bs) {
        float* p = dP + (((b * Lc + l) * H + h) * 2) * (long)C + (long)g * bs + c;
        p[0] = dr[r];
        p[C] = di[r];
      }
    }
  }
}

// ---- launch B3's store: dx is the transform's value itself ------------------------------------------------------------------------------
struct AfnoBwdEpilogue {
  __device__ float operator()(float v, long) const { return v; }
};

// ---- the weight gradients: the workgroups' partials, added in slot order ------------------------------------------------------------------
__global__ __launch_bounds__(256) void afno_wgrad_reduce_kernel(const float* __restrict__ part1, const float* __restrict__ part2, long n_part,
                                                                long n_el, float* __restrict__ dw1, float* __restrict__ dw2, int accumulate) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_el) return;
  const float* part = blockIdx.y == 0 ? part1 : part2;
  float* dw = blockIdx.y == 0 ? dw1 : dw2;
  // eight running sums over the slots p = j (mod 8), combined pairwise: a fixed order with eight loads in flight per lane
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  long p = 0;
  for (; p + 8 <= n_part; p += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += part[(p + j) * n_el + e];
  for (; p < n_part; ++p) s[0] += part[p * n_el + e];
  const float sum = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  dw[e] = accumulate ? dw[e] + sum : sum;
}

TantePerDevice g_afb_attr;

}  // namespace

extern "C" int64_t tante_afno_twiddle_bwd_floats(int H, int W) {
  if (H < 1 || W < 1 || H > AF_MAX || W > AF_MAX) return -1;
  return af_tables(H, W, true).total;
}

extern "C" int64_t tante_afno_filter_bwd_workspace_bytes(int64_t B, int H, int W, int C, int bs) {
  if (af_reason(B, H, W, C, bs)) return -1;
  const AfTables t = af_tables(H, W);
  // dG (B, W, Lc, 2, C), dP (B, Lc, H, 2, C), then per weight the (B Lc) partials of (C / bs, bs, bs, 2)
  return (int64_t)sizeof(float) * 2 * B * t.Lc * ((int64_t)H + W + 2 * (int64_t)bs) * C;
}

extern "C" int tante_afno_filter_bwd(const float* dout, const float* P, int64_t B, int H, int W, int C, int bs, const float* twiddles,
                                     const float* twiddles_bwd, const float* w1, const float* w2, float lambda, float* dx, float* dw1, float* dw2,
                                     int accumulate, uint8_t* keep, void* work, int64_t work_bytes, void* stream) {
  if (const char* why = af_reason(B, H, W, C, bs))
    TANTE_FAIL(-2, "tante_afno_filter_bwd: %s (B %lld, grid %d x %d, C %d, block %d)", why, (long long)B, H, W, C, bs);
  if (!dout || !P || !twiddles || !twiddles_bwd || !w1 || !w2 || !dx || !dw1 || !dw2) TANTE_FAIL(-1, "tante_afno_filter_bwd: null argument");
  if (dx == dout) TANTE_FAIL(-1, "tante_afno_filter_bwd: dx may not alias dout");
  const int64_t need = tante_afno_filter_bwd_workspace_bytes(B, H, W, C, bs);
  if (need > 0 && (!work || work_bytes < need))
    TANTE_FAIL(-1, "tante_afno_filter_bwd: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  const AfTables t = af_tables(H, W), a = af_tables(H, W, true);
  float* dG = (float*)work;
  float* dP = dG + 2 * B * W * (int64_t)t.Lc * C;
  float* part1 = dP + 2 * B * t.Lc * (int64_t)H * C;
  float* part2 = part1 + 2 * B * t.Lc * (int64_t)bs * C;
  hipStream_t s = (hipStream_t)stream;
  if (B > 0) {
    const unsigned cch = (unsigned)((C + DFT_CH - 1) / DFT_CH);
    const long C1 = C, C2 = 2l * C;
    const DftRows bwd_h = {H * W * C1, C1, W * C1, W * t.Lc * C2, t.Lc * C2, C2, W};      // the columns (b, w) of dout -> dG[b][w]
    const DftRows bwd_w = {t.Lc * H * C2, C2, H * C2, H * W * C1, W * C1, C1, H};         // dP[b][l][h] -> dx rows (b, h)
    hipLaunchKernelGGL(dft_r2c_rows_kernel, dim3((unsigned)(B * W), cch), dim3(DFT_THREADS), 0, s, dout, twiddles_bwd + a.re[3],
                       twiddles_bwd + a.im[3], a.Kp[3], dG, bwd_h, H, t.Lc, C);
    TANTE_CHECK_LAUNCH();
    const int bsP = r16(bs);
    const size_t lds = sizeof(float) * (size_t)(2 * r16(t.Kc) + afb_rows_r(H, W, t.Kc)) * (2 * bsP + 4);
    if (lds > (size_t)AFB_LDS_MAX) TANTE_FAIL(-1, "tante_afno_filter_bwd: %zu bytes of LDS, %d planned", lds, AFB_LDS_MAX);
    g_afb_attr.once([] { (void)hipFuncSetAttribute((const void*)afno_bwd_mix_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, AFB_LDS_MAX); });
    hipLaunchKernelGGL(afno_bwd_mix_kernel, dim3((unsigned)t.Lc, (unsigned)(C / bs), (unsigned)B), dim3(AF_THREADS), lds, s, P, (const float*)dG,
                       twiddles + t.re[1], twiddles + t.im[1], t.Kp[1], twiddles_bwd + a.re[2], twiddles_bwd + a.im[2], a.Kp[2],
                       twiddles_bwd + a.re[1], twiddles_bwd + a.im[1], a.Kp[1], w1, w2, lambda, dP, part1, part2, keep, H, W, C, bs, t.Lc, t.Kc);
    TANTE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dft_c2r_rows_kernel<AfnoBwdEpilogue>, dim3((unsigned)(B * H), cch), dim3(DFT_THREADS), 0, s, (const float*)dP,
                       twiddles_bwd + a.re[0], twiddles_bwd + a.im[0], a.Kp[0], dx, bwd_w, t.Lc, W, C, AfnoBwdEpilogue{});
    TANTE_CHECK_LAUNCH();
  }
  const long n_el = 2l * C * bs;
  hipLaunchKernelGGL(afno_wgrad_reduce_kernel, dim3((unsigned)((n_el + 255) / 256), 2), dim3(256), 0, s, (const float*)part1, (const float*)part2,
                     (long)(B * t.Lc), n_el, dw1, dw2, accumulate);
  TANTE_CHECK_LAUNCH();
  return 0;
}
