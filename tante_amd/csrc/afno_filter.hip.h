// What the forward (afno_filter.hip) and the backward (afno_filter_bwd.hip) of the AFNO spectral filter share: the tile constants, the
// layout of a packed twiddle buffer, the complex table product on fp32 MFMA and the shape predicate's reason.
#pragma once
#include "common.hip.h"

namespace {

constexpr int AF_MAX = 64;                 // grid points per axis, channels per block
constexpr int AF_THREADS = 256;            // four waves; a wave owns whole 16 x 16 result tiles
constexpr int AF_CH = 64;                  // channels per workgroup of launches 1 and 3
constexpr int AF_LD1 = AF_CH + 4;          // LDS row stride of launch 1 (real rows)
constexpr int AF_LD = 2 * AF_MAX + 4;      // LDS row stride of launches 2 and 3 ([re | im] rows); 4 (mod 64): the A-operand reads of
                                           // 16 rows x 4 columns fall into 64 different banks
constexpr int AF_ROWS_A = 64;              // launch 2: rows of the P tile (h) / the hidden tile (k)
constexpr int AF_ROWS_B = 48;              // launch 2: rows of the spectrum tile, Kc <= 33 padded to 16

inline int r4(int n) { return (n + 3) & ~3; }
inline int r16(int n) { return (n + 15) & ~15; }

struct AfTables {        // element offsets into the packed twiddle buffer: table t has its real plane at re[t], the imaginary one behind it
  int Lc, Kc;
  int M[4], K[4], Mp[4], Kp[4];
  long re[4], im[4], total;
};

// adjoint = false: T1 (Lc, W), T2 (Kc, H), T3 (W, Kc), T4 (H, Lc); adjoint = true: their conjugate transposes, in the same order
inline AfTables af_tables(int H, int W, bool adjoint = false) {
  AfTables t;
  t.Lc = H < W ? H : W;
  t.Kc = (H / 2 + 1) < (W / 2 + 1) ? (H / 2 + 1) : (W / 2 + 1);
  const int M[4] = {t.Lc, t.Kc, W, H}, K[4] = {W, H, t.Kc, t.Lc};
  long off = 0;
  for (int i = 0; i < 4; ++i) {
    t.M[i] = adjoint ? K[i] : M[i], t.K[i] = adjoint ? M[i] : K[i];
    t.Mp[i] = r16(t.M[i]), t.Kp[i] = r4(t.K[i]);
    t.re[i] = off;
    t.im[i] = off + (long)t.Mp[i] * t.Kp[i];
    off += 2l * t.Mp[i] * t.Kp[i];
  }
  t.total = off;
  return t;
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// (dr + i di) = sum_k (Tr + i Ti)[m0 + i][k] * (B[k][n0 + j] + i B[k][n0 + j + im_off]) over k < Kp (a multiple of 4), B in LDS
template <bool B_COMPLEX, bool WANT_IM>
__device__ __forceinline__ void table_tile(const float* __restrict__ Tr, const float* __restrict__ Ti, int ldt, int m0, const float* Bs, int ldb,
                                           int n0, int im_off, int Kp, f32x4& dr, f32x4& di) {
  const int lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
  const float* tr = Tr + (long)(m0 + i) * ldt + kk;
  const float* ti = Ti + (long)(m0 + i) * ldt + kk;
  const float* b = Bs + kk * ldb + n0 + i;
  for (int k = 0; k < Kp; k += 4) {
    const float ar = tr[k], ai = ti[k];
    const float br = b[k * ldb];
    dr = mfma4(ar, br, dr);
    if (WANT_IM) di = mfma4(ai, br, di);
    if (B_COMPLEX) {
      const float bi = b[k * ldb + im_off];
      dr = mfma4(-ai, bi, dr);
      if (WANT_IM) di = mfma4(ar, bi, di);
    }
  }
}

inline const char* af_reason(int64_t B, int H, int W, int C, int bs) {
  if (H < 1 || W < 1 || H > AF_MAX || W > AF_MAX) return "token grid outside 1..64 points per axis";
  if (bs < 1 || bs > AF_MAX) return "channel block size outside 1..64";
  if (C < 1 || C % bs) return "channels are not a whole number of blocks";
  if (B < 0 || B > 65535) return "more than 65535 samples per call";
  return nullptr;
}

}  // namespace
