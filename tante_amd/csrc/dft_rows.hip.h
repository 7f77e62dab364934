// What the AFNO filter (afno_filter.hip, afno_filter_bwd.hip) and the DPOT mixer (dpot_mixer.hip) share: the layout of a packed twiddle
// buffer, the complex table product on fp32 MFMA, and the two row kernels that apply one table to every slab of a channels-last tensor.
//
//   dft_r2c_rows_kernel   real slab (K rows) -> complex rows:  out[m] = sum_k T[m, k] in[k],  m < M,  out row = [re (C) | im (C)]
//   dft_c2r_rows_kernel   complex slab (K rows of [re (C) | im (C)]) -> real rows:  out[m] = epilogue(Re sum_k T[m, k] in[k])
//
// A workgroup is slab (b, j) and a chunk of 64 channels: grid (B slabs, ceil(C / 64)).  Where slab, input row and result row lie is the
// caller's DftRows record, so one kernel serves a transform along either axis, reading rows or strided columns.  The tables come from
// the host (float64, rounded once, zero padded to whole 16-row / 4-column fragments), so no kernel checks a table bound; data tiles are
// zero filled to the same padding in LDS.  K, M <= 64.
#pragma once
#include "common.hip.h"

namespace {

constexpr int DFT_MAX = 64;                // grid points per axis: rows of a slab, rows of a result
constexpr int DFT_THREADS = 256;           // four waves; a wave owns whole 16 x 16 result tiles
constexpr int DFT_CH = 64;                 // channels per workgroup
constexpr int DFT_LD1 = DFT_CH + 4;        // LDS row stride of a real slab
constexpr int DFT_LD = 2 * DFT_CH + 4;     // LDS row stride of a complex slab ([re | im] rows); 4 (mod 64): the A-operand reads of 16 rows
                                           // x 4 columns fall into 64 different banks

inline int r4(int n) { return (n + 3) & ~3; }
inline int r16(int n) { return (n + 15) & ~15; }

struct DftTables {       // element offsets into the packed twiddle buffer: table t has its real plane at re[t], the imaginary one behind it
  int Kp[4];             // row stride of table t: its columns rounded up to 4
  long re[4], im[4], total;
};

// four tables (M[t], K[t]), each a real then an imaginary plane of r16(M[t]) rows x r4(K[t]) columns
inline DftTables dft_tables(const int (&M)[4], const int (&K)[4]) {
  DftTables t;
  long off = 0;
  for (int i = 0; i < 4; ++i) {
    const long plane = (long)r16(M[i]) * r4(K[i]);
    t.Kp[i] = r4(K[i]);
    t.re[i] = off;
    t.im[i] = off + plane;
    off += 2 * plane;
  }
  t.total = off;
  return t;
}

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

struct DftRows {         // element strides of sample b, slab j and row (input row k, result row m), channel c at + c
  long in_b, in_j, in_row;
  long out_b, out_j, out_row;
  int slabs;             // slabs per sample: blockIdx.x = b slabs + j
};

__global__ __launch_bounds__(DFT_THREADS) void dft_r2c_rows_kernel(const float* __restrict__ in, const float* __restrict__ Tr,
                                                                   const float* __restrict__ Ti, int ldt, float* __restrict__ out, DftRows s, int K,
                                                                   int M, int C) {
  __shared__ float xs[DFT_MAX * DFT_LD1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const long b = blockIdx.x / s.slabs;
  const int j = blockIdx.x % s.slabs;
  const int c0 = blockIdx.y * DFT_CH;
  const int nc = (C - c0) < DFT_CH ? (C - c0) : DFT_CH;
  const int Kp = (K + 3) & ~3;
  const float* src = in + b * s.in_b + j * s.in_j + c0;
  for (int idx = tid; idx < Kp * DFT_CH; idx += DFT_THREADS) {
    const int k = idx / DFT_CH, c = idx % DFT_CH;
    xs[k * DFT_LD1 + c] = (k < K && c < nc) ? src[k * s.in_row + c] : 0.0f;
  }
  __syncthreads();
  float* dst = out + b * s.out_b + j * s.out_j + c0;
  const int MT = (M + 15) >> 4, NT = (nc + 15) >> 4;
  for (int t = wave; t < MT * NT; t += DFT_THREADS / 64) {
    const int mt = t / NT, nt = t % NT;
    f32x4 dr = {0.f, 0.f, 0.f, 0.f}, di = {0.f, 0.f, 0.f, 0.f};
    table_tile<false, true>(Tr, Ti, ldt, mt * 16, xs, DFT_LD1, nt * 16, 0, Kp, dr, di);
    const int c = nt * 16 + i;
    for (int r = 0; r < 4; ++r) {
      const int m = mt * 16 + 4 * kk + r;
      if (m < M && c < nc) {
        float* p = dst + m * s.out_row + c;
        p[0] = dr[r];
        p[C] = di[r];
      }
    }
  }
}

// Epilogue: float operator()(float v, long o) const -- what is stored at element o of `out` for the transform's value v.  `out` may be
// an operand of the epilogue (a residual added in place), each element read and written by the same lane.
template <class Epilogue>
__global__ __launch_bounds__(DFT_THREADS) void dft_c2r_rows_kernel(const float* __restrict__ in, const float* __restrict__ Tr,
                                                                   const float* __restrict__ Ti, int ldt, float* out, DftRows s, int K, int M, int C,
                                                                   Epilogue epilogue) {
  __shared__ float gs[DFT_MAX * DFT_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const long b = blockIdx.x / s.slabs;
  const int j = blockIdx.x % s.slabs;
  const int c0 = blockIdx.y * DFT_CH;
  const int nc = (C - c0) < DFT_CH ? (C - c0) : DFT_CH;
  const int Kp = (K + 3) & ~3;
  const float* src = in + b * s.in_b + j * s.in_j + c0;
  for (int idx = tid; idx < Kp * 2 * DFT_CH; idx += DFT_THREADS) {
    const int k = idx / (2 * DFT_CH), n = idx % (2 * DFT_CH), ri = n / DFT_CH, c = n % DFT_CH;
    gs[k * DFT_LD + n] = (k < K && c < nc) ? src[k * s.in_row + (long)ri * C + c] : 0.0f;
  }
  __syncthreads();
  const long o0 = b * s.out_b + j * s.out_j + c0;
  const int MT = (M + 15) >> 4, NT = (nc + 15) >> 4;
  for (int t = wave; t < MT * NT; t += DFT_THREADS / 64) {
    const int mt = t / NT, nt = t % NT;
    f32x4 dr = {0.f, 0.f, 0.f, 0.f}, di = {0.f, 0.f, 0.f, 0.f};
    table_tile<true, false>(Tr, Ti, ldt, mt * 16, gs, DFT_LD, nt * 16, DFT_CH, Kp, dr, di);
    const int c = nt * 16 + i;
    for (int r = 0; r < 4; ++r) {
      const int m = mt * 16 + 4 * kk + r;
      if (m < M && c < nc) {
        const long o = o0 + m * s.out_row + c;
        out[o] = epilogue(dr[r], o);
      }
    }
  }
}

}  // namespace
