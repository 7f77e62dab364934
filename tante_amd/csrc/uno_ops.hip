// UNO's operator block (reference models/uno.py: OperatorBlock_2D = SpectralConv2d_Uno + pointwise_op_2D, then the erf GELU) on
// channels-first fp32 planes x (B, Ci, Hi, Wi) -> out (B, Co, Ho, Wo), Ho x Wo free of Hi x Wi: the inverse transform does the U-Net's
// resampling.  Both tensors take an IMAGE STRIDE in elements, so a block reads or writes a channel slice of a wider buffer and the
// model's three concatenations are never executed.
//
// Only the kept 2 m1 x m2 modes exist anywhere: no full spectrum, no zero-filled out_ft.  With J = 2 m1, kin = [0..m1-1, Hi-m1..Hi-1],
// kout = [0..m1-1, Ho-m1..Ho-1]:
//
//   P[b,i,h,l]   = sum_w x[b,i,h,w] e^{-2 pi i l w / Wi} / (Hi Wi)            l < m2
//   X[b,i,j,l]   = sum_h e^{-2 pi i kin[j] h / Hi} P[b,i,h,l]                 j < J
//   Y[b,o,j,l]   = sum_i X[b,i,j,l] Wt[i,o,j,l]                               Wt = weights1 (j < m1), weights2 (j >= m1), read in place
//   Z[b,o,y,l]   = sum_j live[j] e^{+2 pi i kout[j] y / Ho} Y[b,o,j,l]        live[j] = 0 for a top-band row the bottom band also writes
//   out[b,o,y,x] = Re sum_l c[l] e^{+2 pi i l x / Wo} Z[b,o,y,l]
//
// Every transform is a REAL product against a host-built table (float64, rounded once): a complex operand is the K-concatenation
// [re | im] of its row, so  Re = [cos | sin] . [re | im]  is one real GEMM, and the pointwise path's resize tables A_w / A_h
// (F.interpolate bicubic, align_corners, antialias, as matrices) are further rows or further K-columns of the same tables:
//
//   the grid shrinks (Ho Wo <= Hi Wi), resize BEFORE the 1 x 1:                the grid grows, 1 x 1 BEFORE the resize:
//   1  P1[b,i,m,h]  = T1 . x rows      T1 = [cos, -sin interleaved ; A_w]     1  P1 = T1 . x rows            T1 = [cos, -sin interleaved]
//   2  X[b,i,m,l]   = T2 . [Pr | Pi]   T2 = [cos | sin ; -sin | cos]          2  X                           as on the left
//   3  S[b,i,y,x]   = A_h . R                                                 3  Y = mode mix
//   4  Y            = mode mix                                                4  V[b,o,h,w] = w . x          the 1 x 1 on the input grid
//   5  U[b,o,y,x]   = w . S            the 1 x 1 on the output grid           5  Zrow[b,o,y,:2 m2] = T4 . [Yr ; Yi]
//   6  Zrow[b,o,y,:] = T4 . [Yr ; Yi]  rows [Zr | Zi]                         6  Zrow[b,o,y,2 m2:] = A_h . V
//   7  out = gelu(T5 . Zrow + U + bias)   T5 = [c cos | -c sin]               7  out = gelu(T5 . Zrow + bias)   T5 = [c cos | -c sin | A_w]
//
// so the sum of the two paths is the K-concatenation of the last product (or its addend), and sum, bias and GELU go in the last store.
// Launches 1, 2, 3, 5, 6, 7 are one kernel, uno_gemm_kernel: D[p] = T . B[p] per plane with element strides on both sides,
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation, in both compute modes).  A operand lane (i = l & 15, k = l >> 4), B
// operand lane (k = l >> 4, j = l & 15), result register r = row 4 (l >> 4) + r, column l & 15.  A wave owns 16 columns and up to four
// 16-row tiles; it shares nothing with the other waves, so there is no LDS and no barrier in it.
//
// The mode mix is a weight stream: weights1 / weights2 (Ci, Co, m1, m2) complex64 are read in place as float2 -- for a fixed input
// channel the (o, k, l) index is contiguous, and the 64 lanes of a wave run along it.  A workgroup's four waves split the input channels
// into four contiguous ranges, each holding up to 8 images' sums in registers; the partial sums meet in LDS in wave order.  Every weight
// is read once per pass of 8 images; every sum has a fixed order (explicit fmaf, no atomics) that does not depend on the image's
// position in the batch.  LDS is plain C++ between barriers.
#include "common.hip.h"

namespace {

constexpr int UNO_MAX_DIM = 512;           // grid points per axis, input and output
constexpr int UNO_MAX_CH = 512;            // channels, input and output
constexpr int UNO_MAX_PLANES = 65535;      // B * max(Ci, Co): the plane index is gridDim.z
constexpr int UNO_THREADS = 256;           // four waves
constexpr int UNO_MT = 4;                  // 16-row tiles per wave of uno_gemm_kernel
constexpr int UNO_PASS = 8;                // images per pass of the mode mix

// D[p][m, n] = act(sum_k T[m, k] B[p][k, n] + add[p][m, n] + bias[p % pdiv]), plane p = (p / pdiv, p % pdiv)
struct UnoGemm {
  const float* T;        // (M, K) dense, row stride ldt
  int ldt, M, K, N;
  const float* B;        // element (k, n) of plane p at B + (p / pdiv) b_hi + (p % pdiv) b_lo + k sk + n sn
  long b_hi, b_lo;
  int sk, sn;
  float* D;              // element (m, n) at D + (p / pdiv) d_hi + (p % pdiv) d_lo + (m % msplit) sm + (m / msplit) sm_hi + n sn_d
  long d_hi, d_lo;
  int sm, sm_hi, msplit, sn_d;
  const float* add;      // NULL, or the addend, indexed as D inside a plane
  long a_hi, a_lo;
  const float* bias;     // NULL, or one value per p % pdiv
  int pdiv, gelu;
};

__global__ __launch_bounds__(UNO_THREADS) void uno_gemm_kernel(const UnoGemm g) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const int n0 = (blockIdx.x * (UNO_THREADS / 64) + wave) * 16;
  if (n0 >= g.N) return;                                    // no barrier in this kernel: a wave may leave alone
  const int m0 = blockIdx.y * (16 * UNO_MT);
  const long p = blockIdx.z, ph = p / g.pdiv, pl = p % g.pdiv;
  const int n = n0 + i;
  const bool nok = n < g.N;
  const float* b = g.B + ph * g.b_hi + pl * g.b_lo + (long)(nok ? n : g.N - 1) * g.sn;     // a column past the end repeats the last one
  f32x4 acc[UNO_MT];
  const float* trow[UNO_MT];
  bool tok[UNO_MT];
#pragma unroll
  for (int mt = 0; mt < UNO_MT; ++mt) {
    acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int m = m0 + mt * 16 + i;
    tok[mt] = m < g.M;
    trow[mt] = g.T + (long)(tok[mt] ? m : g.M - 1) * g.ldt;
  }
  const int MT = (g.M - m0 + 15) >> 4;                      // uniform over the wave
  for (int k = 0; k < g.K; k += 4) {
    const int kx = k + kk;
    const bool kok = kx < g.K;
    const int kc = kok ? kx : g.K - 1;
    const float bv = kok ? b[(long)kc * g.sk] : 0.0f;
#pragma unroll
    for (int mt = 0; mt < UNO_MT; ++mt)
      if (mt < MT) {
        const float av = (kok && tok[mt]) ? trow[mt][kc] : 0.0f;
        acc[mt] = mfma4(av, bv, acc[mt]);
      }
  }
  if (!nok) return;
  float* d = g.D + ph * g.d_hi + pl * g.d_lo + (long)n * g.sn_d;
  const float* a = g.add ? g.add + ph * g.a_hi + pl * g.a_lo + (long)n * g.sn_d : nullptr;
  const float bias = g.bias ? g.bias[pl] : 0.0f;
#pragma unroll
  for (int mt = 0; mt < UNO_MT; ++mt)
    if (mt < MT) {
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + mt * 16 + 4 * kk + r;
        if (m < g.M) {
          const long o = (long)(m % g.msplit) * g.sm + (long)(m / g.msplit) * g.sm_hi;
          float v = acc[mt][r];
          if (a) v += a[o];
          v += bias;
          d[o] = g.gelu ? gelu_erf_f(v) : v;
        }
      }
    }
}

// Y[b][o][ri][j][l] = sum_i X[b][i][ri][j][l] (x) W[band(j)][i][o][k][l], complex; nb <= 8 images from X / Y on
__global__ __launch_bounds__(UNO_THREADS) void uno_mix_kernel(const float* __restrict__ X, const float2* __restrict__ w1, const float2* __restrict__ w2,
                                                              float* __restrict__ Y, int nb, int Ci, int Co, int Q, long xs, long ys) {
  __shared__ float red[3 * 2 * UNO_PASS * 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int band = blockIdx.y;
  const long CoQ = (long)Co * Q;
  const long t = (long)blockIdx.x * 64 + lane;
  const bool valid = t < CoQ;
  const long tc = valid ? t : CoQ - 1;
  const int o = (int)(tc / Q), q = (int)(tc % Q);
  const float2* w = (band ? w2 : w1) + tc;
  const long plane = 2l * Q;                       // the imaginary half of a (b, channel) plane starts here: J m2 = 2 Q
  const float* xq = X + (long)band * Q + q;
  const int chunk = (Ci + 3) >> 2;
  const int i0 = wave * chunk, i1 = (i0 + chunk) < Ci ? (i0 + chunk) : Ci;
  float sr[UNO_PASS], si[UNO_PASS];
#pragma unroll
  for (int b = 0; b < UNO_PASS; ++b) sr[b] = si[b] = 0.0f;
#pragma unroll 4
  for (int i = i0; i < i1; ++i) {
    const float2 wv = w[(long)i * CoQ];
    const float* xi = xq + (long)i * 2 * plane;
#pragma unroll
    for (int b = 0; b < UNO_PASS; ++b)
      if (b < nb) {
        const float xr = xi[b * xs], xim = xi[b * xs + plane];
        sr[b] = fmaf(xr, wv.x, sr[b]);
        sr[b] = fmaf(-xim, wv.y, sr[b]);
        si[b] = fmaf(xr, wv.y, si[b]);
        si[b] = fmaf(xim, wv.x, si[b]);
      }
  }
  if (wave > 0) {
#pragma unroll
    for (int b = 0; b < UNO_PASS; ++b) {
      red[((wave - 1) * 2 * UNO_PASS + 2 * b) * 64 + lane] = sr[b];
      red[((wave - 1) * 2 * UNO_PASS + 2 * b + 1) * 64 + lane] = si[b];
    }
  }
  __syncthreads();
  if (wave == 0 && valid) {
    float* y = Y + (long)o * 2 * plane + (long)band * Q + q;
#pragma unroll
    for (int b = 0; b < UNO_PASS; ++b)
      if (b < nb) {
        float vr = sr[b], vi = si[b];
        for (int v = 0; v < 3; ++v) {
          vr += red[(v * 2 * UNO_PASS + 2 * b) * 64 + lane];
          vi += red[(v * 2 * UNO_PASS + 2 * b + 1) * 64 + lane];
        }
        y[b * ys] = vr;
        y[b * ys + plane] = vi;
      }
  }
}

inline long r4l(long n) { return (n + 3) & ~3l; }

const char* uno_reason(int64_t B, int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int m1, int m2, int64_t x_stride, int64_t out_stride) {
  if (Ci < 1 || Ci > UNO_MAX_CH || Co < 1 || Co > UNO_MAX_CH) return "channels outside 1..512";
  if (Hi < 1 || Wi < 1 || Hi > UNO_MAX_DIM || Wi > UNO_MAX_DIM) return "input grid outside 1..512 points per axis";
  if (Ho < 1 || Wo < 1 || Ho > UNO_MAX_DIM || Wo > UNO_MAX_DIM) return "output grid outside 1..512 points per axis";
  if (m1 < 1 || m2 < 1) return "modes must be at least 1";
  if (m1 > Hi) return "modes1 exceeds the input rows";
  if (m1 > Ho) return "modes1 exceeds the output rows";
  if (m2 > Wi / 2 + 1) return "modes2 exceeds the input's half spectrum";
  if (m2 > Wo / 2 + 1) return "modes2 exceeds the output's half spectrum";
  if (B < 0 || B * (int64_t)(Ci > Co ? Ci : Co) > UNO_MAX_PLANES) return "more than 65535 (image, channel) planes per call";
  if (x_stride < (int64_t)Ci * Hi * Wi) return "the input image stride is shorter than an image";
  if (out_stride < (int64_t)Co * Ho * Wo) return "the output image stride is shorter than an image";
  return nullptr;
}

struct UnoPlan {
  int down, J, M1, K5, ldz;
  long t_off[5];
  int t_rows[5], t_cols[5];
  long t_total;
  long P1, X, S, Y, UV, Z, w_total;      // float offsets into the workspace
};

UnoPlan uno_plan(int64_t B, int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int m1, int m2, int pointwise) {
  UnoPlan p;
  p.down = (long)Ho * Wo <= (long)Hi * Wi;
  p.J = 2 * m1;
  p.M1 = 2 * m2 + ((pointwise && p.down) ? Wo : 0);
  p.K5 = 2 * m2 + ((pointwise && !p.down) ? Wi : 0);
  p.ldz = p.K5;
  const int rows[5] = {p.M1, 2 * p.J, pointwise ? Ho : 0, 2 * Ho, Wo};
  const int cols[5] = {Wi, 2 * Hi, pointwise ? Hi : 0, 2 * p.J, p.K5};
  long off = 0;
  for (int t = 0; t < 5; ++t) {
    p.t_off[t] = off;
    p.t_rows[t] = rows[t];
    p.t_cols[t] = cols[t];
    off += r4l((long)rows[t] * cols[t]);
  }
  p.t_total = off;
  long w = 0;
  p.P1 = w, w += r4l(B * Ci * (long)p.M1 * Hi);
  p.X = w, w += r4l(B * Ci * 2l * p.J * m2);
  p.S = w, w += (pointwise && p.down) ? r4l(B * Ci * (long)Ho * Wo) : 0;
  p.Y = w, w += r4l(B * Co * 2l * p.J * m2);
  p.UV = w, w += pointwise ? r4l(B * Co * (p.down ? (long)Ho * Wo : (long)Hi * Wi)) : 0;
  p.Z = w, w += r4l(B * Co * (long)Ho * p.ldz);
  p.w_total = w;
  return p;
}

int launch_gemm(const UnoGemm& g, long planes, hipStream_t s) {
  const dim3 grid((unsigned)((g.N + 63) / 64), (unsigned)((g.M + 16 * UNO_MT - 1) / (16 * UNO_MT)), (unsigned)planes);
  hipLaunchKernelGGL(uno_gemm_kernel, grid, dim3(UNO_THREADS), 0, s, g);
  TANTE_CHECK_LAUNCH();
  return 0;
}

UnoGemm gemm_of(const float* T, int M, int K, int N) {
  UnoGemm g = {};
  g.T = T, g.ldt = K, g.M = M, g.K = K, g.N = N;
  g.msplit = M > 0 ? M : 1;
  g.pdiv = 1;
  return g;
}

const char* mix_reason(int64_t B, int Ci, int Co, int m1, int m2) {
  if (Ci < 1 || Ci > UNO_MAX_CH || Co < 1 || Co > UNO_MAX_CH) return "channels outside 1..512";
  if (m1 < 1 || m2 < 1 || m1 > UNO_MAX_DIM || m2 > UNO_MAX_DIM / 2 + 1) return "modes outside 1..512 rows, 1..257 columns";
  if (B < 0 || B * (int64_t)(Ci > Co ? Ci : Co) > UNO_MAX_PLANES) return "more than 65535 (image, channel) planes per call";
  return nullptr;
}

int launch_mix(const float* X, const float* w1, const float* w2, float* Y, int64_t B, int Ci, int Co, int m1, int m2, hipStream_t s) {
  const int Q = m1 * m2;
  const long xs = (long)Ci * 4 * Q, ys = (long)Co * 4 * Q;
  const dim3 grid((unsigned)(((long)Co * Q + 63) / 64), 2);
  for (int64_t b0 = 0; b0 < B; b0 += UNO_PASS) {
    const int nb = (int)((B - b0) < UNO_PASS ? (B - b0) : UNO_PASS);
    hipLaunchKernelGGL(uno_mix_kernel, grid, dim3(UNO_THREADS), 0, s, X + b0 * xs, (const float2*)w1, (const float2*)w2, Y + b0 * ys, nb, Ci, Co, Q, xs, ys);
    TANTE_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" int tante_uno_block_supported(int64_t B, int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int m1, int m2, int64_t x_stride,
                                         int64_t out_stride) {
  return uno_reason(B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, x_stride, out_stride) == nullptr ? 1 : 0;
}

extern "C" int64_t tante_uno_table_floats(int Hi, int Wi, int Ho, int Wo, int m1, int m2, int pointwise) {
  if (uno_reason(0, 1, 1, Hi, Wi, Ho, Wo, m1, m2, (int64_t)Hi * Wi, (int64_t)Ho * Wo)) return -1;
  return uno_plan(0, 1, 1, Hi, Wi, Ho, Wo, m1, m2, pointwise ? 1 : 0).t_total;
}

extern "C" int tante_uno_table_layout(int Hi, int Wi, int Ho, int Wo, int m1, int m2, int pointwise, int64_t* layout) {
  if (const char* why = uno_reason(0, 1, 1, Hi, Wi, Ho, Wo, m1, m2, (int64_t)Hi * Wi, (int64_t)Ho * Wo))
    TANTE_FAIL(-2, "tante_uno_table_layout: %s (%d x %d -> %d x %d, modes %d x %d)", why, Hi, Wi, Ho, Wo, m1, m2);
  if (!layout) TANTE_FAIL(-1, "tante_uno_table_layout: null argument");
  const UnoPlan p = uno_plan(0, 1, 1, Hi, Wi, Ho, Wo, m1, m2, pointwise ? 1 : 0);
  for (int t = 0; t < 5; ++t) {
    layout[3 * t] = p.t_off[t];
    layout[3 * t + 1] = p.t_rows[t];
    layout[3 * t + 2] = p.t_cols[t];
  }
  layout[15] = p.down;
  return 0;
}

extern "C" int64_t tante_uno_block_workspace_bytes(int64_t B, int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int m1, int m2, int pointwise) {
  if (uno_reason(B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, (int64_t)Ci * Hi * Wi, (int64_t)Co * Ho * Wo)) return -1;
  return (int64_t)sizeof(float) * uno_plan(B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, pointwise ? 1 : 0).w_total;
}

extern "C" int tante_uno_mode_mix_supported(int64_t B, int Ci, int Co, int m1, int m2) { return mix_reason(B, Ci, Co, m1, m2) == nullptr ? 1 : 0; }

extern "C" int tante_uno_mode_mix(const float* X, const float* w1, const float* w2, float* Y, int64_t B, int Ci, int Co, int m1, int m2, void* stream) {
  if (const char* why = mix_reason(B, Ci, Co, m1, m2))
    TANTE_FAIL(-2, "tante_uno_mode_mix: %s (B %lld, %d -> %d channels, modes %d x %d)", why, (long long)B, Ci, Co, m1, m2);
  if (!X || !w1 || !w2 || !Y) TANTE_FAIL(-1, "tante_uno_mode_mix: null argument");
  if ((uintptr_t)X % 4 || (uintptr_t)Y % 4 || (uintptr_t)w1 % 8 || (uintptr_t)w2 % 8)
    TANTE_FAIL(-2, "tante_uno_mode_mix: the spectra must be 4-byte and the weights 8-byte aligned");
  if (X == Y) TANTE_FAIL(-2, "tante_uno_mode_mix: Y may not alias X");
  if (B == 0) return 0;
  return launch_mix(X, w1, w2, Y, B, Ci, Co, m1, m2, (hipStream_t)stream);
}

extern "C" int tante_uno_block(const float* x, int64_t x_stride, int64_t B, int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int m1, int m2,
                               const float* tables, const float* w1, const float* w2, const float* pw_w, const float* pw_b, int act, float* out,
                               int64_t out_stride, void* work, int64_t work_bytes, void* stream) {
  if (const char* why = uno_reason(B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, x_stride, out_stride))
    TANTE_FAIL(-2, "tante_uno_block: %s (B %lld, %d -> %d channels, %d x %d -> %d x %d, modes %d x %d, strides %lld, %lld)", why, (long long)B, Ci, Co, Hi,
               Wi, Ho, Wo, m1, m2, (long long)x_stride, (long long)out_stride);
  if (act != TANTE_ACT_NONE && act != TANTE_ACT_GELU_ERF) TANTE_FAIL(-1, "tante_uno_block: the activation must be none or the erf GELU");
  if (!x || !tables || !w1 || !w2 || !out) TANTE_FAIL(-1, "tante_uno_block: null argument");
  if ((uintptr_t)x % 4 || (uintptr_t)out % 4 || (uintptr_t)tables % 4 || (uintptr_t)w1 % 8 || (uintptr_t)w2 % 8 || (pw_w && (uintptr_t)pw_w % 4) ||
      (pw_b && (uintptr_t)pw_b % 4))
    TANTE_FAIL(-2, "tante_uno_block: the tensors must be 4-byte and the spectral weights 8-byte aligned");
  if (B > 0) {
    const float* xe = x + (B - 1) * x_stride + (int64_t)Ci * Hi * Wi;
    const float* oe = out + (B - 1) * out_stride + (int64_t)Co * Ho * Wo;
    if (out < xe && x < oe) TANTE_FAIL(-2, "tante_uno_block: the output overlaps the input");
  }
  if (B == 0) return 0;
  const int pw = pw_w ? 1 : 0;
  const UnoPlan p = uno_plan(B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, pw);
  const int64_t need = (int64_t)sizeof(float) * p.w_total;
  if (!work || work_bytes < need) TANTE_FAIL(-1, "tante_uno_block: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  if ((uintptr_t)work % 16) TANTE_FAIL(-1, "tante_uno_block: the workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float* W = (float*)work;
  float *P1 = W + p.P1, *X = W + p.X, *S = W + p.S, *Y = W + p.Y, *UV = W + p.UV, *Z = W + p.Z;
  const int J = p.J, gelu = act == TANTE_ACT_GELU_ERF;
  const long inpl = (long)Hi * Wi, outpl = (long)Ho * Wo, p1pl = (long)p.M1 * Hi, xpl = 2l * J * m2, zpl = (long)Ho * p.ldz;
  int rc;
  {  // 1: the W-axis forward transform (and A_w) of every input row
    UnoGemm g = gemm_of(tables + p.t_off[0], p.M1, Wi, Hi);
    g.B = x, g.b_hi = x_stride, g.b_lo = inpl, g.pdiv = Ci, g.sk = 1, g.sn = Wi;
    g.D = P1, g.d_hi = Ci * p1pl, g.d_lo = p1pl, g.sm = Hi, g.sn_d = 1;
    if ((rc = launch_gemm(g, B * Ci, s))) return rc;
  }
  {  // 2: the H-axis forward transform at the kept rows, rows [Pr | Pi] of 2 Hi
    UnoGemm g = gemm_of(tables + p.t_off[1], 2 * J, 2 * Hi, m2);
    g.B = P1, g.b_hi = Ci * p1pl, g.b_lo = p1pl, g.pdiv = Ci, g.sk = 1, g.sn = 2 * Hi;
    g.D = X, g.d_hi = Ci * xpl, g.d_lo = xpl, g.sm = m2, g.sn_d = 1;
    if ((rc = launch_gemm(g, B * Ci, s))) return rc;
  }
  if (pw && p.down) {  // 3: S = A_h . R, R^T (Wo, Hi) behind the 2 m2 spectral rows of P1
    UnoGemm g = gemm_of(tables + p.t_off[2], Ho, Hi, Wo);
    g.B = P1 + 2l * m2 * Hi, g.b_hi = Ci * p1pl, g.b_lo = p1pl, g.pdiv = Ci, g.sk = 1, g.sn = Hi;
    g.D = S, g.d_hi = Ci * outpl, g.d_lo = outpl, g.sm = Wo, g.sn_d = 1;
    if ((rc = launch_gemm(g, B * Ci, s))) return rc;
  }
  if ((rc = launch_mix(X, w1, w2, Y, B, Ci, Co, m1, m2, s))) return rc;
  if (pw) {  // the 1 x 1 on the smaller grid: planes are images, K runs over the input channels
    const long pix = p.down ? outpl : inpl;
    UnoGemm g = gemm_of(pw_w, Co, Ci, (int)pix);
    g.B = p.down ? S : x, g.b_hi = p.down ? Ci * outpl : x_stride, g.b_lo = 0, g.pdiv = 1, g.sk = (int)pix, g.sn = 1;
    g.D = UV, g.d_hi = Co * pix, g.d_lo = 0, g.sm = (int)pix, g.sn_d = 1;
    if ((rc = launch_gemm(g, B, s))) return rc;
  }
  {  // the H-axis inverse: rows m = (ri, y) land at Zrow[y][ri m2 + l]
    UnoGemm g = gemm_of(tables + p.t_off[3], 2 * Ho, 2 * J, m2);
    g.B = Y, g.b_hi = Co * xpl, g.b_lo = xpl, g.pdiv = Co, g.sk = m2, g.sn = 1;
    g.D = Z, g.d_hi = Co * zpl, g.d_lo = zpl, g.msplit = Ho, g.sm = p.ldz, g.sm_hi = m2, g.sn_d = 1;
    if ((rc = launch_gemm(g, B * Co, s))) return rc;
  }
  if (pw && !p.down) {  // A_h . V beside the spectrum, columns 2 m2 .. of Zrow
    UnoGemm g = gemm_of(tables + p.t_off[2], Ho, Hi, Wi);
    g.B = UV, g.b_hi = Co * inpl, g.b_lo = inpl, g.pdiv = Co, g.sk = Wi, g.sn = 1;
    g.D = Z + 2 * m2, g.d_hi = Co * zpl, g.d_lo = zpl, g.sm = p.ldz, g.sn_d = 1;
    if ((rc = launch_gemm(g, B * Co, s))) return rc;
  }
  {  // the W-axis inverse (and A_w), the sum, the bias and the GELU
    UnoGemm g = gemm_of(tables + p.t_off[4], Wo, p.K5, Ho);
    g.B = Z, g.b_hi = Co * zpl, g.b_lo = zpl, g.pdiv = Co, g.sk = 1, g.sn = p.ldz;
    g.D = out, g.d_hi = out_stride, g.d_lo = outpl, g.sm = 1, g.sn_d = Wo;
    if (pw && p.down) g.add = UV, g.a_hi = Co * outpl, g.a_lo = outpl;
    g.bias = pw ? pw_b : nullptr;
    g.gelu = gelu;
    if ((rc = launch_gemm(g, B * Co, s))) return rc;
  }
  return 0;
}
