// Adaptive-step tail (bf16, deg=False inference): everything a call does after its last backbone, with the frame count decided on the
// device  (tante.py:145-176, 178-230).
//
//   tante_adaptive_rt    every order's step-size head in one entry: a 16-token tile per wave runs  C -> C/2 -> C/4 -> 1  on the matrix
//                        pipe (the intermediates stay MFMA accumulator tiles, re-packed to bf16 in registers as in the derivative head),
//                        clamps, and writes ONE partial sum per tile.  A second, tiny launch adds the partials of an image IN INDEX ORDER
//                        (no floating-point atomics: two runs give the same bits), forms r_k[b], R[b], count[b] = floor(R[b]) and the
//                        modifier FiLM rows a_k[b,:] = 1 + scale_k(r_k[b]), s_k[b,:] = shift_k(r_k[b]).
//   tante_head_adaptive  every order's derivative head and every frame's Taylor sum in one launch.  The body is the fused head kernel's
//                        (head_fused.hip: three transposed-conv stages chained through registers, the workgroup's whole weight stream
//                        resident in LDS) with two changes: the modifier FiLM is applied to the token rows as they are loaded (no d3
//                        tensor), and the number of frames written is read from `count` in device memory -- the host learns it later.
//
// Frame-count forms of the head kernel:
//   SUM  (n_cap == 1)  the orders' derivatives are summed in registers and the one frame is read and written once;
//   !SUM (n_cap <= 8)  the orders run in sequence and accumulate into the output frames by read-modify-write.  A workgroup owns its
//                      output pixels exclusively and the same lanes read what they wrote, in program order; order 0 starts from `last`.
#include "common.hip.h"
#include <stdlib.h>
#include <utility>

namespace {

template <class F, int... Is>
__device__ __forceinline__ void sfor_impl(F&& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void sfor(F&& f) { sfor_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{}); }

__device__ __forceinline__ u32x4 hpack8(const f32x4& a, const f32x4& b) {
  u32x4 f;
  f[0] = pack_bf16x2(a[0], a[1]); f[1] = pack_bf16x2(a[2], a[3]); f[2] = pack_bf16x2(b[0], b[1]); f[3] = pack_bf16x2(b[2], b[3]);
  return f;
}
__device__ __forceinline__ f32x4 hmfma(const u32x4& a, const u32x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 gelu4(const f32x4& v) { return gelu_poly4<false>(v); }
__device__ __forceinline__ f32x4 relu4(const f32x4& v) { return __builtin_elementwise_max(v, f32x4{0.f, 0.f, 0.f, 0.f}); }
template <int NWV>
__device__ __forceinline__ void hglds(const char* __restrict__ g, char* l, int bytes, int tid) {   // 1 KiB per wave pass
  const int wave = tid >> 6, lane = tid & 63;
  for (int off = wave * 1024; off < bytes; off += NWV * 1024)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + off + lane * 16),
                                     (__attribute__((address_space(3))) void*)(l + off), 16, 0, 0);
}

constexpr int HB = 1024;   // bias block bytes per tile (one LDS-DMA pass)

__device__ __forceinline__ int hkperm(int p) {   // position p of a k-permuted row holds source feature c (head_fused.hip)
  const int blk = p >> 5, qq = p & 31, kk = qq >> 3, dt = (qq >> 2) & 1, r = qq & 3;
  return blk * 32 + dt * 16 + kk * 4 + r;
}

// The wave's 16 token rows -> B-operand k-blocks in accumulator (k-permuted) order, through a private LDS piece `xs` (16 rows x 32 CB bf16);
// the fused head kernel's row-form loads.  FILM: row * fa + fs (one FiLM row for the tile: its 16 tokens lie in one image).
template <int CB, bool FILM>
__device__ __forceinline__ void load_rows(const float* __restrict__ Xp, unsigned row0, unsigned n_rows, int r_n0, long r_s1, long r_s0, long r_off,
                                          const float* __restrict__ fa, const float* __restrict__ fs, char* xs, int lane, bool live, u32x4 (&xf)[CB]) {
  static_assert(CB == 8 || CB == 4, "a token row is CB * 128 bytes: one or half a 64-lane instruction");
  constexpr int LPR = CB * 8;                       // lanes per token row (16 bytes each)
  constexpr int RPI = 64 / LPR;                     // rows per instruction
  const int kk = lane >> 4, l15 = lane & 15;
  const unsigned aq0 = row0 / (unsigned)r_n0, ar0 = row0 - aq0 * (unsigned)r_n0;
  auto row_offset = [&](int j) {                    // row0 + j -> element offset of its token row
    long q = aq0; int rem = (int)ar0 + j;
    while (rem >= r_n0) { rem -= r_n0; ++q; }
    return q * r_s1 + (long)rem * r_s0 + r_off;
  };
  f32x4 xraw[16 / RPI];
  f32x4 av = f32x4{1.f, 1.f, 1.f, 1.f}, sv = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (FILM) {
    av = *(const f32x4*)(fa + 4 * (lane % LPR));
    sv = *(const f32x4*)(fs + 4 * (lane % LPR));
  }
#pragma unroll
  for (int j = 0; j < 16 / RPI; ++j) {
    const int rj = RPI * j + lane / LPR;
    const long eo = row0 + (unsigned)rj < n_rows ? row_offset(rj) : r_off;      // dead rows read row 0 of the view (valid memory)
    xraw[j] = *(const f32x4*)(Xp + eo + 4 * (lane % LPR));
  }
#pragma unroll
  for (int j = 0; j < 16 / RPI; ++j) {
    const int rj = RPI * j + lane / LPR, c = lane % LPR;
    f32x4 v = xraw[j];
    if constexpr (FILM) v = v * av + sv;
    u32x2 u;
    u[0] = pack_bf16x2(v[0], v[1]); u[1] = pack_bf16x2(v[2], v[3]);
    *(u32x2*)(xs + rj * (CB * 64) + ((c ^ ((2 * rj) & (LPR - 1))) << 3)) = u;
  }
#pragma unroll
  for (int b = 0; b < CB; ++b) {      // k-block b: features 32 b + 4 kk .. + 3 and 32 b + 16 + 4 kk .. + 3  = 8-byte chunks 8 b + kk, 8 b + 4 + kk
    const u32x2 lo = *(const u32x2*)(xs + l15 * (CB * 64) + (((8 * b + kk) ^ ((2 * l15) & (LPR - 1))) << 3));
    const u32x2 hi = *(const u32x2*)(xs + l15 * (CB * 64) + (((8 * b + 4 + kk) ^ ((2 * l15) & (LPR - 1))) << 3));
    xf[b] = live ? u32x4{lo[0], lo[1], hi[0], hi[1]} : u32x4{0u, 0u, 0u, 0u};
  }
}

// ===== step-size heads ===========================================================================================================
// stream of one interprator:  [W1 (C/2 rows, k-permuted, swizzled) | b1] [W2 (C/4 rows) | b2] [w3 (C/4 floats, bf16 values) , b3 at float 128]
template <int CB>
struct RtGeom {
  static constexpr int C = 32 * CB, C1 = C / 2, C2 = C / 4;
  static constexpr int CPR1 = CB * 4, CPR2 = CB * 2;
  static constexpr int NS1 = C1 / 16, NS2 = C2 / 16, KB2 = C1 / 32;
  static constexpr int T1 = C1 * CPR1 * 16 + HB, T2 = C2 * CPR2 * 16 + HB, T3 = HB;
  static constexpr int STREAM = T1 + T2 + T3;
  static constexpr int NWV = 4;
  static constexpr int XS = NWV * 16 * CB * 64;
  static constexpr int LDS = STREAM + XS;            // C = 256: 83 + 32 KiB
};

struct RtArgs {
  const float *x0, *x1, *x2, *x3;      // token rows of each order, all addressed by (a_n0, a_s1, a_s0, a_off)
  const char *w0, *w1, *w2, *w3;       // each order's stream
  long a_s1, a_s0, a_off; int a_n0;
  int n_tiles;                         // 16-token tiles = n_img * Hp * Wp / 16
  float hi;                            // out_T - 1
  float* part;                         // (n_ord, n_tiles) clamped-token sums
};

template <int CB>
__global__ __launch_bounds__(256, 1) void adaptive_rt_kernel(const RtArgs A) {
  using G = RtGeom<CB>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* w1s = smem;
  char* w2s = smem + G::T1;
  const float* w3s = (const float*)(smem + G::T1 + G::T2);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, l15 = lane & 15;
  const int ord = blockIdx.y;
  const float* Xp = ord == 0 ? A.x0 : ord == 1 ? A.x1 : ord == 2 ? A.x2 : A.x3;
  const char* Wp = ord == 0 ? A.w0 : ord == 1 ? A.w1 : ord == 2 ? A.w2 : A.w3;
  hglds<G::NWV>(Wp, smem, G::STREAM, tid);
  const int tile = __builtin_amdgcn_readfirstlane(blockIdx.x * G::NWV + wave);
  const bool live = tile < A.n_tiles;                                  // wave-uniform: whole tiles only
  const unsigned n_rows = (unsigned)A.n_tiles * 16u;
  const unsigned row0 = live ? (unsigned)tile * 16u : 0u;              // a dead wave reads tile 0 (valid memory) and writes nothing
  u32x4 xf[CB];
  load_rows<CB, false>(Xp, row0, n_rows, A.a_n0, A.a_s1, A.a_s0, A.a_off, nullptr, nullptr, smem + G::STREAM + wave * (16 * CB * 64), lane, true, xf);
  int xo1[CB], xo2[G::KB2];
#pragma unroll
  for (int b = 0; b < CB; ++b) xo1[b] = swz_chunk(l15, b * 4 + kk, G::CPR1) << 4;
#pragma unroll
  for (int b = 0; b < G::KB2; ++b) xo2[b] = swz_chunk(l15, b * 4 + kk, G::CPR2) << 4;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's share of the stream has landed ...
  __syncthreads();                                      // ... and so has everybody else's
  // ---- C -> C/2, relu (bf16 out, as the GEMM chain stores it) ----
  u32x4 h1[G::KB2];
  {
    const float* bias1 = (const float*)(w1s + G::C1 * G::CPR1 * 16);
    f32x4 acc[G::NS1];
#pragma unroll
    for (int ns = 0; ns < G::NS1; ++ns) acc[ns] = *(const f32x4*)(bias1 + ns * 16 + kk * 4);
#pragma unroll
    for (int b = 0; b < CB; ++b)
#pragma unroll
      for (int ns = 0; ns < G::NS1; ++ns) acc[ns] = hmfma(*(const u32x4*)(w1s + (ns * 16 + l15) * G::CPR1 * 16 + xo1[b]), xf[b], acc[ns]);
#pragma unroll
    for (int b = 0; b < G::KB2; ++b) h1[b] = hpack8(relu4(acc[2 * b]), relu4(acc[2 * b + 1]));
  }
  // ---- C/2 -> C/4, relu (bf16), then the dot with w3: lane (kk, l15) holds channels 16 ns + 4 kk + r of token l15 ----
  float s = 0.f;
  {
    const float* bias2 = (const float*)(w2s + G::C2 * G::CPR2 * 16);
    f32x4 acc2[G::NS2];
#pragma unroll
    for (int ns = 0; ns < G::NS2; ++ns) acc2[ns] = *(const f32x4*)(bias2 + ns * 16 + kk * 4);
#pragma unroll
    for (int b = 0; b < G::KB2; ++b)
#pragma unroll
      for (int ns = 0; ns < G::NS2; ++ns) acc2[ns] = hmfma(*(const u32x4*)(w2s + (ns * 16 + l15) * G::CPR2 * 16 + xo2[b]), h1[b], acc2[ns]);
#pragma unroll
    for (int ns = 0; ns < G::NS2; ++ns) {
      const f32x4 h = relu4(acc2[ns]);
      const unsigned u0 = pack_bf16x2(h[0], h[1]), u1 = pack_bf16x2(h[2], h[3]);
      const f32x4 w = *(const f32x4*)(w3s + ns * 16 + kk * 4);
      s += bf16_lo(u0) * w[0];
      s += bf16_hi(u0) * w[1];
      s += bf16_lo(u1) * w[2];
      s += bf16_hi(u1) * w[3];
    }
  }
  s += __shfl_xor(s, 16);
  s += __shfl_xor(s, 32);                              // every lane: token l15's scalar
  const float t = s + w3s[128];
  // t + relu(-t) - relu(t - hi): forward value of the straight-through clamp (tante.py:196-198), as rt_reduce_kernel writes it
  float c = t + fmaxf(-t, 0.0f) - fmaxf(t - A.hi, 0.0f);
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) c += __shfl_xor(c, o);      // the tile's 16 tokens, a fixed butterfly
  if (live && lane == 0) A.part[(long)ord * A.n_tiles + tile] = c;
}

// r_k[b] = (sum of image b's tile partials, in index order) / HW + ep;  R[b] = mean_k r_k[b];  count[b] = floor(R[b]);
// the modifier's FiLM rows of (k, b) by the expression of film_table_kernel (pointwise.hip).  grid (n_img, n_ord), C threads.
// film: per order [sc_w0 | sc_b0 | sc_w2 | sc_b2 | sh_w0 | sh_b0 | sh_w2 | sh_b2] fp32, orders back to back.
__global__ __launch_bounds__(256) void adaptive_finish_kernel(const float* __restrict__ part, int n_ord, int n_img, int tpi, float ep, int C,
                                                              const float* __restrict__ film, float* __restrict__ r, float* __restrict__ R,
                                                              int* __restrict__ count, float* __restrict__ film_a, float* __restrict__ film_s) {
  __shared__ float rs[4];
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  if (tid < n_ord) {
    const float* p = part + ((long)tid * n_img + b) * tpi;
    float s = 0.0f;
    for (int i = 0; i < tpi; ++i) s += p[i];
    rs[tid] = s / (float)(tpi * 16) + ep;
  }
  __syncthreads();
  if (tid == 0) {
    r[k * n_img + b] = rs[k];
    if (k == 0) {
      double m = 0.0;
      for (int j = 0; j < n_ord; ++j) m += (double)rs[j];
      const float Rv = (float)(m / (double)n_ord);
      R[b] = Rv;
      count[b] = (int)floorf(Rv);
    }
  }
  if (tid >= C) return;
  const int Hd = C / 2, c = tid;
  const float* f = film + (long)k * (2L * (2 * Hd + (long)C * Hd + C));
  const float *sc_w0 = f, *sc_b0 = sc_w0 + Hd, *sc_w2 = sc_b0 + Hd, *sc_b2 = sc_w2 + (long)C * Hd;
  const float *sh_w0 = sc_b2 + C, *sh_b0 = sh_w0 + Hd, *sh_w2 = sh_b0 + Hd, *sh_b2 = sh_w2 + (long)C * Hd;
  const float tv = rs[k];
  float sa = sc_b2[c], sb = sh_b2[c];
  for (int j = 0; j < Hd; ++j) {
    sa += sc_w2[c * Hd + j] * fmaxf(sc_w0[j] * tv + sc_b0[j], 0.0f);
    sb += sh_w2[c * Hd + j] * fmaxf(sh_w0[j] * tv + sh_b0[j], 0.0f);
  }
  film_a[((long)k * n_img + b) * C + c] = 1.0f + sa;
  film_s[((long)k * n_img + b) * C + c] = sb;
}

// Linear weights (out, in) of the interprator -> its stream; one thread block per matrix tile (0: W1, 1: W2), block 2: w3 and b3
__global__ void pack_rt_stream_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                      const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3, int C,
                                      char* __restrict__ dst) {
  const int C1 = C / 2, C2 = C / 4;
  const int cpr1 = C / 8, cpr2 = C1 / 8;
  const long T1 = (long)C1 * cpr1 * 16 + HB, T2 = (long)C2 * cpr2 * 16 + HB;
  const int t = blockIdx.x;
  if (t == 2) {
    float* o = (float*)(dst + T1 + T2);
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
      float v = 0.f;
      if (i < C2) v = bf16_lo(pack_bf16x2(w3[i], 0.f));
      else if (i == 128) v = b3[0];
      o[i] = v;
    }
    return;
  }
  const float* w = t == 0 ? w1 : w2;
  const float* b = t == 0 ? b1 : b2;
  const int rows = t == 0 ? C1 : C2, cpr = t == 0 ? cpr1 : cpr2, K = t == 0 ? C : C1;
  char* base = t == 0 ? dst : dst + T1;
  for (int idx = threadIdx.x; idx < rows * cpr; idx += blockDim.x) {
    const int r = idx / cpr, c = idx % cpr;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = w[(long)r * K + hkperm(c * 8 + e)];
    u32x4 o;
    o[0] = pack_bf16x2(v[0], v[1]); o[1] = pack_bf16x2(v[2], v[3]); o[2] = pack_bf16x2(v[4], v[5]); o[3] = pack_bf16x2(v[6], v[7]);
    *((u32x4*)base + (long)r * cpr + swz_chunk(r, c, cpr)) = o;
  }
  float* bias = (float*)(base + (long)rows * cpr * 16);
  for (int r = threadIdx.x; r < 256; r += blockDim.x) bias[r] = r < rows ? b[r] : 0.f;
}

// ===== derivative heads + Taylor sums ============================================================================================
struct AHeadArgs {
  const float *xk0, *xk1, *xk2, *xk3;   // token rows of each order, all addressed by (a_n0, a_s1, a_s0, a_off)
  const char *wk0, *wk1, *wk2, *wk3;    // tante_pack_head streams: [W3 | bias3] [W1 tile p | bias1 p] x4 [W2 tile q | bias2 q] x4
  long a_s1, a_s0, a_off; int a_n0;
  int n_img, Hp, Wp, D, n_ord, n_cap, rule;
  const float* film_a; const float* film_s;   // (n_ord, n_img, C)
  const int* count;                     // (n_img): frames of image b = count[rule ? b : 0], held to [0, n_cap]
  const float* coef;                    // (n_ord, 8): (j dt)^(k+1) / (k+1)!, j = 1 .. 8
  float* out; long out_bstride;
  const float* last; long last_bstride;
  int groups;                           // token groups of 16 NWV
};

template <int CB>
struct HeadGeom {
  static constexpr int C = 32 * CB, C1 = C / 2, C2 = C / 4;
  static constexpr int CPR1 = CB * 4, CPR2 = CB * 2, CPR3 = CB;          // 16-byte chunks per row (K / 8)
  static constexpr int NS1 = C1 / 16, NS2 = C2 / 16;                     // 16-row sub-tiles
  static constexpr int KB2 = C1 / 32, KB3 = C2 / 32;                     // k-blocks of stages 2, 3
  static constexpr int T1 = C1 * CPR1 * 16 + HB, T2 = C2 * CPR2 * 16 + HB, T3 = 64 * CPR3 * 16 + HB;
  static constexpr int XS = 8 * 16 * CB * 64;                            // token-row staging of 8 waves (bf16), overlaid on the W2 tiles
  static constexpr int LDS = T3 + T1 + (4 * T2 > XS ? 4 * T2 : XS);      // C = 256: 9 + 65 + 4 x 17 = 142 KiB
};

// Work split as in fused_head_kernel: a workgroup owns 16 NWV tokens and one stage-1 pixel p, its whole weight stream resident in LDS.
template <int CB, int NWV, bool SUM>
__global__ __launch_bounds__(NWV * 64, 1) void head_adaptive_kernel(const AHeadArgs A) {
  using G = HeadGeom<CB>;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [W3 | bias3][W1 p | bias1 p][W2 q | bias2 q] x 4
  char* w3s = smem;
  char* w1s = smem + G::T3;
  char* w2s = smem + G::T3 + G::T1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, l15 = lane & 15;
  const int p = (blockIdx.x & 31) >> 3;                          // stage-1 pixel (kh, kw) = (p >> 1, p & 1)
  const int grp = (blockIdx.x >> 5) * 8 + (blockIdx.x & 7);
  if (grp >= A.groups) return;
  // the wave's 16 rows are consecutive and lie in ONE image (Hp Wp % 16 == 0): image, position and frame count are wave-uniform
  const int HW = A.Hp * A.Wp;
  const unsigned n_rows = (unsigned)A.n_img * (unsigned)HW;
  const unsigned row0 = (unsigned)__builtin_amdgcn_readfirstlane((grp * NWV + wave) * 16);
  const bool live = row0 < n_rows;
  const int img = live ? (int)(row0 / (unsigned)HW) : 0;
  const int hw = live ? (int)(row0 - (unsigned)img * (unsigned)HW) + l15 : 0;
  const int hp = (int)(((float)hw + 0.5f) * __builtin_amdgcn_rcpf((float)A.Wp)), wp = hw - hp * A.Wp;   // exact: hw < 2^22
  int nb = A.count[A.rule ? img : 0];                            // decided on the device by tante_adaptive_rt
  nb = nb < 0 ? 0 : (nb > A.n_cap ? A.n_cap : nb);
  nb = __builtin_amdgcn_readfirstlane(nb);
  const long frame = (long)A.D * (A.Hp * 8) * (A.Wp * 8);
  const int Wout = A.Wp * 8;
  auto pix_of = [&](int q, int ns) {
    const int y0 = hp * 8 + (p >> 1) * 4 + (q >> 1) * 2, x0 = wp * 8 + (p & 1) * 4 + (q & 1) * 2;
    return ((long)(4 * ns + kk) * (A.Hp * 8) + y0) * Wout + x0;
  };
  f32x4 dsum[SUM ? 4 : 1][4];        // SUM: sum over the orders of coefficient x derivative, per sub-pixel q and channel tile ns
  f32x4 pre[SUM ? 2 : 1][4][2];      // SUM: the frame values the epilogue adds to (fetched during the last order)
  if constexpr (SUM) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) dsum[q][ns] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto run_order = [&](auto is_last_c, const int ord) {
    constexpr bool IS_LAST = decltype(is_last_c)::value;
    // named fields: a run-time index into the kernel arguments would send the struct to scratch
    const float* Xp = ord == 0 ? A.xk0 : ord == 1 ? A.xk1 : ord == 2 ? A.xk2 : A.xk3;
    const char* Wp = ord == 0 ? A.wk0 : ord == 1 ? A.wk1 : ord == 2 ? A.wk2 : A.wk3;
    const float* coefp = A.coef + ord * 8;
    if (ord) __syncthreads();      // every wave is done with the previous order's weights before the DMA overwrites them
    hglds<NWV>(Wp + G::T3 + (long)p * G::T1, w1s, G::T1, tid);
    hglds<NWV>(Wp, w3s, G::T3, tid);
    u32x4 xf[CB];   // the token as B-operand k-blocks, accumulator (k-permuted) order; d_k = X_k * a_k[b] + s_k[b] applied on the way
    const long frow = ((long)ord * A.n_img + img) * G::C;
    load_rows<CB, true>(Xp, row0, n_rows, A.a_n0, A.a_s1, A.a_s0, A.a_off, A.film_a + frow, A.film_s + frow, w2s + wave * (16 * CB * 64), lane,
                        live, xf);
    __syncthreads();      // every wave has its fragments: the W2 tiles may land on the staging pieces
    hglds<NWV>(Wp + G::T3 + 4L * G::T1, w2s, 4 * G::T2, tid);
    int xo1[CB], xo2[G::KB2], xo3[G::KB3];
#pragma unroll
    for (int b = 0; b < CB; ++b) xo1[b] = swz_chunk(l15, b * 4 + kk, G::CPR1) << 4;
#pragma unroll
    for (int b = 0; b < G::KB2; ++b) xo2[b] = swz_chunk(l15, b * 4 + kk, G::CPR2) << 4;
#pragma unroll
    for (int b = 0; b < G::KB3; ++b) xo3[b] = swz_chunk(l15, b * 4 + kk, G::CPR3) << 4;
    if constexpr (SUM && IS_LAST)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ns = 0; ns < 4; ++ns)
          if (4 * ns < A.D && live && nb > 0 && 4 * ns + kk < A.D) {
            const float* lp = A.last + (long)img * A.last_bstride + pix_of(2 * j, ns);
            pre[j][ns][0] = *(const f32x4*)lp;
            pre[j][ns][1] = *(const f32x4*)(lp + Wout);
          }
    // W1 and W3 are complete here: every wave waited for its token rows, which it requested AFTER its share of the two tiles, before the
    // barrier above.  Stage 1 runs while the W2 tiles (and the SUM form's frame values) arrive.
    u32x4 h1[G::KB2];
    {
      const float* bias1 = (const float*)(w1s + G::C1 * G::CPR1 * 16);
      f32x4 acc[G::NS1];
#pragma unroll
      for (int ns = 0; ns < G::NS1; ++ns) acc[ns] = *(const f32x4*)(bias1 + ns * 16 + kk * 4);
#pragma unroll
      for (int b = 0; b < CB; ++b)
#pragma unroll
        for (int ns = 0; ns < G::NS1; ++ns) acc[ns] = hmfma(*(const u32x4*)(w1s + (ns * 16 + l15) * G::CPR1 * 16 + xo1[b]), xf[b], acc[ns]);
#pragma unroll
      for (int b = 0; b < G::KB2; ++b) h1[b] = hpack8(gelu4(acc[2 * b]), gelu4(acc[2 * b + 1]));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // ---- stages 2 + 3: sub-pixel tile q of W2, W3 ----
    const float* bias3 = (const float*)(w3s + 64 * G::CPR3 * 16);
    const float c_sum = coefp[0];
    f32x4 dl[4];
    sfor<4>([&](auto qc) {
      constexpr int q = decltype(qc)::value;           // sub-pixel (kh2, kw2) = (q >> 1, q & 1)
      const char* wt = w2s + q * G::T2;
      const float* bias2 = (const float*)(wt + G::C2 * G::CPR2 * 16);
      f32x4 acc2[G::NS2];
#pragma unroll
      for (int ns = 0; ns < G::NS2; ++ns) acc2[ns] = *(const f32x4*)(bias2 + ns * 16 + kk * 4);
#pragma unroll
      for (int b = 0; b < G::KB2; ++b)
#pragma unroll
        for (int ns = 0; ns < G::NS2; ++ns) acc2[ns] = hmfma(*(const u32x4*)(wt + (ns * 16 + l15) * G::CPR2 * 16 + xo2[b]), h1[b], acc2[ns]);
      u32x4 h2[G::KB3];
#pragma unroll
      for (int b = 0; b < G::KB3; ++b) h2[b] = hpack8(gelu4(acc2[2 * b]), gelu4(acc2[2 * b + 1]));
      // stage 3: rows n3 = (co, kh3, kw3) = 16 ns + 4 kk + r  ->  channel co = 4 ns + kk, r = (kh3, kw3)
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) {
        if (4 * ns < A.D) {   // uniform: this 16-row tile holds real channels
          f32x4 d = *(const f32x4*)(bias3 + ns * 16 + kk * 4);
#pragma unroll
          for (int b = 0; b < G::KB3; ++b) d = hmfma(*(const u32x4*)(w3s + (ns * 16 + l15) * G::CPR3 * 16 + xo3[b]), h2[b], d);
          if constexpr (SUM) {
            dsum[q][ns] += d * c_sum;                    // the frame is touched once, after the last order (below)
          } else if constexpr ((q & 1) == 0) {
            dl[ns] = d;                                  // left half of the pair: kept until its right neighbour exists
          } else if (live && 4 * ns + kk < A.D) {
            // sub-pixel pairs (q - 1, q are horizontal neighbours): 4 pixels = 16 bytes per row and instruction
            const long pix = pix_of(q - 1, ns);
            float* o0 = A.out + (long)img * A.out_bstride + pix;
            const float* l0 = A.last + (long)img * A.last_bstride + pix;
            const f32x4 t0 = f32x4{dl[ns][0], dl[ns][1], d[0], d[1]}, t1 = f32x4{dl[ns][2], dl[ns][3], d[2], d[3]};   // rows y0, y0 + 1
            for (int i = 0; i < nb; ++i) {               // frames past nb are not written
              float* o = o0 + (long)i * frame;
              const float* bp = ord == 0 ? l0 : o;       // order 0 starts from the last input frame, later orders accumulate
              const f32x4 r0 = *(const f32x4*)bp, r1 = *(const f32x4*)(bp + Wout);
              const float c = coefp[i];
              *(f32x4*)o = r0 + t0 * c;
              *(f32x4*)(o + Wout) = r1 + t1 * c;
            }
          }
        }
      }
    });
  };   // run_order
  if constexpr (SUM) {
    for (int ord = 0; ord + 1 < A.n_ord; ++ord) run_order(std::false_type{}, ord);
    run_order(std::true_type{}, A.n_ord - 1);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ns = 0; ns < 4; ++ns)
        if (4 * ns < A.D && live && nb > 0 && 4 * ns + kk < A.D) {
          float* o0 = A.out + (long)img * A.out_bstride + pix_of(2 * j, ns);
          const f32x4 dl_ = dsum[2 * j][ns], dr_ = dsum[2 * j + 1][ns];
          *(f32x4*)o0 = pre[j][ns][0] + f32x4{dl_[0], dl_[1], dr_[0], dr_[1]};
          *(f32x4*)(o0 + Wout) = pre[j][ns][1] + f32x4{dl_[2], dl_[3], dr_[2], dr_[3]};
        }
  } else {
    for (int ord = 0; ord < A.n_ord; ++ord) run_order(std::false_type{}, ord);
  }
}

template <int CB, int NWV, bool SUM>
void launch_ahead_nw(AHeadArgs A, hipStream_t s) {
  using G = HeadGeom<CB>;
  static TantePerDevice attr;
  attr.once([&] {
    (void)hipFuncSetAttribute((const void*)head_adaptive_kernel<CB, NWV, SUM>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS);
  });
  const long rows = (long)A.n_img * A.Hp * A.Wp;
  A.groups = (int)((rows + NWV * 16 - 1) / (NWV * 16));
  const unsigned grid = (unsigned)((A.groups + 7) / 8) * 32;   // 8 token groups x 4 pixels per 32 consecutive workgroups
  hipLaunchKernelGGL((head_adaptive_kernel<CB, NWV, SUM>), dim3(grid), dim3(NWV * 64), G::LDS, s, A);
}

template <int CB, bool SUM>
void launch_ahead(AHeadArgs A, hipStream_t s) {
  // 128-token groups (8 waves) once they still give every CU a workgroup; 64-token groups for small batches (as tante_head_fused)
  const long rows = (long)A.n_img * A.Hp * A.Wp;
  const int force = tante_opt("TANTE_HEAD_WAVES", 0);
  const bool wide = force ? force == 8 : rows >= 128 * 56;
  if (wide) launch_ahead_nw<CB, 8, SUM>(A, s);
  else launch_ahead_nw<CB, 4, SUM>(A, s);
}

template <int CB>
void launch_rt(const RtArgs& A, int n_ord, hipStream_t s) {
  using G = RtGeom<CB>;
  static TantePerDevice attr;
  attr.once([&] { (void)hipFuncSetAttribute((const void*)adaptive_rt_kernel<CB>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS); });
  hipLaunchKernelGGL((adaptive_rt_kernel<CB>), dim3((unsigned)((A.n_tiles + G::NWV - 1) / G::NWV), (unsigned)n_ord), dim3(G::NWV * 64), G::LDS, s, A);
}

int bad_rows(int32_t a_n0, int64_t a_s1, int64_t a_s0, int64_t a_off) { return a_n0 <= 0 || a_n0 % 16 || a_s1 % 4 || a_s0 % 4 || a_off % 4 || a_s1 < 0 || a_s0 < 0 || a_off < 0; }

}  // namespace

extern "C" int tante_adaptive_tail_supported(int C, int D, int Hp, int Wp, int n_ord, int n_cap) {
  return (C == 128 || C == 256) && D >= 1 && D <= 16 && Hp > 0 && Wp > 0 && ((long)Hp * Wp) % 16 == 0 && (long)Hp * Wp < (1L << 22) && n_ord >= 1 &&
         n_ord <= 4 && n_cap >= 1 && n_cap <= 8;
}

extern "C" int64_t tante_adaptive_rt_stream_bytes(int C) {
  const long C1 = C / 2, C2 = C / 4;
  return (C1 * (long)(C / 8) * 16 + HB) + (C2 * (C1 / 8) * 16 + HB) + HB;
}

extern "C" int64_t tante_adaptive_ws_bytes(int n_ord, int n_img, int Hp, int Wp) {
  if (n_ord < 1 || n_img < 1 || Hp < 1 || Wp < 1) return 0;
  return 4L * n_ord * (((long)n_img * Hp * Wp + 15) / 16);
}

extern "C" int tante_pack_adaptive_rt(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, int C,
                                      void* rt_stream, void* stream) {
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !rt_stream) TANTE_FAIL(-1, "tante_pack_adaptive_rt: null pointer");
  if (C != 128 && C != 256) TANTE_FAIL(-2, "tante_pack_adaptive_rt: unsupported C=%d", C);
  hipLaunchKernelGGL(pack_rt_stream_kernel, dim3(3), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, b2, w3, b3, C, (char*)rt_stream);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_adaptive_rt(int n_ord, const float* const* rows, const void* const* rt_streams, const float* film, int32_t a_n0, int64_t a_s1,
                                 int64_t a_s0, int64_t a_off, int n_img, int Hp, int Wp, int C, float out_T, float ep, void* ws, int64_t ws_bytes,
                                 float* r, float* R, int32_t* count, float* film_a, float* film_s, void* stream) {
  if (!rows || !rt_streams || !film || !ws || !r || !R || !count || !film_a || !film_s) TANTE_FAIL(-1, "tante_adaptive_rt: null pointer");
  if (!tante_adaptive_tail_supported(C, 1, Hp, Wp, n_ord, 1)) TANTE_FAIL(-2, "tante_adaptive_rt: unsupported C=%d Hp=%d Wp=%d n_ord=%d", C, Hp, Wp, n_ord);
  if (n_img <= 0 || (long)n_img * Hp * Wp >= (1L << 31)) TANTE_FAIL(-1, "tante_adaptive_rt: bad shape");
  if (bad_rows(a_n0, a_s1, a_s0, a_off)) TANTE_FAIL(-1, "tante_adaptive_rt: row addressing (a_n0 %% 16, strides %% 4, non-negative)");
  if (ws_bytes < tante_adaptive_ws_bytes(n_ord, n_img, Hp, Wp) || ((uintptr_t)ws % 4)) TANTE_FAIL(-1, "tante_adaptive_rt: workspace too small");
  if (((uintptr_t)film_a % 16) || ((uintptr_t)film_s % 16)) TANTE_FAIL(-1, "tante_adaptive_rt: alignment");
  for (int k = 0; k < n_ord; ++k)
    if (!rows[k] || !rt_streams[k] || ((uintptr_t)rows[k] % 16) || ((uintptr_t)rt_streams[k] % 16))
      TANTE_FAIL(-1, "tante_adaptive_rt: order %d: null or misaligned rows / stream", k);
  const float* xs[4] = {nullptr, nullptr, nullptr, nullptr};
  const char* wsm[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < n_ord; ++k) { xs[k] = rows[k]; wsm[k] = (const char*)rt_streams[k]; }
  RtArgs A;
  A.x0 = xs[0]; A.x1 = xs[1]; A.x2 = xs[2]; A.x3 = xs[3];
  A.w0 = wsm[0]; A.w1 = wsm[1]; A.w2 = wsm[2]; A.w3 = wsm[3];
  A.a_n0 = a_n0; A.a_s1 = a_s1; A.a_s0 = a_s0; A.a_off = a_off;
  const int tpi = Hp * Wp / 16;
  A.n_tiles = n_img * tpi;
  A.hi = out_T - 1.0f;
  A.part = (float*)ws;
  if (C == 128) launch_rt<4>(A, n_ord, (hipStream_t)stream);
  else launch_rt<8>(A, n_ord, (hipStream_t)stream);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(adaptive_finish_kernel, dim3((unsigned)n_img, (unsigned)n_ord), dim3(256), 0, (hipStream_t)stream, (const float*)ws, n_ord, n_img,
                     tpi, ep, C, film, r, R, count, film_a, film_s);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_head_adaptive(int n_ord, const float* const* rows, const void* const* head_streams, int32_t a_n0, int64_t a_s1, int64_t a_s0,
                                   int64_t a_off, int n_img, int Hp, int Wp, int C, int D, const float* film_a, const float* film_s,
                                   const int32_t* count, int rule, const float* coefs, int n_cap, float* out, int64_t out_bstride,
                                   const float* last, int64_t last_bstride, void* stream) {
  if (!rows || !head_streams || !film_a || !film_s || !count || !coefs || !out || !last) TANTE_FAIL(-1, "tante_head_adaptive: null pointer");
  if (!tante_adaptive_tail_supported(C, D, Hp, Wp, n_ord, n_cap))
    TANTE_FAIL(-2, "tante_head_adaptive: unsupported C=%d D=%d Hp=%d Wp=%d n_ord=%d n_cap=%d", C, D, Hp, Wp, n_ord, n_cap);
  if (n_img <= 0 || (long)n_img * Hp * Wp >= (1L << 31) || (rule != 0 && rule != 1)) TANTE_FAIL(-1, "tante_head_adaptive: bad shape");
  if (bad_rows(a_n0, a_s1, a_s0, a_off)) TANTE_FAIL(-1, "tante_head_adaptive: row addressing (a_n0 %% 16, strides %% 4, non-negative)");
  if (out_bstride % 4 || last_bstride % 4 || ((uintptr_t)out % 16) || ((uintptr_t)last % 16) || ((uintptr_t)film_a % 16) || ((uintptr_t)film_s % 16))
    TANTE_FAIL(-1, "tante_head_adaptive: alignment");
  for (int k = 0; k < n_ord; ++k)
    if (!rows[k] || !head_streams[k] || ((uintptr_t)rows[k] % 16) || ((uintptr_t)head_streams[k] % 16))
      TANTE_FAIL(-1, "tante_head_adaptive: order %d: null or misaligned rows / stream", k);
  const float* xs[4] = {nullptr, nullptr, nullptr, nullptr};
  const char* wsm[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < n_ord; ++k) { xs[k] = rows[k]; wsm[k] = (const char*)head_streams[k]; }
  AHeadArgs A;
  A.xk0 = xs[0]; A.xk1 = xs[1]; A.xk2 = xs[2]; A.xk3 = xs[3];
  A.wk0 = wsm[0]; A.wk1 = wsm[1]; A.wk2 = wsm[2]; A.wk3 = wsm[3];
  A.a_n0 = a_n0; A.a_s1 = a_s1; A.a_s0 = a_s0; A.a_off = a_off;
  A.n_img = n_img; A.Hp = Hp; A.Wp = Wp; A.D = D; A.n_ord = n_ord; A.n_cap = n_cap; A.rule = rule;
  A.film_a = film_a; A.film_s = film_s; A.count = count; A.coef = coefs;
  A.out = out; A.out_bstride = out_bstride; A.last = last; A.last_bstride = last_bstride;
  A.groups = 0;
  hipStream_t s = (hipStream_t)stream;
  if (C == 128) { if (n_cap == 1) launch_ahead<4, true>(A, s); else launch_ahead<4, false>(A, s); }
  else { if (n_cap == 1) launch_ahead<8, true>(A, s); else launch_ahead<8, false>(A, s); }
  TANTE_CHECK_LAUNCH();
  return 0;
}
