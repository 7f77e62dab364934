// Flash-style softmax attention over a TanteSeq of ANY length, forward and backward, on the matrix cores, with the causal mask and
// probability dropout (nn.MultiheadAttention(dropout = p) in train() mode: attn_backbone.py:47-48, 59-83; the axis letters of
// attn_backbone.py:148-189 are TanteSeq index arithmetic, as in attention.hip).  Head dim 32 (the shipped model's).
//
// Orientation (that of attn_fwd_mfma_kernel): every score tile is computed TRANSPOSED, S^T = K Q^T, so that a lane's column is one
// query (forward, dq pass) -- its running max / sum / lse / delta are per-lane scalars and the row reductions are two cross-group
// shuffles -- and the four accumulator registers are four consecutive keys: they pack straight into the B operand of the next product
// (O^T = V^T P^T, dQ^T = K^T dS^T), whose A operand is a transposing LDS read of the row-major K / V image.  The dk / dv pass swaps the
// roles (S = Q K^T: a lane's column is one KEY held in registers, the registers are four consecutive queries staged in LDS).
//
//   forward      one workgroup = 128 queries of one (sequence, head): 4 waves x 2 tiles of 16 queries; keys walk through LDS in tiles
//                of 64 (K and V row-major, 96-byte rows); online softmax in fp32 registers; key tiles above the causal diagonal are
//                skipped; writes per row  lse2 = max * c + log2(sum)  (c = log2(e) / sqrt(d)) to stats[row * 2]
//   backward Q   the same partition: delta = dO . O per query (written to stats[row * 2 + 1]), P = exp2(s c - lse2) recomputed,
//                dS = P (keep (dO . v) - delta), dQ^T += K^T dS^T
//   backward KV  one workgroup = 128 keys (4 waves x 2 tiles of 16; fp32: 64 keys, 1 tile) held in registers; queries (Q, dO, lse2,
//                delta) walk through LDS in tiles of 64 (fp32: 32), starting at the causal diagonal; dV^T += dO^T Pd, dK^T += Q^T dS
// dq, dk and dv are plain sums in a fixed order: no atomics, deterministic.
//
// Tile sizes.  The 16x16x32 bf16 MFMA fixes the 16-wide tiles and takes the whole head dim as its K.  Two query tiles per wave reuse
// every K / V fragment twice (the LDS reads, not the MFMAs, are the per-tile cost besides the softmax's VALU work) and keep the
// workgroup count at L / 128 per (sequence, head): 2048 workgroups at the shipped 'L' and 'A' geometries (B = 8), eight per CU.  A key
// tile of 64 is 12 KiB of LDS (bf16; 18 KiB fp32), so LDS never limits occupancy; registers do.  hipcc's resource report for gfx950
// (-Rpass-analysis=kernel-resource-usage; no scratch, no spills): bf16 forward 184 VGPRs (2 waves per SIMD), dq pass 122 (3), dk / dv
// pass 178 + 48 accumulator registers (2); fp32 forward 208, dq pass 158, dk / dv pass 130 -- the fp32 dk / dv pass holds one key tile
// and walks 32 queries to stay there; with two key tiles its fragments alone would be 224 registers.  The 96-byte (fp32: 144-byte) rows keep the
// transposing reads of the four 16-lane groups on different banks, as in attention.hip.
//
// The masked form (template parameter MASKED; the unmasked instantiations compile to the code they had): attn_mask / key_padding_mask as
// tante_attention_masked takes them, dense sequences only.  The kernels work on scores in the log2 domain (s c2), so a finite mask
// value enters as mask * log2(e); a -inf entry of either mask never enters a sum -- it makes the key INVALID, like the causal and
// kj < L tests (no -inf - (-inf) is ever formed).  lse2, the recomputed P of both backward passes and delta all include the mask; the
// dropout keep-mask index does not change; masks get no gradient.  Mask reads: a mask entry is used by exactly one lane, so an LDS image
// of the attn_mask tile would buy no reuse, only a second copy and a barrier -- the reads are direct.  In the query-stationary passes a
// lane reads four consecutive keys of its query's mask row (one 16-byte load when L % 4 == 0); over a 64-key tile the 16 lanes of a
// group cover 256 contiguous bytes of the row, two whole 128-byte lines.  The key-stationary pass reads a key column (dword loads; 16
// lanes cover 64 contiguous bytes of one mask row, and a wave's two key tiles share the line).  key_padding_mask IS reused by every
// query, so its 64 entries per key tile sit in LDS beside K / V (query-stationary) or in one register per key tile (key-stationary).
// The all-blocked-row rule is tante_attention_masked's: a query whose keys are all blocked gets o = 0 * (1 / 0) = NaN (torch's softmax
// of such a row), lse2 = -inf and delta = NaN; its dq is 0, and the key-stationary pass stages its Q / dO rows and statistics as zeros,
// so it adds nothing to dk and dv.  Resource report of the masked instantiations (no scratch, no spills): bf16 forward 182 VGPRs, dq
// pass 140, dk / dv pass 196 + 48; fp32 forward 214, dq pass 180, dk / dv pass 142 -- the occupancies of the unmasked forms.
//
// fp32 is the same structure on v_mfma_f32_16x16x4_f32 with scalar LDS fragment reads: exact fp32 products, not tuned.
// Inline assembly: the transposing LDS reads and the wait that covers them are ONE asm statement.
#include "common.hip.h"
#include "fused_common.hip.h"

namespace {

constexpr int FA_D = 32;
constexpr int FA_BK = 64;        // keys per LDS tile (forward, dq pass)
constexpr int FA_QT = 2;         // 16-query tiles per wave (forward, dq pass)
constexpr int FA_BQ = 4 * 16 * FA_QT;

__device__ __forceinline__ long fa_token(const TanteSeq& q, int s, int l) {
  return (long)(s / q.n_s0) * q.S1 + (long)(s % q.n_s0) * q.S0 + (long)(l / q.n_l0) * q.P1 + (long)(l % q.n_l0) * q.P0;
}

// the masked form addresses dense sequences only (token = s L + l): no descriptor arithmetic there
template <bool DENSE>
__device__ __forceinline__ long fa_tok(const TanteSeq& q, int s, int l) {
  if constexpr (DENSE) return (long)s * q.L + l;
  else return fa_token(q, s, l);
}

// ---- operand fragments, per dtype ------------------------------------------------------------------------------------------------
// Frag:  one 16-row tile x 32 dims as an MFMA A or B operand (row = lane & 15).  TFrag: 32 rows x 32 dims, transposed (output row = dim).
template <bool F32>
struct Fa;

template <>
struct Fa<false> {      // bf16
  typedef unsigned short elem;
  static constexpr int RS = 48;      // LDS row stride in elements (96 bytes)
  struct Frag { u32x4 a; };
  struct TFrag { u32x4 a[2]; };
  static __device__ __forceinline__ Frag zero_frag() { return Frag{u32x4{0u, 0u, 0u, 0u}}; }
  static __device__ __forceinline__ Frag from_global(const elem* row, int kk) { return Frag{*(const u32x4*)(row + kk * 8)}; }
  static __device__ __forceinline__ Frag from_lds(const elem* img, int row0, int l15, int kk) {
    return Frag{*(const u32x4*)(img + (row0 + l15) * RS + kk * 8)};
  }
  static __device__ __forceinline__ float dot(const Frag& x, const Frag& y) {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) d += bf16_lo(x.a[i]) * bf16_lo(y.a[i]) + bf16_hi(x.a[i]) * bf16_hi(y.a[i]);
    return d;
  }
  static __device__ __forceinline__ f32x4 mm(const Frag& a, const Frag& b, const f32x4& c) { return mfma_bf16(a.a, b.a, c); }
  // rows row0 .. row0 + 15 and row1 .. row1 + 15 of the image: k-step element j < 4 is row0 + 4 kk + j, j >= 4 is row1 + 4 kk + j - 4
  static __device__ __forceinline__ TFrag t_from_lds(const elem* img, int row0, int row1, int l15, int kk) {
    const char* base = (const char*)img + (4 * kk + (l15 >> 2)) * (RS * 2) + (l15 & 3) * 8;
    TFrag t;
    t.a[0] = lds_tr16_frag(base + row0 * (RS * 2), base + row1 * (RS * 2));
    t.a[1] = lds_tr16_frag(base + row0 * (RS * 2) + 32, base + row1 * (RS * 2) + 32);
    return t;
  }
  static __device__ __forceinline__ void mm_t(const TFrag& t, const f32x4& p0, const f32x4& p1, f32x4 (&acc)[2]) {
    const u32x4 pf = pack8(p0, p1);
    acc[0] = mfma_bf16(t.a[0], pf, acc[0]);
    acc[1] = mfma_bf16(t.a[1], pf, acc[1]);
  }
  // thread -> (row, 8-element chunk) of a staged tile: 4 threads per row
  static __device__ __forceinline__ void stage(elem* img, int row, int c, const elem* src) {
    *(u32x4*)(img + row * RS + c * 8) = src ? *(const u32x4*)(src + c * 8) : u32x4{0u, 0u, 0u, 0u};
  }
  // acc[dt][r] = value of dim dt * 16 + 4 kk + r
  static __device__ __forceinline__ void store(elem* row, int kk, const f32x4 (&acc)[2], float sc) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      u32x2 u;
      u[0] = pack_bf16x2(acc[dt][0] * sc, acc[dt][1] * sc);
      u[1] = pack_bf16x2(acc[dt][2] * sc, acc[dt][3] * sc);
      *(u32x2*)(row + dt * 16 + 4 * kk) = u;
    }
  }
};

template <>
struct Fa<true> {       // fp32: v_mfma_f32_16x16x4_f32, k-step i covers dims 4 i + kk
  typedef float elem;
  static constexpr int RS = 36;      // 144-byte rows
  struct Frag { float a[8]; };
  struct TFrag { float a[2][8]; };   // [dt][tile * 4 + r] = img[row_tile + 4 kk + r][dt * 16 + l15]
  static __device__ __forceinline__ Frag zero_frag() {
    Frag f;
#pragma unroll
    for (int i = 0; i < 8; ++i) f.a[i] = 0.f;
    return f;
  }
  static __device__ __forceinline__ Frag from_global(const elem* row, int kk) {
    Frag f;
#pragma unroll
    for (int i = 0; i < 8; ++i) f.a[i] = row[4 * i + kk];
    return f;
  }
  static __device__ __forceinline__ Frag from_lds(const elem* img, int row0, int l15, int kk) {
    Frag f;
#pragma unroll
    for (int i = 0; i < 8; ++i) f.a[i] = img[(row0 + l15) * RS + 4 * i + kk];
    return f;
  }
  static __device__ __forceinline__ float dot(const Frag& x, const Frag& y) {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) d += x.a[i] * y.a[i];
    return d;
  }
  static __device__ __forceinline__ f32x4 mm(const Frag& a, const Frag& b, f32x4 c) {
#pragma unroll
    for (int i = 0; i < 8; ++i) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.a[i], b.a[i], c, 0, 0, 0);
    return c;
  }
  static __device__ __forceinline__ TFrag t_from_lds(const elem* img, int row0, int row1, int l15, int kk) {
    TFrag t;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        t.a[dt][r] = img[(row0 + 4 * kk + r) * RS + dt * 16 + l15];
        t.a[dt][4 + r] = img[(row1 + 4 * kk + r) * RS + dt * 16 + l15];
      }
    return t;
  }
  static __device__ __forceinline__ void mm_t(const TFrag& t, const f32x4& p0, const f32x4& p1, f32x4 (&acc)[2]) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(t.a[dt][r], p0[r], acc[dt], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(t.a[dt][4 + r], p1[r], acc[dt], 0, 0, 0);
    }
  }
  static __device__ __forceinline__ void stage(elem* img, int row, int c, const elem* src) {
    const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
    *(f32x4*)(img + row * RS + c * 8) = src ? *(const f32x4*)(src + c * 8) : z;
    *(f32x4*)(img + row * RS + c * 8 + 4) = src ? *(const f32x4*)(src + c * 8 + 4) : z;
  }
  static __device__ __forceinline__ void store(elem* row, int kk, const f32x4 (&acc)[2], float sc) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
      *(f32x4*)(row + dt * 16 + 4 * kk) = f32x4{acc[dt][0] * sc, acc[dt][1] * sc, acc[dt][2] * sc, acc[dt][3] * sc};
  }
};

// keep-scale of the four consecutive keys kj0 .. kj0 + 3 of mask row `mrow` (kj0 % 4 == 0): 1 / (1 - p) or 0
__device__ __forceinline__ f32x4 fa_keep_keys(unsigned long long seed, unsigned long long mrow, int kj0, bool aligned, float p, float ksc) {
  f32x4 k;
  if (aligned) {
    const unsigned m4 = dropout_keep4(seed, mrow + (unsigned long long)kj0, p);
#pragma unroll
    for (int r = 0; r < 4; ++r) k[r] = ((m4 >> r) & 1u) ? ksc : 0.f;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) k[r] = dropout_keep(seed, mrow + (unsigned long long)(kj0 + r), p) ? ksc : 0.f;
  }
  return k;
}

// ---- the masked form ----------------------------------------------------------------------------------------------------------------
// nn.MultiheadAttention's attn_mask / key_padding_mask as tante_attention_masked takes them (additive fp32; -inf blocks a key), on DENSE
// sequences (token = s L + l).  The unmasked kernels carry an empty FaMask and none of this code.
template <bool MASKED>
struct FaMask {};
template <>
struct FaMask<true> {
  const float* am;      // (L, L) with bstride 0, or (nseq n_head, L, L) with bstride L L; may be null
  long bstride;
  const float* kpm;     // (nseq, L); may be null
};
constexpr float FA_LOG2E = 1.4426950408889634f;

// attn_mask entries of the keys kj0 .. kj0 + 3 (kj0 % 4 == 0) of one query's mask row: one 16-byte load when L % 4 == 0.  Addresses past
// the row's end are clamped into it: those keys are invalid whatever is read.
__device__ __forceinline__ f32x4 fa_mask_keys(const float* __restrict__ row, int kj0, int L, bool aligned) {
  if (aligned) return *(const f32x4*)(row + min(kj0, L - 4));
  f32x4 a;
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = row[min(kj0 + r, L - 1)];
  return a;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// grid = (ceil(L / 128) * nseq, n_head)
template <bool F32, bool MASKED>
__global__ __launch_bounds__(256) void attn_flash_fwd_kernel(const void* __restrict__ qkv_, void* __restrict__ o_, float* __restrict__ stats, int C,
                                                             int n_head, TanteSeq sq, int nqb, int causal, float c2, float p_drop,
                                                             unsigned long long seed, FaMask<MASKED> mk) {
  typedef Fa<F32> T;
  typedef typename T::elem elem;
  __shared__ __attribute__((aligned(16))) elem sm[2 * FA_BK * T::RS];
  __shared__ __attribute__((aligned(16))) float kps[MASKED ? FA_BK : 1];      // masked: the key tile's key_padding_mask * log2(e)
  const float cs = MASKED ? 1.0f : c2;      // masked: the scores are scaled when the mask is added, so the exponents take them as they are
  elem* Ks = sm;
  elem* Vs = sm + FA_BK * T::RS;
  const elem* qkv = (const elem*)qkv_;
  elem* o = (elem*)o_;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, l15 = lane & 15;
  const int s = blockIdx.x / nqb, qb = blockIdx.x - s * nqb, h = blockIdx.y;
  const int L = sq.L;
  const int q0 = qb * FA_BQ + wave * (16 * FA_QT);      // the wave's first query
  const bool aligned = (L & 3) == 0;
  const float ksc = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

  typename T::Frag qf[FA_QT];
  int qpos[FA_QT];
  bool qlive[FA_QT];
  long qtok[FA_QT];
  float m[FA_QT], lsum[FA_QT];
  f32x4 oa[FA_QT][2];
  const float* arow[FA_QT];      // masked: the query's attn_mask row
#pragma unroll
  for (int qt = 0; qt < FA_QT; ++qt) {
    qpos[qt] = q0 + qt * 16 + l15;
    qlive[qt] = qpos[qt] < L;
    qtok[qt] = qlive[qt] ? fa_tok<MASKED>(sq, s, qpos[qt]) : 0;
    qf[qt] = qlive[qt] ? T::from_global(qkv + qtok[qt] * 3L * C + h * FA_D, kk) : T::zero_frag();
    arow[qt] = nullptr;
    if constexpr (MASKED)
      if (mk.am) arow[qt] = mk.am + ((long)s * n_head + h) * mk.bstride + (long)min(qpos[qt], L - 1) * L;
    m[qt] = -INFINITY;
    lsum[qt] = 0.f;
    oa[qt][0] = oa[qt][1] = zero4;
  }
  const int k_end = causal ? min(L, (qb + 1) * FA_BQ) : L;      // workgroup-uniform
  const int wq_max = q0 + 16 * FA_QT - 1;
  const int srow = tid >> 2, sc4 = tid & 3;
  for (int k0 = 0; k0 < k_end; k0 += FA_BK) {
    __syncthreads();
    {
      const int kj = k0 + srow;
      const elem* src = kj < L ? qkv + fa_tok<MASKED>(sq, s, kj) * 3L * C + C + h * FA_D : nullptr;
      T::stage(Ks, srow, sc4, src);
      T::stage(Vs, srow, sc4, src ? src + C : nullptr);
      if constexpr (MASKED)
        if (tid < FA_BK) kps[tid] = (mk.kpm && k0 + tid < L) ? mk.kpm[(long)s * L + k0 + tid] * FA_LOG2E : 0.f;
    }
    __syncthreads();
    if (causal && k0 > wq_max) continue;      // wave-uniform: this wave's queries all precede the tile
    typename T::Frag kf[4];
    typename T::TFrag vt[2];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) kf[jt] = T::from_lds(Ks, jt * 16, l15, kk);
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) vt[jp] = T::t_from_lds(Vs, jp * 32, jp * 32 + 16, l15, kk);
#pragma unroll
    for (int qt = 0; qt < FA_QT; ++qt) {
      f32x4 st[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) st[jt] = T::mm(kf[jt], qf[qt], zero4);
      unsigned vm = 0;
      float mx = -INFINITY;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        f32x4 ma = zero4, mp = zero4;      // masked: attn_mask and key_padding_mask * log2(e) of the four keys
        if constexpr (MASKED) {
          if (arow[qt]) ma = fa_mask_keys(arow[qt], k0 + jt * 16 + 4 * kk, L, aligned);
          mp = *(const f32x4*)(kps + jt * 16 + 4 * kk);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kj = k0 + jt * 16 + 4 * kk + r;
          bool valid = qlive[qt] && kj < L && (!causal || kj <= qpos[qt]);
          if constexpr (MASKED) {
            const float add = ma[r] * FA_LOG2E + mp[r];
            valid = valid && add != -INFINITY;      // -inf never enters a sum: it makes the key invalid
            // an invalid key's score IS -inf from here on (the reference point mref below is finite, so its exponential is a plain 0):
            // no lane mask stays live across the softmax, which is what this form has no scalar registers for
            st[jt][r] = valid ? st[jt][r] * c2 + add : -INFINITY;
            mx = fmaxf(mx, st[jt][r]);
          } else {
            vm |= (unsigned)valid << (jt * 4 + r);
            if (valid) mx = fmaxf(mx, st[jt][r]);
          }
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m[qt], mx);
      const float mref = (mn == -INFINITY) ? 0.f : mn;
      const float corr = (m[qt] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m[qt] - mref) * cs);
      m[qt] = mn;
      float ls = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = (MASKED || ((vm >> (jt * 4 + r)) & 1)) ? __builtin_amdgcn_exp2f((st[jt][r] - mref) * cs) : 0.f;
          st[jt][r] = e;
          ls += e;
        }
      lsum[qt] = lsum[qt] * corr + ls;      // per-lane partial sums (the lane's keys): the normaliser sees the un-dropped probabilities
      if (p_drop > 0.f) {
        const unsigned long long mrow = (((unsigned long long)s * n_head + h) * L + qpos[qt]) * L;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
          const f32x4 kp = fa_keep_keys(seed, mrow, k0 + jt * 16 + 4 * kk, aligned, p_drop, ksc);
#pragma unroll
          for (int r = 0; r < 4; ++r) st[jt][r] *= kp[r];
        }
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) oa[qt][dt][r] *= corr;
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) T::mm_t(vt[jp], st[2 * jp], st[2 * jp + 1], oa[qt]);
    }
  }
#pragma unroll
  for (int qt = 0; qt < FA_QT; ++qt) {
    float l = lsum[qt];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (!qlive[qt]) continue;
    T::store(o + qtok[qt] * (long)C + h * FA_D, kk, oa[qt], 1.0f / l);
    if (stats && kk == 0) stats[(((long)s * n_head + h) * L + qpos[qt]) * 2] = m[qt] * cs + __builtin_amdgcn_logf(l);
  }
}

// ---- backward, query-stationary: delta and dq ----------------------------------------------------------------------------------------
template <bool F32, bool MASKED>
__global__ __launch_bounds__(256) void attn_flash_bwd_q_kernel(const void* __restrict__ qkv_, const void* __restrict__ o_, const void* __restrict__ do_,
                                                               float* __restrict__ stats, void* __restrict__ dqkv_, int C, int n_head, TanteSeq sq,
                                                               int nqb, int causal, float scale, float c2, float p_drop, unsigned long long seed,
                                                               FaMask<MASKED> mk) {
  typedef Fa<F32> T;
  typedef typename T::elem elem;
  __shared__ __attribute__((aligned(16))) elem sm[2 * FA_BK * T::RS];
  __shared__ __attribute__((aligned(16))) float kps[MASKED ? FA_BK : 1];
  elem* Ks = sm;
  elem* Vs = sm + FA_BK * T::RS;
  const elem* qkv = (const elem*)qkv_;
  const elem* o = (const elem*)o_;
  const elem* dO = (const elem*)do_;
  elem* dqkv = (elem*)dqkv_;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, l15 = lane & 15;
  const int s = blockIdx.x / nqb, qb = blockIdx.x - s * nqb, h = blockIdx.y;
  const int L = sq.L;
  const int q0 = qb * FA_BQ + wave * (16 * FA_QT);
  const bool aligned = (L & 3) == 0;
  const float ksc = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

  typename T::Frag qf[FA_QT], gf[FA_QT];
  int qpos[FA_QT];
  bool qlive[FA_QT];
  long qtok[FA_QT];
  float lse[FA_QT], delta[FA_QT];
  f32x4 dq[FA_QT][2];
  const float* arow[FA_QT];
#pragma unroll
  for (int qt = 0; qt < FA_QT; ++qt) {
    qpos[qt] = q0 + qt * 16 + l15;
    qlive[qt] = qpos[qt] < L;
    qtok[qt] = qlive[qt] ? fa_tok<MASKED>(sq, s, qpos[qt]) : 0;
    arow[qt] = nullptr;
    if constexpr (MASKED)
      if (mk.am) arow[qt] = mk.am + ((long)s * n_head + h) * mk.bstride + (long)min(qpos[qt], L - 1) * L;
    qf[qt] = gf[qt] = T::zero_frag();
    lse[qt] = 0.f;
    float d = 0.f;
    if (qlive[qt]) {
      qf[qt] = T::from_global(qkv + qtok[qt] * 3L * C + h * FA_D, kk);
      gf[qt] = T::from_global(dO + qtok[qt] * (long)C + h * FA_D, kk);
      d = T::dot(gf[qt], T::from_global(o + qtok[qt] * (long)C + h * FA_D, kk));
    }
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    delta[qt] = d;
    if (qlive[qt]) {
      float* st = stats + (((long)s * n_head + h) * L + qpos[qt]) * 2;
      lse[qt] = st[0];
      if (kk == 0) st[1] = d;
    }
    dq[qt][0] = dq[qt][1] = zero4;
  }
  const int k_end = causal ? min(L, (qb + 1) * FA_BQ) : L;
  const int wq_max = q0 + 16 * FA_QT - 1;
  const int srow = tid >> 2, sc4 = tid & 3;
  for (int k0 = 0; k0 < k_end; k0 += FA_BK) {
    __syncthreads();
    {
      const int kj = k0 + srow;
      const elem* src = kj < L ? qkv + fa_tok<MASKED>(sq, s, kj) * 3L * C + C + h * FA_D : nullptr;
      T::stage(Ks, srow, sc4, src);
      T::stage(Vs, srow, sc4, src ? src + C : nullptr);
      if constexpr (MASKED)
        if (tid < FA_BK) kps[tid] = (mk.kpm && k0 + tid < L) ? mk.kpm[(long)s * L + k0 + tid] * FA_LOG2E : 0.f;
    }
    __syncthreads();
    if (causal && k0 > wq_max) continue;
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {      // 32 keys at a time: fewer live fragments than the forward
      typename T::Frag kf[2], vf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        kf[j] = T::from_lds(Ks, jp * 32 + j * 16, l15, kk);
        vf[j] = T::from_lds(Vs, jp * 32 + j * 16, l15, kk);
      }
      const typename T::TFrag kt = T::t_from_lds(Ks, jp * 32, jp * 32 + 16, l15, kk);
#pragma unroll
      for (int qt = 0; qt < FA_QT; ++qt) {
        const unsigned long long mrow = (((unsigned long long)s * n_head + h) * L + qpos[qt]) * L;
        f32x4 ds[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 st = T::mm(kf[j], qf[qt], zero4);
          const f32x4 dp = T::mm(vf[j], gf[qt], zero4);
          const int kj0 = k0 + jp * 32 + j * 16 + 4 * kk;
          f32x4 kp = f32x4{1.f, 1.f, 1.f, 1.f};
          if (p_drop > 0.f) kp = fa_keep_keys(seed, mrow, kj0, aligned, p_drop, ksc);
          f32x4 ma = zero4, mp = zero4;      // masked: attn_mask and key_padding_mask * log2(e) of the four keys
          if constexpr (MASKED) {
            if (arow[qt]) ma = fa_mask_keys(arow[qt], kj0, L, aligned);
            mp = *(const f32x4*)(kps + jp * 32 + j * 16 + 4 * kk);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int kj = kj0 + r;
            bool valid = qlive[qt] && kj < L && (!causal || kj <= qpos[qt]);
            if constexpr (MASKED) {
              const float add = ma[r] * FA_LOG2E + mp[r];
              valid = valid && add != -INFINITY;
              const float p = valid ? __builtin_amdgcn_exp2f(st[r] * c2 + add - lse[qt]) : 0.f;
              ds[j][r] = valid ? p * (dp[r] * kp[r] - delta[qt]) : 0.f;      // a fully blocked row has delta = NaN (its o is): it gets dq = 0
            } else {
              const float p = valid ? __builtin_amdgcn_exp2f(st[r] * c2 - lse[qt]) : 0.f;
              ds[j][r] = p * (dp[r] * kp[r] - delta[qt]);
            }
          }
        }
        T::mm_t(kt, ds[0], ds[1], dq[qt]);
      }
    }
  }
#pragma unroll
  for (int qt = 0; qt < FA_QT; ++qt)
    if (qlive[qt]) T::store(dqkv + qtok[qt] * 3L * C + h * FA_D, kk, dq[qt], scale);
}

// ---- backward, key-stationary: dk and dv -------------------------------------------------------------------------------------------
// KT 16-key tiles per wave in registers, NI 16-query tiles per LDS tile.  grid = (ceil(L / (64 KT)) * nseq, n_head)
template <bool F32, int KT, int NI, bool MASKED>
__global__ __launch_bounds__(256) void attn_flash_bwd_kv_kernel(const void* __restrict__ qkv_, const void* __restrict__ do_,
                                                                const float* __restrict__ stats, void* __restrict__ dqkv_, int C, int n_head,
                                                                TanteSeq sq, int nkb, int causal, float scale, float c2, float p_drop,
                                                                unsigned long long seed, FaMask<MASKED> mk) {
  typedef Fa<F32> T;
  typedef typename T::elem elem;
  constexpr int BQ = NI * 16, BKW = 64 * KT;
  __shared__ __attribute__((aligned(16))) elem sm[2 * BQ * T::RS];
  __shared__ __attribute__((aligned(16))) float sst[2 * BQ];      // lse2 [BQ], delta [BQ]
  elem* Qs = sm;
  elem* Gs = sm + BQ * T::RS;
  const elem* qkv = (const elem*)qkv_;
  const elem* dO = (const elem*)do_;
  elem* dqkv = (elem*)dqkv_;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, l15 = lane & 15;
  const int s = blockIdx.x / nkb, kb = blockIdx.x - s * nkb, h = blockIdx.y;
  const int L = sq.L;
  const int kw0 = kb * BKW + wave * (16 * KT);      // the wave's first key
  const float ksc = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned long long mhead = ((unsigned long long)s * n_head + h) * L;

  typename T::Frag kf[KT], vf[KT];
  int kpos[KT];
  bool klive[KT];
  long ktok[KT];
  f32x4 dk[KT][2], dv[KT][2];
  float kadd[KT];      // masked: the key's key_padding_mask * log2(e); a key it blocks is not live
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    kpos[kt] = kw0 + kt * 16 + l15;
    klive[kt] = kpos[kt] < L;
    kadd[kt] = 0.f;
    ktok[kt] = klive[kt] ? fa_tok<MASKED>(sq, s, kpos[kt]) : 0;
    kf[kt] = vf[kt] = T::zero_frag();
    if (klive[kt]) {
      kf[kt] = T::from_global(qkv + ktok[kt] * 3L * C + C + h * FA_D, kk);
      vf[kt] = T::from_global(qkv + ktok[kt] * 3L * C + 2L * C + h * FA_D, kk);
    }
    dk[kt][0] = dk[kt][1] = dv[kt][0] = dv[kt][1] = zero4;
  }
  bool kopen[KT];      // masked: key_padding_mask leaves the key open
  const float* amh = nullptr;      // masked: this (sequence, head)'s attn_mask
  if constexpr (MASKED) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) kopen[kt] = true;
    if (mk.am) amh = mk.am + ((long)s * n_head + h) * mk.bstride;
    if (mk.kpm) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const float v = mk.kpm[(long)s * L + min(kpos[kt], L - 1)] * FA_LOG2E;
        kopen[kt] = v != -INFINITY;
        kadd[kt] = kopen[kt] ? v : 0.f;
      }
    }
  }
  const int i_start = causal ? (kb * BKW / BQ) * BQ : 0;      // workgroup-uniform: queries before the first key see none of these keys
  const int srow = tid >> 2, sc4 = tid & 3;
  for (int i0 = i_start; i0 < L; i0 += BQ) {
    __syncthreads();
    if (srow < BQ) {
      const int qi = i0 + srow;
      const long tok = qi < L ? fa_tok<MASKED>(sq, s, qi) : 0;
      bool qrow = qi < L;
      // masked: a query with every key blocked (lse2 = -inf; its o and delta are NaN) is staged as zeros, so it adds nothing to dk and dv
      if constexpr (MASKED) qrow = qrow && stats[(((long)s * n_head + h) * L + qi) * 2] != -INFINITY;
      T::stage(Qs, srow, sc4, qrow ? qkv + tok * 3L * C + h * FA_D : nullptr);
      T::stage(Gs, srow, sc4, qrow ? dO + tok * (long)C + h * FA_D : nullptr);
      if (sc4 < 2) sst[sc4 * BQ + srow] = qrow ? stats[(((long)s * n_head + h) * L + qi) * 2 + sc4] : 0.f;
    }
    __syncthreads();
    if (causal && i0 + BQ - 1 < kw0) continue;      // wave-uniform: every query of the tile precedes the wave's keys
#pragma unroll
    for (int ip = 0; ip < NI / 2; ++ip) {      // 32 queries at a time
      typename T::Frag qa[2], ga[2];
      f32x4 lse4[2], dl4[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        qa[j] = T::from_lds(Qs, ip * 32 + j * 16, l15, kk);
        ga[j] = T::from_lds(Gs, ip * 32 + j * 16, l15, kk);
        lse4[j] = *(const f32x4*)(sst + ip * 32 + j * 16 + 4 * kk);
        dl4[j] = *(const f32x4*)(sst + BQ + ip * 32 + j * 16 + 4 * kk);
      }
      const typename T::TFrag qT = T::t_from_lds(Qs, ip * 32, ip * 32 + 16, l15, kk);
      const typename T::TFrag gT = T::t_from_lds(Gs, ip * 32, ip * 32 + 16, l15, kk);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        f32x4 pd[2], ds[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 st = T::mm(qa[j], kf[kt], zero4);      // row = query 4 kk + r, column = key l15
          const f32x4 dp = T::mm(ga[j], vf[kt], zero4);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qi = i0 + ip * 32 + j * 16 + 4 * kk + r;
            bool valid = klive[kt] && qi < L && (!causal || kpos[kt] <= qi);
            float add = 0.f;
            if constexpr (MASKED) {
              valid = valid && kopen[kt];
              if (amh) {      // four consecutive queries of one key column: a strided read, clamped into the mask
                const float a = amh[(long)min(qi, L - 1) * L + min(kpos[kt], L - 1)];
                valid = valid && a != -INFINITY;
                add = a * FA_LOG2E;
              }
              add = valid ? add + kadd[kt] : 0.f;
            }
            const float p = valid ? __builtin_amdgcn_exp2f(MASKED ? st[r] * c2 + add - lse4[j][r] : st[r] * c2 - lse4[j][r]) : 0.f;
            float keep = 1.0f;
            if (p_drop > 0.f) keep = dropout_keep(seed, (mhead + (unsigned long long)qi) * L + (unsigned long long)kpos[kt], p_drop) ? ksc : 0.f;
            pd[j][r] = p * keep;
            ds[j][r] = p * (dp[r] * keep - dl4[j][r]);
          }
        }
        T::mm_t(gT, pd[0], pd[1], dv[kt]);
        T::mm_t(qT, ds[0], ds[1], dk[kt]);
      }
    }
  }
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
    if (klive[kt]) {
      T::store(dqkv + ktok[kt] * 3L * C + C + h * FA_D, kk, dk[kt], scale);
      T::store(dqkv + ktok[kt] * 3L * C + 2L * C + h * FA_D, kk, dv[kt], 1.0f);
    }
}

const char* flash_refusal(int dtype, int C, int n_head, int L) {
  if (dtype != TANTE_F32 && dtype != TANTE_BF16) return "dtype must be TANTE_F32 or TANTE_BF16";
  if (n_head <= 0 || C <= 0 || C % n_head) return "C must be a positive multiple of n_head";
  if (C / n_head != FA_D) return "head dim unsupported (supported: 32)";
  if (L < 1) return "empty sequence";
  return nullptr;
}

int flash_check(const char* who, int dtype, int C, int n_head, const TanteSeq* seq, float p_drop) {
  if (!seq) TANTE_FAIL(-1, "%s: null pointer", who);
  if (seq->nseq <= 0 || seq->L <= 0 || seq->n_s0 <= 0 || seq->n_l0 <= 0) TANTE_FAIL(-1, "%s: bad sequence descriptor", who);
  if (p_drop < 0.0f || p_drop >= 1.0f) TANTE_FAIL(-1, "%s: dropout probability must be in [0, 1)", who);
  if (const char* why = flash_refusal(dtype, C, n_head, seq->L))
    TANTE_FAIL(-2, "%s: %s (dtype=%d, C=%d, n_head=%d, head dim %d)", who, why, dtype, C, n_head, n_head > 0 ? C / n_head : 0);
  if (n_head > 65535) TANTE_FAIL(-2, "%s: too many heads for one launch", who);
  if ((long)seq->nseq * ((seq->L + 63) / 64) > 0x7fffffffL) TANTE_FAIL(-2, "%s: too many sequences for one launch", who);
  return 0;
}


// the launches behind both pairs of entry points; `who` names the entry point in every message
template <bool MASKED>
int flash_fwd(const char* who, const void* qkv, void* o, float* stats, int dtype, int C, int n_head, const TanteSeq* seq, int causal, float p_drop,
              uint64_t seed, FaMask<MASKED> mk, void* stream) {
  if (!qkv || !o) TANTE_FAIL(-1, "%s: null pointer", who);
  if (int rc = flash_check(who, dtype, C, n_head, seq, p_drop)) return rc;
  if (((uintptr_t)qkv % 16) || ((uintptr_t)o % 16) || ((uintptr_t)stats % 8)) TANTE_FAIL(-1, "%s: qkv and o must be 16-byte aligned, stats 8-byte aligned", who);
  const int nqb = (seq->L + FA_BQ - 1) / FA_BQ;
  const dim3 grid((unsigned)(nqb * seq->nseq), (unsigned)n_head);
  const float c2 = 1.4426950408889634f / sqrtf((float)FA_D);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TANTE_BF16)
    hipLaunchKernelGGL((attn_flash_fwd_kernel<false, MASKED>), grid, dim3(256), 0, s, qkv, o, stats, C, n_head, *seq, nqb, causal, c2, p_drop,
                       (unsigned long long)seed, mk);
  else
    hipLaunchKernelGGL((attn_flash_fwd_kernel<true, MASKED>), grid, dim3(256), 0, s, qkv, o, stats, C, n_head, *seq, nqb, causal, c2, p_drop,
                       (unsigned long long)seed, mk);
  TANTE_CHECK_LAUNCH();
  return 0;
}

template <bool MASKED>
int flash_bwd(const char* who, const void* qkv, const void* o, const void* dO, float* stats, void* dqkv, int dtype, int C, int n_head,
              const TanteSeq* seq, int causal, float p_drop, uint64_t seed, FaMask<MASKED> mk, void* stream) {
  if (!qkv || !o || !dO || !stats || !dqkv) TANTE_FAIL(-1, "%s: null pointer", who);
  if (int rc = flash_check(who, dtype, C, n_head, seq, p_drop)) return rc;
  if (((uintptr_t)qkv % 16) || ((uintptr_t)o % 16) || ((uintptr_t)dO % 16) || ((uintptr_t)dqkv % 16) || ((uintptr_t)stats % 8))
    TANTE_FAIL(-1, "%s: qkv, o, dO and dqkv must be 16-byte aligned, stats 8-byte aligned", who);
  const int nqb = (seq->L + FA_BQ - 1) / FA_BQ;
  const float scale = 1.0f / sqrtf((float)FA_D), c2 = 1.4426950408889634f * scale;
  hipStream_t s = (hipStream_t)stream;
  const dim3 gq((unsigned)(nqb * seq->nseq), (unsigned)n_head);
  if (dtype == TANTE_BF16) {
    const int nkb = (seq->L + 127) / 128;
    hipLaunchKernelGGL((attn_flash_bwd_q_kernel<false, MASKED>), gq, dim3(256), 0, s, qkv, o, dO, stats, dqkv, C, n_head, *seq, nqb, causal, scale, c2,
                       p_drop, (unsigned long long)seed, mk);
    hipLaunchKernelGGL((attn_flash_bwd_kv_kernel<false, 2, 4, MASKED>), dim3((unsigned)(nkb * seq->nseq), (unsigned)n_head), dim3(256), 0, s, qkv, dO,
                       (const float*)stats, dqkv, C, n_head, *seq, nkb, causal, scale, c2, p_drop, (unsigned long long)seed, mk);
  } else {
    const int nkb = (seq->L + 63) / 64;
    hipLaunchKernelGGL((attn_flash_bwd_q_kernel<true, MASKED>), gq, dim3(256), 0, s, qkv, o, dO, stats, dqkv, C, n_head, *seq, nqb, causal, scale, c2,
                       p_drop, (unsigned long long)seed, mk);
    hipLaunchKernelGGL((attn_flash_bwd_kv_kernel<true, 1, 2, MASKED>), dim3((unsigned)(nkb * seq->nseq), (unsigned)n_head), dim3(256), 0, s, qkv, dO,
                       (const float*)stats, dqkv, C, n_head, *seq, nkb, causal, scale, c2, p_drop, (unsigned long long)seed, mk);
  }
  TANTE_CHECK_LAUNCH();
  return 0;
}

// the dense descriptor (token = b L + l) and the mask arguments of the masked entry points
int flash_masked_args(const char* who, int Bp, int L, const float* attn_mask, int64_t mask_bstride, const float* key_padding_mask, TanteSeq* seq) {
  if (Bp <= 0 || L <= 0) TANTE_FAIL(-1, "%s: bad shape", who);
  if (attn_mask && mask_bstride != 0 && mask_bstride != (int64_t)L * L) TANTE_FAIL(-1, "%s: mask stride must be 0 (shared) or L * L", who);
  if (((uintptr_t)attn_mask % 16) || ((uintptr_t)key_padding_mask % 4)) TANTE_FAIL(-1, "%s: attn_mask must be 16-byte aligned, key_padding_mask 4-byte aligned", who);
  *seq = TanteSeq{Bp, L, 1, (int64_t)L, 0, L, 0, 1};
  return 0;
}

}  // namespace

extern "C" int64_t tante_attention_flash_stats_floats(int n_head, const TanteSeq* seq) {
  if (!seq || n_head <= 0 || seq->nseq <= 0 || seq->L <= 0) return 0;
  return (int64_t)seq->nseq * n_head * seq->L * 2;
}

extern "C" int tante_attention_flash_supported(int dtype, int C, int n_head, int L) { return flash_refusal(dtype, C, n_head, L) == nullptr; }

extern "C" int tante_attention_flash(const void* qkv, void* o, float* stats, int dtype, int C, int n_head, const TanteSeq* seq, int causal,
                                     float p_drop, uint64_t seed, void* stream) {
  return flash_fwd<false>("tante_attention_flash", qkv, o, stats, dtype, C, n_head, seq, causal, p_drop, seed, FaMask<false>{}, stream);
}

extern "C" int tante_attention_flash_bwd(const void* qkv, const void* o, const void* dO, float* stats, void* dqkv, int dtype, int C, int n_head,
                                         const TanteSeq* seq, int causal, float p_drop, uint64_t seed, void* stream) {
  return flash_bwd<false>("tante_attention_flash_bwd", qkv, o, dO, stats, dqkv, dtype, C, n_head, seq, causal, p_drop, seed, FaMask<false>{}, stream);
}

// With both masks NULL these ARE the unmasked kernels on the dense descriptor (the same bits); a mask selects the masked instantiations.
extern "C" int tante_attention_flash_masked(const void* qkv, void* o, float* stats, int dtype, int C, int n_head, int Bp, int L, int causal,
                                            const float* attn_mask, int64_t mask_bstride, const float* key_padding_mask, float p_drop, uint64_t seed,
                                            void* stream) {
  const char* who = "tante_attention_flash_masked";
  TanteSeq seq;
  if (int rc = flash_masked_args(who, Bp, L, attn_mask, mask_bstride, key_padding_mask, &seq)) return rc;
  if (!attn_mask && !key_padding_mask) return flash_fwd<false>(who, qkv, o, stats, dtype, C, n_head, &seq, causal, p_drop, seed, FaMask<false>{}, stream);
  return flash_fwd<true>(who, qkv, o, stats, dtype, C, n_head, &seq, causal, p_drop, seed, FaMask<true>{attn_mask, (long)mask_bstride, key_padding_mask},
                         stream);
}

extern "C" int tante_attention_flash_masked_bwd(const void* qkv, const void* o, const void* dO, float* stats, void* dqkv, int dtype, int C, int n_head,
                                                int Bp, int L, int causal, const float* attn_mask, int64_t mask_bstride,
                                                const float* key_padding_mask, float p_drop, uint64_t seed, void* stream) {
  const char* who = "tante_attention_flash_masked_bwd";
  TanteSeq seq;
  if (int rc = flash_masked_args(who, Bp, L, attn_mask, mask_bstride, key_padding_mask, &seq)) return rc;
  if (!attn_mask && !key_padding_mask)
    return flash_bwd<false>(who, qkv, o, dO, stats, dqkv, dtype, C, n_head, &seq, causal, p_drop, seed, FaMask<false>{}, stream);
  return flash_bwd<true>(who, qkv, o, dO, stats, dqkv, dtype, C, n_head, &seq, causal, p_drop, seed,
                         FaMask<true>{attn_mask, (long)mask_bstride, key_padding_mask}, stream);
}
