// Fused patch-embed stages 2 + 3 (bf16):  stage-1 image (channels-last bf16, C/4 channels) -> [Conv2d k = s = 2 -> GELU(erf)] ->
// [Conv2d k = s = 2] -> FiLM(t) + spatial / temporal embeddings -> the fp32 token stream   (enc_dec_cnn.py:221-229, tante.py:136-141).
//
// A token's value depends on its own 4 x 4 block of stage-1 pixels only.  A wave owns 16 tokens: for each of the token's 2 x 2
// stage-2 positions it loads the 2 x 2 x (C/4) input patch straight into MFMA B-operand fragments (16-byte runs of the channels-last
// image), multiplies by W2 (resident in LDS), applies GELU on the accumulators and packs them to bf16 -- which IS the matching
// k-block of stage 3's B operand (W3's columns are packed in accumulator order).  Stage 3 then streams W3 through a two-slot LDS
// ring in 32-row tiles and writes tokens with the FiLM + positional epilogue.  Against the two GEMM launches this replaces, the
// (n_img, H/4, W/4, C/2) intermediate (write + read) and one launch disappear.
#include "fused_common.hip.h"
#include <stdlib.h>

namespace {

constexpr int EHDR = 4096;   // stream header: bias2 (C/2 floats) then bias3 (C floats)

template <int CB>
struct EncGeom {
  static constexpr int C = 32 * CB, C1 = C / 4, C2 = C / 2;
  static constexpr int K2 = 4 * C1, K3 = 4 * C2;                 // contraction lengths (taps x channels)
  static constexpr int KB2 = K2 / 32, KB3 = K3 / 32;             // k-blocks
  static constexpr int NS2 = C2 / 16, BPT = C1 / 32;             // stage-2 16-row tiles; k-blocks per tap
  static constexpr int CPR2 = K2 / 8, CPR3 = K3 / 8;             // 16-byte chunks per weight row
  static constexpr int W2B = C2 * K2 * 2;                        // W2 image bytes
  static constexpr int T3ROWS = 32, T3B = T3ROWS * K3 * 2, NT3 = C / T3ROWS;   // stage-3 tiles
  static constexpr int LDS = EHDR + W2B + 2 * T3B;
  static_assert(C1 % 32 == 0, "stage-1 channels must fill whole k-blocks");
};

__device__ __forceinline__ void eglds(const char* __restrict__ g, char* l, int bytes, int tid) {   // 8 waves x 1 KiB per pass
  const int wave = tid >> 6, lane = tid & 63;
  for (int off = wave * 1024; off < bytes; off += 8192)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + off + lane * 16),
                                     (__attribute__((address_space(3))) void*)(l + off), 16, 0, 0);
}

// stage-1 stream (tante_pack_enc1_raw): [8 A fragments x 64 lanes x 16 B, rows in channel order][bias, padded to 1 KiB][the same
// fragments with the rows permuted for the one-launch form]
constexpr int E1C = 64, E1FRAGS = 8, E1PX = 256, E1BIAS = E1FRAGS * 1024, E1PERM = E1BIAS + 1024, E1BYTES = E1PERM + E1FRAGS * 1024;

// = nan_to_num_f of pointwise.hip (NaN -> 0, +-inf -> +-FLT_MAX), on the bit pattern: this file is compiled with -fno-honor-nans, under
// which `v != v` is false by decree
__device__ __forceinline__ float nan_to_num_raw(float v) {
  const unsigned u = __float_as_uint(v), a = u & 0x7fffffffu;
  return __uint_as_float(a > 0x7f800000u ? 0u : a == 0x7f800000u ? (u & 0x80000000u) | 0x7f7fffffu : u);
}

// what nan_to_num leaves of a value once it is rounded to a bf16 operand: +-FLT_MAX rounds to +-inf, so +-inf may stay what it is
__device__ __forceinline__ float nan_to_zero(float v) {
  return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u ? 0.0f : v;
}

struct EncArgs {
  const unsigned short* h1;   // (n_img, H1, W1, C1) bf16, H1 = 4 Hp, W1 = 4 Wp
  const char* w;              // [header][W2 image][W3 tiles]
  const float *film_a, *film_b, *s_emb;   // (T, C), (T, C), (Hp*Wp, C)
  float* out;                 // (n_img * Hp * Wp, C) fp32
  int n_img, Hp, Wp, T;
  // RAW form (the rollout's first window in one launch): stage 1 is computed here from the channels-last batch, h1 is unused
  const float* raw;           // (n_img, 8 Hp, 8 Wp, D) fp32
  const char* w1;             // stage-1 stream (its bias and permuted fragments are used)
  float* frame_out;           // image (b, out_frames - 1) -> frame_out + b * frame_bstride, (D, 8 Hp, 8 Wp), nan_to_num-ed
  long frame_bstride;
  int D;
  int out_frames;             // > 0: no FiLM; images are ordered (b, f), f < out_frames, and image (b, f) is written to the frame-major
                              // row block (f * (n_img / out_frames) + b) * Hp * Wp  (the rollout's pre-FiLM frame cache)
};

// SPLIT > 1 (small inputs, e.g. ONE frame per rollout call = 64 token groups for 256 CUs): the per-wave chain stage 2 -> 8 stage-3
// tiles is what the launch waits for, so SPLIT workgroups share a token group -- each repeats stage 2 (half of the work) and takes
// NT3 / SPLIT of the stage-3 tiles: per-wave work 2 -> 1 + 1 / SPLIT at SPLIT x the (idle) CUs.
template <int CB, int SPLIT, bool RAW = false>
__global__ __launch_bounds__(512, 2) void enc23_kernel(const EncArgs A) {
  using G = EncGeom<CB>;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [header][W2][slot 0][slot 1]
  char* w2s = smem + EHDR;
  char* slots = smem + EHDR + G::W2B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, l15 = lane & 15;
  eglds(A.w, smem, EHDR + G::W2B, tid);
  if constexpr (RAW) eglds(A.w1 + E1BIAS, smem + G::LDS, E1BYTES - E1BIAS, tid);   // [bias, 1 KiB][permuted stage-1 fragments]
  constexpr int NT3L = G::NT3 / SPLIT;                       // stage-3 tiles of this workgroup: t_first .. t_first + NT3L - 1
  const int t_first = (SPLIT > 1) ? (int)blockIdx.y * NT3L : 0;
  const char* w3 = A.w + EHDR + G::W2B + (long)t_first * G::T3B;

  const int HW = A.Hp * A.Wp;
  const long rows = (long)A.n_img * HW;
  const long row = ((long)blockIdx.x * 8 + wave) * 16 + l15;
  const bool live = row < rows;
  const long r = live ? row : 0;
  const unsigned r32 = (unsigned)r;      // rows < 2^31 (a row is 1 KiB of output): 32-bit divisions
  const int img = (int)(r32 / (unsigned)HW), hw = (int)(r32 - (unsigned)img * (unsigned)HW), hp = hw / A.Wp, wp = hw - hp * A.Wp;
  const int H1 = 4 * A.Hp, W1 = 4 * A.Wp;
  const unsigned short* base = A.h1 + (((long)img * H1 + 4 * hp) * W1 + 4 * wp) * G::C1;   // the token's 4 x 4 pixel block

  const int row2 = l15 * G::CPR2 * 16, row3 = l15 * G::CPR3 * 16;

  // input patch of position P as B-operand k-blocks: block b = tap (kh, kw) = b / BPT, channels 32 (b % BPT) + 8 kk .. + 7.
  // One register set: block b of the NEXT position is fetched into xin[b] right after this position's last MFMA on it.
  u32x4 xin[G::KB2];
  auto load_block = [&](int P, int b) {
    const int py = P >> 1, px = P & 1, tap = b / G::BPT, kh = tap >> 1, kw = tap & 1;
    const unsigned short* src = base + ((long)(2 * py + kh) * W1 + (2 * px + kw)) * G::C1 + 32 * (b % G::BPT) + 8 * kk;
    return live ? *(const u32x4*)src : u32x4{0u, 0u, 0u, 0u};
  };
  // RAW: the same blocks from the batch.  Tap (kh, kw) of position P is ONE stage-1 pixel of the token.  For a half position (P, kh) the
  // wave brings the two pixel rows x four pixels that its 16 tokens need -- 32 runs of 16 D bytes, 16 bytes per lane -- into its own
  // 8 KiB of the W3 ring (which is filled only after stage 2 in this form), gathers the 2 x 2 x D patches from there (k = 4 ci + 2 kh
  // + kw: lane kk holds ci = 2 (4 cb + kk), + 1; NaN -> 0 as it reads), runs the two k-steps against the permuted stage-1 weight, adds
  // the bias, applies GELU, and the accumulator pairs packed to bf16 ARE blocks 2 tap and 2 tap + 1.  Tokens of the last slot also
  // write the staged pixels out as their part of the cleaned channels-first frame.
  char* stg = slots + wave * 8192;
  long tok_off = 0;
  bool frame_tok = false;
  if constexpr (RAW) {
    tok_off = (((long)img * (8 * A.Hp) + 8 * hp) * (8 * A.Wp) + 8 * wp) * A.D;
    frame_tok = live && img % A.out_frames == A.out_frames - 1;
  }
  auto stage_half = [&](int P, int kh) {
    const int sy = 2 * (P >> 1) + kh, pxx = P & 1, Wr = 8 * A.Wp, D = A.D, nch = 32 * D;   // nch <= 512 chunks of 16 bytes
    const long in_tok = ((long)(2 * sy) * Wr + 4 * pxx) * D;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      u32x4 t[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * (2 * pass + j), run = min(c / D, 31), cc = c - run * D, tk = run >> 1, rr = run & 1;
        const unsigned lo = (unsigned)__shfl((int)(unsigned)(tok_off & 0xffffffffL), tk);
        const int hi = __shfl((int)(tok_off >> 32), tk), lv = __shfl((int)live, tk);
        const float* g = A.raw + (((long)hi << 32) | (long)lo) + in_tok + (long)rr * Wr * D + 4 * cc;
        t[j] = (c < nch && lv) ? *(const u32x4*)g : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * (2 * pass + j);
        if (c < nch) *(u32x4*)(stg + c * 16) = t[j];
      }
    }
    if (frame_tok) {
      const int Hr = 8 * A.Hp;
      float* fo = A.frame_out + (long)(img / A.out_frames) * A.frame_bstride + (long)(8 * hp + 2 * sy) * Wr + 8 * wp + 4 * pxx;
      for (int it = kk; it < 2 * D; it += 4) {
        const int d = it >> 1, rr = it & 1;
        const float* q = (const float*)stg + (l15 * 2 + rr) * 4 * D + d;
        *(f32x4*)(fo + ((long)d * Hr + rr) * Wr) = f32x4{nan_to_num_raw(q[0]), nan_to_num_raw(q[D]), nan_to_num_raw(q[2 * D]), nan_to_num_raw(q[3 * D])};
      }
    }
  };
  auto stage1_tap = [&](int kw, u32x4& b0, u32x4& b1) {
    const int D = A.D;
    const float* q0 = (const float*)stg + (l15 * 8 + 2 * kw) * D;
    u32x4 xf[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float x[8];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int ci = 2 * (cb * 4 + kk) + e;
        const bool ok = ci < D;                    // dead tokens were staged as zeros
        const float* q = q0 + ci;
        x[4 * e] = ok ? nan_to_zero(q[0]) : 0.0f;
        x[4 * e + 1] = ok ? nan_to_zero(q[D]) : 0.0f;
        x[4 * e + 2] = ok ? nan_to_zero(q[4 * D]) : 0.0f;
        x[4 * e + 3] = ok ? nan_to_zero(q[5 * D]) : 0.0f;
      }
      xf[cb][0] = pack_bf16x2(x[0], x[1]); xf[cb][1] = pack_bf16x2(x[2], x[3]);
      xf[cb][2] = pack_bf16x2(x[4], x[5]); xf[cb][3] = pack_bf16x2(x[6], x[7]);
    }
    const char* w1s = smem + G::LDS;
    auto tile = [&](int t) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = mfma_bf16(*((const u32x4*)(w1s + 1024) + (2 * t) * 64 + lane), xf[0], acc);
      acc = mfma_bf16(*((const u32x4*)(w1s + 1024) + (2 * t + 1) * 64 + lane), xf[1], acc);
      return gelu_poly4<false>(acc + *(const f32x4*)((const float*)w1s + 32 * (t >> 1) + 8 * kk + 4 * (t & 1)));
    };
    b0 = pack8(tile(0), tile(1));
    asm volatile("" : "+v"(b0));      // packed here, as in stage 2: the fp32 halves do not stay live
    b1 = pack8(tile(2), tile(3));
    asm volatile("" : "+v"(b1));
  };
  if constexpr (!RAW) {
#pragma unroll
    for (int b = 0; b < G::KB2; ++b) xin[b] = load_block(0, b);   // in flight together with the W2 image
  }

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if constexpr (!RAW) {
    eglds(w3, slots, G::T3B, tid);                  // stage-3 tiles 0 and 1 land while stage 2 computes
    eglds(w3 + G::T3B, slots + G::T3B, G::T3B, tid);
  }

  // ---- stage 2: the four positions P = (py, px); h2[P * NS2/2 + j] = stage-3 k-block (tap P, channels 32 j .. 32 j + 31) --------
  const float* bias2 = (const float*)smem;
  const float* bias3 = (const float*)smem + G::C2;
  u32x4 h2[G::KB3];
  unsigned bt2[G::KB2];
#pragma unroll
  for (int b = 0; b < G::KB2; ++b) bt2[b] = lds_addr(w2s + row2 + (swz_chunk(l15, b * 4 + kk, G::CPR2) << 4));
  static_for<4>([&](auto pc) {
    constexpr int P = decltype(pc)::value;
    if constexpr (RAW) {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        stage_half(P, kh);
        stage1_tap(0, xin[4 * kh], xin[4 * kh + 1]);
        stage1_tap(1, xin[4 * kh + 2], xin[4 * kh + 3]);
      }
    }
    static_for<2>([&](auto hc) {   // two halves of the C/2 outputs: 16 accumulator registers live instead of 32
      constexpr int hh = decltype(hc)::value, NH2 = G::NS2 / 2;
      f32x4 acc[NH2];
#pragma unroll
      for (int ns = 0; ns < NH2; ++ns) acc[ns] = *(const f32x4*)(bias2 + (hh * NH2 + ns) * 16 + kk * 4);
      mfma_stream<NH2 * G::KB2, 4, false>(
          [&](auto ic) { constexpr int i = decltype(ic)::value; return LdsAddr<(hh * NH2 + i % NH2) * 16 * G::CPR2 * 16>{bt2[i / NH2]}; },
          [&](auto ic, const u32x4& wf) {
            constexpr int i = decltype(ic)::value, ns = i % NH2, kb = i / NH2;
            acc[ns] = mfma_bf16(wf, xin[kb], acc[ns]);
            if constexpr (!RAW && hh == 1 && ns == NH2 - 1 && P < 3) xin[kb] = load_block(P + 1, kb);   // last use of block kb at this position
          });
#pragma unroll
      for (int j = 0; j < NH2 / 2; ++j) {
        u32x4 f = pack8(gelu_poly4<false>(acc[2 * j]), gelu_poly4<false>(acc[2 * j + 1]));
        asm volatile("" : "+v"(f));   // materialise the packed fragment HERE: otherwise the compiler keeps the fp32 halves (spilled) until stage 3
        h2[P * (G::NS2 / 2) + hh * (NH2 / 2) + j] = f;
      }
    });
  });

  if constexpr (RAW) {      // the ring was the waves' staging area until here
    __syncthreads();
    eglds(w3, slots, G::T3B, tid);
    eglds(w3 + G::T3B, slots + G::T3B, G::T3B, tid);
  }

  // ---- stage 3: 32 output features per W3 tile; FiLM + positional epilogue ------------------------------------------------------
  const int t_idx = img % A.T;
  const float* fa = A.film_a + (long)t_idx * G::C;
  const float* fb = A.film_b + (long)t_idx * G::C;
  const float* se = A.s_emb + (long)hw * G::C;
  const int nb = A.out_frames > 0 ? A.n_img / A.out_frames : 1;
  float* orow = A.out + (A.out_frames > 0 ? ((long)(img % A.out_frames) * nb + img / A.out_frames) * HW + hw : r) * G::C;
  unsigned bt3[G::KB3];   // slot-0 bases; the slot and row-tile offsets are instruction immediates
#pragma unroll
  for (int b = 0; b < G::KB3; ++b) bt3[b] = lds_addr(slots + row3 + (swz_chunk(l15, b * 4 + kk, G::CPR3) << 4));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  static_for<NT3L>([&](auto tc) {
    constexpr int t = decltype(tc)::value;             // local tile index (ring slot, prefetch distance); tg = its global index
    const int tg = t_first + t;
    f32x4 acc[2];
#pragma unroll
    for (int ns = 0; ns < 2; ++ns) acc[ns] = *(const f32x4*)(bias3 + tg * 32 + ns * 16 + kk * 4);
    mfma_stream<2 * G::KB3, 4, false>(
        [&](auto ic) { constexpr int i = decltype(ic)::value; return LdsAddr<(t & 1) * G::T3B + (i % 2) * 16 * G::CPR3 * 16>{bt3[i / 2]}; },
        [&](auto ic, const u32x4& wf) {
          constexpr int i = decltype(ic)::value, ns = i % 2, kb = i / 2;
          acc[ns] = mfma_bf16(wf, h2[kb], acc[ns]);
        });
    __syncthreads();                                   // every wave is done with slot t & 1
    if constexpr (t + 2 < NT3L) eglds(w3 + (long)(t + 2) * G::T3B, slots + (t & 1) * G::T3B, G::T3B, tid);
    if constexpr (t + 1 < NT3L) {
      // tile t + 1 was issued one tile ago: all but the pieces just issued for t + 2 must have landed.  (vmcnt counts loads, stores
      // and LDS-DMA together in issue order; the epilogue below comes AFTER this wait so its stores never sit in front of it.)
      if constexpr (t + 2 < NT3L) wait_vmcnt<G::T3B / 8192>();
      else wait_vmcnt<0>();
      __syncthreads();
    }
    if (live) {
#pragma unroll
      for (int ns = 0; ns < 2; ++ns) {
        const int n0 = tg * 32 + ns * 16 + kk * 4;
        const f32x4 a = *(const f32x4*)(fa + n0), b = *(const f32x4*)(fb + n0), sv = *(const f32x4*)(se + n0);
        *(f32x4*)(orow + n0) = A.out_frames > 0 ? acc[ns] : acc[ns] * a + b + sv;
      }
    }
  });
}

// position p inside a 32-block of a k-permuted row holds source channel c:  p = 8*kk + 4*dt + r  ->  c = 16*dt + 4*kk + r
__device__ __forceinline__ int ekperm(int p) {
  const int q = p & 31, kq = q >> 3, dt = (q >> 2) & 1, r = q & 3;
  return (p & ~31) + dt * 16 + kq * 4 + r;
}

// conv2 (C2, C1, 2, 2) -> W2 image rows n, k = (kh, kw, ci);  conv3 (C, C2, 2, 2) -> tiles of 32 rows, k = (tap, c2 permuted in 32-blocks)
__global__ void pack_enc_stream_kernel(const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
                                       const float* __restrict__ b3, int C, char* __restrict__ dst) {
  const int C1 = C / 4, C2 = C / 2, K2 = 4 * C1, K3 = 4 * C2, cpr2 = K2 / 8, cpr3 = K3 / 8;
  const long W2B = (long)C2 * K2 * 2;
  const int part = blockIdx.y;
  if (part == 0) {          // header
    float* h = (float*)dst;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < EHDR / 4; i += gridDim.x * blockDim.x)
      h[i] = i < C2 ? b2[i] : (i < C2 + C ? b3[i - C2] : 0.0f);
  } else if (part == 1) {   // W2
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < (long)C2 * cpr2; idx += (long)gridDim.x * blockDim.x) {
      const int n = (int)(idx / cpr2), c = (int)(idx % cpr2);
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = c * 8 + e, tap = k / C1, ci = k % C1;
        v[e] = w2[(((long)n * C1 + ci) * 2 + (tap >> 1)) * 2 + (tap & 1)];
      }
      u32x4 o;
      o[0] = pack_bf16x2(v[0], v[1]); o[1] = pack_bf16x2(v[2], v[3]); o[2] = pack_bf16x2(v[4], v[5]); o[3] = pack_bf16x2(v[6], v[7]);
      *((u32x4*)(dst + EHDR) + (long)n * cpr2 + swz_chunk(n, c, cpr2)) = o;
    }
  } else {                  // W3 tiles
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < (long)C * cpr3; idx += (long)gridDim.x * blockDim.x) {
      const int n = (int)(idx / cpr3), c = (int)(idx % cpr3);
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int p = c * 8 + e, tap = p / C2, c2 = ekperm(p % C2);
        v[e] = w3[(((long)n * C2 + c2) * 2 + (tap >> 1)) * 2 + (tap & 1)];
      }
      u32x4 o;
      o[0] = pack_bf16x2(v[0], v[1]); o[1] = pack_bf16x2(v[2], v[3]); o[2] = pack_bf16x2(v[4], v[5]); o[3] = pack_bf16x2(v[6], v[7]);
      const int tile = n / 32, rr = n % 32;
      *((u32x4*)(dst + EHDR + W2B + (long)tile * 32 * K3 * 2) + (long)rr * cpr3 + swz_chunk(rr, c, cpr3)) = o;
    }
  }
}

template <int CB, int SPLIT>
void launch_enc23_s(const EncArgs& A, long rows, hipStream_t s) {
  using G = EncGeom<CB>;
  static TantePerDevice attr;
  attr.once([&] {
    hipFuncSetAttribute((const void*)enc23_kernel<CB, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS);
  });
  hipLaunchKernelGGL((enc23_kernel<CB, SPLIT>), dim3((unsigned)((rows + 127) / 128), SPLIT), dim3(512), G::LDS, s, A);
}
template <int CB>
void launch_enc123_raw(const EncArgs& A, hipStream_t s) {
  using G = EncGeom<CB>;
  constexpr int lds = G::LDS + E1BYTES - E1BIAS;
  static TantePerDevice attr;
  attr.once([&] { hipFuncSetAttribute((const void*)enc23_kernel<CB, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
  const long rows = (long)A.n_img * A.Hp * A.Wp;
  hipLaunchKernelGGL((enc23_kernel<CB, 1, true>), dim3((unsigned)((rows + 127) / 128), 1), dim3(512), lds, s, A);
}
template <int CB>
void launch_enc23(const EncArgs& A, hipStream_t s) {
  const long rows = (long)A.n_img * A.Hp * A.Wp;
  const int force = tante_opt("TANTE_ENC23_SPLIT", 0);
  const int groups = (int)((rows + 127) / 128);
  const int split = force ? force : (groups <= 64 ? 4 : groups <= 128 ? 2 : 1);      // fill the CUs when the input is one frame
  if (split >= 4) launch_enc23_s<CB, 4>(A, rows, s);
  else if (split == 2) launch_enc23_s<CB, 2>(A, rows, s);
  else launch_enc23_s<CB, 1>(A, rows, s);
}

// ---- stage 1 straight from the channels-last batch (the rollout's first window) -------------------------------------------------------
// raw (n_img, H, W, D) fp32 as the datamodule yields it -> h1 (n_img, H/2, W/2, 64) bf16 = [Conv2d k = s = 2 -> GELU(erf)] of the
// nan_to_num-ed, channels-first image, which is never written: a workgroup takes one stage-1 row of up to 128 pixels, i.e. two pixel rows
// of up to 256 pixels -- two contiguous, 16-byte aligned runs of 256 D floats (W % 8 == 0) -- into LDS as they lie, and each wave
// gathers its 16-pixel B operands from there, cleaned as it reads.  Images of the LAST time slot also leave their cleaned
// channels-first frame (the Taylor base the model reads in place); the other slots' frames have no reader.
// The bits are those of tante_format_input + gemm_kernel<bf16, CB = 2, TT = 2, AM_NCHW2, EP_LIN_GELU_ERF> (gemm.hip): k = 4 ci + 2 kh + kw
// padded with zeros to 64, the same bf16 operand roundings, acc = 0 -> MFMA(k 0..31) -> MFMA(k 32..63) with the weight as the A operand,
// then + bias, the gelu_poly fma chain, pack_bf16x2.
struct Enc1Args {
  const float* raw;          // (n_img, H, W, D)
  const char* w;             // packed stage-1 stream
  unsigned short* h1;        // (n_img, H / 2, W / 2, 64) bf16
  float* frame_out;          // image (b, T - 1) -> frame_out + b * frame_bstride, (D, H, W)
  long frame_bstride;
  int H, W, D, T;
};

__global__ __launch_bounds__(256) void enc1_raw_kernel(const Enc1Args A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 pixel rows][256 pixels][D], as they lie in memory
  const float* px = (const float*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, l15 = lane & 15;
  const int D = A.D, RS = E1PX * D;
  const int x0 = blockIdx.x * E1PX, ho = blockIdx.y, img = blockIdx.z;
  const int npx = min(E1PX, A.W - x0);                          // a multiple of 8
  const int rbytes = npx * D * 4;                               // a pixel row's run: a multiple of 32 bytes

  // ---- the two pixel rows -> LDS by LDS-DMA (no registers: 1 KiB per wave instruction); nan_to_num is applied where they are read ---
  const char* src = (const char*)(A.raw + (((long)img * A.H + 2 * ho) * A.W + x0) * D);
#pragma unroll
  for (int r = 0; r < 2; ++r)
    for (int off = wave * 1024; off < rbytes; off += 4096)
      if (off + lane * 16 < rbytes)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (long)r * A.W * D * 4 + off + lane * 16),
                                         (__attribute__((address_space(3))) void*)(smem + r * RS * 4 + off), 16, 0, 0);

  // weight fragments and bias: 8.25 KB that every workgroup reads (L2)
  u32x4 wf[E1FRAGS];
#pragma unroll
  for (int f = 0; f < E1FRAGS; ++f) wf[f] = *((const u32x4*)A.w + f * 64 + lane);
  f32x4 bias[4];
#pragma unroll
  for (int ns = 0; ns < 4; ++ns) bias[ns] = *(const f32x4*)((const float*)(A.w + E1BIAS) + ns * 16 + kk * 4);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- slot T - 1: the channels-first frame, 4 pixels (16 bytes) per lane; a wave stores 256 pixels of one field of one row ---------
  if (img % A.T == A.T - 1) {
    float* dst = A.frame_out + (long)(img / A.T) * A.frame_bstride + (long)(2 * ho) * A.W + x0 + 4 * lane;
    if (4 * lane < npx)
      for (int c = wave; c < 2 * D; c += 4) {
        const int d = c >> 1, r = c & 1;
        const float* q = px + r * RS + 4 * lane * D + d;
        const f32x4 o = {nan_to_num_raw(q[0]), nan_to_num_raw(q[D]), nan_to_num_raw(q[2 * D]), nan_to_num_raw(q[3 * D])};
        *(f32x4*)(dst + (long)d * A.H * A.W + r * A.W) = o;
      }
  }

  // ---- stage 1: a wave takes 16 stage-1 pixels at a time ------------------------------------------------------------------------
  const int W1 = A.W / 2, n1 = npx / 2;
  unsigned short* orow = A.h1 + (((long)img * (A.H / 2) + ho) * W1 + x0 / 2) * E1C;
  for (int t0 = wave * 16; t0 < n1; t0 += 64) {
    const int p1 = t0 + l15;
    const bool live = p1 < n1;
    u32x4 xf[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float x[8];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int ci = 2 * (cb * 4 + kk) + e;
        const bool ok = live && ci < D;               // dead pixels and k >= 4 D are selects: nothing past the rows is read
        const float* q = px + (2 * p1) * D + ci;
        x[4 * e] = ok ? nan_to_zero(q[0]) : 0.0f;
        x[4 * e + 1] = ok ? nan_to_zero(q[D]) : 0.0f;
        x[4 * e + 2] = ok ? nan_to_zero(q[RS]) : 0.0f;
        x[4 * e + 3] = ok ? nan_to_zero(q[RS + D]) : 0.0f;
      }
      xf[cb][0] = pack_bf16x2(x[0], x[1]); xf[cb][1] = pack_bf16x2(x[2], x[3]);
      xf[cb][2] = pack_bf16x2(x[4], x[5]); xf[cb][3] = pack_bf16x2(x[6], x[7]);
    }
    u32x2 u[4];
#pragma unroll
    for (int ns = 0; ns < 4; ++ns) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = mfma_bf16(wf[ns * 2], xf[0], acc);
      acc = mfma_bf16(wf[ns * 2 + 1], xf[1], acc);
      const f32x4 y = gelu_poly4<false>(acc + bias[ns]);          // = gelu_poly1 per element: the same fma chain, packed
      u[ns][0] = pack_bf16x2(y[0], y[1]);
      u[ns][1] = pack_bf16x2(y[2], y[3]);
    }
    // a lane holds channels 16 ns + 4 kk .. + 3: the lanes kk = 2 m and 2 m + 1 trade halves, so that the even one stores the 16 bytes
    // of channels 32 p + 8 m .. + 7 and the odd one those of 32 p + 16 + 8 m .. + 7 -- 64 contiguous bytes per pixel and instruction
    const bool odd = kk & 1;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const u32x2 own = odd ? u[2 * p + 1] : u[2 * p], give = odd ? u[2 * p] : u[2 * p + 1];
      u32x2 got;
      got[0] = (unsigned)__shfl_xor((int)give[0], 16);
      got[1] = (unsigned)__shfl_xor((int)give[1], 16);
      const u32x4 o = odd ? u32x4{got[0], got[1], own[0], own[1]} : u32x4{own[0], own[1], got[0], got[1]};
      if (live) *(u32x4*)(orow + (long)p1 * E1C + 32 * p + (odd ? 16 : 0) + 8 * (kk >> 1)) = o;
    }
  }
}

// conv1 (64, D, 2, 2) in its native (ci, kh, kw) k order -> A fragments: fragment (ns, cb), lane (kk, l15) = row 16 ns + l15, k 8 (4 cb + kk) .. + 7;
// the permuted copy: row l15 of tile t = 2 half + dt is channel 32 half + 8 (l15 >> 2) + 4 dt + (l15 & 3), so that the accumulators of the
// tile pair (half, 0), (half, 1) are a lane's channels 32 half + 8 kk .. + 7: a stage-2 B-operand block
__global__ void pack_enc1_raw_kernel(const float* __restrict__ w1, const float* __restrict__ b1, int D, char* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 256) ((float*)(dst + E1BIAS))[i] = i < E1C ? b1[i] : 0.0f;
  if (i >= 2 * E1FRAGS * 64) return;
  const bool perm = i >= E1FRAGS * 64;
  const int q = perm ? i - E1FRAGS * 64 : i;
  const int f = q >> 6, lane = q & 63, ns = f >> 1, cb = f & 1, kq = lane >> 4, l = lane & 15, K = 4 * D;
  const int n = perm ? 32 * (ns >> 1) + 8 * (l >> 2) + 4 * (ns & 1) + (l & 3) : ns * 16 + l;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = (cb * 4 + kq) * 8 + e;
    v[e] = k < K ? w1[(long)n * K + k] : 0.0f;
  }
  u32x4 o;
  o[0] = pack_bf16x2(v[0], v[1]); o[1] = pack_bf16x2(v[2], v[3]); o[2] = pack_bf16x2(v[4], v[5]); o[3] = pack_bf16x2(v[6], v[7]);
  *((u32x4*)(dst + (perm ? E1PERM : 0)) + q) = o;
}

}  // namespace

extern "C" int tante_enc23_supported(int C) { return C == 256; }

extern "C" int64_t tante_enc23_stream_bytes(int C) {
  const long C1 = C / 4, C2 = C / 2;
  return EHDR + C2 * 4 * C1 * 2 + (long)C * 4 * C2 * 2;
}

extern "C" int tante_pack_enc23(const float* w2, const float* b2, const float* w3, const float* b3, int C, void* enc_stream, void* stream) {
  if (!w2 || !b2 || !w3 || !b3 || !enc_stream) TANTE_FAIL(-1, "tante_pack_enc23: null pointer");
  if (!tante_enc23_supported(C)) TANTE_FAIL(-2, "tante_pack_enc23: unsupported C=%d", C);
  hipLaunchKernelGGL(pack_enc_stream_kernel, dim3(64, 3), dim3(256), 0, (hipStream_t)stream, w2, b2, w3, b3, C, (char*)enc_stream);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_enc23_fused(const void* h1, int n_img, int Hp, int Wp, int C, const void* enc_stream, const float* film_a,
                                 const float* film_b, const float* s_emb, int T, float* out, void* stream) {
  if (!h1 || !enc_stream || !film_a || !film_b || !s_emb || !out) TANTE_FAIL(-1, "tante_enc23_fused: null pointer");
  if (!tante_enc23_supported(C)) TANTE_FAIL(-2, "tante_enc23_fused: unsupported C=%d", C);
  if (n_img <= 0 || Hp <= 0 || Wp <= 0 || T <= 0) TANTE_FAIL(-1, "tante_enc23_fused: bad shape");
  if (((uintptr_t)h1 % 16) || ((uintptr_t)out % 16) || ((uintptr_t)film_a % 16) || ((uintptr_t)film_b % 16) || ((uintptr_t)s_emb % 16))
    TANTE_FAIL(-1, "tante_enc23_fused: alignment");
  EncArgs A = {};
  A.h1 = (const unsigned short*)h1; A.w = (const char*)enc_stream; A.film_a = film_a; A.film_b = film_b; A.s_emb = s_emb; A.out = out;
  A.n_img = n_img; A.Hp = Hp; A.Wp = Wp; A.T = T; A.out_frames = 0;
  launch_enc23<8>(A, (hipStream_t)stream);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_enc23_frames(const void* h1, int n_img, int frames, int Hp, int Wp, int C, const void* enc_stream, float* out, void* stream) {
  if (!h1 || !enc_stream || !out) TANTE_FAIL(-1, "tante_enc23_frames: null pointer");
  if (!tante_enc23_supported(C)) TANTE_FAIL(-2, "tante_enc23_frames: unsupported C=%d", C);
  if (n_img <= 0 || frames <= 0 || n_img % frames || Hp <= 0 || Wp <= 0) TANTE_FAIL(-1, "tante_enc23_frames: bad shape");
  if (((uintptr_t)h1 % 16) || ((uintptr_t)out % 16)) TANTE_FAIL(-1, "tante_enc23_frames: alignment");
  EncArgs A = {};
  A.h1 = (const unsigned short*)h1; A.w = (const char*)enc_stream; A.film_a = A.film_b = A.s_emb = out; A.out = out;   // tables unused
  A.n_img = n_img; A.Hp = Hp; A.Wp = Wp; A.T = 1; A.out_frames = frames;
  launch_enc23<8>(A, (hipStream_t)stream);
  TANTE_CHECK_LAUNCH();
  return 0;
}

// ---- the rollout's first window straight from the channels-last batch ----------------------------------------------------------------
extern "C" int tante_enc1_raw_supported(int C, int D) { return C == 256 && D >= 1 && 4 * D <= 64; }

extern "C" int64_t tante_enc1_raw_stream_bytes(void) { return E1BYTES; }

extern "C" int tante_pack_enc1_raw(const float* w1, const float* b1, int C, int D, void* enc1_stream, void* stream) {
  if (!w1 || !b1 || !enc1_stream) TANTE_FAIL(-1, "tante_pack_enc1_raw: null pointer");
  if (!tante_enc1_raw_supported(C, D)) TANTE_FAIL(-2, "tante_pack_enc1_raw: unsupported C=%d D=%d", C, D);
  if ((uintptr_t)enc1_stream % 16) TANTE_FAIL(-1, "tante_pack_enc1_raw: alignment");
  hipLaunchKernelGGL(pack_enc1_raw_kernel, dim3(4), dim3(256), 0, (hipStream_t)stream, w1, b1, D, (char*)enc1_stream);
  TANTE_CHECK_LAUNCH();
  return 0;
}

// raw (B, T, H, W, D) fp32 channels-last -> z (T, B, H/8 * W/8, C) fp32, the pre-FiLM frame cache tante_enc23_frames(frames = T) writes, and
// the nan_to_num-ed channels-first frame of slot T - 1 at frame_out + b * frame_bstride.  h1: (B T H/2 W/2 C/4) bf16 of scratch.
// Two launches: stage 1 from the batch where it lies, then the stage 2 + 3 kernel.  Option TANTE_RAW_ENCODE_ONE_LAUNCH = 1: one launch,
// enc23_kernel<.., RAW = true> computes stage 1 itself and h1 is not touched.
extern "C" int tante_encode_window_raw(const float* raw, int B, int T, int H, int W, int D, int C, const void* enc1_stream,
                                       const void* enc_stream, void* h1, float* z, float* frame_out, int64_t frame_bstride, void* stream) {
  if (!raw || !enc1_stream || !enc_stream || !h1 || !z || !frame_out) TANTE_FAIL(-1, "tante_encode_window_raw: null pointer");
  if (!tante_enc1_raw_supported(C, D)) TANTE_FAIL(-2, "tante_encode_window_raw: unsupported C=%d D=%d", C, D);
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8 || frame_bstride < (int64_t)D * H * W)
    TANTE_FAIL(-1, "tante_encode_window_raw: bad shape");
  const long n_img = (long)B * T;
  if (n_img > 65535 || H / 2 > 65535 || n_img * (H / 8) * (W / 8) >= (1L << 31)) TANTE_FAIL(-2, "tante_encode_window_raw: too many images / rows");
  if (((uintptr_t)raw % 16) || ((uintptr_t)enc1_stream % 16) || ((uintptr_t)h1 % 16) || ((uintptr_t)z % 16) || ((uintptr_t)frame_out % 16) ||
      frame_bstride % 4)
    TANTE_FAIL(-1, "tante_encode_window_raw: alignment");
  if (tante_opt("TANTE_RAW_ENCODE_ONE_LAUNCH", 0)) {   // the one-launch form: same bits, measured 10 us slower than the two launches below
    EncArgs A = {};
    A.h1 = nullptr; A.w = (const char*)enc_stream; A.film_a = A.film_b = A.s_emb = z; A.out = z;
    A.n_img = (int)n_img; A.Hp = H / 8; A.Wp = W / 8; A.T = 1; A.out_frames = T;
    A.raw = raw; A.w1 = (const char*)enc1_stream; A.frame_out = frame_out; A.frame_bstride = frame_bstride; A.D = D;
    launch_enc123_raw<8>(A, (hipStream_t)stream);
    TANTE_CHECK_LAUNCH();
    return 0;
  }
  Enc1Args E;
  E.raw = raw; E.w = (const char*)enc1_stream; E.h1 = (unsigned short*)h1; E.frame_out = frame_out; E.frame_bstride = frame_bstride;
  E.H = H; E.W = W; E.D = D; E.T = T;
  const size_t lds = (size_t)2 * E1PX * D * sizeof(float);      // the kernel's row stride is 256 pixels whatever W is
  hipLaunchKernelGGL(enc1_raw_kernel, dim3((unsigned)((W + E1PX - 1) / E1PX), (unsigned)(H / 2), (unsigned)n_img), dim3(256), lds,
                     (hipStream_t)stream, E);
  TANTE_CHECK_LAUNCH();
  EncArgs A = {};
  A.h1 = (const unsigned short*)h1; A.w = (const char*)enc_stream; A.film_a = A.film_b = A.s_emb = z; A.out = z;   // tables unused
  A.n_img = (int)n_img; A.Hp = H / 8; A.Wp = W / 8; A.T = 1; A.out_frames = T;
  launch_enc23<8>(A, (hipStream_t)stream);
  TANTE_CHECK_LAUNCH();
  return 0;
}
