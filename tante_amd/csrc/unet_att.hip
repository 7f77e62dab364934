// AttentionUNet's operations that no other path of the library serves (reference models/unet_att.py): a dense 3 x 3 convolution as an
// implicit GEMM on the matrix pipe, and the attention gate as one launch.
//
// ---- tante_conv3x3_mfma: y = act(conv3x3(src) * scale + shift), padding 1, stride 1, channels-last (n, H, W, C) ----------------------------
// Eval-mode BatchNorm and the conv bias are folded by the caller (unet_att.py:11-16, 31-33): scale rides the packed weights, shift is
// added in the epilogue before the optional ReLU.
// A workgroup of four waves (2 x 2) owns a tile of TH x 16 pixels of ONE image and CG output channels; a wave owns RW pixel rows of 16 and
// NW tiles of 16 output channels (TH = 2 RW, CG = 32 NW).  The product is formed transposed, y^T (channel x pixel) += W (channel x k)
// x^T (k x pixel): the A operand is a weight fragment read straight from the packed stream (L2), the B operand is a pixel row of the halo
// tile in LDS, and the result registers of a lane are 4 consecutive channels of one pixel -- a 16-byte channels-last store.
//   staging   the tile with its 1-pixel halo ((TH + 2) x 18 pixels) is staged in LDS in chunks of 64 input channels (128 under the smallest tile form), fp32 (TANTE_F32) or
//             rounded to bf16 (TANTE_BF16).  Loads are bounded by THIS image's H and W; positions outside it, and channels past Cin, are
//             zeros; the neighbouring image of the batch is never read.  The staging loop takes the source form, so that the pooled, the
//             upsampled and the concatenated tensors of the model are never written:
//               plain      src (n, H, W, Ca) [and a second source (n, H, W, Cb) for channels Ca .. Ca + Cb - 1: torch.cat, unet_att.py:149-169]
//               pooled     src (n, Hs, Ws, Ca), H = Hs / 2, W = Ws / 2 (floor): the max over the 2 x 2 window (MaxPool2d(2, 2), unet_att.py:94)
//               upsampled  src (n, H / 2, W / 2, Ca) read at (y >> 1, x >> 1) (nn.Upsample(scale_factor=2), nearest, unet_att.py:30)
//   K order   channel chunk, then k-step of 16 (fp32) or 32 (bf16) channels inside it, then tap (dy, dx): fixed, the same in every tile
//             form, so a pixel's sum does not depend on the tile form, on where its tile lies or on its image's place in the batch.
//   products  v_mfma_f32_16x16x4_f32, or v_mfma_f32_16x16x32_bf16 with fp32 accumulation.
// No atomics, no split-K through memory.  The tile form is chosen per launch (ua_pick): the deep levels of the pyramid have few pixels
// and many channels, and the widest form that still gives two (8 x 16 x 64) or four (4 x 16 x 32) workgroups per CU is taken.
//
// ---- tante_attn_gate: AttentionBlock.forward (unet_att.py:70-76) on channels-last rows, one launch ------------------------------------------
//   psi = sigmoid(w_psi . relu(W [g | x] + b) + b_psi),  out = x * psi
// with the three BatchNorms folded by the caller.  h^T (hidden x token) = W [g | x]^T on the matrix pipe (A: weight fragments from L2,
// B: the tokens' rows straight from memory), the hidden values stay in the result registers, the dot product with w_psi runs over a
// lane's registers in index order, then over the four lane groups by two xor shuffles, then (64 hidden columns and more, where the
// four waves of a workgroup split the hidden columns of 16 tokens) over the waves in wave order through LDS -- a fixed order -- and the
// gate multiplies the fp32 x rows.
#include "common.hip.h"

namespace {

constexpr int UA_THREADS = 256;
constexpr int UA_TW = 16;                   // pixels per tile row = one MFMA column block
constexpr int UA_MAXCIN = 2048, UA_MAXCOUT = 1024;
constexpr int UA_PLAIN = 0, UA_POOLED = 1, UA_UPSAMPLED = 2;
constexpr int AG_MAXK = 1024, AG_MAXN = 256;

__device__ __forceinline__ f32x4 ua_mfma32(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- channels [c, c + 4) of the concatenation [a | b] at pixel `pix`; zeros past Ca + Cb and where !ok.  Branch-free: an element that
// is not wanted reads a[pix * Ca] (always a valid address) and is replaced by zero, so that every load of a staging pass is in flight
// at once instead of waiting behind its own branch.  VEC: Ca and Cb are multiples of 4 and the rows start on 16 bytes -----------------------
__device__ __forceinline__ float ua_at(const float* __restrict__ a, const float* __restrict__ b, int Ca, int Cb, long pix, int c, bool ok) {
  const bool valid = ok && c < Ca + Cb;
  const bool first = !valid || c < Ca;
  const float* base = first ? a : b;
  const int cc = valid ? (first ? c : c - Ca) : 0;
  const float v = base[pix * (first ? Ca : Cb) + cc];
  return valid ? v : 0.0f;
}
template <bool VEC>
__device__ __forceinline__ f32x4 ua_at4(const float* __restrict__ a, const float* __restrict__ b, int Ca, int Cb, long pix, int c, bool ok) {
  if constexpr (VEC) {
    const bool valid = ok && c < Ca + Cb;
    const bool first = !valid || c < Ca;
    const float* base = first ? a : b;
    const int cc = valid ? (first ? c : c - Ca) : 0;
    const f32x4 v = *(const f32x4*)(base + pix * (first ? Ca : Cb) + cc);
    return valid ? v : f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    return f32x4{ua_at(a, b, Ca, Cb, pix, c, ok), ua_at(a, b, Ca, Cb, pix, c + 1, ok), ua_at(a, b, Ca, Cb, pix, c + 2, ok), ua_at(a, b, Ca, Cb, pix, c + 3, ok)};
  }
}
__device__ __forceinline__ f32x4 ua_max4(const f32x4& p, const f32x4& q) {
  return f32x4{fmaxf(p[0], q[0]), fmaxf(p[1], q[1]), fmaxf(p[2], q[2]), fmaxf(p[3], q[3])};
}

// ---- geometry of the packed weights: [cout tile][k-step][tap][lane][4 floats | 8 bf16] ---------------------------------------------------
struct UaGeom {
  int CT, G, KS;      // tiles of 16 output channels, k-steps, channels per k-step
};
__host__ __device__ inline UaGeom ua_geom(int Cin, int Cout, bool bf) {
  UaGeom g;
  g.KS = bf ? 32 : 16;
  g.CT = (Cout + 15) / 16;
  g.G = (Cin + g.KS - 1) / g.KS;
  return g;
}
inline int64_t ua_pack_bytes(int Cin, int Cout, bool bf) {
  const UaGeom g = ua_geom(Cin, Cout, bf);
  return (int64_t)g.CT * g.G * 9 * 64 * 16;      // 16 bytes per lane in either mode
}

__global__ __launch_bounds__(UA_THREADS) void ua_pack_kernel(const float* __restrict__ w, int Cin, int Cout, int bf, void* __restrict__ out, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const UaGeom g = ua_geom(Cin, Cout, bf != 0);
  const int E = bf ? 8 : 4;
  const int el = (int)(e % E), lane = (int)((e / E) & 63);
  long rest = e / (64 * E);
  const int tap = (int)(rest % 9);
  rest /= 9;
  const int gk = (int)(rest % g.G), ct = (int)(rest / g.G);
  const int co = ct * 16 + (lane & 15), ci = gk * g.KS + E * (lane >> 4) + el;
  float v = 0.0f;
  if (co < Cout && ci < Cin) v = w[((long)co * Cin + ci) * 9 + tap];
  if (bf) ((__bf16*)out)[e] = (__bf16)v;
  else ((float*)out)[e] = v;
}

// ---- the convolution ------------------------------------------------------------------------------------------------------------------
struct UaArgs {
  const float* a;
  const float* b;
  const void* wp;
  const float* shift;
  void* y;
  int Ca, Cb, Cout, H, W, Hs, Ws, relu, bf16_out, tiles_x, tiles_y;
};

constexpr int ua_ch(int RW) { return RW == 1 ? 128 : 64; }                                 // input channels per staged chunk: the smallest tile takes more
constexpr int ua_rs(int CH, bool BF) { return BF ? (CH + 8) / 2 : CH + 4; }                // LDS row stride of one halo pixel, in 4-byte words
constexpr int ua_lds(int RW, bool BF) { return 4 * (2 * RW + 2) * (UA_TW + 2) * ua_rs(ua_ch(RW), BF); }

template <int RW, int NW, int FORM, bool BF, bool VEC>
__global__ __launch_bounds__(UA_THREADS) void ua_conv_kernel(const UaArgs p) {
  constexpr int TH = 2 * RW, HW = UA_TW + 2, HP = (TH + 2) * HW, CH = ua_ch(RW), RS = ua_rs(CH, BF), KS = BF ? 32 : 16;
  constexpr int NG = CH / 4, PER = (HP * NG + UA_THREADS - 1) / UA_THREADS;      // 4-channel groups per pixel; staged items per thread
  extern __shared__ __attribute__((aligned(16))) unsigned ua_halo[];
  const int H = p.H, W = p.W, Ca = p.Ca, Cb = p.Cb, Cin = Ca + Cb, Cout = p.Cout;
  const long blk = blockIdx.x;
  const int tiles = p.tiles_x * p.tiles_y;
  const long img = blk / tiles;
  const int tile = (int)(blk % tiles);
  const int y0 = (tile / p.tiles_x) * TH, x0 = (tile % p.tiles_x) * UA_TW;
  const long spix = (long)p.Hs * p.Ws;
  const float* sa = p.a + img * spix * Ca;
  const float* sb = p.b ? p.b + img * spix * Cb : nullptr;
  const int Ws = p.Ws;
  const bool bf16_out = p.bf16_out != 0;

  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 15, kk = l >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const UaGeom g = ua_geom(Cin, Cout, BF);
  int ct[NW];
  const u32x4* wf[NW];
#pragma unroll
  for (int n = 0; n < NW; ++n) {
    ct[n] = ((int)blockIdx.y * 2 + wn) * NW + n;
    const int ctv = ct[n] < g.CT ? ct[n] : g.CT - 1;             // a tile past the last one recomputes the last; its stores are masked
    wf[n] = (const u32x4*)p.wp + (long)ctv * g.G * 9 * 64 + l;
  }
  f32x4 acc[RW][NW];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int n = 0; n < NW; ++n) acc[r][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // item i of a chunk = 4 channels of one halo pixel: its value from the source (zeros outside the image and past Cin) ...
  auto load_item = [&](int i, int c0) -> f32x4 {
    const int grp = i % NG, hp = i / NG;
    const int gy = y0 + hp / HW - 1, gx = x0 + hp % HW - 1;
    const int c = c0 + 4 * grp;
    const bool ok = hp < HP && gy >= 0 && gy < H && gx >= 0 && gx < W;
    const int cy = gy < 0 ? 0 : (gy >= H ? H - 1 : gy), cx = gx < 0 ? 0 : (gx >= W ? W - 1 : gx);      // a valid pixel either way
    if constexpr (FORM == UA_POOLED) {
      const long q = (long)(2 * cy) * Ws + 2 * cx;
      return ua_max4(ua_max4(ua_at4<VEC>(sa, sb, Ca, Cb, q, c, ok), ua_at4<VEC>(sa, sb, Ca, Cb, q + 1, c, ok)),
                     ua_max4(ua_at4<VEC>(sa, sb, Ca, Cb, q + Ws, c, ok), ua_at4<VEC>(sa, sb, Ca, Cb, q + Ws + 1, c, ok)));
    } else if constexpr (FORM == UA_UPSAMPLED) {
      return ua_at4<VEC>(sa, sb, Ca, Cb, (long)(cy >> 1) * Ws + (cx >> 1), c, ok);
    } else {
      return ua_at4<VEC>(sa, sb, Ca, Cb, (long)cy * Ws + cx, c, ok);
    }
  };
  // ... and its place in LDS
  auto store_item = [&](int i, const f32x4& v) {
    const int grp = i % NG, hp = i / NG;
    if (hp >= HP) return;
    if constexpr (BF) {
      *(u32x2*)(ua_halo + hp * RS + 2 * grp) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    } else {
      *(f32x4*)(ua_halo + hp * RS + 4 * grp) = v;
    }
  };
  // The two small tile forms run where a level has few workgroups, so nothing else on the CU covers a chunk's load latency: a thread
  // holds its share of the NEXT chunk in registers while the matrix pipe works on this one.  The wide form runs with several workgroups
  // per CU, which cover each other; it stages directly and keeps its registers for occupancy.
  constexpr bool PRE = RW < 4;
  f32x4 pre[PRE ? PER : 1];
  const int CinP = g.G * KS;
  if constexpr (PRE) {
#pragma unroll
    for (int u = 0; u < PER; ++u) pre[u] = load_item(threadIdx.x + u * UA_THREADS, 0);
  }
  for (int c0 = 0; c0 < CinP; c0 += CH) {
    const int cn = (CinP - c0) < CH ? (CinP - c0) : CH;
    __syncthreads();                                              // the previous chunk's reads of the halo are done
    if constexpr (PRE) {
#pragma unroll
      for (int u = 0; u < PER; ++u) store_item(threadIdx.x + u * UA_THREADS, pre[u]);
    } else {
#pragma unroll 4
      for (int i = threadIdx.x; i < HP * NG; i += UA_THREADS) store_item(i, load_item(i, c0));
    }
    __syncthreads();
    if constexpr (PRE) {
      if (c0 + CH < CinP) {
#pragma unroll
        for (int u = 0; u < PER; ++u) pre[u] = load_item(threadIdx.x + u * UA_THREADS, c0 + CH);
      }
    }
    const int nks = cn / KS;
    for (int ks = 0; ks < nks; ++ks) {
      const long gk = c0 / KS + ks;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3, dx = tap % 3;
        u32x4 wv[NW];
#pragma unroll
        for (int n = 0; n < NW; ++n) wv[n] = wf[n][(gk * 9 + tap) * 64];
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          const int hp = (wm * RW + r + dy) * HW + j + dx;
          // 16 bytes of pixel hp: fp32 channels 16 ks + 4 kk .. + 3, or bf16 channels 32 ks + 8 kk .. + 7 -- the same word offset
          const u32x4 t = *(const u32x4*)(ua_halo + hp * RS + ks * 16 + 4 * kk);
          if constexpr (BF) {
#pragma unroll
            for (int n = 0; n < NW; ++n) acc[r][n] = ua_mfma32(wv[n], t, acc[r][n]);
          } else {
            const f32x4 tf = __builtin_bit_cast(f32x4, t);
#pragma unroll
            for (int n = 0; n < NW; ++n) {
              const f32x4 wq = __builtin_bit_cast(f32x4, wv[n]);
#pragma unroll
              for (int s = 0; s < 4; ++s) acc[r][n] = mfma4(wq[s], tf[s], acc[r][n]);
            }
          }
        }
      }
    }
  }

  // epilogue: lane (j, kk), register r = channel 16 ct + 4 kk + r of pixel (row, x0 + j)
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const int py = y0 + wm * RW + r, px = x0 + j;
    if (py >= H || px >= W) continue;
    const long base = ((img * H + py) * (long)W + px) * Cout;
#pragma unroll
    for (int n = 0; n < NW; ++n) {
      const int c = ct[n] * 16 + 4 * kk;
      if (c >= Cout) continue;
      f32x4 v = acc[r][n];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (p.shift && c + e < Cout) v[e] += p.shift[c + e];
        if (p.relu) v[e] = fmaxf(v[e], 0.0f);
      }
      if (VEC && c + 4 <= Cout && (Cout & 3) == 0) {
        if (bf16_out) *(u32x2*)((__bf16*)p.y + base + c) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        else *(f32x4*)((float*)p.y + base + c) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e < Cout) {
            if (bf16_out) ((__bf16*)p.y)[base + c + e] = (__bf16)v[e];
            else ((float*)p.y)[base + c + e] = v[e];
          }
      }
    }
  }
}

// the tile forms, widest first: {RW, NW} -> TH = 2 RW pixel rows, CG = 32 NW output channels
constexpr int UA_FORMS = 3;
constexpr int UA_FORM_RW[UA_FORMS] = {4, 2, 1};
constexpr int UA_FORM_NW[UA_FORMS] = {2, 1, 1};
// workgroups a form must give to be taken: measured on the reference config's 18 shapes at B = 1 and B = 4 with every form forced
// (DESIGN 4.9): the 8 x 16 x 64 form wins from two workgroups per CU on, the 4 x 16 x 32 form from four; below that a level has too few
// waves per SIMD to cover the latency of its weight stream, and the narrowest form, which gives the most workgroups, is the fastest
constexpr long UA_FORM_MIN_WGS[UA_FORMS] = {512, 1024, 0};

inline long ua_wgs(int f, int64_t n_img, int H, int W, int Cout) {
  const int TH = 2 * UA_FORM_RW[f], CG = 32 * UA_FORM_NW[f];
  return (long)n_img * ((H + TH - 1) / TH) * ((W + UA_TW - 1) / UA_TW) * ((Cout + CG - 1) / CG);
}
// the widest form that gives its minimum of workgroups, else the narrowest; TANTE_CONV3_FORM = 1..3 forces one (A/B)
inline int ua_pick(int64_t n_img, int H, int W, int Cout) {
  const int forced = tante_opt("TANTE_CONV3_FORM", 0);
  if (forced >= 1 && forced <= UA_FORMS) return forced - 1;
  for (int f = 0; f < UA_FORMS; ++f)
    if (ua_wgs(f, n_img, H, W, Cout) >= UA_FORM_MIN_WGS[f]) return f;
  return UA_FORMS - 1;
}

template <int RW, int NW>
void ua_launch(const UaArgs& a, int64_t n_img, int form, bool bf, bool vec, hipStream_t s) {
  const dim3 grid((unsigned)(n_img * a.tiles_x * a.tiles_y), (unsigned)((a.Cout + 32 * NW - 1) / (32 * NW)));
#define UA_GO(FORM, BF, VEC) hipLaunchKernelGGL((ua_conv_kernel<RW, NW, FORM, BF, VEC>), grid, dim3(UA_THREADS), ua_lds(RW, BF), s, a)
#define UA_FORM(FORM)                                              \
  if (bf) {                                                        \
    if (vec) UA_GO(FORM, true, true); else UA_GO(FORM, true, false);   \
  } else {                                                         \
    if (vec) UA_GO(FORM, false, true); else UA_GO(FORM, false, false); \
  }
  if (form == UA_POOLED) { UA_FORM(UA_POOLED) }
  else if (form == UA_UPSAMPLED) { UA_FORM(UA_UPSAMPLED) }
  else { UA_FORM(UA_PLAIN) }
#undef UA_FORM
#undef UA_GO
}

const char* ua_reason(int64_t n_img, int Ca, int Cb, int Cout, int H, int W, int form) {
  if (form != UA_PLAIN && form != UA_POOLED && form != UA_UPSAMPLED) return "an unknown source form";
  if (Ca < 1 || Cb < 0 || (int64_t)Ca + Cb > UA_MAXCIN) return "input channels outside 1..2048";
  if (Cb > 0 && form != UA_PLAIN) return "a second source with a pooled or upsampled form";
  if (Cout < 1 || Cout > UA_MAXCOUT) return "output channels outside 1..1024";
  if (H < 1 || W < 1) return "an empty image";
  if (form == UA_UPSAMPLED && ((H | W) & 1)) return "an upsampled image of odd height or width";
  if (n_img < 0) return "a negative image count";
  const int64_t tiles = (int64_t)((W + UA_TW - 1) / UA_TW) * ((H + 1) / 2);
  if (tiles > 2147483647ll || n_img * tiles > 2147483647ll) return "more than 2^31 - 1 tiles per call";
  return nullptr;
}

// ---- the attention gate -----------------------------------------------------------------------------------------------------------------
// stream: floats [bias NP][w_psi NP][b_psi, 0, 0, 0] then the fragments [hidden tile][k-step][lane][4 floats | 8 bf16]
struct AgGeom {
  int NT, NP, G, KS;
  long frag;          // offset of the fragments in floats
};
__host__ __device__ inline AgGeom ag_geom(int K, int N, bool bf) {
  AgGeom g;
  int nt = 1;
  while (nt * 16 < N) nt *= 2;
  g.NT = nt;
  g.NP = 16 * nt;
  g.KS = bf ? 32 : 16;
  g.G = (K + g.KS - 1) / g.KS;
  g.frag = 2l * g.NP + 4;
  return g;
}
inline int64_t ag_stream_bytes(int K, int N, bool bf) {
  const AgGeom g = ag_geom(K, N, bf);
  return 4ll * g.frag + (int64_t)g.NT * g.G * 64 * 16;
}

__global__ __launch_bounds__(UA_THREADS) void ag_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ wpsi,
                                                             float bpsi, int K, int N, int bf, float* __restrict__ out, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const AgGeom g = ag_geom(K, N, bf != 0);
  if (e < g.frag) {
    float v = 0.0f;
    if (e < g.NP) v = e < N ? bias[e] : 0.0f;
    else if (e < 2 * g.NP) v = (e - g.NP) < N ? wpsi[e - g.NP] : 0.0f;
    else if (e == 2 * g.NP) v = bpsi;
    out[e] = v;
    return;
  }
  const long i = e - g.frag;
  if (i >= total) return;
  const int E = bf ? 8 : 4;
  const int el = (int)(i % E), lane = (int)((i / E) & 63);
  const long rest = i / (64 * E);
  const int gk = (int)(rest % g.G), nt = (int)(rest / g.G);
  const int n = nt * 16 + (lane & 15), k = gk * g.KS + E * (lane >> 4) + el;
  const float v = (n < N && k < K) ? w[(long)n * K + k] : 0.0f;
  if (bf) ((__bf16*)(out + g.frag))[i] = (__bf16)v;
  else out[g.frag + i] = v;
}

// SPLIT = false: a wave owns 16 tokens and all NTW hidden tiles (a workgroup 64 tokens).  SPLIT = true (64 hidden columns and more): the four
// waves of a workgroup share 16 tokens and own NTW hidden tiles each -- four times the workgroups on a level with few tokens, a quarter
// of the weight stream per wave -- and their partial dot products meet in LDS, added in wave order.
template <int NTW, bool SPLIT, bool BF, bool VEC>
__global__ __launch_bounds__(UA_THREADS) void ag_kernel(const float* __restrict__ gt, const float* __restrict__ x, long M, int Cg, int Cx,
                                                        const float* __restrict__ stream, float* __restrict__ out) {
  constexpr int KS = BF ? 32 : 16, NT = SPLIT ? 4 * NTW : NTW;
  __shared__ float zs[4][16];
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 15, kk = l >> 4;
  const long t0 = SPLIT ? (long)blockIdx.x * 16 : ((long)blockIdx.x * 4 + wave) * 16;
  if (!SPLIT && t0 >= M) return;                                  // wave-uniform; this form has no barrier (SPLIT: the grid is ceil(M / 16))
  const long tok = t0 + j;
  const long row = tok < M ? tok : M - 1;                         // a token past the end re-reads the last one; its store is masked
  const int K = Cg + Cx;
  const AgGeom g = ag_geom(K, NT * 16, BF);
  const int n0 = SPLIT ? wave * NTW : 0;
  const int G = (K + KS - 1) / KS;
  const u32x4* wf = (const u32x4*)(stream + g.frag) + (long)n0 * G * 64 + l;
  f32x4 acc[NTW];
#pragma unroll
  for (int n = 0; n < NTW; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int gk = 0; gk < G; ++gk) {
    if constexpr (BF) {
      const int k = gk * 32 + 8 * kk;
      const f32x4 lo = ua_at4<VEC>(gt, x, Cg, Cx, row, k, true), hi = ua_at4<VEC>(gt, x, Cg, Cx, row, k + 4, true);
      const u32x4 t = u32x4{pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]), pack_bf16x2(hi[0], hi[1]), pack_bf16x2(hi[2], hi[3])};
#pragma unroll
      for (int n = 0; n < NTW; ++n) acc[n] = ua_mfma32(wf[((long)n * G + gk) * 64], t, acc[n]);
    } else {
      const f32x4 t = ua_at4<VEC>(gt, x, Cg, Cx, row, gk * 16 + 4 * kk, true);
#pragma unroll
      for (int n = 0; n < NTW; ++n) {
        const f32x4 wq = __builtin_bit_cast(f32x4, wf[((long)n * G + gk) * 64]);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[n] = mfma4(wq[s], t[s], acc[n]);
      }
    }
  }
  // register r of tile n = hidden column 16 (n0 + n) + 4 kk + r of token j
  const float* bias = stream + n0 * 16;
  const float* wpsi = stream + NT * 16 + n0 * 16;
  float z = 0.0f;
#pragma unroll
  for (int n = 0; n < NTW; ++n) {
    const f32x4 bb = *(const f32x4*)(bias + n * 16 + 4 * kk), ww = *(const f32x4*)(wpsi + n * 16 + 4 * kk);
#pragma unroll
    for (int r = 0; r < 4; ++r) z = fmaf(fmaxf(acc[n][r] + bb[r], 0.0f), ww[r], z);
  }
  z += __shfl_xor(z, 16);
  z += __shfl_xor(z, 32);
  if constexpr (SPLIT) {
    if (kk == 0) zs[wave][j] = z;
    __syncthreads();
    z = ((zs[0][j] + zs[1][j]) + zs[2][j]) + zs[3][j];
  }
  const float psi = 1.0f / (1.0f + expf(-(z + stream[2 * NT * 16])));
  if (tok >= M) return;
  const float* xr = x + tok * Cx;
  float* orow = out + tok * Cx;
  const int q = SPLIT ? 4 * wave + kk : kk, nq = SPLIT ? 16 : 4;  // the lanes that share token j take the channels in turn
  if (VEC) {
    for (int c = 4 * q; c < Cx; c += 4 * nq) {
      const f32x4 v = *(const f32x4*)(xr + c);
      *(f32x4*)(orow + c) = f32x4{v[0] * psi, v[1] * psi, v[2] * psi, v[3] * psi};
    }
  } else {
    for (int c = q; c < Cx; c += nq) orow[c] = xr[c] * psi;
  }
}

template <int NTW, bool SPLIT>
void ag_launch(const float* g, const float* x, int64_t M, int Cg, int Cx, const float* st, bool bf, bool vec, float* out, hipStream_t s) {
  const dim3 grid((unsigned)(SPLIT ? (M + 15) / 16 : (M + 63) / 64));
#define AG_GO(BF, VEC) hipLaunchKernelGGL((ag_kernel<NTW, SPLIT, BF, VEC>), grid, dim3(UA_THREADS), 0, s, g, x, (long)M, Cg, Cx, st, out)
  if (bf) { if (vec) AG_GO(true, true); else AG_GO(true, false); }
  else { if (vec) AG_GO(false, true); else AG_GO(false, false); }
#undef AG_GO
}

const char* ag_reason(int64_t M, int Cg, int Cx, int N) {
  if (Cg < 1 || Cx < 1 || (int64_t)Cg + Cx > AG_MAXK) return "channels outside 1..1024 (gate plus skip)";
  if (N < 1 || N > AG_MAXN) return "coefficients outside 1..256";
  if (M < 0 || (M + 15) / 16 > 2147483647ll) return "rows outside 0..2^35 - 16";
  return nullptr;
}

}  // namespace

// ================================================================ C ABI ==================================================================
extern "C" int tante_conv3x3_mfma_supported(int64_t n_img, int Ca, int Cb, int Cout, int H, int W, int form) {
  return ua_reason(n_img, Ca, Cb, Cout, H, W, form) == nullptr ? 1 : 0;
}

extern "C" int64_t tante_conv3x3_pack_bytes(int Cin, int Cout, int compute) {
  if (Cin < 1 || Cin > UA_MAXCIN || Cout < 1 || Cout > UA_MAXCOUT || (compute != TANTE_F32 && compute != TANTE_BF16)) return -1;
  return ua_pack_bytes(Cin, Cout, compute == TANTE_BF16);
}

extern "C" int tante_pack_conv3x3(const float* w, int Cin, int Cout, int compute, void* out, void* stream) {
  if (Cin < 1 || Cin > UA_MAXCIN) TANTE_FAIL(-2, "tante_pack_conv3x3: input channels outside 1..2048 (Cin %d)", Cin);
  if (Cout < 1 || Cout > UA_MAXCOUT) TANTE_FAIL(-2, "tante_pack_conv3x3: output channels outside 1..1024 (Cout %d)", Cout);
  if (compute != TANTE_F32 && compute != TANTE_BF16) TANTE_FAIL(-1, "tante_pack_conv3x3: compute must be fp32 or bf16");
  if (!w || !out) TANTE_FAIL(-1, "tante_pack_conv3x3: null argument");
  if ((uintptr_t)out % 16) TANTE_FAIL(-1, "tante_pack_conv3x3: the packed weights must be 16-byte aligned");
  const bool bf = compute == TANTE_BF16;
  const long total = (long)(ua_pack_bytes(Cin, Cout, bf) / (bf ? 2 : 4));
  hipLaunchKernelGGL(ua_pack_kernel, dim3((unsigned)((total + UA_THREADS - 1) / UA_THREADS)), dim3(UA_THREADS), 0, (hipStream_t)stream, w, Cin, Cout, bf ? 1 : 0,
                     out, total);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_conv3x3_mfma(const float* a, int Ca, const float* b, int Cb, int64_t n_img, int H, int W, int form, int Hs, int Ws, const void* packed,
                                  const float* shift, int Cout, int act, int compute, void* y, int y_dtype, void* stream) {
  if (const char* why = ua_reason(n_img, Ca, Cb, Cout, H, W, form))
    TANTE_FAIL(-2, "tante_conv3x3_mfma: %s (images %lld, Cin %d + %d, Cout %d, %d x %d, form %d)", why, (long long)n_img, Ca, Cb, Cout, H, W, form);
  const bool fits = form == UA_PLAIN ? (Hs == H && Ws == W) : form == UA_POOLED ? (Hs / 2 == H && Ws / 2 == W) : (2 * Hs == H && 2 * Ws == W);
  if (!fits) TANTE_FAIL(-2, "tante_conv3x3_mfma: a source of %d x %d does not give %d x %d in form %d", Hs, Ws, H, W, form);
  if (compute != TANTE_F32 && compute != TANTE_BF16) TANTE_FAIL(-1, "tante_conv3x3_mfma: compute must be fp32 or bf16");
  if (y_dtype != TANTE_F32 && y_dtype != TANTE_BF16) TANTE_FAIL(-1, "tante_conv3x3_mfma: output dtype must be fp32 or bf16");
  if (act != TANTE_ACT_NONE && act != TANTE_ACT_RELU) TANTE_FAIL(-1, "tante_conv3x3_mfma: the activation must be none or ReLU");
  if (!a || !packed || !y || (Cb > 0 && !b)) TANTE_FAIL(-1, "tante_conv3x3_mfma: null argument");
  if ((const void*)a == (const void*)y || (b && (const void*)b == (const void*)y)) TANTE_FAIL(-1, "tante_conv3x3_mfma: y must not alias a source");
  if ((uintptr_t)packed % 16) TANTE_FAIL(-1, "tante_conv3x3_mfma: the packed weights must be 16-byte aligned");
  if (n_img == 0) return 0;
  const int f = ua_pick(n_img, H, W, Cout);
  UaArgs args;
  args.a = a;
  args.b = Cb > 0 ? b : nullptr;
  args.wp = packed;
  args.shift = shift;
  args.y = y;
  args.Ca = Ca;
  args.Cb = Cb;
  args.Cout = Cout;
  args.H = H;
  args.W = W;
  args.Hs = Hs;
  args.Ws = Ws;
  args.relu = act == TANTE_ACT_RELU ? 1 : 0;
  args.bf16_out = y_dtype == TANTE_BF16 ? 1 : 0;
  args.tiles_x = (W + UA_TW - 1) / UA_TW;
  args.tiles_y = (H + 2 * UA_FORM_RW[f] - 1) / (2 * UA_FORM_RW[f]);
  // 16-byte loads and stores: every row of every tensor starts on 16 bytes
  const bool vec = (Ca % 4 == 0) && (Cb % 4 == 0) && (Cout % 4 == 0) && ((uintptr_t)a % 16 == 0) && (!args.b || (uintptr_t)b % 16 == 0) && ((uintptr_t)y % 16 == 0);
  const bool bf = compute == TANTE_BF16;
  hipStream_t s = (hipStream_t)stream;
  switch (f) {
    case 0: ua_launch<4, 2>(args, n_img, form, bf, vec, s); break;
    case 1: ua_launch<2, 1>(args, n_img, form, bf, vec, s); break;
    default: ua_launch<1, 1>(args, n_img, form, bf, vec, s); break;
  }
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_attn_gate_supported(int64_t M, int Cg, int Cx, int N) { return ag_reason(M, Cg, Cx, N) == nullptr ? 1 : 0; }

extern "C" int64_t tante_attn_gate_stream_bytes(int Cg, int Cx, int N, int compute) {
  if (ag_reason(0, Cg, Cx, N) || (compute != TANTE_F32 && compute != TANTE_BF16)) return -1;
  return ag_stream_bytes(Cg + Cx, N, compute == TANTE_BF16);
}

extern "C" int tante_pack_attn_gate(const float* w, const float* bias, const float* wpsi, float bpsi, int Cg, int Cx, int N, int compute, void* out,
                                    void* stream) {
  if (const char* why = ag_reason(0, Cg, Cx, N)) TANTE_FAIL(-2, "tante_pack_attn_gate: %s (Cg %d, Cx %d, N %d)", why, Cg, Cx, N);
  if (compute != TANTE_F32 && compute != TANTE_BF16) TANTE_FAIL(-1, "tante_pack_attn_gate: compute must be fp32 or bf16");
  if (!w || !bias || !wpsi || !out) TANTE_FAIL(-1, "tante_pack_attn_gate: null argument");
  if ((uintptr_t)out % 16) TANTE_FAIL(-1, "tante_pack_attn_gate: the stream must be 16-byte aligned");
  const bool bf = compute == TANTE_BF16;
  const AgGeom g = ag_geom(Cg + Cx, N, bf);
  const long total = (long)g.NT * g.G * 64 * (bf ? 8 : 4);
  hipLaunchKernelGGL(ag_pack_kernel, dim3((unsigned)((g.frag + total + UA_THREADS - 1) / UA_THREADS)), dim3(UA_THREADS), 0, (hipStream_t)stream, w, bias, wpsi,
                     bpsi, Cg + Cx, N, bf ? 1 : 0, (float*)out, total);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_attn_gate(const float* g, const float* x, int64_t M, int Cg, int Cx, int N, const void* gate_stream, int compute, float* out,
                               void* stream) {
  if (const char* why = ag_reason(M, Cg, Cx, N)) TANTE_FAIL(-2, "tante_attn_gate: %s (rows %lld, Cg %d, Cx %d, N %d)", why, (long long)M, Cg, Cx, N);
  if (compute != TANTE_F32 && compute != TANTE_BF16) TANTE_FAIL(-1, "tante_attn_gate: compute must be fp32 or bf16");
  if (!g || !x || !gate_stream || !out) TANTE_FAIL(-1, "tante_attn_gate: null argument");
  if ((uintptr_t)gate_stream % 16) TANTE_FAIL(-1, "tante_attn_gate: the stream must be 16-byte aligned");
  if (M == 0) return 0;
  const bool bf = compute == TANTE_BF16;
  const bool vec = (Cg % 4 == 0) && (Cx % 4 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)x % 16 == 0) && ((uintptr_t)out % 16 == 0);
  const float* st = (const float*)gate_stream;
  hipStream_t s = (hipStream_t)stream;
  switch (ag_geom(Cg + Cx, N, bf).NT) {
    case 1: ag_launch<1, false>(g, x, M, Cg, Cx, st, bf, vec, out, s); break;
    case 2: ag_launch<2, false>(g, x, M, Cg, Cx, st, bf, vec, out, s); break;
    case 4: ag_launch<1, true>(g, x, M, Cg, Cx, st, bf, vec, out, s); break;
    case 8: ag_launch<2, true>(g, x, M, Cg, Cx, st, bf, vec, out, s); break;
    case 16: ag_launch<4, true>(g, x, M, Cg, Cx, st, bf, vec, out, s); break;
    default: TANTE_FAIL(-2, "tante_attn_gate: coefficients outside 1..256 (N %d)", N);
  }
  TANTE_CHECK_LAUNCH();
  return 0;
}
