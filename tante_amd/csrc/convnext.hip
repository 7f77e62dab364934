// UNetConvNext's operations that no other path of the library serves (reference models/unet_convnext.py): the ConvNeXt block as one
// launch, its first half alone, the token-local part of the channels-first norm, and a direct 3 x 3 convolution for the two edges.
//
// ---- tante_convnext_block: Block.forward (unet_convnext.py:134-148) on x (n_img, H, W, C) fp32 channels-last, out of place --------------
// A workgroup of four waves owns a tile of 8 x 16 pixels of one image (128 tokens, 32 per wave).
//   1  depthwise 7 x 7 + bias.  The tile with its 3-pixel halo (14 x 22 pixels) is staged in LDS in chunks of CH channels (32, 16 at the
//      widest stream) with zeros where the image ends -- the loads are bounded by this image's H and W, the neighbouring image of the
//      batch is never read.  A thread owns a run of 8 pixels of one row for one channel: per tap row it reads 14 values and forms
//      8 x 7 multiply-adds, taps in the order (dy, dx), fp32.  The sums go to the token rows in LDS (fp32, row stride KP + 4 floats).
//   2  LayerNorm over the TRUE C per token, four lanes per token: mean first, then the centred squares, lanes combined by two xor
//      shuffles; the padded channels C .. KP - 1 are written as zeros and never enter a statistic.  The affine is folded into W1 / b1.
//   3  the MLP, transposed so that no hidden value leaves the registers: per step of 32 hidden columns a wave forms
//      h^T (hidden x token) = W1 a^T for its two token tiles (A operand: W1 fragments straight from L2, B operand: the token rows from
//      LDS), adds b1, applies erf GELU, and uses the result registers AS the B operand of y^T (channel x token) += W2 h^T -- the
//      MFMA result layout (register r of lane l = row 4 (l >> 4) + r, column l & 15) is a valid B operand once the packed W2 fragment
//      orders its k index the same way, which tante_pack_convnext does.  fp32 mode: v_mfma_f32_16x16x4_f32; bf16 mode:
//      v_mfma_f32_16x16x32_bf16 with the token rows and the hidden values rounded to bf16 at the operand, fp32 accumulation.
//   4  y = x + (acc + b2) (gamma folded into W2 / b2), fp32, only for pixels inside the image and channels below C.
// No atomics; a token's arithmetic does not depend on where its tile or its image lies.
//
// ---- tante_dwconv_ln: steps 1 and 2 alone, with an optional affine, rows written fp32 or bf16 (the modular route: two tante_gemm follow) --
// ---- tante_l2norm_rows: x / max(||x||_2, eps) per row (F.normalize, unet_convnext.py:69) -----------------------------------------------
// ---- tante_conv3x3: 3 x 3, pad 1, stride 1, either layout in and out, fp32 (unet_convnext.py:227-232) ---------------------------------
#include "common.hip.h"
#include "convnext_stages.hip.h"

namespace {

constexpr int CN_TH = 8, CN_TW = 16;       // the fused kernel's tile
constexpr int CN_MAXC = 256;
constexpr int C3_CO = 16;                  // output channels per workgroup of the 3 x 3 convolution
constexpr int C3_MAXCIN = 128, C3_MAXCOUT = 64;

__device__ __forceinline__ f32x4 mfma32(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- geometry of the packed stream of one block ---------------------------------------------------------------------------------------
struct CnGeom {
  int NT, CP, HP, KPB;          // 16-channel tiles (a power of two), padded C, padded 4 C, the bf16 mode's K of the first product
  long taps, dwb, b1, b2, w1;   // offsets in floats; w2 follows w1
};
__host__ __device__ inline CnGeom cn_geom(int C) {
  CnGeom g;
  int nt = 1;
  while (nt * 16 < C) nt *= 2;
  g.NT = nt;
  g.CP = 16 * nt;
  g.HP = 4 * g.CP;
  g.KPB = g.CP < 32 ? 32 : g.CP;
  g.taps = 0;
  g.dwb = 49l * g.CP;
  g.b1 = g.dwb + g.CP;
  g.b2 = g.b1 + g.HP;
  g.w1 = g.b2 + g.CP;
  return g;
}
inline int64_t cn_stream_bytes(int C) {
  const CnGeom g = cn_geom(C);
  return 4ll * (g.w1 + (long)g.HP * g.KPB + (long)g.HP * g.CP);     // the fp32 form; the bf16 form needs less
}

__global__ __launch_bounds__(CN_THREADS) void cn_pack_kernel(const float* __restrict__ dw_w, const float* __restrict__ dw_b, const float* __restrict__ w1,
                                                             const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, int C,
                                                             int bf, float* __restrict__ out) {
  const CnGeom g = cn_geom(C);
  const int KP = bf ? g.KPB : g.CP;
  const long n1 = (long)g.HP * KP, n2 = (long)g.HP * g.CP;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int H4 = 4 * C;
  if (e < g.w1) {
    float v = 0.0f;
    if (e < g.dwb) {
      const int t = (int)(e / g.CP), c = (int)(e % g.CP);
      if (c < C) v = dw_w[c * 49 + t];
    } else if (e < g.b1) {
      const int c = (int)(e - g.dwb);
      if (c < C) v = dw_b[c];
    } else if (e < g.b2) {
      const int h = (int)(e - g.b1);
      if (h < H4) v = b1[h];
    } else {
      const int c = (int)(e - g.b2);
      if (c < C) v = b2[c];
    }
    out[e] = v;
    return;
  }
  long i = e - g.w1;
  if (i >= n1 + n2) return;
  float v = 0.0f;
  if (!bf) {
    float* dst = out + g.w1;
    if (i < n1) {
      const int s = (int)(i & 3), lane = (int)((i >> 2) & 63);
      const long rest = i >> 8;
      const int gg = (int)(rest % (KP / 16)), ht = (int)(rest / (KP / 16));
      const int row = ht * 16 + (lane & 15), col = 16 * gg + 4 * (lane >> 4) + s;
      if (row < H4 && col < C) v = w1[(long)row * C + col];
    } else {
      const long k = i - n1;
      const int r = (int)(k & 3), lane = (int)((k >> 2) & 63);
      const long rest = k >> 8;
      const int ct = (int)(rest % g.NT), ht = (int)(rest / g.NT);
      const int c = ct * 16 + (lane & 15), hid = ht * 16 + 4 * (lane >> 4) + r;
      if (c < C && hid < H4) v = w2[(long)c * H4 + hid];
    }
    dst[i] = v;
  } else {
    __bf16* dst = (__bf16*)(out + g.w1);
    if (i < n1) {
      const int el = (int)(i & 7), lane = (int)((i >> 3) & 63);
      const long rest = i >> 9;
      const int gg = (int)(rest % (KP / 32)), ht = (int)(rest / (KP / 32));
      const int row = ht * 16 + (lane & 15), col = 32 * gg + 8 * (lane >> 4) + el;
      if (row < H4 && col < C) v = w1[(long)row * C + col];
    } else {
      const long k = i - n1;
      const int el = (int)(k & 7), lane = (int)((k >> 3) & 63);
      const long rest = k >> 9;
      const int ct = (int)(rest % g.NT), hs = (int)(rest / g.NT);
      const int kk = lane >> 4;
      const int c = ct * 16 + (lane & 15), hid = hs * 32 + (el < 4 ? 4 * kk + el : 16 + 4 * kk + (el - 4));
      if (c < C && hid < H4) v = w2[(long)c * H4 + hid];
    }
    dst[i] = (__bf16)v;
  }
}

// ---- the fused block --------------------------------------------------------------------------------------------------------------------
constexpr int cn_ch(int NT) { return NT == 16 ? 16 : 32; }
constexpr int cn_kp(int NT, bool BF) { return (BF && NT == 1) ? 32 : 16 * NT; }
constexpr int cn_lds(int NT, bool BF) {
  return 4 * (CN_TH * CN_TW * (cn_kp(NT, BF) + 4) + (CN_TH + 6) * (CN_TW + 6) * cn_ch(NT));
}

__device__ __forceinline__ u32x4 to_bf16x8(const f32x4& a, const f32x4& b) {
  return u32x4{pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(b[0], b[1]), pack_bf16x2(b[2], b[3])};
}

template <int NT, bool BF>
__global__ __launch_bounds__(CN_THREADS) void cn_block_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ stream, int H, int W,
                                                              int C, int tiles_x, int tiles_y, float eps) {
  constexpr int CP = 16 * NT, HP = 4 * CP, KP = cn_kp(NT, BF), RS = KP + 4, CH = cn_ch(NT);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* rows = lds;
  float* halo = lds + CN_TH * CN_TW * RS;
  const long blk = blockIdx.x;
  const int tiles = tiles_x * tiles_y;
  const long img = blk / tiles;
  const int tile = (int)(blk % tiles);
  const int y0 = (tile / tiles_x) * CN_TH, x0 = (tile % tiles_x) * CN_TW;
  const float* ximg = x + img * (long)H * W * C;
  float* yimg = y + img * (long)H * W * C;
  const CnGeom g = cn_geom(C);

  dw_stage(ximg, H, W, C, y0, x0, CN_TH, CN_TW, stream + g.taps, CP, 1, stream + g.dwb, halo, CH, rows, RS);
  ln_stage(rows, RS, CN_TH * CN_TW, C, KP, eps, nullptr, nullptr);

  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 15, kk = l >> 4;
  const float* a0 = rows + ((2 * wave) * 16 + j) * RS;
  const float* a1 = a0 + 16 * RS;
  const float* b1p = stream + g.b1;
  f32x4 acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[m][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int hs = 0; hs < HP / 32; ++hs) {
    f32x4 h[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int ht = 0; ht < 2; ++ht) h[m][ht] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (!BF) {
      const f32x4* w1f = (const f32x4*)(stream + g.w1);
#pragma unroll 2
      for (int gg = 0; gg < KP / 16; ++gg) {
        const f32x4 t0 = *(const f32x4*)(a0 + 16 * gg + 4 * kk);
        const f32x4 t1 = *(const f32x4*)(a1 + 16 * gg + 4 * kk);
#pragma unroll
        for (int ht = 0; ht < 2; ++ht) {
          const f32x4 w = w1f[((long)(hs * 2 + ht) * (KP / 16) + gg) * 64 + l];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            h[0][ht] = mfma4(w[s], t0[s], h[0][ht]);
            h[1][ht] = mfma4(w[s], t1[s], h[1][ht]);
          }
        }
      }
    } else {
      const u32x4* w1b = (const u32x4*)(stream + g.w1);
#pragma unroll 2
      for (int gg = 0; gg < KP / 32; ++gg) {
        const f32x4* p0 = (const f32x4*)(a0 + 32 * gg + 8 * kk);
        const f32x4* p1 = (const f32x4*)(a1 + 32 * gg + 8 * kk);
        const u32x4 t0 = to_bf16x8(p0[0], p0[1]);
        const u32x4 t1 = to_bf16x8(p1[0], p1[1]);
#pragma unroll
        for (int ht = 0; ht < 2; ++ht) {
          const u32x4 w = w1b[((long)(hs * 2 + ht) * (KP / 32) + gg) * 64 + l];
          h[0][ht] = mfma32(w, t0, h[0][ht]);
          h[1][ht] = mfma32(w, t1, h[1][ht]);
        }
      }
    }
#pragma unroll
    for (int ht = 0; ht < 2; ++ht) {
      const f32x4 bb = *(const f32x4*)(b1p + hs * 32 + ht * 16 + 4 * kk);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        if constexpr (BF) {
          h[m][ht] = gelu_poly4<false>(h[m][ht] + bb);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) h[m][ht][r] = gelu_erf_f(h[m][ht][r] + bb[r]);
        }
      }
    }
    if constexpr (!BF) {
      const f32x4* w2f = (const f32x4*)(stream + g.w1 + (long)HP * KP);
#pragma unroll
      for (int ht = 0; ht < 2; ++ht)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          const f32x4 w = w2f[((long)(hs * 2 + ht) * NT + ct) * 64 + l];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            acc[0][ct] = mfma4(w[r], h[0][ht][r], acc[0][ct]);
            acc[1][ct] = mfma4(w[r], h[1][ht][r], acc[1][ct]);
          }
        }
    } else {
      const u32x4* w2b = (const u32x4*)((const __bf16*)(stream + g.w1) + (long)HP * KP);
      const u32x4 hb0 = to_bf16x8(h[0][0], h[0][1]);
      const u32x4 hb1 = to_bf16x8(h[1][0], h[1][1]);
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const u32x4 w = w2b[((long)hs * NT + ct) * 64 + l];
        acc[0][ct] = mfma32(w, hb0, acc[0][ct]);
        acc[1][ct] = mfma32(w, hb1, acc[1][ct]);
      }
    }
  }

  const float* b2p = stream + g.b2;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int py = y0 + 2 * wave + m, px = x0 + j;
    if (py >= H || px >= W) continue;
    const long base = ((long)py * W + px) * C;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = ct * 16 + 4 * kk + r;
        if (c < C) yimg[base + c] = ximg[base + c] + (acc[m][ct][r] + b2p[c]);
      }
  }
}

TantePerDevice g_cn_attr[10];

template <int NT, bool BF>
void cn_launch(int slot, const float* x, float* y, const float* stream, int64_t n_img, int H, int W, int C, float eps, hipStream_t s) {
  g_cn_attr[slot].once([] { (void)hipFuncSetAttribute((const void*)cn_block_kernel<NT, BF>, hipFuncAttributeMaxDynamicSharedMemorySize, cn_lds(NT, BF)); });
  const int tx = (W + CN_TW - 1) / CN_TW, ty = (H + CN_TH - 1) / CN_TH;
  hipLaunchKernelGGL((cn_block_kernel<NT, BF>), dim3((unsigned)(n_img * tx * ty)), dim3(CN_THREADS), cn_lds(NT, BF), s, x, y, stream, H, W, C, tx, ty, eps);
}

const char* cn_reason(int64_t n_img, int H, int W, int C) {
  if (C < 1 || C > CN_MAXC) return "channels outside 1..256";
  if (H < 1 || W < 1) return "an empty image";
  if (n_img < 0) return "a negative image count";
  const int64_t tiles = (int64_t)((W + CN_TW - 1) / CN_TW) * ((H + CN_TH - 1) / CN_TH);
  if (tiles > 2147483647ll || n_img * tiles > 2147483647ll) return "more than 2^31 - 1 tiles per call";
  return nullptr;
}

// ---- tante_dwconv_ln -------------------------------------------------------------------------------------------------------------------

template <bool BF16_OUT>
__global__ __launch_bounds__(CN_THREADS) void dl_kernel(const float* __restrict__ x, void* __restrict__ y, const float* __restrict__ dw_w,
                                                        const float* __restrict__ dw_b, const float* __restrict__ gw, const float* __restrict__ gb, int H, int W,
                                                        int C, int TH, int RS, int tiles_x, int tiles_y, float eps) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* rows = lds;
  float* halo = lds + TH * DL_TW * RS;
  const long blk = blockIdx.x;
  const int tiles = tiles_x * tiles_y;
  const long img = blk / tiles;
  const int tile = (int)(blk % tiles);
  const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * DL_TW;
  const float* ximg = x + img * (long)H * W * C;
  dw_stage(ximg, H, W, C, y0, x0, TH, DL_TW, dw_w, 1, 49, dw_b, halo, DL_CH, rows, RS);
  ln_stage(rows, RS, TH * DL_TW, C, C, eps, gw, gb);
  const int ntok = TH * DL_TW;
  for (int i = threadIdx.x; i < ntok * C; i += CN_THREADS) {
    const int t = i / C, c = i % C;
    const int py = y0 + t / DL_TW, px = x0 + t % DL_TW;
    if (py >= H || px >= W) continue;
    const long o = ((img * H + py) * (long)W + px) * C + c;
    const float v = rows[t * RS + c];
    if (BF16_OUT) ((__bf16*)y)[o] = (__bf16)v;
    else ((float*)y)[o] = v;
  }
}

TantePerDevice g_dl_attr[2];

// ---- tante_l2norm_rows: one wave per row ---------------------------------------------------------------------------------------------------
template <bool BF16_OUT>
__global__ __launch_bounds__(CN_THREADS) void l2_kernel(const float* __restrict__ x, void* __restrict__ y, long M, int C, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                                         // wave-uniform
  const int l = threadIdx.x & 63;
  const float* r = x + row * C;
  float s = 0.0f;
  for (int c = l; c < C; c += 64) s = fmaf(r[c], r[c], s);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  const float div = fmaxf(sqrtf(s), eps);
  for (int c = l; c < C; c += 64) {
    const float v = r[c] / div;
    if (BF16_OUT) ((__bf16*)y)[row * C + c] = (__bf16)v;
    else ((float*)y)[row * C + c] = v;
  }
}

const char* l2_reason(int64_t M, int C) {
  if (C < 1 || C > (1 << 24)) return "channels outside 1..2^24";
  if (M < 0 || (M + 3) / 4 > 2147483647ll) return "rows outside 0..2^33 - 4";
  return nullptr;
}

// ---- tante_conv3x3 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CN_THREADS) void c3_kernel(const float* __restrict__ x, long xsn, long xsc, long xsh, long xsw, const float* __restrict__ w,
                                                        const float* __restrict__ b, float* __restrict__ y, long ysn, long ysc, long ysh, long ysw, int Cin,
                                                        int Cout, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) float wl[];      // [Cin 9][16]
  const int co0 = blockIdx.y * C3_CO;
  const long img = blockIdx.z;
  for (int i = threadIdx.x; i < Cin * 9 * C3_CO; i += CN_THREADS) {
    const int co = i & (C3_CO - 1), k = i / C3_CO;
    wl[i] = (co0 + co < Cout) ? w[(long)(co0 + co) * Cin * 9 + k] : 0.0f;
  }
  __syncthreads();
  const long p = (long)blockIdx.x * CN_THREADS + threadIdx.x;
  if (p >= (long)H * W) return;
  const int py = (int)(p / W), px = (int)(p % W);
  float acc[C3_CO];
#pragma unroll
  for (int co = 0; co < C3_CO; ++co) acc[co] = (b && co0 + co < Cout) ? b[co0 + co] : 0.0f;
  const float* xi = x + img * xsn;
  for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int gy = py + t / 3 - 1, gx = px + t % 3 - 1;
      float v = 0.0f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xi[ci * xsc + gy * xsh + gx * xsw];
      const f32x4* wp = (const f32x4*)(wl + (ci * 9 + t) * C3_CO);
#pragma unroll
      for (int q = 0; q < C3_CO / 4; ++q) {
        const f32x4 wv = wp[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * q + e] = fmaf(v, wv[e], acc[4 * q + e]);
      }
    }
  }
  float* yo = y + img * ysn + py * ysh + px * ysw;
#pragma unroll
  for (int co = 0; co < C3_CO; ++co)
    if (co0 + co < Cout) yo[(co0 + co) * ysc] = acc[co];
}

TantePerDevice g_c3_attr;

const char* c3_reason(int64_t n_img, int Cin, int Cout, int H, int W) {
  if (Cin < 1 || Cin > C3_MAXCIN) return "input channels outside 1..128";
  if (Cout < 1 || Cout > C3_MAXCOUT) return "output channels outside 1..64";
  if (H < 1 || W < 1) return "an empty image";
  if (n_img < 0 || n_img > 65535) return "images outside 0..65535";
  if (((int64_t)H * W + CN_THREADS - 1) / CN_THREADS > 2147483647ll) return "more than 2^39 pixels per image";
  return nullptr;
}

}  // namespace

// ================================================================ C ABI ==================================================================
extern "C" int tante_convnext_block_supported(int64_t n_img, int H, int W, int C) { return cn_reason(n_img, H, W, C) == nullptr ? 1 : 0; }

extern "C" int64_t tante_convnext_stream_bytes(int C) {
  if (C < 1 || C > CN_MAXC) return -1;
  return cn_stream_bytes(C);
}

extern "C" int tante_pack_convnext(const float* dw_w, const float* dw_b, const float* w1, const float* b1, const float* w2, const float* b2, int C, int compute,
                                   void* out, void* stream) {
  if (C < 1 || C > CN_MAXC) TANTE_FAIL(-2, "tante_pack_convnext: channels outside 1..256 (C %d)", C);
  if (compute != TANTE_F32 && compute != TANTE_BF16) TANTE_FAIL(-1, "tante_pack_convnext: compute must be fp32 or bf16");
  if (!dw_w || !dw_b || !w1 || !b1 || !w2 || !b2 || !out) TANTE_FAIL(-1, "tante_pack_convnext: null argument");
  if ((uintptr_t)out % 16) TANTE_FAIL(-1, "tante_pack_convnext: the stream must be 16-byte aligned");
  const CnGeom g = cn_geom(C);
  const int KP = compute == TANTE_BF16 ? g.KPB : g.CP;
  const long total = g.w1 + (long)g.HP * KP + (long)g.HP * g.CP;
  hipLaunchKernelGGL(cn_pack_kernel, dim3((unsigned)((total + CN_THREADS - 1) / CN_THREADS)), dim3(CN_THREADS), 0, (hipStream_t)stream, dw_w, dw_b, w1, b1, w2,
                     b2, C, compute == TANTE_BF16 ? 1 : 0, (float*)out);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_convnext_block(const float* x, float* y, const void* block_stream, int64_t n_img, int H, int W, int C, int compute, float eps,
                                    void* stream) {
  if (const char* why = cn_reason(n_img, H, W, C))
    TANTE_FAIL(-2, "tante_convnext_block: %s (images %lld, %d x %d, C %d)", why, (long long)n_img, H, W, C);
  if (compute != TANTE_F32 && compute != TANTE_BF16) TANTE_FAIL(-1, "tante_convnext_block: compute must be fp32 or bf16");
  if (!x || !y || !block_stream) TANTE_FAIL(-1, "tante_convnext_block: null argument");
  if (x == y) TANTE_FAIL(-1, "tante_convnext_block: y must not alias x (neighbouring tiles read each other's halo)");
  if ((uintptr_t)block_stream % 16) TANTE_FAIL(-1, "tante_convnext_block: the stream must be 16-byte aligned");
  if (n_img == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const float* st = (const float*)block_stream;
  const int NT = cn_geom(C).NT;
  const bool bf = compute == TANTE_BF16;
#define CN_CASE(nt, slot)                                                      \
  case nt:                                                                     \
    if (bf) cn_launch<nt, true>(slot + 5, x, y, st, n_img, H, W, C, eps, s);   \
    else cn_launch<nt, false>(slot, x, y, st, n_img, H, W, C, eps, s);         \
    break;
  switch (NT) {
    CN_CASE(1, 0)
    CN_CASE(2, 1)
    CN_CASE(4, 2)
    CN_CASE(8, 3)
    CN_CASE(16, 4)
    default: TANTE_FAIL(-2, "tante_convnext_block: channels outside 1..256 (C %d)", C);
  }
#undef CN_CASE
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_dwconv_ln_supported(int64_t n_img, int H, int W, int C) { return dl_reason(n_img, H, W, C) == nullptr ? 1 : 0; }

extern "C" int tante_dwconv_ln(const float* x, int64_t n_img, int H, int W, int C, const float* dw_w, const float* dw_b, float eps, const float* ln_w,
                               const float* ln_b, void* y, int y_dtype, void* stream) {
  if (const char* why = dl_reason(n_img, H, W, C)) TANTE_FAIL(-2, "tante_dwconv_ln: %s (images %lld, %d x %d, C %d)", why, (long long)n_img, H, W, C);
  if (y_dtype != TANTE_F32 && y_dtype != TANTE_BF16) TANTE_FAIL(-1, "tante_dwconv_ln: output dtype must be fp32 or bf16");
  if (!x || !dw_w || !dw_b || !y) TANTE_FAIL(-1, "tante_dwconv_ln: null argument");
  if (ln_b && !ln_w) TANTE_FAIL(-1, "tante_dwconv_ln: the affine takes a weight (and an optional bias)");
  if ((const void*)x == (const void*)y) TANTE_FAIL(-1, "tante_dwconv_ln: y must not alias x");
  if (n_img == 0) return 0;
  const int TH = dl_th(C), RS = dl_rs(C), lds = dl_lds(C);
  const int tx = (W + DL_TW - 1) / DL_TW, ty = (H + TH - 1) / TH;
  hipStream_t s = (hipStream_t)stream;
  if (y_dtype == TANTE_BF16) {
    g_dl_attr[1].once([] { (void)hipFuncSetAttribute((const void*)dl_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    hipLaunchKernelGGL(dl_kernel<true>, dim3((unsigned)(n_img * tx * ty)), dim3(CN_THREADS), lds, s, x, y, dw_w, dw_b, ln_w, ln_b, H, W, C, TH, RS, tx, ty, eps);
  } else {
    g_dl_attr[0].once([] { (void)hipFuncSetAttribute((const void*)dl_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    hipLaunchKernelGGL(dl_kernel<false>, dim3((unsigned)(n_img * tx * ty)), dim3(CN_THREADS), lds, s, x, y, dw_w, dw_b, ln_w, ln_b, H, W, C, TH, RS, tx, ty, eps);
  }
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_l2norm_rows_supported(int64_t M, int C) { return l2_reason(M, C) == nullptr ? 1 : 0; }

extern "C" int tante_l2norm_rows(const float* x, int64_t M, int C, float eps, void* y, int y_dtype, void* stream) {
  if (const char* why = l2_reason(M, C)) TANTE_FAIL(-2, "tante_l2norm_rows: %s (rows %lld, C %d)", why, (long long)M, C);
  if (y_dtype != TANTE_F32 && y_dtype != TANTE_BF16) TANTE_FAIL(-1, "tante_l2norm_rows: output dtype must be fp32 or bf16");
  if (!x || !y) TANTE_FAIL(-1, "tante_l2norm_rows: null argument");
  if (M == 0) return 0;
  const unsigned grid = (unsigned)((M + 3) / 4);
  if (y_dtype == TANTE_BF16) hipLaunchKernelGGL(l2_kernel<true>, dim3(grid), dim3(CN_THREADS), 0, (hipStream_t)stream, x, y, (long)M, C, eps);
  else hipLaunchKernelGGL(l2_kernel<false>, dim3(grid), dim3(CN_THREADS), 0, (hipStream_t)stream, x, y, (long)M, C, eps);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_conv3x3_supported(int64_t n_img, int Cin, int Cout, int H, int W) { return c3_reason(n_img, Cin, Cout, H, W) == nullptr ? 1 : 0; }

extern "C" int tante_conv3x3(const float* x, int64_t n_img, int Cin, int H, int W, int in_nchw, const float* w, const float* bias, int Cout, float* y,
                             int out_nchw, void* stream) {
  if (const char* why = c3_reason(n_img, Cin, Cout, H, W))
    TANTE_FAIL(-2, "tante_conv3x3: %s (images %lld, Cin %d, Cout %d, %d x %d)", why, (long long)n_img, Cin, Cout, H, W);
  if (!x || !w || !y) TANTE_FAIL(-1, "tante_conv3x3: null argument");
  if (n_img == 0) return 0;
  const long HW = (long)H * W;
  const long xsn = HW * Cin, xsc = in_nchw ? HW : 1, xsh = in_nchw ? W : (long)W * Cin, xsw = in_nchw ? 1 : Cin;
  const long ysn = HW * Cout, ysc = out_nchw ? HW : 1, ysh = out_nchw ? W : (long)W * Cout, ysw = out_nchw ? 1 : Cout;
  g_c3_attr.once([] { (void)hipFuncSetAttribute((const void*)c3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, C3_MAXCIN * 9 * C3_CO * 4); });
  hipLaunchKernelGGL(c3_kernel, dim3((unsigned)((HW + CN_THREADS - 1) / CN_THREADS), (unsigned)((Cout + C3_CO - 1) / C3_CO), (unsigned)n_img), dim3(CN_THREADS),
                     Cin * 9 * C3_CO * 4, (hipStream_t)stream, x, xsn, xsc, xsh, xsw, w, bias, y, ysn, ysc, ysh, ysw, Cin, Cout, H, W);
  TANTE_CHECK_LAUNCH();
  return 0;
}
