// The backward of UNetConvNext's two operations that no shared training node serves (reference models/unet_convnext.py), for a model
// that opted in through UNetConvNext.set_trainable().  fp32 arithmetic, no atomics: every sum has a fixed order that depends only on the
// shape, so two runs give the same bits.
//
// ---- tante_dwconv_ln_bwd: y = LN(dwconv7x7(x) + b) [* ln_w + ln_b]  (Block.forward, unet_convnext.py:136-139) ---------------------------
// Only x is saved by the forward; u = dwconv(x) + b, the statistics and xh = (u - mean) rstd are recomputed by the forward's own stages
// (convnext_stages.hip.h), so they are the forward's bits.  Three launches:
//   A  per tile of the forward's geometry (8 x 8 tokens up to C = 512, 4 x 8 beyond): dw_stage, ln_stage without the affine, then with
//      g = dy ln_w per token  m1 = mean_c g, m2 = mean_c (g xh)  (four lanes per token, two xor shuffles, as ln_stage sums), and per
//      channel  du = rstd (g - m1 - xh m2)  -> the fp32 workspace (n, H, W, C), with the sums over the workgroup's in-image tokens of
//      dy xh, dy and du: a thread owns a channel (and, below 256 channels, a run of tokens; the runs are combined in order).  A workgroup
//      walks the tiles blockIdx.x, + gridDim.x, ... and keeps its channel sums in registers: one partial row (3, C) per workgroup.
//   B  per (walker, 32-channel chunk): du and x of an 8 x 8 tile with their 3-pixel halos in LDS, zeros outside THIS image;
//      dx[p] = sum_t w[t] du[p - (t - 3)]  (the forward's loop with the taps flipped) and
//      d_taps[t] += sum_{p in tile} du[p] x[p + (t - 3)]: a thread owns (channel, tile row) and keeps its 49 sums in registers across the
//      tiles it walks; the eight rows' sums are combined in thread order: one partial row (C, 49) per walker.
//   C  the partial rows summed into d_taps, d_dwbias, d_ln_w, d_ln_b (or added onto them: accumulate): sixteen interleaved slices of the
//      rows, each in workgroup order, then the slices in order.
// At most DLB_CAP workgroups walk in A, at most DLB_CAP / chunks in B, which bounds the partial rows by 512 x 3 x 1024 and
// 512 x 32 x 49 floats whatever the image.
//
// ---- tante_l2norm_rows_bwd: y = x / max(||x||_2, eps)  (F.normalize, unet_convnext.py:69) -------------------------------------------------
// One wave per row.  r = ||x||: r > eps: dx = (dy - y (y . dy)) / r; r <= eps: dx = dy / eps (the clamp passes no gradient to the norm).
#include "common.hip.h"
#include "convnext_stages.hip.h"

namespace {

constexpr int DLB_CAP = 512;               // workgroups that walk tiles (launch A; launch B: per channel chunk, DLB_CAP / chunks)
constexpr int DLB_T = 8;                   // launch B: 8 x 8 tiles
constexpr int DLB_HW = DLB_T + 6;
constexpr int DLB_HALO = DLB_HW * DLB_HW * DL_CH;

__device__ __forceinline__ float ld(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float ld(const __bf16* p, long i) { return (float)p[i]; }

struct DlbPlan {
  int TH, tx, ty, chunks;
  long tiles_a, tiles_b;     // over all images
  int n_a, n_walk;           // workgroups (= partial rows) of launch A, walkers of launch B
  long du, part_a, part_b, total;   // floats
};
DlbPlan dlb_plan(int64_t n_img, int H, int W, int C) {
  DlbPlan p;
  p.TH = dl_th(C);
  p.tx = (W + DL_TW - 1) / DL_TW;
  p.ty = (H + p.TH - 1) / p.TH;
  p.tiles_a = (long)n_img * p.tx * p.ty;
  p.tiles_b = (long)n_img * ((W + DLB_T - 1) / DLB_T) * ((H + DLB_T - 1) / DLB_T);
  p.chunks = (C + DL_CH - 1) / DL_CH;
  p.n_a = (int)(p.tiles_a < DLB_CAP ? p.tiles_a : DLB_CAP);
  const int cap_b = DLB_CAP / p.chunks;
  p.n_walk = (int)(p.tiles_b < cap_b ? p.tiles_b : cap_b);
  p.du = (((long)n_img * H * W * C + 3) / 4) * 4;
  p.part_a = (long)p.n_a * 3 * C;
  p.part_b = (long)p.n_walk * C * 49;
  p.total = p.du + p.part_a + p.part_b;
  return p;
}

// ---- launch A ----------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CN_THREADS) void dlb_a_kernel(const T* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ dw_w,
                                                           const float* __restrict__ dw_b, const float* __restrict__ gw, float* __restrict__ du,
                                                           float* __restrict__ part, int H, int W, int C, int TH, int RS, int tiles_x, int tiles_y,
                                                           long total_tiles, float eps) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int ntok = TH * DL_TW;
  float* rows = lds;
  float* halo = lds + ntok * RS;
  float* stat = halo + (TH + 6) * (DL_TW + 6) * DL_CH;     // rstd, m1, m2 per token
  float* scr = halo;                                        // the token runs' sums (free once dw_stage is through)
  const int tid = threadIdx.x, q = tid & 3;
  const int tiles = tiles_x * tiles_y;
  int TG = C >= CN_THREADS ? 1 : CN_THREADS / C;            // token runs per channel
  if (TG > ntok) TG = ntok;
  const int tpg = (ntok + TG - 1) / TG;
  float acc[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0f;

  for (long tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
    const long img = tile / tiles;
    const int tl = (int)(tile % tiles);
    const int y0 = (tl / tiles_x) * TH, x0 = (tl % tiles_x) * DL_TW;
    dw_stage(x + img * (long)H * W * C, H, W, C, y0, x0, TH, DL_TW, dw_w, 1, 49, dw_b, halo, DL_CH, rows, RS);
    ln_stage<true>(rows, RS, ntok, C, C, eps, nullptr, nullptr, stat);
    // per token: m1 = mean g, m2 = mean g xh
    for (int t0 = 0; t0 < ntok; t0 += CN_THREADS / 4) {
      const int t = t0 + (tid >> 2);
      const int py = y0 + t / DL_TW, px = x0 + t % DL_TW;
      const bool on = t < ntok && py < H && px < W;
      float s1 = 0.0f, s2 = 0.0f;
      if (on) {
        const long o = ((img * H + py) * (long)W + px) * C;
        const float* r = rows + t * RS;
        for (int c = q; c < C; c += 4) {
          float g = ld(dy, o + c);
          if (gw) g *= gw[c];
          s1 += g;
          s2 = fmaf(g, r[c], s2);
        }
      }
      s1 += __shfl_xor(s1, 1);
      s1 += __shfl_xor(s1, 2);
      s2 += __shfl_xor(s2, 1);
      s2 += __shfl_xor(s2, 2);
      if (t < ntok && q == 0) {
        stat[ntok + t] = s1 / (float)C;
        stat[2 * ntok + t] = s2 / (float)C;
      }
    }
    __syncthreads();
    // per channel (and token run): du and the three sums
#pragma unroll
    for (int k = 0; k < 4; ++k) {                             // (below 256 channels C TG <= 256: k = 0 alone)
      const int idx = tid + k * CN_THREADS;
      if (idx >= C * TG) break;
      const int c = idx % C, grp = idx / C;
      const float w = gw ? gw[c] : 1.0f;
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
      const int te = (grp + 1) * tpg < ntok ? (grp + 1) * tpg : ntok;
      for (int t = grp * tpg; t < te; ++t) {
        const int py = y0 + t / DL_TW, px = x0 + t % DL_TW;
        if (py >= H || px >= W) continue;
        const long o = ((img * H + py) * (long)W + px) * C + c;
        const float d = ld(dy, o), xh = rows[t * RS + c];
        const float g = gw ? d * w : d;
        const float v = stat[t] * (g - stat[ntok + t] - xh * stat[2 * ntok + t]);
        du[o] = v;
        s0 = fmaf(d, xh, s0);
        s1 += d;
        s2 += v;
      }
      if (TG == 1) {
        acc[k][0] += s0;
        acc[k][1] += s1;
        acc[k][2] += s2;
      } else {
        scr[idx * 3] = s0;
        scr[idx * 3 + 1] = s1;
        scr[idx * 3 + 2] = s2;
      }
    }
    if (TG > 1) {
      __syncthreads();
      if (tid < C)
        for (int grp = 0; grp < TG; ++grp) {                 // run order
          acc[0][0] += scr[(grp * C + tid) * 3];
          acc[0][1] += scr[(grp * C + tid) * 3 + 1];
          acc[0][2] += scr[(grp * C + tid) * 3 + 2];
        }
    }
  }
  float* pr = part + (long)blockIdx.x * 3 * C;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = tid + k * CN_THREADS;
    if (c < C) {
      pr[c] = acc[k][0];
      pr[C + c] = acc[k][1];
      pr[2 * C + c] = acc[k][2];
    }
  }
}

// ---- launch B ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CN_THREADS) void dlb_b_kernel(const float* __restrict__ du, const float* __restrict__ x, const float* __restrict__ dw_w,
                                                           float* __restrict__ dx, float* __restrict__ tpart, int H, int W, int C, int tiles_x, int tiles_y,
                                                           long total_tiles) {
  __shared__ float lds[2 * DLB_HALO];
  float* hd = lds;
  float* hx = lds + DLB_HALO;
  const int tid = threadIdx.x, c = tid & (DL_CH - 1), ty = tid / DL_CH;
  const int c0 = blockIdx.y * DL_CH;
  const int cn = (C - c0) < DL_CH ? (C - c0) : DL_CH;
  const bool active = c < cn;
  const int tiles = tiles_x * tiles_y;
  float w[49], acc[49];
#pragma unroll
  for (int t = 0; t < 49; ++t) {
    w[t] = active ? dw_w[(long)(c0 + c) * 49 + t] : 0.0f;
    acc[t] = 0.0f;
  }
  for (long tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
    const long img = tile / tiles;
    const int tl = (int)(tile % tiles);
    const int y0 = (tl / tiles_x) * DLB_T, x0 = (tl % tiles_x) * DLB_T;
    const long ibase = img * (long)H * W * C;
    __syncthreads();                                            // the previous tile's reads of the halos are done
    for (int i = tid; i < DLB_HALO; i += CN_THREADS) {
      const int cc = i % DL_CH, p = i / DL_CH;
      const int gy = y0 + p / DLB_HW - 3, gx = x0 + p % DLB_HW - 3;
      float vd = 0.0f, vx = 0.0f;
      if (cc < cn && gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const long o = ibase + ((long)gy * W + gx) * C + c0 + cc;
        vd = du[o];
        vx = x[o];
      }
      hd[i] = vd;
      hx[i] = vx;
    }
    __syncthreads();
    if (!active) continue;                                      // (the trip count is the workgroup's: every thread meets the next barriers)
    float o8[8], d8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      o8[i] = 0.0f;
      d8[i] = hd[((ty + 3) * DLB_HW + i + 3) * DL_CH + c];
    }
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      float r[14];
      const float* hp = hd + ((ty + 6 - a) * DLB_HW) * DL_CH + c;
#pragma unroll
      for (int j = 0; j < 14; ++j) r[j] = hp[j * DL_CH];
#pragma unroll
      for (int b = 0; b < 7; ++b)
#pragma unroll
        for (int i = 0; i < 8; ++i) o8[i] = fmaf(r[i + 6 - b], w[a * 7 + b], o8[i]);
      const float* xp = hx + ((ty + a) * DLB_HW) * DL_CH + c;
#pragma unroll
      for (int j = 0; j < 14; ++j) r[j] = xp[j * DL_CH];
#pragma unroll
      for (int b = 0; b < 7; ++b)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[a * 7 + b] = fmaf(d8[i], r[i + b], acc[a * 7 + b]);
    }
    const int py = y0 + ty;
    if (py < H)
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (x0 + i < W) dx[ibase + ((long)py * W + x0 + i) * C + c0 + c] = o8[i];
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 49; ++t) lds[(ty * DL_CH + c) * 49 + t] = acc[t];
  __syncthreads();
  for (int e = tid; e < DL_CH * 49; e += CN_THREADS) {
    const int cc = e / 49, t = e % 49;
    if (cc >= cn) continue;
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < CN_THREADS / DL_CH; ++r) s += lds[(r * DL_CH + cc) * 49 + t];      // thread order
    tpart[((long)blockIdx.x * C + c0 + cc) * 49 + t] = s;
  }
}

// ---- launch C ----------------------------------------------------------------------------------------------------------------------------
// A workgroup owns DLC_OUT outputs; slice s of DLC_SL sums the rows s, s + DLC_SL, ... in order, then the slices are added in order.
constexpr int DLC_OUT = 16, DLC_SL = CN_THREADS / DLC_OUT;
__global__ __launch_bounds__(CN_THREADS) void dlb_c_kernel(const float* __restrict__ part_a, int n_a, const float* __restrict__ part_b, int n_b, int C,
                                                           float* __restrict__ d_taps, float* __restrict__ d_dwb, float* __restrict__ d_lnw,
                                                           float* __restrict__ d_lnb, int accumulate) {
  __shared__ float red[DLC_SL][DLC_OUT + 1];
  const int o = threadIdx.x % DLC_OUT, sl = threadIdx.x / DLC_OUT;
  const long e = (long)blockIdx.x * DLC_OUT + o;
  const long nt = 49l * C;
  const bool live = e < nt + 3l * C;
  float s = 0.0f;
  if (live) {
    if (e < nt)
      for (int r = sl; r < n_b; r += DLC_SL) s += part_b[r * nt + e];           // walker order within the slice
    else
      for (int r = sl; r < n_a; r += DLC_SL) s += part_a[r * 3l * C + (e - nt)];  // workgroup order within the slice
  }
  red[sl][o] = s;
  __syncthreads();
  if (sl != 0 || !live) return;
  float t = 0.0f;
#pragma unroll
  for (int i = 0; i < DLC_SL; ++i) t += red[i][o];                               // slice order
  float* out;
  if (e < nt) {
    out = d_taps ? d_taps + e : nullptr;
  } else {
    const long k = e - nt;
    const int j = (int)(k / C), c = (int)(k % C);
    float* base = j == 0 ? d_lnw : (j == 1 ? d_lnb : d_dwb);
    out = base ? base + c : nullptr;
  }
  if (out) *out = accumulate ? *out + t : t;
}

TantePerDevice g_dlb_attr[2];

template <typename T>
void dlb_launch(int slot, const void* dy, const float* x, const float* dw_w, const float* dw_b, const float* ln_w, float* dx, float* d_taps, float* d_dwb,
                float* d_lnw, float* d_lnb, int accumulate, float* work, int64_t n_img, int H, int W, int C, float eps, hipStream_t s) {
  const DlbPlan p = dlb_plan(n_img, H, W, C);
  float* du = work;
  float* part_a = work + p.du;
  float* part_b = part_a + p.part_a;
  const int lds = dl_lds(C) + 4 * 3 * p.TH * DL_TW;
  g_dlb_attr[slot].once([] { (void)hipFuncSetAttribute((const void*)dlb_a_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
  hipLaunchKernelGGL(dlb_a_kernel<T>, dim3((unsigned)p.n_a), dim3(CN_THREADS), lds, s, (const T*)dy, x, dw_w, dw_b, ln_w, du, part_a, H, W, C, p.TH, dl_rs(C),
                     p.tx, p.ty, p.tiles_a, eps);
  hipLaunchKernelGGL(dlb_b_kernel, dim3((unsigned)p.n_walk, (unsigned)p.chunks), dim3(CN_THREADS), 0, s, (const float*)du, x, dw_w, dx, part_b, H, W, C,
                     (W + DLB_T - 1) / DLB_T, (H + DLB_T - 1) / DLB_T, p.tiles_b);
  hipLaunchKernelGGL(dlb_c_kernel, dim3((unsigned)((52l * C + DLC_OUT - 1) / DLC_OUT)), dim3(CN_THREADS), 0, s, (const float*)part_a, p.n_a,
                     (const float*)part_b, p.n_walk, C, d_taps, d_dwb, d_lnw, d_lnb, accumulate);
}

// ---- tante_l2norm_rows_bwd: one wave per row -------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CN_THREADS) void l2_bwd_kernel(const T* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, long M, int C,
                                                            float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                                         // wave-uniform
  const int l = threadIdx.x & 63;
  const float* r = x + row * C;
  float s = 0.0f, d = 0.0f;
  for (int c = l; c < C; c += 64) {
    s = fmaf(r[c], r[c], s);
    d = fmaf(r[c], ld(dy, row * C + c), d);
  }
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) {
    s += __shfl_xor(s, k);
    d += __shfl_xor(d, k);
  }
  const float nrm = sqrtf(s);
  if (nrm > eps) {
    const float proj = d / nrm / nrm;                           // (y . dy) / r
    for (int c = l; c < C; c += 64) dx[row * C + c] = (ld(dy, row * C + c) - r[c] * proj) / nrm;
  } else {
    for (int c = l; c < C; c += 64) dx[row * C + c] = ld(dy, row * C + c) / eps;
  }
}

const char* l2b_reason(int64_t M, int C) {
  if (C < 1 || C > (1 << 24)) return "channels outside 1..2^24";
  if (M < 0 || (M + 3) / 4 > 2147483647ll) return "rows outside 0..2^33 - 4";
  return nullptr;
}

}  // namespace

// ================================================================ C ABI ==================================================================
extern "C" int tante_dwconv_ln_bwd_supported(int64_t n_img, int H, int W, int C) { return dl_reason(n_img, H, W, C) == nullptr ? 1 : 0; }

extern "C" int64_t tante_dwconv_ln_bwd_workspace_bytes(int64_t n_img, int H, int W, int C) {
  if (dl_reason(n_img, H, W, C)) return -1;
  return (int64_t)sizeof(float) * dlb_plan(n_img, H, W, C).total;
}

extern "C" int tante_dwconv_ln_bwd(const void* dy, int dy_dtype, const float* x, int64_t n_img, int H, int W, int C, const float* dw_w, const float* dw_b,
                                   float eps, const float* ln_w, float* dx, float* d_taps, float* d_dwbias, float* d_ln_w, float* d_ln_b, int accumulate,
                                   void* work, int64_t work_bytes, void* stream) {
  if (const char* why = dl_reason(n_img, H, W, C))
    TANTE_FAIL(-2, "tante_dwconv_ln_bwd: %s (images %lld, %d x %d, C %d)", why, (long long)n_img, H, W, C);
  if (dy_dtype != TANTE_F32 && dy_dtype != TANTE_BF16) TANTE_FAIL(-1, "tante_dwconv_ln_bwd: dy must be fp32 or bf16");
  if (!dy || !x || !dw_w || !dw_b || !dx) TANTE_FAIL(-1, "tante_dwconv_ln_bwd: null argument");
  if (!ln_w && (d_ln_w || d_ln_b)) TANTE_FAIL(-1, "tante_dwconv_ln_bwd: affine gradients without the affine's weight");
  if ((const void*)dx == dy || dx == x) TANTE_FAIL(-1, "tante_dwconv_ln_bwd: dx may alias neither dy nor x");
  const int64_t need = tante_dwconv_ln_bwd_workspace_bytes(n_img, H, W, C);
  if (n_img > 0 && (!work || work_bytes < need))
    TANTE_FAIL(-1, "tante_dwconv_ln_bwd: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  if (n_img > 0 && (uintptr_t)work % 16) TANTE_FAIL(-1, "tante_dwconv_ln_bwd: the workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (n_img == 0) {      // no tokens: the parameter gradients are zero
    hipLaunchKernelGGL(dlb_c_kernel, dim3((unsigned)((52l * C + DLC_OUT - 1) / DLC_OUT)), dim3(CN_THREADS), 0, s, (const float*)nullptr, 0,
                       (const float*)nullptr, 0, C, d_taps, d_dwbias, d_ln_w, d_ln_b, accumulate);
    TANTE_CHECK_LAUNCH();
    return 0;
  }
  if (dy_dtype == TANTE_BF16)
    dlb_launch<__bf16>(1, dy, x, dw_w, dw_b, ln_w, dx, d_taps, d_dwbias, d_ln_w, d_ln_b, accumulate, (float*)work, n_img, H, W, C, eps, s);
  else
    dlb_launch<float>(0, dy, x, dw_w, dw_b, ln_w, dx, d_taps, d_dwbias, d_ln_w, d_ln_b, accumulate, (float*)work, n_img, H, W, C, eps, s);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_l2norm_rows_bwd_supported(int64_t M, int C) { return l2b_reason(M, C) == nullptr ? 1 : 0; }

extern "C" int tante_l2norm_rows_bwd(const void* dy, int dy_dtype, const float* x, int64_t M, int C, float eps, float* dx, void* stream) {
  if (const char* why = l2b_reason(M, C)) TANTE_FAIL(-2, "tante_l2norm_rows_bwd: %s (rows %lld, C %d)", why, (long long)M, C);
  if (dy_dtype != TANTE_F32 && dy_dtype != TANTE_BF16) TANTE_FAIL(-1, "tante_l2norm_rows_bwd: dy must be fp32 or bf16");
  if (!dy || !x || !dx) TANTE_FAIL(-1, "tante_l2norm_rows_bwd: null argument");
  if (M == 0) return 0;
  const unsigned grid = (unsigned)((M + 3) / 4);
  if (dy_dtype == TANTE_BF16)
    hipLaunchKernelGGL(l2_bwd_kernel<__bf16>, dim3(grid), dim3(CN_THREADS), 0, (hipStream_t)stream, (const __bf16*)dy, x, dx, (long)M, C, eps);
  else
    hipLaunchKernelGGL(l2_bwd_kernel<float>, dim3(grid), dim3(CN_THREADS), 0, (hipStream_t)stream, (const float*)dy, x, dx, (long)M, C, eps);
  TANTE_CHECK_LAUNCH();
  return 0;
}
