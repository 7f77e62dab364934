// AViT's operations that no other path of the library serves (reference models/avit.py): the two instance norms over the token plane,
// axial attention along W and H from one q, k, v, attention over the T steps of a token with an additive bias, and the per-sample field
// statistics taken before the stem and undone after the head.
//
// ---- tante_instnorm: RMSInstanceNorm2d (avit.py:125-139) / nn.InstanceNorm2d(affine) (avit.py:292-293) on x (n_img, HW, C) fp32 --------
// Statistics per (image, channel) run over the HW tokens.  A lane owns a channel (64 channels per workgroup: the rows are read
// coalesced), the four waves take the rows of a slab in turn.  The rows are cut into S <= 64 slabs; launch 1 computes per slab the mean
// FIRST and then the centred sum of squares about that mean (never E[x^2] - mean^2); launch 2 combines the slabs' (n, mean, M2) in slab
// order with the pairwise update  mean += d n_i / n,  M2 += M2_i + d^2 n_old n_i / n  (exact for a partition), normalises, applies the
// weight (and the bias of the instance form), an optional activation, and the optional epilogue  out = residual + gamma[c] * value.
// Every sum has a fixed order: a thread's rows in order, the four waves in order, the slabs in order; no atomics.
//
// ---- tante_axial_attention: AxialAttentionBlock.forward's middle (avit.py:257-273) on the qkv rows (n_img H W, 3 E) fp32 ----------------
// Channel order as the reference's input_head leaves it: (head, [q | k | v], hd).  One workgroup owns one line (a row of W tokens in
// pass 0, a column of H tokens in pass 1) of one head: it loads q, k, v of the line into LDS, applies the q / k LayerNorm (mean first,
// centred variance, one thread per vector), forms the L x L logits and then P V on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32
// accumulation, in both compute modes), with the softmax between them in fp32 with the row maximum subtracted.  Pass 0 stores its result,
// pass 1 stores (stored + result) / 2.  A operand lane (i = l & 15, k = l >> 4), B operand lane (k = l >> 4, j = l & 15), result register
// r = row 4 (l >> 4) + r, column l & 15.  LDS is plain C++ between barriers: no hand-placed waits.
//
// ---- tante_time_attention: AttentionBlock.forward's middle (avit.py:317-326) on rows ordered ((t b), h, w) ------------------------------
// One sequence of T <= 16 steps per (b, token, head).  A workgroup stages floor(64 / T) sequences of one head in LDS, normalises q and k
// there, and one lane per query row forms its T logits (+ bias[head, tq, tk]), the softmax and the weighted sum of v.
//
// ---- tante_field_stats / tante_field_affine: avit.py:423-426, 448 ----------------------------------------------------------------------
// Mean and unbiased std over (t, h, w) per (b, c) of the b t c h w batch, with the same mean-then-centred, fixed-order rules (lanes by
// shuffle, waves in order, slabs in order); eps is added to the std.  The normalised batch is written channels-last with images ordered
// (t b); the affine kernel undoes it on the head's (t b)-ordered channels-first images and writes b t c h w.
#include "common.hip.h"

namespace {

constexpr int AV_THREADS = 256;
constexpr int IN_STRIP = 64;               // channels per workgroup of the instance norms
constexpr int IN_MAX_HW = 4096;
constexpr int IN_SLABS = 64;               // slabs per image at most
constexpr int IN_MIN_ROWS = 32;            // rows a slab aims for at least
constexpr int AX_MAX = 64;                 // tokens per axis
constexpr int TM_MAX_T = 16;               // time steps
constexpr int TM_THREADS = 128;
constexpr int TM_TOK = 64;                 // tokens a workgroup of the time kernel stages
constexpr int FS_SLAB = 4096;              // elements a slab of the field statistics aims for
constexpr int FS_SLABS = 64;

// ================================================================ instance norms ========================================================
struct InPlan {
  int R, S, strips;      // rows per slab, slabs, 64-channel strips
};

InPlan in_plan(int HW, int C) {
  InPlan p;
  int R = (HW + IN_SLABS - 1) / IN_SLABS;
  if (R < IN_MIN_ROWS) R = IN_MIN_ROWS;
  if (R > HW) R = HW;
  p.R = R;
  p.S = (HW + R - 1) / R;
  p.strips = (C + IN_STRIP - 1) / IN_STRIP;
  return p;
}

const char* in_reason(int64_t n_img, int HW, int C) {
  if (HW < 2 || HW > IN_MAX_HW) return "tokens per image outside 2..4096";
  if (C < 1 || C > (1 << 24)) return "channels outside 1..2^24";
  if (n_img < 0 || n_img * (int64_t)((C + IN_STRIP - 1) / IN_STRIP) > 2147483647ll) return "more than 2^31 - 1 (image, channel strip) pairs per call";
  return nullptr;
}

__global__ __launch_bounds__(AV_THREADS) void in_stats_kernel(const float* __restrict__ x, float* __restrict__ part, int HW, int C, int strips, int R,
                                                              int S) {
  __shared__ float red[4][IN_STRIP];
  const long bs = blockIdx.x;
  const int s = blockIdx.y;
  const long img = bs / strips;
  const int strip = (int)(bs % strips);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = strip * IN_STRIP + lane;
  const bool on = c < C;
  const int r0 = s * R;
  const int nr = (HW - r0) < R ? (HW - r0) : R;
  const float* base = x + (img * HW + r0) * (long)C + c;
  float a = 0.0f;
  if (on)
    for (int r = wv; r < nr; r += 4) a += base[(long)r * C];
  red[wv][lane] = a;
  __syncthreads();
  const float mean = ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) / (float)nr;
  __syncthreads();
  float q = 0.0f;
  if (on)
    for (int r = wv; r < nr; r += 4) {
      const float d = base[(long)r * C] - mean;
      q += d * d;
    }
  red[wv][lane] = q;
  __syncthreads();
  if (wv == 0 && on) {
    float* p = part + ((img * S + s) * 2) * (long)C + c;
    p[0] = mean;
    p[C] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  }
}

template <bool RMS, bool BF16_OUT>
__global__ __launch_bounds__(AV_THREADS) void in_apply_kernel(const float* __restrict__ x, const float* __restrict__ part, const float* __restrict__ weight,
                                                              const float* __restrict__ bias, int act, const float* residual,
                                                              const float* __restrict__ gamma, void* y, int HW, int C, int strips, int R, int S,
                                                              float eps) {
  const long bs = blockIdx.x;
  const int s = blockIdx.y;
  const long img = bs / strips;
  const int strip = (int)(bs % strips);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = strip * IN_STRIP + lane;
  if (c >= C) return;
  // every thread combines its channel's slabs in slab order
  float cnt = 0.0f, mean = 0.0f, m2 = 0.0f;
  for (int i = 0; i < S; ++i) {
    const int nri = (HW - i * R) < R ? (HW - i * R) : R;
    const float ni = (float)nri;
    const float* p = part + ((img * S + i) * 2) * (long)C + c;
    const float mi = p[0], qi = p[C];
    const float d = mi - mean, nn = cnt + ni;
    mean += d * (ni / nn);
    m2 += qi + d * d * (cnt * (ni / nn));
    cnt = nn;
  }
  const float wv_ = weight ? weight[c] : 1.0f;
  const float bv = (!RMS && bias) ? bias[c] : 0.0f;
  const float gv = gamma ? gamma[c] : 0.0f;
  const float div = RMS ? (sqrtf(m2 / (cnt - 1.0f)) + eps) : sqrtf(m2 / cnt + eps);
  const int r0 = s * R;
  const int nr = (HW - r0) < R ? (HW - r0) : R;
  const long off = (img * HW + r0) * (long)C + c;
  for (int r = wv; r < nr; r += 4) {
    const long o = off + (long)r * C;
    float v = RMS ? (x[o] / div) * wv_ : ((x[o] - mean) / div) * wv_ + bv;
    if (act != TANTE_ACT_NONE) v = apply_act(v, act);
    if (residual) v = fmaf(gv, v, residual[o]);
    if (BF16_OUT)
      ((__bf16*)y)[o] = (__bf16)v;
    else
      ((float*)y)[o] = v;
  }
}

// ================================================================ q / k LayerNorm in LDS ================================================
// one thread normalises one vector of HD floats in place: mean first, then the centred (biased) variance, eps inside the root
template <int HD>
__device__ __forceinline__ void ln_vec(float* p, const float* __restrict__ w, const float* __restrict__ b, float eps) {
  float s = 0.0f;
  for (int c = 0; c < HD; ++c) s += p[c];
  const float mean = s / (float)HD;
  float q = 0.0f;
  for (int c = 0; c < HD; ++c) {
    const float d = p[c] - mean;
    q += d * d;
  }
  const float rstd = 1.0f / sqrtf(q / (float)HD + eps);
  for (int c = 0; c < HD; ++c) p[c] = (p[c] - mean) * rstd * w[c] + b[c];
}

// ================================================================ axial attention =======================================================
const char* ax_reason(int64_t n_img, int heads, int H, int W, int hd) {
  if (H < 1 || H > AX_MAX || W < 1 || W > AX_MAX) return "token axes outside 1..64";
  if (hd != 16 && hd != 32 && hd != 64) return "head dim not one of 16, 32, 64";
  if (heads < 1 || heads > 65535) return "heads outside 1..65535";
  if (n_img < 0 || n_img * (int64_t)(H > W ? H : W) > 2147483647ll) return "more than 2^31 - 1 lines per call";
  return nullptr;
}

inline int ax_lds_bytes(int L, int hd) {
  const int Lp = (L + 15) & ~15;
  return (3 * Lp * (hd + 4) + Lp * (Lp + 4)) * (int)sizeof(float);
}

template <int HD>
__global__ __launch_bounds__(AV_THREADS) void axial_kernel(const float* __restrict__ qkv, const float* __restrict__ qw, const float* __restrict__ qb,
                                                           const float* __restrict__ kw, const float* __restrict__ kb, float* out, int H, int W, int E,
                                                           int pass, float eps, float scale) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int LD = HD + 4;
  const int L = pass ? H : W;
  const int Lp = (L + 15) & ~15;
  const int LS = Lp + 4;
  float* Qs = lds;
  float* Ks = Qs + Lp * LD;
  float* Vs = Ks + Lp * LD;
  float* Ss = Vs + Lp * LD;
  const long line = blockIdx.x;
  const int head = blockIdx.y;
  const int tid = threadIdx.x;
  long tok0, step;
  if (!pass) {
    tok0 = line * W;           // line = img H + h
    step = 1;
  } else {
    tok0 = (line / W) * (long)H * W + line % W;      // line = img W + w
    step = W;
  }
  const long ld3 = 3L * E;
  // 16-byte loads, four in flight per thread before the first LDS store (a token's q | k | v of one head are 3 HD contiguous floats)
  constexpr int V4 = 3 * HD / 4;
  for (int base = 0; base < Lp * V4; base += 4 * AV_THREADS) {
    f32x4 r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * AV_THREADS + tid, tok = idx / V4;
      r[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (idx < Lp * V4 && tok < L) r[u] = *(const f32x4*)(qkv + (tok0 + tok * step) * ld3 + (long)head * 3 * HD + 4 * (idx % V4));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * AV_THREADS + tid, tok = idx / V4, j = 4 * (idx % V4), which = j / HD, c = j % HD;
      if (idx < Lp * V4) *(f32x4*)((which == 0 ? Qs : which == 1 ? Ks : Vs) + tok * LD + c) = r[u];
    }
  }
  __syncthreads();
  if (tid < 2 * L) {
    const int tok = tid >> 1;
    if (tid & 1)
      ln_vec<HD>(Ks + tok * LD, kw, kb, eps);
    else
      ln_vec<HD>(Qs + tok * LD, qw, qb, eps);
  }
  __syncthreads();
  const int nT = Lp >> 4;
  const int lane = tid & 63, wv = tid >> 6, i = lane & 15, kk = lane >> 4;
  // logits: tile (ti, tj) = Q rows of tile ti against K rows of tile tj, K = HD
  for (int t = wv; t < nT * nT; t += 4) {
    const int ti = t / nT, tj = t % nT;
    const float* a = Qs + (ti * 16 + i) * LD + kk;
    const float* b = Ks + (tj * 16 + i) * LD + kk;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < HD; k0 += 4) acc = mfma4(a[k0], b[k0], acc);
    for (int r = 0; r < 4; ++r) Ss[(ti * 16 + 4 * kk + r) * LS + tj * 16 + i] = acc[r] * scale;
  }
  __syncthreads();
  if (tid < L) {
    float* p = Ss + tid * LS;
    float m = p[0];
    for (int j = 1; j < L; ++j) m = fmaxf(m, p[j]);
    float s = 0.0f;
    for (int j = 0; j < L; ++j) {
      const float e = expf(p[j] - m);
      p[j] = e;
      s += e;
    }
    const float inv = 1.0f / s;
    for (int j = 0; j < L; ++j) p[j] *= inv;
    for (int j = L; j < Lp; ++j) p[j] = 0.0f;
  }
  __syncthreads();
  // P V: tile (ti, tc) = probability rows of tile ti against 16 columns of V, K = Lp (the padding of both is zero)
  constexpr int nC = HD / 16;
  for (int t = wv; t < nT * nC; t += 4) {
    const int ti = t / nC, tc = t % nC;
    const float* a = Ss + (ti * 16 + i) * LS + kk;
    const float* b = Vs + kk * LD + tc * 16 + i;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < Lp; k0 += 4) acc = mfma4(a[k0], b[k0 * LD], acc);
    for (int r = 0; r < 4; ++r) {
      const int row = ti * 16 + 4 * kk + r;
      if (row < L) {
        float* o = out + (tok0 + row * step) * (long)E + (long)head * HD + tc * 16 + i;
        *o = pass ? (*o + acc[r]) * 0.5f : acc[r];
      }
    }
  }
}

TantePerDevice g_ax_attr[3];

template <int HD>
void ax_launch(int idx, const float* qkv, const float* qw, const float* qb, const float* kw, const float* kb, float* out, int64_t n_img, int heads,
               int H, int W, float eps, hipStream_t s) {
  g_ax_attr[idx].once([] { (void)hipFuncSetAttribute((const void*)axial_kernel<HD>, hipFuncAttributeMaxDynamicSharedMemorySize, ax_lds_bytes(AX_MAX, HD)); });
  const int E = heads * HD;
  const float scale = 1.0f / sqrtf((float)HD);
  hipLaunchKernelGGL(axial_kernel<HD>, dim3((unsigned)(n_img * H), heads), dim3(AV_THREADS), ax_lds_bytes(W, HD), s, qkv, qw, qb, kw, kb, out, H, W, E,
                     0, eps, scale);
  hipLaunchKernelGGL(axial_kernel<HD>, dim3((unsigned)(n_img * W), heads), dim3(AV_THREADS), ax_lds_bytes(H, HD), s, qkv, qw, qb, kw, kb, out, H, W, E,
                     1, eps, scale);
}

// ================================================================ time attention ========================================================
const char* tm_reason(int64_t nseq, int T, int heads, int hd) {
  if (T < 1 || T > TM_MAX_T) return "time steps outside 1..16";
  if (hd != 16 && hd != 32 && hd != 64) return "head dim not one of 16, 32, 64";
  if (heads < 1 || heads > 65535) return "heads outside 1..65535";
  if (nseq < 0 || nseq > 2147483647ll) return "more than 2^31 - 1 sequences per call";
  return nullptr;
}

template <int HD>
__global__ __launch_bounds__(TM_THREADS) void time_kernel(const float* __restrict__ qkv, const float* __restrict__ qw, const float* __restrict__ qb,
                                                          const float* __restrict__ kw, const float* __restrict__ kb, const float* __restrict__ bias,
                                                          float* __restrict__ out, long nseq, int T, int E, int spw, float eps, float scale) {
  constexpr int LDT = 3 * HD + 1;          // odd: the per-token serial loops of neighbouring lanes fall on different banks
  constexpr int LDL = TM_MAX_T + 1;
  __shared__ float buf[TM_TOK * LDT];
  __shared__ float lg[TM_TOK * LDL];
  const int head = blockIdx.y;
  const int tid = threadIdx.x;
  const long seq0 = (long)blockIdx.x * spw;
  const int ns = (nseq - seq0) < spw ? (int)(nseq - seq0) : spw;
  const int ntok = ns * T;                  // <= 64
  const long ld3 = 3L * E;
  // 16-byte loads, eight in flight per thread before the first LDS store (a token's q | k | v of one head are 3 HD contiguous floats)
  constexpr int V4 = 3 * HD / 4;
  for (int base = 0; base < ntok * V4; base += 8 * TM_THREADS) {
    f32x4 r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * TM_THREADS + tid, tok = idx / V4;
      r[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (idx < ntok * V4) r[u] = *(const f32x4*)(qkv + ((long)(tok % T) * nseq + seq0 + tok / T) * ld3 + (long)head * 3 * HD + 4 * (idx % V4));
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * TM_THREADS + tid;
      if (idx < ntok * V4) {
        float* d = buf + (idx / V4) * LDT + 4 * (idx % V4);
        d[0] = r[u][0], d[1] = r[u][1], d[2] = r[u][2], d[3] = r[u][3];
      }
    }
  }
  __syncthreads();
  if (tid < 2 * ntok) {
    const int tok = tid >> 1;
    if (tid & 1)
      ln_vec<HD>(buf + tok * LDT + HD, kw, kb, eps);
    else
      ln_vec<HD>(buf + tok * LDT, qw, qb, eps);
  }
  __syncthreads();
  if (tid < ntok) {
    const int sq = tid / T, tq = tid % T;
    float* q = buf + tid * LDT;
    float* l = lg + tid * LDL;
    const float* bq = bias + ((long)head * T + tq) * T;
    float m = -INFINITY;
    for (int tk = 0; tk < T; ++tk) {
      const float* kp = buf + (sq * T + tk) * LDT + HD;
      float d = 0.0f;
      for (int c = 0; c < HD; ++c) d += q[c] * kp[c];
      d = d * scale + bq[tk];
      l[tk] = d;
      m = fmaxf(m, d);
    }
    float s = 0.0f;
    for (int tk = 0; tk < T; ++tk) {
      const float e = expf(l[tk] - m);
      l[tk] = e;
      s += e;
    }
    const float inv = 1.0f / s;
    for (int tk = 0; tk < T; ++tk) l[tk] *= inv;
    // the result takes the place of this row's q, which nothing reads any more
    for (int c = 0; c < HD; ++c) {
      float a = 0.0f;
      for (int tk = 0; tk < T; ++tk) a += l[tk] * buf[(sq * T + tk) * LDT + 2 * HD + c];
      q[c] = a;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < ntok * HD; idx += TM_THREADS) {
    const int tok = idx / HD, c = idx % HD;
    const long row = (long)(tok % T) * nseq + seq0 + tok / T;
    out[row * (long)E + (long)head * HD + c] = buf[tok * LDT + c];
  }
}

template <int HD>
void tm_launch(const float* qkv, const float* qw, const float* qb, const float* kw, const float* kb, const float* bias, float* out, int64_t nseq, int T,
               int heads, float eps, hipStream_t s) {
  const int spw = TM_TOK / T;
  const int64_t wgs = (nseq + spw - 1) / spw;
  hipLaunchKernelGGL(time_kernel<HD>, dim3((unsigned)wgs, heads), dim3(TM_THREADS), 0, s, qkv, qw, qb, kw, kb, bias, out, (long)nseq, T, heads * HD, spw,
                     eps, 1.0f / sqrtf((float)HD));
}

// ================================================================ field statistics ======================================================
struct FsPlan {
  int64_t n, SZ;
  int S;
};

FsPlan fs_plan(int T, int64_t HW) {
  FsPlan p;
  p.n = (int64_t)T * HW;
  p.SZ = (p.n + FS_SLABS - 1) / FS_SLABS;
  if (p.SZ < FS_SLAB) p.SZ = FS_SLAB;
  p.S = (int)((p.n + p.SZ - 1) / p.SZ);
  return p;
}

const char* fs_reason(int64_t B, int T, int C, int64_t HW) {
  if (T < 1 || HW < 1 || C < 1) return "an empty axis";
  if ((int64_t)T * HW < 2) return "fewer than two values per (sample, field)";
  if ((int64_t)T * HW > (1ll << 30)) return "more than 2^30 values per (sample, field)";
  if (B < 0 || B * (int64_t)C > 2147483647ll) return "more than 2^31 - 1 (sample, field) pairs per call";
  if (B * (int64_t)C * T * HW > (1ll << 38)) return "more than 2^38 values per call";
  return nullptr;
}

const char* fa_reason(int64_t B, int Tk, int C, int64_t HW) {
  if (Tk < 1 || HW < 1 || C < 1) return "an empty axis";
  if (B < 0 || B * (int64_t)C > 2147483647ll) return "more than 2^31 - 1 (sample, field) pairs per call";
  if (HW > (1ll << 38) || (int64_t)Tk * HW > (1ll << 38) || (B * C > 0 && (int64_t)Tk * HW > (1ll << 38) / (B * C))) return "more than 2^38 values per call";
  return nullptr;
}

// the sum of v over the 256 threads, the same value in every thread: lanes by shuffle, then the four waves in order
__device__ __forceinline__ float fs_block_sum(float v, float* s) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s[0] + s[1]) + (s[2] + s[3]);
}

__global__ __launch_bounds__(AV_THREADS) void fs_stats_kernel(const float* __restrict__ x, float* __restrict__ part, int T, int C, long HW, long n, long SZ,
                                                              int S) {
  __shared__ float red[4];
  const long bc = blockIdx.x;
  const int s = blockIdx.y;
  const long b = bc / C;
  const int c = (int)(bc % C);
  const long e0 = s * SZ;
  const long ne = (n - e0) < SZ ? (n - e0) : SZ;
  const float* base = x + (b * T * C + c) * HW;      // element e = (t, p) lies at base[t C HW + p]
  float a = 0.0f;
  for (long e = threadIdx.x; e < ne; e += AV_THREADS) {
    const long g = e0 + e;
    a += base[(g / HW) * C * HW + g % HW];
  }
  const float mean = fs_block_sum(a, red) / (float)ne;
  float q = 0.0f;
  for (long e = threadIdx.x; e < ne; e += AV_THREADS) {
    const long g = e0 + e;
    const float d = base[(g / HW) * C * HW + g % HW] - mean;
    q += d * d;
  }
  const float m2 = fs_block_sum(q, red);
  if (threadIdx.x == 0) {
    part[(bc * S + s) * 2] = mean;
    part[(bc * S + s) * 2 + 1] = m2;
  }
}

__global__ void fs_combine_kernel(const float* __restrict__ part, float* __restrict__ stats, long BC, long n, long SZ, int S, float eps) {
  const long bc = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (bc >= BC) return;
  float cnt = 0.0f, mean = 0.0f, m2 = 0.0f;
  for (int i = 0; i < S; ++i) {
    const long nei = (n - i * SZ) < SZ ? (n - i * SZ) : SZ;
    const float ni = (float)nei;
    const float mi = part[(bc * S + i) * 2], qi = part[(bc * S + i) * 2 + 1];
    const float d = mi - mean, nn = cnt + ni;
    mean += d * (ni / nn);
    m2 += qi + d * d * (cnt * (ni / nn));
    cnt = nn;
  }
  stats[bc * 2] = mean;
  stats[bc * 2 + 1] = sqrtf(m2 / (cnt - 1.0f)) + eps;
}

// xn ((t b), HW, C) = (x (b, t, C, HW) - mean[b, c]) / std[b, c]
__global__ __launch_bounds__(AV_THREADS) void fs_norm_kernel(const float* __restrict__ x, const float* __restrict__ stats, float* __restrict__ xn, long B, int T,
                                                             int C, long HW, long total) {
  const long idx = (long)blockIdx.x * AV_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long p = (idx / C) % HW;
  const long tb = idx / ((long)C * HW);
  const long t = tb / B, b = tb % B;
  const float* st = stats + (b * C + c) * 2;
  xn[idx] = (x[((b * T + t) * C + c) * HW + p] - st[0]) / st[1];
}

// out (b, Tk, C, HW) = y ((t b), C, HW) * std[b, c] + mean[b, c]
__global__ __launch_bounds__(AV_THREADS) void fs_affine_kernel(const float* __restrict__ y, const float* __restrict__ stats, float* __restrict__ out, long B,
                                                               int Tk, int C, long HW, long total) {
  const long idx = (long)blockIdx.x * AV_THREADS + threadIdx.x;
  if (idx >= total) return;
  const long p = idx % HW;
  const int c = (int)((idx / HW) % C);
  const long bt = idx / ((long)C * HW);
  const long b = bt / Tk, t = bt % Tk;
  const float* st = stats + (b * C + c) * 2;
  out[idx] = y[((t * B + b) * C + c) * HW + p] * st[1] + st[0];
}

}  // namespace

// ================================================================ entry points ==========================================================
extern "C" int tante_instnorm_supported(int64_t n_img, int HW, int C) { return in_reason(n_img, HW, C) == nullptr ? 1 : 0; }

extern "C" int64_t tante_instnorm_workspace_bytes(int64_t n_img, int HW, int C) {
  if (in_reason(n_img, HW, C)) return -1;
  const InPlan p = in_plan(HW, C);
  return n_img * p.S * 2 * (int64_t)C * (int64_t)sizeof(float);
}

extern "C" int tante_instnorm(const float* x, int64_t n_img, int HW, int C, int form, float eps, const float* weight, const float* bias, int act,
                              const float* residual, const float* gamma, void* y, int y_dtype, void* work, int64_t work_bytes, void* stream) {
  if (const char* why = in_reason(n_img, HW, C)) TANTE_FAIL(-2, "tante_instnorm: %s (images %lld, tokens %d, C %d)", why, (long long)n_img, HW, C);
  if (form != TANTE_INSTNORM_INSTANCE && form != TANTE_INSTNORM_RMS) TANTE_FAIL(-1, "tante_instnorm: form must be instance (0) or rms (1)");
  if (y_dtype != TANTE_F32 && y_dtype != TANTE_BF16) TANTE_FAIL(-1, "tante_instnorm: output dtype must be fp32 or bf16");
  if (act < TANTE_ACT_NONE || act > TANTE_ACT_RELU) TANTE_FAIL(-1, "tante_instnorm: unknown activation %d", act);
  if ((residual == nullptr) != (gamma == nullptr)) TANTE_FAIL(-1, "tante_instnorm: the epilogue takes residual and gamma together");
  if (!x || !y) TANTE_FAIL(-1, "tante_instnorm: null argument");
  if (n_img == 0) return 0;
  const int64_t need = tante_instnorm_workspace_bytes(n_img, HW, C);
  if (!work || work_bytes < need) TANTE_FAIL(-1, "tante_instnorm: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  const InPlan p = in_plan(HW, C);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(n_img * p.strips), p.S);
  hipLaunchKernelGGL(in_stats_kernel, grid, dim3(AV_THREADS), 0, s, x, (float*)work, HW, C, p.strips, p.R, p.S);
  TANTE_CHECK_LAUNCH();
#define IN_APPLY(RMS_, BF_)                                                                                                                     \
  hipLaunchKernelGGL((in_apply_kernel<RMS_, BF_>), grid, dim3(AV_THREADS), 0, s, x, (const float*)work, weight, bias, act, residual, gamma, y, HW, C, \
                     p.strips, p.R, p.S, eps)
  const bool rms = form == TANTE_INSTNORM_RMS, bf = y_dtype == TANTE_BF16;
  if (rms && bf) IN_APPLY(true, true);
  else if (rms) IN_APPLY(true, false);
  else if (bf) IN_APPLY(false, true);
  else IN_APPLY(false, false);
#undef IN_APPLY
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_axial_attention_supported(int64_t n_img, int heads, int H, int W, int hd) { return ax_reason(n_img, heads, H, W, hd) == nullptr ? 1 : 0; }

extern "C" int tante_axial_attention(const float* qkv, int64_t n_img, int heads, int H, int W, int hd, const float* qw, const float* qb, const float* kw,
                                     const float* kb, float eps, float* out, void* stream) {
  if (const char* why = ax_reason(n_img, heads, H, W, hd))
    TANTE_FAIL(-2, "tante_axial_attention: %s (images %lld, heads %d, grid %d x %d, head dim %d)", why, (long long)n_img, heads, H, W, hd);
  if (!qkv || !qw || !qb || !kw || !kb || !out) TANTE_FAIL(-1, "tante_axial_attention: null argument");
  if ((uintptr_t)qkv % 16) TANTE_FAIL(-1, "tante_axial_attention: qkv must be 16-byte aligned");
  if (n_img == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (hd == 16) ax_launch<16>(0, qkv, qw, qb, kw, kb, out, n_img, heads, H, W, eps, s);
  else if (hd == 32) ax_launch<32>(1, qkv, qw, qb, kw, kb, out, n_img, heads, H, W, eps, s);
  else ax_launch<64>(2, qkv, qw, qb, kw, kb, out, n_img, heads, H, W, eps, s);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_time_attention_supported(int64_t nseq, int T, int heads, int hd) { return tm_reason(nseq, T, heads, hd) == nullptr ? 1 : 0; }

extern "C" int tante_time_attention(const float* qkv, int64_t nseq, int T, int heads, int hd, const float* qw, const float* qb, const float* kw,
                                    const float* kb, float eps, const float* bias, float* out, void* stream) {
  if (const char* why = tm_reason(nseq, T, heads, hd))
    TANTE_FAIL(-2, "tante_time_attention: %s (sequences %lld, T %d, heads %d, head dim %d)", why, (long long)nseq, T, heads, hd);
  if (!qkv || !qw || !qb || !kw || !kb || !bias || !out) TANTE_FAIL(-1, "tante_time_attention: null argument");
  if ((uintptr_t)qkv % 16) TANTE_FAIL(-1, "tante_time_attention: qkv must be 16-byte aligned");
  if (nseq == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (hd == 16) tm_launch<16>(qkv, qw, qb, kw, kb, bias, out, nseq, T, heads, eps, s);
  else if (hd == 32) tm_launch<32>(qkv, qw, qb, kw, kb, bias, out, nseq, T, heads, eps, s);
  else tm_launch<64>(qkv, qw, qb, kw, kb, bias, out, nseq, T, heads, eps, s);
  TANTE_CHECK_LAUNCH();
  return 0;
}

extern "C" int tante_field_stats_supported(int64_t B, int T, int C, int64_t HW) { return fs_reason(B, T, C, HW) == nullptr ? 1 : 0; }

extern "C" int64_t tante_field_stats_workspace_bytes(int64_t B, int T, int C, int64_t HW) {
  if (fs_reason(B, T, C, HW)) return -1;
  return B * C * fs_plan(T, HW).S * 2 * (int64_t)sizeof(float);
}

extern "C" int tante_field_stats(const float* x, int64_t B, int T, int C, int64_t HW, float eps, float* stats, float* xn, void* work, int64_t work_bytes,
                                 void* stream) {
  if (const char* why = fs_reason(B, T, C, HW))
    TANTE_FAIL(-2, "tante_field_stats: %s (B %lld, T %d, C %d, pixels %lld)", why, (long long)B, T, C, (long long)HW);
  if (!x || !stats) TANTE_FAIL(-1, "tante_field_stats: null argument");
  if (B == 0) return 0;
  const int64_t need = tante_field_stats_workspace_bytes(B, T, C, HW);
  if (!work || work_bytes < need) TANTE_FAIL(-1, "tante_field_stats: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  const FsPlan p = fs_plan(T, HW);
  hipStream_t s = (hipStream_t)stream;
  const long BC = (long)(B * C);
  hipLaunchKernelGGL(fs_stats_kernel, dim3((unsigned)BC, p.S), dim3(AV_THREADS), 0, s, x, (float*)work, T, C, (long)HW, (long)p.n, (long)p.SZ, p.S);
  TANTE_CHECK_LAUNCH();
  hipLaunchKernelGGL(fs_combine_kernel, dim3((unsigned)((BC + 63) / 64)), dim3(64), 0, s, (const float*)work, stats, BC, (long)p.n, (long)p.SZ, p.S, eps);
  TANTE_CHECK_LAUNCH();
  if (xn) {
    const long total = BC * p.n;
    hipLaunchKernelGGL(fs_norm_kernel, dim3((unsigned)((total + AV_THREADS - 1) / AV_THREADS)), dim3(AV_THREADS), 0, s, x, (const float*)stats, xn, (long)B,
                       T, C, (long)HW, total);
    TANTE_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int tante_field_affine_supported(int64_t B, int Tk, int C, int64_t HW) { return fa_reason(B, Tk, C, HW) == nullptr ? 1 : 0; }

extern "C" int tante_field_affine(const float* y, const float* stats, int64_t B, int Tk, int C, int64_t HW, float* out, void* stream) {
  if (const char* why = fa_reason(B, Tk, C, HW))
    TANTE_FAIL(-2, "tante_field_affine: %s (B %lld, steps %d, C %d, pixels %lld)", why, (long long)B, Tk, C, (long long)HW);
  if (!y || !stats || !out) TANTE_FAIL(-1, "tante_field_affine: null argument");
  if (B == 0) return 0;
  const long total = (long)(B * C) * Tk * HW;
  hipLaunchKernelGGL(fs_affine_kernel, dim3((unsigned)((total + AV_THREADS - 1) / AV_THREADS)), dim3(AV_THREADS), 0, (hipStream_t)stream, y, stats, out, (long)B,
                     Tk, C, (long)HW, total);
  TANTE_CHECK_LAUNCH();
  return 0;
}
