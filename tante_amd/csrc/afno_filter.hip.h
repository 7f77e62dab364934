// What the forward (afno_filter.hip) and the backward (afno_filter_bwd.hip) of the AFNO spectral filter share beyond dft_rows.hip.h:
// the tile constants of the mix launches, which tables a packed twiddle buffer holds, and the shape predicate's reason.
#pragma once
#include "dft_rows.hip.h"

namespace {

constexpr int AF_MAX = DFT_MAX;            // grid points per axis, channels per block
constexpr int AF_THREADS = DFT_THREADS;
constexpr int AF_LD = 2 * AF_MAX + 4;      // LDS row stride of launch 2 ([re | im] rows of a channel block), 4 (mod 64) like DFT_LD
constexpr int AF_ROWS_A = 64;              // launch 2: rows of the P tile (h) / the hidden tile (k)
constexpr int AF_ROWS_B = 48;              // launch 2: rows of the spectrum tile, Kc <= 33 padded to 16

struct AfTables : DftTables {
  int Lc, Kc;
};

// adjoint = false: T1 (Lc, W), T2 (Kc, H), T3 (W, Kc), T4 (H, Lc); adjoint = true: their conjugate transposes, in the same order
inline AfTables af_tables(int H, int W, bool adjoint = false) {
  const int Lc = H < W ? H : W, Kc = (H / 2 + 1) < (W / 2 + 1) ? (H / 2 + 1) : (W / 2 + 1);
  const int M[4] = {Lc, Kc, W, H}, K[4] = {W, H, Kc, Lc};
  return AfTables{adjoint ? dft_tables(K, M) : dft_tables(M, K), Lc, Kc};
}

inline const char* af_reason(int64_t B, int H, int W, int C, int bs) {
  if (H < 1 || W < 1 || H > AF_MAX || W > AF_MAX) return "token grid outside 1..64 points per axis";
  if (bs < 1 || bs > AF_MAX) return "channel block size outside 1..64";
  if (C < 1 || C % bs) return "channels are not a whole number of blocks";
  if (B < 0 || B > 65535) return "more than 65535 samples per call";
  return nullptr;
}

}  // namespace
