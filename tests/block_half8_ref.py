"""The 8-wave form of the half-size block launches (tante_amd/csrc/block_sliced.hip: tante_fs_half8_launch, TANTE_FS_HALF8): its rule
restated, and the cases tests/test_hip_block_half8.py runs.  Nothing here touches the GPU or tante_amd; tests/test_block_half8_cpu.py
holds the rule against the source text and against block_forms_ref.fs_route (the launches that reach the 4-wave 2-tile instances)."""
import block_forms_ref as R

OPTION_DEFAULTS = dict(R.OPTION_DEFAULTS, TANTE_FS_HALF8=1)
HALF4_ROUTES = ("fs<TPS1,NTT2,NW4>", "fs<TPS2,NTT2,NW4>")      # what these launches take under TANTE_FS_HALF8 = 0


def _opt(options, name):
    return (options or {}).get(name, OPTION_DEFAULTS[name])


def half8_rule(L: int, nseq: int, causal: bool, options=None):
    """tante_fs_half8_launch restated: None where it returns 0 (the caller takes tante_fs_launch), else (TPS, sequences per workgroup,
    workgroups).  Plain inference launches only: the propagator, the last-slot form and training never ask it."""
    if nseq >= R.FS_MAX_NSEQ:
        raise R.Refused(f"nseq={nseq}")
    waves = 8 if (_opt(options, "TANTE_FS_WAVES") == 8 or L > 64) else 4
    if nseq < 1 or L < 1 or 32 % L != 0 or (L == 32 and causal) or waves != 4:
        return None
    if not _opt(options, "TANTE_FS_HALF") or not _opt(options, "TANTE_FS_HALF8"):
        return None

    def nwg_at(ntt):
        spw = 16 * ntt // L
        return (nseq + spw - 1) // spw

    def rounds(ntt):
        return ((nwg_at(ntt) + 511) // 512) * ntt
    ntt_full = 3 if (L != 32 and rounds(3) < rounds(4)) else 4
    if nwg_at(ntt_full) * 4 > 512:
        return None
    return (2 if L == 32 else 1, 32 // L, nwg_at(2))


# ---- the cases of the GPU test: the smallest shapes at which the form can go wrong ---------------------------------------------------------
SUB_GRID = (2, 4, 32, 3)         # (B, T, H, W): the H letter of the slot-(T - 1) sub-grid is L = 32 (covered), its W letter L = 3 (not covered)
SUB_GRID_W = (2, 4, 3, 32)       # ... and the grid whose W letter is L = 32 from a non-zero row0 (covered)
_H4 = {1: "fs<TPS1,NTT2,NW4>", 2: "fs<TPS2,NTT2,NW4>"}


def _dense(L, nseq, causal):
    return R._fs(f"half8-L{L}x{nseq}{'c' if causal else ''}", L, nseq, causal, _H4[2 if L == 32 else 1])


COVERED = ([_dense(32, 1, False), _dense(32, 5, False),                 # one workgroup; an odd count
            R._letter("half8-subH-2x4x32x3", 256, 256, "H", SUB_GRID, _H4[2], sub=True),
            R._letter("half8-subW-2x4x3x32", 256, 256, "W", SUB_GRID_W, _H4[2], sub=True),
            _dense(16, 3, False)]                                        # two sequences per workgroup, the last workgroup half dead
           + [_dense(L, n, c) for L in (8, 4) for n in (5, 9) for c in (False, True)]
           + [_dense(1, 3, False)])
# shapes the rule does not cover: today's kernel either way
NOT_COVERED = [R._letter("half8-subW-2x4x32x3", 256, 256, "W", SUB_GRID, "fs<TPS0,NTT4,NW4>", sub=True),      # L = 3
               R._fs("half8-L32x257", 32, 257, False, "fs<TPS2,NTT4,NW4>")]                                    # past 256 half-size workgroups
