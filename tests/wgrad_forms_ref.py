"""The weight-gradient GEMM (tante_amd/csrc/wgrad.hip) alone: its dispatch restated, float64 references and the case list.

Plain torch on the CPU, no GPU import.  tests/test_wgrad_forms_cpu.py pins the restatement to the text of wgrad.hip, the gather / scatter
restatements to torch's own operators and the bars to wrong results; tests/test_hip_wgrad_forms.py runs every case on the device.

Route names.  One launch is an ATOM:
    gen<f32|bf16,T64|T128,MU,MV>+atomic|slab      wgrad_kernel<BF16, T, MU, MV>, added with atomics / through wgrad_gen_reduce_kernel
    tr<4,1>|tr<8,1>|tr<4,2>+atomic|slab           wgrad_tr_kernel<WNBUF, RG>, added with atomics / through wgrad_reduce_kernel
    jobs                                          wgrad_tr_jobs_kernel + wgrad_reduce_jobs_kernel
tante_wgrad / tante_wgrad_ws return one atom; tante_wgrad_multi_ws returns "multi: <atom> x<segments> | ..." (one entry per launch, equal
neighbours folded as "N*(...)"); tante_wgrad_jobs_ws returns "jobs" or "one-by-one[<why>]: <multi route> ; ...".  ALL_ROUTES holds the
atoms: a composite route is covered through `route_atoms`.
"""
import re
import zlib

import torch

F32, BF16 = 0, 1
A_LINEAR, A_PATCH_NHWC, A_PATCH_NCHW = 0, 1, 2
W_LINEAR, W_CONV_NHWC, W_DECONV_NHWC, W_DECONV_NCHW = 0, 1, 2, 3
LAYOUT_NAMES = {W_LINEAR: "LINEAR", W_CONV_NHWC: "CONV_NHWC", W_DECONV_NHWC: "DECONV_NHWC", W_DECONV_NCHW: "DECONV_NCHW"}

# ---- constants of wgrad.hip (read back out of its text by test_wgrad_route_matches_the_source) ---------------------------------------
RC, WT, WRC, WSEG, WJOBS, WGJ_OCC = 64, 128, 32, 8, 4, 2
SLAB_MIN_CHUNKS = 8                    # slab_ok: R >= 8 * RC
DEFAULTS = {"TANTE_WGRAD_WGS": 512, "TANTE_WGRAD_SLAB_WGS": 1536, "TANTE_WGRAD_JOBS_WGS": 256 * WGJ_OCC, "TANTE_WGRAD_NO_TR": 0,
            "TANTE_WGRAD_NO_SLAB": 0, "TANTE_WGRAD_RG": 1, "TANTE_WGRAD_DEEP": -1, "TANTE_WGRAD_JOBS": 1, "TANTE_WGRAD_TR_WGS": 0}
# (mu, mv) -> the instantiated pair, in the order of launch_wgrad's if-chain; None = any
STAGE_TABLE = [("ROWMAJOR", "ROWMAJOR", "ROWMAJOR", "ROWMAJOR"), ("COLMAJOR", "COLMAJOR", "COLMAJOR", "COLMAJOR"),
               ("ROWMAJOR", "PATCH_NHWC", "ROWMAJOR", "PATCH_NHWC"), ("ROWMAJOR", "PATCH_NCHW2", "ROWMAJOR", "PATCH_NCHW2"),
               ("ROWMAJOR", None, "ROWMAJOR", "GENERIC"), (None, None, "GENERIC", "GENERIC")]
SHORT = {"ROWMAJOR": "ROW", "COLMAJOR": "COL", "PATCH_NHWC": "PATCH_NHWC", "PATCH_NCHW2": "PATCH_NCHW2", "GENERIC": "GEN"}
# the lines of wgrad.hip that the functions below restate, verbatim: an edited line is no longer found and fails the CPU test
SOURCE_LINES = [
    # rm_stage_mode
    "if (m.mode == TANTE_A_PATCH_NHWC && ((uintptr_t)m.p % 16) == 0 && m.Cin % 4 == 0 && m.off % 4 == 0 && m.s1 % 4 == 0 && ncols % 4 == 0)\n    return ST_PATCH_NHWC;",
    "if (m.mode == TANTE_A_PATCH_NCHW && m.P == 2 && ((uintptr_t)m.p % 16) == 0 && (m.Win / 2) % 4 == 0 && m.Win % 8 == 0 && m.off % 8 == 0 &&\n"
    "      m.s1 % 8 == 0 && ((long)m.Hin * m.Win) % 8 == 0 && ncols % 4 == 0)\n    return ST_PATCH_NCHW2;",
    "if (m.mode != TANTE_A_LINEAR || ((uintptr_t)m.p % 16)) return ST_GENERIC;",
    "const int al = m.dtype == TANTE_BF16 ? 4 : 4;",
    "if (m.es == 1 && m.s1 % al == 0 && m.s0 % al == 0 && m.off % al == 0 && ncols % 4 == 0) return ST_ROWMAJOR;",
    "if (m.dtype == TANTE_F32 && m.s0 == 1 && m.es % 4 == 0 && m.n0 % 4 == 0 && m.s1 % 4 == 0 && m.off % 4 == 0) return ST_COLMAJOR;",
    # wgrad_tr_ok
    "return m.mode == TANTE_A_LINEAR && m.dtype == TANTE_BF16 && m.es == 1 && (m.s1 == 0 || m.n0 >= R) && m.s0 % 8 == 0 && m.off % 8 == 0 &&\n"
    "         ((uintptr_t)m.p % 16) == 0 && ncols % WT == 0 && m.s0 >= ncols;",
    # launch_wgrad
    "const int ti = (I + T - 1) / T, tj = (J + T - 1) / T;",
    "const bool slab_ok = ws != nullptr && ti == 1 && tj == 1 && slab_target > 0 && R >= 8 * RC && ws_bytes >= 2 * ((long)I * J + I) * 4;",
    "long split = (slab_ok ? slab_target : wg_target) / ((long)ti * tj);",
    "if (split < 1) split = 1;\n  const long max_split = slab_ok ? (R + RC - 1) / RC : (R + 4 * RC - 1) / (4 * RC);\n  if (split > max_split) split = max_split;",
    "if (slab_ok && split * ((long)I * J + I) * 4 > ws_bytes) split = ws_bytes / (((long)I * J + I) * 4);\n  if (split > 65535) split = 65535;",
    "long per = (R + split - 1) / split;\n  per = (per + RC - 1) / RC * RC;\n  split = (R + per - 1) / per;",
    "const bool use_slab = slab_ok && split > 1;",
    "(unsigned)(split >= 64 ? 16 : 1)",
    # wgrad_tr_launch
    "if (no_tr || n_seg < 1 || n_seg > WSEG || R % WRC) return false;",
    "if (!wgrad_tr_ok(U[g], R, I) || !wgrad_tr_ok(V[g], R, J) || U[g].s0 != U[0].s0 || V[g].s0 != V[0].s0) return false;",
    'const int wg_env = tante_opt("TANTE_WGRAD_TR_WGS", tante_opt("TANTE_WGRAD_WGS", 0));',
    "const bool want_slab = ws != nullptr && !no_slab;",
    "const int RGv = (want_slab && rg_env == 2 && deep_env <= 0) ? 2 : 1;",
    "const int wg_target = wg_env > 0 ? wg_env : (want_slab ? 512 / RGv : (ti * tj <= 4 ? 128 : 256));",
    "long split = wg_target / ((long)ti * tj * n_seg);\n  if (split < 1) split = 1;\n  const long nch = R / WRC;\n"
    "  if (split > nch / (4 * RGv)) split = nch / (4 * RGv) > 0 ? nch / (4 * RGv) : 1;\n  long per = ((nch + split - 1) / split) * WRC;\n"
    "  if (per % (RGv * WRC)) per += WRC;\n  while (R % per && per < R) per += RGv * WRC;",
    "if (R % per || per % (RGv * WRC)) return false;\n  split = R / per;\n  const long total = split * n_seg;\n  if (total > 65535) return false;",
    "const bool use_slab = want_slab && total > 1 && need <= ws_bytes && ((uintptr_t)ws % 16) == 0;",
    "if (RGv == 2 && use_slab)\n    hipLaunchKernelGGL((wgrad_tr_kernel<4, 2>)",
    "else if (deep_env > 0)\n    hipLaunchKernelGGL((wgrad_tr_kernel<8, 1>)",
    "else\n    hipLaunchKernelGGL((wgrad_tr_kernel<4, 1>)",
    # wgrad_one / tante_wgrad_ws / tante_wgrad_multi_ws
    "if (compute == TANTE_BF16 && wgrad_tr_launch(U, V, 1, (long)R, I, J, dW, dbias, layout, P, C_other, swap, s)) {",
    "if (I > 64 || J > 64) launch_wgrad<true, 128>",
    "else launch_wgrad<true, 64>",
    "launch_wgrad<false, 64>",
    "float* ws = (workspace && workspace_bytes > 0 && ((uintptr_t)workspace % 16) == 0) ? (float*)workspace : nullptr;",
    "const int n = n_seg - g < WSEG ? n_seg - g : WSEG;",
    "if (compute == TANTE_BF16 && n > 1 && wgrad_tr_launch(U + g, V + g, n, (long)R, I, J, dW, dbias, layout, P, C_other, swap, s, workspace, workspace_bytes)) {",
    "const int rc = wgrad_one(U + g, V + g, R, I, J, dW, dbias, layout, P, C_other, swap, compute, s);",
    # tante_wgrad_jobs_ws
    'bool ok = compute == TANTE_BF16 && n_jobs >= 2 && n_jobs <= WJOBS && workspace && ((uintptr_t)workspace % 16) == 0 && tante_opt("TANTE_WGRAD_JOBS", 1) &&\n'
    '            !tante_opt("TANTE_WGRAD_NO_SLAB", 0) && !tante_opt("TANTE_WGRAD_NO_TR", 0);',
    "jb.n_seg < 1 || jb.n_seg > WSEG || jb.R <= 0 || jb.R % WRC || jb.I <= 0 || jb.J <= 0 || jb.I % WT || jb.J % WT) { ok = false; break; }",
    "const long total = ((nch + c - 1) / c) * jobs[k].n_seg;",
    "for (int x = 0; x < 8; ++x) load[(x + r) & 7] += (total / 8 + (x < total % 8 ? 1 : 0)) * ntile;\n        r = (int)((r + total) & 7);",
    "long lo = 4, hi = 4;",
    "if (busiest(mid) * 8 <= wg_total) hi = mid; else lo = mid + 1;",
    "while (busiest(cper) * 8 > wg_total && cper < hi) ++cper;",
    "long split = (nch + cper - 1) / cper;      // splits per segment\n    if (split < 1) split = 1;\n    if (split > nch) split = nch;",
    "ws_off += ((int64_t)total * ntile * WT * WT + (int64_t)total * jb.I + 3) / 4 * 4;",
    "if (ws_off * (int64_t)sizeof(float) > workspace_bytes) return one_by_one();",
    # the kernels' own row ranges
    "r_begin = (sp * nch_seg / seg_splits) * WRC;\n    r_end = ((sp + 1) * nch_seg / seg_splits) * WRC;",
    "const int bz = (slot / ntile) * 8 + ((xcd - xcd_rot) & 7), tile = slot % ntile;",
]


def _opt(options, name, dflt=None):
    return (options or {}).get(name, DEFAULTS[name] if dflt is None else dflt)


def _addr(m):
    return int(m.p or 0)


def rm_stage_mode(m, ncols):
    if m.mode == A_PATCH_NHWC and _addr(m) % 16 == 0 and m.Cin % 4 == 0 and m.off % 4 == 0 and m.s1 % 4 == 0 and ncols % 4 == 0:
        return "PATCH_NHWC"
    if (m.mode == A_PATCH_NCHW and m.P == 2 and _addr(m) % 16 == 0 and (m.Win // 2) % 4 == 0 and m.Win % 8 == 0 and m.off % 8 == 0 and
            m.s1 % 8 == 0 and (m.Hin * m.Win) % 8 == 0 and ncols % 4 == 0):
        return "PATCH_NCHW2"
    if m.mode != A_LINEAR or _addr(m) % 16:
        return "GENERIC"
    al = 4
    if m.es == 1 and m.s1 % al == 0 and m.s0 % al == 0 and m.off % al == 0 and ncols % 4 == 0:
        return "ROWMAJOR"
    if m.dtype == F32 and m.s0 == 1 and m.es % 4 == 0 and m.n0 % 4 == 0 and m.s1 % 4 == 0 and m.off % 4 == 0:
        return "COLMAJOR"
    return "GENERIC"


def wgrad_tr_ok(m, R, ncols):
    return (m.mode == A_LINEAR and m.dtype == BF16 and m.es == 1 and (m.s1 == 0 or m.n0 >= R) and m.s0 % 8 == 0 and m.off % 8 == 0 and
            _addr(m) % 16 == 0 and ncols % WT == 0 and m.s0 >= ncols)


class Launch:
    """One kernel launch (+ its reduce launch): the atom's name, the segments it serves, the splits per segment and every split's row
    range inside its segment; `chunks` = staged chunks per workgroup (and per row group), `reduce_y` the reduce grid's y."""

    def __init__(self, name, n_seg, split, ranges, chunk_rows, rg=1, reduce_y=0, extra=None):
        self.name, self.n_seg, self.split, self.ranges, self.rg, self.reduce_y = name, n_seg, split, ranges, rg, reduce_y
        self.chunks = [-(-(b - a) // chunk_rows) // rg for a, b in ranges]
        self.extra = extra or {}


class Plan:
    def __init__(self, name, launches):
        self.name, self.launches = name, launches

    @property
    def split(self):
        return self.launches[0].split

    @property
    def ranges(self):
        return self.launches[0].ranges


def gen_launch(U, V, R, I, J, compute, ws_bytes, options):
    """launch_wgrad<BF16, T>: the template pair, the split arithmetic and the epilogue."""
    bf = compute == BF16
    T = 128 if bf and (I > 64 or J > 64) else 64
    mu, mv = rm_stage_mode(U, I), rm_stage_mode(V, J)
    MU, MV = next((a, b) for cu, cv, a, b in STAGE_TABLE if cu in (None, mu) and cv in (None, mv))
    ti, tj = -(-I // T), -(-J // T)
    wg_target, slab_target = _opt(options, "TANTE_WGRAD_WGS"), _opt(options, "TANTE_WGRAD_SLAB_WGS")
    partial = (I * J + I) * 4
    slab_ok = ws_bytes > 0 and ti == 1 and tj == 1 and slab_target > 0 and R >= SLAB_MIN_CHUNKS * RC and ws_bytes >= 2 * partial
    split = (slab_target if slab_ok else wg_target) // (ti * tj)
    split = max(split, 1)
    max_split = -(-R // RC) if slab_ok else -(-R // (4 * RC))
    split = min(split, max_split)
    if slab_ok and split * partial > ws_bytes:
        split = ws_bytes // partial
    split = min(split, 65535)
    per = -(-R // split)
    per = -(-per // RC) * RC
    split = -(-R // per)
    use_slab = slab_ok and split > 1
    name = f"gen<{'bf16' if bf else 'f32'},T{T},{SHORT[MU]},{SHORT[MV]}>+{'slab' if use_slab else 'atomic'}"
    ranges = [(k * per, min(R, (k + 1) * per)) for k in range(split)]
    return Launch(name, 1, split, ranges, RC, reduce_y=(16 if split >= 64 else 1) if use_slab else 0, extra=dict(T=T, ti=ti, tj=tj, per=per))


def tr_launch(U, V, n_seg, R, I, J, ws_bytes, options, ws_ptr=0):
    """wgrad_tr_launch -> a Launch, or None where it returns false.  ws_bytes > 0: a workspace was passed."""
    if _opt(options, "TANTE_WGRAD_NO_TR") or n_seg < 1 or n_seg > WSEG or R % WRC:
        return None
    for g in range(n_seg):
        if not wgrad_tr_ok(U[g], R, I) or not wgrad_tr_ok(V[g], R, J) or U[g].s0 != U[0].s0 or V[g].s0 != V[0].s0:
            return None
    ti, tj = I // WT, J // WT
    wg_env = (options or {}).get("TANTE_WGRAD_TR_WGS", (options or {}).get("TANTE_WGRAD_WGS", 0))
    want_slab = ws_bytes > 0 and not _opt(options, "TANTE_WGRAD_NO_SLAB")
    rg_env, deep_env = _opt(options, "TANTE_WGRAD_RG"), _opt(options, "TANTE_WGRAD_DEEP")
    RGv = 2 if (want_slab and rg_env == 2 and deep_env <= 0) else 1
    wg_target = wg_env if wg_env > 0 else (512 // RGv if want_slab else (128 if ti * tj <= 4 else 256))
    split = max(wg_target // (ti * tj * n_seg), 1)
    nch = R // WRC
    if split > nch // (4 * RGv):
        split = nch // (4 * RGv) if nch // (4 * RGv) > 0 else 1
    per = -(-nch // split) * WRC
    if per % (RGv * WRC):
        per += WRC
    while R % per and per < R:
        per += RGv * WRC
    if R % per or per % (RGv * WRC):
        return None
    split = R // per
    total = split * n_seg
    if total > 65535:
        return None
    need = (total * ti * tj * WT * WT + total * I) * 4
    use_slab = want_slab and total > 1 and need <= ws_bytes and ws_ptr % 16 == 0
    if RGv == 2 and use_slab:
        kern, rg = "tr<4,2>", 2
    elif deep_env > 0:
        kern, rg = "tr<8,1>", 1
    else:
        kern, rg = "tr<4,1>", 1
    ranges = [(k * per, (k + 1) * per) for k in range(split)]
    return Launch(f"{kern}+{'slab' if use_slab else 'atomic'}", n_seg, split, ranges, WRC, rg=rg, reduce_y=(4 if total >= 16 else 1) if use_slab else 0,
                  extra=dict(ti=ti, tj=tj, per=per, total=total, ring=8 if kern == "tr<8,1>" else 4))


def one_launch(U, V, R, I, J, compute, ws_bytes, options):
    """wgrad_one: the transposed-read path never sees the workspace here (atomic epilogue); the generic kernel does."""
    if compute == BF16:
        t = tr_launch([U], [V], 1, R, I, J, 0, options)
        if t:
            return t
    return gen_launch(U, V, R, I, J, compute, ws_bytes, options)


def multi_launches(U, V, n_seg, R, I, J, compute, ws_bytes, options, ws_ptr=0):
    out, g = [], 0
    while g < n_seg:
        n = min(n_seg - g, WSEG)
        t = tr_launch(U[g:g + n], V[g:g + n], n, R, I, J, ws_bytes, options, ws_ptr) if compute == BF16 and n > 1 else None
        if t:
            out.append(t)
            g += n
            continue
        out.append(one_launch(U[g], V[g], R, I, J, compute, 0, options))
        g += 1
    return out


def _fold(names):
    out = []
    for n in names:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return " | ".join(n if k == 1 else f"{k}*({n})" for n, k in out)


def _multi_name(launches):
    return "multi: " + _fold([f"{l.name} x{l.n_seg}" for l in launches])


class JobDesc:
    """What tante_wgrad_jobs_ws reads of a TanteWgradJob for its plan."""

    def __init__(self, U, V, n_seg, R, I, J, layout=W_LINEAR):
        self.U, self.V, self.n_seg, self.R, self.I, self.J, self.layout = U, V, n_seg, R, I, J, layout


def jobs_plan(jobs, compute, ws_bytes, options, ws_ptr=0):
    n_jobs = len(jobs)

    def one_by_one(why):
        ls = [multi_launches(j.U, j.V, j.n_seg, j.R, j.I, j.J, compute, ws_bytes, options, ws_ptr) for j in jobs]
        return Plan(f"one-by-one[{why}]: " + " ; ".join(_multi_name(l) for l in ls), [l for group in ls for l in group])
    if not (compute == BF16 and 2 <= n_jobs <= WJOBS):
        return one_by_one("fp32 compute" if compute != BF16 else f"{n_jobs} jobs")
    if not (ws_bytes > 0 and ws_ptr % 16 == 0):
        return one_by_one("no workspace")
    for o in ("TANTE_WGRAD_JOBS", "TANTE_WGRAD_NO_SLAB", "TANTE_WGRAD_NO_TR"):
        if bool(_opt(options, o)) != (o == "TANTE_WGRAD_JOBS"):
            return one_by_one(f"{o}={_opt(options, o)}")
    for j in jobs:
        if j.n_seg < 1 or j.n_seg > WSEG or j.R <= 0 or j.R % WRC or j.I % WT or j.J % WT:
            return one_by_one("a job outside the shape rules")
        for g in range(j.n_seg):
            if not wgrad_tr_ok(j.U[g], j.R, j.I) or not wgrad_tr_ok(j.V[g], j.R, j.J) or j.U[g].s0 != j.U[0].s0 or j.V[g].s0 != j.V[0].s0:
                return one_by_one("a job outside the operand rules")
    wg_total = _opt(options, "TANTE_WGRAD_JOBS_WGS")
    rot = [0] * n_jobs

    def busiest(c):
        load, r = [0] * 8, 0
        for k, j in enumerate(jobs):
            nch, ntile = j.R // WRC, (j.I // WT) * (j.J // WT)
            total = -(-nch // c) * j.n_seg
            rot[k] = r
            for x in range(8):
                load[(x + r) & 7] += (total // 8 + (1 if x < total % 8 else 0)) * ntile
            r = (r + total) & 7
        return max(load)
    lo = hi = 4
    for j in jobs:
        hi = max(hi, j.R // WRC)
    while lo < hi:
        mid = (lo + hi) // 2
        if busiest(mid) * 8 <= wg_total:
            hi = mid
        else:
            lo = mid + 1
    cper = lo
    while busiest(cper) * 8 > wg_total and cper < hi:
        cper += 1
    busiest(cper)
    ws_off, per_job = 0, []
    for k, j in enumerate(jobs):
        ntile, nch = (j.I // WT) * (j.J // WT), j.R // WRC
        split = min(max(-(-nch // cper), 1), nch)
        total = split * j.n_seg
        if total > 65535:
            return one_by_one("too many splits")
        ws_off += (total * ntile * WT * WT + total * j.I + 3) // 4 * 4
        ranges = [((sp * nch // split) * WRC, ((sp + 1) * nch // split) * WRC) for sp in range(split)]
        per_job.append(Launch("jobs", j.n_seg, split, ranges, WRC, extra=dict(total=total, rot=rot[k], ntile=ntile, cper=cper)))
    if ws_off * 4 > ws_bytes:
        return one_by_one("workspace too small")
    return Plan("jobs", per_job)


def wgrad_plan(entry, U, V, n_seg, R, I, J, compute, ws_bytes, options=None, ws_ptr=0):
    """entry: "one" (tante_wgrad / tante_wgrad_ws; U, V one row matrix each), "multi" (tante_wgrad_multi / _ws; lists of n_seg), "jobs"
    (tante_wgrad_jobs_ws; U is the list of JobDesc, the shape arguments are ignored).  ws_bytes = 0: no workspace."""
    if entry == "one":
        if ws_ptr % 16:
            ws_bytes = 0
        l = one_launch(U, V, R, I, J, compute, ws_bytes, options)
        return Plan(l.name, [l])
    if entry == "multi":
        ls = multi_launches(U, V, n_seg, R, I, J, compute, ws_bytes, options, ws_ptr)
        return Plan(_multi_name(ls), ls)
    assert entry == "jobs"
    return jobs_plan(U, compute, ws_bytes, options, ws_ptr)


def wgrad_route(entry, U, V, n_seg, R, I, J, compute, ws_bytes, options=None, ws_ptr=0):
    return wgrad_plan(entry, U, V, n_seg, R, I, J, compute, ws_bytes, options, ws_ptr).name


ATOM = re.compile(r"gen<[^>]*>\+\w+|tr<\d,\d>\+\w+|jobs")


def route_atoms(route):
    return set(ATOM.findall(route.split("]:", 1)[-1] if route.startswith("one-by-one") else route))


def all_routes():
    r = set()
    for prec in ("f32,T64", "bf16,T64", "bf16,T128"):
        for _, _, a, b in STAGE_TABLE:
            for ep in ("atomic", "slab"):
                r.add(f"gen<{prec},{SHORT[a]},{SHORT[b]}>+{ep}")
    r |= {"tr<4,1>+atomic", "tr<4,1>+slab", "tr<8,1>+atomic", "tr<8,1>+slab", "tr<4,2>+slab", "jobs"}
    return r


ALL_ROUTES = all_routes()
COVERED_ELSEWHERE = {}      # route -> (why, "tests/<file>.py::<test>"): nothing is left to other files


# ---- the gather and the scatter, restated ----------------------------------------------------------------------------------------------
def rm_index(m, R, ncols):
    """rm_elem's element offset (from m.p) of every (row, column): a (R, ncols) LongTensor."""
    r, c = torch.arange(R)[:, None], torch.arange(ncols)[None, :]
    if m.mode == A_LINEAR:
        return (r // m.n0) * m.s1 + (r % m.n0) * m.s0 + m.off + c * m.es
    Wo, Ho = m.Win // m.P, m.Hin // m.P
    img, rem = r // (Ho * Wo), r % (Ho * Wo)
    ho, wo = rem // Wo, rem % Wo
    img_off = (img // m.n0) * m.s1 + (img % m.n0) * (m.Cin * m.Hin * m.Win) + m.off
    if m.mode == A_PATCH_NHWC:
        seg = m.P * m.Cin
        kh, rest = c // seg, c % seg
        return img_off + ((ho * m.P + kh) * m.Win + wo * m.P) * m.Cin + rest
    pp = m.P * m.P
    ci, kh, kw = c // pp, (c % pp) // m.P, c % m.P
    return img_off + (ci * m.Hin + ho * m.P + kh) * m.Win + wo * m.P + kw


def out_index(layout, I, J, P, Co, swap):
    """out_index of every (i, j): an (I, J) LongTensor of offsets into the parameter."""
    i, j = torch.arange(I)[:, None].expand(I, J), torch.arange(J)[None, :].expand(I, J)
    n, k = (j, i) if swap else (i, j)
    N, K = (J, I) if swap else (I, J)
    if layout == W_CONV_NHWC:
        kh, kw, ci = k // (P * Co), (k // Co) % P, k % Co
        return ((n * Co + ci) * P + kh) * P + kw
    if layout == W_DECONV_NHWC:
        kh, kw, co = n // (P * Co), (n // Co) % P, n % Co
        return ((k * Co + co) * P + kh) * P + kw
    if layout == W_DECONV_NCHW:
        return k * N + n
    return n * K + k


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
class Mat:
    """A TanteRowMat by value; `lead` = elements between the (16-byte aligned) buffer and m.p."""
    p = 0

    def __init__(self, dtype, mode, R, ncols, s1=0, s0=0, off=0, es=1, n0=1, Hin=0, Win=0, Cin=0, P=0, lead=0):
        self.dtype, self.mode, self.R, self.ncols, self.s1, self.s0, self.off, self.es, self.n0 = dtype, mode, R, ncols, s1, s0, off, es, n0
        self.Hin, self.Win, self.Cin, self.P, self.lead = Hin, Win, Cin, P, lead
        self.p = lead * (2 if dtype == BF16 else 4)


def rows(dtype, R, ncols, pad=0, off=0, n0=None, gap=0, lead=0):
    """Row-major rows s0 = ncols + pad apart; n0: blocks of n0 rows, `gap` elements between blocks."""
    s0 = ncols + pad
    if n0 is None:
        return Mat(dtype, A_LINEAR, R, ncols, s1=0, s0=s0, off=off, n0=R, lead=lead)
    return Mat(dtype, A_LINEAR, R, ncols, s1=n0 * s0 + gap, s0=s0, off=off, n0=n0, lead=lead)


def lines(R, ncols, n0=12, es=16, gap=8, off=4, lead=0):
    """fp32 lines: consecutive rows are consecutive addresses inside blocks of n0 rows, columns es apart (the axis propagators)."""
    return Mat(F32, A_LINEAR, R, ncols, s1=es * ncols + gap, s0=1, off=off, es=es, n0=n0, lead=lead)


def patches(dtype, nhwc, n_img, Hin, Win, Cin, P, n0=None, gap=0, off=0, lead=0):
    R, ncols = n_img * (Hin // P) * (Win // P), Cin * P * P
    n0v = n_img if n0 is None else n0
    return Mat(dtype, A_PATCH_NHWC if nhwc else A_PATCH_NCHW, R, ncols, s1=0 if n0 is None else n0 * Cin * Hin * Win + gap, off=off, n0=n0v,
               Hin=Hin, Win=Win, Cin=Cin, P=P, lead=lead)


class Job:
    def __init__(self, U, V, layout=W_LINEAR, P=0, Co=0, swap=0, bias=True):
        self.U, self.V = (U if isinstance(U, list) else [U]), (V if isinstance(V, list) else [V])
        self.n_seg, self.R, self.I, self.J = len(self.U), self.U[0].R, self.U[0].ncols, self.V[0].ncols
        assert len(self.V) == self.n_seg and all(m.R == self.R for m in self.U + self.V)
        self.layout, self.P, self.Co, self.swap, self.bias = layout, P, Co, swap, bias

    def desc(self):
        return JobDesc(self.U, self.V, self.n_seg, self.R, self.I, self.J, self.layout)


BIG_WS = 32 << 20
F32_BARS, F32_SUM_BARS, BF16_BARS, SUM_TERMS = (2e-5, 1e-4), (1e-4, 5e-4), (5e-3, 1.6e-2), 4096      # tests/test_hip_train_ops.py


class Case:
    def __init__(self, group, name, entry, jobs, compute, ws=0, options=None, accumulate=0, vkey=None):
        self.group, self.name, self.entry, self.compute, self.options, self.accumulate = group, name, entry, compute, dict(options or {}), accumulate
        self.jobs = jobs if isinstance(jobs, list) else [jobs]
        self.ws_bytes = ws
        self.vkey = vkey or f"{group}-{name}"       # cases with one vkey and the same shapes draw the same values
        self.plan = self.route_for()
        self.route = self.plan.name
        short = self.route.split("]:")[0] + "]" if self.route.startswith("one-by-one") else self.route      # (the launches are in .route)
        self.id = f"{group}-{name}-{'bf16' if compute == BF16 else 'fp32'}-{short}".replace(" ", "")

    def route_for(self, mats=None, ws_ptr=0):
        """The plan of this case; `mats` replaces the row matrices (job -> (U list, V list)) with ones that carry real pointers."""
        j = self.jobs[0]
        get = (lambda k: (self.jobs[k].U, self.jobs[k].V)) if mats is None else (lambda k: mats[k])
        if self.entry == "one":
            return wgrad_plan("one", get(0)[0][0], get(0)[1][0], 1, j.R, j.I, j.J, self.compute, self.ws_bytes, self.options, ws_ptr)
        if self.entry == "multi":
            return wgrad_plan("multi", get(0)[0], get(0)[1], j.n_seg, j.R, j.I, j.J, self.compute, self.ws_bytes, self.options, ws_ptr)
        descs = [JobDesc(get(k)[0], get(k)[1], jb.n_seg, jb.R, jb.I, jb.J, jb.layout) for k, jb in enumerate(self.jobs)]
        return wgrad_plan("jobs", descs, None, 0, 0, 0, 0, self.compute, self.ws_bytes, self.options, ws_ptr)

    @property
    def acc(self):
        return 1 if self.entry == "jobs" else self.accumulate

    def rounds_sources(self):
        """bf16 compute on fp32 sources: the generic kernel rounds the operands (pack_bf16x2, to nearest even)."""
        return self.compute == BF16 and any(m.dtype == F32 for jb in self.jobs for m in jb.U + jb.V)

    def bars(self, job, exact=True):
        """fp32 bars (wider past 4096 summed terms) wherever only the fp32 accumulation differs from the reference; the bf16 bars for the
        unrounded reference of a case whose sources the kernel rounds."""
        if not exact and self.rounds_sources():
            return BF16_BARS
        return F32_BARS if job.R * job.n_seg <= SUM_TERMS else F32_SUM_BARS


class Inputs:
    pass


def _draw(key, R, ncols, shift):
    gen = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    return torch.randn(R, (ncols + 3) // 4 * 4, generator=gen)[:, :ncols] + shift


def make_inputs(c):
    """Per job and segment: the flat source buffers (NaN wherever no element of the matrix lives) and the matrices as the kernel reads them
    (gathered back through rm_index); the gradient slots' pre-fill.  U carries a +0.25 offset: its column sum is the bias gradient."""
    inp = Inputs()
    inp.bufs, inp.mats, inp.pre = [], [], []
    for k, jb in enumerate(c.jobs):
        bufs, mats = [], []
        for side, ms, ncols in (("U", jb.U, jb.I), ("V", jb.V, jb.J)):
            bl, ml = [], []
            for g, m in enumerate(ms):
                tdt = torch.bfloat16 if m.dtype == BF16 else torch.float32
                vals = _draw(f"{c.vkey}/{k}/{g}/{side}", jb.R, ncols, 0.25 if side == "U" else 0.0).to(tdt)
                idx = rm_index(m, jb.R, ncols) + m.lead
                assert int(idx.min()) >= 0 and idx.unique().numel() == idx.numel()
                buf = torch.full((int(idx.max()) + 1 + 8,), float("nan"), dtype=tdt)
                buf[idx.reshape(-1)] = vals.reshape(-1)
                bl.append(buf)
                ml.append(buf[idx].double())
            bufs.append(bl)
            mats.append(ml)
        inp.bufs.append(bufs)
        inp.mats.append(mats)
        gen = torch.Generator().manual_seed(zlib.crc32(f"{c.vkey}/{k}/pre".encode()))
        inp.pre.append((torch.randn(jb.I * jb.J, generator=gen), torch.randn(jb.I, generator=gen)))
    return inp


BUGS = ("drop_tail", "drop_split", "drop_segment", "double_chunk", "swap_colgroups", "transpose_tile")


def bug_applies(c, bug):
    jb, l = c.jobs[0], c.plan.launches[0]
    if bug == "drop_tail":
        return jb.R % RC != 0 and l.name.startswith("gen<")
    if bug == "drop_split":
        return l.split > 1
    if bug == "drop_segment":
        return jb.n_seg > 1
    if bug == "double_chunk":
        return jb.R >= 2 * WRC
    if bug == "swap_colgroups":
        return jb.J >= 32
    return min(jb.I, jb.J) >= 16


def reference(c, inp=None, exact_bf16=False, bug=None):
    """Per job: (dW scattered into the flat parameter, dbias or None), float64, on top of the pre-fill when the case accumulates.
    exact_bf16: fp32 operands rounded to bf16 first (what the generic kernel multiplies in bf16 compute).  bug: one of BUGS, applied to the
    first job -- the wrong results the bars must see."""
    inp = make_inputs(c) if inp is None else inp
    out = []
    for k, jb in enumerate(c.jobs):
        dW, db = torch.zeros(jb.I, jb.J, dtype=torch.float64), torch.zeros(jb.I, dtype=torch.float64)
        for g in range(jb.n_seg):
            U, V = inp.mats[k][0][g], inp.mats[k][1][g]
            if exact_bf16 and c.compute == BF16:
                U, V = U.float().bfloat16().double(), V.float().bfloat16().double()
            w = torch.ones(jb.R, dtype=torch.float64)
            if bug and k == 0:
                last = g == jb.n_seg - 1
                if bug == "drop_tail" and last:
                    w[jb.R - jb.R % RC:] = 0
                if bug == "drop_split" and last:
                    a, b = c.plan.launches[-1].ranges[-1] if c.entry != "jobs" else c.plan.launches[0].ranges[-1]
                    w[a:b] = 0
                if bug == "drop_segment" and last:
                    w[:] = 0
                if bug == "double_chunk" and g == 0:
                    w[WRC:2 * WRC] = 2
            dW += U.t() @ (V * w[:, None])
            db += (U * w[:, None]).sum(0)
        if bug == "swap_colgroups" and k == 0:
            dW = torch.cat([dW[:, 16:32], dW[:, :16], dW[:, 32:]], 1)
        if bug == "transpose_tile" and k == 0:
            t = min(jb.I, jb.J, WT)
            dW = dW.clone()
            dW[:t, :t] = dW[:t, :t].t().clone()
        flat = torch.zeros(jb.I * jb.J, dtype=torch.float64)
        flat[out_index(jb.layout, jb.I, jb.J, jb.P, jb.Co, jb.swap).reshape(-1)] = dW.reshape(-1)
        if c.acc:
            flat, db = flat + inp.pre[k][0].double(), db + inp.pre[k][1].double()
        out.append((flat, db if jb.bias else None))
    return out


def errors(got, ref):
    """(relative L2, max-norm) of got against ref; infinite when got is not finite."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    return float((got - ref).norm() / (ref.norm() + 1e-300)), float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def _dt(compute):
    return BF16 if compute == BF16 else F32


def _patch_operand(kind, dtype, n_img):
    """A patch operand that stages as `kind`."""
    if kind == "PATCH_NHWC":       # 7 x 5 patches per image: R = 35 n_img is odd with n_img
        return patches(dtype, True, n_img, 14, 10, 4, 2)
    if kind == "PATCH_NCHW2":      # 7 x 8 patches per image
        return patches(dtype, False, n_img, 14, 16, 4, 2)
    assert kind == "GEN_PATCH"     # P = 4 on a channels-first image: no fast gather
    return patches(dtype, False, n_img, 28, 20, 2, 4)


def build_cases():
    cs = []

    def add(*a, **k):
        cs.append(Case(*a, **k))
        return cs[-1]
    # (a) staging modes: the six (MU, MV) pairs x {fp32 T64, bf16 T64, bf16 T128} x {atomic, slab}
    for compute, T in ((F32, 64), (BF16, 64), (BF16, 128)):
        I = 40 if T == 64 else 72
        sd = _dt(compute)
        for ep in ("atomic", "slab"):
            n_img = 3 if ep == "atomic" else 17          # 105 / 595 rows of 7 x 5 patches, 168 / 952 of 7 x 8
            Rl = 333 if ep == "atomic" else 589
            ws = 0 if ep == "atomic" else BIG_WS
            tag = f"T{T}-{ep}"
            add("a", f"row-row-{tag}", "one", Job(rows(sd, Rl, I, pad=4, off=4), rows(sd, Rl, 36, pad=8)), compute, ws)
            add("a", f"col-col-{tag}", "one", Job(lines(Rl, I), lines(Rl, 36, n0=8, es=8, gap=0, off=0)), compute, ws)
            for kind in ("PATCH_NHWC", "PATCH_NCHW2", "GEN_PATCH"):
                V = _patch_operand(kind, sd, n_img)
                add("a", f"row-{kind.lower()}-{tag}", "one", Job(rows(sd, V.R, I, pad=4), V), compute, ws)
            add("a", f"gen-gen-{tag}", "one", Job(rows(sd, Rl, I, pad=4, lead=2 if sd == BF16 else 1), rows(sd, Rl, 36)), compute, ws)
    # bf16 compute on fp32 rows (the kernel rounds), fp32 compute on bf16 rows (exact)
    add("a", "f32rows-bf16compute", "one", Job(rows(F32, 333, 40, pad=4), rows(F32, 333, 36)), BF16)
    add("a", "bf16rows-fp32compute", "one", Job(rows(BF16, 333, 40, pad=4), rows(BF16, 333, 36)), F32)
    # I, J no tile multiples over several tiles; R ragged
    for compute in (F32, BF16):
        add("a", "72x132", "one", Job(rows(_dt(compute), 333, 72, pad=4, off=4), rows(_dt(compute), 333, 132)), compute)
        add("a", "72x132-lines", "one", Job(lines(333, 72), lines(333, 132, n0=16, es=20)), compute)
        # n0 / s1 blocks: 4-row blocks straddle two blocks (n0 = 6) or never do (n0 = 8)
        for n0 in (6, 8):
            add("a", f"blocks-n0={n0}", "one", Job(rows(_dt(compute), 333, 40, pad=4, off=4, n0=n0, gap=8), rows(_dt(compute), 333, 36, n0=n0, gap=4)), compute)
        # frames inside a rollout buffer: image blocks of n0 = 2, a gap between blocks
        for kind, nhwc, geo in (("nhwc", True, (14, 10, 4, 2)), ("nchw2", False, (14, 16, 4, 2))):
            V = patches(_dt(compute), nhwc, 5, *geo, n0=2, gap=16, off=8)
            add("a", f"frames-{kind}", "one", Job(rows(_dt(compute), V.R, 40), V), compute)
    # every reason to leave a fast gather, next to the twin that stays on it (same values)
    for compute in (F32, BF16):
        sd = _dt(compute)
        one = 2 if sd == BF16 else 1                      # elements in 4 bytes
        add("a", "twin-rows", "one", Job(rows(sd, 333, 40, pad=4), rows(sd, 333, 36)), compute, vkey="a-rows")
        add("a", "v+4B", "one", Job(rows(sd, 333, 40, pad=4), rows(sd, 333, 36, lead=one)), compute, vkey="a-rows")
        add("a", "u+4B", "one", Job(rows(sd, 333, 40, pad=4, lead=one), rows(sd, 333, 36)), compute, vkey="a-rows")
        add("a", "twin-J68", "one", Job(rows(sd, 333, 40), rows(sd, 333, 68, pad=4)), compute, vkey="a-ncols")
        add("a", "ncols%4-J66", "one", Job(rows(sd, 333, 40), rows(sd, 333, 66, pad=6)), compute, vkey="a-ncols")
        for name, nhwc, geo in (("Cin%4", True, (14, 10, 6, 2)), ("Win%8", False, (14, 12, 4, 2)), ("P=4-nchw", False, (28, 20, 2, 4))):
            V = patches(sd, nhwc, 3, *geo)
            add("a", f"twin-{name}", "one", Job(rows(sd, V.R, 40), rows(sd, V.R, V.ncols)), compute, vkey=f"a-{name}")
            add("a", name, "one", Job(rows(sd, V.R, 40), V), compute, vkey=f"a-{name}")
        for kind, nhwc, geo in (("nhwc", True, (14, 10, 4, 2)), ("nchw2", False, (14, 16, 4, 2))):
            add("a", f"twin-{kind}", "one", Job(rows(sd, 3 * 7 * geo[1] // 2, 40), patches(sd, nhwc, 3, *geo)), compute, vkey=f"a-img-{kind}")
            add("a", f"{kind}+4B", "one", Job(rows(sd, 3 * 7 * geo[1] // 2, 40), patches(sd, nhwc, 3, *geo, lead=one)), compute, vkey=f"a-img-{kind}")
    # (b) layouts x swap x dbias, accumulate alternating; the natural operands of each parameter
    P, Ci, Co = 2, 4, 6
    n = 0
    for layout in (W_LINEAR, W_CONV_NHWC, W_DECONV_NHWC, W_DECONV_NCHW):
        for swap in (0, 1):
            for bias in (True, False):
                compute = (F32, BF16)[n % 2]
                sd = _dt(compute)
                acc = (n // 2 + n) % 2
                n += 1
                if layout == W_LINEAR:
                    A, B, Cother = rows(sd, 333, 20, pad=4), rows(sd, 333, 12), 0
                elif layout == W_CONV_NHWC:          # n = cout rows (dPre), k = (kh, kw, ci) patches of the channels-last input
                    B = patches(sd, True, 3, 14, 10, Ci, P)
                    A, Cother = rows(sd, B.R, Co), Ci
                    if swap:
                        A, B = B, A
                elif layout == W_DECONV_NHWC:        # k = cin rows (pixels), n = (kh, kw, co) patches of the channels-last output gradient
                    A = patches(sd, True, 3, 14, 10, Co, P)
                    B, Cother = rows(sd, A.R, Ci), Co
                    if swap:
                        A, B = B, A
                else:                                # k = cin rows, n = (co, kh, kw) patches of the channels-first output gradient
                    A = patches(sd, False, 3, 14, 16, Co, P)
                    B, Cother = rows(sd, A.R, Ci), Co
                    if swap:
                        A, B = B, A
                add("b", f"{LAYOUT_NAMES[layout]}-swap{swap}-{'bias' if bias else 'nobias'}-acc{acc}", "one",
                    Job(A, B, layout=layout, P=P, Co=Cother, swap=swap, bias=bias), compute, accumulate=acc)
    # (c) the single-tile slab form
    for compute in (F32, BF16):
        sd = _dt(compute)

        def st(name, R, ws=BIG_WS, **k):
            return add("c", name, "one", Job(rows(sd, R, 24, pad=4), rows(sd, R, 16), bias=k.pop("bias", True)), compute, ws, **k)
        for R in (511, 512, 513):
            st(f"R{R}", R, accumulate=R % 2)
        st("split63", 63 * RC)
        st("split64", 64 * RC)
        st("split65-ragged", 64 * RC + 5, bias=False)
        st("ws-limits-split", 4096, ws=10 * (24 * 16 + 24) * 4)
        st("ws-two-partials", 4096, ws=2 * (24 * 16 + 24) * 4)
        st("ws-below-two-partials", 4096, ws=2 * (24 * 16 + 24) * 4 - 16)
        st("ws-below-one-partial", 4096, ws=16, accumulate=1)
        st("slab-wgs-80", 8192, options={"TANTE_WGRAD_SLAB_WGS": 80})
    # (d) the transposed-read path
    def tr_job(R, I, J, n_seg=1, pad=0, off=0, bias=True, lead=0):
        return Job([rows(BF16, R, I, pad=pad, off=off, lead=lead) for _ in range(n_seg)], [rows(BF16, R, J, pad=pad, off=off) for _ in range(n_seg)], bias=bias)
    for I, J in ((128, 128), (256, 128), (128, 256), (256, 384)):
        add("d", f"{I}x{J}", "one", tr_job(32 * 12, I, J, bias=(I + J) % 256 == 0), BF16, vkey=f"d-{I}x{J}")
        add("d", f"{I}x{J}-ws", "multi", tr_job(32 * 12, I, J, n_seg=2, pad=8, off=8, bias=(I + J) % 256 != 0), BF16, BIG_WS, accumulate=1)
    for nch in (1, 2, 3, 4, 5, 8, 9):
        add("d", f"one-split-{nch}chunks", "one", tr_job(32 * nch, 128, 128), BF16, options={"TANTE_WGRAD_TR_WGS": 1})
        add("d", f"one-split-{nch}chunks-ws", "multi", tr_job(32 * nch, 128, 128, n_seg=2), BF16, BIG_WS, options={"TANTE_WGRAD_TR_WGS": 1})
    for R in (32 * 12, 32 * 13, 4064):
        add("d", f"per-search-R{R}", "one", tr_job(R, 128, 256, pad=8, off=8), BF16, vkey=f"d-R{R}")
        add("d", f"per-search-R{R}-ws", "multi", tr_job(R, 256, 128, n_seg=3, bias=False), BF16, BIG_WS)
    add("d", "ws-too-small", "multi", tr_job(32 * 16, 128, 128, n_seg=2), BF16, 4096)
    add("d", "no-slab", "multi", tr_job(32 * 16, 128, 128, n_seg=2), BF16, BIG_WS, options={"TANTE_WGRAD_NO_SLAB": 1}, vkey="d-noslab")
    add("d", "twin-no-slab", "multi", tr_job(32 * 16, 128, 128, n_seg=2), BF16, BIG_WS, vkey="d-noslab")
    add("d", "R%32", "one", tr_job(32 * 12 + 8, 128, 128), BF16)
    add("d", "s0%8", "one", tr_job(32 * 12, 128, 128, pad=4), BF16)
    add("d", "I192", "one", tr_job(32 * 12, 192, 128), BF16)
    add("d", "u+4B", "one", tr_job(32 * 12, 128, 128, lead=2), BF16)
    for I, J in ((128, 128), (256, 384)):
        add("d", f"no-tr-{I}x{J}", "one", tr_job(32 * 12, I, J, bias=(I + J) % 256 == 0), BF16, options={"TANTE_WGRAD_NO_TR": 1}, vkey=f"d-{I}x{J}")
    for nch in (1, 7, 8, 9, 17):
        o = {"TANTE_WGRAD_DEEP": 1, "TANTE_WGRAD_TR_WGS": 1}
        add("d", f"deep-{nch}chunks", "one", tr_job(32 * nch, 128, 128), BF16, options=o, vkey=f"d-deep{nch}")
        add("d", f"twin-deep-{nch}chunks", "one", tr_job(32 * nch, 128, 128), BF16, options={"TANTE_WGRAD_TR_WGS": 1}, vkey=f"d-deep{nch}")
    add("d", "deep-ws", "multi", tr_job(32 * 36, 128, 256, n_seg=2), BF16, BIG_WS, options={"TANTE_WGRAD_DEEP": 1})
    for nch in (6, 16, 24):
        add("d", f"rg2-{nch}chunks", "multi", tr_job(32 * nch, 256, 128, n_seg=2, bias=nch != 16), BF16, BIG_WS, options={"TANTE_WGRAD_RG": 2}, vkey=f"d-rg{nch}")
        add("d", f"twin-rg2-{nch}chunks", "multi", tr_job(32 * nch, 256, 128, n_seg=2, bias=nch != 16), BF16, BIG_WS, options={"TANTE_WGRAD_DEEP": 1}, vkey=f"d-rg{nch}")
    add("d", "rg2-5chunks-refused", "multi", tr_job(32 * 5, 128, 128, n_seg=2), BF16, BIG_WS, options={"TANTE_WGRAD_RG": 2})
    # (e) tante_wgrad_multi_ws
    for n_seg in (2, 8, 9, 11):
        add("e", f"{n_seg}seg", "multi", tr_job(32 * 8, 128, 128, n_seg=n_seg, bias=n_seg != 8), BF16, BIG_WS, accumulate=n_seg % 2)
    add("e", "3seg-no-ws", "multi", tr_job(32 * 8, 128, 256, n_seg=3), BF16, 0)
    jb = tr_job(32 * 8, 128, 128, n_seg=3)
    jb.U[1] = rows(BF16, 32 * 8, 128, pad=8)
    add("e", "3seg-one-s0-differs", "multi", jb, BF16, BIG_WS)
    add("e", "3seg-fp32", "multi", tr_job(32 * 8, 128, 128, n_seg=3), F32, BIG_WS)
    add("e", "2seg-gen", "multi", Job([rows(BF16, 333, 40), rows(BF16, 333, 40, pad=4)], [rows(BF16, 333, 36), rows(BF16, 333, 36)]), BF16, BIG_WS)
    # (f) tante_wgrad_jobs_ws
    def jobs_of(shapes):
        out = []
        for R, I, J, n_seg, layout, swap, bias in shapes:
            jb = tr_job(R, I, J, n_seg=n_seg, pad=8 if bias else 0, bias=bias)
            jb.layout, jb.swap = layout, swap
            if layout != W_LINEAR:                   # a 2 x 2 transposed convolution's weight (cin, cout, 2, 2): n = (co, kh, kw) or (kh, kw, co)
                jb.P, jb.Co = 2, (J if swap else I) // 4
            out.append(jb)
        return out
    S = [(32 * 13, 128, 128, 1, W_LINEAR, 0, True), (32 * 8, 256, 128, 3, W_LINEAR, 1, False), (32 * 20, 128, 256, 2, W_DECONV_NCHW, 1, True),
         (32 * 9, 128, 128, 8, W_DECONV_NHWC, 1, False)]
    add("f", "2jobs", "jobs", jobs_of(S[:2]), BF16, BIG_WS)
    add("f", "3jobs", "jobs", jobs_of(S[:3]), BF16, BIG_WS)
    add("f", "4jobs", "jobs", jobs_of(S), BF16, BIG_WS, vkey="f-4jobs")
    add("f", "4jobs-one-by-one", "jobs", jobs_of(S), BF16, BIG_WS, options={"TANTE_WGRAD_JOBS": 0}, vkey="f-4jobs")
    add("f", "2jobs-wgs8", "jobs", jobs_of([(32 * 16, 128, 128, 4, W_LINEAR, 0, True), (32 * 12, 128, 128, 4, W_LINEAR, 0, True)]), BF16, BIG_WS,
        options={"TANTE_WGRAD_JOBS_WGS": 8})
    add("f", "1job", "jobs", jobs_of(S[1:2]), BF16, BIG_WS)
    add("f", "5jobs", "jobs", jobs_of(S + S[:1]), BF16, BIG_WS)
    add("f", "job-R%32", "jobs", jobs_of([S[0], (32 * 8 + 8, 128, 128, 2, W_LINEAR, 0, True)]), BF16, BIG_WS)
    add("f", "ws-too-small", "jobs", jobs_of(S[:2]), BF16, 1 << 16)
    return cs


CASES = build_cases()
