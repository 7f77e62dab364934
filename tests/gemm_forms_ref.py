"""The GEMM front end (tante_gemm, tante_amd/csrc/gemm.hip) restated for its tests: float64 references of the descriptor's semantics
as include/tante_hip.h states them, the exact-bf16 evaluation of the same expressions, the dispatch rule as a function of the
descriptor (`gemm_route`), and the list of cases tests/test_hip_gemm_forms.py runs.  Plain torch on the CPU: tests/test_gemm_forms_cpu.py
pins the references to oracle.tante_oracle, the dispatch table to the text of gemm.hip, and the bars to wrong results.

A case is data only.  `make_inputs(case)` draws its operands and lays them out in flat buffers by the header's addressing formulas (NaN
wherever the descriptor must not read); `reference(case, inp)` computes the expected output from the LOGICAL operands (the dense rows /
the images / the weight in its source layout) with plain torch, so a mistake in the addressing cannot cancel between the two."""
import math
import types
import zlib

import torch

F32, BF16 = 0, 1                                            # include/tante_hip.h
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU = 0, 1, 2, 3
A_LINEAR, A_PATCH_NHWC, A_PATCH_NCHW = 0, 1, 2
E_LINEAR, E_FILM, E_DECONV_NHWC, E_DECONV_NCHW = 0, 1, 2, 3
W_LINEAR, W_CONV_NHWC, W_DECONV_NHWC, W_DECONV_NCHW, W_LINEAR_T, W_CONV_NHWC_T, W_DECONV_NHWC_T, W_DECONV_NCHW_T = range(8)

ACT_NAME = {ACT_NONE: "none", ACT_GELU_ERF: "gelu_erf", ACT_GELU_TANH: "gelu_tanh", ACT_RELU: "relu"}
ACT_CODE = {v: k for k, v in ACT_NAME.items()}

# the project's per-format bars: relative L2, max-norm against float64
BARS = {"fp32": (2e-5, 1e-4), "bf16": (1e-2, 2e-2)}

# one K per chunk-block count CB (k_pad = CB * 32 in bf16, CB * 16 in fp32)
K_OF_CB = {"bf16": {2: 64, 4: 128, 8: 256, 16: 512}, "fp32": {2: 32, 4: 64, 8: 128, 16: 256, 32: 512}}


# ---- the dispatch, restated --------------------------------------------------------------------------------------------------------
SMALL_M_MAX = 1024          # tante_opt("TANTE_GEMM_SMALLM", 1024)
SMALL_K = 512               # gemm_small_kernel: CB = 16 in bf16
LITE_M_MIN = 4096           # gemm_lite_kernel: M >= 4096
LITE_CBS = (4, 8, 16)       # try_lite<CB> is instantiated for 4 <= CB <= 16 (bf16): K = CB * 32 in {128, 256, 512}
PATCH_LITE_CBS = (8, 16)
K_MAX = 512

# launch_gemm's list of dedicated kernels, in its order: (LN, AM, EP); anything else runs (LN, AM_GEN, EP_GEN)
KERNEL_VARIANTS = [
    (True, "AM_LIN", "EP_LIN_NONE"), (True, "AM_LIN", "EP_LIN_GELU_TANH"), (True, "AM_LIN", "EP_LIN_GELU_ERF"),
    (False, "AM_LIN", "EP_LIN_NONE"), (False, "AM_LIN", "EP_LIN_RELU"), (False, "AM_LIN", "EP_LIN_GELU_ERF"),
    (False, "AM_LIN", "EP_LIN_GELU_TANH"), (False, "AM_NCHW2", "EP_LIN_GELU_ERF"), (False, "AM_NCHW2", "EP_LIN_NONE"),
    (False, "AM_NHWC", "EP_LIN_GELU_ERF"), (False, "AM_NHWC", "EP_FILM"), (False, "AM_LIN", "EP_DNHWC_GELU_ERF"),
    (False, "AM_LIN", "EP_DNCHW_NONE"), (False, "AM_LIN", "EP_DNHWC_NONE"), (False, "AM_NHWC", "EP_LIN_NONE"),
    (True, "AM_GEN", "EP_GEN"), (False, "AM_GEN", "EP_GEN"),
]
SMALL_VARIANTS = [(True, "EP_LIN_NONE"), (True, "EP_LIN_GELU_ERF"), (False, "EP_LIN_NONE"), (False, "EP_LIN_GELU_ERF")]
# launch_lite<CB, EP, TR, AM>: (EP, TR, AM).  TR: 0 plain, 1 dropout, 2 act', 3 / 4 channels-first rows (none / GELU), 5 / 6 the 2 x 2
# channels-first pixel shuffle (none / GELU).  AM: 0 bf16 rows, 5 fp32 rows, 1 - 4 patch fragments (P 4 bf16 / fp32, P 2 bf16 / fp32).
LITE_PLAIN = [("EP_LIN_NONE", 0, 0), ("EP_LIN_RELU", 0, 0), ("EP_LIN_GELU_TANH", 0, 0), ("EP_LIN_GELU_ERF", 0, 0)]
LITE_DNCHW2 = [("EP_LIN_NONE", 5, 0), ("EP_LIN_NONE", 6, 0), ("EP_LIN_NONE", 5, 5), ("EP_LIN_NONE", 6, 5)]
LITE_TRAIN = [("EP_LIN_NONE", 1, 0), ("EP_LIN_NONE", 2, 0)]
LITE_PATCH = [(ep, tr, am) for am in (1, 2, 3, 4) for ep, tr in (("EP_LIN_NONE", 3), ("EP_LIN_NONE", 4), ("EP_LIN_NONE", 0), ("EP_LIN_GELU_ERF", 0))]

# forms this file's cases leave to other tests (by route family -> the test that runs it alone)
COVERED_ELSEWHERE = {
    "lite-train": ("lite<CB*,EP_LIN_NONE,TR1,AM0> / TR2: the dropout and activation-gradient epilogues",
                   "tests/test_hip_parity.py::test_gemm_training_epilogues and the BranchOutFn cases of tests/test_hip_train_nodes.py"),
    "lite-patch": ("lite<CB8|CB16,*,TR0|TR3|TR4,AM1..4>: the patch gather as the fragment load, a_pad",
                   "tests/test_hip_round5.py::test_conv_stage_gathers_patches_inside_the_gemm"),
}


class Refused(Exception):
    """gemm_route: tante_gemm refuses the descriptor before any launch (the message is the C side's)."""


def pack_geom(N, K, compute):
    kb = 32 if compute == BF16 else 16
    need = (K + kb - 1) // kb
    cb = 2
    while cb < need:
        cb *= 2
    if cb > (16 if compute == BF16 else 32):
        raise Refused("exceeds the register-stationary limit")
    nt = min(512 // cb, 64)
    n_pad = (N + nt - 1) // nt * nt
    return types.SimpleNamespace(cb=cb, k_pad=cb * kb, nt=nt, n_pad=n_pad, n_tiles=n_pad // nt)


def _addr(p):
    if p is None:
        return 0
    return int(p) if not hasattr(p, "value") else int(p.value or 0)


def _patch_lite_ok(g, flags, cb):
    e_lin = bool(flags & 2) and g.e_mode == E_LINEAR
    e_cf = g.e_mode == E_DECONV_NCHW and g.Po == 1 and g.out_dtype == F32 and g.N % 4 == 0 and _addr(g.out) % 4 == 0
    return (g.a_mode == A_PATCH_NCHW and g.compute == BF16 and not g.ln and g.drop_p <= 0 and not _addr(g.dact) and (e_lin or e_cf)
            and cb in PATCH_LITE_CBS and g.K == cb * 32 and g.M >= LITE_M_MIN and g.P in (2, 4) and _addr(g.a) % 16 == 0
            and g.a_dtype in (BF16, F32) and (g.a_pad == 0 or (g.a_pad == 1 and g.P == 4)) and g.act in (ACT_NONE, ACT_GELU_ERF))


def gemm_route(g, small_m=SMALL_M_MAX, no_lite=False):
    """The kernel template a descriptor reaches.  `g` has the fields of TanteGemm (a tante_amd._lib.Gemm, or any object with the same
    attribute names); pointers count only through their alignment.  Raises Refused where tante_gemm returns an error."""
    if g.M <= 0 or g.N <= 0 or g.K <= 0:
        raise Refused("bad shape")
    geo = pack_geom(g.N, g.K, g.compute)
    bf = g.compute == BF16
    E = 8 if bf else 4
    al = E if g.a_dtype == BF16 else 4
    a, out, res, dact = _addr(g.a), _addr(g.out), _addr(g.residual), _addr(getattr(g, "dact", 0))
    flags = 0
    if g.a_mode == A_LINEAR:
        if g.a_n0 <= 0:
            raise Refused("a_n0 must be > 0")
        if a % 16 == 0 and g.a_s1 % al == 0 and g.a_s0 % al == 0 and g.a_off % al == 0:
            flags |= 1
    else:
        if g.P <= 0 or g.Hin % g.P or g.Win % g.P or g.Cin <= 0:
            raise Refused("bad patch geometry")
        if g.K != g.Cin * g.P * g.P:
            raise Refused("K != Cin*P*P")
        if g.M % ((g.Hin // g.P) * (g.Win // g.P)):
            raise Refused("M is not a whole number of images")
        if g.a_n0 <= 0:
            raise Refused("a_n0 (images per batch item) must be > 0")
        if g.a_s1 % 4 or g.a_off % 4:
            raise Refused("image strides must be multiples of 4 elements")
        if g.a_mode == A_PATCH_NHWC and a % 16 == 0 and (g.P * g.Cin) % E == 0 and g.Cin % al == 0:
            flags |= 1
    o_ok = out % 16 == 0
    if g.e_mode == E_LINEAR:
        if o_ok and g.N % 4 == 0 and g.out_ld % 4 == 0 and (not res or (g.res_ld % 4 == 0 and res % 16 == 0)):
            flags |= 2
    elif g.e_mode == E_FILM:
        if g.T <= 0 or g.HW <= 0:
            raise Refused("FILM epilogue needs tables")
        if o_ok and g.N % 4 == 0 and g.out_ld % 4 == 0:
            flags |= 2
    else:
        if g.Hi <= 0 or g.Wi <= 0 or g.Po <= 0 or g.Cout <= 0:
            raise Refused("bad deconv geometry")
        if g.N != g.Cout * g.Po * g.Po:
            raise Refused("N != Cout*P*P")
        if g.M % (g.Hi * g.Wi):
            raise Refused("M is not a whole number of images")
        if g.e_mode == E_DECONV_NCHW and g.out_dtype != F32:
            raise Refused("NCHW output is fp32")
        if g.e_mode == E_DECONV_NHWC and o_ok and g.Cout % 4 == 0:
            flags |= 2
    drop = g.drop_p > 0
    train_epi = drop or bool(dact)
    dact_scatter = bool(dact) and not drop and g.e_mode == E_DECONV_NHWC and bool(flags & 2) and g.act == ACT_NONE and dact % 16 == 0
    if train_epi and not dact_scatter and (not bf or g.e_mode != E_LINEAR or g.a_mode != A_LINEAR or g.a_dtype != BF16 or g.ln or g.act != ACT_NONE
                                           or (flags & 3) != 3 or g.M < LITE_M_MIN or g.K not in (128, 256, 512) or (drop and dact)
                                           or (dact and (dact % 16 or g.N % 4))):
        raise Refused("the dropout / activation-gradient epilogues need dense 16-byte aligned bf16 rows")
    if g.a_pad < 0 or (g.a_pad != 0 and not _patch_lite_ok(g, flags, geo.cb)):
        raise Refused("a_pad needs a channels-first bf16-compute patch stage")
    cb = geo.cb
    if cb == 32 and bf:
        raise Refused("K too large for bf16 path")
    # launch_gemm
    k_ok = g.K % E == 0
    am = "AM_GEN"
    if (flags & 1) and k_ok and g.a_mode == A_LINEAR:
        am = "AM_LIN"
    if (flags & 1) and k_ok and g.a_mode == A_PATCH_NHWC:
        am = "AM_NHWC"
    if g.a_mode == A_PATCH_NCHW and g.P == 2 and g.a_dtype == F32 and g.Win % 2 == 0 and a % 8 == 0:
        am = "AM_NCHW2"
    ov = bool(flags & 2)
    ep = "EP_GEN"
    if ov and g.e_mode == E_LINEAR:
        ep = {ACT_NONE: "EP_LIN_NONE", ACT_RELU: "EP_LIN_RELU", ACT_GELU_TANH: "EP_LIN_GELU_TANH"}.get(g.act, "EP_LIN_GELU_ERF")
    elif ov and g.e_mode == E_FILM and g.act == ACT_NONE:
        ep = "EP_FILM"
    elif ov and g.e_mode == E_DECONV_NHWC and g.act == ACT_GELU_ERF:
        ep = "EP_DNHWC_GELU_ERF"
    elif ov and g.e_mode == E_DECONV_NHWC and g.act == ACT_NONE:
        ep = "EP_DNHWC_NONE"
    elif g.e_mode == E_DECONV_NCHW and g.act == ACT_NONE:
        ep = "EP_DNCHW_NONE"
    ln = bool(g.ln)
    lnn = "LN" if ln else "noLN"
    # try_small
    if bf and cb == 16 and not (g.M > small_m or g.K != SMALL_K or am != "AM_LIN" or (flags & 3) != 3 or g.e_mode != E_LINEAR or drop or dact):
        if (ln, ep) in SMALL_VARIANTS:
            return f"small<{lnn},{ep}>"
    # try_lite
    if bf and cb in LITE_CBS:
        lite = _lite_form(g, flags, cb, no_lite, drop, dact)
        if lite is not None:
            return "lite<CB%d,%s,TR%d,AM%d>" % ((cb,) + lite)
    if (ln, am, ep) not in KERNEL_VARIANTS:
        am, ep = "AM_GEN", "EP_GEN"
    return f"kernel<{'bf16' if bf else 'fp32'},CB{cb},{lnn},{am},{ep}>"


def _lite_form(g, flags, cb, off, drop, dact):
    if g.a_mode == A_PATCH_NCHW:
        if (off and not g.a_pad) or not _patch_lite_ok(g, flags, cb) or cb < 8:
            return None
        am = (1 if g.a_dtype == BF16 else 2) if g.P == 4 else (3 if g.a_dtype == BF16 else 4)
        if g.e_mode == E_DECONV_NCHW:
            return ("EP_LIN_NONE", 3 if g.act == ACT_NONE else 4, am)
        return ("EP_LIN_NONE" if g.act == ACT_NONE else "EP_LIN_GELU_ERF", 0, am)
    if g.a_mode == A_LINEAR and g.e_mode == E_DECONV_NCHW:
        if (off or g.ln or drop or dact or g.Po != 2 or g.out_dtype != F32 or not (flags & 1) or g.K != cb * 32 or g.M < LITE_M_MIN
                or _addr(g.out) % 8 or g.act not in (ACT_NONE, ACT_GELU_ERF) or g.a_dtype not in (BF16, F32)):
            return None
        return ("EP_LIN_NONE", 6 if g.act == ACT_GELU_ERF else 5, 0 if g.a_dtype == BF16 else 5)
    if (off and not drop and not dact) or g.ln or g.a_mode != A_LINEAR or g.a_dtype != BF16 or (flags & 3) != 3 or g.e_mode != E_LINEAR:
        return None
    if g.K != cb * 32 or g.M < LITE_M_MIN:
        return None
    if drop or dact:
        if g.act != ACT_NONE or (drop and dact):
            return None
        return ("EP_LIN_NONE", 1 if drop else 2, 0)
    return ({ACT_NONE: "EP_LIN_NONE", ACT_RELU: "EP_LIN_RELU", ACT_GELU_TANH: "EP_LIN_GELU_TANH", ACT_GELU_ERF: "EP_LIN_GELU_ERF"}[g.act], 0, 0)


def all_routes():
    """Every name gemm_route can return, with the family it belongs to."""
    out = {}
    for mode, cbs in (("bf16", (2, 4, 8, 16)), ("fp32", (2, 4, 8, 16, 32))):
        for cb in cbs:
            for ln, am, ep in KERNEL_VARIANTS:
                out[f"kernel<{mode},CB{cb},{'LN' if ln else 'noLN'},{am},{ep}>"] = "kernel"
    for ln, ep in SMALL_VARIANTS:
        out[f"small<{'LN' if ln else 'noLN'},{ep}>"] = "small"
    for cb in LITE_CBS:
        for fam, forms in (("lite", LITE_PLAIN), ("lite-dnchw2", LITE_DNCHW2), ("lite-train", LITE_TRAIN)):
            for ep, tr, am in forms:
                out["lite<CB%d,%s,TR%d,AM%d>" % (cb, ep, tr, am)] = fam
    for cb in PATCH_LITE_CBS:
        for ep, tr, am in LITE_PATCH:
            out["lite<CB%d,%s,TR%d,AM%d>" % (cb, ep, tr, am)] = "lite-patch"
    return out


def route_template(route):
    """A route without its CB and compute mode: the line of the source it names."""
    import re
    return re.sub(r"(bf16|fp32),CB\d+,|CB\d+,", "", route)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case:
    """One descriptor, as data.  Fields not given keep the defaults below; `id` carries the route."""
    DEFAULTS = dict(
        mode="fp32", a_dtype="f32", out_dtype="f32", M=17, N=64, K=64, a_mode="lin",
        a_n0=None, a_s0=None, a_s1=0, a_off=0, a_lead=0,       # LINEAR addressing (elements); a_lead: elements the pointer sits past a 16-byte boundary
        img=None,                                              # patch modes: dict(B, n0, Ttot, Hin, Win, Cin, P, gap): window of a (B, Ttot, ...) buffer
        ln=False, ln_eps=1e-5, affine="mild", rows="randn",
        act="none", e_mode="lin", out_ld=None, out_lead=0, res=None, res_ld=None, res_lead=0,
        film=None,                                             # (B, T, HW)
        dec=None,                                              # dict(n_img, Hi, Wi, Po, Cout)
        small_m=SMALL_M_MAX, note="")

    def __init__(self, group, name, **kw):
        for k, v in self.DEFAULTS.items():
            setattr(self, k, kw.pop(k, v))
        assert not kw, kw
        self.group, self.name = group, name
        if self.img is not None:
            i = self.img
            self.M = i["B"] * i["n0"] * (i["Hin"] // i["P"]) * (i["Win"] // i["P"])
            self.K = i["Cin"] * i["P"] * i["P"]
        if self.dec is not None:
            d = self.dec
            self.N = d["Cout"] * d["Po"] * d["Po"]
            if self.img is None:
                self.M = d["n_img"] * d["Hi"] * d["Wi"]
        if self.film is not None and self.img is None:
            self.M = self.film[0] * self.film[1] * self.film[2]
        if self.a_n0 is None:
            self.a_n0 = self.M
        if self.a_s0 is None:
            self.a_s0 = self.K
        if self.out_ld is None:
            self.out_ld = self.N + (4 if self.N % 4 == 0 else 3)
        if self.res == "out":
            self.res_ld, self.res_lead = self.out_ld, self.out_lead
        elif self.res == "other" and self.res_ld is None:
            self.res_ld = self.N + 8
        self.seed = zlib.crc32(f"{group}/{name}/{self.mode}".encode())
        self.route = gemm_route(fields(self), small_m=self.small_m)
        self.id = f"{group}-{name}-{self.mode}-{self.route}"

    @property
    def compute(self):
        return BF16 if self.mode == "bf16" else F32

    @property
    def bars(self):
        """The compute format's bar; an fp32-compute result stored as bf16 carries the output rounding on top: bf16 keeps 8 significant bits,
        so rounding to nearest moves an element by at most 2^-8 of itself (its unit roundoff), hence at most 2^-8 in both norms."""
        if self.mode == "fp32" and self.out_dtype == "bf16":
            return (BARS["fp32"][0] + 2.0 ** -8, BARS["fp32"][1] + 2.0 ** -8)
        return BARS[self.mode]

    def operand_rounding_only(self):
        """bf16 compute whose only roundings are the operands': held to the fp32 bar against the exact-bf16 evaluation."""
        return self.mode == "bf16" and not self.ln and self.act in ("none", "relu") and self.out_dtype == "f32"


def _esize(dt):
    return 2 if dt == "bf16" else 4


def fields(c, base=1 << 20):
    """TanteGemm's fields for a case, with stand-in addresses that have the case's alignments (tests fill in the real ones)."""
    g = types.SimpleNamespace()
    g.a = base + c.a_lead * _esize(c.a_dtype)
    g.a_dtype = BF16 if c.a_dtype == "bf16" else F32
    g.a_mode = {"lin": A_LINEAR, "nhwc": A_PATCH_NHWC, "nchw": A_PATCH_NCHW}[c.a_mode]
    g.M, g.K, g.N = c.M, c.K, c.N
    g.a_s1, g.a_s0, g.a_off, g.a_n0 = c.a_s1, c.a_s0, c.a_off, c.a_n0
    g.Hin = g.Win = g.Cin = g.P = 0
    if c.img is not None:
        i = c.img
        g.Hin, g.Win, g.Cin, g.P = i["Hin"], i["Win"], i["Cin"], i["P"]
        chw = i["Cin"] * i["Hin"] * i["Win"]
        g.a_n0, g.a_s1, g.a_off, g.a_s0 = i["n0"], i["Ttot"] * chw + i["gap"], i.get("off", chw), 0
    g.ln, g.ln_eps = int(c.ln), c.ln_eps
    g.compute = c.compute
    g.act = ACT_CODE[c.act]
    g.e_mode = {"lin": E_LINEAR, "film": E_FILM, "dnhwc": E_DECONV_NHWC, "dnchw": E_DECONV_NCHW}[c.e_mode]
    g.out = base + c.out_lead * _esize(c.out_dtype)
    g.out_dtype = BF16 if c.out_dtype == "bf16" else F32
    g.out_ld = c.out_ld
    g.residual = (base + c.res_lead * 4) if c.res else 0
    g.res_ld = c.res_ld or 0
    g.T, g.HW = (c.film[1], c.film[2]) if c.film else (0, 0)
    g.Hi = g.Wi = g.Po = g.Cout = 0
    if c.dec is not None:
        g.Hi, g.Wi, g.Po, g.Cout = c.dec["Hi"], c.dec["Wi"], c.dec["Po"], c.dec["Cout"]
    g.drop_p, g.dact, g.a_pad = 0.0, 0, 0
    return g


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def w_layout(c):
    """(TANTE_W_* layout, source shape, P, C_other) of the weight a case packs."""
    if c.dec is not None:
        d = c.dec
        return (W_DECONV_NCHW if c.e_mode == "dnchw" else W_DECONV_NHWC), (c.K, d["Cout"], d["Po"], d["Po"]), d["Po"], d["Cout"]
    if c.a_mode == "nhwc":
        i = c.img
        return W_CONV_NHWC, (c.N, i["Cin"], i["P"], i["P"]), i["P"], i["Cin"]
    if c.a_mode == "nchw":
        i = c.img
        return W_LINEAR, (c.N, i["Cin"], i["P"], i["P"]), 0, 0
    return W_LINEAR, (c.N, c.K), 0, 0


def row_starts(c, n0=None, s1=None, s0=None, off=None):
    """TANTE_A_LINEAR: element offset of row r."""
    r = torch.arange(c.M)
    n0 = c.a_n0 if n0 is None else n0
    return (r // n0) * (c.a_s1 if s1 is None else s1) + (r % n0) * (c.a_s0 if s0 is None else s0) + (c.a_off if off is None else off)


def image_starts(c, off=None):
    i = c.img
    g = fields(c)
    n = torch.arange(i["B"] * i["n0"])
    return (n // g.a_n0) * g.a_s1 + (n % g.a_n0) * (i["Cin"] * i["Hin"] * i["Win"]) + (g.a_off if off is None else off)


def make_inputs(c):
    """Operands of a case on the CPU.  Logical: `A` (M, K) or `x` (n_img, Cin, Hin, Win), `w` in its source layout, `bias`, `gamma`, `beta`,
    `res` (M, N), film tables.  Flat buffers as the descriptor addresses them: `a_buf`, `res_buf` (with the leading elements of a
    misaligned pointer included: the pointer is buf[lead:])."""
    gen = torch.Generator().manual_seed(c.seed)
    inp = types.SimpleNamespace()
    adt = torch.bfloat16 if c.a_dtype == "bf16" else torch.float32
    lay, wshape, _, _ = w_layout(c)
    fan = c.K
    inp.w = torch.randn(wshape, generator=gen) / math.sqrt(fan)
    nb = c.dec["Cout"] if c.dec is not None else c.N
    inp.bias = torch.randn(nb, generator=gen)
    inp.gamma = inp.beta = None
    if c.ln:
        s, o = (0.2, 0.2) if c.affine == "mild" else (3.0, 5.0)
        inp.gamma = (1.0 if c.affine == "mild" else -4.0) + s * torch.randn(c.K, generator=gen)
        inp.beta = (0.0 if c.affine == "mild" else 2.0) + o * torch.randn(c.K, generator=gen)
    if c.img is None:
        A = torch.randn(c.M, c.K, generator=gen) * 1.5 + 0.3
        if c.rows == "mean1e3":
            A = torch.randn(c.M, c.K, generator=gen) + 1e3
        elif c.rows == "const":                   # every third row constant (2.5 sums exactly), the others random
            A[::3] = 2.5
        A = A.to(adt)
        inp.A = A
        starts = row_starts(c)
        size = int(starts.max()) + c.K + 8
        buf = torch.full((c.a_lead + size,), float("nan"), dtype=adt)
        idx = c.a_lead + starts[:, None] + torch.arange(c.K)[None, :]
        buf[idx.reshape(-1)] = A.reshape(-1)
        inp.a_buf = buf
    else:
        i = c.img
        n_img, chw = i["B"] * i["n0"], i["Cin"] * i["Hin"] * i["Win"]
        g = fields(c)
        size = (i["B"] - 1) * g.a_s1 + i["Ttot"] * chw + 8
        buf = torch.full((c.a_lead + size,), float("nan"), dtype=adt)
        for b in range(i["B"]):                  # every frame of the long buffer holds data: a wrong window reads finite, wrong values
            buf[c.a_lead + b * g.a_s1: c.a_lead + b * g.a_s1 + i["Ttot"] * chw] = torch.randn(i["Ttot"] * chw, generator=gen).to(adt)
        x = torch.randn(n_img, i["Cin"], i["Hin"], i["Win"], generator=gen).to(adt)
        inp.x = x
        st = image_starts(c)
        img = x if c.a_mode == "nchw" else x.permute(0, 2, 3, 1)
        idx = c.a_lead + st[:, None] + torch.arange(chw)[None, :]
        buf[idx.reshape(-1)] = img.reshape(-1)
        inp.a_buf = buf
    inp.res = inp.res_buf = None
    if c.res:
        inp.res = torch.randn(c.M, c.N, generator=gen)
        rb = torch.full((c.res_lead + (c.M + 1) * c.res_ld + 8,), float("nan"))
        idx = c.res_lead + torch.arange(c.M)[:, None] * c.res_ld + torch.arange(c.N)[None, :]
        rb[idx.reshape(-1)] = inp.res.reshape(-1)
        inp.res_buf = rb
    inp.film_a = inp.film_b = inp.s_emb = None
    if c.film:
        _, T, HW = c.film
        inp.film_a = 1.0 + torch.randn(T, c.N, generator=gen)
        inp.film_b = torch.randn(T, c.N, generator=gen)
        inp.s_emb = torch.randn(HW, c.N, generator=gen)
    return inp


# ---- references --------------------------------------------------------------------------------------------------------------------
def gelu_erf64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


ACT_FN = {"none": lambda x: x, "relu": torch.relu, "gelu_erf": gelu_erf64, "gelu_tanh": gelu_tanh64}


def layer_norm64(x, gamma, beta, eps):
    """nn.LayerNorm over the last dim: biased variance."""
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    return xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps) * gamma + beta


def patch_rows(x, P, nchw):
    """(n_img, Cin, H, W) -> (n_img * H/P * W/P, Cin * P * P): rows (img, ho, wo); k = (ci, kh, kw) [nchw] or (kh, kw, ci) [channels last]."""
    n, C_, H, W = x.shape
    u = x.unfold(2, P, P).unfold(3, P, P)                 # (n, C, Ho, Wo, kh, kw)
    u = u.permute(0, 2, 3, 1, 4, 5) if nchw else u.permute(0, 2, 3, 4, 5, 1)
    return u.reshape(n * (H // P) * (W // P), C_ * P * P)


def weight_nk(c, w, k_nchw=None):
    """The source-layout weight as the (N, K) matrix of the product, rows / columns in the descriptor's n / k order."""
    if c.dec is not None:                                  # ConvTranspose2d (Cin, Cout, P, P)
        return (w.permute(1, 2, 3, 0) if c.e_mode == "dnchw" else w.permute(2, 3, 1, 0)).reshape(c.N, c.K)
    if c.a_mode == "nhwc":
        return w.permute(0, 2, 3, 1).reshape(c.N, c.K)
    return w.reshape(c.N, c.K)


def bias_n(c, b):
    if c.dec is None:
        return b
    pp = c.dec["Po"] ** 2
    return b.repeat_interleave(pp) if c.e_mode == "dnchw" else b.repeat(pp)


def gather_by_header(c, a_buf, **over):
    """The rows as the header's addressing formulas find them in the flat buffer (NaN where an index leaves it).  `over` overrides
    descriptor fields: how the wrong gathers of the near-miss test are made.  k_order: "nchw" / "nhwc" decode of k in a patch mode."""
    buf = a_buf[c.a_lead:].double()
    k = torch.arange(c.K)
    if c.img is None:
        idx = row_starts(c, **over)[:, None] + k[None, :]
    else:
        i = c.img
        P, Cin, Win, Hin = i["P"], i["Cin"], i["Win"], i["Hin"]
        Ho, Wo = Hin // P, Win // P
        r = torch.arange(c.M)
        im, rem = r // (Ho * Wo), r % (Ho * Wo)
        ho, wo = rem // Wo, rem % Wo
        st = image_starts(c, off=over.get("off"))[im]
        order = over.get("k_order", c.a_mode)
        if order == "nchw":
            ci, kh, kw = k // (P * P), (k % (P * P)) // P, k % P
        else:
            kh, kw, ci = k // (P * Cin), (k // Cin) % P, k % Cin
        hh, ww = ho[:, None] * P + kh[None, :], wo[:, None] * P + kw[None, :]
        if c.a_mode == "nchw":
            idx = st[:, None] + (ci[None, :] * Hin + hh) * Win + ww
        else:
            idx = st[:, None] + (hh * Win + ww) * Cin + ci[None, :]
    ok = (idx >= 0) & (idx < buf.numel())
    out = buf[idx.clamp(0, buf.numel() - 1)]
    out[~ok] = float("nan")
    return out


def reference(c, inp, exact_bf16=False, bug=None):
    """The expected output, float64, in the output's logical shape: (M, N) [lin / film], (n_img, Hi Po, Wi Po, Cout) [dnhwc],
    (n_img, Cout, Hi Po, Wi Po) [dnchw].  exact_bf16: both operands of every product rounded to bf16 as the kernel rounds them
    (W gamma formed in fp32 and then rounded; the row normalised in fp32 and then rounded), float64 accumulation.
    bug: one of WRONG -- the same expression with that mistake in it."""
    bf = exact_bf16 and c.mode == "bf16"
    if c.img is None:
        A = inp.A.double()
    else:
        A = patch_rows(inp.x.double(), c.img["P"], c.a_mode == "nchw")
    if bug == "dense_rows":
        A = gather_by_header(c, inp.a_buf, n0=c.M, s1=0, s0=c.K)
    elif bug == "no_a_off":
        A = gather_by_header(c, inp.a_buf, off=0)
    elif bug == "window_early":
        A = gather_by_header(c, inp.a_buf, off=fields(c).a_off - (c.img["Cin"] * c.img["Hin"] * c.img["Win"] if c.img else c.a_s0))
    elif bug == "nchw_k_for_nhwc":
        A = gather_by_header(c, inp.a_buf, k_order="nchw")
    W = weight_nk(c, inp.w)
    b = bias_n(c, inp.bias).double()
    if c.ln:
        if bf:
            x32 = A.float()
            mu = x32.mean(-1, keepdim=True)
            xc = x32 - mu
            An = _bf(xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + c.ln_eps)).double()
            Wn = _bf(W * inp.gamma[None, :]).double()
        else:
            mu = A.mean(-1, keepdim=True)
            xc = A - mu
            q = (xc * xc).sum(-1, keepdim=True)
            if bug == "ln_var_padding":           # the zero padding of the last chunk counted as K_pad - K more elements
                q = q + (pack_geom(c.N, c.K, c.compute).k_pad - c.K) * mu * mu
            if bug == "ln_unbiased":
                q = q * c.K / (c.K - 1)
            An = xc * torch.rsqrt(q / c.K + c.ln_eps)
            Wn = W.double() * inp.gamma.double()[None, :]
        b = b + W.double() @ inp.beta.double()
        Y = An @ Wn.t()
    else:
        Y = (_bf(A.float()).double() if bf else A) @ (_bf(W).double() if bf else W.double()).t()
    if bug == "no_bias_last_tile" and c.N % 16:
        b = b.clone()
        b[c.N // 16 * 16:] = 0.0
    Y = Y + b
    act = ACT_FN["gelu_tanh" if bug == "tanh_for_erf" and c.act == "gelu_erf" else c.act]
    if c.e_mode == "lin":
        res = None if inp.res is None else inp.res.double()
        if bug == "res_ld_for_out_ld" and res is not None:
            rb = inp.res_buf[c.res_lead:].double()
            idx = torch.arange(c.M)[:, None] * c.out_ld + torch.arange(c.N)[None, :]
            res = rb[idx.clamp(max=rb.numel() - 1)]
            res[idx >= rb.numel()] = float("nan")
        if bug == "res_before_act" and res is not None:
            return act(Y + res)
        Y = act(Y)
        return Y if res is None else Y + res
    Y = act(Y)
    if c.e_mode == "film":
        _, T, HW = c.film
        r = torch.arange(c.M)
        t, hw = (r // HW) % T, r % HW
        fa, fb, se = inp.film_a.double(), inp.film_b.double(), inp.s_emb.double()
        if bug == "t_no_mod":
            t = r // HW
            pad = torch.full((int(t.max()) + 1 - T, c.N), float("nan"), dtype=torch.float64)
            fa, fb = torch.cat([fa, pad]), torch.cat([fb, pad])
        elif bug == "t_hw_swapped":               # rows taken for (b, hw, t)
            t, hw = r % T, (r // T) % HW
        elif bug == "film_t_plus_1":
            t = (t + 1) % T
        return Y * fa[t] + fb[t] + se[hw]
    d = c.dec
    n_img, Hi, Wi, Po, Co = c.M // (d["Hi"] * d["Wi"]), d["Hi"], d["Wi"], d["Po"], d["Cout"]
    if c.e_mode == "dnhwc":
        Y6 = Y.view(n_img, Hi, Wi, Co, Po, Po).permute(0, 1, 2, 4, 5, 3) if bug == "co_khkw_order" else Y.view(n_img, Hi, Wi, Po, Po, Co)
        if bug == "shuffle_khkw_swapped":
            Y6 = Y6.transpose(3, 4)
        return Y6.permute(0, 1, 3, 2, 4, 5).reshape(n_img, Hi * Po, Wi * Po, Co)      # (img, hi, kh, wi, kw, co)
    Y6 = Y.view(n_img, Hi, Wi, Co, Po, Po)
    if bug == "shuffle_khkw_swapped":
        Y6 = Y6.transpose(4, 5)
    return Y6.permute(0, 3, 1, 4, 2, 5).reshape(n_img, Co, Hi * Po, Wi * Po)          # (img, co, hi, kh, wi, kw)


def errors(got, ref):
    """(relative L2, max-norm) of got against ref; infinite when got is not finite."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    return float((got - ref).norm() / (ref.norm() + 1e-300)), float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


# wrong results these kernels can produce -> which cases exercise them
WRONG = {
    "dense_rows": lambda c: c.img is None and (c.a_s0 != c.K or c.a_n0 != c.M),
    "no_a_off": lambda c: fields(c).a_off != 0,
    "window_early": lambda c: c.img is not None,
    "t_no_mod": lambda c: c.e_mode == "film" and c.film[0] > 1,
    "t_hw_swapped": lambda c: c.e_mode == "film",
    "film_t_plus_1": lambda c: c.e_mode == "film",
    "res_before_act": lambda c: c.res is not None and c.act != "none",
    "no_bias_last_tile": lambda c: c.N % 16 != 0 and c.e_mode == "lin",
    "ln_var_padding": lambda c: c.ln and c.K != pack_geom(c.N, c.K, c.compute).k_pad,
    "shuffle_khkw_swapped": lambda c: c.dec is not None and c.dec["Po"] > 1,
    "co_khkw_order": lambda c: c.e_mode == "dnhwc" and c.dec["Po"] > 1 and c.dec["Cout"] > 1,
    "nchw_k_for_nhwc": lambda c: c.a_mode == "nhwc",
    "res_ld_for_out_ld": lambda c: c.res == "other" and c.res_ld != c.out_ld,
}
# what a format cannot see (stated, and asserted as such by the CPU test): an unbiased variance moves the result by 1 / (2 K) -- beyond
# twice the fp32 bar at every K <= 512, beyond twice the bf16 bar only for K < 25; tanh-GELU for erf-GELU differs by about 1e-4 of the
# output's scale: beyond the fp32 bar, an order of magnitude inside the bf16 one.
BLIND = {"ln_unbiased": lambda c: c.ln and c.rows == "randn", "tanh_for_erf": lambda c: c.act == "gelu_erf" and c.e_mode == "lin"}


def _win(K, pad=8, extra=16, off=24):
    """The window of group (b): rows[r] = (r // 5) * s1 + (r % 5) * s0 + off with s0 > K, s1 != 5 s0, off != 0."""
    return dict(a_n0=5, a_s0=K + pad, a_s1=5 * (K + pad) + extra, a_off=off)


def _img(Cin, P, Hin, Win, B=2, n0=2, gap=4):
    return dict(B=B, n0=n0, Ttot=n0 + 2, Hin=Hin, Win=Win, Cin=Cin, P=P, gap=gap)


def build_cases():
    cs = []

    def add(group, name, **kw):
        cs.append(Case(group, name, **kw))
    MS, NS = (1, 17, 65, 130), (1, 20, 64, 100, 132, 768)
    # (a) every dedicated linear line; LN + none and no-LN + none at every CB.  (The patch / deconv / FiLM lines: groups e and f.)
    for mode in ("bf16", "fp32"):
        ks = K_OF_CB[mode]
        for j, (cb, K) in enumerate(ks.items()):
            big = mode == "bf16" and K == 512          # bf16 K = 512 at M <= 1024 is the small kernel's: 1025 rows reach gemm_kernel
            add("a", f"ln-none-K{K}", mode=mode, M=1025 if big else MS[1 + j % 3], N=NS[2 + j % 4], K=K, ln=True, out_ld=NS[2 + j % 4])
            add("a", f"none-K{K}", mode=mode, M=1025 if big else MS[1 + (j + 1) % 3], N=NS[2 + (j + 1) % 4], K=K, res="out" if j % 2 else None)
        k2, k4, k8 = ks[2], ks[4], ks[8]
        add("a", "ln-gelu_tanh", mode=mode, M=65, N=132, K=k4, ln=True, act="gelu_tanh")
        add("a", "ln-gelu_erf", mode=mode, M=130, N=64, K=k8, ln=True, act="gelu_erf")
        add("a", "relu", mode=mode, M=17, N=100, K=k2, act="relu")
        add("a", "gelu_erf-res", mode=mode, M=65, N=768, K=k4, act="gelu_erf", res="out", out_ld=768)
        add("a", "gelu_tanh", mode=mode, M=130, N=20, K=k8, act="gelu_tanh")
        add("a", "generic-ln-K100-N100", mode=mode, M=65, N=100, K=100, ln=True, act="gelu_erf")
        add("a", "generic-K44-N1", mode=mode, M=130, N=1, K=44, act="relu")
        add("a", "generic-ln-relu", mode=mode, M=17, N=64, K=k2, ln=True, act="relu", note="LN + relu has no dedicated line")
    # (b) linear addressing: a window of a NaN-padded buffer
    for mode in ("bf16", "fp32"):
        ks = K_OF_CB[mode]
        add("b", "win-none", mode=mode, M=17, N=64, K=ks[2], **_win(ks[2]))
        add("b", "win-ln-gelu_tanh", mode=mode, M=130, N=100, K=ks[4], ln=True, act="gelu_tanh", **_win(ks[4]))
        add("b", "win-ln-none-res", mode=mode, M=65, N=132, K=ks[8], ln=True, res="other", **_win(ks[8]))
        # the heads' last-slot read of the token stream (B, T, HW, C): rows (b, hw) of slot T - 1
        T, HW, C_ = 3, 65, ks[4]
        last = dict(a_n0=HW, a_s1=T * HW * C_, a_s0=C_, a_off=(T - 1) * HW * C_)
        add("b", "lastslot-dnhwc-gelu", mode=mode, K=C_, act="gelu_erf", e_mode="dnhwc", dec=dict(n_img=2, Hi=5, Wi=13, Po=2, Cout=8), **last)
        add("b", "lastslot-dnchw-none", mode=mode, K=C_, e_mode="dnchw", dec=dict(n_img=2, Hi=5, Wi=13, Po=2, Cout=3), **last)
    add("b", "win-small", mode="bf16", M=65, N=64, K=512, ln=True, **_win(512))
    add("b", "win-small-res", mode="bf16", M=130, N=100, K=512, act="gelu_erf", res="other", **_win(512))
    add("b", "win-lite", mode="bf16", a_dtype="bf16", M=4096, N=64, K=256, act="relu", **_win(256))
    # (e) epilogues
    for mode in ("bf16", "fp32"):
        for N in (64, 66):
            add("e", f"film-nhwc-N{N}", mode=mode, N=N, a_mode="nhwc", e_mode="film", film=(2, 3, 5), img=_img(16, 2, 2, 10, B=2, n0=3))
            add("e", f"film-lin-N{N}", mode=mode, N=N, K=K_OF_CB[mode][4], e_mode="film", film=(2, 3, 5))
        for Po in (2, 4):
            for act in ("gelu_erf", "none"):
                for Co in (4, 5):
                    add("e", f"dnhwc-Po{Po}-{act}-Co{Co}", mode=mode, K=K_OF_CB[mode][2], act=act, e_mode="dnhwc",
                        dec=dict(n_img=2, Hi=5, Wi=13, Po=Po, Cout=Co))
        for Po in (1, 2, 4):
            for act in ("none", "gelu_erf"):
                add("e", f"dnchw-Po{Po}-{act}", mode=mode, K=K_OF_CB[mode][4], act=act, e_mode="dnchw", dec=dict(n_img=1, Hi=5, Wi=13, Po=Po, Cout=3))
    # (f) patch gathers, each from a window of a longer (B, T_total, ...) buffer, one frame in
    for mode in ("bf16", "fp32"):
        add("f", "nhwc-Cin8-gelu", mode=mode, N=64, a_mode="nhwc", act="gelu_erf", img=_img(8, 2, 4, 6))
        add("f", "nhwc-Cin16-none", mode=mode, N=100, a_mode="nhwc", img=_img(16, 2, 4, 6))
        add("f", "nhwc-Cin6-gelu", mode=mode, N=20, a_mode="nhwc", act="gelu_erf", img=_img(6, 2, 4, 6))
        add("f", "nchw-P2-gelu", mode=mode, N=64, a_mode="nchw", act="gelu_erf", img=_img(16, 2, 4, 10))
        add("f", "nchw-P2-none-Cin11", mode=mode, N=132, a_mode="nchw", img=_img(11, 2, 4, 10))
        add("f", "nchw-P1-oddW", mode=mode, N=64, a_mode="nchw", act="gelu_erf", img=_img(16, 1, 4, 5))
        add("f", "nchw-P4", mode=mode, N=64, a_mode="nchw", act="gelu_erf", img=_img(4, 4, 8, 8))
        add("f", "nchw-P2-bf16img", mode=mode, a_dtype="bf16", N=64, a_mode="nchw", act="gelu_erf", img=_img(16, 2, 4, 10))
        add("f", "nchw-P2-4B-off", mode=mode, N=64, a_mode="nchw", act="gelu_erf", a_lead=1, img=_img(16, 2, 4, 10))
    # (g) mixed dtypes
    add("g", "bf16a-fp32compute", mode="fp32", a_dtype="bf16", M=65, N=64, K=64, act="gelu_erf")
    add("g", "bf16a-fp32compute-K44", mode="fp32", a_dtype="bf16", M=17, N=100, K=44)
    add("g", "f32a-bf16compute-K100", mode="bf16", M=65, N=64, K=100)
    for mode in ("bf16", "fp32"):
        add("g", "bf16out-N20", mode=mode, out_dtype="bf16", M=130, N=20, K=K_OF_CB[mode][2], act="gelu_tanh")
        add("g", "bf16out-N1", mode=mode, out_dtype="bf16", M=17, N=1, K=K_OF_CB[mode][4])
        add("g", "bf16out-N64", mode=mode, out_dtype="bf16", M=65, N=64, K=K_OF_CB[mode][4], act="relu")
    # (h) LayerNorm
    add("h", "K44-tail", mode="fp32", M=65, N=64, K=44, ln=True)
    add("h", "K100-tail", mode="bf16", M=65, N=64, K=100, ln=True)
    add("h", "K100-tail", mode="fp32", M=17, N=100, K=100, ln=True, act="gelu_erf")
    add("h", "K512", mode="fp32", M=130, N=64, K=512, ln=True, act="gelu_erf")
    add("h", "K512-res", mode="fp32", M=65, N=132, K=512, ln=True, res="other")
    for mode in ("bf16", "fp32"):
        K = K_OF_CB[mode][4]
        add("h", "const-rows", mode=mode, M=65, N=64, K=K, ln=True, rows="const")
        add("h", "const-rows-K44", mode=mode, M=17, N=20, K=44, ln=True, rows="const")
        add("h", "mean1e3", mode=mode, M=65, N=64, K=K, ln=True, rows="mean1e3")
        add("h", "mean1e3-K100", mode=mode, M=17, N=64, K=100, ln=True, rows="mean1e3", note="a K tail under a large mean: padding counted in the variance shows")
        add("h", "eps1e-2", mode=mode, M=65, N=64, K=K, ln=True, ln_eps=1e-2)
        add("h", "eps1e-2-K44", mode=mode, M=17, N=100, K=44, ln=True, ln_eps=1e-2, act="gelu_tanh")
        add("h", "far-affine", mode=mode, M=65, N=64, K=K, ln=True, affine="far")
    # (i) the small kernel: what test_small_row_gemm_against_float64 lacks
    add("i", "M1", mode="bf16", M=1, N=64, K=512, ln=True)
    add("i", "M1024", mode="bf16", M=1024, N=64, K=512)
    add("i", "M1025", mode="bf16", M=1025, N=64, K=512, note="one row past TANTE_GEMM_SMALLM: gemm_kernel")
    add("i", "N36", mode="bf16", M=17, N=36, K=512, ln=True, act="gelu_erf")
    add("i", "res-other", mode="bf16", M=65, N=64, K=512, act="gelu_erf", res="other")
    add("i", "relu", mode="bf16", M=17, N=64, K=512, act="relu", note="no small form: gemm_kernel")
    add("i", "ln-gelu_tanh", mode="bf16", M=17, N=64, K=512, ln=True, act="gelu_tanh", note="no small form: gemm_kernel")
    # (j) the lite kernel: what test_gemm_training_shapes lacks, and the channels-first 2 x 2 pixel shuffle's four forms
    add("j", "M4096", mode="bf16", a_dtype="bf16", M=4096, N=64, K=256, out_ld=64)
    add("j", "M4097", mode="bf16", a_dtype="bf16", M=4097, N=100, K=256, act="gelu_erf")
    add("j", "M4095", mode="bf16", a_dtype="bf16", M=4095, N=64, K=256, note="one row short: gemm_kernel")
    add("j", "K128-res", mode="bf16", a_dtype="bf16", M=4096, N=132, K=128, act="gelu_tanh", res="other")
    add("j", "K512", mode="bf16", a_dtype="bf16", M=4097, N=64, K=512)
    for adt in ("bf16", "f32"):
        for act in ("none", "gelu_erf"):
            add("j", f"dnchw2-{adt}-{act}", mode="bf16", a_dtype=adt, K=128, act=act, e_mode="dnchw", dec=dict(n_img=1, Hi=64, Wi=64, Po=2, Cout=3))
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CASES = build_cases()
