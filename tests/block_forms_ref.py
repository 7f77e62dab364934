"""The inference block kernels alone (tante_amd/csrc/block_sliced.hip, block_fused.hip: tante_block_fused, tante_block_fused_tprop,
tante_block_fused_last): cases, the float64 reference on the flat (tokens, C) buffer a launch gets, its exact-bf16 evaluation, per-token
error figures, planted faults and the restated launch dispatch.  Nothing here touches the GPU or tante_amd: tests/test_block_forms_cpu.py
pins this file to the oracle, to the text of the two sources and to wrong results; tests/test_hip_block_forms.py runs the kernels against it.

The operation, per sequence of L tokens (TanteSeq says which rows of the buffer they are):
    [tprop, L = 4:  x_t += b2[t] + sum_j w2[t][j] gelu_erf(b1[j] + sum_a w1[j][a] x_a)   per channel]
    x += Wo Attention(LayerNorm1(x)) + bo ;   x += W2 gelu_tanh(W1 LayerNorm2(x) + b1) + b2
in place; a `last` launch writes the rows at slot L - 1 only and leaves slots 0 .. L - 2 as they were (not even propagated).
The exact-bf16 evaluation rounds to bf16 exactly where the feature-sliced kernel does (fs_pack_body: W gamma [log2(e) / sqrt(32) for q]
rounded once, the betas / the value bias folded into fp32 biases, no key bias; block_fs_kernel: the LayerNorm images without affine,
q, k, v, the un-normalised exp2 probabilities, the per-head outputs after the division by the fp32 sum, the GELU-ed hidden layer) and keeps
everything else in float64: its distance to float64 is the format's share of a kernel's error."""
import math
import zlib
from collections import namedtuple
from typing import Dict, Optional

import torch

# ---- bars -----------------------------------------------------------------------------------------------------------------------------
# The project's bf16 bars over the whole tensor: relative L2 and scale-relative max on y, relative L2 on the block's contribution y - x.
BAR_L2, BAR_MAX, BAR_DELTA = 1e-2, 2e-2, 2e-2
# Per token, on y - x:  || (y - x)_got - (y - x)_ref || / || (y - x)_ref ||.  Twice the worst per-token error of the exact-bf16 evaluation
# against float64 over all of BLOCK_CASES, rounded up to one significant digit; measured on the CPU from this file alone (never from a
# kernel): EXACT_BF16_WORST_TOKEN below, pinned by test_block_forms_cpu.py::test_exact_bf16_headroom_and_bar_rule.
EXACT_BF16_WORST_TOKEN = 5.5e-3      # case ts16-C64h128-L1x129c; the feature-sliced cases stay below 4.9e-3
BAR_TOKEN = 2e-2


def bar_token_rule(worst_exact_bf16: float) -> float:
    """2 x the figure, rounded up to one significant digit."""
    v = 2.0 * worst_exact_bf16
    e = math.floor(math.log10(v))
    return math.ceil(v / 10.0 ** e - 1e-9) * 10.0 ** e


def bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even), back in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


# ---- TanteSeq: which rows a launch addresses -------------------------------------------------------------------------------------------
Seq = namedtuple("Seq", "nseq L n_s0 S1 S0 n_l0 P1 P0")


def dense_seq(nseq: int, L: int) -> Seq:
    return Seq(nseq, L, 1, L, 0, L, 0, 1)


def make_seq(letter: str, B: int, T: int, H: int, W: int) -> Seq:
    """kernels.make_seq restated (test_hip_block_forms.py compares the fields)."""
    HW, THW = H * W, T * H * W
    return {"T": Seq(B * HW, T, HW, THW, 1, T, 0, HW), "H": Seq(B * T * W, H, W, HW, 1, H, 0, W), "W": Seq(B * T * H, W, 1, W, 0, W, 0, 1),
            "L": Seq(B * T, HW, 1, HW, 0, HW, 0, 1), "Y": Seq(B * W, T * H, W, THW, 1, H, HW, W), "X": Seq(B * H, T * W, H, THW, W, W, HW, 1),
            "A": Seq(B, THW, 1, THW, 0, THW, 0, 1)}[letter]


def last_slot_seq(letter: str, B: int, T: int, H: int, W: int) -> Seq:
    """kernels.last_slot_seq restated: an H / W / L letter on the (b, T - 1) planes, token indices from row (T - 1) H W."""
    HW, THW = H * W, T * H * W
    return {"H": Seq(B * W, H, W, THW, 1, H, 0, W), "W": Seq(B * H, W, H, THW, W, W, 0, 1), "L": Seq(B, HW, 1, THW, 0, HW, 0, 1)}[letter]


def seq_tokens(q: Seq, row0: int = 0) -> torch.Tensor:
    """(nseq, L) rows of the buffer:  row0 + (s / n_s0) S1 + (s % n_s0) S0 + (l / n_l0) P1 + (l % n_l0) P0."""
    s, l = torch.arange(q.nseq)[:, None], torch.arange(q.L)[None, :]
    return row0 + (s // q.n_s0) * q.S1 + (s % q.n_s0) * q.S0 + (l // q.n_l0) * q.P1 + (l % q.n_l0) * q.P0


# ---- the block on (nseq, L, C) -----------------------------------------------------------------------------------------------------------
QSCALE = 0.17677669529663687 * 1.44269504088896340736      # log2(e) / sqrt(32): the kernels' softmax is exp2 of the scores


def tprop_ref(X: torch.Tensor, tp) -> torch.Tensor:
    """The temporal propagator on (nseq, 4, C): tp = (w1 (4, 4), b1, w2 (4, 4), b2); oracle._axis_mlp along T, residual."""
    w1, b1, w2, b2 = [t.double() for t in tp]
    xt = X.transpose(1, 2)                                        # (nseq, C, T)
    h = gelu_erf(xt @ w1.t() + b1)
    return X + (h @ w2.t() + b2).transpose(1, 2)


def block_ref(w: Dict[str, torch.Tensor], X: torch.Tensor, causal: bool, exact_bf16: bool = False, bug=None, eps: float = 1e-5) -> torch.Tensor:
    """One TransformerBlock on X (nseq, L, C) in float64; w under the oracle's names.  bug (a planted fault, one sequence or token):
    ("drop_last_key", s)  ("causal_off_by_one", s)  ("drop_head", s, l, h)  ("ln_c_minus_1", s, l)."""
    X = X.double()
    nseq, L, C = X.shape
    d, nh = 32, C // 32
    g = {k: v.double() for k, v in w.items()}
    kind = bug[0] if bug else None

    def norm(v, which):
        mu = v.mean(-1, keepdim=True)
        var = ((v - mu) ** 2).mean(-1, keepdim=True)
        if which == 1 and kind == "ln_c_minus_1":
            row = v[bug[1], bug[2], :C - 1]
            mu[bug[1], bug[2]] = row.mean()
            var[bug[1], bug[2]] = ((row - row.mean()) ** 2).mean()
        return (v - mu) * torch.rsqrt(var + eps)

    w_in, b_in = g["attn.in_proj_weight"], g["attn.in_proj_bias"]
    if exact_bf16:
        def fold(wm, gamma, scale=1.0):      # fs_pack_body: (w gamma) scale in fp32, rounded to bf16 once
            v = wm.float() * gamma.float()[None, :] if gamma is not None else wm.float()
            return (v * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16).double()
        g1, be1, g2, be2 = g["ln1.weight"], g["ln1.bias"], g["ln2.weight"], g["ln2.bias"]
        xh = bf16(norm(X, 1))
        q = bf16(xh @ fold(w_in[:C], g1, QSCALE).t() + (b_in[:C] + w_in[:C] @ be1) * QSCALE)
        k = bf16(xh @ fold(w_in[C:2 * C], g1).t())                                           # the key bias cancels in the softmax
        v = bf16(xh @ fold(w_in[2 * C:], g1).t())                                            # the value bias rides the out-proj bias
        bo = g["attn.out_proj.bias"] + g["attn.out_proj.weight"] @ (b_in[2 * C:] + w_in[2 * C:] @ be1)
        wo, rd = fold(g["attn.out_proj.weight"], None), bf16
        w1, b1 = fold(g["mlp.0.weight"], g2), g["mlp.0.bias"] + g["mlp.0.weight"] @ be2
        w2 = fold(g["mlp.2.weight"], None)
    else:
        xh = norm(X, 1) * g["ln1.weight"] + g["ln1.bias"]
        qkv = xh @ w_in.t() + b_in
        q, k, v = qkv[..., :C] * (1.0 / math.sqrt(d)), qkv[..., C:2 * C], qkv[..., 2 * C:]
        bo, wo, rd = g["attn.out_proj.bias"], g["attn.out_proj.weight"], (lambda t: t)
        w1, b1, w2 = g["mlp.0.weight"], g["mlp.0.bias"], g["mlp.2.weight"]
    q, k, v = (t.reshape(nseq, L, nh, d).transpose(1, 2) for t in (q, k, v))                # (nseq, nh, L, d)
    sc = q @ k.transpose(-1, -2)
    allow = torch.ones(nseq, 1, L, L, dtype=torch.bool)
    if causal:
        allow &= torch.tril(torch.ones(L, L, dtype=torch.bool))
        if kind == "causal_off_by_one":
            allow[bug[1]] = torch.tril(torch.ones(L, L, dtype=torch.bool), diagonal=1)
    if kind == "drop_last_key":
        allow[bug[1], :, :, L - 1] = False
        allow[bug[1], :, L - 1, L - 1] = L == 1        # (a one-token sequence keeps its only key)
    sc = sc.masked_fill(~allow, float("-inf"))
    e = sc - sc.amax(-1, keepdim=True)
    p = (torch.exp2(e) if exact_bf16 else torch.exp(e)).masked_fill(~allow, 0.0)
    o = rd((rd(p) @ v) / p.sum(-1, keepdim=True))
    if kind == "drop_head":
        o[bug[1], bug[3], bug[2]] = 0.0
    o = o.transpose(1, 2).reshape(nseq, L, C)
    x1 = X + o @ wo.t() + bo
    xh2 = norm(x1, 2)
    xh2 = rd(xh2) if exact_bf16 else xh2 * g["ln2.weight"] + g["ln2.bias"]
    return x1 + rd(gelu_tanh(xh2 @ w1.t() + b1)) @ w2.t() + g["mlp.2.bias"]


# ---- restated dispatch ----------------------------------------------------------------------------------------------------------------
FS_C, FS_MAX_L, FS_MAX_NSEQ = 256, 128, 1 << 23
CUS, TILE = 256, 16                                         # tante_fs_launch: resident = 256L * (8 / nw); 16-token tiles
SKEW_WINDOW = (257, 512)                                    # nwg > 256 && nwg <= 512
OPTION_DEFAULTS = {"TANTE_BLOCK_KERNEL": 0, "TANTE_FS_WAVES": 0, "TANTE_FS_HALF": 1, "TANTE_FS_GROUPS": 0, "TANTE_FS_SKEW": 0}
FS_KEYS = (412, 422, 413, 414, 424, 433, 444, 404, 818, 816, 828, 826, 836, 848, 808)
TS_INSTANCES = ((2, 2), (2, 4), (4, 4), (4, 8), (8, 8))    # (CB, HB) = (C / 32, hidden / 32)

FsRoute = namedtuple("FsRoute", "name key spw nwg skew")
TsRoute = namedtuple("TsRoute", "name per_wg nwg")


class Refused(Exception):
    pass


def _opt(options, name):
    return (options or {}).get(name, OPTION_DEFAULTS[name])


def fs_supported(C: int, n_head: int, hidden: int, L: int) -> bool:
    return C == FS_C and n_head == 8 and hidden == FS_C and 1 <= L <= FS_MAX_L


def ts_supported(C: int, n_head: int, hidden: int, L: int) -> bool:
    """block_ts_supported: the round-1 kernels."""
    if n_head <= 0 or C % n_head or C // n_head != 32 or C not in (64, 128, 256):
        return False
    if hidden not in (C, 2 * C) or (hidden > 256 and C == 256):
        return False
    return 0 < L <= 32 and 32 % L == 0


def use_fs(C: int, n_head: int, hidden: int, L: int, options=None) -> bool:
    if not fs_supported(C, n_head, hidden, L):
        return False
    return _opt(options, "TANTE_BLOCK_KERNEL") == 0 or not ts_supported(C, n_head, hidden, L)


def fs_route(L: int, nseq: int, causal: bool, tprop: bool = False, last: bool = False, options=None) -> FsRoute:
    """tante_fs_launch (inference) restated."""
    if nseq >= FS_MAX_NSEQ or ((tprop or last) and L != 4):
        raise Refused(f"L={L} nseq={nseq} tprop={tprop} last={last}")
    nw = 4 if (tprop or last) else (8 if (_opt(options, "TANTE_FS_WAVES") == 8 or L > 64) else 4)
    tps = 1 if TILE % L == 0 else (L // TILE if (not causal and L in (32, 48, 64)) else 0)
    full, tq = (8, 6) if nw == 8 else (4, 3)
    resident = CUS * (8 // nw)

    def rounds(ntt):
        spw = TILE * ntt // L
        nwg = (nseq + spw - 1) // spw
        return ((nwg + resident - 1) // resident) * ntt
    ntt = full
    if tps == 3:
        ntt = tq
    elif tps >= 1 and (TILE * tq) % L == 0 and (TILE * tq) // L >= 1 and (tps == 1 or tq % tps == 0) and rounds(tq) < rounds(full):
        ntt = tq
    if nw == 4 and tps in (1, 2) and 32 % L == 0 and _opt(options, "TANTE_FS_HALF"):
        spw_full = TILE * ntt // L
        if (nseq + spw_full - 1) // spw_full * 4 <= resident:
            ntt = 2
    if last and ntt == tq:
        ntt = full
    spw = TILE * ntt // L if tps else (TILE * full) // L
    nwg = (nseq + spw - 1) // spw
    skew = _opt(options, "TANTE_FS_SKEW") if (nw == 4 and SKEW_WINDOW[0] <= nwg <= SKEW_WINDOW[1]) else 0
    key = nw * 100 + tps * 10 + ntt
    name = f"fs<TPS{tps},NTT{ntt},NW{nw}"
    if last:
        name += (",TPROP" if tprop else "") + ",LASTQ"
    else:
        if key not in FS_KEYS:
            raise Refused(f"no instance for key {key}")
        if tprop:
            name += ",TPROP"
        elif nw == 4 and key not in (412, 422) and _opt(options, "TANTE_FS_GROUPS") == 2:      # fs_launch_t; 412 / 422 launch directly
            name += ",G2"
    return FsRoute(name + ">", key, spw, nwg, skew)


def ts_route(C: int, hidden: int, L: int, nseq: int, option: int = 0) -> TsRoute:
    """launch_block / launch_block16 restated: only option value 32 selects the 256-thread form."""
    if (C // 32, hidden // 32) not in TS_INSTANCES or not ts_supported(C, C // 32, hidden, L):
        raise Refused(f"C={C} hidden={hidden} L={L}")
    if option != 32 and (L == 32 or 16 % L == 0):
        per_wg = 4 if L == 32 else 8 * (16 // L)
        return TsRoute(f"block16<{C // 32},{hidden // 32}>", per_wg, (nseq + per_wg - 1) // per_wg)
    spw = 32 // L
    waves = (nseq + spw - 1) // spw
    return TsRoute(f"block32<{C // 32},{hidden // 32}>", 4 * spw, (waves + 3) // 4)


def route(c, options=None) -> str:
    """The kernel instance a case's launch reaches under `options` (the library's option values)."""
    if (c.tprop or c.last) and not use_fs(c.C, c.C // 32, c.hidden, c.L, options):
        raise Refused("tprop / last need the feature-sliced kernel")
    if use_fs(c.C, c.C // 32, c.hidden, c.L, options):
        return fs_route(c.L, c.nseq, c.causal, c.tprop, c.last, options).name
    return ts_route(c.C, c.hidden, c.L, c.nseq, _opt(options, "TANTE_BLOCK_KERNEL")).name


ALL_FS_ROUTES = ({f"fs<TPS{k // 10 % 10},NTT{k % 10},NW{k // 100}>" for k in FS_KEYS}
                 | {f"fs<TPS1,NTT{n},NW4,TPROP>" for n in (2, 3, 4)}
                 | {f"fs<TPS1,NTT{n},NW4{t},LASTQ>" for n in (2, 4) for t in ("", ",TPROP")}
                 | {f"fs<TPS{k // 10 % 10},NTT{k % 10},NW4,G2>" for k in (413, 414, 424, 433, 444, 404)})
ALL_TS_ROUTES = {f"block{n}<{cb},{hb}>" for n in (16, 32) for cb, hb in TS_INSTANCES}
# instances the launchers name that no shape can reach (none: every one above has a case; test_block_forms_cpu.py holds the union)
UNREACHABLE_ROUTES: Dict[str, str] = {}


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
class BlockCase(namedtuple("BlockCase", "name C hidden L nseq causal tprop last options route layout")):
    """options: ((name, value), ...) set for the launch.  layout: None (dense sequences), (letter, B, T, H, W) (make_seq on a grid) or
    ("sub", letter, B, T, H, W) (last_slot_seq from row (T - 1) H W: block_fused_subgrid).  nseq, L of a layout case are the letter's."""
    __slots__ = ()

    @property
    def id(self):
        return self.name

    @property
    def seed(self):
        return zlib.crc32(self.shape_id.encode()) & 0x7fffffff

    @property
    def shape_id(self):
        """Cases with the same shape_id share inputs, weights and references (the launch form differs, not the function)."""
        return f"C{self.C}h{self.hidden}-L{self.L}x{self.nseq}-{'c' if self.causal else 'n'}{'-tp' if self.tprop else ''}-{self.layout}"

    @property
    def opts(self):
        return dict(self.options)

    def seq(self) -> Seq:
        if self.layout is None:
            return dense_seq(self.nseq, self.L)
        if self.layout[0] == "sub":
            return last_slot_seq(*self.layout[1:])
        return make_seq(*self.layout)

    @property
    def row0(self):
        if self.layout is not None and self.layout[0] == "sub":
            _, _, B, T, H, W = self.layout
            return (T - 1) * H * W
        return 0


def _fs(name, L, nseq, causal, route_, tprop=False, last=False, layout=None, **opt):
    return BlockCase(name, 256, 256, L, nseq, causal, tprop, last, tuple(sorted(opt.items())), route_, layout)


def _letter(name, C, hidden, letter, grid, route_, sub=False, **opt):
    q = last_slot_seq(letter, *grid) if sub else make_seq(letter, *grid)
    lay = ("sub", letter) + grid if sub else (letter,) + grid
    return BlockCase(name, C, hidden, q.L, q.nseq, letter == "T", False, False, tuple(sorted(opt.items())), route_, lay)


W8, H0, G2 = {"TANTE_FS_WAVES": 8}, {"TANTE_FS_HALF": 0}, {"TANTE_FS_GROUPS": 2}
BIG16, BIG32, BIGT = 1537, 769, (1, 4, 77, 80)      # the smallest launches past one resident round of three-quarter workgroups (see the rule)

FS_CASES = [
    # 412: L | 16, half-size workgroups, ragged last workgroup; with the propagator; the last-slot form with and without it
    _fs("412-L4x37c", 4, 37, True, "fs<TPS1,NTT2,NW4>"), _fs("412-L1x70", 1, 70, False, "fs<TPS1,NTT2,NW4>"),
    _fs("412-L16x3", 16, 3, False, "fs<TPS1,NTT2,NW4>"), _fs("412-L2x33c", 2, 33, True, "fs<TPS1,NTT2,NW4>"),
    _fs("412-L8x9c", 8, 9, True, "fs<TPS1,NTT2,NW4>"),
    _fs("412-L4x37c-tprop", 4, 37, True, "fs<TPS1,NTT2,NW4,TPROP>", tprop=True),
    _fs("412-L4x37c-last", 4, 37, True, "fs<TPS1,NTT2,NW4,LASTQ>", last=True),
    _fs("412-L4x37c-tprop-last", 4, 37, True, "fs<TPS1,NTT2,NW4,TPROP,LASTQ>", tprop=True, last=True),
    _fs("422-L32x5", 32, 5, False, "fs<TPS2,NTT2,NW4>"),
    _fs("433-L48x3", 48, 3, False, "fs<TPS3,NTT3,NW4>"),
    _fs("444-L64x3", 64, 3, False, "fs<TPS4,NTT4,NW4>"),
    # 404: element masks -- 12 sequences per workgroup and a ragged second one; lengths that straddle tiles; causal tile-aligned lengths
    _fs("404-L5x13c", 5, 13, True, "fs<TPS0,NTT4,NW4>"), _fs("404-L12x23", 12, 23, False, "fs<TPS0,NTT4,NW4>"),
    _fs("404-L24x1", 24, 1, False, "fs<TPS0,NTT4,NW4>"), _fs("404-L50x3", 50, 3, False, "fs<TPS0,NTT4,NW4>"),
    _fs("404-L32x7c", 32, 7, True, "fs<TPS0,NTT4,NW4>"), _fs("404-L48x3c", 48, 3, True, "fs<TPS0,NTT4,NW4>"),
    _fs("404-L64x2c", 64, 2, True, "fs<TPS0,NTT4,NW4>"),
    # 413: more than 128 three-quarter workgroups (129, the last one ragged), or the half rule switched off
    _fs("413-L16x385", 16, 385, False, "fs<TPS1,NTT3,NW4>"),
    _fs("413-L4x37c-half0", 4, 37, True, "fs<TPS1,NTT3,NW4>", **H0),
    _fs("413-L4x1537c", 4, 1537, True, "fs<TPS1,NTT3,NW4>"),
    _fs("413-L4x1537c-tprop", 4, 1537, True, "fs<TPS1,NTT3,NW4,TPROP>", tprop=True),
    _fs("413-L4x37c-half0-tprop", 4, 37, True, "fs<TPS1,NTT3,NW4,TPROP>", tprop=True, **H0),
    _fs("413-L4x1537c-last", 4, 1537, True, "fs<TPS1,NTT4,NW4,LASTQ>", last=True),          # three quarters -> the 4-tile last-slot form
    _fs("413-L4x1537c-tprop-last", 4, 1537, True, "fs<TPS1,NTT4,NW4,TPROP,LASTQ>", tprop=True, last=True),
    # 414: past 512 three-quarter workgroups (385 full ones: the one place the entry skew applies)
    _fs("414-L16x1537", 16, BIG16, False, "fs<TPS1,NTT4,NW4>"),
    _fs("414-L16x1537-skew3", 16, BIG16, False, "fs<TPS1,NTT4,NW4>", TANTE_FS_SKEW=3),
    _letter("414-T-1x4x77x80", 256, 256, "T", BIGT, "fs<TPS1,NTT4,NW4>"),
    _letter("414-T-1x4x77x80-tprop", 256, 256, "T", BIGT, "fs<TPS1,NTT4,NW4,TPROP>")._replace(tprop=True),
    _fs("424-L32x257", 32, 257, False, "fs<TPS2,NTT4,NW4>"),
    # 808: more than 64 tokens per sequence, or 8 waves forced on lengths that are no tile multiple
    _fs("808-L65x2", 65, 2, False, "fs<TPS0,NTT8,NW8>"), _fs("808-L100x3", 100, 3, False, "fs<TPS0,NTT8,NW8>"),
    _fs("808-L128x2", 128, 2, False, "fs<TPS0,NTT8,NW8>"), _fs("808-L100x2c", 100, 2, True, "fs<TPS0,NTT8,NW8>"),
    _fs("808-L5x13-w8", 5, 13, False, "fs<TPS0,NTT8,NW8>", **W8), _fs("808-L20x7c-w8", 20, 7, True, "fs<TPS0,NTT8,NW8>", **W8),
    # the tile-aligned 8-wave keys
    _fs("816-L4x37-w8", 4, 37, False, "fs<TPS1,NTT6,NW8>", **W8), _fs("826-L32x5-w8", 32, 5, False, "fs<TPS2,NTT6,NW8>", **W8),
    _fs("836-L48x3-w8", 48, 3, False, "fs<TPS3,NTT6,NW8>", **W8), _fs("848-L64x3-w8", 64, 3, False, "fs<TPS4,NTT8,NW8>", **W8),
    _fs("818-L16x1537-w8", 16, BIG16, False, "fs<TPS1,NTT8,NW8>", **W8), _fs("828-L32x769-w8", 32, BIG32, False, "fs<TPS2,NTT8,NW8>", **W8),
    # the paired form: an odd workgroup count, the last workgroup's second group is empty
    _fs("413-L16x385-g2", 16, 385, False, "fs<TPS1,NTT3,NW4,G2>", **G2), _fs("414-L16x1537-g2", 16, BIG16, False, "fs<TPS1,NTT4,NW4,G2>", **G2),
    _fs("424-L32x257-g2", 32, 257, False, "fs<TPS2,NTT4,NW4,G2>", **G2), _fs("433-L48x3-g2", 48, 3, False, "fs<TPS3,NTT3,NW4,G2>", **G2),
    _fs("444-L64x3-g2", 64, 3, False, "fs<TPS4,NTT4,NW4,G2>", **G2), _fs("404-L12x23-g2", 12, 23, False, "fs<TPS0,NTT4,NW4,G2>", **G2),
]

GRID_A, GRID_B, GRID_TS = (2, 4, 5, 3), (1, 3, 16, 7), (3, 4, 8, 2)      # (B, T, H, W), no two extents equal
LAYOUT_CASES = [
    _letter("T-2x4x5x3", 256, 256, "T", GRID_A, "fs<TPS1,NTT2,NW4>"), _letter("H-2x4x5x3", 256, 256, "H", GRID_A, "fs<TPS0,NTT4,NW4>"),
    _letter("W-2x4x5x3", 256, 256, "W", GRID_A, "fs<TPS0,NTT4,NW4>"), _letter("L-2x4x5x3", 256, 256, "L", GRID_A, "fs<TPS0,NTT4,NW4>"),
    _letter("Y-2x4x5x3", 256, 256, "Y", GRID_A, "fs<TPS0,NTT4,NW4>"), _letter("X-2x4x5x3", 256, 256, "X", GRID_A, "fs<TPS0,NTT4,NW4>"),
    _letter("T-1x3x16x7", 256, 256, "T", GRID_B, "fs<TPS0,NTT4,NW4>"), _letter("H-1x3x16x7", 256, 256, "H", GRID_B, "fs<TPS1,NTT2,NW4>"),
    _letter("W-1x3x16x7", 256, 256, "W", GRID_B, "fs<TPS0,NTT4,NW4>"), _letter("L-1x3x16x7", 256, 256, "L", GRID_B, "fs<TPS0,NTT8,NW8>"),
    _letter("Y-1x3x16x7", 256, 256, "Y", GRID_B, "fs<TPS3,NTT3,NW4>"), _letter("X-1x3x16x7", 256, 256, "X", GRID_B, "fs<TPS0,NTT4,NW4>"),
    _letter("subH-2x4x5x3", 256, 256, "H", GRID_A, "fs<TPS0,NTT4,NW4>", sub=True),
    _letter("subW-1x3x16x7", 256, 256, "W", GRID_B, "fs<TPS0,NTT4,NW4>", sub=True),
    _letter("ts-T-3x4x8x2", 128, 128, "T", GRID_TS, "block16<4,4>"), _letter("ts-H-3x4x8x2", 128, 128, "H", GRID_TS, "block16<4,4>"),
    _letter("ts-W-3x4x8x2", 128, 128, "W", GRID_TS, "block32<4,4>", TANTE_BLOCK_KERNEL=32),
]


def _ts_cases():
    out = []
    for ci, (C, hidden) in enumerate(((64, 64), (64, 128), (128, 128), (128, 256), (256, 256))):
        shapes = [(L, "wg+1", c) for L in (1, 4, 32) for c in (False, True)] + [(L, "1", (ci + i) % 2 == 1) for i, L in enumerate((1, 4, 32))]
        shapes.append(((2, 8, 16, 2, 8)[ci], "wg+1", ci % 2 == 0))      # L in {2, 8, 16}: every one of them once (twice over the five widths)
        for L, n, causal in shapes:
            per_wg = 4 if L == 32 else 8 * (16 // L)
            nseq = per_wg + 1 if n == "wg+1" else 1
            for k in (16, 32) + ((0,) if C < 256 else ()):      # at C = 64 / 128 the 16 form is the shipping kernel: also with no choice made
                form = 32 if k == 32 else 16
                out.append(BlockCase(f"ts{k}-C{C}h{hidden}-L{L}x{nseq}{'c' if causal else ''}", C, hidden, L, nseq, causal, False, False,
                                     (("TANTE_BLOCK_KERNEL", k),), f"block{form}<{C // 32},{hidden // 32}>", None))
    return out


TS_CASES = _ts_cases()
BLOCK_CASES = FS_CASES + LAYOUT_CASES + TS_CASES
CASE_BY_ID = {c.id: c for c in BLOCK_CASES}
assert len(CASE_BY_ID) == len(BLOCK_CASES)


# ---- weights and inputs ---------------------------------------------------------------------------------------------------------------
def block_weights(C: int, hidden: int, seed: int) -> Dict[str, torch.Tensor]:
    """A default-initialised TransformerBlock (LayerNorm, nn.MultiheadAttention, Linear - GELU - Linear) under the oracle's names, with the
    perturbations test_fused_block applies: LayerNorm affines away from (1, 0), non-zero attention biases."""
    nn = torch.nn
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        attn = nn.MultiheadAttention(C, C // 32, batch_first=True, dropout=0.0, bias=True)
        fc1, fc2 = nn.Linear(C, hidden), nn.Linear(hidden, C)
        w = {"ln1.weight": torch.ones(C), "ln1.bias": torch.zeros(C), "ln2.weight": torch.ones(C), "ln2.bias": torch.zeros(C),
             "attn.in_proj_weight": attn.in_proj_weight, "attn.in_proj_bias": attn.in_proj_bias, "attn.out_proj.weight": attn.out_proj.weight,
             "attn.out_proj.bias": attn.out_proj.bias, "mlp.0.weight": fc1.weight, "mlp.0.bias": fc1.bias, "mlp.2.weight": fc2.weight,
             "mlp.2.bias": fc2.bias}
        w = {k: v.detach().clone() for k, v in w.items()}
        for k in ("ln1.weight", "ln1.bias", "ln2.weight", "ln2.bias"):
            w[k] += 0.2 * torch.randn(C)
        w["attn.in_proj_bias"] += 0.1 * torch.randn(3 * C)
        w["attn.out_proj.bias"] += 0.1 * torch.randn(C)
        tp = [nn.Linear(4, 4), nn.Linear(4, 4)]
        w["tprop"] = torch.cat([3.0 * p.detach().reshape(-1) for p in (tp[0].weight, tp[0].bias, tp[1].weight, tp[1].bias)])     # a propagator that matters
    return w


PACK_ORDER = ("ln1.weight", "ln1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
              "ln2.weight", "ln2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias")      # kernels.pack_block's params


def tprop_parts(w):
    t = w["tprop"]
    return t[:16].reshape(4, 4), t[16:20], t[20:36].reshape(4, 4), t[36:40]


SLACK_ROWS = 3      # rows behind the last addressed one (and, for a sub-grid, the rows before row0 come with the layout)


class Inputs:
    """buf (rows, C) fp32: 1.5 randn + 0.3 + a per-sequence offset on the addressed rows, NaN everywhere else (the kernels read addressed
    rows only: a dead slot reads the row at the base pointer, which is token (0, 0));  tok (nseq, L) the addressed rows;  w the weights."""


def make_inputs(c: BlockCase) -> Inputs:
    g = torch.Generator().manual_seed(c.seed)
    inp = Inputs()
    inp.tok = seq_tokens(c.seq(), c.row0)
    rows = int(inp.tok.max()) + 1 + SLACK_ROWS
    X = 1.5 * torch.randn(c.nseq, c.L, c.C, generator=g) + 0.3 + 0.25 * ((torch.arange(c.nseq) % 7) - 3.0)[:, None, None]
    inp.buf = torch.full((rows, c.C), float("nan"))
    inp.buf[inp.tok.reshape(-1)] = X.reshape(-1, c.C)
    inp.wseed = c.seed % 100003
    inp.w = block_weights(c.C, c.hidden, inp.wseed)
    assert inp.tok.reshape(-1).unique().numel() == c.nseq * c.L, "a row addressed twice"
    return inp


def written_rows(c: BlockCase, inp: Inputs) -> torch.Tensor:
    """bool (rows,): the rows a launch of the case writes (slot L - 1 alone for a `last` launch)."""
    m = torch.zeros(inp.buf.shape[0], dtype=torch.bool)
    m[(inp.tok[:, c.L - 1] if c.last else inp.tok).reshape(-1)] = True
    return m


def launch_ref(c: BlockCase, inp: Inputs, exact_bf16: bool = False, bug=None) -> torch.Tensor:
    """The buffer after the launch, float64 (rows, C).  Faults at this level (the others are block_ref's):
    ("row_from_next_seq", s, l)  ("last_seq_unwritten",)  ("skip_tprop", s)  ("last_rewrites_slot0", s)."""
    kind = bug[0] if bug else None
    X = inp.buf.double()[inp.tok]                                  # (nseq, L, C)
    if kind == "row_from_next_seq":
        X = X.clone()
        X[bug[1], bug[2]] = X[bug[1] + 1, bug[2]]
    Xp = X
    if c.tprop:
        Xp = tprop_ref(X, tprop_parts(inp.w))
        if kind == "skip_tprop":
            Xp[bug[1]] = X[bug[1]]
    Y = block_ref(inp.w, Xp, c.causal, exact_bf16, bug if kind in ("drop_last_key", "causal_off_by_one", "drop_head", "ln_c_minus_1") else None)
    out = inp.buf.double().clone()
    if c.last:
        out[inp.tok[:, c.L - 1]] = Y[:, c.L - 1]
        if kind == "last_rewrites_slot0":
            out[inp.tok[bug[1], 0]] = Y[bug[1], 0]
    else:
        out[inp.tok.reshape(-1)] = Y.reshape(-1, c.C)
    if kind == "last_seq_unwritten":
        out[inp.tok[c.nseq - 1]] = inp.buf.double()[inp.tok[c.nseq - 1]]
    return out


FAULTS = ("drop_last_key", "causal_off_by_one", "drop_head", "row_from_next_seq", "last_seq_unwritten", "ln_c_minus_1", "skip_tprop",
          "last_rewrites_slot0")
SINGLE_TOKEN_FAULTS = ("drop_head", "row_from_next_seq", "ln_c_minus_1")


def fault_for(c: BlockCase, kind: str):
    """The bug tuple of a fault on a case, or None where the case cannot have it."""
    s, l = c.nseq // 2, c.L // 2
    if kind == "drop_last_key":
        return (kind, s) if c.L > 1 else None
    if kind == "causal_off_by_one":
        return (kind, s) if c.causal and c.L > 1 and not c.last else None      # (the slot-(L - 1) query sees every key either way)
    if kind == "drop_head":
        return (kind, s, c.L - 1 if c.last else l, 1)
    if kind == "row_from_next_seq":
        return (kind, s, c.L - 1 if c.last else l) if s + 1 < c.nseq else None
    if kind == "last_seq_unwritten":
        return (kind,)
    if kind == "ln_c_minus_1":
        return (kind, s, c.L - 1 if c.last else l)
    if kind == "skip_tprop":
        return (kind, s) if c.tprop else None
    if kind == "last_rewrites_slot0":
        return (kind, s) if c.last else None
    raise ValueError(kind)


# ---- error figures --------------------------------------------------------------------------------------------------------------------
def _same(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Row-wise equality of two (rows, C) buffers where NaN equals NaN (fp32 values are exact in float64)."""
    a, b = a.double(), b.double()
    return ((a == b) | (torch.isnan(a) & torch.isnan(b))).all(dim=1)


def errors(got: torch.Tensor, ref: torch.Tensor, x: torch.Tensor, written: torch.Tensor):
    """Over the written rows: (relative L2 of y, scale-relative max of y, relative L2 of y - x)."""
    g, r, xx = got.double()[written], ref.double()[written], x.double()[written]
    return (float((g - r).norm() / r.norm()), float((g - r).abs().max() / r.abs().max()), float((g - r).norm() / (r - xx).norm()))


def token_errors(got: torch.Tensor, ref: torch.Tensor, x: torch.Tensor, written: torch.Tensor) -> torch.Tensor:
    """One figure per ROW OF THE BUFFER, none left out.  A written row:  || (y - x)_got - (y - x)_ref || / || (y - x)_ref ||  -- on the
    block's own contribution, never on y, which the residual dominates (NaN in `got` gives inf).  Any other row -- before row0, between
    the addressed ones, the slack, slots 0 .. L - 2 of a `last` launch -- must hold the bits it held: 0 if it does, inf if not."""
    g, r, xx = got.double(), ref.double(), x.double()
    out = torch.where(_same(g, xx), 0.0, float("inf")).double()
    rn = (r[written] - xx[written]).norm(dim=1)
    assert bool((rn > 0).all()), "a written token whose reference contribution is zero"
    e = (g[written] - r[written]).norm(dim=1) / rn
    out[written] = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    return out


def worst_token(got, ref, x, written) -> float:
    return float(token_errors(got, ref, x, written).max())
