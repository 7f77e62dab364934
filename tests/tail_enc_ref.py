"""The head and encoder kernels alone (tante_amd/csrc/head_fused.hip, head_enc.hip, enc_fused.hip): cases, float64 references, the
exact-bf16 evaluation of each reference, per-token error figures and the restated launch dispatch.  Nothing here touches the GPU:
tests/test_tail_enc_cpu.py pins this file to the oracle, to the text of the three sources and to wrong results;
tests/test_hip_tail_enc.py runs the kernels against it.

The operations, per token (patch_scale 8: three 2 x 2 stages, no overlap, so a token's 8 x 8 x D pixel block depends on that token alone):
  head     rows (C) -> ConvTranspose2d k = s = 2 -> GELU(erf) -> ConvTranspose2d -> GELU -> ConvTranspose2d -> d (D, 8, 8);
           out_i = base + sum_k coef_ik d_k
  encoder  (D, 8, 8) -> Conv2d k = s = 2 -> GELU -> Conv2d -> GELU -> Conv2d -> z (C);  enc23 starts from the stage-1 image h1 (bf16)
           and ends in  z a[img % T] + b[img % T] + s_emb[hw]  or in the frame-major row order  (f, b) <- image (b, f).
The exact-bf16 evaluation rounds to bf16 exactly where the kernels do (token rows, weights, every GELU output, and for head_enc the frame
block that feeds encoder stage 1), uses the kernels' GELU polynomial (common.hip.h, gelu_poly<false>) and keeps everything else in
float64: its distance to float64 is the format's share of a kernel's error, what the kernel adds to it is the kernel's own."""
import math
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

# the project's bf16 bars (relative L2, max-norm) over the whole tensor, and the same relative L2 bar applied to every token's own block
BAR_L2, BAR_MAX, BAR_TOKEN = 1e-2, 2e-2, 1e-2

# ---- GELU -----------------------------------------------------------------------------------------------------------------------------
# common.hip.h, gelu_poly<false>:  x * sat(0.5 + x * Q(min(x^2, X0^2))),  Q of degree 7 in x^2 (Horner, highest coefficient first)
GELU_X0SQ = 18.0625
GELU_Q = (-8.949876396e-10, 7.897345000e-08, -3.026334298e-06, 6.673120515e-05, -9.494310943e-04, 9.293001145e-03, -6.551689655e-02,
          3.984565735e-01)
GELU_POLY_ERR = 8.3e-5        # what common.hip.h states against the erf form on [-10, 10]


def gelu_erf(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_poly(x: torch.Tensor) -> torch.Tensor:
    """The kernels' polynomial with its fp32 coefficients, evaluated in the precision of x."""
    s = torch.clamp(x * x, max=GELU_X0SQ)
    q = torch.full_like(x, float(torch.tensor(GELU_Q[0], dtype=torch.float32)))
    for c in GELU_Q[1:]:
        q = q * s + float(torch.tensor(c, dtype=torch.float32))
    return x * torch.clamp(x * q + 0.5, 0.0, 1.0)


def bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even), back in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _ops(exact_bf16: bool):
    if exact_bf16:
        return bf16, lambda v: bf16(gelu_poly(v))
    return (lambda v: v), gelu_erf


# ---- float64 references ---------------------------------------------------------------------------------------------------------------
def head_blocks(X: torch.Tensor, w, exact_bf16: bool = False, bug: Optional[str] = None) -> torch.Tensor:
    """X (rows, C); w = (w1, b1, w2, b2, w3, b3) of the three ConvTranspose2d (Cin, Cout, 2, 2) -> d (rows, D, 8, 8): pixel
    (y, x) = (4 kh1 + 2 kh2 + kh3, 4 kw1 + 2 kw2 + kw3) of the token's block.  bug = "subpixel_order": stage 2's (kh2, kw2) transposed,
    the one-line mutation test_tail_enc_cpu.py plants."""
    rd, act = _ops(exact_bf16)
    w1, b1, w2, b2, w3, b3 = [t.double() for t in w]
    x = rd(X.double())
    h1 = act(torch.einsum("rc,coab->rabo", x, rd(w1)) + b1)                       # (rows, kh1, kw1, C/2)
    h2 = act(torch.einsum("rabc,cokl->rabklo", h1, rd(w2)) + b2)                  # (rows, kh1, kw1, kh2, kw2, C/4)
    order = "rdalmbkn" if bug == "subpixel_order" else "rdakmbln"
    d = torch.einsum("rabklc,cdmn->" + order, h2, rd(w3)) + b3[None, :, None, None, None, None, None, None]
    return d.reshape(X.shape[0], b3.numel(), 8, 8)


def blocks_to_frames(blk: torch.Tensor, n_img: int, Hp: int, Wp: int) -> torch.Tensor:
    """(rows, D, 8, 8), rows = (img, hp, wp) -> (n_img, D, 8 Hp, 8 Wp)."""
    D = blk.shape[1]
    return blk.reshape(n_img, Hp, Wp, D, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(n_img, D, 8 * Hp, 8 * Wp)


def frames_to_blocks(fr: torch.Tensor) -> torch.Tensor:
    """(n_img, D, 8 Hp, 8 Wp) -> (rows, D, 8, 8)."""
    n, D, H, W = fr.shape
    return fr.reshape(n, D, H // 8, 8, W // 8, 8).permute(0, 2, 4, 1, 3, 5).reshape(n * (H // 8) * (W // 8), D, 8, 8)


def head_derivative(Xs, ws, coefs, exact_bf16: bool = False, bug: Optional[str] = None) -> torch.Tensor:
    """sum_k coef_ik d_k as token blocks: Xs[k] (rows, C), ws[k] the six tensors of order k, coefs (n_out, n_ord) -> (n_out, rows, D, 8, 8)."""
    ds = torch.stack([head_blocks(X, w, exact_bf16, bug) for X, w in zip(Xs, ws)])            # (n_ord, rows, D, 8, 8)
    return torch.einsum("ik,krdyx->irdyx", torch.as_tensor(coefs, dtype=torch.float64), ds)


def enc_stage1(frames: torch.Tensor, w1, b1, exact_bf16: bool = False) -> torch.Tensor:
    """(n_img, D, H, W) -> channels-last (n_img, H / 2, W / 2, C / 4) after GELU."""
    rd, act = _ops(exact_bf16)
    n, D, H, W = frames.shape
    x = rd(frames.double()).reshape(n, D, H // 2, 2, W // 2, 2)
    return act(torch.einsum("ndhkwl,odkl->nhwo", x, rd(w1.double())) + b1.double())


def enc23_rows(h1: torch.Tensor, w, exact_bf16: bool = False, bug: Optional[str] = None) -> torch.Tensor:
    """h1 (n_img, 4 Hp, 4 Wp, C / 4); w = (w2, b2, w3, b3) of the two Conv2d (Cout, Cin, 2, 2) -> (n_img Hp Wp, C), rows (img, hp, wp).
    bug = ("bias3", ch): the stage-3 bias of one channel dropped."""
    rd, act = _ops(exact_bf16)
    w2, b2, w3, b3 = [t.double() for t in w]
    if isinstance(bug, tuple) and bug[0] == "bias3":
        b3 = b3.clone()
        b3[bug[1]] = 0.0
    n, H1, W1, C1 = h1.shape
    x = h1.double().reshape(n, H1 // 4, 2, 2, W1 // 4, 2, 2, C1)                   # (img, hp, py, kh, wp, px, kw, c)
    s2 = act(torch.einsum("nhpkwqlc,ockl->nhwpqo", x, rd(w2)) + b2)               # (img, hp, wp, py, px, C / 2)
    s3 = torch.einsum("nhwpqc,ocpq->nhwo", s2, rd(w3)) + b3
    return s3.reshape(-1, b3.numel())


def encoder_rows(frames: torch.Tensor, w, exact_bf16: bool = False, bug: Optional[str] = None) -> torch.Tensor:
    """The whole three-stage encoder of a frame: w = (w1, b1, w2, b2, w3, b3) -> z (n_img Hp Wp, C) before FiLM."""
    return enc23_rows(enc_stage1(frames, w[0], w[1], exact_bf16), w[2:], exact_bf16, bug)


def film_epilogue(z: torch.Tensor, fa, fb, s_emb, T: int, HW: int, t_shift: int = 0) -> torch.Tensor:
    """rows (img, hw): z a[img % T] + b[img % T] + s_emb[hw].  t_shift = 1: the table row of slot t + 1 (a planted fault)."""
    r = torch.arange(z.shape[0])
    t = (r // HW + t_shift) % T
    return z * fa.double()[t] + fb.double()[t] + s_emb.double()[r % HW]


def frame_major(z: torch.Tensor, n_img: int, frames: int, HW: int, swap: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """Image (b, f) = b frames + f goes to row block f (n_img / frames) + b.  swap: two images exchanged (a planted fault)."""
    nb = n_img // frames
    blocks = z.reshape(n_img, HW, -1)
    src = list(range(n_img))
    if swap is not None:
        src[swap[0]], src[swap[1]] = src[swap[1]], src[swap[0]]
    out = torch.empty_like(blocks)
    for img in range(n_img):
        out[(img % frames) * nb + img // frames] = blocks[src[img]]
    return out.reshape(n_img * HW, -1)


# ---- error figures --------------------------------------------------------------------------------------------------------------------
def errors(got: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """(relative L2, max-norm) over the whole tensor."""
    g, r = got.double(), ref.double()
    return float((g - r).norm() / r.norm()), float((g - r).abs().max())


def token_errors(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """Relative L2 of every token's own block against that block's reference norm.  (rows, C) gives one figure per row;
    (n_out, rows, D, 8, 8) one per frame and token.  Nothing is left out: a token whose reference block is zero has no figure and fails the
    assertion below instead of being skipped."""
    g, r = got.double(), ref.double()
    lead = 1 if r.dim() == 2 else 2
    n = 1
    for s in r.shape[:lead]:
        n *= s
    g, r = g.reshape(n, -1), r.reshape(n, -1)
    rn = r.norm(dim=1)
    assert bool((rn > 0).all()), "a token with a zero reference block"
    return (g - r).norm(dim=1) / rn


def worst_token(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float(token_errors(got, ref).max())


# ---- restated dispatch ----------------------------------------------------------------------------------------------------------------
HEAD_WIDE_ROWS = 128 * 56       # launch_head / he_group_tokens: 128-token groups once they still give every CU a workgroup


def head_group_tokens(rows: int, option: int = 0) -> int:
    """Tokens per workgroup of the head kernels: TANTE_HEAD_WAVES (0 = unset) forces 8 waves (128) or anything else (64)."""
    wide = (option == 8) if option else rows >= HEAD_WIDE_ROWS
    return 128 if wide else 64


ENC23_SPLIT4_GROUPS, ENC23_SPLIT2_GROUPS = 64, 128


def enc23_split(rows: int, option: int = 0) -> int:
    """Workgroups that share a 128-row group in stage 3 of enc23_kernel: TANTE_ENC23_SPLIT (0 = unset) forces it."""
    groups = (rows + 127) // 128
    split = option if option else (4 if groups <= ENC23_SPLIT4_GROUPS else 2 if groups <= ENC23_SPLIT2_GROUPS else 1)
    return 4 if split >= 4 else 2 if split == 2 else 1


def head_enc_ndt(D: int) -> int:
    """16-row stage-3 tiles that hold real channels: the NDT template value of head_enc_kernel."""
    return min((D + 3) // 4, 4)


def head_route(C: int, multi: bool, rows: int, option: int = 0) -> str:
    return f"head<CB{C // 32},NWV{head_group_tokens(rows, option) // 16},{'MULTI' if multi else 'ONE'}>"


def head_enc_route(D: int, enc: bool, rows: int, option: int = 0) -> str:
    return f"head_enc<NWV{head_group_tokens(rows, option) // 16},{'ENC' if enc else 'NOENC'},NDT{head_enc_ndt(D)}>"


def enc23_route(rows: int, option: int = 0) -> str:
    return f"enc23<SPLIT{enc23_split(rows, option)}>"


def swz_chunk(r: int, c: int, cpr: int) -> int:
    """common.hip.h: where 16-byte chunk c of row r of a packed weight tile lies inside that row (cpr chunks per row)."""
    return (c ^ (r & 15)) if cpr >= 16 else (c ^ ((r >> 1) & 7)) if cpr >= 8 else (c ^ ((r >> 2) & 3))


def head_tiles(C: int):
    """(rows, chunks per row) of the head stream's three kinds of tile (HeadGeom<C / 32>): W1 pixel tile, W2 sub-pixel tile, W3."""
    return [(C // 2, C // 8), (C // 4, C // 16), (64, C // 32)]


ALL_HEAD_ROUTES = {f"head<CB{cb},NWV{nw},{m}>" for cb in (4, 8) for nw in (4, 8) for m in ("ONE", "MULTI")}
ALL_HEAD_ENC_ROUTES = {f"head_enc<NWV{nw},{e},NDT{n}>" for nw in (4, 8) for e in ("ENC", "NOENC") for n in (1, 2, 3, 4)}
ALL_ENC23_ROUTES = {f"enc23<SPLIT{s}>" for s in (4, 2, 1)}


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Addr:
    """Row r of a stream lies at (r // a_n0) * a_s1 + (r % a_n0) * a_s0 + a_off (elements); `size` elements hold every addressed row."""
    a_n0: int
    a_s1: int
    a_s0: int
    a_off: int
    size: int

    def offsets(self, rows: int) -> torch.Tensor:
        r = torch.arange(rows)
        return (r // self.a_n0) * self.a_s1 + (r % self.a_n0) * self.a_s0 + self.a_off


@dataclass
class HeadCase:
    """kind "one": tante_head_fused (one order per launch, n_out frames);  "multi": tante_head_fused_multi and _streams (n_ord orders, one
    frame);  "head_enc": tante_head_enc_fused (n_ord orders, one frame, C = 256, whole 16-token tiles).
    options: the TANTE_HEAD_WAVES values the case runs under (0 = unset, the default rule)."""
    kind: str
    C: int
    D: int
    shape: Tuple[int, int, int]          # (n_img, Hp, Wp)
    n_ord: int = 1
    n_out: int = 1
    last: str = "given"                  # "given": out_i = last + ...;  "null": accumulate onto a pre-filled out (kind "one" only)
    addr: str = "model"                  # "model": a_n0 = HW, a_s1 = T HW C, a_off = last slot;  "padded": a_s0 = C + 4;  "odd": a_n0 = 11
    out_gap: int = 0                     # frames of slack between the batch entries of out (out_bstride = (n_out + out_gap) frames)
    last_pad: int = 0                    # elements of slack between the batch entries of last (last_bstride = frame + last_pad)
    options: Tuple[int, ...] = (4, 8)

    @property
    def rows(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def id(self):
        n, h, w = self.shape
        s = f"{self.kind}-C{self.C}-D{self.D}-{n}x{h}x{w}-ord{self.n_ord}-out{self.n_out}"
        for flag, name in ((self.last == "null", "acc"), (self.addr != "model", self.addr), (self.out_gap, f"gap{self.out_gap}"),
                           (self.last_pad, f"lastpad{self.last_pad}"), (self.options == (0,), "default")):
            if flag:
                s += "-" + name
        return s

    @property
    def seed(self):
        return zlib.crc32(self.id.encode()) & 0x7fffffff

    def address(self) -> Addr:
        n_img, Hp, Wp = self.shape
        HW, C, T = Hp * Wp, self.C, 2
        if self.addr == "odd":          # 11 divides neither 16 nor any HW of the list: addressing blocks straddle tiles and images
            a_n0, a_s0, a_off = 11, C, 12
            a_s1 = a_n0 * a_s0 + 8
            return Addr(a_n0, a_s1, a_s0, a_off, ((self.rows + a_n0 - 1) // a_n0) * a_s1 + a_off + 4)
        s0 = C + (4 if self.addr == "padded" else 0)
        return Addr(HW, T * HW * s0, s0, (T - 1) * HW * s0, n_img * T * HW * s0)

    def routes(self):
        if self.kind == "head_enc":
            return [head_enc_route(self.D, e, self.rows, o) for o in self.options for e in (True, False)]
        return [head_route(self.C, self.kind == "multi", self.rows, o) for o in self.options]

    def coefs(self):
        """(n_out, n_ord), all distinct, of order one (a coefficient of 1e-3 would leave the derivative part of an fp32 frame a few
        significant digits only)."""
        return [[(0.9 - 0.08 * i - 0.13 * k) * (-1.0) ** k for k in range(self.n_ord)] for i in range(self.n_out)]


S45, S147, S567, S1071 = (3, 5, 3), (7, 3, 7), (9, 7, 9), (17, 7, 9)

HEAD_CASES = [
    # tante_head_fused: every output form, both widths, D over a partly filled tile / a second tile with one live channel / the full 16
    HeadCase("one", 128, 3, S45, n_out=3),
    HeadCase("one", 128, 16, S147, last="null"),
    HeadCase("one", 128, 5, S567, n_out=8, out_gap=2, last_pad=24),
    HeadCase("one", 128, 1, S1071),
    HeadCase("one", 256, 11, S45, n_out=1, last_pad=8),
    HeadCase("one", 256, 4, S147, n_out=3, last="null", out_gap=1),
    HeadCase("one", 256, 1, S567, n_out=8),
    HeadCase("one", 256, 16, S1071),
    HeadCase("one", 256, 5, S147, addr="padded"),
    HeadCase("one", 256, 3, S45, addr="odd", n_out=3),
    HeadCase("one", 128, 11, S147, addr="odd"),
    HeadCase("one", 256, 1, (7, 32, 32), options=(0,)),        # exactly 7168 rows: the 8-wave form by the default rule
    # tante_head_fused_multi (dense copies) and _streams (whole streams)
    HeadCase("multi", 256, 4, S45, n_ord=1),
    HeadCase("multi", 256, 11, S147, n_ord=2),
    HeadCase("multi", 256, 3, S567, n_ord=3),
    HeadCase("multi", 256, 5, S1071, n_ord=4),
    HeadCase("multi", 128, 16, S45, n_ord=4, last_pad=16),
    HeadCase("multi", 128, 1, S147, n_ord=3, addr="padded"),
    HeadCase("multi", 128, 5, S567, n_ord=2, out_gap=1),
    HeadCase("multi", 128, 3, S1071, n_ord=1),
]

HEAD_ENC_CASES = [
    HeadCase("head_enc", 256, 1, (3, 4, 4), n_ord=1),            # 48 rows: one tile per image, the last group has dead tiles
    HeadCase("head_enc", 256, 4, (3, 4, 4), n_ord=2),
    HeadCase("head_enc", 256, 5, (3, 4, 12), n_ord=2, last_pad=32),
    HeadCase("head_enc", 256, 9, (10, 8, 8), n_ord=3),           # 640 rows: 10 groups at 64 tokens
    HeadCase("head_enc", 256, 16, (18, 8, 8), n_ord=4, out_gap=1),   # 1152 rows: 9 groups at 128 tokens
]


@dataclass
class Enc23Case:
    """tante_enc23_fused (FiLM tables of T rows) and tante_enc23_frames (frames = T) on the same stage-1 image; every split by option."""
    shape: Tuple[int, int, int]
    T: int
    options: Tuple[int, ...] = (4, 2, 1)
    C: int = 256

    @property
    def rows(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def id(self):
        n, h, w = self.shape
        return f"enc23-{n}x{h}x{w}-T{self.T}"

    @property
    def seed(self):
        return zlib.crc32(self.id.encode()) & 0x7fffffff

    def routes(self):
        return [enc23_route(self.rows, o) for o in self.options]


ENC23_CASES = [
    Enc23Case((6, 5, 9), 3),       # 270 rows: 3 workgroups, the last one ragged; tokens straddle images
    Enc23Case((2, 1, 1), 2),       # 2 rows
    Enc23Case((4, 8, 8), 4),       # 256 rows: exactly 2 groups
]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
class Inputs:
    pass


def _default_init(mod_ctor, seed: int):
    """The parameters of a torch module under its default initialisation (what dec_CNN / enc_CNN hold when they are built)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = mod_ctor()
    return m.weight.detach().clone(), m.bias.detach().clone()


def dec_weights(C: int, D: int, seed: int):
    """(w1, b1, w2, b2, w3, b3) of dec_CNN(embed_dim = C, patch_scale = 8, n_fields = D): ConvTranspose2d (Cin, Cout, 2, 2)."""
    out = []
    for i, (ci, co) in enumerate(((C, C // 2), (C // 2, C // 4), (C // 4, D))):
        out += _default_init(lambda: torch.nn.ConvTranspose2d(ci, co, (2, 2), stride=(2, 2)), seed * 8 + i)
    return tuple(out)


def enc_weights(C: int, D: int, seed: int):
    """(w1, b1, w2, b2, w3, b3) of enc_CNN(embed_dim = C, patch_scale = 8, n_fields = D): Conv2d (Cout, Cin, 2, 2)."""
    out = []
    for i, (ci, co) in enumerate(((D, C // 4), (C // 4, C // 2), (C // 2, C))):
        out += _default_init(lambda: torch.nn.Conv2d(ci, co, (2, 2), stride=(2, 2)), seed * 8 + 4 + i)
    return tuple(out)


def make_head_inputs(c: HeadCase) -> Inputs:
    """Unit-variance token rows per order, laid into NaN-filled stream buffers by the case's addressing; dense copies of the same rows;
    `last` with its batch stride (NaN in the slack); for "null" the pre-filled frames."""
    g = torch.Generator().manual_seed(c.seed)
    n_img, Hp, Wp = c.shape
    inp = Inputs()
    inp.addr = c.address()
    off = inp.addr.offsets(c.rows)
    inp.X, inp.streams, inp.w = [], [], []
    for k in range(c.n_ord):
        X = torch.randn(c.rows, c.C, generator=g)
        buf = torch.full((inp.addr.size,), float("nan"))
        buf[(off[:, None] + torch.arange(c.C)[None, :]).reshape(-1)] = X.reshape(-1)
        inp.X.append(X)
        inp.streams.append(buf)
        inp.w.append(dec_weights(c.C, c.D, c.seed % 100000 + k))
    inp.frame = c.D * 64 * Hp * Wp
    inp.base = torch.randn(n_img, c.n_out if c.last == "null" else 1, c.D, 8 * Hp, 8 * Wp, generator=g)
    inp.last_bstride = inp.frame + c.last_pad
    inp.out_bstride = (c.n_out + c.out_gap) * inp.frame
    if c.kind == "head_enc":
        inp.we = enc_weights(c.C, c.D, c.seed % 100000 + 7)
    return inp


def head_reference(c: HeadCase, inp: Inputs, exact_bf16: bool = False, bug: Optional[str] = None) -> torch.Tensor:
    """The derivative part  out_i - base  as token blocks (n_out, rows, D, 8, 8)."""
    return head_derivative(inp.X, inp.w, c.coefs(), exact_bf16, bug)


def head_base_blocks(c: HeadCase, inp: Inputs) -> torch.Tensor:
    """What the derivative is added to, as token blocks (n_out, rows, D, 8, 8): `last` for every frame, or the pre-filled frames."""
    b = inp.base.double()
    if c.last != "null":
        b = b.expand(-1, c.n_out, -1, -1, -1)
    return torch.stack([frames_to_blocks(b[:, i]) for i in range(c.n_out)])


def make_enc23_inputs(c: Enc23Case) -> Inputs:
    """h1 drawn directly as bf16 with the statistics of a stage-1 image of unit-variance frames (GELU of a zero-mean value of variance 1 / 3:
    default-initialised Conv2d weights give var(out) = var(in) / 3); FiLM tables with distinct rows per t, of the size of the embeddings'
    default initialisation -- tables of unit size would bury the encoder's own values, and with them its errors, in every figure."""
    g = torch.Generator().manual_seed(c.seed)
    n_img, Hp, Wp = c.shape
    inp = Inputs()
    inp.h1 = gelu_erf(torch.randn(n_img, 4 * Hp, 4 * Wp, c.C // 4, generator=g, dtype=torch.float64) / math.sqrt(3.0)).to(torch.bfloat16)
    inp.w = enc_weights(c.C, 4, c.seed % 100000)[2:]
    inp.film_a = 1.0 + 0.5 * torch.randn(c.T, c.C, generator=g)
    inp.film_b = 0.1 * torch.randn(c.T, c.C, generator=g)
    inp.s_emb = 0.1 * torch.randn(Hp * Wp, c.C, generator=g)
    return inp


def enc23_reference(c: Enc23Case, inp: Inputs, form: str, exact_bf16: bool = False, bug=None) -> torch.Tensor:
    """form "film": the FiLM + position epilogue;  "frames": the frame-major order, no FiLM;  "rows": neither."""
    n_img, Hp, Wp = c.shape
    z = enc23_rows(inp.h1, inp.w, exact_bf16, bug if isinstance(bug, tuple) and bug[0] == "bias3" else None)
    if form == "film":
        return film_epilogue(z, inp.film_a, inp.film_b, inp.s_emb, c.T, Hp * Wp, t_shift=1 if bug == "film_t+1" else 0)
    if form == "frames":
        return frame_major(z, n_img, c.T, Hp * Wp, swap=bug[1] if isinstance(bug, tuple) and bug[0] == "swap" else None)
    return z
