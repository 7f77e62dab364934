"""No GPU: what tests/test_hip_tail_enc.py relies on is itself held here.  The float64 references of tests/tail_enc_ref.py against
oracle.tante_oracle; the restated launch dispatch against the text of head_fused.hip, head_enc.hip and enc_fused.hip; the case list
against the launch switches (every template instance reached); the exact-bf16 evaluation's own distance to float64 (at most half the
per-token bar on every case); and the bars against wrong results of the kinds these kernels can produce.

Why a per-token bar.  PLANTED below lists, for each fault planted into the exact-bf16 result of the largest case of a kernel, whether
the whole-tensor bars the model-level tests hold would have passed it, as (the relative L2 bars, the max-norm bar): for the heads
`out = last + c d` relative L2 < 1e-2 with the derivative part's relative L2 < 2e-2, and max < 2e-2 on `out`
(tests/test_hip_parity.py::test_fused_head_against_oracle); for encoder rows relative L2 < 1e-2, max < 2e-2.  Measured here:
  the relative L2 bars pass every single-token fault of the heads -- a token with its neighbour's block (7168 tokens: out 1.4e-3,
  derivative 6.1e-3; 1071 tokens, four orders: 2.8e-3 / 1.06e-2) and two swapped sub-pixels of one token (1.1e-3 / 4.9e-3 and
  8.4e-4 / 3.2e-3) -- and nothing else of the list;
  the max-norm bar rejects them at coefficients of order one, and only because it is absolute: a wrong value of these derivative
  fields is 0.2 - 0.4.  Under the coefficient of the third Taylor order at dt = 0.5, (dt)^3 / 3! = 1 / 48, the same wrong token is
  5.5e-3 at most and BOTH whole-tensor bars pass it.
The per-token bar (every token's block within 1e-2 relative L2 of its own reference block) is relative where the fault is: it rejects
every fault of the list, the weakest by a factor of 2.4 (the dropped stage-3 bias of one channel under FiLM, 2.4e-2), the single-token
faults by 10 - 140, whatever the coefficient."""
import os
import re

import pytest
import torch

import tail_enc_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "tante_amd", "csrc")
HEAD_SRC = open(os.path.join(CSRC, "head_fused.hip")).read()
HE_SRC = open(os.path.join(CSRC, "head_enc.hip")).read()
ENC_SRC = open(os.path.join(CSRC, "enc_fused.hip")).read()

# fault -> (do the relative L2 bars of the model-level tests pass it?, does their max-norm bar?)  (measured by test_bars_reject_near_misses, which asserts this table)
PLANTED = {
    "head one: a token gets its neighbour's block": (True, False),
    "head one: two sub-pixels of one token swapped": (True, False),
    "head one, coefficients / 48: a token gets its neighbour's block": (True, True),
    "head multi: a token gets its neighbour's block": (True, False),
    "head multi: two sub-pixels of one token swapped": (True, False),
    "head multi: the coefficients of two orders exchanged": (False, False),
    "head (all tokens): stage 2's sub-pixel order transposed": (False, False),
    "head_enc z: a token gets its neighbour's row": (False, False),
    "head_enc z: the stage-3 bias of one channel dropped": (False, False),
    "enc23 film: a token gets its neighbour's row": (False, False),
    "enc23 film: the stage-3 bias of one channel dropped": (False, False),
    "enc23 film: the FiLM row of slot t + 1": (False, False),
    "enc23 frames: the stage-3 bias of one channel dropped": (False, False),
    "enc23 frames: two images swapped in the frame-major order": (False, False),
}


def _largest(cases, kind=None):
    cs = [c for c in cases if kind is None or c.kind == kind]
    return max(cs, key=lambda c: c.rows)


@pytest.fixture(scope="module")
def evaluated():
    """Every case's inputs, float64 reference and exact-bf16 evaluation, computed once.  Heads: the derivative part as token blocks;
    head_enc: also z of the float64 frame (standing in for the frame a kernel wrote); enc23: both epilogues."""
    out = {}
    for c in R.HEAD_CASES + R.HEAD_ENC_CASES:
        inp = R.make_head_inputs(c)
        e = {"inp": inp, "ref": R.head_reference(c, inp), "bf": R.head_reference(c, inp, exact_bf16=True)}
        if c.kind == "head_enc":
            n_img, Hp, Wp = c.shape
            frame = (R.blocks_to_frames((R.head_base_blocks(c, inp) + e["ref"])[0], n_img, Hp, Wp)).float()
            e["frame"] = frame
            e["z_ref"] = R.encoder_rows(frame, inp.we)
            e["z_bf"] = R.encoder_rows(frame, inp.we, exact_bf16=True)
        out[c.id] = e
    for c in R.ENC23_CASES:
        inp = R.make_enc23_inputs(c)
        out[c.id] = {"inp": inp, **{f: (R.enc23_reference(c, inp, f), R.enc23_reference(c, inp, f, exact_bf16=True)) for f in ("film", "frames")}}
    return out


# ---- against the oracle ---------------------------------------------------------------------------------------------------------------
def test_references_match_the_oracle():
    """head_blocks / head_derivative against dec_cnn + taylor_coeff, encoder_rows against enc_cnn, enc23_rows + film_epilogue against
    tante_embed (FiLM of a real MLP, s_emb, t_emb), frame_major against a permute: float64 on the same weights, to 1e-10.  The restated
    GELU polynomial stays within the 8.3e-5 of common.hip.h of the erf form on [-10, 10], in float64 and evaluated in float32."""
    from oracle import tante_oracle as O
    g = torch.Generator().manual_seed(11)
    for C, D, (B, Hp, Wp), n_ord, n_out in ((128, 3, (3, 5, 3), 2, 3), (256, 11, (2, 3, 7), 3, 1)):
        rows = B * Hp * Wp
        Xs = [torch.randn(rows, C, generator=g, dtype=torch.float64) for _ in range(n_ord)]
        ws = [R.dec_weights(C, D, 40 + k) for k in range(n_ord)]
        last = torch.randn(B, D, 8 * Hp, 8 * Wp, generator=g, dtype=torch.float64)
        dt = 0.5
        coefs = [[O.taylor_coeff(i + 1, dt, k + 1) for k in range(n_ord)] for i in range(n_out)]
        want = last[:, None].repeat(1, n_out, 1, 1, 1)
        for k in range(n_ord):
            wd = {f"dec_conv_{i + 1}.deconv.{n}": ws[k][2 * i + j].double() for i in range(3) for j, n in enumerate(("weight", "bias"))}
            d = O.dec_cnn(wd, Xs[k].view(B, 1, Hp, Wp, C), 8, 0.0)                     # (B, 1, D, H, W)
            rel, mx = R.errors(R.blocks_to_frames(R.head_blocks(Xs[k], ws[k]), B, Hp, Wp), d[:, 0])
            assert rel < 1e-10 and mx < 1e-10, (C, D, rel, mx)
            for i in range(n_out):
                want[:, i] += d[:, 0] * coefs[i][k]
        der = R.head_derivative(Xs, ws, coefs)
        got = torch.stack([last + R.blocks_to_frames(der[i], B, Hp, Wp) for i in range(n_out)], 1)
        rel, mx = R.errors(got, want)
        assert rel < 1e-10 and mx < 1e-10, (C, D, rel, mx)
        assert torch.equal(R.frames_to_blocks(R.blocks_to_frames(der[0], B, Hp, Wp)), der[0])
    # the encoder, alone and under FiLM + embeddings
    C, D, B, T, Hp, Wp = 256, 5, 2, 3, 5, 9
    we = R.enc_weights(C, D, 3)
    x = torch.randn(B, T, D, 8 * Hp, 8 * Wp, generator=g, dtype=torch.float64)
    w = {f"encoder.enc_conv_{i + 1}.conv.{n}": we[2 * i + j].double() for i in range(3) for j, n in enumerate(("weight", "bias"))}
    for n in ("scale", "shift"):
        for i, p, s in ((0, "weight", (7, 1)), (0, "bias", (7,)), (2, "weight", (C, 7)), (2, "bias", (C,))):
            w[f"t_encode.condition_to_{n}.{i}.{p}"] = torch.randn(*s, generator=g, dtype=torch.float64)
    w["s_emb"] = torch.randn(1, Hp, Wp, C, generator=g, dtype=torch.float64)
    w["t_emb"] = torch.randn(1, T, C, generator=g, dtype=torch.float64)
    frames = x.reshape(B * T, D, 8 * Hp, 8 * Wp)
    z = R.encoder_rows(frames, we)
    rel, mx = R.errors(z, O.enc_cnn(O.sub(w, "encoder."), x, 8, 0.0).reshape(-1, C))
    assert rel < 1e-10 and mx < 1e-10, (rel, mx)
    h1 = R.enc_stage1(frames, we[0], we[1])
    assert torch.equal(R.enc23_rows(h1, we[2:]), z)
    cfg = O.TanteCfg(T, D, (8 * Hp, 8 * Wp), taylor_order=1, attn_axes="T", embed_dim=C, patch_scale=8)
    t = O.t_series(T, cfg.frame_interval).double()
    fa = 1.0 + O._film_mlp(O.sub(w, "t_encode."), "condition_to_scale", t)
    fb = O._film_mlp(O.sub(w, "t_encode."), "condition_to_shift", t) + w["t_emb"][0]
    got = R.film_epilogue(z, fa, fb, w["s_emb"].reshape(Hp * Wp, C), T, Hp * Wp)
    rel, mx = R.errors(got, O.tante_embed(w, cfg, x).reshape(-1, C))
    assert rel < 1e-10 and mx < 1e-10, (rel, mx)
    fm = R.frame_major(z, B * T, T, Hp * Wp)
    assert torch.equal(fm, z.reshape(B, T, Hp * Wp, C).permute(1, 0, 2, 3).reshape(-1, C))
    # GELU
    xs = torch.linspace(-10.0, 10.0, 400001, dtype=torch.float64)
    assert float((R.gelu_poly(xs) - R.gelu_erf(xs)).abs().max()) <= R.GELU_POLY_ERR
    assert float((R.gelu_poly(xs.float()).double() - R.gelu_erf(xs)).abs().max()) <= R.GELU_POLY_ERR
    assert float((R.gelu_erf(xs) - O.gelu_erf(xs)).abs().max()) < 1e-15


# ---- against the source text ----------------------------------------------------------------------------------------------------------
def test_dispatch_matches_the_source():
    """The restated thresholds, options and GELU coefficients are read out of the sources, and the template instances the three launchers
    can select are counted from their launch switches: a changed threshold or a new instance fails THIS test."""
    # head_fused.hip
    m = re.search(r'const int force = tante_opt\("TANTE_HEAD_WAVES", 0\);\n\s*const bool wide = force \? force == 8 : rows >= (\d+) \* (\d+);', HEAD_SRC)
    assert m and int(m.group(1)) * int(m.group(2)) == R.HEAD_WIDE_ROWS
    assert sorted(int(x) for x in re.findall(r"launch_head_nw<CB, (\d), MULTI>\(A, s\)", HEAD_SRC)) == [4, 8]
    heads = re.findall(r"launch_head<(\d)(, true)?>\(A, \(hipStream_t\)stream\)", HEAD_SRC)
    assert sorted(heads) == [("4", ""), ("4", ", true"), ("8", ""), ("8", ", true")]
    assert "A.groups = (int)((rows + NWV * 16 - 1) / (NWV * 16));" in HEAD_SRC
    assert 'return (C == 128 || C == 256) && D >= 1 && D <= 16;' in HEAD_SRC
    inst = {f"head<CB{cb},NWV{nw},{'MULTI' if mu else 'ONE'}>" for cb, mu in heads for nw in (4, 8)}
    assert inst == R.ALL_HEAD_ROUTES and len(inst) == 8
    # head_enc.hip
    m = re.search(r'const int force = tante_opt\("TANTE_HEAD_WAVES", 0\);\n\s*return \(force \? force == 8 : rows >= (\d+) \* (\d+)\) \? 128 : 64;', HE_SRC)
    assert m and int(m.group(1)) * int(m.group(2)) == R.HEAD_WIDE_ROWS
    assert "switch ((A.D + 3) / 4) {" in HE_SRC
    ndt = re.findall(r"(case (\d)|default): launch_head_enc_k<NWV, TT, ENC, (\d)>\(A, s\); break;", HE_SRC)
    assert [(a[1] or "default", a[2]) for a in ndt] == [("1", "1"), ("2", "2"), ("3", "3"), ("default", "4")]
    nw = re.findall(r"launch_head_enc_nw<(\d), 1, (true|false)>\(A, s\)", HE_SRC)
    assert sorted(nw) == [("4", "false"), ("4", "true"), ("8", "false"), ("8", "true")]
    assert "if (gt == 128) { if (enc) launch_head_enc_nw<8, 1, true>" in HE_SRC and "const bool enc = enc_stream != nullptr;" in HE_SRC
    inst = {f"head_enc<NWV{n},{'ENC' if e == 'true' else 'NOENC'},NDT{a[2]}>" for n, e in nw for a in ndt}
    assert inst == R.ALL_HEAD_ENC_ROUTES and len(inst) == 16
    assert [R.head_enc_ndt(D) for D in (1, 4, 5, 8, 9, 12, 13, 16)] == [1, 1, 2, 2, 3, 3, 4, 4]
    # the guard of the C entry point stands in front of the launch
    guard = HE_SRC.index("if (((long)Hp * Wp) % 16 || a_n0 % 16)")
    assert HE_SRC.index('extern "C" int tante_head_enc_fused(') < guard < HE_SRC.index("if (gt == 128) { if (enc) launch_head_enc_nw")
    assert "TANTE_FAIL(-2, \"tante_head_enc_fused: whole 16-token tiles expected" in HE_SRC
    # enc_fused.hip
    m = re.search(r'const int force = tante_opt\("TANTE_ENC23_SPLIT", 0\);\n\s*const int groups = \(int\)\(\(rows \+ 127\) / 128\);\n'
                  r"\s*const int split = force \? force : \(groups <= (\d+) \? 4 : groups <= (\d+) \? 2 : 1\);", ENC_SRC)
    assert m and (int(m.group(1)), int(m.group(2))) == (R.ENC23_SPLIT4_GROUPS, R.ENC23_SPLIT2_GROUPS)
    assert re.findall(r"(if \(split >= 4\)|else if \(split == 2\)|else) launch_enc23_s<CB, (\d)>\(A, rows, s\);", ENC_SRC) == [
        ("if (split >= 4)", "4"), ("else if (split == 2)", "2"), ("else", "1")]
    assert ENC_SRC.count("launch_enc23<8>(A, (hipStream_t)stream);") == 3       # fused, frames, and the raw window's second launch
    assert {f"enc23<SPLIT{s}>" for s in re.findall(r"launch_enc23_s<CB, (\d)>\(A, rows, s\);", ENC_SRC)} == R.ALL_ENC23_ROUTES
    # the thresholds, on either side
    assert (R.head_group_tokens(7167), R.head_group_tokens(7168), R.head_group_tokens(45, 8), R.head_group_tokens(10 ** 6, 4)) == (64, 128, 128, 64)
    assert [R.enc23_split(r) for r in (1, 64 * 128, 64 * 128 + 1, 128 * 128, 128 * 128 + 1)] == [4, 4, 2, 2, 1]
    assert [R.enc23_split(270, o) for o in (4, 2, 1, 8, 3)] == [4, 2, 1, 4, 1]
    # the GELU polynomial
    common = open(os.path.join(CSRC, "common.hip.h")).read()
    erf_side = [float(x) for x in re.findall(r"splat\(TANH \? [-+0-9.e]+f : ([-+0-9.e]+)f\)", common)]
    assert erf_side[0] == R.GELU_X0SQ and tuple(erf_side[1:]) == R.GELU_Q
    assert "|error| <= 8.3e-5 for the erf form" in common and R.GELU_POLY_ERR == 8.3e-5
    for src in (HEAD_SRC, HE_SRC, ENC_SRC):
        assert "gelu_poly4<false>" in src and "gelu_poly4<true>" not in src


def test_cases_reach_every_template_instance():
    """Each case names the launch forms it runs (its options through the restated dispatch); together they are every instance counted above.
    The one case without an option takes the 8-wave form by the default rule, at exactly the threshold."""
    reached = set()
    for c in R.HEAD_CASES + R.HEAD_ENC_CASES + R.ENC23_CASES:
        reached |= set(c.routes())
    assert reached == R.ALL_HEAD_ROUTES | R.ALL_HEAD_ENC_ROUTES | R.ALL_ENC23_ROUTES
    dflt = [c for c in R.HEAD_CASES if c.options == (0,)]
    assert len(dflt) == 1 and dflt[0].rows == R.HEAD_WIDE_ROWS and dflt[0].routes() == ["head<CB8,NWV8,ONE>"]
    assert all(c.rows <= 1152 for c in R.HEAD_CASES + R.HEAD_ENC_CASES + R.ENC23_CASES if c.options != (0,))
    ids = [c.id for c in R.HEAD_CASES + R.HEAD_ENC_CASES + R.ENC23_CASES]
    assert len(set(ids)) == len(ids)
    # the mechanisms of the list: ragged tiles, dead waves, straddled images, both grid blocks, every D class, every NDT, every output form
    for kind in ("one", "multi"):
        cs = [c for c in R.HEAD_CASES if c.kind == kind]
        assert {c.C for c in cs} == {128, 256} and {c.shape for c in cs} >= {R.S45, R.S147, R.S567, R.S1071}
    assert {c.D for c in R.HEAD_CASES} == {1, 3, 4, 5, 11, 16}
    one = [c for c in R.HEAD_CASES if c.kind == "one"]
    assert {c.n_out for c in one} == {1, 3, 8} and {c.last for c in one} == {"given", "null"} and {c.addr for c in one} == {"model", "padded", "odd"}
    assert any(c.out_gap for c in one) and any(c.last_pad for c in one)
    assert {c.n_ord for c in R.HEAD_CASES if c.kind == "multi"} == {1, 2, 3, 4}
    assert (R.S567[0] * R.S567[1] * R.S567[2] + 63) // 64 == 9 and (1071 + 127) // 128 == 9          # more than 8 groups: the second grid block
    for c in R.HEAD_CASES:
        if c.addr == "odd":
            a = c.address()
            assert 16 % a.a_n0 and (c.shape[1] * c.shape[2]) % a.a_n0
    assert {c.D for c in R.HEAD_ENC_CASES} == {1, 4, 5, 9, 16} and {c.n_ord for c in R.HEAD_ENC_CASES} == {1, 2, 3, 4}
    assert {c.shape for c in R.HEAD_ENC_CASES} == {(3, 4, 4), (3, 4, 12), (10, 8, 8), (18, 8, 8)}
    assert all((c.shape[1] * c.shape[2]) % 16 == 0 and c.address().a_n0 % 16 == 0 for c in R.HEAD_ENC_CASES)
    assert {(c.shape, c.T) for c in R.ENC23_CASES} == {((6, 5, 9), 3), ((2, 1, 1), 2), ((4, 8, 8), 4)}


def test_streams_hold_nan_outside_the_addressed_rows():
    """The stream buffers of every head case: the header's addressing formula finds exactly the token rows, everything else is NaN."""
    for c in R.HEAD_CASES + R.HEAD_ENC_CASES:
        inp = R.make_head_inputs(c)
        off = inp.addr.offsets(c.rows)
        idx = (off[:, None] + torch.arange(c.C)[None, :]).reshape(-1)
        assert int(idx.max()) < inp.addr.size and idx.unique().numel() == idx.numel(), c.id
        assert inp.addr.a_s0 % 4 == 0 and inp.addr.a_s1 % 4 == 0 and inp.addr.a_off % 4 == 0
        for X, buf in zip(inp.X, inp.streams):
            assert torch.equal(buf[idx].view(c.rows, c.C), X), c.id
            assert int(torch.isnan(buf).sum()) == buf.numel() - idx.numel(), c.id
            assert abs(float(X.std()) - 1.0) < 0.05


def test_weight_tile_swizzle_stays_inside_the_tile():
    """Every (row, chunk) of a head weight tile has a slot of its own inside the tile, at both widths.  (With 4 chunks per row -- W3 at
    C = 128 -- the swizzle of the 8-chunk rows gave chunk indices up to 7: rows 8 k + 7 and 8 k + 8 shared a slot and the last row lay
    on the bias block behind the tile, so C = 128 gave wrong derivatives for D >= 4; tests/test_hip_tail_enc.py found it at
    one-C128-D16-7x3x7-ord1-out1-acc.)  The restated swizzle is read from common.hip.h."""
    common = open(os.path.join(CSRC, "common.hip.h")).read()
    body = re.search(r"int swz_chunk\(int r, int c, int cpr\) \{(.*?)\n\}", common, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    assert re.sub(r"\s+", " ", body).strip() == "return (cpr >= 16) ? (c ^ (r & 15)) : (cpr >= 8) ? (c ^ ((r >> 1) & 7)) : (c ^ ((r >> 2) & 3));"
    assert "CPR1 = CB * 4, CPR2 = CB * 2, CPR3 = CB;" in HEAD_SRC and "*((u32x4*)base + (long)r * cpr + swz_chunk(r, c, cpr)) = o;" in HEAD_SRC
    for C in (128, 256):
        for rows, cpr in R.head_tiles(C):
            slots = sorted(r * cpr + R.swz_chunk(r, c, cpr) for r in range(rows) for c in range(cpr))
            assert slots == list(range(rows * cpr)), (C, rows, cpr)
            assert all(0 <= R.swz_chunk(r, c, cpr) < cpr for r in range(rows) for c in range(cpr))
    # a 16-lane read (rows 0..15, one chunk index) touches 16 distinct 16-byte slots of the 256-byte bank row at every width
    for cpr in (4, 8, 16, 32):
        for c in range(cpr):
            assert len({((r * cpr + R.swz_chunk(r, c, cpr)) * 16) % 256 for r in range(16)}) == 16, (cpr, c)


# ---- headroom and near misses ---------------------------------------------------------------------------------------------------------
def test_exact_bf16_headroom(evaluated):
    """On every case the exact-bf16 evaluation's own worst per-token error against float64 is at most half the per-token bar (and its
    whole-tensor figures at most half theirs): the bars leave a kernel room for its fp32 accumulation, not for a fault."""
    worst = {}

    def hold(key, cid, bf, ref):
        tok = R.worst_token(bf, ref)
        rel, mx = R.errors(bf, ref)
        assert tok <= 0.5 * R.BAR_TOKEN and rel <= 0.5 * R.BAR_L2 and mx <= 0.5 * R.BAR_MAX, (cid, tok, rel, mx)
        w = worst.setdefault(key, [1.0, 0.0])
        w[0], w[1] = min(w[0], tok), max(w[1], tok)
    for c in R.HEAD_CASES + R.HEAD_ENC_CASES:
        e = evaluated[c.id]
        hold(f"head {c.kind} C{c.C}", c.id, e["bf"], e["ref"])
        if c.kind == "head_enc":
            hold("head_enc z", c.id, e["z_bf"], e["z_ref"])
    for c in R.ENC23_CASES:
        for f in ("film", "frames"):
            ref, bf = evaluated[c.id][f]
            hold(f"enc23 {f}", c.id, bf, ref)
    print({k: (f"{v[0]:.2e}", f"{v[1]:.2e}") for k, v in sorted(worst.items())})


def _swap_subpixels(blk):
    """(.., D, 8, 8): sub-pixels (kh2, kw2) = (0, 0) and (0, 1) of stage-1 pixel (0, 0) exchanged."""
    out = blk.clone()
    out[..., 0:2, 0:2], out[..., 0:2, 2:4] = blk[..., 0:2, 2:4], blk[..., 0:2, 0:2]
    return out


def test_bars_reject_near_misses(evaluated):
    """Each fault of PLANTED, planted into the exact-bf16 result of the largest case of its kernel: the per-token bar rejects every one;
    which of them the whole-tensor bars of the model-level tests alone would have passed is measured and equals PLANTED.  The transposed
    sub-pixel order is the one-line mutation of the reference (head_blocks, bug = "subpixel_order"): against the mutated reference the
    unmutated result -- what a correct kernel gives -- fails every bar, so a kernel that disagrees with the reference about the order of a
    token's pixels cannot pass tests/test_hip_tail_enc.py."""
    seen = {}

    def head_fault(name, c, faulty, scale=1.0):
        e = evaluated[c.id]
        faulty, ref = faulty * scale, e["ref"] * scale
        tok = R.worst_token(faulty, ref)
        base = R.head_base_blocks(c, e["inp"])
        rel_o, mx_o = R.errors(base + faulty, base + ref)
        rel_d, mx_d = R.errors(faulty, ref)
        seen[name] = dict(token=tok, out=(rel_o, mx_o), der=(rel_d, mx_d), whole_passes=(rel_o < 1e-2 and rel_d < 2e-2, mx_o < 2e-2))

    def row_fault(name, faulty, ref):
        rel, mx = R.errors(faulty, ref)
        seen[name] = dict(token=R.worst_token(faulty, ref), out=(rel, mx), whole_passes=(rel < R.BAR_L2, mx < R.BAR_MAX))
    for kind in ("one", "multi"):
        c = _largest(R.HEAD_CASES, kind)
        bf = evaluated[c.id]["bf"]
        r = c.rows // 2 + 3
        f = bf.clone()
        f[:, r] = bf[:, r + 1]
        head_fault(f"head {kind}: a token gets its neighbour's block", c, f)
        if kind == "one":
            head_fault("head one, coefficients / 48: a token gets its neighbour's block", c, f, scale=1.0 / 48.0)
        f = bf.clone()
        f[:, r] = _swap_subpixels(bf[:, r])
        head_fault(f"head {kind}: two sub-pixels of one token swapped", c, f)
    c = _largest(R.HEAD_CASES, "multi")
    assert c.n_ord == 4
    co = [row[:] for row in c.coefs()]
    for row in co:
        row[1], row[2] = row[2], row[1]
    inp = evaluated[c.id]["inp"]
    head_fault("head multi: the coefficients of two orders exchanged", c, R.head_derivative(inp.X, inp.w, co, exact_bf16=True))
    # the one-line mutation: the kernel's stand-in against the MUTATED reference
    e = evaluated[c.id]
    mut = R.head_reference(c, inp, bug="subpixel_order")
    assert R.worst_token(e["bf"], mut) > 10 * R.BAR_TOKEN and R.errors(e["bf"], mut)[0] > 10 * R.BAR_L2
    head_fault("head (all tokens): stage 2's sub-pixel order transposed", c, R.head_reference(c, inp, exact_bf16=True, bug="subpixel_order"))
    # head_enc: z
    c = _largest(R.HEAD_ENC_CASES)
    e = evaluated[c.id]
    r = c.rows // 2 + 3
    f = e["z_bf"].clone()
    f[r] = e["z_bf"][r + 1]
    row_fault("head_enc z: a token gets its neighbour's row", f, e["z_ref"])
    ch = int(e["inp"].we[5].abs().argmax())
    row_fault("head_enc z: the stage-3 bias of one channel dropped", R.encoder_rows(e["frame"], e["inp"].we, exact_bf16=True, bug=("bias3", ch)),
              e["z_ref"])
    # enc23
    c = _largest(R.ENC23_CASES)
    e = evaluated[c.id]
    inp = e["inp"]
    ref, bf = e["film"]
    f = bf.clone()
    f[r % c.rows] = bf[r % c.rows + 1]
    row_fault("enc23 film: a token gets its neighbour's row", f, ref)
    ch = int((inp.w[3].abs() * inp.film_a.abs().min(0).values).argmax())
    row_fault("enc23 film: the stage-3 bias of one channel dropped", R.enc23_reference(c, inp, "film", True, bug=("bias3", ch)), ref)
    row_fault("enc23 film: the FiLM row of slot t + 1", R.enc23_reference(c, inp, "film", True, bug="film_t+1"), ref)
    ref, bf = e["frames"]
    ch = int(inp.w[3].abs().argmax())
    row_fault("enc23 frames: the stage-3 bias of one channel dropped", R.enc23_reference(c, inp, "frames", True, bug=("bias3", ch)), ref)
    row_fault("enc23 frames: two images swapped in the frame-major order", R.enc23_reference(c, inp, "frames", True, bug=("swap", (1, 2))), ref)
    for k, v in seen.items():
        print(k, {a: (f"{b:.2e}" if isinstance(b, float) else tuple(f"{x:.2e}" for x in b) if isinstance(b, tuple) else b) for a, b in v.items()})
    assert set(seen) == set(PLANTED)
    for k, v in seen.items():
        assert v["token"] > R.BAR_TOKEN, (k, v)
    assert {k: v["whole_passes"] for k, v in seen.items()} == PLANTED
