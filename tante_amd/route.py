"""Which kernels an inference call takes: ONE record, planned once per call (TANTE.forward) and read by name -- what
train_forward.BlockPlan is for a training block.  plan_route answers for a model call, plan_rollout for the loop around the calls
(rollout.py); the public predicates of TANTE read the helpers both share, so the two sides cannot disagree.  Everything here is pure:
no device is touched, the library is asked through its *_supported entries only, and nothing is cached across calls (the answer
depends on the compute mode, the switches, the blocks' .fused flags, the grad mode and parameter alignment)."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

from . import _lib as L
from . import kernels as K


class Route(NamedTuple):
    """One inference call of TANTE."""
    source: str        # the token stream comes from: "encoder" | "cache_fused" (frame cache, the first propagator applies FiLM on load)
    #                    | "cache_film_pass" (frame cache + tante_film_pos_fwd_frames) | "cache_film_vp" (frame cache, FiLM inside the
    #                    vertical propagator's launch: film_frames)
    tail: str          # "adaptive" (adaptive_rt, head_adaptive) | "head_enc" (head_enc_fused) | "head_multi" (head_fused_multi)
    #                    | "head_per_order" (one head_fused per order) | "decoders" (decoders, then taylor) | "unfused" (the deg=False chain)
    streams: bool      # orders after the first write stream buffers of their own; False: the last-slot rows are copied aside
    last_slot: bool    # the last order's backbone runs with last_slot_only
    n_cap: int         # frame cap of the adaptive tail, else 0
    heads: bool        # the fused head kernel serves this model ("unfused" uses it once the frame count is known; the other tails imply it)


class RolloutRoute(NamedTuple):
    """The loop around the calls of one rollout."""
    first: str         # the first window arrives by: "raw" (encode_window_raw on the channels-last batch) | "format" (tante_format_input)
    #                    | "copy" (the formatted window is copied in)
    cache: bool        # every frame is encoded once; the calls read the frame cache (enc_cache=)
    tail_enc: bool     # the tail launch of a call also writes the predicted frame's encoding (enc_next=)


def stages_2x2(mod) -> bool:
    """`mod` (an encoder or a decoder) is the three 2 x 2 stages of patch_scale 8 without overlap: the one geometry the fused encoder,
    head and tail kernels are written for."""
    return getattr(mod, "P", None) == (2, 2, 2) and mod.overlap == 0.0


def own_streams(model, compute: int) -> bool:
    """Every backbone after the first can write a stream buffer of its own (its first launch runs out of place), so the earlier orders'
    streams stay intact for the head."""
    return all(b.takes_x_in(compute) for b in model.blocks[1:model.taylor_order])


def taylor_coefs(dt, k: int, n: int) -> list:
    """Order k's weights in the Taylor sum of frames j = 1 .. n: (j dt)^(k+1) / (k+1)!   (tante.py:165-171)."""
    return [(j * dt) ** (k + 1) / math.factorial(k + 1) for j in range(1, n + 1)]


def fused_heads(model, compute: int) -> bool:
    return bool(compute == L.BF16 and model.fused_head and stages_2x2(model.decoders[0]) and K.head_fused_supported(model.C, model.D))


def tail_fused(model, compute: int, head_enc: bool) -> bool:
    """Every order's head, the Taylor sum and the re-encoding of the predicted frame as ONE launch (csrc/head_enc.hip): bf16, C = 256,
    one output frame, at most four orders, each with a stream of its own."""
    return bool(head_enc and model.deg and model.output_length == 1 and 1 <= model.taylor_order <= 4 and compute == L.BF16 and model.fused_head
                and type(model.encoder).__name__ == "enc_CNN" and stages_2x2(model.decoders[0])
                and K.head_enc_supported(model.C, model.D, model.H_p, model.W_p) and own_streams(model, compute))


def adaptive_cap(model, compute: int, out_T, adaptive_tail: bool) -> int:
    """n_cap = floor(out_T - 1 + ep) when a deg=False call with this out_T takes the adaptive tail (csrc/adaptive_tail.hip), else 0."""
    if model.deg or not adaptive_tail or compute != L.BF16 or not model.fused_head or not stages_2x2(model.decoders[0]):
        return 0
    ep = model.interprators[0].ep
    if any(ip.ep != ep for ip in model.interprators):
        return 0
    n_cap = K.adaptive_n_cap(out_T, ep)
    return n_cap if K.adaptive_tail_supported(model.C, model.D, model.H_p, model.W_p, model.taylor_order, n_cap) else 0


def cache_source(model, compute: int, B: Optional[int] = None) -> Optional[str]:
    """How a call reads the rollout's frame cache (Route.source), None where the model has none.  Without B the two spectral forms are
    not told apart ("cache_film_pass")."""
    enc = type(model.encoder).__name__
    Hp, Wp, C_ = model.H_p, model.W_p, model.C
    if enc == "enc_CNN":
        return "cache_fused" if model.encoder.fuses_23(compute) and K.axis_hw_supported(Hp, Wp, C_) else None
    if enc != "enc_FNO" or C_ != 256 or not 1 <= model.T <= 8:      # enc_FNO is per frame too (enc_dec_fno.py:224-273)
        return None
    vp = model.blocks[0].vertical_propagator
    # planes too large for the whole-plane kernel: the vertical propagator applies FiLM + the positional terms while it loads its tiles
    # (the FiLM tables are fresh allocations, always aligned; the parameters may have been loaded at any address)
    if (B is not None and compute == L.BF16 and not K.axis_hw_supported(Hp, Wp, C_, compute)
            and L.lib().tante_axis_mlp_film_supported(B, model.T, Hp, Wp * C_, C_)
            and all(q.data_ptr() % 16 == 0 for q in (vp[0].weight, vp[0].bias, vp[2].weight, vp[2].bias, model.s_emb))):
        return "cache_film_vp"
    return "cache_film_pass"


def plan_route(model, compute: int, out_T, cache: bool, enc_next: bool, grad: bool, B: int, *, head_multi: bool, head_streams: bool,
               head_enc: bool, last_slot: bool, adaptive_tail: bool) -> Route:
    """The route of model(x[B], out_T, enc_cache= given or not, enc_next= given or not) under `compute`, the grad mode and the host
    switches.  Raises where the call asks for a cache or a re-encoding this model has no path for."""
    n_ord, heads = model.taylor_order, fused_heads(model, compute)
    n_cap = adaptive_cap(model, compute, out_T, adaptive_tail)
    streams = False
    if n_cap:
        tail, streams = "adaptive", own_streams(model, compute)
    elif not model.deg:
        tail = "unfused"
    elif tail_fused(model, compute, head_enc):
        tail, streams = "head_enc", True
    elif heads and model.output_length == 1 and 2 <= n_ord <= 4 and head_multi:
        tail, streams = "head_multi", head_streams and own_streams(model, compute)
    else:
        tail = "head_per_order" if heads else "decoders"
    source = "encoder"
    if cache:      # deg=False: only the adaptive tail reads the cache
        source = cache_source(model, compute, B) if (model.deg or n_cap) else None
        if source is None:
            raise RuntimeError("enc_cache: this model / compute mode has no frame-encoding cache path")
    if enc_next and not (tail == "head_enc" and model.encoder.fuses_23(compute)):
        raise RuntimeError("enc_next: this model / compute mode has no fused head + re-encoding path (tail_fused_supported())")
    # the last order's stream is read at slot T - 1 only, by the one head launch: its backbone may leave the other slots unfinished
    return Route(source, tail, streams, last_slot and tail in ("head_enc", "head_multi") and not grad, n_cap, heads)


def plan_rollout(model, compute: int, raw=None, out_T=None, *, raw_encode: bool, no_enc_cache: bool, no_tail_enc: bool,
                 no_fused_format: bool) -> RolloutRoute:
    """The loop of rollout_model (out_T None) or of the in-place adaptive rollout (out_T given) under the rollout switches.  raw: the
    (B, T, H, W, D) channels-last batch when the default formatter's input pass may be fused into the loop, else None."""
    cache = bool(not no_enc_cache and model.enc_cache_supported(out_T))
    tail_enc = bool(cache and not no_tail_enc and model.output_length == 1 and model.tail_fused_supported())
    first = "copy"
    if raw is not None and not no_fused_format:
        # the raw encode needs the fused frame cache, 4 D <= 64 and a 16-byte aligned batch of whole 8 x 8 patches
        first = "raw" if (raw_encode and cache and cache_source(model, compute) == "cache_fused" and model.encoder.raw_window_supported(compute)
                          and raw.data_ptr() % 16 == 0 and raw.shape[2] % 8 == 0 and raw.shape[3] % 8 == 0) else "format"
    return RolloutRoute(first, cache, tail_enc)
