"""Host side of the flash attention kernels (csrc/attn_flash.hip): which kernel takes which attention call, and the two launches.

By default the flash kernels take ONLY the calls the older kernels refuse; every call that worked before keeps its kernel and its bits:

  forward (training, AttentionFn.forward)     p > 0, L > 256                  flash            (was refused)
                                              p > 0, L <= 256                 tante_attention_dropout
                                              p = 0                           tante_attention  [flash when TANTE_ATTN_FLASH and L > 256]
  forward (inference, K.attention)            any L                           tante_attention  [flash when TANTE_ATTN_FLASH and L > 256]
  backward (AttentionFn.backward)             L <= 128                        tante_attention_bwd
                                              L > 128, p > 0                  flash            (was refused)
                                              L > 128, p = 0, strided         flash            (was refused)
                                              L > 128, p = 0, dense           tante_attention_masked_bwd  [flash when TANTE_ATTN_FLASH]

The bracketed routes need a shape the flash kernels support (head dim 32); the unbracketed flash routes are taken whatever the shape, so
that an unsupported one fails with tante_attention_flash's message instead of the older kernels' "not yet".  When the backward is the
flash one but the forward was not (128 < L <= 256 with dropout, or p = 0), the backward RECOMPUTES the row statistics: it runs the flash
forward once into scratch (same seed, so the same mask) and differentiates that.

Masked attention (attn_mask / key_padding_mask on dense sequences; masked_route):

  forward and backward                        p > 0                           flash, masked    (no other kernel has masks with dropout)
                                              p = 0, L > 128                  tante_attention_masked(_bwd)  [flash, masked, when TANTE_ATTN_FLASH]
                                              p = 0, L <= 128                 tante_attention_masked(_bwd)
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import options

# 1: also route the calls that work without them to the flash kernels (inference past 256 tokens, the dense p = 0 backward past 128) -- an
# A/B switch for tools/attn_flash_ab.py and the parity tests; the default keeps every existing call on its kernel
ATTN_FLASH = options.register("TANTE_ATTN_FLASH", 0, __name__, "ATTN_FLASH")

FWD_FLASH, FWD_DROPOUT, FWD_PLAIN = "flash", "attention_dropout", "attention"
BWD_FLASH, BWD_MFMA, BWD_MASKED = "flash_bwd", "attention_bwd", "attention_masked_bwd"
MASKED_FLASH, MASKED_LANES = "flash_masked", "attention_masked"      # one route for a masked call's forward and backward
HEAD_DIMS = (32,)
_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16}


def supported(dtype: int, C_: int, n_head: int, Lq: int) -> bool:
    """Mirror of tante_attention_flash_supported (pure: no library call)."""
    return dtype in (L.F32, L.BF16) and n_head > 0 and C_ > 0 and C_ % n_head == 0 and C_ // n_head in HEAD_DIMS and Lq >= 1


def seq_is_dense(q) -> bool:
    """token(s, l) = s L + l: the sequences tante_attention_masked_bwd addresses."""
    return q.n_s0 == 1 and q.S1 == q.L and q.n_l0 >= q.L and q.P0 == 1


def forward_route(Lq: int, p: float, ok: bool, flash_opt: int = 0) -> str:
    """Kernel of an attention forward.  ok = supported(...); flash_opt = the TANTE_ATTN_FLASH switch."""
    if p > 0.0:
        return FWD_FLASH if Lq > 256 else FWD_DROPOUT
    return FWD_FLASH if (flash_opt and ok and Lq > 256) else FWD_PLAIN


def backward_route(Lq: int, p: float, dense: bool, ok: bool, flash_opt: int = 0) -> str:
    """Kernel of an attention backward."""
    if Lq <= 128:
        return BWD_MFMA
    if p > 0.0 or not dense:
        return BWD_FLASH
    return BWD_FLASH if (flash_opt and ok) else BWD_MASKED


def masked_route(Lq: int, p: float, ok: bool, flash_opt: int = 0) -> str:
    """Kernels of an attention call with attn_mask / key_padding_mask (forward and backward alike)."""
    if p > 0.0:
        return MASKED_FLASH      # whatever the shape: an unsupported one fails with the flash kernels' message
    return MASKED_FLASH if (flash_opt and ok and Lq > 128) else MASKED_LANES


def _stream():
    return torch.cuda.current_stream().cuda_stream


def new_stats(qkv: torch.Tensor, n_head: int, seq) -> torch.Tensor:
    return torch.empty(max(int(L.lib().tante_attention_flash_stats_floats(n_head, C.byref(seq))), 2), dtype=torch.float32, device=qkv.device)


def _mask_args(who: str, qkv, Lq: int, attn_mask, key_padding_mask):
    """(attn_mask pointer, stride, key_padding_mask pointer) of the additive fp32 masks TransformerBlock._masks builds."""
    for t in (attn_mask, key_padding_mask):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"attn_flash.{who}: masks must be contiguous float32 GPU tensors (additive; -inf blocks)")
    stride = 0 if attn_mask is None or attn_mask.shape[0] == 1 or attn_mask.dim() == 2 else Lq * Lq
    return (attn_mask.data_ptr() if attn_mask is not None else None, stride,
            key_padding_mask.data_ptr() if key_padding_mask is not None else None)


def forward(qkv: torch.Tensor, o: torch.Tensor, stats, C_: int, n_head: int, seq, causal: bool, p: float = 0.0, seed: int = 0,
            attn_mask=None, key_padding_mask=None):
    """attn_mask (1, L, L) | (L, L) | (nseq n_head, L, L) and key_padding_mask (nseq, L): additive float32, dense `seq` only."""
    if not (qkv.is_cuda and o.is_cuda and (stats is None or stats.is_cuda)) or qkv.dtype != o.dtype or qkv.dtype not in _DT:
        raise RuntimeError("attn_flash.forward: qkv and o must be GPU tensors of one dtype (float32 or bfloat16)")
    if attn_mask is not None or key_padding_mask is not None:
        if not seq_is_dense(seq):
            raise RuntimeError("attn_flash.forward: masks need a dense sequence (token = s L + l)")
        am, stride, kp = _mask_args("forward", qkv, seq.L, attn_mask, key_padding_mask)
        L.check(L.lib().tante_attention_flash_masked(qkv.data_ptr(), o.data_ptr(), stats.data_ptr() if stats is not None else None, _DT[qkv.dtype],
                                                     C_, n_head, seq.nseq, seq.L, int(causal), am, stride, kp, float(p), int(seed), _stream()),
                "tante_attention_flash_masked")
        return o
    L.check(L.lib().tante_attention_flash(qkv.data_ptr(), o.data_ptr(), stats.data_ptr() if stats is not None else None, _DT[qkv.dtype], C_, n_head,
                                          C.byref(seq), int(causal), float(p), int(seed), _stream()), "tante_attention_flash")
    return o


def backward(qkv: torch.Tensor, o: torch.Tensor, do: torch.Tensor, stats: torch.Tensor, dqkv: torch.Tensor, C_: int, n_head: int, seq,
             causal: bool, p: float = 0.0, seed: int = 0, attn_mask=None, key_padding_mask=None):
    if not all(t.is_cuda for t in (qkv, o, do, stats, dqkv)) or not (qkv.dtype == o.dtype == do.dtype == dqkv.dtype) or qkv.dtype not in _DT:
        raise RuntimeError("attn_flash.backward: qkv, o, dO and dqkv must be GPU tensors of one dtype (float32 or bfloat16), stats a GPU tensor")
    if attn_mask is not None or key_padding_mask is not None:
        if not seq_is_dense(seq):
            raise RuntimeError("attn_flash.backward: masks need a dense sequence (token = s L + l)")
        am, stride, kp = _mask_args("backward", qkv, seq.L, attn_mask, key_padding_mask)
        L.check(L.lib().tante_attention_flash_masked_bwd(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), stats.data_ptr(), dqkv.data_ptr(),
                                                         _DT[qkv.dtype], C_, n_head, seq.nseq, seq.L, int(causal), am, stride, kp, float(p),
                                                         int(seed), _stream()), "tante_attention_flash_masked_bwd")
        return dqkv
    L.check(L.lib().tante_attention_flash_bwd(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), stats.data_ptr(), dqkv.data_ptr(), _DT[qkv.dtype], C_,
                                              n_head, C.byref(seq), int(causal), float(p), int(seed), _stream()), "tante_attention_flash_bwd")
    return dqkv
