"""The host-side shell every model file shares: the device and inference-only gates, the training opt-in, the compute-mode switch, the
per-site compute rule and the two layout helpers.  Plain functions and two mixins; nothing here launches a kernel."""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from . import kernels as K


def gpu_only(x: torch.Tensor, model: str):
    if not x.is_cuda:
        raise RuntimeError(f"tante_amd.{model} runs on the GPU only (no CPU fallback); move the model and its input to cuda")


def inference_only(module: nn.Module, model: str, why: str):
    """Refuse train() mode, and grad mode with a parameter that requires a gradient; `why` names the backward kernels that are not built."""
    if module.training or (torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters())):
        raise NotImplementedError(f"tante_amd.{model} is inference only: training is out of scope ({why}); call .eval() under torch.no_grad()")


class Trainable:
    """The training opt-in of a module whose forward can build an autograd graph; mix in before nn.Module."""

    _trainable = False

    def set_trainable(self, flag: bool = True):
        """Opt in to (or out of) training: under grad, forward then builds an autograd graph instead of refusing.  Not a constructor
        argument and not part of the state_dict; propagates to the children and returns self."""
        for m in self.modules():
            if isinstance(m, Trainable):
                m._trainable = bool(flag)
        return self


def wants_graph(module: nn.Module, x: torch.Tensor, refuse: Callable[[nn.Module], None]) -> bool:
    """True: build the autograd graph (opted in through set_trainable, grad enabled, something to differentiate).  A module that has not
    opted in is handed to the model's own `refuse`, which raises as that model always did or returns; an opted-in one takes the inference
    path under no_grad, in train() as in eval()."""
    if not getattr(module, "_trainable", False):
        refuse(module)
        return False
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


class ComputeSwitch:
    """The compute mode of a model: None follows torch.autocast, 'fp32' / 'bf16' pin it."""

    compute: Optional[str] = None

    def set_compute(self, mode: Optional[str]):
        if mode is not None and mode not in K.COMPUTE:
            raise ValueError("compute must be None, 'fp32' or 'bf16'")
        self.compute = mode
        return self


def site(compute: int, name: str, sites: Sequence[str]) -> int:
    """The compute mode of one GEMM group: the caller's for the groups in `sites` (the model's BF16_SITES), fp32 for the rest."""
    return compute if name in sites else L.F32


def to_nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()


def to_nchw(y: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return y.permute(0, 3, 1, 2).contiguous().to(like.dtype)
