"""CPU: tante_amd/model_shell.py alone, on two-line stub modules -- the training gate's truth table under the shared inference-only policy
and under AFNO's, the opt-in's reach, the compute switch, the device gate and the per-site compute rule.  No library call."""
import contextlib
import itertools

import pytest
import torch
import torch.nn as nn

from tante_amd import _lib as L
from tante_amd import model_shell as MS

WHY = "the backward is not built"
SHARED_TEXT = f"tante_amd.Stub is inference only: training is out of scope ({WHY}); call .eval() under torch.no_grad()"
AFNO_TEXT = ("tante_amd.AFNO is inference only unless set_trainable() was called: training is out of scope for this model as it stands; "
             "opt in, or call it in eval mode under torch.no_grad()")


class Leaf(MS.Trainable, nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(2))


class Tree(MS.Trainable, MS.ComputeSwitch, nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b, self.plain = Leaf(), nn.Sequential(Leaf(), Leaf()), nn.Linear(2, 2)


def shared_refuse(module):
    MS.inference_only(module, "Stub", WHY)


def expected(policy, opted, grad, training, p_grad, x_grad):
    """The bool the gate returns, or the text it raises with, restated from the two policies' descriptions."""
    if opted:
        return grad and (p_grad or x_grad)
    if policy == "shared":
        return SHARED_TEXT if training or (grad and p_grad) else False
    return AFNO_TEXT if grad and p_grad else False


@pytest.mark.parametrize("policy", ["shared", "afno"])
def test_wants_graph_truth_table(policy):
    import tante_amd.afno as A
    refuse = shared_refuse if policy == "shared" else A._refuse
    seen = set()
    for opted, grad, training, p_grad, x_grad in itertools.product([False, True], repeat=5):
        m = Leaf().train(training).set_trainable(opted)
        m.w.requires_grad_(p_grad)
        x = torch.zeros(2, requires_grad=x_grad)
        want = expected(policy, opted, grad, training, p_grad, x_grad)
        with torch.enable_grad() if grad else torch.no_grad():
            if isinstance(want, str):
                with pytest.raises(NotImplementedError) as e:
                    MS.wants_graph(m, x, refuse)
                assert str(e.value) == want
            else:
                got = MS.wants_graph(m, x, refuse)
                assert got is want, (opted, grad, training, p_grad, x_grad)
        seen.add(want)
    assert seen == {True, False, SHARED_TEXT if policy == "shared" else AFNO_TEXT}


def test_wants_graph_takes_a_module_without_the_mixin_as_not_opted_in():
    m = nn.Linear(2, 2).eval()
    with torch.no_grad():
        assert MS.wants_graph(m, torch.zeros(2), shared_refuse) is False
    with pytest.raises(NotImplementedError) as e:
        MS.wants_graph(m, torch.zeros(2), shared_refuse)
    assert str(e.value) == SHARED_TEXT


def test_set_trainable_reaches_nested_children_and_not_siblings():
    t = Tree()
    keys = set(t.state_dict())
    leaves = [t.a, t.b[0], t.b[1]]
    assert not t._trainable and not any(c._trainable for c in leaves)
    assert t.set_trainable() is t and t._trainable and all(c._trainable for c in leaves)
    assert set(t.state_dict()) == keys and "_trainable" not in dict(t.named_buffers())
    assert not hasattr(t.plain, "_trainable") and not hasattr(t.b, "_trainable")
    assert t.set_trainable(False) is t and not t._trainable and not any(c._trainable for c in leaves)
    assert t.b[0].set_trainable() is t.b[0] and t.b[0]._trainable
    assert not t._trainable and not t.a._trainable and not t.b[1]._trainable
    assert t.b[0].set_trainable(0)._trainable is False


def test_set_compute_modes_and_refusal():
    t = Tree()
    assert t.compute is None and "compute" not in t.state_dict()
    for mode in ("fp32", "bf16", None):
        assert t.set_compute(mode) is t and t.compute == mode
    for bad in ("fp16", "", 16, L.BF16 + 100):
        with pytest.raises(ValueError) as e:
            t.set_compute(bad)
        assert str(e.value) == "compute must be None, 'fp32' or 'bf16'"
    assert t.compute is None and Tree().compute is None


@pytest.mark.parametrize("name", ["AFNO", "DPOT", "AViT", "UNetConvNext", "AttentionUNet", "UNO"])
def test_gpu_only_names_the_model(name):
    with pytest.raises(RuntimeError) as e:
        MS.gpu_only(torch.zeros(1), name)
    assert str(e.value) == f"tante_amd.{name} runs on the GPU only (no CPU fallback); move the model and its input to cuda"


@pytest.mark.parametrize("module,model", [("dpot", "DPOT"), ("avit", "AViT"), ("convnext", "UNetConvNext"), ("unet_att", "AttentionUNet"),
                                          ("uno", "UNO")])
def test_inference_only_texts_of_the_five_models(module, model):
    """The sentence is assembled from the model's own reason; train() refuses under no_grad, eval() under grad with a parameter that
    requires one, and eval() under no_grad passes."""
    import importlib
    why = importlib.import_module("tante_amd." + module).WHY_INFERENCE_ONLY
    want = f"tante_amd.{model} is inference only: training is out of scope ({why}); call .eval() under torch.no_grad()"
    m = Leaf()
    for training, scope in ((True, torch.no_grad()), (False, contextlib.nullcontext())):
        with scope, pytest.raises(NotImplementedError) as e:
            MS.inference_only(m.train(training), model, why)
        assert str(e.value) == want
    with torch.no_grad():
        MS.inference_only(m.eval(), model, why)
    m.w.requires_grad_(False)
    MS.inference_only(m.eval(), model, why)


def test_site_passes_a_listed_group_and_forces_fp32_for_the_rest():
    sites = ("block", "skip")
    for compute in (L.F32, L.BF16):
        assert MS.site(compute, "block", sites) == compute and MS.site(compute, "skip", sites) == compute
        assert MS.site(compute, "head", sites) == L.F32 and MS.site(compute, "block", ()) == L.F32


def test_layout_helpers():
    x = torch.arange(2 * 3 * 4 * 5, dtype=torch.float64).reshape(2, 3, 4, 5).requires_grad_(True)
    y = MS.to_nhwc(x)
    assert y.dtype == torch.float32 and y.is_contiguous() and not y.requires_grad and tuple(y.shape) == (2, 4, 5, 3)
    assert torch.equal(y, x.detach().float().permute(0, 2, 3, 1))
    back = MS.to_nchw(y, x)
    assert back.dtype == torch.float64 and back.is_contiguous() and torch.equal(back, x.detach())
