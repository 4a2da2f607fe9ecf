"""Fused loss+grad: the CPU emulation (the kernel's rounding points in fp32)
against float64 autograd through the same net with the same roundings."""
import pytest
import torch

from shifu_amd.models.mlp import ShifuMLP
from shifu_amd.ops.fused_mlp import (GRAD_LDS_LIMIT, _grad_lds_bytes, _shapes_of,
                                     fused_grad_eligible, fused_loss_and_grad)
from shifu_amd.ops.linear import _act_fwd_ref, _act_grad_from_y_ref

NETS = [([16], ["tanh"]), ([50, 50], ["tanh", "tanh"]),
        ([33, 17], ["sigmoid", "leakyrelu"]), ([24, 8], ["relu", "relu"])]
KINDS = ["weighted_mse", "sigmoid_ce"]


def _r(t):                      # bf16 rounding of a float64 tensor
    return t.float().to(torch.bfloat16).double()


class _Round(torch.autograd.Function):
    """bf16 rounding with a straight-through gradient (input and weights)."""
    @staticmethod
    def forward(ctx, t):
        return _r(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _Act(torch.autograd.Function):
    """H = bf16(act(Z)); backward dZ = bf16(dH * act'(H)) from the rounded H."""
    @staticmethod
    def forward(ctx, z, act):
        h = _r(_act_fwd_ref(z, act))
        ctx.save_for_backward(h)
        ctx.act = act
        return h

    @staticmethod
    def backward(ctx, g):
        return _r(_act_grad_from_y_ref(g, ctx.saved_tensors[0], ctx.act)), None


class _RoundGrad(torch.autograd.Function):
    """identity whose gradient (dlogit) is rounded to bf16"""
    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return _r(g)


def reference_f64(model, dense, target, weight, kind):
    """(loss, [(dW, db), ...]) in float64.  The count division is applied
    after the backward pass, as the kernel's reduce step does."""
    layers = list(model.hidden) + [model.shifu_output_0]
    ws = [l.weight.detach().double().requires_grad_() for l in layers]
    bs = [l.bias.detach().double().requires_grad_() for l in layers]
    x = _r(dense.double())
    for l, w, b in zip(layers[:-1], ws, bs):
        x = _Act.apply(x @ _Round.apply(w).t() + b, l._act)
    z = _RoundGrad.apply((x @ _Round.apply(ws[-1]).t() + bs[-1]).reshape(-1))
    y, sw = target.double(), weight.double()
    if kind == "weighted_mse":
        total = (sw * (torch.sigmoid(z) - y) ** 2).sum()
    else:
        total = (sw * torch.nn.functional.binary_cross_entropy_with_logits(
            z, y, reduction="none")).sum()
    total.backward()
    cnt = (sw != 0).double().sum().clamp_min(1e-12)
    return total.detach() / cnt, [(w.grad / cnt, b.grad / cnt) for w, b in zip(ws, bs)]


def make_case(k0, hidden, acts, b, seed=0):
    g = torch.Generator().manual_seed(seed)
    model = ShifuMLP(k0, hidden, acts, seed=7)
    for p in model.parameters():            # nonzero biases
        if p.dim() == 1:
            p.data = torch.randn(p.shape, generator=g) * 0.1
    dense = torch.randn(b, k0, generator=g)
    target = (torch.rand(b, generator=g) > 0.5).float()
    weight = torch.ones(b)
    weight[2::5] = 0.0
    weight[-1] = 0.375
    return model, dense, target, weight


def rel_err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hidden,acts", NETS)
def test_emulation_matches_float64(hidden, acts, kind):
    k0, b = 37, 70
    model, dense, target, weight = make_case(k0, hidden, acts, b)
    loss, grads = fused_loss_and_grad(model, dense, target, weight, kind)
    ref_loss, ref = reference_f64(model, dense, target, weight, kind)
    # fp32 round-off: worst case n * 2^-24 for an n-term fp32 sum, n <= 70 here,
    # through forward, dgrad and wgrad (3 chained sums) -> 3 * 70 * 2^-24
    tol = 3 * max(k0, b) * 2.0 ** -24
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert abs(float(loss) - float(ref_loss)) <= tol * abs(float(ref_loss))
    for (dw, db), (rw, rb), n in zip(grads, ref, hidden + [1]):
        assert dw.shape == rw.shape and db.shape == (n,)
        assert rel_err(dw, rw) <= tol, rel_err(dw, rw)
        assert rel_err(db, rb) <= tol, rel_err(db, rb)


def test_eligibility():
    default = ShifuMLP(200, [50, 50], ["tanh", "tanh"])
    assert fused_grad_eligible(default) == (True, "")
    assert _grad_lds_bytes(_shapes_of(default)) <= GRAD_LDS_LIMIT
    ok, why = fused_grad_eligible(ShifuMLP(200, [96, 96], ["relu", "relu"]))
    assert not ok and "row staging" in why     # fits the scoring kernel, not this one
    ok, why = fused_grad_eligible(ShifuMLP(600, [16], ["relu"]))
    assert not ok and "input width" in why
    with pytest.raises(ValueError, match="not eligible"):
        fused_loss_and_grad(ShifuMLP(600, [16], ["relu"]), torch.zeros(2, 600),
                            torch.zeros(2), torch.ones(2))


def test_autograd_surface_accumulates_scaled_grads():
    model, dense, target, weight = make_case(37, [16], ["tanh"], 20)
    _, grads = fused_loss_and_grad(model, dense, target, weight)
    for _ in range(2):                      # two backward passes accumulate
        (model.fused_loss(dense, target, weight) * 0.5).backward()
    assert torch.allclose(model.hidden[0].weight.grad, grads[0][0])
    assert torch.allclose(model.shifu_output_0.bias.grad, grads[1][1])
