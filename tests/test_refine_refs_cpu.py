"""The float64 references of latent refinement (tests/refine_refs.py) against torch itself: the
rate derivative against autograd of the oracle's bits function, the Adam update against
torch.optim.Adam, the masked distortion gradient against a torch expression. No GPU."""
import numpy as np
import pytest
import torch

import refine_refs as F
import step_refs as S


@pytest.mark.parametrize("shape", F.STEP_SHAPES)
def test_rate_derivative_is_autograd_of_the_bits(shape):
    c = F.step_case(shape)
    d = S.deltas(F.STEP_INDICES, torch.float64)
    z = torch.round(c["y"].double() / d).requires_grad_(True)
    F.bits_of(z, c["rate"], d).sum().backward()
    got = F.dbits_dz(z.detach(), c["rate"], d)
    err = ((got - z.grad).abs().max() / z.grad.abs().max()).item()
    print(f"dbits/dz {shape}: {err:.2e} from float64 autograd")
    assert err <= 1e-12


def test_three_adam_steps_are_torch_optim_adam():
    torch.manual_seed(0)
    p0 = torch.randn(5, 7, dtype=torch.float64)
    grads = [torch.randn(5, 7, dtype=torch.float64) * s for s in (1.0, 0.01, 30.0)]
    lr = 0.05 * 1.4142135381698608
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t, g in enumerate(grads, start=1):
        q.grad = g.clone()
        opt.step()
        p, m, v = F.adam_step(p, g, m, v, lr, t)
        state = opt.state[q]
        assert torch.allclose(p, q.detach(), rtol=1e-14, atol=1e-15), t
        assert torch.allclose(m, state["exp_avg"], rtol=1e-14, atol=0.0), t
        assert torch.allclose(v, state["exp_avg_sq"], rtol=1e-14, atol=0.0), t


def test_masked_distortion_gradient():
    """Against ∂/∂recon of Σ_b wt_b·Σ_{inside b} (recon − ref/255)², by autograd; exact zeros on the
    padding."""
    rng = np.random.default_rng(3)
    refs = [rng.integers(0, 256, (17, 33, 3), dtype=np.uint8),
            rng.integers(0, 256, (32, 48, 3), dtype=np.uint8)]
    wt = torch.tensor([216.75, 3.0], dtype=torch.float64)
    recon = torch.rand(2, 3, 32, 48, dtype=torch.float64, requires_grad=True) * 1.4 - 0.2
    recon = recon.detach().requires_grad_(True)
    loss = 0
    for b, im in enumerate(refs):
        H, W = im.shape[:2]
        x = torch.from_numpy(im).permute(2, 0, 1).double() / 255
        loss = loss + wt[b] * ((recon[b, :, :H, :W] - x) ** 2).sum()
    loss.backward()
    got = F.grad_recon(recon.detach(), refs, wt)
    assert torch.allclose(got, recon.grad, rtol=1e-14, atol=0.0)
    assert bool((got[0, :, 17:, :] == 0).all()) and bool((got[0, :, :, 33:] == 0).all())


def test_iteration_rounds_half_to_even_and_scales_lr_by_the_step():
    d = S.deltas((5, 12), torch.float64)
    y = torch.tensor([0.5, 1.5, -2.5, 7.0], dtype=torch.float64).view(1, 4, 1, 1).repeat(2, 1, 1, 1) * d
    zero = torch.zeros_like(y)
    g = torch.ones_like(y)
    out = F.latent_iteration(zero, zero, y, zero, zero, d, None, 0.05, 1, g=g)
    # step 1 of Adam moves every element by −lr·Δ·g/(|g| + ε·√(1 − β2)…) ≈ −lr·Δ
    assert torch.allclose((out["y"] - y) / d, torch.full_like(y, -0.05), rtol=1e-6)
    q = torch.round(out["y"] / d)
    assert torch.equal(out["y_hat"], q) and torch.equal(out["y_deq"], d * q)
    assert F.objective(10.0, 65025, 3.0) == 11.0
