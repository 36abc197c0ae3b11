"""Float64 definitions of latent refinement's kernels (csrc/refine.hip) and of the
latent part of one loop iteration, with the inputs the refinement tests share.

Per image b at step Δ_b, λ_b in train.py's units:

    J_b = bits_b + (λ_b/3)·SSE8_b/255²                                   (``objective``)
    g_recon = (λ_b/3)·2·(recon − ref/255) on the image's own pixels, 0 on the padding
    g = g_ỹ + ∂bits/∂z(ŷ)/Δ_b                                              (straight through)
    Adam (torch.optim.Adam: β = 0.9, 0.999, ε = 1e-8, bias correction) on y with lr·Δ_b
    ŷ' = rint(y'/Δ_b),  ỹ' = Δ_b·ŷ'

Every function computes in the dtype it is given; the rate model is step_refs' (the oracle's
factorised model on the step pack). Tensors are NCHW as the oracle's; the GPU tests permute to the
kernels' NHWC.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import backward_refs as R
import step_refs as S
from iclr_17_compression_amd import synth

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
REL = 1e-5     # m, v and y' against the float64 evaluation fed the kernel's own g (DESIGN.md §0f's bar)


def objective(bits, sse, lam):
    """J in float64, the operations in the order codec.refine_objective and the device take."""
    return float(bits) + (float(lam) / 3.0) * float(int(sse)) / 65025.0


def bits_of(z, rate, d):
    """Σ element bits per image [B] of z on the step pack of d [B,1,1,1], in z's dtype."""
    p = {"bitEstimator." + k: rate[k].to(z.dtype) for k in S.RATE_ORDER}
    return S.step_element_bits(z, p, d.to(z.dtype)).sum(dim=(1, 2, 3))


def dbits_dz(z, rate, d):
    """∂bits_b/∂z written out (step_refs.rate_backward with a unit upstream gradient)."""
    ones = torch.ones(z.shape[0], dtype=z.dtype)
    return S.rate_backward(z, rate, d.to(z.dtype), ones)[0]


def grad_recon(recon, refs, wt):
    """recon [B,3,Hc,Wc]; refs: B uint8 HWC arrays (H_b ≤ Hc, W_b ≤ Wc); wt [B] →
    wt_b·(2·(recon − ref/255)) inside each image, 0 outside, in recon's dtype."""
    g = torch.zeros_like(recon)
    for b, im in enumerate(refs):
        H, W = im.shape[:2]
        x = torch.from_numpy(np.ascontiguousarray(im)).permute(2, 0, 1).to(recon.dtype) / 255
        g[b, :, :H, :W] = wt[b].to(recon.dtype) * (2 * (recon[b, :, :H, :W] - x))
    return g


def adam_step(p, g, m, v, lr, t):
    """Step number t ≥ 1 of torch.optim.Adam's single-tensor update → (p', m', v'); lr a scalar or
    broadcastable tensor."""
    m = m + (1 - BETA1) * (g - m)
    v = v * BETA2 + (1 - BETA2) * g * g
    bc1, bc2 = 1 - BETA1 ** t, 1 - BETA2 ** t
    denom = v.sqrt() / math.sqrt(bc2) + EPS
    return p + (-(lr / bc1)) * m / denom, m, v


def latent_iteration(y_hat, g_deq, y, m, v, d, rate, lr, t, g=None):
    """The latent part of one iteration in the inputs' dtype → {"g", "y", "m", "v", "y_hat",
    "y_deq"}. ``g``: use this gradient (the kernel's own) instead of the formula's."""
    if g is None:
        g = g_deq + dbits_dz(y_hat, rate, d) / d
    y2, m2, v2 = adam_step(y, g, m, v, lr * d, t)
    q = torch.round(y2 / d)     # half to even, as rintf
    return {"g": g, "y": y2, "m": m2, "v": v2, "y_hat": q, "y_deq": d * q}


def keep(bits, sse, lam, qstatus, recon_status, best_J):
    """refine_keep's decision per image → (kept [bool], the new best_J): J < best_J strictly; a NaN,
    a non-zero quantiser status and a non-zero reconstruction status are not better."""
    J = [objective(b, s, l) for b, s, l in zip(bits, sse, lam)]
    kept = [not recon_status and not q and j < old for j, q, old in zip(J, qstatus, best_J)]
    return kept, [j if k else old for j, k, old in zip(J, kept, best_J)]


# ------------------------------------------------------------------------------- inputs
# (B, h, w, C) with ladder indices 5 and 12: 6720 elements per image (two chunks, a ragged tail),
# and 1536 (less than one chunk)
STEP_SHAPES = ((2, 5, 7, 192), (2, 3, 4, 128))
STEP_INDICES = (5, 12)
LR = 0.05


def step_case(shape):
    """{"y", "g_deq", "m", "v" (NCHW fp32), "rate"}: a latent, a decoder gradient of the rate
    term's size and moments as a few steps leave them (v ≥ 0)."""
    B, h, w, C = shape
    s = 7000 + 10 * h + w
    g = R.normal(s + 1, (B, C, h, w), 0.5)
    return {"y": R.normal(s, (B, C, h, w), S.Y_STD), "g_deq": g,
            "m": 0.1 * R.normal(s + 2, (B, C, h, w), 0.5),
            "v": 0.001 * R.normal(s + 3, (B, C, h, w), 0.5) ** 2,
            "rate": S.rate_params_any(C)}


# the end-to-end tests: synthetic weights N = 128, three images on two canvases
E2E_N, E2E_SEED, E2E_STEP, E2E_ITERS, E2E_LAMBDA = 128, 3, 8, 3, 650.25
E2E_SIZES = ((40, 56), (64, 64), (17, 33))


def e2e_images():
    """uint8 HWC images of E2E_SIZES."""
    return [np.ascontiguousarray(synth.image_u8(20 + k, 1, H, W)[0].transpose(1, 2, 0))
            for k, (H, W) in enumerate(E2E_SIZES)]
