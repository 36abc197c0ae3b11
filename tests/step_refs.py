"""Plain-torch reference of the stepped training step, its explicit backward
formulas, the inputs the stepped tests share and their bars.

The definition, per image b with Δ_b = codec.step_size(s_b) as an fp32 value:

    z = y/Δ_b + u,   ỹ = Δ_b·z,   bits_b = Σ element_bits(z, step pack of Δ_b),
    bpp_b = bits_b/(H·W),   mse_b = mean over 3·H·W of (recon_b − x_b)²,  recon unclipped

written from oracle.analysis, oracle.synthesis and oracle.bitparm, with the factorised model's
first layer evaluated as x·(softplus(h1)·Δ) + b1 (the step pack's row 0 is that product). Every
function computes in the dtype it is given: torch.float32 is the definition (op for op what the
kernels evaluate), torch.float64 its evaluation without fp32 rounding. Tensors are NCHW, the
oracle's layout; the GPU tests permute to the kernels' NHWC.

As in backward_refs.py the rate-parameter gradients have the fp32 reference's autograd as their
definition (the fp32 sigmoid's saturation is part of it), and so has the rate term of ∂L/∂y.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import backward_refs as R
from iclr_17_compression_amd import codec
from oracle import codec_ref as oracle

REL = R.REL              # per-element outputs
GRAD_REL = R.GRAD_REL    # sums over pixels
RATE_ORDER = R.RATE_ORDER


def deltas(steps, dtype=torch.float32):
    """Ladder indices → Δ [B, 1, 1, 1]: the fp32 values of codec.step_size, cast to ``dtype``."""
    d = torch.tensor([codec.step_size(int(s)) for s in steps], dtype=torch.float32)
    return d.to(dtype).view(-1, 1, 1, 1)


def _cast(p, dtype):
    return {k: (v if v.dtype == dtype else v.to(dtype)) for k, v in p.items()}


# ------------------------------------------------------------------------------ forward
def step_cdf(v, p, d, prefix="bitEstimator."):
    """The factorised CDF of the step pack at v: oracle.bit_estimator with f1's multiplier
    softplus(h1) replaced by the product softplus(h1)·Δ (one rounding in fp32, as the pack's)."""
    sp0 = F.softplus(p[prefix + "f1.h"]) * d
    t = v * sp0 + p[prefix + "f1.b"]
    v = t + torch.tanh(t) * torch.tanh(p[prefix + "f1.a"])
    for f in ("f2", "f3"):
        v = oracle.bitparm(v, p[f"{prefix}{f}.h"], p[f"{prefix}{f}.b"], p[f"{prefix}{f}.a"])
    return oracle.bitparm(v, p[prefix + "f4.h"], p[prefix + "f4.b"], None)


def step_element_bits(z, p, d):
    """oracle.element_bits (model.py:71-73) on ``step_cdf``."""
    prob = step_cdf(z + 0.5, p, d) - step_cdf(z - 0.5, p, d)
    return torch.clamp(-1.0 * torch.log(prob + 1e-10) / math.log(2.0), 0, 50)


def quantise(y, noise, d):
    """(z, ỹ) of the definition: a divide, an add, a product."""
    z = y / d + noise
    return z, d * z


def forward(x, p, noise, steps, dtype=torch.float32):
    """The stepped training forward → {"y", "z", "y_deq", "recon", "bits_el", "bits" [B],
    "bpp" [B], "mse" [B]} in ``dtype``; differentiable in the entries of ``p`` that require it
    when they already are of ``dtype``."""
    p = _cast(p, dtype)
    x = x.to(dtype)
    d = deltas(steps, dtype)
    y = oracle.analysis(x, p)
    z, y_deq = quantise(y, noise.to(dtype), d)
    recon = oracle.synthesis(y_deq, p)
    bits_el = step_element_bits(z, p, d)
    bits = bits_el.sum(dim=(1, 2, 3))
    H, W = x.shape[2], x.shape[3]
    return {"y": y, "z": z, "y_deq": y_deq, "recon": recon, "bits_el": bits_el, "bits": bits,
            "bpp": bits / (H * W), "mse": ((recon - x) ** 2).mean(dim=(1, 2, 3))}


def loss(out, lams):
    """mean_b(λ_b·mse_b + bpp_b)."""
    lam = torch.as_tensor(lams, dtype=out["mse"].dtype)
    return torch.mean(lam * out["mse"] + out["bpp"])


# ------------------------------------------------------------------- explicit backward
def rate_backward(z, rate, d, g_bits):
    """The backward of bits_b = Σ step_element_bits(z) for upstream g_bits [B], written out from
    the forward (no autograd): (g_bits[b]·∂bits_b/∂z, the 11 per-channel partials [11, C] in
    RATE_ORDER's slots with respect to softplus(h), b and tanh(a) of the UNscaled model: slot 0
    is ∂/∂softplus(h1) = Δ·∂/∂(softplus(h1)·Δ)). ``rate``: R.rate_params-style dict of raw
    [1, C, 1, 1] parameters; computes in z's dtype."""
    dt = z.dtype
    q = [rate[k].detach().to(dt).view(1, -1, 1, 1) for k in RATE_ORDER]
    sp = [F.softplus(q[3 * k]) for k in range(4)]
    ta = [torch.tanh(q[3 * k + 2]) for k in range(3)]
    bb = [q[3 * k + 1] for k in range(4)]
    sp0 = sp[0] * d                                   # the step pack's row 0
    mult = [sp0, sp[1], sp[2]]
    halves = []
    for half in (0.5, -0.5):
        xs, Ts = [z + half], []
        for k in range(3):
            t = xs[-1] * mult[k] + bb[k]
            Ts.append(torch.tanh(t))
            xs.append(t + Ts[-1] * ta[k])
        Fv = torch.sigmoid(xs[3] * sp[3] + bb[3])
        halves.append((xs, Ts, Fv))
    prob = halves[0][2] - halves[1][2]
    raw = -1.0 * torch.log(prob + 1e-10) / math.log(2.0)
    g0 = torch.where((raw >= 0) & (raw <= 50), g_bits.to(dt).view(-1, 1, 1, 1).expand_as(raw),
                     torch.zeros_like(raw))
    gl = g0 / math.log(2.0) * -1.0 / (prob + 1e-10)
    part = [torch.zeros(z.shape[1], dtype=dt) for _ in range(11)]
    dz = torch.zeros_like(z)
    psum = lambda t: t.sum(dim=(0, 2, 3))  # noqa: E731
    for sign, (xs, Ts, Fv) in zip((1.0, -1.0), halves):
        gt4 = sign * gl * (1 - Fv) * Fv
        part[10] = part[10] + psum(gt4)
        part[9] = part[9] + psum(gt4 * xs[3])
        gx = gt4 * sp[3]
        for k in (2, 1, 0):
            part[3 * k + 2] = part[3 * k + 2] + psum(gx * Ts[k])
            gt = gx + gx * ta[k] * (1 - Ts[k] * Ts[k])
            part[3 * k + 1] = part[3 * k + 1] + psum(gt)
            # ∂t/∂softplus(h_k) = x_k, for k = 0 times Δ (t = x·(softplus(h1)·Δ) + b1)
            part[3 * k] = part[3 * k] + psum(gt * xs[k] * (d if k == 0 else 1.0))
            gx = gt * mult[k]
        dz = dz + gx
    return dz, torch.stack(part)


def quantise_backward(g_deq, dz, d):
    """∂L/∂y from ∂L/∂ỹ and g_bits·∂bits/∂z: ỹ = Δ·(y/Δ + u) passes g_deq on (Δ·(1/Δ)), z = y/Δ + u
    divides the rate term by Δ."""
    return g_deq + dz / d


def rate_param_grads(part, rate):
    """[11, C] partials → the 11 raw gradients (R.rate_param_grad on a single row block)."""
    return R.rate_param_grad(part.unsqueeze(0), rate)


def rate_term_fp32(z, rate, steps, g_bits):
    """The definition of the rate term: the fp32 reference's autograd of Σ_b g_bits[b]·bits_b with
    respect to z and to the raw rate parameters (RATE_ORDER) → (∂/∂z, [11 gradients])."""
    zz = z.detach().float().clone().requires_grad_(True)
    p = {"bitEstimator." + k: rate[k].detach().float().clone().requires_grad_(True)
         for k in RATE_ORDER}
    bits = step_element_bits(zz, p, deltas(steps)).sum(dim=(1, 2, 3))
    (bits * torch.as_tensor(g_bits, dtype=torch.float32)).sum().backward()
    return zz.grad, [p["bitEstimator." + k].grad for k in RATE_ORDER]


def grad_recon_images(recon, x, g_mse=None, g_clip=None):
    """R.grad_recon with the weight of image b's mean((recon_b − x_b)²) in g_mse[b]."""
    g = torch.zeros_like(recon)
    per = recon[0].numel()
    if g_mse is not None:
        g = g + g_mse.to(recon.dtype).view(-1, 1, 1, 1) / per * 2 * (recon - x.to(recon.dtype))
    if g_clip is not None:
        g = g + g_clip.to(recon.dtype) * ((recon >= 0) & (recon <= 1)).to(recon.dtype)
    return g


# ------------------------------------------------------------------------------- inputs
# (B, h, w, C) of the kernel tests: one element per channel; a ragged single 4096-element chunk;
# two chunks with a ragged tail (and, for the backward's 16-pixel blocks: 1, 15 and 16 + 16 + 3
# pixels per image). Steps mix the ladder's ends and the unit step.
KERNEL_SHAPES = ((1, 1, 1, 128), (2, 3, 5, 192), (3, 5, 7, 192))
# The kernels take any channel count: fewer channels than a wave (the backward launches one wave,
# 57 lanes idle) and more than 256 (a backward thread owns two channels; the forward's rows of 300
# floats straddle its chunks and waves). What these cases can go wrong in is indexing, so the GPU
# test holds them to exact properties: the bits to rate_bits, and every per-channel result to the
# 192- / 128-channel run on the same data, bit for bit. Their ∂L/∂y is not held to the g_y bar,
# which belongs to KERNEL_SHAPES. Finding: at the finest step (Δ = ¼) the bins are narrow, the
# probability F(z + ½) − F(z − ½) is a difference of nearly equal fp32 values and the gradient a
# difference of two more, and the fp32 definition's own ∂L/∂y is 0.8–1.4e-5 of max|∂L/∂y| away
# from its float64 evaluation on every case that has such an image. Two fp32 evaluations with
# different tanhf / expf / logf (the CPU's and the GPU's) then stand about as far apart: measured
# 1.1e-5 and 6.9e-6 on KERNEL_SHAPES, and 2.4e-5 on the 12000-element (2, 4, 5, 300) case, above
# the standing 2e-5. The arithmetic is rate_bwd_element's, shared with the unstepped step.
EXTRA_SHAPES = ((1, 3, 3, 7), (2, 4, 5, 300))
KERNEL_STEPS = {1: (31,), 2: (0, 8), 3: (0, 8, 31)}
Y_STD = 3.0


def rate_params_any(C):
    """R.rate_params for the codec's channel counts; for another C the first C channels of the
    192- and 128-channel sets side by side (every channel is a model of its own)."""
    if C in (128, 192):
        return R.rate_params(C)
    a, b = R.rate_params(192), R.rate_params(128)
    return {k: torch.cat([a[k], b[k]], dim=1)[:, :C].contiguous() for k in RATE_ORDER}


def kernel_case(shape):
    """{"y", "noise", "g_deq" (NCHW fp32), "steps", "g_bits" [B], "rate"} of one kernel case.
    g_bits as a training step has it (∂mean_b bpp_b/∂bits_b = 1/(B·H·W), H·W = 256·h·w) and a
    decoder gradient of the rate term's size, so both terms of ∂L/∂y carry weight."""
    B, h, w, C = shape
    s = 9000 + 100 * B + 10 * h + w
    count = float(B * 256 * h * w)
    return {"y": R.normal(s, (B, C, h, w), Y_STD),
            "noise": R.uniform(s + 1, (B, C, h, w), -0.5, 0.5),
            "g_deq": R.normal(s + 2, (B, C, h, w), 2.0 / count),
            "steps": KERNEL_STEPS[B], "g_bits": torch.full((B,), 1.0 / count),
            "rate": rate_params_any(C)}


# the chain tests: N = 128, x [3, 3, 32, 48], synthetic weights, steps (2, 8, 19), fixed noise
CHAIN_N, CHAIN_SHAPE, CHAIN_STEPS, CHAIN_SEED = 128, (3, 3, 32, 48), (2, 8, 19), 2
CHAIN_LAM = 0.01 * 255.0 ** 2


# --------------------------------------------------------------------------------- bars
# CPU_FP32: the worst error of the formulas above evaluated by torch on the CPU in fp32 against
# their float64 evaluation over KERNEL_SHAPES, as tests/test_step_refs_cpu.py::test_cpu_fp32_figures
# measures and prints them (rounded up). BARS follow backward_refs.py's rule: min(4 × that figure,
# the standing bar of the output's kind).
CPU_FP32 = {}
BARS = {}


def _bar(key, cpu, standing, widen=None):
    """widen: a written reason to use the standing bar itself instead of 4 × the CPU figure."""
    CPU_FP32[key] = cpu
    BARS[key] = standing if widen else min(4 * cpu, standing)


# z and ỹ are single correctly rounded fp32 operations: the kernels must give torch's fp32 bits
# (the GPU test asserts equality); against float64 they stand half an ulp off.
_bar("z", 5.5e-8, REL)
_bar("y_deq", 8.0e-8, REL)
# ∂L/∂y = g_deq + dz/Δ with the whole formula in fp32 against the whole formula in float64, on the
# same z. With y ~ N(0, 3²) and the ladder's finest step some elements sit where the fp32
# sigmoid's 1 − F has lost digits, and the fp32 evaluation itself is 1.4e-5 off: 4 × that is above
# the standing bar, which therefore holds. As in backward_refs.py ("deconv_rate.g_rate") the GPU
# test's reference takes the rate term from the fp32 definition's autograd (rate_term_fp32) and
# evaluates the sum in float64; "g_y.sum_only" is what the fp32 evaluation loses in that last
# divide and add alone (recorded, not a bar).
_bar("g_y", 1.5e-5, REL)
CPU_FP32["g_y.sum_only"] = 6.0e-8
FP32_DEFINES = "the reference is the fp32 definition's autograd; sums over pixels keep GRAD_REL"
_bar("rate_params", 0.0, GRAD_REL, widen=FP32_DEFINES)
# Per-image bpp and mse of the chain (relative error per image). The CPU figure is that of a mean
# over ~1e3..1e4 terms whose fp32 rounding errors average out; the x6 / h3 contractions' dropped
# part products and the MFMA's summation order do not average that way, and the whole network
# lies between the input and these numbers: 4 × 8e-8 says nothing about a correct chain. They keep
# the standing bar of contraction outputs.
CHAIN_MEAN = "a mean over pixels behind the whole network; see above"
_bar("bpp", 8.0e-8, REL, widen=CHAIN_MEAN)
_bar("mse", 6.5e-8, REL, widen=CHAIN_MEAN)
