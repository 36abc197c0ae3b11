"""Plain-torch references of the backward kernels (CPU, float64 by default), the comparator the
backward-kernel tests share, their synthetic inputs and their bars.

Every helper is an explicit formula of the operation a HIP backward entry point computes, written
from the forward definition (models/GDN.py:64-94, analysis_17.py, synthesis_17.py) and not through
autograd; tests/test_backward_refs_cpu.py checks each one against float64 autograd, which is a
second, independent derivation. The one exception is the rate term of ``bwd_deconv_rate``: its
ground truth is the fp32 oracle's autograd (oracle.estimate_bits), whose fp32 sigmoid saturation
is part of the definition.

Tensors are NCHW here (the oracle's layout); the GPU tests permute to the kernels' NHWC. A helper
computes in the dtype of its first argument, so the same code gives the float64 reference and the
"torch on the CPU in fp32" evaluation the bars are derived from. The effective GDN parameters are
always oracle.gdn_effective_params of the raw fp32 parameters (what the packing kernel computes),
cast to the working dtype.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from iclr_17_compression_amd import synth
from oracle import codec_ref as oracle

# The project's standing bars: contraction outputs (REL of tests/test_gpu_parity.py) and sums over
# pixels (GRAD_REL of tests/test_gpu_backward.py). No bar below is looser than its standing bar.
REL = 2e-5
GRAD_REL = 1e-4
ROW_FLOOR = 1e-3          # per-row denominators are at least ROW_FLOOR · max|ref|

RATE_ORDER = ("f1.h", "f1.b", "f1.a", "f2.h", "f2.b", "f2.a", "f3.h", "f3.b", "f3.a", "f4.h",
              "f4.b")


# ------------------------------------------------------------------------------ comparator
def global_err(got, ref):
    """max|Δ| / max|ref| over the whole tensor (the project's existing norm)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def row_err(got, ref, dims):
    """The worst row: max over the rows of max_row|Δ| / max(max_row|ref|, ROW_FLOOR·max|ref|), a
    row being the elements that differ only in ``dims`` (the channel axes). NCHW activations:
    dims=(1,) → one row per pixel (b, i, j); [M][C][kh][kw] gradients: dims=(0, 1) → one row per
    tap. Every element takes part; one wrong pixel or tap is not diluted by the others."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = (got - ref).abs().amax(dim=dims)
    r = ref.abs().amax(dim=dims).clamp_min(ROW_FLOOR * ref.abs().max().item()).clamp_min(1e-300)
    return (d / r).max().item()


def errors(got, ref, dims=None):
    """{"global": …[, "row": …]}; NaN anywhere in ``got`` gives NaN errors, which pass no bar."""
    e = {"global": global_err(got, ref)}
    if dims is not None:
        e["row"] = row_err(got, ref, dims)
    return e


def within(errs, bars):
    """True when every error is at most its bar (a NaN error is not)."""
    return all(errs[k] <= bars[k] for k in errs)


# ------------------------------------------------------------------------- GDN / IGDN backward
def effective_params(beta, gamma, dtype=torch.float64):
    """(β_eff [C], γ_eff [C, C]) of raw GDN parameters: the fp32 values of GDN.py:73-79."""
    be, ge = oracle.gdn_effective_params(beta.detach().float(), gamma.detach().float())
    return be.to(dtype), ge.to(dtype)


def norm_pool(v, be, ge):
    """n = β_eff + γ_eff · v² (a 1×1 contraction over channels), NCHW."""
    return be.view(1, -1, 1, 1) + torch.einsum("ij,bjhw->bihw", ge, v * v)


def igdn_backward(t, v, be, ge):
    """s = v·√n(v), upstream t = ∂L/∂s → (∂L/∂v, dn = ∂L/∂n)."""
    s = torch.sqrt(norm_pool(v, be, ge))
    dn = t * v / (2 * s)
    return t * s + 2 * v * torch.einsum("ij,bihw->bjhw", ge, dn), dn


def gdn_backward(t, u, be, ge):
    """a = u/√n(u), upstream t = ∂L/∂a → (∂L/∂u, dn = ∂L/∂n)."""
    n = norm_pool(u, be, ge)
    s = torch.sqrt(n)
    dn = -t * u / (2 * n * s)
    return t / s + 2 * u * torch.einsum("ij,bihw->bjhw", ge, dn), dn


# ------------------------------------------------------------------ the four fused kernels
def bwd_deconv3_igdn(g_recon, w_deconv3, v_saved, beta, gamma):
    """deconv3's input gradient (its adjoint conv2d, weight [N,3,9,9]) then IGDN2 backward."""
    dt = g_recon.dtype
    t = F.conv2d(g_recon, w_deconv3.to(dt), stride=4, padding=4)
    return igdn_backward(t, v_saved.to(dt), *effective_params(beta, gamma, dt))


def bwd_deconv_igdn(g_v, w_deconv, v_prev, beta, gamma):
    """deconv2's input gradient (conv2d, weight [N,N,5,5]) then IGDN1 backward."""
    dt = g_v.dtype
    t = F.conv2d(g_v, w_deconv.to(dt), stride=2, padding=2)
    return igdn_backward(t, v_prev.to(dt), *effective_params(beta, gamma, dt))


def bwd_conv_gdn(g_u, w_conv, u_prev, beta, gamma):
    """conv3's / conv2's input gradient (conv_transpose2d, weight [N,N,5,5]) then GDN backward."""
    dt = g_u.dtype
    t = F.conv_transpose2d(g_u, w_conv.to(dt), stride=2, padding=2, output_padding=1)
    return gdn_backward(t, u_prev.to(dt), *effective_params(beta, gamma, dt))


def rate_term(y_tilde, rate_params, g_bpp, count):
    """(g_bpp / count)·∂Σbits/∂ỹ and the same factor times ∂Σbits/∂(h, b, a) in RATE_ORDER: the
    fp32 oracle's autograd of model.py:71-78 (bpp = Σbits / count, upstream g_bpp)."""
    y = y_tilde.detach().float().clone().requires_grad_(True)
    p = {"bitEstimator." + k: rate_params[k].detach().float().clone().requires_grad_(True)
         for k in RATE_ORDER}
    bits, _ = oracle.estimate_bits(y, p)
    (bits / float(count)).backward(torch.tensor(float(g_bpp)))
    return y.grad, [p["bitEstimator." + k].grad for k in RATE_ORDER]


def bwd_deconv_rate(g_v1, w_deconv1, y_tilde=None, rate_params=None, g_bpp=None, count=None):
    """deconv1's input gradient (conv2d) → (∂L/∂ỹ, rate-parameter gradients | None); with g_bpp
    the rate term is added (fp32 oracle autograd, see ``rate_term``)."""
    dt = g_v1.dtype
    g = F.conv2d(g_v1, w_deconv1.to(dt), stride=2, padding=2)
    if g_bpp is None:
        return g, None
    dy, pg = rate_term(y_tilde, rate_params, g_bpp, count)
    return g + dy.to(dt), pg


def pixel_sum(x):
    """Σ over pixels of an NCHW tensor → [C] (bias and β_eff gradients)."""
    return x.sum(dim=(0, 2, 3))


# ------------------------------------------------------- weight, bias, parameter gradients
def wgrad(G, X, k, stride, pad):
    """dW[m][c][kh][kw] = Σ_{b,o} G[b,m,o] · X[b,c,stride·o − pad + (kh,kw)]: G [B,M,Ho,Wo],
    X [B,C,stride·Ho,stride·Wo], both NCHW (torch.nn.grad.conv2d_weight, tap by tap)."""
    B, M, Ho, Wo = G.shape
    X = X.to(G.dtype)
    xp = F.pad(X, (pad, pad, pad, pad))
    dW = torch.empty(M, X.shape[1], k, k, dtype=G.dtype)
    for kh in range(k):
        for kw in range(k):
            xs = xp[:, :, kh:kh + stride * Ho:stride, kw:kw + stride * Wo:stride]
            dW[:, :, kh, kw] = torch.einsum("bmij,bcij->mc", G, xs)
    return dW


def wgrad_k5(G, X):
    return wgrad(G, X, 5, 2, 2)


def wgrad_k9(G, X):
    return wgrad(G, X, 9, 4, 4)


def gdn_wgrad(dn, u):
    """dγ_eff[i][j] = Σ_p dn[p][i] · u[p][j]², dn and u [P, C]."""
    u = u.to(dn.dtype)
    return dn.t() @ (u * u)


def gdn_param_chain(beta, gamma, dbeta_eff, dgamma_eff, beta_bound, gamma_bound):
    """GDN.py:10-24,73-79 backward: x_eff = max(x, bound)² − pedestal, and LowerBound passes a
    gradient where x ≥ bound or the gradient is negative."""
    dt = dbeta_eff.dtype

    def chain(x, g_eff, bound):
        x = x.to(dt)
        g = g_eff * 2 * torch.clamp_min(x, bound)
        return torch.where((x >= bound) | (g < 0), g, torch.zeros_like(g))

    return chain(beta, dbeta_eff, beta_bound), chain(gamma, dgamma_eff, gamma_bound)


def rate_param_grad(partial, rate_params):
    """Rate partials [T, 11, C] (∂L/∂softplus(h), ∂L/∂b, ∂L/∂tanh(a) per slot) → the 11 raw
    gradients (bitEstimator.py:13-25): Σ_T, then softplus' = sigmoid and tanh' = 1 − tanh²."""
    dt = partial.dtype
    S = partial.sum(0)
    out = []
    for i, k in enumerate(RATE_ORDER):
        p = rate_params[k].detach().reshape(-1).to(dt)
        role = k[-1]
        out.append(S[i] * torch.sigmoid(p) if role == "h" else S[i] if role == "b"
                   else S[i] * (1 - torch.tanh(p) ** 2))
    return out


def grad_recon(recon, x, g_mse=None, g_clip=None):
    """∂/∂recon of g_mse·mean((recon − x)²) + Σ g_clip·clamp(recon, 0, 1); torch's clamp passes
    the gradient on the closed interval."""
    g = torch.zeros_like(recon)
    if g_mse is not None:
        g = g + g_mse / recon.numel() * 2 * (recon - x.to(recon.dtype))
    if g_clip is not None:
        g = g + g_clip.to(recon.dtype) * ((recon >= 0) & (recon <= 1)).to(recon.dtype)
    return g


# ------------------------------------------------------------------------------- inputs
SEED = 5
GRID_SHAPES = ((1, 1, 1), (1, 5, 7), (2, 8, 8), (3, 9, 17))       # (B, h, w) of the kernel
IMAGE_SHAPES = ((1, 16, 16), (2, 48, 80), (1, 32, 144))           # (B, H, W) for bwd_deconv3_igdn
WGRAD_K5_SHAPES = ((1, 5, 7), (2, 16, 16), (3, 23, 23))           # (B, Ho, Wo): P = 35, 512, 1587
WGRAD_K9_SHAPES = ((192, 1, 5, 7), (128, 2, 16, 16), (192, 3, 20, 12), (192, 2, 33, 9))
GDN_WGRAD_SHAPES = ((192, 1000 + 17), (128, 4096 + 5), (192, 40))  # (C, P)
BIAS_NHWC_SHAPES = ((192, 1), (192, 1023), (192, 1025), (192, 5000), (3, 1025), (128, 1025))
BIAS_NCHW_SHAPES = ((1, 3, 256), (3, 3, 4096 + 5), (2, 192, 64))  # (B, C, HW)
RATE_T = (1, 7, 300)


@functools.lru_cache(maxsize=None)
def state(N):
    """synth.trained_like_state_dict(N, SEED) as fp32 torch tensors (β, γ entries below their
    bounds as they come)."""
    return {k: torch.from_numpy(v.copy()) for k, v in synth.trained_like_state_dict(N, SEED).items()}


def rate_params(N):
    sd = state(N)
    return {k: sd["bitEstimator." + k] for k in RATE_ORDER}


def normal(seed, shape, std=1.0):
    return torch.from_numpy(synth.normal_like(seed, shape, std))


def uniform(seed, shape, lo, hi):
    return torch.from_numpy(synth.uniform(seed, shape, lo, hi))


def fused_case(kernel, N, shape):
    """The fp32 NCHW inputs of one fused-kernel case and what its reference needs:
    {"g", "saved", "w", "beta", "gamma"} (bwd_deconv_rate: {"g", "y", "w", "rate", "g_bpp",
    "count"}). Independent draws, not a chained forward."""
    sd = state(N)
    B, h, w = shape
    s = 1000 * (1 + ("deconv3_igdn", "deconv_igdn", "conv_gdn", "deconv_rate").index(kernel)) + \
        100 * B + 10 * h + w
    if kernel == "deconv3_igdn":       # shape = (B, H, W) of the image
        return {"g": normal(s, (B, 3, h, w)), "saved": normal(s + 1, (B, N, h // 4, w // 4)),
                "w": sd["Decoder.deconv3.weight"], "beta": sd["Decoder.igdn2.beta"],
                "gamma": sd["Decoder.igdn2.gamma"]}
    if kernel == "deconv_igdn":
        return {"g": normal(s, (B, N, 2 * h, 2 * w)), "saved": normal(s + 1, (B, N, h, w)),
                "w": sd["Decoder.deconv2.weight"], "beta": sd["Decoder.igdn1.beta"],
                "gamma": sd["Decoder.igdn1.gamma"]}
    if kernel == "conv_gdn":
        return {"g": normal(s, (B, N, h, w)), "saved": normal(s + 1, (B, N, 2 * h, 2 * w)),
                "w": sd["Encoder.conv3.weight"], "beta": sd["Encoder.gdn2.beta"],
                "gamma": sd["Encoder.gdn2.gamma"]}
    assert kernel == "deconv_rate"
    # as a training step: bpp = Σbits / (B·H·W) with upstream 1, and a decoder gradient of the
    # rate term's size, so that both terms of ∂L/∂ỹ carry weight under either norm
    count = float(B * 256 * h * w)
    return {"g": normal(s, (B, N, 2 * h, 2 * w), 2.0 / count), "y": uniform(s + 1, (B, N, h, w), -6, 6),
            "w": sd["Decoder.deconv1.weight"], "rate": rate_params(N), "g_bpp": 1.0, "count": count}


def fused_reference(kernel, case, dtype=torch.float64, rate=False):
    """The reference outputs of ``fused_case``: (g_prev, dn) NCHW, or for deconv_rate
    (g_y, rate-parameter gradients | None)."""
    g = case["g"].to(dtype)
    if kernel == "deconv_rate":
        if rate:
            return bwd_deconv_rate(g, case["w"], case["y"], case["rate"], case["g_bpp"], case["count"])
        return bwd_deconv_rate(g, case["w"])
    fn = {"deconv3_igdn": bwd_deconv3_igdn, "deconv_igdn": bwd_deconv_igdn,
          "conv_gdn": bwd_conv_gdn}[kernel]
    return fn(g, case["w"], case["saved"], case["beta"], case["gamma"])


def wgrad_case(kind, M, B, Ho, Wo):
    """(G [B,M,Ho,Wo], X) NCHW fp32: k5 X [B,M,2Ho,2Wo] normal, k9 X [B,3,4Ho,4Wo] in [0, 1]."""
    s = 7000 + 1000 * kind + M + 100 * B + 10 * Ho + Wo
    G = normal(s, (B, M, Ho, Wo))
    if kind == 5:
        return G, normal(s + 1, (B, M, 2 * Ho, 2 * Wo))
    return G, uniform(s + 1, (B, 3, 4 * Ho, 4 * Wo), 0.0, 1.0)


# --------------------------------------------------------------------------------- bars
# CPU_FP32: the worst error of the same formulas evaluated by torch on the CPU in fp32 against
# their float64 evaluation, over every shape above and N = 128, 192, as measured by
# tests/test_backward_refs_cpu.py::test_cpu_fp32_within_bars (which prints them), rounded up.
# BARS = 4 × that (the MFMA's other fp32 summation order; the x6 scheme's dropped part products),
# never above the standing bar of the output's kind. Where 4 × the CPU figure says nothing, the
# standing bar holds and the reason is given.
CPU_FP32 = {}
BARS = {}


def _bar(key, cpu_global, cpu_row, standing, widen=None):
    """widen: a written reason to use the standing bar itself instead of 4 × the CPU figure."""
    CPU_FP32[key] = {"global": cpu_global, "row": cpu_row}
    BARS[key] = {n: standing if widen else min(4 * v, standing)
                 for n, v in (("global", cpu_global), ("row", cpu_row)) if v is not None}


# The k5 s2 convolution of bwd_deconv_igdn and bwd_deconv_rate adds its K = 25·N products (4800 at
# N = 192) into a running fp32 accumulator per output (engine.h: every MFMA of the fp32 form, every
# 32-channel step of the x6 form, adds into the same registers; only the forward GDN and quantiser
# layers accumulate per tap), where torch's CPU convolution sums in blocks. A running sum of K
# random terms carries an error of the order sqrt(K/2)·2^-24 of the sum's scale (3e-6 at K = 4800,
# and the worst of ~1e5 outputs is a few times the typical one), against the blocked sum's 5e-7:
# a correct kernel of this design cannot meet 4 × the CPU figure. These outputs keep the standing
# bar of contraction outputs instead. (The transposed form of bwd_conv_gdn has at most 9·N terms
# per output and meets 4 ×, as does everything else: bwd_deconv_igdn's dn, which scales that sum by
# v/(2·√n), comes closest, 3.2e-6 against its 3.3e-6, and keeps 4 × because it meets it.)
RUNNING_SUM = "a running fp32 accumulator over K = 25·N terms; see above"

#    key                     CPU fp32: global, per row     standing
_bar("deconv3_igdn.g",       7.4e-7, 1.1e-6, REL)
_bar("deconv3_igdn.dn",      5.9e-7, 1.2e-6, REL)
_bar("deconv3_igdn.sum_g",   3.4e-7, None, GRAD_REL)
_bar("deconv3_igdn.sum_dn",  4.1e-7, None, GRAD_REL)
_bar("deconv_igdn.g",        4.9e-7, 9.3e-7, REL, widen=RUNNING_SUM)
_bar("deconv_igdn.dn",       8.3e-7, 1.7e-6, REL)
# Σ g_prev adds outputs that each carry that error: no better than its addends, so their bar
_bar("deconv_igdn.sum_g",    5.9e-7, None, REL, widen=RUNNING_SUM)
_bar("deconv_igdn.sum_dn",   4.8e-7, None, GRAD_REL)
_bar("conv_gdn.g",           6.8e-7, 1.7e-6, REL)
_bar("conv_gdn.dn",          1.4e-6, 2.4e-6, REL)
_bar("conv_gdn.sum_g",       4.7e-7, None, GRAD_REL)
_bar("conv_gdn.sum_dn",      9.8e-7, None, GRAD_REL)
_bar("deconv_rate.g",        5.3e-7, 9.3e-7, REL, widen=RUNNING_SUM)
_bar("deconv_rate.g_rate",   5.3e-7, 8.7e-7, REL, widen=RUNNING_SUM)
# The oracle's fp32 autograd is the definition of the rate-parameter gradients, so torch's fp32
# evaluation has no error of its own to take 4 × of: the standing bar for sums over pixels.
_bar("deconv_rate.params",   0.0, None, GRAD_REL,
     widen="the reference is the fp32 oracle itself; sums over pixels keep GRAD_REL")
_bar("wgrad_k5",             5.7e-7, 6.3e-7, GRAD_REL)
_bar("wgrad_k9",             6.1e-7, 6.8e-7, GRAD_REL)
_bar("gdn_wgrad",            5.8e-7, None, GRAD_REL)
_bar("bias_nhwc",            1.7e-7, None, GRAD_REL)
_bar("bias_nchw",            1.2e-7, None, GRAD_REL)
_bar("grad_recon",           4.2e-8, None, REL)
_bar("gdn_param_chain",      3.4e-8, None, REL)
_bar("rate_param_grad",      2.3e-7, None, GRAD_REL)
