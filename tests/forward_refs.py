"""Plain-torch references of the six forward operations of the codec (CPU, float64 by default), the
synthetic inputs the forward-kernel tests share, and their bars. The comparator (two norms), the
weights and the random draws are those of tests/backward_refs.py.

Every helper is the layer's definition (analysis_17.py:14-23, synthesis_17.py:15-25, GDN.py:64-94,
model.py:71-78) written with F.conv2d / F.conv_transpose2d and the explicit GDN formula, and takes
a ``dtype``: float64 gives the reference, float32 the "torch on the CPU in fp32" evaluation the bars
are derived from. tests/test_forward_refs_cpu.py checks the GDN formula and the bit sums against
the oracle's own (oracle.gdn, oracle.estimate_bits) in float64.

Tensors are NCHW here; the GPU tests permute to the kernels' NHWC. The effective GDN parameters are
always oracle.gdn_effective_params of the raw fp32 parameters (what the packing kernel computes),
cast to the working dtype; weights and biases are the fp32 parameters, widened.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import backward_refs as B
from oracle import codec_ref as oracle

F64 = torch.float64

# The project's standing bars: contraction outputs (REL of tests/test_gpu_parity.py) and per-image
# sums over pixels, bits and SSE (METRIC_REL there). No bar below is looser than its standing bar.
REL = 2e-5
METRIC_REL = 1e-5

OPS = ("conv1", "conv2", "conv3", "deconv1", "deconv2", "deconv3")

# (B, H, W) of the image; every layer's grid derives from it (H/4, H/8, H/16).
SHAPES = ((1, 16, 16),      # grids 4², 2², 1²: every tile partial, every pixel has taps in the padding
          (2, 16, 48),      # } an H / W mix-up shows
          (2, 48, 16),      # }
          (2, 80, 112),     # grids 20×28, 10×14, 5×7: ragged both ways for 8- and 16-wide tiles, odd
          (1, 144, 272))    # grids 36×68, 18×34, 9×17: one past a whole 8-, 16- and 32-tile
TILE_ROWS_SHAPE = (2, 80, 112)   # its two images, repeated, flip the h3 engine to 16-row tiles
GUARD_SHAPES = ((2, 80, 112), (1, 144, 272))


# ---------------------------------------------------------------------------- references
def gdn(u, beta, gamma, inverse):
    """GDN.py:64-94: u / √n(u) (GDN) or u · √n(u) (IGDN), n = β_eff + γ_eff · u²."""
    be, ge = B.effective_params(beta, gamma, u.dtype)
    s = torch.sqrt(B.norm_pool(u, be, ge))
    return u * s if inverse else u / s


def conv1_gdn(x, w, b, beta, gamma, dtype=F64):
    """conv 9×9 s4 p4 + bias, then GDN1 → (pre, out)."""
    pre = F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=4, padding=4)
    return pre, gdn(pre, beta, gamma, False)


def conv2_gdn(x, w, b, beta, gamma, dtype=F64):
    """conv 5×5 s2 p2 + bias, then GDN2 → (pre, out)."""
    pre = F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=2, padding=2)
    return pre, gdn(pre, beta, gamma, False)


def conv3(x, w, dtype=F64):
    """conv 5×5 s2 p2, no bias → y."""
    return F.conv2d(x.to(dtype), w.to(dtype), None, stride=2, padding=2)


def deconv_igdn(x, w, b, beta, gamma, dtype=F64):
    """transposed 5×5 s2 p2 op1 + bias, then IGDN (deconv1 and deconv2) → (pre, out)."""
    pre = F.conv_transpose2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=2, padding=2,
                             output_padding=1)
    return pre, gdn(pre, beta, gamma, True)


def deconv3(x, w, b, dtype=F64):
    """transposed 9×9 s4 p4 op3 + bias → (recon, clamp(recon, 0, 1))."""
    recon = F.conv_transpose2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=4, padding=4,
                               output_padding=3)
    return recon, recon.clamp(0, 1)


def bits(z, rate_params, dtype=F64):
    """Per-image Σ of oracle.element_bits (model.py:71-78) of an NCHW latent → [B]."""
    p = {"bitEstimator." + k: v.to(dtype) for k, v in rate_params.items()}
    return oracle.element_bits(z.to(dtype), p).sum(dim=(1, 2, 3))


def sse(out, x, dtype=F64):
    """Per-image Σ (out − x)² → [B]."""
    return ((out.to(dtype) - x.to(dtype)) ** 2).sum(dim=(1, 2, 3))


def image_rows(t):
    """An image batch [B,3,H,W] → [B,48,H/4,W/4]: the 4×4 output block with its three channels that
    one stride-4 position of conv1 / deconv3 covers, as the channel axis. A pixel's three values are
    too small a row for the per-row norm (torch's CPU fp32 already reads 3e-5 there)."""
    b, c, h, w = t.shape
    return t.reshape(b, c, h // 4, 4, w // 4, 4).permute(0, 1, 3, 5, 2, 4).reshape(b, c * 16, h // 4, w // 4)


# ------------------------------------------------------------------------------- inputs
def case(op, N, shape):
    """The fp32 NCHW inputs of one layer at image shape (B, H, W) and the parameters its reference
    needs. Independent draws per layer, not a chained forward: errors do not compound."""
    sd = B.state(N)
    b, H, W = shape
    s = 20000 + 1000 * OPS.index(op) + 100 * b + H + 3 * W
    if op == "conv1":
        return {"x": B.uniform(s, (b, 3, H, W), 0.0, 1.0), "w": sd["Encoder.conv1.weight"],
                "b": sd["Encoder.conv1.bias"], "beta": sd["Encoder.gdn1.beta"],
                "gamma": sd["Encoder.gdn1.gamma"]}
    if op == "conv2":
        return {"x": B.normal(s, (b, N, H // 4, W // 4), 0.7), "w": sd["Encoder.conv2.weight"],
                "b": sd["Encoder.conv2.bias"], "beta": sd["Encoder.gdn2.beta"],
                "gamma": sd["Encoder.gdn2.gamma"]}
    if op == "conv3":
        return {"x": B.normal(s, (b, N, H // 8, W // 8), 0.7), "w": sd["Encoder.conv3.weight"],
                "noise": B.uniform(s + 1, (b, N, H // 16, W // 16), -0.5, 0.5),
                "rate": B.rate_params(N)}
    if op == "deconv1":      # an integer latent: the h3 int_in form applies
        return {"x": torch.round(B.uniform(s, (b, N, H // 16, W // 16), -6, 6)),
                "w": sd["Decoder.deconv1.weight"], "b": sd["Decoder.deconv1.bias"],
                "beta": sd["Decoder.igdn1.beta"], "gamma": sd["Decoder.igdn1.gamma"]}
    if op == "deconv2":
        return {"x": B.normal(s, (b, N, H // 8, W // 8), 0.7), "w": sd["Decoder.deconv2.weight"],
                "b": sd["Decoder.deconv2.bias"], "beta": sd["Decoder.igdn2.beta"],
                "gamma": sd["Decoder.igdn2.gamma"]}
    assert op == "deconv3"
    return {"x": B.normal(s, (b, N, H // 4, W // 4), 0.5), "w": sd["Decoder.deconv3.weight"],
            "b": sd["Decoder.deconv3.bias"], "x_ref": B.uniform(s + 1, (b, 3, H, W), 0.0, 1.0)}


def reference(op, c, dtype=F64, x=None):
    """The reference outputs of ``case`` as a dict: {"pre", "out"}, conv3 {"y"}, deconv3 {"recon",
    "clipped"}. ``x`` replaces the case's input (the h3 tests pass what the kernel sees: the merged
    h3 planes of the input, float64)."""
    x = c["x"] if x is None else x
    if op == "conv1":
        pre, out = conv1_gdn(x, c["w"], c["b"], c["beta"], c["gamma"], dtype)
    elif op == "conv2":
        pre, out = conv2_gdn(x, c["w"], c["b"], c["beta"], c["gamma"], dtype)
    elif op == "conv3":
        return {"y": conv3(x, c["w"], dtype)}
    elif op == "deconv3":
        recon, clipped = deconv3(x, c["w"], c["b"], dtype)
        return {"recon": recon, "clipped": clipped}
    else:
        pre, out = deconv_igdn(x, c["w"], c["b"], c["beta"], c["gamma"], dtype)
    return {"pre": pre, "out": out}


def rows_of(key, t):
    """The tensor whose axis 1 is the row of the per-row norm: channels, or for the image outputs
    of deconv3 the 48 values of ``image_rows``."""
    return image_rows(t) if key.startswith("deconv3.") else t


def errors(key, got, ref):
    """backward_refs.errors of an NCHW output under the norms of bar ``key``."""
    if key.startswith(("bits", "sse")):      # per-image sums: one norm
        return B.errors(got, ref)
    return B.errors(rows_of(key, got), rows_of(key, ref), (1,))


def tie_band(y_ref):
    """The half-width of the band round a rounding boundary k + ½ inside which ŷ may differ from
    round(y_ref): the per-row bar of y times max|y_ref|. Fixed by the reference alone."""
    return BARS["conv3.y"]["row"] * y_ref.abs().max().item()


def excusable(y_ref):
    """The mask of the latents a correct fp32 kernel may round the other way."""
    return (y_ref - (torch.floor(y_ref) + 0.5)).abs() <= tie_band(y_ref)


EXCUSABLE_MAX = 1e-3      # of the elements, at every shape (measured on the CPU: at most 3.4e-4)


def tile_rows_batch(gh, gw, phases=1):
    """The smallest even batch at which the h3 engine takes 16-row tiles for a grid gh × gw
    (h3_tile_rows in csrc/engine_h3.hip: ⌈gh/16⌉·⌈gw/16⌉·B·phases ≥ 256 workgroups)."""
    b = math.ceil(256 / (math.ceil(gh / 16) * math.ceil(gw / 16) * phases))
    return b + b % 2


# --------------------------------------------------------------------------------- bars
# CPU_FP32: the worst error of the same formulas evaluated by torch on the CPU in fp32 against their
# float64 evaluation, over SHAPES and N = 128, 192, as measured by
# tests/test_forward_refs_cpu.py::test_cpu_fp32_within_bars (which prints them), rounded up.
# BARS = 4 × that (the MFMA's other fp32 summation order; the 2^-22 / 2^-24 representation error of
# the h3 / x6 operands), never above the standing bar of the output's kind: backward_refs._bar.
# Rows are one pixel's channels; for deconv3's image outputs the 48 values of ``image_rows``.
CPU_FP32 = {}
BARS = {}


def _bar(key, cpu_global, cpu_row, standing, widen=None):
    """backward_refs._bar, with the entry moved into this module's tables."""
    B._bar(key, cpu_global, cpu_row, standing, widen)
    CPU_FP32[key] = B.CPU_FP32.pop(key)
    BARS[key] = B.BARS.pop(key)


def bars(key, form=None):
    """The bars of output ``key`` in ``form``: a form with an entry of its own ("key@form", a
    widened one with its reason) takes that."""
    return BARS.get(f"{key}@{form}", BARS[key])


#    key                CPU fp32: global, per row   standing
_bar("conv1.pre",       7.4e-7, 1.1e-6, REL)
_bar("conv1.out",       8.9e-7, 1.1e-6, REL)
_bar("conv2.pre",       5.3e-7, 7.4e-7, REL)
_bar("conv2.out",       7.9e-7, 1.1e-6, REL)
_bar("conv3.y",         5.4e-7, 7.5e-7, REL)       # y, and ỹ = y + noise
# The plain fp32 conv3 (EPI_PLAIN in csrc/engine.h: no per-tap sums, those are for the layers whose
# output is rounded) adds its 25·N products into one running fp32 accumulator per output, as the
# backward k5 convolutions do: backward_refs.RUNNING_SUM. It measures 2.5e-6 / 3.6e-6.
_bar("conv3.y@plain",   5.4e-7, 7.5e-7, REL, widen=B.RUNNING_SUM)
# conv2 on the h3 engine runs without the two-level sums conv3 has there (SEP = false in
# csrc/engine_h3.hip): the three part products of all 25·N MACs of an output, 14400 terms at
# N = 192, go through one MFMA chain that rounds at the scale of its running sum. The same
# sqrt(K/2)·2^-24 argument gives 3e-6; it measures 1.8e-6 / 3.0e-6, a hair above 4 × the CPU's
# blocked sum. (Its GDN output meets 4 × and keeps it; the h3 deconvolutions have at most 9·N MACs
# per output and stay below 1e-6.)
H3_CHAIN = "one MFMA chain over the 3·25·N part products of an output; see above"
_bar("conv2.pre@h3",    5.3e-7, 7.4e-7, REL, widen=H3_CHAIN)
_bar("deconv1.pre",     7.0e-7, 1.1e-6, REL)
_bar("deconv1.out",     9.1e-7, 1.6e-6, REL)
_bar("deconv2.pre",     1.2e-6, 2.0e-6, REL)
_bar("deconv2.out",     1.2e-6, 2.0e-6, REL)
_bar("deconv3.recon",   1.5e-6, 2.6e-6, REL)
_bar("deconv3.clipped", 1.6e-6, 3.7e-6, REL)
# per-image sums, each of the kernel's own output in fp32 against the same sum in float64
_bar("bits.round",      1.4e-7, None, METRIC_REL)
_bar("bits.noise",      9.1e-8, None, METRIC_REL)
_bar("sse",             1.2e-7, None, METRIC_REL)
