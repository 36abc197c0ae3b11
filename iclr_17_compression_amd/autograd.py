"""Autograd glue for the HIP kernels (forward and backward both run in libiclr17.so).

* ``CodecTrainFn`` — the fused training step of ImageCompressor (model.py:47-80 with the loss
  terms train.py:97-102 intends): outputs (clipped, ỹ, bpp, mse_unclipped); its backward is the
  reference autograd graph of ``rd_loss.backward()`` (train.py:105) as fused kernels.
* ``AnalysisFn`` / ``SynthesisFn`` — Encoder / Decoder used on their own (NewTests-style
  callers, train_decoder_new.py:66-105 trains a Decoder alone).
* ``GDNFn`` / ``BitEstimatorFn`` / ``BitparmFn`` — the stand-alone modules with their own
  backward kernels.
* Where no backward is wired (ImageCompressor.forward in eval mode with autograd on), outputs
  carry a grad_fn that raises instead of silently producing wrong gradients.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import chain, kernels

Tensor = torch.Tensor


class _NoBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, name, out, *inputs):
        ctx.name = name
        return out.view_as(out)

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError(f"iclr17: backward of {ctx.name} is not implemented by the HIP path yet")


def no_backward(out: Tensor, name: str, params: Sequence[Tensor], x: Tensor):
    needs = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
    if not needs:
        return out
    return _NoBackward.apply(name, out, x, *params)


def gdn_apply(x: Tensor, module) -> Tensor:
    if needs_grad(x, (module.beta, module.gamma)):
        return GDNFn.apply(x, module, module.beta, module.gamma)
    beta_eff, gp = module.effective_params()
    return kernels.gdn(x, beta_eff, gp, module.inverse)


class GDNFn(torch.autograd.Function):
    """Stand-alone GDN / IGDN (GDN.py:64-94) with its autograd: ∂x from the fused backward
    kernel, ∂β / ∂γ through GDN.py:73-79 (LowerBound's gradient rule included)."""

    @staticmethod
    def forward(ctx, x, module, beta, gamma):
        beta_eff, gp = module.effective_params()
        ctx.module = module
        ctx.x6 = chain.train_mode(kernels.precision()).backward.x6   # dγ's contraction
        ctx.save_for_backward(x)
        return kernels.gdn(x, beta_eff, gp, module.inverse)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        m = ctx.module
        be, gp, gpt = m.effective_params_bwd()
        dx, dn, u = kernels.gdn_backward(x, g, be, gp, gpt, m.inverse)
        bb, gb, _ = m.bounds_f32()
        dbeta, dgamma = kernels.gdn_param_grads(dn, u, kernels.bias_grad_nhwc(dn), m.beta, m.gamma,
                                                bb, gb, x6=ctx.x6)
        return dx, None, dbeta.view_as(m.beta), dgamma.view_as(m.gamma)


class BitEstimatorFn(torch.autograd.Function):
    """BitEstimator.forward (bitEstimator.py:38-42) with its autograd."""

    @staticmethod
    def forward(ctx, x, module, *params):
        ctx.module = module
        ctx.save_for_backward(x)
        return kernels.bit_estimator(x, module.packed(), module.channel)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        m = ctx.module
        dx, part = kernels.bit_estimator_backward(x, g, m.packed(), m.channel)
        grads = kernels.rate_param_grads(part, m.params_in_order())
        return (dx.view_as(x), None, *[gr.view_as(p) for gr, p in zip(grads, m.params_in_order())])


class BitparmFn(torch.autograd.Function):
    """One Bitparm layer (bitEstimator.py:20-25) with its autograd."""

    @staticmethod
    def forward(ctx, x, module, *params):
        ctx.module = module
        ctx.save_for_backward(x)
        return kernels.bitparm(x, module.h, module.b, module.a)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        m = ctx.module
        dx, part = kernels.bitparm_backward(x, g, m.h, m.b, m.a)
        if m.a is not None:   # slots 0-2 of the rate table: (h, b, a) as BitEstimator's f1
            grads = kernels.rate_param_grads(part, [m.h, m.b, m.a] * 3 + [m.h, m.b])[:3]
        else:                 # slots 9-10: the final layer's (h, b)
            grads = kernels.rate_param_grads(part, [m.h, m.b, m.h] * 3 + [m.h, m.b])[9:]
        ps = [p for p in (m.h, m.b, m.a) if p is not None]
        return (dx.view_as(x), None, *[gr.view_as(p) for gr, p in zip(grads, ps)])


def needs_grad(x: Optional[Tensor], params: Sequence[Tensor]) -> bool:
    return torch.is_grad_enabled() and ((x is not None and x.requires_grad) or
                                        any(p.requires_grad for p in params))


# ------------------------------------------------------------------------------ analysis
def conv1_input_grad(enc, g_u1: Tensor) -> Tensor:
    """∂L/∂x of conv1 (analysis_17.py:32, k9 s4 p4): the transposed convolution of ∂L/∂u1
    (NHWC) with conv1's own weights — the shape and arithmetic of deconv3 (k9 s4 p4 op3, N → 3),
    so it runs on the exact-f32 deconv3 kernel with conv1.weight in deconv3's packing, a zero
    bias and the unclipped output."""
    w = enc.packed_conv1_t()
    zero = torch.zeros(3, device=g_u1.device, dtype=torch.float32)
    _, dx, _ = kernels.deconv3(g_u1.contiguous(), w, zero, want_recon=True)
    return dx


def analysis_backward(enc, feats: chain.AnalysisFeats, g_y: Tensor,
                      g_y_split: Optional[Tensor] = None, want_dx: bool = False, *,
                      mode: str) -> Dict[str, Tensor]:
    """∂L/∂y (NHWC) → parameter gradients of Analysis_net_17 (analysis_17.py:14-39). ``mode``: the
    one the forward that made ``feats`` ran in; its ``backward`` object (chain.py) holds what
    differs: exact f32 on fp32 gradients, or x6 on split-form gradients (g_y_split, or split
    here), each kernel handing the next its gradient in that form."""
    bw = chain.train_mode(mode).backward
    gdn1, gdn2 = enc.gdn1, enc.gdn2
    bb1, gb1, _ = gdn1.bounds_f32()
    bb2, gb2, _ = gdn2.bounds_f32()
    w3t, w2t = enc.packed_bwd()
    g = bw.grad(g_y, g_y_split)
    p2, p1 = bw.gdn_params(gdn2), bw.gdn_params(gdn1)
    a1, a2 = bw.analysis_operands(feats)
    dW3 = bw.wgrad_k5(g[bw.form], a2)
    g_u2, dn2, db2, dbe2 = bw.layer(kernels.bwd_conv_gdn, g, w3t, feats.u2, p2)
    dW2 = bw.wgrad_k5(g_u2[bw.form], a1)
    dbeta2, dgamma2 = kernels.gdn_param_grads(dn2, feats.u2, dbe2, gdn2.beta, gdn2.gamma, bb2, gb2,
                                              x6=bw.x6)
    g_u1, dn1, db1, dbe1 = bw.layer(kernels.bwd_conv_gdn, g_u2, w2t, feats.u1, p1, want_f32=want_dx)
    dW1 = bw.wgrad_k9(g_u1[bw.form], feats.x)
    dbeta1, dgamma1 = kernels.gdn_param_grads(dn1, feats.u1, dbe1, gdn1.beta, gdn1.gamma, bb1, gb1,
                                              x6=bw.x6)
    grads = {"conv1.weight": dW1, "conv1.bias": db1, "gdn1.beta": dbeta1, "gdn1.gamma": dgamma1,
             "conv2.weight": dW2, "conv2.bias": db2, "gdn2.beta": dbeta2, "gdn2.gamma": dgamma2,
             "conv3.weight": dW3}
    if want_dx:
        grads["x"] = conv1_input_grad(enc, g_u1[0])
    return grads


# ----------------------------------------------------------------------------- synthesis
def synthesis_backward(dec, saved: chain.SynthesisSaved, g_recon: Tensor,
                       g_bpp: Optional[Tensor] = None, rate_packed: Optional[Tensor] = None,
                       count: float = 0.0, want_split: bool = False, *, mode: str):
    """∂L/∂recon (NCHW) → (∂L/∂ỹ NHWC incl. the rate term when g_bpp is given, parameter
    gradients of Synthesis_net_17, rate-parameter partials, ∂L/∂ỹ in split form: with
    ``want_split`` where the mode's gradients travel split, else None). ``mode`` as in
    ``analysis_backward``."""
    bw = chain.train_mode(mode).backward
    igdn1, igdn2 = dec.igdn1, dec.igdn2
    bq1, gq1, _ = igdn1.bounds_f32()
    bq2, gq2, _ = igdn2.bounds_f32()
    d3, d2c, d1c = dec.packed_bwd(bw.x6)
    q2, q1 = bw.gdn_params(igdn2), bw.gdn_params(igdn1)
    _, h, w, _ = saved.y.shape
    y, s1, s2 = bw.synthesis_operands(saved)
    dWd3 = bw.wgrad_k9(s2, g_recon)
    dbd3 = kernels.bias_grad_nchw(g_recon)
    g_v2, dnq2, dbd2, dbeq2 = bw.deconv3_layer(g_recon, d3, saved.v2, q2)
    dWd2 = bw.wgrad_k5(s1, g_v2[bw.form])
    dbq2, dgq2 = kernels.gdn_param_grads(dnq2, saved.v2, dbeq2, igdn2.beta, igdn2.gamma, bq2, gq2,
                                         x6=bw.x6)
    g_v1, dnq1, dbd1, dbeq1 = bw.layer(kernels.bwd_deconv_igdn, g_v2, d2c, saved.v1, q1)
    dWd1 = bw.wgrad_k5(y, g_v1[bw.form])
    dbq1, dgq1 = kernels.gdn_param_grads(dnq1, saved.v1, dbeq1, igdn1.beta, igdn1.gamma, bq1, gq1,
                                         x6=bw.x6)
    g_y, rpart, g_ys = bw.rate_layer(g_v1, d1c, saved.y if g_bpp is not None else None,
                                     rate_packed, g_bpp, count, h, w, want_split=want_split)
    grads = {"deconv1.weight": dWd1, "deconv1.bias": dbd1, "igdn1.beta": dbq1, "igdn1.gamma": dgq1,
             "deconv2.weight": dWd2, "deconv2.bias": dbd2, "igdn2.beta": dbq2, "igdn2.gamma": dgq2,
             "deconv3.weight": dWd3, "deconv3.bias": dbd3}
    return g_y, grads, rpart, g_ys


def synthesis_latent_grad(dec, saved: chain.SynthesisSaved, g_recon: Tensor, *, mode: str) -> Tensor:
    """∂L/∂recon (NCHW) → ∂L/∂ỹ (fp32 NHWC) alone: the data-gradient chain of
    ``synthesis_backward`` — the same three fused input-gradient kernels on the same operands, so
    the same ∂L/∂ỹ — without the weight, bias and GDN-parameter gradients and with no rate term.
    What latent refinement (codec.refine_loop) runs per iteration. ``mode`` as there."""
    bw = chain.train_mode(mode).backward
    d3, d2c, d1c = dec.packed_bwd(bw.x6)
    q2, q1 = bw.gdn_params(dec.igdn2), bw.gdn_params(dec.igdn1)
    _, h, w, _ = saved.y.shape
    g_v2, _, _, _ = bw.deconv3_layer(g_recon, d3, saved.v2, q2)
    g_v1, _, _, _ = bw.layer(kernels.bwd_deconv_igdn, g_v2, d2c, saved.v1, q1)
    g_y, _, _ = bw.rate_layer(g_v1, d1c, None, None, None, 0.0, h, w, want_split=False)
    return g_y


def _ordered(module, prefix: str, grads: Dict[str, Tensor]) -> List[Optional[Tensor]]:
    return [grads.get(name) for name, _ in module.named_parameters()]


# --------------------------------------------------------------------------- Functions
class CodecTrainFn(torch.autograd.Function):
    """ImageCompressor training forward: (clipped, ỹ NCHW-view, bpp, mse of unclipped recon)."""

    @staticmethod
    def forward(ctx, x, noise, net, mode, *params):
        ctx.set_materialize_grads(False)
        enc, dec, be = net.Encoder, net.Decoder, net.bitEstimator
        B, _, H, W = x.shape
        m = chain.train_mode(mode)
        saved_a = m.train_analysis(enc, x)
        rate = be.packed()
        y_tilde, bits_part, latent = m.train_conv3(enc, saved_a, rate, noise)
        clipped, recon, sse_part, saved_s = m.train_synthesis(dec, y_tilde, latent, x)
        _, bpp = kernels.reduce_partials(bits_part, 1.0 / (B * H * W), per_image=False)
        _, mse = kernels.reduce_partials(sse_part, 1.0 / (B * 3 * H * W), per_image=False)
        ctx.net, ctx.mode = net, mode
        ctx.saved_a, ctx.saved_s = saved_a, saved_s
        ctx.recon, ctx.x, ctx.rate, ctx.count = recon, x, rate, float(B * H * W)
        return clipped, y_tilde.permute(0, 3, 1, 2), bpp, mse

    @staticmethod
    def backward(ctx, g_clipped, g_ytilde, g_bpp, g_mse):
        net = ctx.net
        enc, dec, be = net.Encoder, net.Decoder, net.bitEstimator
        grads: List[Optional[Tensor]] = []
        if g_clipped is None and g_mse is None:
            g_recon = torch.zeros_like(ctx.recon)
        else:
            g_recon = kernels.grad_recon(ctx.recon, ctx.x, g_mse, g_clipped)
        g_y, gs, rpart, g_ys = synthesis_backward(dec, ctx.saved_s, g_recon, g_bpp, ctx.rate,
                                                  ctx.count, want_split=g_ytilde is None,
                                                  mode=ctx.mode)
        red = getattr(net, "_grad_reducer", None)
        red = red if red is not None and red.active else None
        if red is not None:   # the synthesis gradients all-reduce during the analysis backward
            red.launch(list(dec.parameters()), _ordered(dec, "", gs))
        if g_ytilde is not None:
            g_y = g_y + g_ytilde.permute(0, 2, 3, 1)
        want_dx = ctx.needs_input_grad[0]
        rg = (kernels.rate_param_grads(rpart, be.params_in_order())
              if g_bpp is not None else [None] * 11)
        ga = analysis_backward(enc, ctx.saved_a, g_y.contiguous(), g_ys, want_dx=want_dx,
                               mode=ctx.mode)
        grads += _ordered(enc, "Encoder.", ga)
        grads += _ordered(dec, "Decoder.", gs)
        names = [n for n, _ in be.named_parameters()]
        order = ["f1.h", "f1.b", "f1.a", "f2.h", "f2.b", "f2.a", "f3.h", "f3.b", "f3.a", "f4.h", "f4.b"]
        rmap = dict(zip(order, rg))
        grads += [rmap[n] for n in names]
        if red is not None:
            red.launch(list(enc.parameters()) + list(be.parameters()),
                       _ordered(enc, "", ga) + [rmap[n] for n in names])
        dx = ga.get("x")
        if dx is not None and g_mse is not None:   # the loss's own x: ∂mse/∂x = −∂mse/∂recon
            dx = dx - kernels.grad_recon(ctx.recon, ctx.x, g_mse, None)
        ctx.saved_a = ctx.saved_s = ctx.recon = None
        return (dx, None, None, None, *grads)


RATE_PARAM_ORDER = ["f1.h", "f1.b", "f1.a", "f2.h", "f2.b", "f2.a", "f3.h", "f3.b", "f3.a", "f4.h",
                    "f4.b"]


class StepTrainFn(torch.autograd.Function):
    """ImageCompressor training forward with a ladder step per image:
    (clipped, bpp [B], mse of the unclipped recon [B]). ``steps_dev``: fp32 [B], Δ per image.
    The analysis and synthesis halves are CodecTrainFn's; between them y (the mode's unrounded
    conv3 output) goes through kernels.step_noise_rate, and the rate term of the backward through
    its own kernel instead of deconv1's rate epilogue."""

    @staticmethod
    def forward(ctx, x, noise, steps_dev, net, mode, *params):
        ctx.set_materialize_grads(False)
        enc, dec, be = net.Encoder, net.Decoder, net.bitEstimator
        B, _, H, W = x.shape
        m = chain.train_mode(mode)
        saved_a = m.train_analysis(enc, x)
        y = enc.y_nhwc(x, m.name, feats=saved_a)
        rate = be.packed()
        z, y_deq, bits_part = kernels.step_noise_rate(y, noise, steps_dev, rate)
        # inside the chain train_analysis began: an overflow in either half ends in a NaN distortion
        latent = m.chained_latent(y_deq)
        clipped, recon, sse_part, saved_s = m.train_synthesis(dec, y_deq, latent, x)
        bits, _ = kernels.reduce_partials(bits_part)
        sse, _ = kernels.reduce_partials(sse_part)
        ctx.net, ctx.mode = net, m.name
        ctx.saved_a, ctx.saved_s = saved_a, saved_s
        ctx.recon, ctx.x, ctx.rate, ctx.z, ctx.steps = recon, x, rate, z, steps_dev
        ctx.pixels = float(H * W)
        return clipped, (bits / (H * W)).float(), (sse / (3 * H * W)).float()

    @staticmethod
    def backward(ctx, g_clipped, g_bpp, g_mse):
        net = ctx.net
        enc, dec, be = net.Encoder, net.Decoder, net.bitEstimator
        if g_clipped is None and g_mse is None:
            g_recon = torch.zeros_like(ctx.recon)
        else:
            g_recon = kernels.grad_recon_images(ctx.recon, ctx.x, g_mse, g_clipped)
        g_y, gs, _, _ = synthesis_backward(dec, ctx.saved_s, g_recon, mode=ctx.mode)
        red = getattr(net, "_grad_reducer", None)
        red = red if red is not None and red.active else None
        if red is not None:   # the synthesis gradients all-reduce during the analysis backward
            red.launch(list(dec.parameters()), _ordered(dec, "", gs))
        rg = [None] * 11
        if g_bpp is not None:
            g_bits = (g_bpp.detach().float() / ctx.pixels).contiguous()
            g_y, rpart = kernels.step_noise_rate_backward(ctx.z, g_y, ctx.steps, ctx.rate, g_bits)
            rg = kernels.rate_param_grads(rpart, be.params_in_order())
        ga = analysis_backward(enc, ctx.saved_a, g_y.contiguous(), mode=ctx.mode)
        names = [n for n, _ in be.named_parameters()]
        rmap = dict(zip(RATE_PARAM_ORDER, rg))
        grads = _ordered(enc, "Encoder.", ga) + _ordered(dec, "Decoder.", gs) + \
            [rmap[n] for n in names]
        if red is not None:
            red.launch(list(enc.parameters()) + list(be.parameters()),
                       _ordered(enc, "", ga) + [rmap[n] for n in names])
        ctx.saved_a = ctx.saved_s = ctx.recon = ctx.z = None
        return (None, None, None, None, None, *grads)


class MsSsimFn(torch.autograd.Function):
    """Per-image MS-SSIM [B] (kernels.ms_ssim, bitwise) with its backward: the forward keeps the
    derivative maps in a workspace (with the dY maps only when Y needs a gradient), the backward
    computes the gradients ``needs_input_grad`` asks for and drops the workspace."""

    @staticmethod
    def forward(ctx, X, Y, data_range):
        ctx.set_materialize_grads(False)
        x, y = X.contiguous(), Y.contiguous()
        ctx.saved_dy = bool(ctx.needs_input_grad[1])
        out, ctx.ws = kernels.ms_ssim_fwd_saved(x, y, data_range, want_dy=ctx.saved_dy)
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            ctx.ws = None
            return None, None, None
        if ctx.ws is None:
            raise RuntimeError("iclr17: ms_ssim_diff was already differentiated (its workspace is "
                               "dropped after the backward)")
        x, y = ctx.saved_tensors
        dx, dy = kernels.ms_ssim_bwd(x, y, ctx.ws, g, ctx.saved_dy,
                                     want_dx=ctx.needs_input_grad[0],
                                     want_dy=ctx.needs_input_grad[1])
        ctx.ws = None
        return dx, dy, None


class SsimFn(torch.autograd.Function):
    """Per-image single-scale (ssim [B], cs [B]) (kernels.ssim, bitwise) with its backward."""

    @staticmethod
    def forward(ctx, X, Y, data_range):
        ctx.set_materialize_grads(False)
        x, y = X.contiguous(), Y.contiguous()
        ctx.saved_dy = bool(ctx.needs_input_grad[1])
        s, cs, ctx.ws = kernels.ssim_fwd_saved(x, y, data_range, want_dy=ctx.saved_dy)
        ctx.save_for_backward(x, y)
        return s, cs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_ssim, g_cs):
        if (g_ssim is None and g_cs is None) or \
                not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            ctx.ws = None
            return None, None, None
        if ctx.ws is None:
            raise RuntimeError("iclr17: ssim_diff was already differentiated (its workspace is "
                               "dropped after the backward)")
        x, y = ctx.saved_tensors
        dx, dy = kernels.ssim_bwd(x, y, ctx.ws, g_ssim, g_cs, ctx.saved_dy,
                                  want_dx=ctx.needs_input_grad[0],
                                  want_dy=ctx.needs_input_grad[1])
        ctx.ws = None
        return dx, dy, None


class AnalysisFn(torch.autograd.Function):
    """Analysis_net_17.forward with autograd: y, contiguous NCHW, from the codec's own analysis
    kernels (``Analysis_net_17.y_nhwc``), so round(y) is the codec's ŷ with grad on or off."""

    @staticmethod
    def forward(ctx, x, enc, mode, *params):
        ctx.set_materialize_grads(False)
        saved = chain.train_mode(mode).train_analysis(enc, x)
        ctx.enc, ctx.saved, ctx.mode = enc, saved, mode
        return enc.y_nhwc(x, mode, feats=saved).permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(ctx, g_y):
        if g_y is None:
            return (None, None, None) + (None,) * len(list(ctx.enc.parameters()))
        ga = analysis_backward(ctx.enc, ctx.saved, g_y.permute(0, 2, 3, 1).contiguous(),
                               want_dx=ctx.needs_input_grad[0], mode=ctx.mode)
        ctx.saved = None
        return (ga.get("x"), None, None, *_ordered(ctx.enc, "", ga))


class SynthesisFn(torch.autograd.Function):
    """Synthesis_net_17.forward with autograd: unclipped reconstruction (NCHW)."""

    @staticmethod
    def forward(ctx, y, dec, mode, *params):
        ctx.set_materialize_grads(False)
        m = chain.train_mode(mode)   # no latent form, no reference: the Decoder on its own
        _, recon, _, saved = m.train_synthesis(dec, dec.to_nhwc(y), None, None)
        ctx.dec, ctx.saved, ctx.mode = dec, saved, mode
        return recon

    @staticmethod
    def backward(ctx, g_recon):
        n_params = len(list(ctx.dec.parameters()))
        if g_recon is None:
            return (None, None, None) + (None,) * n_params
        g_y, gs, _, _ = synthesis_backward(ctx.dec, ctx.saved, g_recon.contiguous(), mode=ctx.mode)
        ctx.saved = None
        return (g_y.permute(0, 3, 1, 2), None, None, *_ordered(ctx.dec, "", gs))
