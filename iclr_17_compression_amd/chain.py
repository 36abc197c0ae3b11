"""The chain of each precision mode (kernels.PRECISIONS), in one place: which kernels its eval and
training forwards launch, which packed parameters they read, which form the latent takes between
the analysis and the synthesis half, (h3) when the chain's range flag is cleared, and which form
a gradient takes between the backward's kernels. ``MODES`` maps the mode string to its object,
``train_mode`` to the one whose training kernels a step runs. Callers read ``kernels.precision()``
once per public call, pick the object and pass it (or its name) down; nothing below them asks
again.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

from torch import Tensor

from . import kernels


def _gdns(net):
    return (net.Encoder.gdn1, net.Encoder.gdn2, net.Decoder.igdn1, net.Decoder.igdn2)


def _latents(operand, y_hat, bits_partial, y, latent) -> Dict[str, object]:
    return {"operand": operand, "y_hat": y_hat, "bits_partial": bits_partial, "y": y,
            "latent": latent}


@dataclass
class AnalysisFeats:
    """What a training analysis forward keeps of x, for conv3 and for the backward: the image, the
    GDN pre-activations, and conv1+GDN1's / conv2+GDN2's outputs in the forms the mode has."""
    x: Tensor
    u1: Tensor
    u2: Tensor
    a1: Optional[Tensor] = None    # fp32 NHWC (fp32, x6)
    a2: Optional[Tensor] = None
    a1s: Optional[Tensor] = None   # x6 split form (x6, h3)
    a2s: Optional[Tensor] = None
    a2h: Optional[Tensor] = None   # h3 form (h3)


@dataclass
class SynthesisSaved:
    """What a training synthesis forward keeps for the backward: the latent, the IGDN
    pre-activations, and deconv1+IGDN1's / deconv2+IGDN2's outputs in the forms the mode has."""
    y: Tensor
    v1: Tensor
    v2: Tensor
    s1: Optional[Tensor] = None    # fp32 NHWC (fp32, x6)
    s2: Optional[Tensor] = None
    ys: Optional[Tensor] = None    # x6 split form (ys: x6; s1s, s2s: x6, h3)
    s1s: Optional[Tensor] = None
    s2s: Optional[Tensor] = None


class _F32Backward:
    """What autograd.analysis_backward / synthesis_backward run over. Between the kernels a
    gradient travels as the pair (fp32 | None, split | None); a weight gradient reads
    ``g[form]``. Exact f32: (fp32, None), the saved fp32 activations, the plain kernels."""
    x6 = False   # also kernels.gdn_param_grads' flag
    form = 0
    wgrad_k5 = staticmethod(kernels.wgrad_k5)
    wgrad_k9 = staticmethod(kernels.wgrad_k9)

    def grad(self, g, g_split=None):
        """An incoming fp32 gradient (and its split form, where its producer made one) → pair."""
        return g, None

    def gdn_params(self, gdn):
        """(β_eff, γ, γᵀ, γ split, γᵀ split) of a layer's fused input-gradient kernel."""
        return (*gdn.effective_params_bwd(), None, None)

    def analysis_operands(self, feats):
        return feats.a1, feats.a2

    def synthesis_operands(self, saved):
        return saved.y, saved.s1, saved.s2

    def layer(self, fn, g, w, pre, p, want_f32=False):
        """bwd_conv_gdn / bwd_deconv_igdn → (the next pair, dn, ∂bias, ∂β_eff); the fp32 half of
        an x6 pair is written only with ``want_f32``."""
        g_f32, dn, db, dbe, *g_split = fn(g[0], w, pre, *p[:3], g_split=g[1], want_split=self.x6,
                                          g6=p[3], g6t=p[4], want_f32=want_f32 or not self.x6)
        return (g_f32, *(g_split or [None])), dn, db, dbe

    def deconv3_layer(self, g_recon, d3, pre, p):
        """bwd_deconv3_igdn with ``d3`` = dec.packed_bwd(x6)[0], the packing of this form."""
        w, w_split = (None, d3) if self.x6 else (d3, None)
        g_f32, dn, db, dbe, *g_split = kernels.bwd_deconv3_igdn(
            g_recon, w, pre, *p[:3], w_split=w_split, want_split=self.x6, g6=p[3], g6t=p[4],
            want_f32=not self.x6)
        return (g_f32, *(g_split or [None])), dn, db, dbe

    def rate_layer(self, g, *args, want_split):
        """bwd_deconv_rate → (∂ỹ fp32, rate partials, ∂ỹ split | None)."""
        g_y, rpart, *g_ys = kernels.bwd_deconv_rate(g[0], *args, g_split=g[1],
                                                    want_split=want_split and self.x6)
        return g_y, rpart, (g_ys or [None])[0]


class _X6Backward(_F32Backward):
    """The x6 contractions on split-form gradients: (fp32 | None, split), the saved split
    activations, the x6 kernels and the split γ packs."""
    x6 = True
    form = 1
    wgrad_k5 = staticmethod(kernels.wgrad_k5_x6)
    wgrad_k9 = staticmethod(kernels.wgrad_k9_x6)

    def grad(self, g, g_split=None):
        return g, (g_split if g_split is not None else kernels.split_planes(g))

    def gdn_params(self, gdn):
        return gdn.effective_params_bwd_x6()

    def analysis_operands(self, feats):
        return feats.a1s, feats.a2s

    def synthesis_operands(self, saved):
        return saved.ys, saved.s1s, saved.s2s


class _H3Backward(_X6Backward):
    """The h3 forward's backward is the x6 one. That forward hands ỹ on in the h3 form only:
    where the x6 forward saved ỹ's split form, this splits ỹ at backward time."""

    def synthesis_operands(self, saved):
        return kernels.split_planes(saved.y), saved.s1s, saved.s2s


class Mode:
    """One precision mode's chain. ``operand``: the keyword under which
    ``Synthesis_net_17.decode`` and ``encode_latents`` carry its latent form (None: the fp32 NHWC
    latent itself). ``train_as``: the mode whose training kernels a step in it runs
    (``train_mode``).

    ``analysis`` → {"y_hat", "bits_partial", "y" (None unless want_y), "latent" (the form
    ``latent_operand`` makes, of ŷ / ỹ; None for fp32, and where not ``want_latent`` lets the mode
    leave it out), "operand" (of the chain that ran)}. ``feats``: ``train_analysis``' record of x
    in the same mode; where its conv2+GDN2 output is this chain's own conv3 operand
    (``conv3_operand``) only conv3 runs, and the chain it began goes on.

    A mode with training kernels also has ``train_analysis(enc, x)`` → AnalysisFeats (conv1+GDN1,
    conv2+GDN2 keeping what the backward needs; h3 begins the chain here), ``train_conv3(enc,
    feats, rate_packed, noise)`` → (ỹ, bit partials, ỹ's latent form | None),
    ``train_synthesis(dec, y_nhwc, latent, x_ref)`` → (clipped, unclipped, SSE partials | None,
    SynthesisSaved) with ``latent`` None for a latent from outside (``latent_operand`` makes the
    form) and the SSE of the unclipped reconstruction, and ``backward``: the object
    autograd.analysis_backward / synthesis_backward run over.

    ``synthesis`` → (clipped NCHW, unclipped | None, SSE partials | None[, bpp total[, per-image
    bit sums]]). ``bits`` = (conv3's bit partials, scale) asks for the total; ``bits_per_image``
    for the per-image sums, which only the h3 kernel has: another mode then folds nothing and
    returns the three values, and the caller reduces the partials.

    ``warm(net, backward)``, inside kernels.batched_packs(): the fp32-derived packs the forward
    reads, with ``backward`` the training step's."""
    name: str
    train_as: str
    operand: Optional[str] = None

    def begin(self, device) -> None:
        """The start of a chain on the current stream of ``device`` (h3: clear the range flag)."""

    def latent_operand(self, y_nhwc):
        """The synthesis input form of an fp32 NHWC latent."""
        return y_nhwc

    def chained_latent(self, y_nhwc):
        """``latent_operand`` of a latent made inside a running chain (the stepped training
        step's ỹ = Δ·z, between ``train_analysis`` and ``train_synthesis``): the chain goes on."""
        return self.latent_operand(y_nhwc)

    def warm_h3(self, net) -> None:
        """Inside kernels.batched_h3_packs(), once ``warm``'s batch is written: the h3 layouts."""

    def warm_eval(self, net) -> None:
        """After both batches, eval only: the round quantiser's rate table."""
        net.bitEstimator.rate_table()


class _Fp32(Mode):
    name = train_as = "fp32"
    backward = _F32Backward()

    def conv3_operand(self, feats):
        return feats.a2

    def train_analysis(self, enc, x):
        w1, w2, _, g1, g2 = enc.packed()
        a1, u1 = kernels.conv1_gdn(x, w1, enc.conv1.bias, g1[0], g1[1], enc.out_channel_N,
                                   want_pre=True)
        a2, u2 = kernels.conv2_gdn(a1, w2, enc.conv2.bias, g2[0], g2[1], want_pre=True)
        return AnalysisFeats(x, u1, u2, a1=a1, a2=a2)

    def train_conv3(self, enc, feats, rate_packed, noise):
        return (*kernels.conv3_quant_rate(self.conv3_operand(feats), enc.packed_w3(), rate_packed,
                                          noise), None)

    def train_synthesis(self, dec, y_nhwc, latent, x_ref):
        d1, d2, d3, q1, q2 = dec.packed()
        s1, v1 = kernels.deconv_igdn(y_nhwc, d1, dec.deconv1.bias, q1[0], q1[1], want_pre=True)
        s2, v2 = kernels.deconv_igdn(s1, d2, dec.deconv2.bias, q2[0], q2[1], want_pre=True)
        out = kernels.deconv3(s2, d3, dec.deconv3.bias, x_ref=x_ref, want_recon=True,
                              sse_unclipped=x_ref is not None)
        return (*out, SynthesisSaved(y_nhwc, v1, v2, s1=s1, s2=s2))

    def analysis(self, enc, x, rate_packed, rtab, noise, want_y, feats=None, want_latent=True):
        w1, w2, w3, g1, g2 = enc.packed()
        if feats is not None:
            h = self.conv3_operand(feats)
        else:
            h = kernels.conv1_gdn(x, w1, enc.conv1.bias, g1[0], g1[1], enc.out_channel_N)
            h = kernels.conv2_gdn(h, w2, enc.conv2.bias, g2[0], g2[1])
        q = kernels.conv3_quant_rate(h, w3, rate_packed, noise, want_y=want_y, rtab=rtab)
        return _latents(None, q[0], q[1], q[2] if want_y else None, None)

    def synthesis(self, dec, y_nhwc, latent, x_ref, want_recon, y_integral, bits, bits_per_image):
        d1, d2, d3, g1, g2 = dec.packed()
        h = kernels.deconv_igdn(y_nhwc, d1, dec.deconv1.bias, g1[0], g1[1])
        h = kernels.deconv_igdn(h, d2, dec.deconv2.bias, g2[0], g2[1])
        out = kernels.deconv3(h, d3, dec.deconv3.bias, x_ref=x_ref, want_recon=want_recon)
        if bits is None or bits_per_image:
            return out
        # the exact-f32 deconv3 has no folded bit reduction: a launch of its own
        return (*out, kernels.reduce_partials(bits[0], bits[1], per_image=False)[1])

    def warm(self, net, backward):
        net.Encoder.packed()
        net.Decoder.packed()
        net.bitEstimator.packed()
        if backward:
            net.Encoder.packed_bwd()
            net.Decoder.packed_bwd(False)
            for g in _gdns(net):
                g.effective_params_bwd()


class _X6(Mode):
    name = train_as = "x6"
    operand = "y_split"
    backward = _X6Backward()

    def latent_operand(self, y_nhwc):
        return kernels.split_planes(y_nhwc)

    def conv3_operand(self, feats):
        return feats.a2s

    def train_analysis(self, enc, x):
        # the kernels also hand conv2 and conv3 (and the weight gradients) their input split
        _, w2, _, _, _ = enc.packed()
        e1, e2 = enc.gdn1.effective_params_x6(), enc.gdn2.effective_params_x6()
        a1s, a1, u1 = kernels.conv1x6_gdn(x, enc.packed_conv1_x6(), enc.conv1.bias, e1[0], e1[2],
                                          enc.out_channel_N, want_f32=True, want_pre=True)
        a2s, a2, u2 = kernels.conv2_gdn_x6(a1s, w2, enc.conv2.bias, *e2, want_f32=True,
                                           want_pre=True)
        return AnalysisFeats(x, u1, u2, a1=a1, a2=a2, a1s=a1s, a2s=a2s)

    def train_conv3(self, enc, feats, rate_packed, noise):
        # not the eval chain's pre-split-weights entry: a step does not warm packed_w3_split
        y_tilde, bits, _, y_split = kernels.conv3_quant_rate_x6(self.conv3_operand(feats),
                                                                enc.packed_w3(), rate_packed, noise)
        return y_tilde, bits, y_split

    def train_synthesis(self, dec, y_nhwc, latent, x_ref):
        d1, d2, _, _, _ = dec.packed()
        if latent is None:
            latent = self.latent_operand(y_nhwc)
        e1, e2 = dec.igdn1.effective_params_x6(), dec.igdn2.effective_params_x6()
        s1s, s1, v1 = kernels.deconv_igdn_x6(latent, d1, dec.deconv1.bias, *e1, want_f32=True,
                                             want_pre=True)
        # NHWC split (not chunk-major): s2s is also deconv3's x6 weight-gradient operand
        s2s, s2, v2 = kernels.deconv_igdn_x6(s1s, d2, dec.deconv2.bias, *e2, want_f32=True,
                                             want_pre=True)
        out = kernels.deconv3_x6(s2s, dec.packed_x6(), dec.deconv3.bias, x_ref=x_ref,
                                 want_recon=True, sse_unclipped=x_ref is not None)
        return (*out, SynthesisSaved(y_nhwc, v1, v2, s1=s1, s2=s2, ys=latent, s1s=s1s, s2s=s2s))

    def analysis(self, enc, x, rate_packed, rtab, noise, want_y, feats=None, want_latent=True):
        _, w2, w3, _, _ = enc.packed()
        if feats is not None:
            hs = self.conv3_operand(feats)
        else:
            e1, e2 = enc.gdn1.effective_params_x6(), enc.gdn2.effective_params_x6()
            hs, _, _ = kernels.conv1x6_gdn(x, enc.packed_conv1_x6(), enc.conv1.bias, e1[0], e1[2],
                                           enc.out_channel_N)
            hs, _, _ = kernels.conv2_gdn_x6(hs, w2, enc.conv2.bias, *e2)
        q = kernels.conv3_quant_rate_x6(hs, w3, rate_packed, noise, want_y=want_y, rtab=rtab,
                                        w_split=enc.packed_w3_split())
        return _latents(_X6.operand, q[0], q[1], q[2], q[3])   # x6's also when bf16 ran this

    def synthesis(self, dec, y_nhwc, latent, x_ref, want_recon, y_integral, bits, bits_per_image):
        d1, d2, _, _, _ = dec.packed()
        q1, q2 = dec.igdn1.effective_params_x6(), dec.igdn2.effective_params_x6()
        hs, _, _ = kernels.deconv_igdn_x6(latent, d1, dec.deconv1.bias, *q1)
        hs, _, _ = kernels.deconv_igdn_x6(hs, d2, dec.deconv2.bias, *q2, chunk_major=True)
        return kernels.deconv3_x6(hs, dec.packed_x6(), dec.deconv3.bias, x_ref=x_ref,
                                  want_recon=want_recon, bits=None if bits_per_image else bits)

    def warm(self, net, backward):
        net.Encoder.packed()
        net.Decoder.packed()
        net.bitEstimator.packed()
        net.Encoder.packed_conv1_x6()
        net.Encoder.packed_w3_split()
        net.Decoder.packed_x6()
        for g in _gdns(net):
            g.effective_params_x6()
        if backward:
            self._warm_backward(net)

    def _warm_backward(self, net):
        net.Encoder.packed_bwd()
        net.Decoder.packed_bwd(True)
        for g in _gdns(net):
            g.effective_params_bwd_x6()


class _H3(_X6):
    """The parity mode on the f16 MFMA: every contraction of the chain in the h3 form (three fp16
    part products per MAC), ŷ handed on in the h3 form. Its backward is the x6 one, and eval
    warms the x6 chain's packs too (evaluate / compress fall back to it on a range overflow)."""
    name = train_as = "h3"
    operand = "y_h3"
    backward = _H3Backward()

    def begin(self, device):
        kernels.h3_chain_begin(device)

    def latent_operand(self, y_nhwc):
        # a latent that enters the synthesis from outside starts a chain of its own
        self.begin(y_nhwc.device)
        return kernels.h3_planes(y_nhwc, cm=kernels.DECONV_CM)

    def chained_latent(self, y_nhwc):
        # no begin(): that would clear a range flag the analysis half had just set
        return kernels.h3_planes(y_nhwc, cm=kernels.DECONV_CM)

    def conv3_operand(self, feats):
        return feats.a2h

    def train_analysis(self, enc, x):
        # the codec's own h3 kernels, which also write the split forms (the x6 weight-gradient
        # operands) and the pre-activations
        self.begin(x.device)
        e1, e2 = enc.gdn1.effective_params_h3(), enc.gdn2.effective_params_h3()
        w2h, _ = enc.packed_h3()
        a1h, _, a1s, u1 = kernels.conv1_gdn_h3(x, enc.packed_conv1_h3(), enc.conv1.bias, *e1,
                                               enc.out_channel_N, want_x6=True, want_pre=True)
        a2h, _, a2s, u2 = kernels.conv2_gdn_h3(a1h, w2h, enc.conv2.bias, *e2, want_x6=True,
                                               want_pre=True)
        return AnalysisFeats(x, u1, u2, a1s=a1s, a2s=a2s, a2h=a2h)

    def train_conv3(self, enc, feats, rate_packed, noise):
        y_tilde, bits, _, y_h3 = kernels.conv3_quant_rate_h3(self.conv3_operand(feats),
                                                             enc.packed_h3()[1], rate_packed, noise)
        return y_tilde, bits, y_h3

    def train_synthesis(self, dec, y_nhwc, latent, x_ref):
        if latent is None:   # the Decoder on its own: its chain starts here
            latent = self.latent_operand(y_nhwc)
        e1, e2 = dec.igdn1.effective_params_h3(), dec.igdn2.effective_params_h3()
        w1, w2, w3 = dec.packed_h3k()
        s1h, _, s1s, v1 = kernels.deconv_igdn_h3(latent, w1, dec.deconv1.bias, *e1, want_x6=True,
                                                 want_pre=True)
        s2h, _, s2s, v2 = kernels.deconv_igdn_h3(s1h, w2, dec.deconv2.bias, *e2, want_x6=True,
                                                 want_pre=True, chunk_major=True)
        out = kernels.deconv3_h3(s2h, w3, dec.deconv3.bias, x_ref=x_ref, want_recon=True,
                                 sse_unclipped=x_ref is not None)
        return (*out, SynthesisSaved(y_nhwc, v1, v2, s1s=s1s, s2s=s2s))

    def analysis(self, enc, x, rate_packed, rtab, noise, want_y, feats=None, want_latent=True):
        w2h, w3h = enc.packed_h3()
        if feats is not None:   # train_analysis began this chain
            hs = self.conv3_operand(feats)
        else:
            self.begin(x.device)
            e1, e2 = enc.gdn1.effective_params_h3(), enc.gdn2.effective_params_h3()
            hs, _ = kernels.conv1_gdn_h3(x, enc.packed_conv1_h3(), enc.conv1.bias, *e1,
                                         enc.out_channel_N)
            hs, _, _ = kernels.conv2_gdn_h3(hs, w2h, enc.conv2.bias, *e2)
        q = kernels.conv3_quant_rate_h3(hs, w3h, rate_packed, noise, want_y=want_y, rtab=rtab,
                                        want_h3=want_latent)
        return _latents(self.operand, q[0], q[1], q[2], q[3])

    def synthesis(self, dec, y_nhwc, latent, x_ref, want_recon, y_integral, bits, bits_per_image):
        q1, q2 = dec.igdn1.effective_params_h3(), dec.igdn2.effective_params_h3()
        w1, w2, w3 = dec.packed_h3k()
        # on ŷ the integer-input form skips the lo products (the same bits: Decoder(round(y))
        # reproduces the codec's reconstruction without knowing its input is ŷ)
        hs, _, _ = kernels.deconv_igdn_h3(latent, w1, dec.deconv1.bias, *q1, int_in=y_integral)
        hs, _, _ = kernels.deconv_igdn_h3(hs, w2, dec.deconv2.bias, *q2, chunk_major=True)
        return kernels.deconv3_h3(hs, w3, dec.deconv3.bias, x_ref=x_ref, want_recon=want_recon,
                                  bits=bits, bits_per_image=bits_per_image)

    def warm(self, net, backward):
        if not backward:
            return super().warm(net, False)
        # an h3 training step reads only these fp32 packings (and has no x6 forward)
        net.Encoder.packed_w3()
        net.Decoder.packed_d3()
        for g in _gdns(net):
            g.effective_params()
        net.bitEstimator.packed()
        self._warm_backward(net)

    def warm_h3(self, net):
        net.Decoder.packed_h3k()
        net.Encoder.packed_h3()
        net.Encoder.packed_conv1_h3()
        for g in _gdns(net):
            g.effective_params_h3()


class _Bf16(_X6):
    """The throughput mode: bf16 activations and weights, one bf16 product per MAC. Its conv3 has
    only the round quantiser and it has no training kernels: with noise, and in a training step
    (``train_as``, ``warm``), the x6 chain runs."""
    name = "bf16"
    operand = "y_bf16"

    def latent_operand(self, y_nhwc):
        return kernels.to_bf16(y_nhwc)

    def analysis(self, enc, x, rate_packed, rtab, noise, want_y, feats=None, want_latent=True):
        if noise is not None:
            return super().analysis(enc, x, rate_packed, rtab, noise, want_y)
        # feats are the x6 training kernels': a different function at bf16 precision, not reused
        w1b, w2b, w3b = enc.packed_bf16()
        e1, e2 = enc.gdn1.effective_params_bf16(), enc.gdn2.effective_params_bf16()
        h = kernels.conv1_gdn_bf16(x, w1b, enc.conv1.bias, *e1, enc.out_channel_N)
        h = kernels.conv2_gdn_bf16(h, w2b, enc.conv2.bias, *e2)
        q = kernels.conv3_quant_rate_bf16(h, w3b, rate_packed, rtab, want_y=want_y)
        return _latents(self.operand, q[0], q[1], q[2], q[3])

    def synthesis(self, dec, y_nhwc, latent, x_ref, want_recon, y_integral, bits, bits_per_image):
        b1, b2, b3 = dec.packed_bf16()
        q1, q2 = dec.igdn1.effective_params_bf16(), dec.igdn2.effective_params_bf16()
        h = kernels.deconv_igdn_bf16(latent, b1, dec.deconv1.bias, *q1)
        h = kernels.deconv_igdn_bf16(h, b2, dec.deconv2.bias, *q2)
        return kernels.deconv3_bf16(h, b3, dec.deconv3.bias, x_ref=x_ref, want_recon=want_recon,
                                    bits=None if bits_per_image else bits)

    def warm_eval(self, net):
        super().warm_eval(net)
        net.Encoder.packed_bf16()
        net.Decoder.packed_bf16()
        for g in _gdns(net):
            g.effective_params_bf16()


MODES: Dict[str, Mode] = {m.name: m for m in (_X6(), _H3(), _Fp32(), _Bf16())}


def train_mode(name: str) -> Mode:
    """The mode object whose training kernels a step in mode ``name`` runs: h3, fp32, or x6 (also
    for bf16)."""
    return MODES[MODES[name].train_as]
