"""The forward chain of each precision mode (kernels.PRECISIONS), in one place: which kernels it
launches, which packed parameters they read, which form the latent takes between the analysis
and the synthesis half, and (h3) when the chain's range flag is cleared. ``MODES`` maps the mode
string to its object. Callers read ``kernels.precision()`` once per public call, pick the object
and pass it (or its name) down; nothing below them asks again.
"""
from __future__ import annotations

from typing import Dict, Optional

from . import kernels


def _gdns(net):
    return (net.Encoder.gdn1, net.Encoder.gdn2, net.Decoder.igdn1, net.Decoder.igdn2)


def _latents(operand, y_hat, bits_partial, y, latent) -> Dict[str, object]:
    return {"operand": operand, "y_hat": y_hat, "bits_partial": bits_partial, "y": y,
            "latent": latent}


class Mode:
    """One precision mode's chain. ``operand``: the keyword under which
    ``Synthesis_net_17.decode`` and ``encode_latents`` carry its latent form (None: the fp32 NHWC
    latent itself). ``train_as``: the mode whose training kernels a step in it runs.

    ``analysis`` → {"y_hat", "bits_partial", "y" (None unless want_y), "latent" (the form
    ``latent_operand`` makes, of ŷ / ỹ; None for fp32, and where not ``want_latent`` lets the mode
    leave it out), "operand" (of the chain that ran)}. ``feats``: the training forward's features
    of x; where its conv2+GDN2 output is this chain's own conv3 operand only conv3 runs.

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

    def warm_h3(self, net) -> None:
        """Inside kernels.batched_h3_packs(), once ``warm``'s batch is written: the h3 layouts."""

    def warm_eval(self, net) -> None:
        """After both batches, eval only: the round quantiser's rate table."""
        net.bitEstimator.rate_table()


class _Fp32(Mode):
    name = train_as = "fp32"

    def analysis(self, enc, x, rate_packed, rtab, noise, want_y, feats=None, want_latent=True):
        w1, w2, w3, g1, g2 = enc.packed()
        if feats is not None:
            h = feats["a2"]
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

    def latent_operand(self, y_nhwc):
        return kernels.split_planes(y_nhwc)

    def analysis(self, enc, x, rate_packed, rtab, noise, want_y, feats=None, want_latent=True):
        _, w2, w3, _, _ = enc.packed()
        if feats is not None:
            hs = feats["a2s"]
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

    def begin(self, device):
        kernels.h3_chain_begin(device)

    def latent_operand(self, y_nhwc):
        # a latent that enters the synthesis from outside starts a chain of its own
        self.begin(y_nhwc.device)
        return kernels.h3_planes(y_nhwc, cm=kernels.DECONV_CM)

    def analysis(self, enc, x, rate_packed, rtab, noise, want_y, feats=None, want_latent=True):
        w2h, w3h = enc.packed_h3()
        if feats is not None:   # the training forward began this chain
            hs = feats["a2h"]
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
