"""Top-level codec — surface of the reference model.py:1-81.

``ImageCompressor(out_channel_N=128)`` owns ``Encoder`` (Analysis_net_17), ``Decoder``
(Synthesis_net_17) and ``bitEstimator`` (BitEstimator) with the reference's state_dict keys,
and ``forward(x) -> (clipped_recon, y_hat, bpp)`` (model.py:47-80). The forward is one chain
of fused gfx950 kernels:

    conv1+GDN → conv2+GDN → conv3+quantise+rate → deconv1+IGDN → deconv2+IGDN →
    deconv3+bias+clamp → deterministic bit reduction

``save_model`` / ``load_model`` keep the reference's file naming and merge semantics
(model.py:18-35).
"""
from __future__ import annotations

import logging  # noqa: F401  (re-exported: train.py uses it via `from model import *`)
import math  # noqa: F401
import os
from typing import Dict, Optional

import numpy as np  # noqa: F401  (re-exported, train.py:117)
import torch
import torch.nn as nn

from . import chain, kernels
from .models import *  # noqa: F401,F403
from .models import Analysis_net_17, BitEstimator, Synthesis_net_17
from .packcache import PackCache


def save_model(model, iter, name):
    """model.py:18-19"""
    torch.save(model.state_dict(), os.path.join(name, "iter_{}.pth.tar".format(iter)))


def load_model(model, f):
    """model.py:22-35: merge the checkpoint's matching keys; always returns step 0 (D7)."""
    with open(f, "rb") as fh:
        pretrained_dict = torch.load(fh, map_location="cpu", weights_only=True)
        model_dict = model.state_dict()
        pretrained_dict = {k: v for k, v in pretrained_dict.items() if k in model_dict}
        model_dict.update(pretrained_dict)
        model.load_state_dict(model_dict)
    return 0


class ImageCompressor(nn.Module):
    def __init__(self, out_channel_N=128):
        super().__init__()
        self.Encoder = Analysis_net_17(out_channel_N=out_channel_N)
        self.Decoder = Synthesis_net_17(out_channel_N=out_channel_N)
        self.bitEstimator = BitEstimator(channel=out_channel_N)
        self.out_channel_N = out_channel_N

    # -------------------------------------------------------------------------------------
    def _latent_noise(self, x: torch.Tensor) -> torch.Tensor:
        # model.py:48-49: U(-0.5, 0.5) of shape [B, N, H//16, W//16] on the device RNG
        B, _, H, W = x.shape
        return torch.empty(B, self.out_channel_N, H // 16, W // 16, device=x.device,
                           dtype=torch.float32).uniform_(-0.5, 0.5)

    def run(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None, training: Optional[bool] = None,
            x_ref_sse: bool = False, want_recon: bool = False,
            want_y: bool = False, mode: Optional[str] = None) -> Dict[str, torch.Tensor]:
        """The fused forward. Returns a dict with ``clipped`` (NCHW), ``y_hat`` (NHWC), bits
        partials and, on request, per-image SSE partials (vs x) and the unclipped recon; in a mode
        whose deconv3 sums the bits per image (h3) also ``bits_per_image``. ``mode``: the
        precision mode (default: kernels.precision(), read once here)."""
        training = self.training if training is None else training
        x = x.contiguous()
        q = self.encode_latents(x, noise, training, want_y, mode or kernels.precision())
        B, _, H, W = x.shape
        # h3: the per-image bit sums folded into deconv3's kernel, which writes them (and every
        # other result) as NaN when a value of the chain did not fit the h3 form
        res = self.Decoder.decode(q["y_hat"], x_ref=x if x_ref_sse else None, want_recon=want_recon,
                                  y_split=q["y_split"], y_bf16=q["y_bf16"], y_h3=q["y_h3"],
                                  y_integral=not training,
                                  bits=(q["bits_partial"], 1.0 / (B * H * W)), bits_per_image=True)
        out = {"y_hat": q["y_hat"], "bits_partial": q["bits_partial"], "y": q["y"],
               "clipped": res[0], "recon": res[1], "sse_partial": res[2]}
        if len(res) == 5:
            out["bits_per_image"] = res[4]
        return out

    def encode_latents(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None,
                       training: bool = False, want_y: bool = False,
                       mode: Optional[str] = None) -> Dict[str, torch.Tensor]:
        """The analysis half of ``run``: conv1+GDN → conv2+GDN → conv3+quantise+rate in ``mode``
        (default: kernels.precision()). Returns ``y_hat`` (NHWC), the bits partials, ``y`` and the
        latent in the form the mode's synthesis reads: ``y_split`` (x6), ``y_h3`` (h3) or
        ``y_bf16`` (bf16), the others None."""
        kernels._check(x, "image", 4)
        if training and noise is None:
            noise = self._latent_noise(x)
        if not training:
            noise = None
        rtab = self.bitEstimator.rate_table() if noise is None else None
        r = chain.MODES[mode or kernels.precision()].analysis(
            self.Encoder, x.contiguous(), self.bitEstimator.packed(), rtab, noise, want_y)
        out = {"y_hat": r["y_hat"], "bits_partial": r["bits_partial"], "y": r["y"],
               "y_split": None, "y_h3": None, "y_bf16": None}
        if r["latent"] is not None:
            out[r["operand"]] = r["latent"]
        return out

    def forward(self, input_image, noise: Optional[torch.Tensor] = None):
        """model.py:47-80 → (clipped_recon, ŷ or ỹ, bpp). In training mode with autograd on, the
        fused training kernels run and every output is differentiable."""
        from .autograd import needs_grad, no_backward
        params = list(self.parameters())
        mode = kernels.precision()
        if self.training and needs_grad(input_image, params):
            clipped, y_tilde, bpp, _ = self._train_outputs(input_image, noise, params, mode)
            return clipped, y_tilde, bpp
        B, _, H, W = input_image.shape
        if not self.training and needs_grad(input_image, params):
            return self._eval_autograd(input_image, mode)
        # run() with bpp's reduction (model.py:71-78) folded into deconv3's kernel
        q = self.encode_latents(input_image.contiguous(), noise, self.training, mode=mode)
        clipped, _, _, bpp = self.Decoder.decode(q["y_hat"], want_recon=False, y_split=q["y_split"],
                                                 y_bf16=q["y_bf16"], y_integral=not self.training,
                                                 bits=(q["bits_partial"], 1.0 / (B * H * W)),
                                                 y_h3=q["y_h3"])
        y_hat = q["y_hat"].permute(0, 3, 1, 2).contiguous()   # NCHW like model.py:56
        clipped = no_backward(clipped, "ImageCompressor (training mode, no grad)", params,
                              input_image)
        return clipped, y_hat, bpp

    def _eval_autograd(self, x, mode):
        """model.py:47-80 in eval mode with autograd on. torch.round (model.py:56) has a zero
        gradient, so nothing flows back into the encoder or the image; the reconstruction is
        differentiable in the synthesis parameters (the fused synthesis forward/backward,
        autograd.SynthesisFn) and the rate in the BitEstimator parameters (model.py:71-78 on
        the module's autograd kernels). The encoder's parameters and the image get no gradient
        where torch would give zeros."""
        B, _, H, W = x.shape
        with torch.no_grad():
            y_hat = self.encode_latents(x, mode=mode)["y_hat"].permute(0, 3, 1, 2).contiguous()
        recon = self.Decoder(y_hat)
        clipped = recon.clamp(0., 1.)                                        # model.py:59
        prob = self.bitEstimator(y_hat + 0.5) - self.bitEstimator(y_hat - 0.5)   # model.py:71-72
        total_bits = torch.sum(torch.clamp(-1.0 * torch.log(prob + 1e-10) / math.log(2.0), 0, 50))
        bpp = total_bits / (B * H * W)                                       # model.py:76-78
        return clipped, y_hat, bpp

    def _train_outputs(self, x, noise, params, mode):
        from .autograd import CodecTrainFn
        kernels._check(x, "image", 4)
        if noise is None:
            noise = self._latent_noise(x)
        self._warm_packs(backward=True, mode=mode)   # one batched pack per parameter update
        return CodecTrainFn.apply(x.contiguous(), noise.contiguous(), self, mode, *params)

    def forward_train(self, input_image, noise: Optional[torch.Tensor] = None,
                      distortion: str = "mse", steps=None):
        """The tuple train.py:97 unpacks, as model.py:81 intends:
        (clipped_recon, mse of the UNclipped recon (model.py:61), bpp), all differentiable.

        ``distortion="ms-ssim"`` returns (clipped_recon, 1 − mean MS-SSIM(clipped_recon, x), bpp)
        instead (losses.ms_ssim_diff on the clipped reconstruction, so the gradient reaches the
        codec's backward through the clamp). In the h3 mode a step whose activations do not fit
        the form has a NaN reconstruction, and so a NaN distortion, as its mse would be.

        ``steps`` (an int, a sequence or an integer tensor of B codec.step_size indices 0..31)
        trains along the quantiser-step ladder: image b is quantised with the
        noise proxy of the coder's convention at Δ_b, z = y/Δ_b + u, synthesised from Δ_b·z, and
        its bits are the step pack's on z. The return is then per image, (clipped_recon,
        dist [B], bpp [B]), all differentiable in the parameters; ``x.requires_grad`` is not
        supported with ``steps``."""
        if distortion not in ("mse", "ms-ssim"):
            raise kernels.Iclr17Error(f"iclr17: distortion must be 'mse' or 'ms-ssim' "
                                      f"(got {distortion!r})")
        if steps is not None:
            return self._forward_train_steps(input_image, noise, distortion, steps)
        clipped, _, bpp, mse = self._train_outputs(input_image, noise, list(self.parameters()),
                                                   kernels.precision())
        if distortion == "ms-ssim":
            from .losses import ms_ssim_diff
            return clipped, 1 - ms_ssim_diff(clipped, input_image, data_range=1.0), bpp
        return clipped, mse, bpp

    @staticmethod
    def _step_indices(steps, B: int):
        """``forward_train``'s ``steps`` → B ladder indices, checked on the host."""
        from . import codec
        if isinstance(steps, torch.Tensor):
            if steps.dtype.is_floating_point or steps.dtype in (torch.bool, torch.complex64,
                                                                torch.complex128):
                raise kernels.Iclr17Error(f"iclr17: forward_train: steps must be an integer tensor "
                                          f"(got {steps.dtype})")
            idx = [int(v) for v in steps.detach().reshape(-1).cpu().tolist()]
        elif isinstance(steps, (int, np.integer)) and not isinstance(steps, bool):
            idx = [int(steps)] * B
        else:
            try:
                idx = list(steps)
            except TypeError:
                raise kernels.Iclr17Error(f"iclr17: forward_train: steps must be an int, a sequence "
                                          f"or an integer tensor (got {steps!r})") from None
        if len(idx) != B:
            raise kernels.Iclr17Error(f"iclr17: forward_train: {len(idx)} steps for a batch of {B} "
                                      "images")
        for s in idx:
            codec.step_size(s)   # raises on anything but an integer in 0..31
        return [int(s) for s in idx]

    def _forward_train_steps(self, x, noise, distortion, steps):
        from . import codec
        from .autograd import StepTrainFn
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise kernels.Iclr17Error("iclr17: forward_train: the image batch must be a 4-D tensor")
        idx = self._step_indices(steps, x.shape[0])
        if x.requires_grad:
            raise kernels.Iclr17Error("iclr17: forward_train: steps with an image that requires a "
                                      "gradient is not supported")
        kernels._check(x, "image", 4)
        if noise is None:
            noise = self._latent_noise(x)
        mode = kernels.precision()
        self._warm_packs(backward=True, mode=mode)
        steps_dev = torch.tensor([codec.step_size(s) for s in idx], dtype=torch.float32).to(
            x.device, non_blocking=True)
        clipped, bpp, mse = StepTrainFn.apply(x.contiguous(), noise.contiguous(), steps_dev, self,
                                              mode, *self.parameters())
        if distortion == "ms-ssim":
            from .losses import ms_ssim_diff
            return clipped, 1 - ms_ssim_diff(clipped, x, data_range=1.0, size_average=False), bpp
        return clipped, mse, bpp

    # ------------------------------------------------------------- rate control (codec.py)
    @torch.no_grad()
    def latents(self, x: torch.Tensor) -> torch.Tensor:
        """The unquantised latent y of an image batch, fp32 NHWC [B, H/16, W/16, N]: the analysis
        transform of the current precision mode (its conv3 rounds this very y to ŷ), with
        ``compress``'s fall-back to the x6 chain when an activation does not fit the h3 form."""
        mode = kernels.precision()
        y = self.encode_latents(x, want_y=True, mode=mode)["y"]
        if mode == "h3" and kernels.h3_range_overflowed(x.device):
            with kernels.precision_scope("x6"):
                y = self.encode_latents(x, want_y=True)["y"]
        return y

    @torch.no_grad()
    def synthesis_gains(self) -> torch.Tensor:
        """The channel weights of rate–distortion optimised quantisation: fp32 [N]
        on the device, g_c = Σ over pixels of (synthesis of a unit impulse in channel c at the
        centre of an 8×8 zero latent − synthesis of the zero latent)², unclipped, normalised to
        mean 1. One Decoder call on N + 1 latents (the response is 57 pixels wide and fits the
        128×128 output), in the x6 mode whatever the current one; a linearisation of the synthesis
        at zero and no more. Cached until a parameter changes."""
        sd = self.state_dict()
        keys = sorted(sd)
        cache = self.__dict__.setdefault("_codec_cache", PackCache())

        def build() -> torch.Tensor:
            g = self.synthesis_gains_raw()
            return (g / g.mean()).contiguous()

        return cache.get("synthesis_gains", [sd[k] for k in keys], build)

    @torch.no_grad()
    def synthesis_gains_raw(self) -> torch.Tensor:
        """``synthesis_gains`` before its division by the mean: fp32 [N] on the device, g_c in
        squared pixel units (of the [0, 1] range) per unit squared latent error, the default
        weights of ``distortion_sweep``. Cached until a parameter changes."""
        sd = self.state_dict()
        keys = sorted(sd)
        cache = self.__dict__.setdefault("_codec_cache", PackCache())

        def build() -> torch.Tensor:
            N = self.out_channel_N
            dev = next(self.parameters()).device
            probe = torch.zeros(N + 1, N, 8, 8, device=dev, dtype=torch.float32)
            probe[torch.arange(N), torch.arange(N), 4, 4] = 1.0
            with kernels.precision_scope("x6"):
                out = self.Decoder(probe)
            return ((out[:N] - out[N:]) ** 2).sum(dim=(1, 2, 3)).contiguous()

        return cache.get("synthesis_gains_raw", [sd[k] for k in keys], build)

    @torch.no_grad()
    def distortion_sweep(self, x_or_y: torch.Tensor, steps=range(32), weights=None,
                         latent: Optional[bool] = None) -> torch.Tensor:
        """The weighted squared quantisation error of every image's latent at every ladder step of
        ``steps`` (codec.step_size indices, at most 32): float64 [B, S] on the device, E[b][s] =
        Σ w_c·(Δ_s·rint(y/Δ_s) − y)², from one analysis pass and one read of y
        (kernels.distortion_sweep). The argument as ``rate_sweep``'s; ``weights``: [N] channel
        weights, finite and ≥ 0, default ``synthesis_gains_raw`` — E is then the linearised
        synthesis's prediction of the squared pixel error a step adds (it orders
        the probes of a quality target and decides nothing)."""
        from . import codec
        kernels._check(x_or_y, "image or latent", 4)
        if latent is None:
            latent = x_or_y.shape[1] != 3
        y = x_or_y if latent else self.latents(x_or_y)
        N = self.out_channel_N
        if y.shape[3] != N:
            raise kernels.Iclr17Error(f"iclr17: distortion_sweep: the latent has {y.shape[3]} "
                                      f"channels, the model {N}")
        if weights is None:
            g = self.synthesis_gains_raw()
        else:
            g = torch.as_tensor(weights, dtype=torch.float32).to(y.device)
            if tuple(g.shape) != (N,):
                raise kernels.Iclr17Error(f"iclr17: distortion_sweep: weights must have shape "
                                          f"[{N}] (got {tuple(g.shape)})")
        return kernels.distortion_sweep(y, g.contiguous(), [codec.step_size(s) for s in steps])

    def _rdo_lam(self, rdo, rdo_weights, what: str) -> torch.Tensor:
        """lam[c] = rdo · weight_c for kernels.quantise_rdo / rate_sweep_rdo: fp32 [N] on the
        device; the weights default to ``synthesis_gains``."""
        from . import codec
        lam = codec.rdo_value(rdo)
        N = self.out_channel_N
        dev = next(self.parameters()).device
        if rdo_weights is None:
            g = self.synthesis_gains()
        else:
            g = torch.as_tensor(rdo_weights, dtype=torch.float32).to(dev)
            if tuple(g.shape) != (N,):
                raise kernels.Iclr17Error(f"iclr17: {what}: rdo_weights must have shape [{N}] "
                                          f"(got {tuple(g.shape)})")
        return (g * lam).contiguous()

    @torch.no_grad()
    def rate_sweep(self, x_or_y: torch.Tensor, steps=range(32),
                   latent: Optional[bool] = None, rdo=None, rdo_weights=None) -> torch.Tensor:
        """Estimated bits of every image at every ladder step of ``steps`` (codec.step_size
        indices, at most 32): float64 [B, S] on the device, from one analysis pass and one read
        of y (kernels.rate_sweep). The argument is an image batch [B,3,H,W] or, with a second
        dimension other than 3 or ``latent=True``, the NHWC latent of ``latents``. With ``rdo``
        (λ ≥ 0; ``rdo_weights``: [N] channel weights, default ``synthesis_gains``) the bits of the
        rate–distortion optimised levels (kernels.rate_sweep_rdo)."""
        from . import codec
        lam = None if rdo is None else self._rdo_lam(rdo, rdo_weights, "rate_sweep")
        kernels._check(x_or_y, "image or latent", 4)
        if latent is None:
            latent = x_or_y.shape[1] != 3
        y = x_or_y if latent else self.latents(x_or_y)
        if y.shape[3] != self.out_channel_N:
            raise kernels.Iclr17Error(f"iclr17: rate_sweep: the latent has {y.shape[3]} channels, "
                                      f"the model {self.out_channel_N}")
        if lam is not None:
            return kernels.rate_sweep_rdo(y, self.bitEstimator.packed(),
                                          [codec.step_size(s) for s in steps], lam)
        return kernels.rate_sweep(y, self.bitEstimator.packed(),
                                  [codec.step_size(s) for s in steps])

    @torch.no_grad()
    def rate_sweep_offsets(self, y: torch.Tensor, offsets, block: int = 4) -> torch.Tensor:
        """``rate_sweep`` of the NHWC latent ``y`` at all 32 BASE indices with a ladder offset per
        block (``offsets``: integers [B, mh, mw], codec.map_shape): float64 [B, 32], row s summing
        every element at index clamp(s + offset, 0, 31) (kernels.rate_sweep_offsets)."""
        from . import codec
        kernels._check(y, "latent", 4)
        if y.shape[3] != self.out_channel_N:
            raise kernels.Iclr17Error(f"iclr17: rate_sweep_offsets: the latent has {y.shape[3]} "
                                      f"channels, the model {self.out_channel_N}")
        return kernels.rate_sweep_offsets(y, self.bitEstimator.packed(),
                                          [codec.step_size(s) for s in range(codec.STEPS)],
                                          offsets, block)

    def _map_tables(self, step_map, K):
        """A step map's ladder indices [B, mh, mw] → (the stacked tables of the indices it uses,
        ascending, and the map translated to their slots)."""
        m = np.asarray(step_map)
        if m.dtype.kind not in "iu" or m.ndim != 3 or not m.size or m.min() < 0 or m.max() > 31:
            raise kernels.Iclr17Error("iclr17: step_map must be ladder indices 0..31 of shape "
                                      f"[B, mh, mw] (got {m.dtype} {m.shape})")
        used = [int(e) for e in np.unique(m)]
        slot = np.zeros(32, dtype=np.uint8)
        slot[used] = np.arange(len(used), dtype=np.uint8)
        return self.bitEstimator.stacked_tables(K, used), slot[m]

    @torch.no_grad()
    def compress_latents(self, y: torch.Tensor, step: Optional[int],
                         streams_per_image: int = kernels.STREAMS_PER_IMAGE,
                         K: int = kernels.ENTROPY_K, step_map=None,
                         block: int = 4, rdo=None, rdo_weights=None,
                         tile: Optional[int] = None) -> Dict[str, object]:
        """``compress`` from the latent of ``latents`` at ladder step ``step``: ŷ = rint(y/Δ)
        (kernels.quantise_step), then rANS with the step's tables. Returns ``compress``'s dict and
        "y_hat" (NHWC). With ``step_map`` (ladder indices per block, integers [B, mh, mw] for
        blocks of ``block``×``block`` latent positions; ``step`` is then None) every block is
        quantised at its own step and coded with that step's tables (kernels.quantise_step_map,
        kernels.rans_encode_map).

        With ``rdo`` (λ ≥ 0, finite; ``rdo_weights``: [N] channel weights, default
        ``synthesis_gains``) the levels are rate–distortion optimised (kernels.quantise_rdo,
        DESIGN.md §0j) and coded with the step's same tables; the dict gains "est_bits", the
        model's estimate of ŷ per image (float64 [B] on the device). Not with ``step_map``.

        With ``tile`` (8, 16, 32 or 64) the same ŷ is coded with a stream per tile of
        ``tile``×``tile`` latent positions and channel group (kernels.rans_encode_tiled, DESIGN.md
        §0k): a string then holds th·tw·P word counts, in (tile row, tile column, group) order,
        and the words. Not with ``step_map``."""
        from . import codec
        if tile is not None and step_map is not None:
            raise kernels.Iclr17Error(codec.TILE_WITH_MAP)
        if rdo is not None:
            if step_map is not None:
                raise kernels.Iclr17Error(codec.RDO_WITH_MAP)
            lam = self._rdo_lam(rdo, rdo_weights, "compress_latents")
            y_hat, _, est = kernels.quantise_rdo(y, self.bitEstimator.packed(),
                                                 codec.step_size(step), lam)
            enc = self._entropy_code(y_hat, self.bitEstimator.entropy_tables(K, step=step),
                                     streams_per_image, K, tile=tile)
            enc["est_bits"] = est
            return enc
        if step_map is None:
            y_hat, _ = kernels.quantise_step(y, codec.step_size(step))
            return self._entropy_code(y_hat, self.bitEstimator.entropy_tables(K, step=step),
                                      streams_per_image, K, tile=tile)
        if step is not None:
            raise kernels.Iclr17Error("iclr17: compress_latents: step and step_map given together")
        tables, slots = self._map_tables(step_map, K)
        y_hat, _ = kernels.quantise_step_map(y, step_map, block,
                                             [codec.step_size(s) for s in range(codec.STEPS)])
        return self._entropy_code(y_hat, tables, streams_per_image, K, slots, block)

    def _entropy_code(self, y_hat, tables, P, K, slots=None, block=None, tile=None):
        B, h, w, N = y_hat.shape
        S = P   # streams per image
        if tile is not None:
            th, tw = kernels.tile_grid(h, w, tile)
            S = th * tw * P
            words, offsets = kernels.rans_encode_tiled(y_hat, tables, tile, K, P)
        elif slots is None:
            words, offsets = kernels.rans_encode(y_hat, tables, K, P)
        else:
            words, offsets = kernels.rans_encode_map(y_hat, tables, slots, block, K, P)
        off = offsets.cpu().numpy()
        wv = words.cpu().numpy().view("<u2")
        strings = []
        for b in range(B):
            o = off[b * S:(b + 1) * S + 1]
            strings.append(np.diff(o).astype("<u4").tobytes() + wv[o[0]:o[-1]].tobytes())
        return {"strings": strings, "shape": (h, w), "streams_per_image": P, "K": K,
                "y_hat": y_hat}

    # ------------------------------------------------------------- entropy coding (§8 f4)
    @torch.no_grad()
    def compress(self, x: torch.Tensor, streams_per_image: int = kernels.STREAMS_PER_IMAGE,
                 K: int = kernels.ENTROPY_K, tile: Optional[int] = None) -> Dict[str, object]:
        """Encode images to byte strings: the analysis transform, rounding, then rANS over the
        factorised BitEstimator (the model the reference uses only to estimate bpp). Per image:
        P little-endian uint32 stream word counts, then the stream words (uint16 LE).
        Returns {"strings": [bytes] * B, "shape": (h, w), "streams_per_image": P, "K": K}.
        With ``tile`` the same ŷ in tiled streams, as ``compress_latents(tile=)`` lays them out."""
        mode = kernels.precision()
        y_hat = self.encode_latents(x, mode=mode)["y_hat"]
        if mode == "h3" and kernels.h3_range_overflowed(x.device):
            # an activation did not fit the h3 form (conv3 wrote ŷ as NaN): encode from the x6
            # chain's ŷ instead (full fp32 operands). The flag read is one synchronisation, and
            # the stream sizes below synchronise anyway.
            with kernels.precision_scope("x6"):
                y_hat = self.encode_latents(x)["y_hat"]
        enc = self._entropy_code(y_hat, self.bitEstimator.entropy_tables(K), streams_per_image, K,
                                 tile=tile)
        del enc["y_hat"]
        return enc

    @torch.no_grad()
    def decompress(self, strings, shape, streams_per_image: int = kernels.STREAMS_PER_IMAGE,
                   K: int = kernels.ENTROPY_K, device=None, step: Optional[int] = None,
                   step_map=None, block: int = 4,
                   tile: Optional[int] = None, recon=None,
                   recon_strength=1.0) -> Dict[str, torch.Tensor]:
        """Inverse of ``compress``: byte strings → {"y_hat": NCHW latents, "x_hat": the clipped
        reconstruction} (bit-identical latents; the synthesis as in ``forward``). With ``step``
        the inverse of ``compress_latents`` at that ladder step: the step's tables decode ŷ, and
        the synthesis runs on Δ·ŷ as a general (non-integer) latent. With ``step_map`` /
        ``block`` the inverse of ``compress_latents(step_map=…)``; with ``tile`` the inverse of
        ``compress`` / ``compress_latents`` with that tile edge.

        ``recon`` / ``recon_strength`` (codec.recon_value): "centroid" places every
        level at ``recon_strength`` of the way from its bin's centre to the bin's mean under the
        rate model, "zero" the zero bin alone; the synthesis then runs on Δ·(ŷ + offset)
        (kernels.dequantise_recon / dequantise_recon_map; a plain stream counts as ladder index
        8). None and "centre" are the call without them: no other kernel, the same bytes."""
        from . import codec
        rc = codec.recon_value(recon, recon_strength)   # before any device use
        if step is not None and step_map is not None:
            raise kernels.Iclr17Error("iclr17: decompress: step and step_map given together")
        P, N = streams_per_image, self.out_channel_N
        h, w = shape
        if tile is not None:
            if step_map is not None:
                raise kernels.Iclr17Error(codec.TILE_WITH_MAP)
            th, tw = kernels.tile_grid(h, w, tile)
            P = th * tw * streams_per_image   # streams per image
        device = device or next(self.parameters()).device
        counts, payload = [], []
        for sbytes in strings:
            head = np.frombuffer(sbytes[:4 * P], dtype="<u4")
            if head.size != P:
                raise kernels.Iclr17Error("iclr17: decompress: truncated stream header")
            body = np.frombuffer(sbytes[4 * P:], dtype="<u2")
            if body.size != int(head.sum()):
                raise kernels.Iclr17Error("iclr17: decompress: stream lengths do not match the payload")
            counts.append(head.astype(np.int64))
            payload.append(body)
        B = len(strings)
        off = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
        words = torch.from_numpy(np.concatenate(payload).view(np.int16).copy()).to(device)
        offsets = torch.from_numpy(off).to(device)
        if tile is not None:
            y_hat = kernels.rans_decode_tiled(words, offsets,
                                              self.bitEstimator.entropy_tables(K, step=step),
                                              B, h, w, N, tile, K, streams_per_image)
        elif step_map is None:
            y_hat = kernels.rans_decode(words, offsets,
                                        self.bitEstimator.entropy_tables(K, step=step),
                                        B, h, w, N, K, P)
        else:
            tables, slots = self._map_tables(step_map, K)
            y_hat = kernels.rans_decode_map(words, offsets, tables, slots, block, B, h, w, N, K, P)
        m = chain.MODES[kernels.precision()]
        if step_map is not None:
            if rc is None:
                y_deq = kernels.dequantise_step_map(y_hat, step_map, block,
                                                    [codec.step_size(s) for s in range(codec.STEPS)])
            else:   # _map_tables' slots: the indices the map uses, ascending
                used = [int(e) for e in np.unique(np.asarray(step_map))]
                y_deq = kernels.dequantise_recon_map(
                    y_hat, slots, block, [codec.step_size(s) for s in used],
                    self.bitEstimator.stacked_recon_offsets(K, used, *rc), K)
            clipped, _, _ = m.synthesis(self.Decoder, y_deq, m.latent_operand(y_deq), None, False,
                                        False, None, False)
        elif rc is not None:
            e = codec.UNIT_STEP if step is None else step
            y_deq = kernels.dequantise_recon(y_hat, codec.step_size(e),
                                             self.bitEstimator.recon_offsets(K, e, *rc), K)
            clipped, _, _ = m.synthesis(self.Decoder, y_deq, m.latent_operand(y_deq), None, False,
                                        False, None, False)
        elif step is None:
            clipped, _, _ = m.synthesis(self.Decoder, y_hat, m.latent_operand(y_hat), None, False,
                                        True, None, False)
        else:
            y_deq = kernels.dequantise_step(y_hat, codec.step_size(step))
            clipped, _, _ = m.synthesis(self.Decoder, y_deq, m.latent_operand(y_deq), None, False,
                                        False, None, False)
        return {"y_hat": y_hat.permute(0, 3, 1, 2).contiguous(), "x_hat": clipped}

    # ------------------------------------------------------------- image files (§1 f5, codec.py)
    @torch.no_grad()
    def compress_images(self, images, max_batch: int = 64,
                        streams_per_image: int = kernels.STREAMS_PER_IMAGE,
                        K: int = kernels.ENTROPY_K, step: Optional[int] = None,
                        max_bytes=None, bpp=None, stats: Optional[dict] = None,
                        step_offsets=None, block: int = 4, rdo=None, rdo_weights=None,
                        tile: Optional[int] = None, psnr=None, estimate: Optional[bool] = None,
                        msssim=None, refine=None, refine_lambda=None, refine_lr=None):
        """8-bit images of any sizes ≥ 1×1 (a sequence of uint8 HWC RGB arrays, numpy or torch) →
        one self-describing blob per image, in input order: codec.py's 28-byte header (true size,
        N, P, K, weights fingerprint) + the image's ``compress`` string. Images are batched by
        canvas (the size rounded up to multiples of 16, edges replicated), at most ``max_batch``
        per batch; each batch is one pinned upload, kernels.image_ingest and ``compress`` as it
        stands (its x6 fall-back on an h3 overflow included). The precision mode is not recorded:
        the latents decode bit-exactly in every mode, decoded pixels may differ by one 8-bit step
        between modes, and within one mode a blob does not depend on its batch.

        At most one of ``step`` / ``max_bytes`` / ``bpp`` selects another rate from the same
        weights (codec.py, "Quantiser steps"): ``step`` a ladder index 0..31 (8 is Δ = 1),
        ``max_bytes`` a byte budget on the whole blob and ``bpp`` one of ⌊bpp·H·W/8⌋ bytes, each
        a scalar or one value per image; a budget picks per image the finest step that fits.
        These blobs carry the magic I17Q and their step; ``stats`` (a dict) receives
        "reencodes", the budget loop's re-encodes per image.

        ``step_offsets`` codes regions of interest (codec.py, "Step maps"): per image None or a
        signed integer offset per block of ``block``×``block`` latent positions ([mh, mw],
        codec.map_shape; codec.roi_offsets makes one from pixel boxes). A block is coded at
        ladder index clamp(base + offset, 0, 31), the base being ``step``, what a budget picks,
        or 8; these blobs carry the magic I17M and their map. No quality claim is made.

        ``rdo`` (λ ≥ 0, finite) quantises rate–distortion optimised (codec.py, "RDO"): each
        level is the cheapest of rint(y/Δ), its neighbour toward zero and zero under
        bits + λ·g_c·Δ²·error², with ``rdo_weights`` [N] as g (default ``synthesis_gains``). It goes
        with ``step`` or a budget and alone means the unit step; the blobs are ordinary I17Q ones
        and record nothing of it. With ``step_offsets`` it raises (per-block RDO is not built).

        ``tile`` (8, 16, 32 or 64 latent positions, 16 pixels each; None: today's streams) codes
        the same latents with an independent stream per tile and channel group (codec.py, "Tiled
        streams"): many waves code one large image, and ``decompress_region`` decodes a pixel box
        from the tiles it needs alone. It goes with ``step``, a budget (the tile overhead
        counted) and ``rdo``; alone it codes ``compress``'s own ŷ. These blobs carry the magic
        I17T, a ladder index (8 when no rate option is given) and the tile edge. With
        ``step_offsets`` it raises (tiled step maps are not built).

        ``psnr`` (dB, finite and > 0; a scalar or one value per image) is a quality target, the
        fourth rate option (codec.py, "Quality targets"): each image is coded at the coarsest
        ladder index found whose 8-bit decode reaches the target, decided on the integer SSE
        against codec.sse_limit; the index passed, and it is 31 or its coarser neighbour was
        measured and failed. At most 8 probes per image, each a quantise–synthesis–SSE pass on
        the device without entropy coding; ``estimate=True`` orders them by
        ``distortion_sweep``'s prediction, False bisects (None: codec.DEFAULT_ESTIMATE, which is
        bisection). The blobs are byte for byte those of ``step=`` at the index found (I17Q, or I17T with ``tile``); ``stats`` receives
        "probes" and "sse" (the SSE at the index) per image. A target above what index 0 reaches
        raises; with ``rdo`` or ``step_offsets`` it raises (not built).

        ``msssim`` (0 < T < 1; a scalar or one value per image) is the same target in MS-SSIM, the
        fifth rate option (codec.py, "MS-SSIM targets"): an index passes when the
        fp32 MS-SSIM of its 8-bit decode over the image's own H×W is ≥ T. Plain bisection, at most
        6 probes per image, each a quantise–synthesis–MS-SSIM pass on the device
        (kernels.image_msssim); ``stats`` receives "probes" and "ms_ssim" (the value at the index,
        which is ``evaluate_images``' ``ms_ssim`` of the blob). Both sides of every image must be
        at least 161; with another rate option, ``rdo``, ``step_offsets`` or ``estimate=True`` it
        raises.

        ``refine`` (K ≥ 0 gradient iterations; 0 and None: today's code and bytes) refines the
        latent of each image before it is coded (codec.py, "Latent refinement"):
        Adam steps on y lower J = bits + (λ/3)·SSE8/255² through the real synthesis and the real
        rate model, straight through the rounding, and the best ŷ seen is coded where its 8-bit
        decode has a strictly lower J than the plain one. ``refine_lambda`` (finite, ≥ 0; a scalar
        or one value per image; required) is λ in train.py's units (λ·mse + bpp), ``refine_lr`` the
        Adam learning rate in units of Δ (None: codec.DEFAULT_REFINE_LR). It goes with ``step``
        (none given: index 8) and ``tile``; the blobs are ordinary I17Q / I17T ones and any decoder
        reads them. With a budget, a quality target, ``rdo`` or ``step_offsets`` and in the bf16
        mode it raises. ``stats`` receives "refine_kept", "objective", "objective_plain" and
        "refine_iters" per image.

        ``refine_lambda=codec.msssim_lambda(λ)`` (a scalar or one per image; not mixed with plain
        values) makes the distortion MS-SSIM: J = bits + λ·H·W·(1 − MS-SSIM8),
        λ in the units of train.py's λ·(1 − MS-SSIM) + bpp. Both sides of every image must then be
        at least 161, and ``stats`` also receives "refine_distortion" ("ms-ssim"), "ms_ssim" and
        "ms_ssim_plain", the judged values."""
        from . import codec
        return codec.compress_images(self, images, max_batch, streams_per_image, K, step=step,
                                     max_bytes=max_bytes, bpp=bpp, stats=stats,
                                     step_offsets=step_offsets, block=block, rdo=rdo,
                                     rdo_weights=rdo_weights, tile=tile, psnr=psnr,
                                     estimate=codec.DEFAULT_ESTIMATE if estimate is None else estimate,
                                     msssim=msssim, refine=refine, refine_lambda=refine_lambda,
                                     refine_lr=refine_lr)

    @torch.no_grad()
    def refine_latents(self, y: torch.Tensor, steps, refine_lambda, packed, offsets, shapes,
                       refine: int, refine_lr=None, stats: Optional[dict] = None) -> torch.Tensor:
        """Latent refinement of one canvas batch → the ŷ to code, fp32 NHWC,
        integer-valued. ``y``: the batch's latent (``latents``); ``steps``: a ladder index or one
        per image; ``refine_lambda``: λ, a scalar or one per image; ``packed`` / ``offsets`` /
        ``shapes``: the 8-bit originals on the device as codec.upload_packed returns them (all of
        one canvas); ``refine``: the iterations K; ``refine_lr``: the learning rate in units of Δ
        (None: codec.DEFAULT_REFINE_LR). K + 1 passes of quantiser, training forward of the
        synthesis, 8-bit SSE and keep-the-best with K data-gradient backwards between them, no
        host synchronisation inside (codec.refine_loop); then the best iterate and the plain
        ŷ = rint(y/Δ) are judged through the eval chain, and the best is returned only where its
        J = bits + (λ/3)·SSE8/255² is strictly lower. ``stats`` as in ``compress_images``. Not in the
        bf16 mode. With codec.msssim_lambda values the distortion is MS-SSIM, as there."""
        from . import codec
        B = y.shape[0]
        idx = self._step_indices(steps, B)
        lams = codec._per_image("refine_lambda", refine_lambda, B, codec.refine_lambda_value)
        return codec.refine_latents(self, y, idx, lams, packed, offsets, shapes, refine,
                                    refine_lr, stats)

    @torch.no_grad()
    def decompress_images(self, blobs, max_batch: int = 64, recon=None, recon_strength=1.0):
        """Inverse of ``compress_images``: blobs → uint8 HWC numpy arrays of the true sizes, in
        input order (``decompress`` per canvas batch, then kernels.image_egress: round-half-even of
        the clipped reconstruction·255, cropped). Plain (I17C), stepped (I17Q), mapped (I17M) and
        tiled (I17T) blobs may be mixed; a batch holds blobs of one canvas, P, K and step (mapped
        ones: of one block edge; tiled ones: of one tile edge). Raises Iclr17Error on a foreign or truncated blob, a corrupt step map,
        another N or other weights (the header's fingerprint). Within one precision mode
        the bytes are reproducible and independent of the batch; between modes a pixel may differ
        by one 8-bit step. ``recon`` / ``recon_strength`` as ``decompress`` takes them, for every
        blob of the call whatever its kind."""
        from . import codec
        return codec.decode_groups(self, list(blobs), max_batch, recon=recon,
                                   recon_strength=recon_strength)[0]

    @torch.no_grad()
    def decompress_region(self, blob, box, stats: Optional[dict] = None, recon=None,
                          recon_strength=1.0):
        """The pixels ``box`` = (x0, y0, x1, y1) (half-open, inside the image) of one blob → uint8
        [y1 − y0, x1 − x0, 3], byte for byte ``decompress_images([blob])[0][y0:y1, x0:x1]``. Of a
        tiled (I17T) blob only the streams of the tiles that cover the latent positions the box
        depends on (codec.region_window) are decoded, and the synthesis runs on that rectangle of
        the latent as an image of its own; any other blob is decoded whole. ``stats`` (a dict)
        receives "streams_decoded" and "streams_total". ``recon`` / ``recon_strength`` as
        ``decompress_images`` takes them; the equality above holds with the same two arguments on
        both sides."""
        from . import codec
        return codec.decode_region(self, blob, box, stats, recon=recon,
                                   recon_strength=recon_strength)

    @torch.no_grad()
    def evaluate_images(self, images, want_msssim: bool = False, max_batch: int = 64,
                        step: Optional[int] = None, max_bytes=None, bpp=None, step_offsets=None,
                        block: int = 4, rdo=None, rdo_weights=None, tile: Optional[int] = None,
                        psnr=None, estimate: Optional[bool] = None, recon=None,
                        recon_strength=1.0, msssim=None, refine=None, refine_lambda=None,
                        refine_lr=None):
        """The real codec path per image, compress_images then decompress_images, measured on
        the 8-bit decoded image as codecs are reported: a dict per image with ``bytes``, ``bpp`` =
        8·len(blob)/(H·W) (header included, true pixel count), ``sse_u8`` (int), ``psnr_u8`` =
        10·log10(255²·3HW / sse_u8) (float64; inf at 0), ``recon`` (uint8 HWC) and, with
        ``want_msssim``, ``ms_ssim`` / ``ms_ssim_db`` of the cropped pair (None for an image too
        small for 5 levels) and ``step`` (the blob's ladder step; None for a plain blob).
        ``step`` / ``max_bytes`` / ``bpp`` / ``step_offsets`` / ``block`` / ``rdo`` /
        ``rdo_weights`` as in ``compress_images``; a mapped blob's row has its base index as
        ``step`` and also ``step_map`` and ``block``; with ``tile`` a row has the blob's ladder
        index as ``step`` and also ``tile``. ``psnr`` / ``estimate`` as in ``compress_images``: the
        row's ``step`` is the index found; so is ``msssim``, whose rows also carry ``ms_ssim`` and
        ``ms_ssim_db`` as ``want_msssim`` gives them. ``refine`` / ``refine_lambda`` /
        ``refine_lr`` as in ``compress_images``: the rows then also carry ``refine_kept``,
        ``objective``, ``objective_plain`` and ``refine_iters``. ``recon`` /
        ``recon_strength`` as ``decompress_images`` takes them (the encode is untouched): the rows
        then also carry ``recon_mode`` and ``recon_strength`` (``recon`` is the decoded image);
        with ``psnr``, ``msssim`` or ``refine`` a codec.RECON_WITH "is not built" error. Precision
        as ``decompress_images``."""
        from . import codec
        return codec.evaluate_images(self, images, want_msssim, max_batch, step=step,
                                     max_bytes=max_bytes, bpp=bpp, step_offsets=step_offsets,
                                     block=block, rdo=rdo, rdo_weights=rdo_weights, tile=tile,
                                     psnr=psnr,
                                     estimate=codec.DEFAULT_ESTIMATE if estimate is None else estimate,
                                     msssim=msssim, refine=refine, refine_lambda=refine_lambda,
                                     refine_lr=refine_lr, recon=recon,
                                     recon_strength=recon_strength)

    @torch.no_grad()
    def evaluate(self, x: torch.Tensor, want_y: bool = False,
                 want_msssim: bool = False, h3_overflow: str = "nan") -> Dict[str, torch.Tensor]:
        """testKodak-style per-image metrics (train.py:157-190): bpp, MSE of the clipped
        reconstruction and PSNR per image, all from deterministic on-device reductions; with
        ``want_msssim`` also MS-SSIM (train.py:178, on the GPU) and MS-SSIM-DB (train.py:179).

        ``h3_overflow`` (the h3 mode: an activation of magnitude ≥ 2^22 does not fit the form):
        "nan" (default, no host synchronisation) — the reconstruction, bpp, MSE and PSNR of the
        batch come back NaN; "raise" — read the range flag (one synchronisation) and raise
        Iclr17Error; "x6" — read it and, when set, evaluate the batch again in the x6 mode (full
        fp32 operands) and return those results."""
        if h3_overflow not in ("nan", "raise", "x6"):
            raise kernels.Iclr17Error(f"iclr17: h3_overflow must be 'nan', 'raise' or 'x6' "
                                      f"(got {h3_overflow!r})")
        mode = kernels.precision()
        res = self._evaluate(x, want_y, want_msssim, mode)
        if h3_overflow != "nan" and mode == "h3" and kernels.h3_range_overflowed(x.device):
            if h3_overflow == "raise":
                raise kernels.Iclr17Error(kernels.H3_RANGE_MESSAGE)
            with kernels.precision_scope("x6"):
                res = self._evaluate(x, want_y, want_msssim, kernels.precision())
        return res

    def _evaluate(self, x, want_y, want_msssim, mode):
        B, _, H, W = x.shape
        out = self.run(x, training=False, x_ref_sse=True, want_y=want_y, mode=mode)
        bits = out.get("bits_per_image")
        if bits is None:
            bits, _ = kernels.reduce_partials(out["bits_partial"])
        sse, _ = kernels.reduce_partials(out["sse_partial"])
        bpp = bits / (H * W)
        mse = sse / (3 * H * W)
        psnr = 10.0 * torch.log10(1.0 / mse)
        res = {"clipped": out["clipped"], "y_hat": out["y_hat"].permute(0, 3, 1, 2).contiguous(),
               "bpp": bpp, "mse": mse, "psnr": psnr}
        if want_y:
            res["y"] = out["y"].permute(0, 3, 1, 2).contiguous()
        if want_msssim:
            ms = kernels.ms_ssim(out["clipped"], x, data_range=1.0)
            res["ms_ssim"] = ms
            res["ms_ssim_db"] = -10 * (torch.log(1 - ms) / math.log(10))
        return res

    def _warm_packs(self, backward: bool = False, mode: Optional[str] = None) -> None:
        """Build (or refresh) every derived parameter layout ``run`` reads in ``mode`` (default:
        kernels.precision(); with ``backward`` also those of the training backward) on the current
        stream, the stale ones as one batched packing launch pair (kernels.batched_packs)."""
        m = chain.MODES[mode or kernels.precision()]
        with kernels.batched_packs():
            m.warm(self, backward)
        # the h3 layouts (the codec's, and the training forward's in this mode) split the packs
        # above, which the batch writes only at its exit; they form a batch of their own
        with kernels.batched_h3_packs():
            m.warm_h3(self)
        if not backward:   # eval: the rate table of the round quantiser (+ the bf16 layouts)
            m.warm_eval(self)

    def evaluate_many(self, batches, want_y: bool = False,
                      want_msssim: bool = False):
        """``evaluate`` of several batches (e.g. Kodak's landscape and portrait images, which
        cannot share one batch) on concurrent HIP streams: the first on the current stream, each
        other on a side stream, so one batch's partly filled last round of workgroups in every
        layer overlaps the other's work. Same kernels and inputs per batch, so the results are
        bitwise those of sequential ``evaluate`` calls."""
        batches = list(batches)
        if len(batches) <= 1 or not batches[0].is_cuda:
            return [self.evaluate(b, want_y=want_y, want_msssim=want_msssim) for b in batches]
        cur = torch.cuda.current_stream(batches[0].device)
        streams = getattr(self, "_side_streams", [])
        while len(streams) < len(batches) - 1:
            streams.append(torch.cuda.Stream(device=batches[0].device))
        self._side_streams = streams
        self._warm_packs()   # packs are written on cur before any side stream reads them
        outs = [None] * len(batches)
        for i, b in enumerate(batches):
            if i == 0:
                continue
            s = streams[i - 1]
            s.wait_stream(cur)
            b.record_stream(s)
            with torch.cuda.stream(s):
                outs[i] = self.evaluate(b, want_y=want_y, want_msssim=want_msssim)
        outs[0] = self.evaluate(batches[0], want_y=want_y, want_msssim=want_msssim)
        for i in range(1, len(batches)):
            cur.wait_stream(streams[i - 1])
            for t in outs[i].values():
                if isinstance(t, torch.Tensor):
                    t.record_stream(cur)
        return outs
