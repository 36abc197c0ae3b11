"""Image-file codec: 8-bit RGB images of any size in, self-describing byte strings out, 8-bit
images back (``ImageCompressor.compress_images`` / ``decompress_images`` / ``evaluate_images`` and
the command line below). The reference has neither padding nor a bitstream, so the contract is
this module's own.

Padding. The transforms take multiples of 16, so an H×W image travels on the smallest *canvas*
``canvas(H, W)`` that holds it, top left, with its bottom and right edges replicated
(kernels.image_ingest); decoding crops the canvas back to H×W (kernels.image_egress). Images are
batched by canvas, so none is padded by more than 15 rows or columns.

Container. One blob per image: a 28-byte little-endian header, then the image's string exactly as
``ImageCompressor.compress`` emits it (P uint32 stream word counts, then the rANS words).

    struct "<4sBBHHxxIIQ":  magic b"I17C" | version u8 = 1 | P u8 (streams per image) |
                            N u16 (channels) | K u16 (entropy alphabet half-width) | 2 pad bytes |
                            H u32 | W u32 (the true size) | fingerprint u64

The fingerprint is the first 8 bytes (little-endian) of the SHA-256 over the model's state_dict
tensors, in sorted key order, as fp32 little-endian bytes: a stream decoded with other weights
fails loudly instead of returning noise.

Precision. The stream does not record the precision mode (kernels.precision()). The latents decode
bit-exactly in every mode; the synthesis transform then runs in the decoder's mode, so decoded
pixels may differ by one 8-bit step between modes. Within one mode the decoded bytes are
reproducible and do not depend on the batch an image travelled in.

Quantiser steps. One checkpoint gives many rates by scaling the quantiser: with a step Δ the
coder codes ŷ = rint(y/Δ) under the rate model evaluated on Δ-wide bins, and the synthesis runs on
Δ·ŷ. Δ comes from a ladder of 32 quarter-octave values (``step_size``; index 8 is Δ = 1).
``compress_images(..., step=s)`` codes at one index; ``max_bytes=`` / ``bpp=`` give a budget on the
whole blob, and each image gets the finest index that fits:

  1. one analysis pass and one ``rate_sweep`` (the estimated bits of every image at all 32 indices)
     per canvas batch;
  2. per image the finest index, scanning 0 → 31, whose ⌈bits/8⌉ + header + 4P + 256P fits
     (``choose_step``); the coarsest when no estimate fits;
  3. the images are coded grouped by index;
  4. an image whose actual blob exceeds its budget moves one index coarser and is coded again;
  5. at index 31 that raises Iclr17Error.

Stepped blobs have their own magic and carry the index in the first pad byte; everything else is
the plain header, and the payload starts at the same byte:

    struct "<4sBBHHBxIIQ":  magic b"I17Q" | version u8 = 1 | P | N | K | step u8 | pad | H | W |
                            fingerprint

Blobs coded with ``step=8`` are I17Q too, with the plain blob's payload; only the call without a
rate option writes I17C. ``decompress_images`` takes both kinds in one call. The weights were
trained at Δ = 1: away from the unit step the quality is whatever the model gives.

Step maps (regions of interest). ``compress_images(..., step_offsets=maps, block=g)`` gives every
block of g×g latent positions (g in 1, 2, 4, 8, 16; 16·g pixels square on the canvas) a step of its
own. The latent of a canvas is h×w, the map mh×mw = ⌈h/g⌉×⌈w/g⌉ (``map_shape``), row-major, ragged at
the bottom and right; position (i, j) reads block (i // g, j // g). ``maps`` holds per image None
(all zero) or signed integer offsets [mh, mw] (``roi_offsets`` makes one from pixel boxes). With a
base index — ``step``, what a budget picks, or 8 — block e is coded at the effective index
clamp(base + offset, 0, 31): ŷ = rint(y/Δ_e), the synthesis runs on Δ_e·ŷ, and each channel's
symbol is coded with that channel's table of step e. A budget works as above with one
``rate_sweep_offsets`` per batch (the estimate of every image at all 32 *bases*), the map's bytes
counted in the overhead, and a blob over budget moving the base one index coarser. The blob:

    struct "<4sBBHHBBIIQ":  magic b"I17M" | version u8 = 1 | P | N | K | base u8 | log2 g u8 |
                            H | W | fingerprint
    then mh·mw bytes of effective indices (each < 32: the decoder needs no clamp rule), then the
    payload as in the other kinds.

Every call with ``step_offsets`` writes I17M, zero offsets included; without it the other two
kinds are written byte for byte as before. ``decompress_images`` takes the three kinds mixed. No
quality claim is made: the weights were trained at Δ = 1, and PSNR inside or outside a region is
whatever the model gives.

RDO. ``compress_images(..., rdo=λ)`` quantises rate–distortion optimised: at the
step Δ each element of channel c sends, instead of r = rint(y/Δ) whatever it costs, the level among
r, its neighbour toward zero and zero of least  bits + λ·g_c·Δ²·(level − y/Δ)²,  the bits being
the rate model's own and g the ``rdo_weights`` (default ``ImageCompressor.synthesis_gains()``: the
squared pixel response of the synthesis to a unit impulse in the channel, mean 1). It is an
encoder-side choice: the blobs are ordinary I17Q ones, nothing of ``rdo`` is recorded and the
decoder is unchanged. ``rdo`` goes with ``step``, ``max_bytes`` or ``bpp`` and alone means the unit
step; a budget then estimates with the optimised levels' bits (``rate_sweep(..., rdo=)``). With
``step_offsets`` it raises: per-block RDO is not built. The estimate is the rate model's; the
coder's escape cost beyond ±K is not modelled. No quality claim is made.

Tiled streams. ``compress_images(..., tile=t)`` (t in 8, 16, 32, 64 latent positions: 128 to 1024
pixels square) codes the same latents with independent streams per spatial tile.
The h×w latent of the canvas is cut into th×tw = ⌈h/t⌉×⌈w/t⌉ tiles (``tile_shape``), ragged at the
bottom and right; there is one stream per (tile row, tile column, channel group), in that order,
with the tile's symbols in (channel, row, column) order: the words of a tile are the words the
plain coder gives that tile as a latent of its own. Only the layout changes: the quantiser, the
tables and the levels are those of the untiled call with the same ``step``, budget or ``rdo``, and
the decoded latents and pixels are the same. A budget counts the real overhead, 28 + th·tw·P·260
bytes (``tiled_blob_overhead``). ``tile`` with ``step_offsets`` raises: tiled step maps are not
built. The blob:

    struct "<4sBBHHBBIIQ":  magic b"I17T" | version u8 = 1 | P | N | K | step u8 | log2 t u8 |
                            H | W | fingerprint
    then th·tw·P little-endian uint32 word counts (tile row, tile column, group), then the words.

It always carries a ladder index: a call with ``tile`` and no rate option writes index 8 and codes
``compress``'s own ŷ. ``decompress_images`` takes the four kinds mixed.

Quality targets. ``compress_images(..., psnr=T)`` is the opposite request: at
least T dB, as small as the ladder allows. An index *passes* for an image when the integer SSE of
its 8-bit decode is ≤ ``sse_limit(H, W, T)`` = ⌊255²·3·H·W·10^(−T/10)⌋; ``search_quality`` brackets the
boundary with at most 8 probes per image, and the image is coded at the index L it ends on: L
passed, and it is 31 or index L + 1 was measured and failed. The SSE is not assumed monotone along
the ladder. A probe (``quality_probe``) quantises every unfinished image of a canvas batch at its
own index, runs the synthesis and sums the squared 8-bit error on the device: no entropy coding,
no pixel transfer. ``estimate=True`` orders the probes by ``distortion_sweep``'s prediction and never
decides; the default bisects (measured: guiding saves no probes). The blobs are those of ``step=`` at the index found, byte for byte (I17Q, with ``tile``
I17T): encoder-side only. A target index 0 misses raises; ``psnr`` with another rate option, ``rdo``
or ``step_offsets`` raises (the last two: not built). No claim is made about the rate–distortion
trade away from Δ = 1.

MS-SSIM targets. ``compress_images(..., msssim=T)`` (0 < T < 1) is the same request
in the measure the model is trained and compared in: an index passes when the fp32 MS-SSIM of its
8-bit decode against the original, over the image's own H×W and read as a float64, is ≥ T (NaN does
not pass). The search is ``search_quality``'s plain bisection (at most 6 probes); the probe
(``msssim_probe``) is ``quality_probe`` with ``kernels.image_msssim`` as its last step, whose value
is bit for bit what ``evaluate_images(want_msssim=True)`` reports for the decode at that index.
Both sides of an image must be at least 161 (five levels of an 11-tap window): a smaller image
raises on the host, before the ingest. Blobs, ``tile`` and the combinations that raise are as for
``psnr``; ``estimate=True`` raises too (``distortion_sweep`` predicts squared error).

Latent refinement. ``compress_images(..., step=s, refine=K, refine_lambda=λ)``
improves the latent of each image before it is coded: K Adam steps on y lower
J = bits + (λ/3)·SSE8/255² — the rate model's bits of ŷ = rint(y/Δ) and the squared 8-bit error of its
decode over the image's own pixels, H·W times train.py's λ·mse + bpp — with the gradient taken
through the synthesis and the rate model and straight through the rounding (``refine_loop``: no
host synchronisation). The best ŷ seen is then judged against the plain one through the eval
chain, as ``evaluate_images`` measures, and coded only where its J is strictly lower
(``refine_latents``), so ``stats["objective"]`` ≤ ``stats["objective_plain"]`` and a diverged run
gives the plain blob. It is an encoder-side choice: ordinary I17Q blobs (with ``tile`` I17T), any
decoder reads them. ``refine`` goes with ``step`` (none: index 8) and ``tile``; with a budget, a
quality target, ``rdo`` or ``step_offsets`` and in the bf16 mode it raises; 0 and None are the call
without it. ``refine_lr`` (in units of Δ) defaults to ``DEFAULT_REFINE_LR``.

The objective rides on λ: ``refine_lambda=msssim_lambda(λ)`` (a scalar, or one per
image; mixing the two kinds raises) refines for J = bits + λ·H·W·(1 − MS-SSIM8), H·W times train.py's
λ·(1 − MS-SSIM) + bpp on the 8-bit decode. The loop then measures with
``kernels.image_msssim_fwd_saved``, decides with ``kernels.refine_keep_msssim`` and takes the
distortion gradient from ``kernels.image_msssim_bwd``; the judge measures ``image_msssim`` on both
decodes. Both sides of every image must be at least 161. ``stats`` and ``evaluate_images`` rows
also carry ``refine_distortion`` ("ms-ssim"), ``ms_ssim`` and ``ms_ssim_plain``.

Region decode. ``decompress_region(blob, box)`` returns the pixels of ``box`` = (x0, y0, x1, y1)
(half-open, inside the image), byte for byte the crop of the full decode, from the tiles it needs
alone. The synthesis is deconv 5×5/s2/p2, IGDN, deconv 5×5/s2/p2, IGDN, deconv 9×9/s4/p4; IGDN is
pointwise in space, output o of a 5×5/s2/p2 deconv reads inputs ⌈(o − 2)/2⌉ … ⌊(o + 2)/2⌋ and output
o of the 9×9/s4/p4 one ⌈(o − 4)/4⌉ … ⌊(o + 4)/4⌋. ``region_window`` maps the box's first and last
pixel through the three layers (at most one latent position up and left of the box's own and two
down and right), clamps to the latent, and takes the tiles that cover that rectangle; those
streams are decoded into a compact latent, which is dequantised and synthesised as an image of
its own, and ``image_egress`` runs on the crop.

    python -m iclr_17_compression_amd.codec encode IN.png OUT.i17c --weights CKPT [--N 192]
                                            [--step S | --max-bytes B | --bpp R | --psnr T |
                                             --msssim T]
                                            [--roi X0,Y0,X1,Y1,OFF ...] [--block G] [--rdo L]
                                            [--tile T] [--refine K --refine-lambda L [--refine-lr R]
                                             [--refine-distortion mse|ms-ssim]]
    python -m iclr_17_compression_amd.codec decode IN.i17c OUT.png --weights CKPT
                                            [--region X0,Y0,X1,Y1]
    python -m iclr_17_compression_amd.codec eval IMG... --weights CKPT [--ms-ssim] [--steps 4,8,12]
                                            [--rdo L] [--psnr T | --msssim T]
                                            [--refine K --refine-lambda L [--refine-lr R]
                                             [--refine-distortion mse|ms-ssim]]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import struct
import sys
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kernels
from ._lib import Iclr17Error
from .packcache import PackCache

MAGIC = b"I17C"
VERSION = 1
HEADER = struct.Struct("<4sBBHHxxIIQ")
assert HEADER.size == 28

Header = namedtuple("Header", "P N K H W fingerprint")

STEP_MAGIC = b"I17Q"
STEP_HEADER = struct.Struct("<4sBBHHBxIIQ")
assert STEP_HEADER.size == HEADER.size   # the payload starts at the same byte in both kinds

MAP_MAGIC = b"I17M"
MAP_HEADER = struct.Struct("<4sBBHHBBIIQ")
assert MAP_HEADER.size == HEADER.size    # the map starts where the other kinds' payload does
DEFAULT_BLOCK = 4                        # block edge in latent positions: 64×64 pixels

# what parse_blob gives for a mapped blob in place of a ladder index: the base index, the block
# edge g, the effective indices (uint8 [mh, mw]) and the byte at which the payload starts
StepMap = namedtuple("StepMap", "base block indices payload")

TILE_MAGIC = b"I17T"
TILE_HEADER = struct.Struct("<4sBBHHBBIIQ")
assert TILE_HEADER.size == HEADER.size   # the count table starts where the other kinds' payload does

# what parse_blob gives for a tiled blob in place of a ladder index: the ladder index, the tile
# edge t, the streams' word counts (int64 [th, tw, P]) and the byte at which the words start
TileInfo = namedtuple("TileInfo", "step tile counts words")

# region_window's answer: the latent rectangle (i0, j0, i1, j1) and the tile rectangle (r0, c0, r1,
# c1), both half-open, and the box's (x, y) inside the reconstruction of the tile rectangle
RegionWindow = namedtuple("RegionWindow", "latent tiles offset")

# ------------------------------------------------------------------------------ ladder
STEPS = 32
UNIT_STEP = 8
# the fp32 values nearest to 2^0, 2^¼, 2^½, 2^¾, as literals: the same bits on every host
_STEP_MANTISSAS = (1.0, 1.1892070770263672, 1.4142135381698608, 1.6817928552627563)


def step_size(s: int) -> float:
    """Δ_s = M[s % 4] · 2^(s // 4 − 2) for the ladder index 0 ≤ s < 32: a quarter octave per
    index from 0.25 to about 53.8, each exactly an fp32 value, Δ_8 = 1."""
    if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= s < STEPS:
        raise Iclr17Error(f"iclr17: codec: quantiser step index {s!r} is not an integer in 0..{STEPS - 1}")
    return _STEP_MANTISSAS[int(s) % 4] * 2.0 ** (int(s) // 4 - 2)


def choose_step(est_bits_row, budget: int, overhead: int) -> int:
    """The budget rule's first pick for one image: the finest ladder index, scanning 0 → 31,
    whose estimated size ⌈bits/8⌉ + overhead fits ``budget`` bytes. ``est_bits_row``: the image's
    row of ``rate_sweep`` (one estimate per index). The row is not assumed monotone: the first
    index that fits wins. Raises Iclr17Error when none fits."""
    sizes = [math.ceil(float(b) / 8.0) + overhead for b in est_bits_row]
    for s, size in enumerate(sizes):
        if size <= budget:
            return s
    raise Iclr17Error(f"iclr17: codec: no quantiser step fits {budget} bytes (the smallest estimate "
                      f"is {min(sizes)} bytes)" if sizes else "iclr17: codec: empty estimate row")


def encode_to_budget(chosen: Sequence[int], budgets: Sequence[Optional[int]], encode,
                     labels: Sequence[str]) -> Tuple[List[bytes], List[int]]:
    """Steps 3–5 of the budget rule for one batch (a pure host function: the coding is
    ``encode``). ``chosen``: each image's first ladder index; ``budgets``: its byte budget (None:
    none); ``encode(members, s)`` codes the images ``members`` (ascending positions) at index s
    and returns their blobs. Images are coded grouped by index; one whose blob exceeds its budget
    moves one index coarser and is coded again, and at index 31 that raises, naming
    ``labels[k]``, the budget and the size reached → (blobs, re-encodes per image)."""
    chosen = list(chosen)
    blobs: List[Optional[bytes]] = [None] * len(chosen)
    reencodes = [0] * len(chosen)
    todo = list(range(len(chosen)))
    while todo:
        again = []
        for members in _group([chosen[k] for k in todo], len(todo)):
            ks = [todo[m] for m in members]
            s = chosen[ks[0]]
            for k, blob in zip(ks, encode(ks, s)):
                if budgets[k] is None or len(blob) <= budgets[k]:
                    blobs[k] = blob
                elif s == STEPS - 1:
                    raise Iclr17Error(f"iclr17: codec: {labels[k]} does not fit its budget of "
                                      f"{budgets[k]} bytes: the coarsest step gives {len(blob)}")
                else:
                    chosen[k] = s + 1
                    reencodes[k] += 1
                    again.append(k)
        todo = sorted(again)
    return blobs, reencodes


# ------------------------------------------------------------------------------ quality targets
MAX_PROBES = 8    # per image: 6 bisect the 33 outcomes, 2 more are the guided probes'

# one image of a quality search: its name in messages, the target in dB, its size and sse_limit
QualityTarget = namedtuple("QualityTarget", "label psnr H W limit")
# search_quality's answer, one entry per image: the ladder index, the probes spent, the SSE
# measured at the index, and the guided search's first guess (None: none was made)
QualityResult = namedtuple("QualityResult", "indices probes sse guesses")


def psnr_value(psnr) -> float:
    """A PSNR target in dB checked on the host: a real number, not a bool, finite and > 0."""
    if isinstance(psnr, bool) or not isinstance(psnr, (int, float, np.integer, np.floating)):
        raise Iclr17Error(f"iclr17: codec: psnr must be a real number (got {psnr!r})")
    t = float(psnr)
    if not (math.isfinite(t) and t > 0.0):
        raise Iclr17Error(f"iclr17: codec: psnr must be finite and > 0 (got {psnr!r})")
    return t


def msssim_value(msssim) -> float:
    """An MS-SSIM target checked on the host: a real number, not a bool, finite, 0 < T < 1."""
    if isinstance(msssim, bool) or not isinstance(msssim, (int, float, np.integer, np.floating)):
        raise Iclr17Error(f"iclr17: codec: msssim must be a real number (got {msssim!r})")
    t = float(msssim)
    if not (math.isfinite(t) and 0.0 < t < 1.0):
        raise Iclr17Error(f"iclr17: codec: msssim must be finite, > 0 and < 1 (got {msssim!r})")
    return t


# one image of an MS-SSIM search: its name in messages, the target and its size
MsssimTarget = namedtuple("MsssimTarget", "label msssim H W")


def msssim_passes(target, value) -> bool:
    """``search_quality``'s pass rule of an MS-SSIM target: the measured fp32 MS-SSIM, read as a
    float64, is ≥ the target. Nothing is rounded to dB; NaN does not pass."""
    return float(value) >= target.msssim


def msssim_failure(target, value) -> str:
    return (f"iclr17: codec: {target.label} cannot reach MS-SSIM {target.msssim!r}: the finest step "
            f"(index 0) gives {float(value)!r}")


def sse_limit(H: int, W: int, psnr) -> int:
    """The largest integer SSE of an 8-bit H×W RGB image that still reaches ``psnr`` dB:
    ⌊255²·3·H·W·10^(−psnr/10)⌋, evaluated in float64. A ladder index *passes* when the integer SSE
    of its 8-bit decode is ≤ this; nothing is decided on a rounded dB value."""
    t = psnr_value(psnr)
    if H < 1 or W < 1:
        raise Iclr17Error(f"iclr17: codec: image size {H}x{W} must be at least 1x1")
    return int(math.floor(255.0 ** 2 * 3.0 * float(H) * float(W) * 10.0 ** (-t / 10.0)))


def _psnr_of(sse: int, H: int, W: int) -> float:
    return 10.0 * math.log10(255.0 ** 2 * 3 * H * W / sse) if sse else math.inf


def _guided_guess(seed, limit: int, sse0: int) -> int:
    """The coarsest index the calibrated prediction passes, −1 when none: the prediction is
    base + seed[s] with base = max(0, SSE(UNIT_STEP) − seed[UNIT_STEP])."""
    base = max(0.0, float(sse0) - float(seed[UNIT_STEP]))
    ok = [s for s in range(STEPS) if base + float(seed[s]) <= limit]
    return max(ok) if ok else -1


def sse_passes(target, sse) -> bool:
    return sse <= target.limit


def psnr_failure(target, sse) -> str:
    return (f"iclr17: codec: {target.label} cannot reach {target.psnr:g} dB: the finest step "
            f"(index 0) gives {_psnr_of(sse, target.H, target.W):.4f} dB")


def search_quality(probe, n: int, seeds=None, targets=None, passes=None,
                   failure=None) -> QualityResult:
    """The search of a quality target for ``n`` images (a pure host function: the measuring is
    ``probe``). ``targets``: one ``QualityTarget`` per image. Per image the bracket L < F holds an
    index that passed (L, −1 at first: virtual) and one that failed (F, 32 at first: virtual).
    Every round calls ``probe(members, indices)`` once for all unfinished images (ascending
    positions), one index per image strictly inside its bracket, gets their integer SSEs back and
    moves L (SSE ≤ limit) or F. An image is done at F == L + 1: L is its answer, and L == −1
    raises Iclr17Error with the PSNR reached at index 0. Nothing assumes the SSE monotone along the
    ladder: the answer passed, and it is index 31 or its coarser neighbour was measured failing.

    The probe index is the bracket's midpoint ⌊(L + F)/2⌋: 6 probes at most. With ``seeds[k]`` (32
    predicted SSE contributions of the quantiser, 255²·``distortion_sweep``'s row; None: plain
    bisection) image k first probes UNIT_STEP, then the coarsest index that the prediction
    calibrated on that probe passes (``_guided_guess``, moved inside the bracket), then that
    index's neighbour on the side of the boundary, then bisects: ``MAX_PROBES`` = 8 at most. An
    image's sequence depends on its own seed, limit and measurements alone.

    ``passes(target, value)`` and ``failure(target, value at index 0)`` (the message of a target
    that index 0 misses) make the same search serve another measure: by default the probe's values
    are integer SSEs against ``target.limit``; with ``passes`` they are kept as the probe returns
    them (``msssim_passes`` / ``msssim_failure``: fp32 MS-SSIM values, seeds unused)."""
    convert = int if passes is None else (lambda e: e)
    passes = sse_passes if passes is None else passes
    failure = psnr_failure if failure is None else failure
    if targets is None or len(targets) != n or (seeds is not None and len(seeds) != n):
        raise Iclr17Error(f"iclr17: codec: search_quality takes one target (and seed) per image "
                          f"for {n} images")
    lo, hi = [-1] * n, [STEPS] * n
    seen: List[Dict[int, int]] = [{} for _ in range(n)]
    guesses: List[Optional[int]] = [None] * n
    last: List[Optional[int]] = [None] * n      # the guided probes' previous index

    def next_index(k: int) -> int:
        L, F = lo[k], hi[k]
        seed = None if seeds is None else seeds[k]
        if seed is not None:
            if not seen[k]:
                return UNIT_STEP
            if len(seen[k]) == 1:
                g = guesses[k] = _guided_guess(seed, targets[k].limit, seen[k][UNIT_STEP])
                return min(max(g, L + 1), F - 1)
            if len(seen[k]) == 2 and last[k] is not None:
                c = last[k] + 1 if lo[k] == last[k] else last[k] - 1
                if L < c < F:
                    return c
        return (L + F) // 2

    todo = list(range(n))
    while todo:
        indices = [next_index(k) for k in todo]
        sses = probe(list(todo), list(indices))
        if len(sses) != len(todo):
            raise Iclr17Error("iclr17: codec: search_quality: the probe returned "
                              f"{len(sses)} sums for {len(todo)} images")
        for k, s, e in zip(todo, indices, sses):
            if not lo[k] < s < hi[k] or len(seen[k]) >= MAX_PROBES:
                raise Iclr17Error("iclr17: codec: search_quality: probe outside its bracket or cap")
            seen[k][s] = convert(e)
            last[k] = s
            if passes(targets[k], seen[k][s]):
                lo[k] = s
            else:
                hi[k] = s
        todo = [k for k in todo if hi[k] > lo[k] + 1]
    for k, t in enumerate(targets):
        if lo[k] < 0:
            raise Iclr17Error(failure(t, seen[k][0]))
    return QualityResult(list(lo), [len(v) for v in seen], [seen[k][lo[k]] for k in range(n)],
                         guesses)


def blob_overhead(P: int) -> int:
    """Bytes of a blob that are not renormalisation words: the header, the P stream word counts
    and each stream's 64 final rANS states."""
    return HEADER.size + 4 * P + 256 * P


def tile_shape(H: int, W: int, tile: int) -> Tuple[int, int]:
    """(th, tw) of an H×W image coded with tiles of ``tile``×``tile`` latent positions (8, 16, 32 or
    64): its canvas's latent is h×w = canvas/16, and th×tw = ⌈h/tile⌉×⌈w/tile⌉."""
    Hc, Wc = canvas(H, W)
    return kernels.tile_grid(Hc // 16, Wc // 16, tile)


def tiled_blob_overhead(P: int, H: int, W: int, tile: int) -> int:
    """``blob_overhead`` of a tiled blob of an H×W image: the header, and per stream — th·tw·P of
    them — its word count and its 64 final rANS states."""
    th, tw = tile_shape(H, W, tile)
    return TILE_HEADER.size + th * tw * P * (4 + 256)


# ------------------------------------------------------------------------------ canvas
def canvas(H: int, W: int) -> Tuple[int, int]:
    """The smallest multiples of 16 ≥ H and W."""
    if H < 1 or W < 1:
        raise Iclr17Error(f"iclr17: codec: image size {H}x{W} must be at least 1x1")
    return -(-H // 16) * 16, -(-W // 16) * 16


def _group(keys: Sequence, max_batch: int) -> List[List[int]]:
    """Indices grouped by equal key, at most ``max_batch`` per group; groups in the order their
    first member appears, indices ascending inside a group."""
    if max_batch < 1:
        raise Iclr17Error(f"iclr17: codec: max_batch must be at least 1 (got {max_batch})")
    by_key: Dict[object, List[int]] = {}
    for i, k in enumerate(keys):
        by_key.setdefault(k, []).append(i)
    return [idx[s:s + max_batch] for idx in by_key.values() for s in range(0, len(idx), max_batch)]


def group_by_canvas(shapes: Sequence[Tuple[int, int]], max_batch: int = 64) -> List[List[int]]:
    """Index groups of ``shapes`` [(H, W)]: every group holds images of one canvas, at most
    ``max_batch`` of them (Kodak's landscape and portrait images: two groups)."""
    return _group([canvas(H, W) for H, W in shapes], max_batch)


# ------------------------------------------------------------------------------ container
def fingerprint(model) -> int:
    """u64 of the model's weights (module docstring); cached on the model until a parameter
    changes (the parameters' version counters, as packcache does for the packed layouts)."""
    sd = model.state_dict()
    keys = sorted(sd)
    cache = model.__dict__.setdefault("_codec_cache", PackCache())

    def build() -> int:
        h = hashlib.sha256()
        for k in keys:
            h.update(sd[k].detach().to(torch.float32).cpu().contiguous().numpy().astype("<f4").tobytes())
        return int.from_bytes(h.digest()[:8], "little")

    return cache.get("fingerprint", [sd[k] for k in keys], build)


def pack_header(P: int, N: int, K: int, H: int, W: int, fingerprint: int) -> bytes:
    if H < 1 or W < 1:
        raise Iclr17Error(f"iclr17: codec: image size {H}x{W} must be at least 1x1")
    if not (1 <= P <= 255 and 1 <= N <= 65535 and 1 <= K <= 65535 and H < 2 ** 32 and W < 2 ** 32):
        raise Iclr17Error(f"iclr17: codec: header field out of range (P={P} N={N} K={K} {H}x{W})")
    return HEADER.pack(MAGIC, VERSION, P, N, K, H, W, fingerprint & (2 ** 64 - 1))


def _checked_header(kind, magic, version, P, n, K, H, W, fp, N, fingerprint) -> Header:
    if magic != kind:
        raise Iclr17Error(f"iclr17: codec: bad magic {magic!r} (not an {kind.decode()} stream)")
    if version != VERSION:
        raise Iclr17Error(f"iclr17: codec: unknown version {version} (this build reads {VERSION})")
    if H == 0 or W == 0:
        raise Iclr17Error(f"iclr17: codec: image size {H}x{W} must be at least 1x1")
    if N is not None and n != N:
        raise Iclr17Error(f"iclr17: codec: the stream is for N={n}, the model has N={N}")
    if fingerprint is not None and fp != fingerprint:
        raise Iclr17Error(f"iclr17: codec: weights fingerprint mismatch (stream {fp:016x}, model "
                          f"{fingerprint:016x}): the stream was coded with other weights")
    return Header(P, n, K, H, W, fp)


def parse_header(blob: bytes, N: Optional[int] = None, fingerprint: Optional[int] = None) -> Header:
    """The header of a plain (I17C) blob; with ``N`` / ``fingerprint`` (the decoding model's) also
    checked against them. The payload (blob[HEADER.size:]) is checked by ``decompress``."""
    if len(blob) < HEADER.size:
        raise Iclr17Error(f"iclr17: codec: truncated header ({len(blob)} of {HEADER.size} bytes)")
    magic, version, P, n, K, H, W, fp = HEADER.unpack_from(blob)
    return _checked_header(MAGIC, magic, version, P, n, K, H, W, fp, N, fingerprint)


def pack_step_header(P: int, N: int, K: int, step: int, H: int, W: int, fingerprint: int) -> bytes:
    """The header of a stepped blob: ``pack_header``'s fields under the magic I17Q, with the
    ladder index in the first of the two pad bytes."""
    step_size(step)
    pack_header(P, N, K, H, W, fingerprint)   # the shared fields' range checks
    return STEP_HEADER.pack(STEP_MAGIC, VERSION, P, N, K, int(step), H, W, fingerprint & (2 ** 64 - 1))


def parse_step_header(blob: bytes, N: Optional[int] = None,
                      fingerprint: Optional[int] = None) -> Tuple[Header, int]:
    """The header of a stepped (I17Q) blob → (Header, ladder index), checked as ``parse_header``
    checks a plain one; an index outside the ladder raises."""
    if len(blob) < STEP_HEADER.size:
        raise Iclr17Error(f"iclr17: codec: truncated header ({len(blob)} of {STEP_HEADER.size} bytes)")
    magic, version, P, n, K, step, H, W, fp = STEP_HEADER.unpack_from(blob)
    head = _checked_header(STEP_MAGIC, magic, version, P, n, K, H, W, fp, N, fingerprint)
    if step >= STEPS:
        raise Iclr17Error(f"iclr17: codec: quantiser step {step} in the stream (this build reads "
                          f"0..{STEPS - 1})")
    return head, step


def pack_map_header(P: int, N: int, K: int, base: int, block: int, H: int, W: int,
                    fingerprint: int, indices) -> bytes:
    """The header of a mapped blob and its map: ``pack_header``'s fields under the magic I17M with
    the base index and log2 of the block edge in the two pad bytes, then the mh·mw effective
    ladder indices (``map_shape``), one byte each, row-major."""
    step_size(base)
    pack_header(P, N, K, H, W, fingerprint)   # the shared fields' range checks
    mh, mw = map_shape(H, W, block)
    a = np.asarray(indices)
    if a.dtype.kind not in "iu" or a.shape != (mh, mw) or a.min() < 0 or a.max() >= STEPS:
        raise Iclr17Error(f"iclr17: codec: the step map of a {H}x{W} image with block {block} is "
                          f"[{mh}, {mw}] ladder indices 0..{STEPS - 1} (got {a.dtype} {a.shape})")
    return MAP_HEADER.pack(MAP_MAGIC, VERSION, P, N, K, int(base), kernels.MAP_BLOCKS.index(block), H, W,
                           fingerprint & (2 ** 64 - 1)) + a.astype(np.uint8).tobytes()


def parse_map_header(blob: bytes, N: Optional[int] = None,
                     fingerprint: Optional[int] = None) -> Tuple[Header, StepMap]:
    """The header and map of a mapped (I17M) blob → (Header, StepMap), checked as ``parse_header``
    checks a plain one; a base or map byte outside the ladder, a block edge above 16 and a
    truncated map raise."""
    if len(blob) < MAP_HEADER.size:
        raise Iclr17Error(f"iclr17: codec: truncated header ({len(blob)} of {MAP_HEADER.size} bytes)")
    magic, version, P, n, K, base, lg, H, W, fp = MAP_HEADER.unpack_from(blob)
    head = _checked_header(MAP_MAGIC, magic, version, P, n, K, H, W, fp, N, fingerprint)
    if base >= STEPS:
        raise Iclr17Error(f"iclr17: codec: quantiser step {base} in the stream (this build reads "
                          f"0..{STEPS - 1})")
    if lg > 4:
        raise Iclr17Error(f"iclr17: codec: step-map block of 2^{lg} latent positions in the stream "
                          "(this build reads 2^0..2^4)")
    mh, mw = map_shape(H, W, 1 << lg)
    end = MAP_HEADER.size + mh * mw
    if len(blob) < end:
        raise Iclr17Error(f"iclr17: codec: truncated step map ({len(blob) - MAP_HEADER.size} of "
                          f"{mh * mw} bytes)")
    indices = np.frombuffer(bytes(blob[MAP_HEADER.size:end]), dtype=np.uint8).reshape(mh, mw)
    if indices.size and int(indices.max()) >= STEPS:
        raise Iclr17Error(f"iclr17: codec: quantiser step {int(indices.max())} in the stream's step "
                          f"map (this build reads 0..{STEPS - 1})")
    return head, StepMap(base, 1 << lg, indices, end)


def pack_tile_header(P: int, N: int, K: int, step: int, tile: int, H: int, W: int,
                     fingerprint: int) -> bytes:
    """The header of a tiled blob: ``pack_header``'s fields under the magic I17T with the ladder
    index and log2 of the tile edge in the two pad bytes."""
    step_size(step)
    pack_header(P, N, K, H, W, fingerprint)   # the shared fields' range checks
    tile_shape(H, W, tile)                    # the tile edge's
    return TILE_HEADER.pack(TILE_MAGIC, VERSION, P, N, K, int(step), kernels.TILES.index(tile) + 3,
                            H, W, fingerprint & (2 ** 64 - 1))


def parse_tile_header(blob: bytes, N: Optional[int] = None,
                      fingerprint: Optional[int] = None) -> Tuple[Header, TileInfo]:
    """The header and count table of a tiled (I17T) blob → (Header, TileInfo), checked as
    ``parse_header`` checks a plain one; a step outside the ladder, a tile edge this build does
    not read, a truncated count table, counts that do not sum to the words that follow and an odd
    rest raise. All of it on the host: nothing of a bad blob reaches the device."""
    if len(blob) < TILE_HEADER.size:
        raise Iclr17Error(f"iclr17: codec: truncated header ({len(blob)} of {TILE_HEADER.size} bytes)")
    magic, version, P, n, K, step, lg, H, W, fp = TILE_HEADER.unpack_from(blob)
    head = _checked_header(TILE_MAGIC, magic, version, P, n, K, H, W, fp, N, fingerprint)
    if step >= STEPS:
        raise Iclr17Error(f"iclr17: codec: quantiser step {step} in the stream (this build reads "
                          f"0..{STEPS - 1})")
    if not 3 <= lg <= 6:
        raise Iclr17Error(f"iclr17: codec: tiles of 2^{lg} latent positions in the stream (this "
                          "build reads 2^3..2^6)")
    if P < 1:
        raise Iclr17Error("iclr17: codec: a tiled stream with no channel groups")
    th, tw = tile_shape(H, W, 1 << lg)
    end = TILE_HEADER.size + 4 * th * tw * P
    if len(blob) < end:
        raise Iclr17Error(f"iclr17: codec: truncated tile count table ({len(blob) - TILE_HEADER.size} "
                          f"of {4 * th * tw * P} bytes)")
    if (len(blob) - end) % 2:
        raise Iclr17Error(f"iclr17: codec: truncated stream ({len(blob)} bytes)")
    counts = np.frombuffer(bytes(blob[TILE_HEADER.size:end]), dtype="<u4").astype(np.int64)
    if int(counts.sum()) != (len(blob) - end) // 2:
        raise Iclr17Error(f"iclr17: codec: the tile counts sum to {int(counts.sum())} words, the "
                          f"stream holds {(len(blob) - end) // 2}")
    return head, TileInfo(step, 1 << lg, counts.reshape(th, tw, P), end)


def parse_blob(blob: bytes, N: Optional[int] = None, fingerprint: Optional[int] = None):
    """The header of any kind of blob → (Header, ladder index | None for a plain blob | StepMap
    for a mapped one | TileInfo for a tiled one)."""
    if bytes(blob[:4]) == STEP_MAGIC:
        return parse_step_header(blob, N, fingerprint)
    if bytes(blob[:4]) == MAP_MAGIC:
        return parse_map_header(blob, N, fingerprint)
    if bytes(blob[:4]) == TILE_MAGIC:
        return parse_tile_header(blob, N, fingerprint)
    return parse_header(blob, N, fingerprint), None


# ------------------------------------------------------------------------------ regions
def _checked_box(H: int, W: int, box) -> Tuple[int, int, int, int]:
    try:
        x0, y0, x1, y1 = box
        ok = all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) for v in box)
    except (TypeError, ValueError):
        ok = False
    if not ok or not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
        raise Iclr17Error(f"iclr17: codec: a region is (x0, y0, x1, y1) in pixels, half-open, not "
                          f"empty and inside the {H}x{W} image (got {box!r})")
    return int(x0), int(y0), int(x1), int(y1)


def _latent_span(lo: int, hi: int, n: int) -> Tuple[int, int]:
    """The latent positions, first and last, that the synthesis reads for the output pixels
    lo..hi of one axis with n latent positions: back through deconv 9×9/s4/p4 and two deconvs
    5×5/s2/p2 (the module docstring has the rule), each layer's range clamped to its grid."""
    for k, p, size in ((4, 4, 4 * n), (2, 2, 2 * n), (2, 2, n)):
        lo = max(-((p - lo) // k), 0)          # ⌈(lo − p)/k⌉
        hi = min((hi + p) // k, size - 1)      # ⌊(hi + p)/k⌋
    return lo, hi


def region_window(H: int, W: int, tile: int, box) -> RegionWindow:
    """What a decoder needs for the pixels ``box`` = (x0, y0, x1, y1) (half-open, inside the H×W
    image) of an image coded with tiles of ``tile`` latent positions → RegionWindow: the rectangle
    of the latent those pixels depend on and no more (from the layer geometry, module docstring),
    the rectangle of tiles that covers it, both half-open, and where the box lies in the
    reconstruction of that tile rectangle, in pixels (x, y). A pure host function."""
    x0, y0, x1, y1 = _checked_box(H, W, box)
    Hc, Wc = canvas(H, W)
    kernels.tile_grid(Hc // 16, Wc // 16, tile)
    i0, i1 = _latent_span(y0, y1 - 1, Hc // 16)
    j0, j1 = _latent_span(x0, x1 - 1, Wc // 16)
    r0, c0, r1, c1 = i0 // tile, j0 // tile, i1 // tile + 1, j1 // tile + 1
    return RegionWindow((i0, j0, i1 + 1, j1 + 1), (r0, c0, r1, c1),
                        (x0 - 16 * tile * c0, y0 - 16 * tile * r0))


# ------------------------------------------------------------------------------ step maps
def map_shape(H: int, W: int, block: int = DEFAULT_BLOCK) -> Tuple[int, int]:
    """(mh, mw) of the step map of an H×W image: its canvas's latent is h×w = canvas/16, a block
    is ``block``×``block`` latent positions (1, 2, 4, 8 or 16), and mh×mw = ⌈h/block⌉×⌈w/block⌉."""
    Hc, Wc = canvas(H, W)
    return kernels.map_shape(Hc // 16, Wc // 16, block)


def effective_indices(base: int, offsets) -> np.ndarray:
    """clamp(base + offset, 0, 31) per block as uint8: what the stream's map holds."""
    step_size(base)
    return np.clip(int(base) + np.asarray(offsets, dtype=np.int64), 0, STEPS - 1).astype(np.uint8)


def roi_offsets(H: int, W: int, boxes, block: int = DEFAULT_BLOCK) -> np.ndarray:
    """Step offsets of an H×W image from pixel boxes → int32 [mh, mw] (``map_shape``). ``boxes``:
    (x0, y0, x1, y1, offset) with x0 ≤ x < x1, y0 ≤ y < y1 in pixels; a block (16·block pixels
    square on the canvas) that intersects a box gets its offset, where boxes overlap the most
    negative (finest) offset wins, and every other block gets 0."""
    mh, mw = map_shape(H, W, block)
    side = 16 * block
    out = np.zeros((mh, mw), dtype=np.int32)
    hit = np.zeros((mh, mw), dtype=bool)
    for box in boxes:
        if len(box) != 5:
            raise Iclr17Error(f"iclr17: codec: a box is (x0, y0, x1, y1, offset) (got {box!r})")
        x0, y0, x1, y1, off = box
        if isinstance(off, bool) or not isinstance(off, (int, np.integer)):
            raise Iclr17Error(f"iclr17: codec: a box's offset is an integer (got {off!r})")
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, mw * side), min(y1, mh * side)
        if x0 >= x1 or y0 >= y1:
            continue   # empty, or outside the canvas
        rows = slice(int(y0 // side), int(-(-y1 // side)))
        cols = slice(int(x0 // side), int(-(-x1 // side)))
        out[rows, cols] = np.where(hit[rows, cols], np.minimum(out[rows, cols], off), off)
        hit[rows, cols] = True
    return out


def checked_offsets(shapes: Sequence[Tuple[int, int]], step_offsets, block: int) -> List[np.ndarray]:
    """``compress_images``'s ``step_offsets`` for images of sizes ``shapes``, checked on the host:
    one entry per image, each None (all zero) or an integer array [mh, mw] → int8 arrays, the
    values cut to −31..31 (beyond that the clamp to the ladder gives the same index)."""
    if isinstance(step_offsets, np.ndarray) and step_offsets.ndim == 2:
        step_offsets = [step_offsets]
    if len(step_offsets) != len(shapes):
        raise Iclr17Error(f"iclr17: codec: step_offsets has {len(step_offsets)} entries for "
                          f"{len(shapes)} images")
    out = []
    for i, ((H, W), off) in enumerate(zip(shapes, step_offsets)):
        mh, mw = map_shape(H, W, block)
        if off is None:
            out.append(np.zeros((mh, mw), dtype=np.int8))
            continue
        a = off.detach().cpu().numpy() if isinstance(off, torch.Tensor) else np.asarray(off)
        if a.dtype.kind not in "iu" or a.shape != (mh, mw):
            raise Iclr17Error(f"iclr17: codec: step_offsets[{i}] must be integers of shape "
                              f"[{mh}, {mw}] for a {H}x{W} image with block {block} (got {a.dtype} "
                              f"{tuple(a.shape)})")
        out.append(np.clip(a.astype(np.int64), 1 - STEPS, STEPS - 1).astype(np.int8))
    return out


# ------------------------------------------------------------------------------ batches
def as_u8_hwc(image) -> np.ndarray:
    """A uint8 HWC RGB array (numpy or torch) as a contiguous numpy array."""
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise Iclr17Error(f"iclr17: codec: images are uint8 HWC RGB arrays of at least 1x1 (got "
                          f"{a.dtype} {a.shape})")
    a = np.ascontiguousarray(a)
    return a if a.flags.writeable else a.copy()   # torch.from_numpy wants a writable array


def upload_packed(images: Sequence[np.ndarray], device):
    """The images back to back in one pinned buffer and one upload → (device uint8 tensor, byte
    offsets, [(H, W)])."""
    sizes = [im.size for im in images]
    offsets = [0] + list(np.cumsum(sizes)[:-1])
    host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
    flat = host.numpy()
    for im, o in zip(images, offsets):
        flat[o:o + im.size] = im.reshape(-1)
    return host.to(device, non_blocking=True), [int(o) for o in offsets], [im.shape[:2] for im in images]


TILE_WITH_MAP = ("iclr17: codec: tile with step_offsets / a step map: tiled step maps are not "
                 "built")
RDO_WITH_MAP = ("iclr17: codec: rdo with step_offsets / a step map: per-block rate–distortion "
                "optimised quantisation is not built")


def rdo_value(rdo) -> float:
    """``rdo`` (λ of rate–distortion optimised quantisation) checked on the host: a real number,
    not a bool, finite (as an fp32 value too) and ≥ 0 → float."""
    if isinstance(rdo, bool) or not isinstance(rdo, (int, float, np.integer, np.floating)):
        raise Iclr17Error(f"iclr17: codec: rdo must be a real number (got {rdo!r})")
    lam = float(rdo)
    if not (math.isfinite(lam) and 0.0 <= lam <= float(np.finfo(np.float32).max)):
        raise Iclr17Error(f"iclr17: codec: rdo must be finite and >= 0 (got {rdo!r})")
    return lam


PSNR_WITH_RDO = ("iclr17: codec: psnr with rdo: a quality target over rate–distortion optimised "
                 "levels is not built")
PSNR_WITH_MAP = ("iclr17: codec: psnr with step_offsets / a step map: a quality target over "
                 "per-block steps is not built")


MSSSIM_WITH_RDO = ("iclr17: codec: msssim with rdo: a quality target over rate–distortion optimised "
                   "levels is not built")
MSSSIM_WITH_MAP = ("iclr17: codec: msssim with step_offsets / a step map: a quality target over "
                   "per-block steps is not built")
MSSSIM_WITH_ESTIMATE = ("iclr17: codec: msssim with estimate=True: a guided probe order for "
                        "MS-SSIM is not built (distortion_sweep predicts squared error)")


def _per_image(name: str, value, n: int, check) -> List[float]:
    """A scalar or one value per image of a quality target, each through ``check``."""
    if isinstance(value, (list, tuple)):    # element by element: an array would turn a bool
        per = list(value)                   # among floats into 1.0
    else:
        per = [value] * n if np.ndim(value) == 0 else list(np.asarray(value).reshape(-1))
    if len(per) != n:
        raise Iclr17Error(f"iclr17: codec: {name} has {len(per)} values for {n} images")
    return [check(v.item() if isinstance(v, np.generic) else v) for v in per]


# ------------------------------------------------------------------------------ reconstruction
# Where the decoder places a level inside its bin: None / "centre" at Δ·ŷ, as ever;
# "centroid" at the bin's mean under the rate model; "zero" the same for the zero bin alone.
RECON_MODES = (None, "centre", "centroid", "zero")

_RECON_NOT_BUILT = {
    "psnr": "a quality target that knows the decoder's reconstruction points",
    "msssim": "a quality target that knows the decoder's reconstruction points",
    "refine": "refinement towards the decoder's reconstruction points",
}
RECON_WITH = {k: f"iclr17: codec: recon with {k}: {v} is not built (the search and the objective "
                 "assume bin centres)" for k, v in _RECON_NOT_BUILT.items()}


def recon_value(recon, strength=1.0) -> Optional[Tuple[str, float]]:
    """``recon`` / ``recon_strength`` checked on the host: ``recon`` one of None, "centre",
    "centroid", "zero"; ``strength`` a real number, not a bool, finite, in [0, 1]. → None for the
    bin centre (None, "centre"), else (mode, strength)."""
    if not (recon is None or isinstance(recon, str)) or recon not in RECON_MODES:
        raise Iclr17Error(f"iclr17: codec: recon must be one of {RECON_MODES} (got {recon!r})")
    if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)):
        raise Iclr17Error(f"iclr17: codec: recon_strength must be a real number (got {strength!r})")
    a = float(strength)
    if not (math.isfinite(a) and 0.0 <= a <= 1.0):
        raise Iclr17Error(f"iclr17: codec: recon_strength must be finite and in [0, 1] "
                          f"(got {strength!r})")
    return None if recon in (None, "centre") else (recon, a)


# ------------------------------------------------------------------------------ refinement
# refine_lr=None: the learning rate in units of Δ per Adam step that tools/refine_rd.py's sweep
# chose (profiles/refine_rd.txt)
DEFAULT_REFINE_LR = 0.003

_REFINE_NOT_BUILT = {
    "max_bytes": "refinement under a byte budget",
    "bpp": "refinement under a byte budget",
    "psnr": "refinement under a quality target",
    "msssim": "refinement under a quality target",
    "rdo": "refinement of rate–distortion optimised levels",
    "step_offsets": "refinement over per-block steps",
}
REFINE_WITH = {k: f"iclr17: codec: refine with {'step_offsets / a step map' if k == 'step_offsets' else k}"
                  f": {v} is not built" for k, v in _REFINE_NOT_BUILT.items()}
REFINE_NEEDS_LAMBDA = ("iclr17: codec: refine without refine_lambda: the objective bits + λ·SSE needs "
                       "its λ (train.py's units: 650.25 for the golden checkpoints)")
REFINE_IN_BF16 = ("iclr17: codec: refine in the bf16 precision mode: that mode has no training "
                  "kernels, and refining through another chain than the decoder's is not built")


def refine_value(refine) -> int:
    """``refine`` (gradient iterations of latent refinement) checked on the host: None (0) or an
    integer ≥ 0, not a bool → int."""
    if refine is None:
        return 0
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0:
        raise Iclr17Error(f"iclr17: codec: refine must be an integer >= 0 (got {refine!r})")
    return int(refine)


class MsssimLambda(float):
    """A ``refine_lambda`` whose distortion is MS-SSIM: J = bits + λ·H·W·(1 −
    MS-SSIM of the 8-bit decode), H·W times train.py's λ·(1 − MS-SSIM) + bpp. The objective rides
    on λ, whose unit it fixes; make one with ``msssim_lambda``."""
    __slots__ = ()

    def __repr__(self) -> str:
        return f"msssim_lambda({float(self)!r})"


def msssim_lambda(lam) -> MsssimLambda:
    """λ of latent refinement for MS-SSIM, checked as ``refine_lambda_value`` checks a plain one:
    ``compress_images(..., refine=K, refine_lambda=msssim_lambda(8.0))``."""
    return MsssimLambda(refine_lambda_value(float(lam) if isinstance(lam, MsssimLambda) else lam))


def refine_lambda_value(lam) -> float:
    """One ``refine_lambda`` checked on the host: a real number, not a bool, finite (as an fp32
    value too) and ≥ 0 → float; a ``MsssimLambda`` stays one."""
    if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)):
        raise Iclr17Error(f"iclr17: codec: refine_lambda must be a real number (got {lam!r})")
    v = float(lam)
    if not (math.isfinite(v) and 0.0 <= v <= float(np.finfo(np.float32).max)):
        raise Iclr17Error(f"iclr17: codec: refine_lambda must be finite and >= 0 (got {lam!r})")
    return MsssimLambda(v) if isinstance(lam, MsssimLambda) else v


REFINE_DISTORTIONS = ("mse", "ms-ssim")   # what refine_objective_kind answers; --refine-distortion
REFINE_MIXED_OBJECTIVES = ("iclr17: codec: refine_lambda mixes plain and MS-SSIM values: mixed "
                           "objectives in one call are not built")


def refine_objective_kind(lams) -> str:
    """"ms-ssim" when every λ is a ``MsssimLambda``, "mse" when none is; a mixture raises
    ``REFINE_MIXED_OBJECTIVES``."""
    kinds = {isinstance(v, MsssimLambda) for v in lams}
    if len(kinds) > 1:
        raise Iclr17Error(REFINE_MIXED_OBJECTIVES)
    return "ms-ssim" if kinds == {True} else "mse"


def refine_lr_value(lr) -> float:
    """``refine_lr`` checked on the host: None (``DEFAULT_REFINE_LR``) or a real number, not a
    bool, finite and > 0 → float. The Adam learning rate of image b is this times Δ_b."""
    if lr is None:
        return DEFAULT_REFINE_LR
    if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)):
        raise Iclr17Error(f"iclr17: codec: refine_lr must be a real number (got {lr!r})")
    v = float(lr)
    if not (math.isfinite(v) and v > 0.0):
        raise Iclr17Error(f"iclr17: codec: refine_lr must be finite and > 0 (got {lr!r})")
    return v


def refine_objective(bits: float, sse: int, lam: float) -> float:
    """J = bits + (λ/3)·SSE8/255² in float64, evaluated left to right as written here (the device
    evaluates the same operations, kernels.refine_keep): H·W times train.py's λ·mse + bpp of the
    8-bit decode."""
    return float(bits) + (float(lam) / 3.0) * float(int(sse)) / 65025.0


def refine_objective_msssim(bits: float, ms: float, lam: float, H: int, W: int) -> float:
    """J = bits + λ·(H·W)·(1 − MS-SSIM8) in float64, evaluated left to right as written here (the
    device evaluates the same operations, kernels.refine_keep_msssim; ``ms`` is the fp32 value,
    widened): H·W times train.py's λ·(1 − MS-SSIM) + bpp on the real 8-bit decode."""
    return float(bits) + float(lam) * float(int(H) * int(W)) * (1.0 - float(ms))


def rate_request(n: int, step=None, max_bytes=None, bpp=None, step_offsets=None, rdo=None,
                 tile=None, psnr=None, msssim=None, estimate: bool = False, refine=None,
                 refine_lambda=None, refine_lr=None):
    """The rate options of ``compress_images`` for ``n`` images, checked on the host before any
    device use → None (the plain path), ("step", index), ("budget", per-image values, is_bpp) or,
    for ``psnr`` (a quality target in dB, a scalar or one value per image; not with another rate
    option, ``rdo`` or ``step_offsets``; with ``tile``), ("quality", per-image values), or, for
    ``msssim`` (an MS-SSIM target in (0, 1), the fifth rate option, under ``psnr``'s rules and not
    with ``estimate=True``), ("msssim", per-image values).
    At most one option; a budget is a scalar or one value per image. ``step_offsets`` goes with
    any one of them, the option then giving the base index; alone it means the unit step. So does
    ``rdo`` (``rdo_value`` checks it); ``rdo`` with ``step_offsets`` raises. ``tile`` (the tile
    edge of tiled streams: 8, 16, 32 or 64) changes the layout and not the rate: it goes with every
    option but ``step_offsets``, with which it raises, and does not change the answer.

    ``refine`` (K > 0 iterations of latent refinement, ``refine_value``) goes with ``step`` (none
    given: the unit step) and ``tile`` and gives ("refine", index, K, per-image λ, learning rate);
    with ``max_bytes``, ``bpp``, ``psnr``, ``msssim``, ``rdo`` or ``step_offsets`` (``REFINE_WITH``),
    without ``refine_lambda`` (a scalar or one value per image, ``refine_lambda_value``) and in the
    bf16 precision mode it raises. ``refine`` 0 or None gives the request of the call without it.
    The λ carry the objective: ``msssim_lambda`` values (all of them: a mixture raises
    ``REFINE_MIXED_OBJECTIVES``) stay ``MsssimLambda`` in the request and mean MS-SSIM."""
    iters = refine_value(refine)
    if refine_lambda is not None:
        lams = _per_image("refine_lambda", refine_lambda, n, refine_lambda_value)
        refine_objective_kind(lams)   # one objective per call
    lr = refine_lr_value(refine_lr)
    if iters:
        for name, v in (("max_bytes", max_bytes), ("bpp", bpp), ("psnr", psnr), ("msssim", msssim),
                        ("rdo", rdo), ("step_offsets", step_offsets)):
            if v is not None:
                raise Iclr17Error(REFINE_WITH[name])
        if refine_lambda is None:
            raise Iclr17Error(REFINE_NEEDS_LAMBDA)
        if kernels.precision() == "bf16":
            raise Iclr17Error(REFINE_IN_BF16)
    if tile is not None:
        if (isinstance(tile, bool) or not isinstance(tile, (int, np.integer))
                or tile not in kernels.TILES):
            raise Iclr17Error(f"iclr17: codec: tile must be one of {kernels.TILES} latent positions "
                              f"(got {tile!r})")
        if step_offsets is not None:
            raise Iclr17Error(TILE_WITH_MAP)
    if rdo is not None:
        rdo_value(rdo)
        if step_offsets is not None:
            raise Iclr17Error(RDO_WITH_MAP)
    given = [k for k, v in (("step", step), ("max_bytes", max_bytes), ("bpp", bpp), ("psnr", psnr),
                            ("msssim", msssim)) if v is not None]
    if len(given) > 1:
        raise Iclr17Error(f"iclr17: codec: {' and '.join(given)} given together (at most one of "
                          f"step, max_bytes, bpp{'' if psnr is None else ', psnr'}"
                          f"{'' if msssim is None else ', msssim'})")
    if psnr is not None:
        per = _per_image("psnr", psnr, n, psnr_value)
        if rdo is not None:
            raise Iclr17Error(PSNR_WITH_RDO)
        if step_offsets is not None:
            raise Iclr17Error(PSNR_WITH_MAP)
        return "quality", per
    if msssim is not None:
        per = _per_image("msssim", msssim, n, msssim_value)
        if rdo is not None:
            raise Iclr17Error(MSSSIM_WITH_RDO)
        if step_offsets is not None:
            raise Iclr17Error(MSSSIM_WITH_MAP)
        if estimate:
            raise Iclr17Error(MSSSIM_WITH_ESTIMATE)
        return "msssim", per
    if not given and iters:
        return "refine", UNIT_STEP, iters, lams, lr
    if not given:
        return None if step_offsets is None and rdo is None else ("step", UNIT_STEP)
    if step is not None:
        step_size(step)
        return ("refine", int(step), iters, lams, lr) if iters else ("step", int(step))
    value = max_bytes if max_bytes is not None else bpp
    per = [value] * n if np.ndim(value) == 0 else list(np.asarray(value).reshape(-1))
    if len(per) != n:
        raise Iclr17Error(f"iclr17: codec: {given[0]} has {len(per)} values for {n} images")
    if not all(np.isfinite(float(v)) and float(v) > 0 for v in per):
        raise Iclr17Error(f"iclr17: codec: {given[0]} must be finite and positive")
    return "budget", per, bpp is not None


# Plain bisection: measured on trained weights the guided order does not lower the mean probe count
# (DESIGN.md §0l), so ``estimate=True`` is an option and not the default.
DEFAULT_ESTIMATE = False


def quality_seeds(net, y) -> np.ndarray:
    """``search_quality``'s seeds of a latent batch: 255²·``net.distortion_sweep`` at the 32 ladder
    indices, float64 [B, 32] on the host — the SSE in 8-bit units that the linearised synthesis
    predicts the quantiser alone adds."""
    return 255.0 ** 2 * net.distortion_sweep(y, latent=True).cpu().numpy()


# What a probe measures on the device: the kernel's name in messages, its *_device wrapper, the
# bytes and dtype of a value in the buffer that comes back, and the host type of a value.
Measure = namedtuple("Measure", "what device_fn size dtype host")
SSE_MEASURE = Measure("image_sse", kernels.image_sse_device, 8, torch.int64, int)
MSSSIM_MEASURE = Measure("image_msssim", kernels.image_msssim_device, 4, torch.float32, float)


def quality_probe(net, y, packed, offsets, shapes, measure: Measure = SSE_MEASURE):
    """``search_quality``'s probe of one canvas batch: ``y`` its NHWC latent, ``packed`` /
    ``offsets`` / ``shapes`` the uploaded originals as ``upload_packed`` returns them. A call
    quantises every member at its own index (kernels.quantise_steps), runs the synthesis of the
    current precision mode as ``decompress`` does and sums the squared 8-bit error on the device
    (kernels.image_sse): no entropy coding, no 8-bit pixels, and 8·members + 8 bytes come back.
    The sums are those of the real decode at that index. Raises as ``quantise_step`` and
    ``image_egress`` do (in h3: ``H3_RANGE_MESSAGE``). With another ``measure`` the last step is
    that kernel's (``msssim_probe``)."""
    from . import chain
    device = y.device
    B = y.shape[0]
    Hc, Wc = canvas(*shapes[0])
    desc = kernels._image_desc(measure.what, packed.numel(), offsets, shapes, (Hc, Wc)).to(device)
    ladder = torch.tensor([step_size(s) for s in range(STEPS)], dtype=torch.float32, device=device)

    def probe(members, indices):
        pick = torch.tensor(members, device=device)
        whole = len(members) == B
        sel = y if whole else y[pick]
        steps_dev = ladder[torch.tensor(indices, device=device)]
        _, y_deq, qstatus = kernels.quantise_steps_device(sel, steps_dev, want_hat=False)
        m = chain.MODES[kernels.precision()]
        clipped, _, _ = m.synthesis(net.Decoder, y_deq, m.latent_operand(y_deq), None, False, False,
                                    None, False)
        buf, _, _, spare = measure.device_fn(clipped, None, None, packed,
                                             desc if whole else desc[pick].contiguous())
        spare.copy_(qstatus)
        host = buf.cpu()
        n = len(members)
        words = host[measure.size * n:].view(torch.int32)
        kernels._step_status(words[1:2], "quantise_steps")
        if int(words[0]):
            if kernels.precision() == "h3":
                raise Iclr17Error(kernels.H3_RANGE_MESSAGE)
            raise Iclr17Error(f"iclr17: {measure.what}: non-finite reconstruction")
        return [measure.host(v) for v in host[:measure.size * n].view(measure.dtype)]

    return probe


def msssim_probe(net, y, packed, offsets, shapes):
    """``quality_probe`` measuring MS-SSIM (kernels.image_msssim) in place of the squared error:
    per member the fp32 MS-SSIM of its 8-bit decode at its index against the original over its own
    H×W, as a float — the value ``evaluate_images(step=index, want_msssim=True)`` reports, bit for
    bit — and 4·members + 8 bytes come back. The images must be large enough for MS-SSIM
    (kernels.check_msssim_shapes): the caller checks, before any device use."""
    return quality_probe(net, y, packed, offsets, shapes, MSSSIM_MEASURE)


# what refine_loop leaves on the device: the best iterate's ŷ and the plain ŷ (fp32 NHWC), per
# image the iteration kept (int32; −1: none passed), its J, bits (float64) and SSE (int64) as the
# loop measured them, and iteration 0's bits and quantiser status (int32 [B]). With the MS-SSIM
# objective (``refine_loop(..., area=)``) ``best_sse`` holds the best iterate's MS-SSIM, fp32 [B]:
# the field is the distortion measure of the objective in hand.
RefineState = namedtuple("RefineState", "best plain best_iter best_J best_bits best_sse bits0 status0")


def refine_loop(net, y, steps_dev, lam, wt, packed, desc, iters: int, lr: float,
                mode: str, area=None) -> RefineState:
    """The K + 1 iterations of latent refinement on one canvas batch, without a
    host synchronisation: everything it decides is decided on the device. ``y``: the fp32 NHWC
    latent of ``net.latents`` (not modified); ``steps_dev`` fp32 [B] (Δ_b), ``lam`` float64 [B]
    (λ_b) and ``wt`` fp32 [B] (λ_b/3) on the device; ``packed`` / ``desc`` the uploaded originals
    and their checked descriptors on the device; ``mode`` a precision mode with training kernels,
    whose packs the caller has warmed (``net._warm_packs``: their first build may synchronise).

    Iteration t: ŷ_t = rint(y/Δ_b) and its bits (kernels.refine_step), the training forward of the
    synthesis from Δ_b·ŷ_t, the 8-bit SSE of its output over the image's own pixels
    (kernels.image_sse_device on the unclipped output, which the kernel clamps as the clipped one
    is: the same sums, and a non-finite value is seen), keep-the-best (kernels.refine_keep), and
    while t < K the gradient of the distortion through the synthesis
    (kernels.refine_grad_recon, autograd.synthesis_latent_grad) into the next refine_step, which
    adds the rate derivative straight through the rounding and takes the Adam step.

    With ``area`` (float64 [B], H_b·W_b, on the device) the distortion is MS-SSIM:
    ``wt`` is then g_b = −λ_b·H_b·W_b (fp32 [B]), the measure is kernels.image_msssim_fwd_saved on
    the unclipped output, the decision kernels.refine_keep_msssim and the gradient
    kernels.image_msssim_bwd, on a workspace made once before the loop; ``best_sse`` of the result
    holds the best iterate's MS-SSIM (fp32). The images have passed
    ``kernels.check_msssim_shapes``."""
    from . import chain
    from .autograd import synthesis_latent_grad
    m = chain.train_mode(mode)
    dec, rate = net.Decoder, net.bitEstimator.packed()
    dev, B = y.device, y.shape[0]
    y = y.clone().contiguous()
    mom, var = torch.zeros_like(y), torch.zeros_like(y)
    y_hat, y_deq, best = torch.empty_like(y), torch.empty_like(y), torch.zeros_like(y)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    flag = torch.zeros(B, device=dev, dtype=torch.int32)
    partial = kernels.refine_bits_partials(y)
    best_J = torch.full((B,), math.inf, device=dev, dtype=torch.float64)
    best_iter = torch.full((B,), -1, device=dev, dtype=torch.int32)
    best_bits = torch.zeros(B, device=dev, dtype=torch.float64)
    msssim = area is not None
    best_sse = torch.zeros(B, device=dev, dtype=torch.float32 if msssim else torch.int64)
    if msssim:
        ws = kernels.image_msssim_grad_workspace(B, 16 * y.shape[1], 16 * y.shape[2], dev)
        measured = (torch.empty(B, device=dev, dtype=torch.float32),
                    torch.empty(1, device=dev, dtype=torch.int32))
        d_recon = torch.empty(B, 3, 16 * y.shape[1], 16 * y.shape[2], device=dev)
    plain = bits0 = status0 = None
    with kernels.precision_scope(m.name):
        kernels.refine_step(y, steps_dev, rate, y_hat, y_deq, status, partial)
        for t in range(iters + 1):
            _, recon, _, saved = m.train_synthesis(dec, y_deq, None, None)
            if msssim:
                recon = recon.contiguous()   # the chain's NCHW output: no copy
                ms, rstatus = kernels.image_msssim_fwd_saved(recon, packed, desc, ws, measured)
                bits, _ = kernels.reduce_partials(partial)
                kernels.refine_keep_msssim(bits, ms, lam, area, status, rstatus, y_hat, t, best_J,
                                           best_iter, best_bits, best_sse, best, flag)
            else:
                _, sse, rstatus, _ = kernels.image_sse_device(recon, None, None, packed, desc)
                bits, _ = kernels.reduce_partials(partial)
                kernels.refine_keep(bits, sse, lam, status, rstatus, y_hat, t, best_J, best_iter,
                                    best_bits, best_sse, best, flag)
            if t == 0:
                plain, bits0, status0 = y_hat.clone(), bits, status.clone()
            if t < iters:
                g_recon = (kernels.image_msssim_bwd(recon, packed, desc, ws, wt, d_recon)
                           if msssim else kernels.refine_grad_recon(recon, packed, desc, wt))
                g_y = synthesis_latent_grad(dec, saved, g_recon, mode=m.name)
                kernels.refine_step(y, steps_dev, rate, y_hat, y_deq, status, partial,
                                    g_deq=g_y.contiguous(), m=mom, v=var, lr=lr, t=t + 1)
    return RefineState(best, plain, best_iter, best_J, best_bits, best_sse, bits0, status0)


def refine_latents(net, y, indices: Sequence[int], lams: Sequence[float], packed, offsets, shapes,
                   iters: int, lr: Optional[float] = None, stats: Optional[dict] = None):
    """``ImageCompressor.refine_latents``: the ŷ to code (fp32 NHWC, integer-valued) for one canvas
    batch after ``iters`` iterations of refinement. ``y``: its latent (``net.latents``);
    ``indices`` / ``lams``: per image the ladder index and λ; ``packed`` / ``offsets`` / ``shapes``
    the originals as ``upload_packed`` returns them.

    After ``refine_loop`` the choice is judged as ``evaluate_images`` measures: the best iterate
    and the plain ŷ = rint(y/Δ) are synthesised through the eval chain of the current precision
    mode (as a decoder does), ``image_sse`` is taken on both, and with the bits the loop summed
    J = ``refine_objective`` of both; the best iterate is coded only where its J is strictly lower
    (a non-finite decode counts as +inf), else the plain ŷ. One transfer, the call's only
    synchronisation. ``stats`` (a dict) receives per image "refine_kept" (the iteration coded; 0:
    the plain ŷ), "objective", "objective_plain" and "refine_iters".

    With ``MsssimLambda`` values in ``lams`` (all of them) the images must pass
    ``kernels.check_msssim_shapes``, the judge takes ``image_msssim`` on both decodes and
    J = ``refine_objective_msssim``; a NaN J (an MS-SSIM that is NaN: a level's mean is not
    positive) counts as +inf on either side, as the device's "NaN is not better". ``stats`` then
    also receives "refine_distortion" ("ms-ssim"), "ms_ssim" and "ms_ssim_plain", the judged values."""
    from . import chain
    mode = kernels.precision()
    if mode == "bf16":
        raise Iclr17Error(REFINE_IN_BF16)
    iters, lr = refine_value(iters), refine_lr_value(lr)
    kernels._check(y, "latent", 4)
    B, dev = y.shape[0], y.device
    if not (len(indices) == len(lams) == len(shapes) == B):
        raise Iclr17Error(f"iclr17: codec: refine_latents takes one index, λ and shape per image "
                          f"for {B} images")
    lams = [refine_lambda_value(v) for v in lams]
    msssim = refine_objective_kind(lams) == "ms-ssim"
    if msssim:   # on the host, before any device work
        kernels.check_msssim_shapes(shapes, [f"image {b} ({H}x{W})" for b, (H, W) in enumerate(shapes)])
    Hc, Wc = canvas(*shapes[0])
    if (y.shape[1], y.shape[2]) != (Hc // 16, Wc // 16):
        raise Iclr17Error("iclr17: codec: refine_latents: the latent is not the canvas batch's")
    desc = kernels._image_desc("refine", packed.numel(), offsets, shapes, (Hc, Wc))
    host = torch.empty(B, 4, dtype=torch.float64, pin_memory=True)
    for b in range(B):
        area = float(int(shapes[b][0]) * int(shapes[b][1]))
        # the weight of the distortion gradient: λ_b/3 on 2·(recon − x), or ∂J/∂MS-SSIM_b
        weight = float(np.float32(-(float(lams[b]) * area))) if msssim else lams[b] / 3.0
        host[b, 0], host[b, 1], host[b, 2], host[b, 3] = step_size(indices[b]), lams[b], weight, area
    args = host.to(dev, non_blocking=True)
    steps_dev, lam = args[:, 0].float().contiguous(), args[:, 1].contiguous()
    wt = args[:, 2].float().contiguous()
    desc = desc.pin_memory().to(dev, non_blocking=True)
    net._warm_packs(backward=True, mode=mode)
    net._warm_packs(mode=mode)
    st = refine_loop(net, y, steps_dev, lam, wt, packed, desc, iters, lr, mode,
                     area=args[:, 3].contiguous() if msssim else None)
    em = chain.MODES[mode]
    measure = MSSSIM_MEASURE if msssim else SSE_MEASURE

    def decode_measure(y_hat):
        y_deq = y_hat * steps_dev.view(B, 1, 1, 1)   # the fp32 product dequantise_step writes
        clipped, _, _ = em.synthesis(net.Decoder, y_deq, em.latent_operand(y_deq), None, False,
                                     False, None, False)
        return measure.device_fn(clipped, None, None, packed, desc)[0]

    parts = [decode_measure(st.best), decode_measure(st.plain), st.best_bits.view(torch.uint8),
             st.bits0.view(torch.uint8), st.best_iter.view(torch.uint8),
             st.status0.view(torch.uint8)]
    flat = torch.cat(parts).cpu().numpy()
    size = measure.size * B
    n = size + 8
    dt = np.float32 if msssim else np.int64
    got_b, bad_b = flat[:size].view(dt), int(flat[size:size + 4].view(np.int32)[0])
    got_p = flat[n:n + size].view(dt)
    bad_p = int(flat[n + size:n + size + 4].view(np.int32)[0])
    rest = flat[2 * n:]
    bits_b, bits_p = rest[:8 * B].view(np.float64), rest[8 * B:16 * B].view(np.float64)
    kept = rest[16 * B:20 * B].view(np.int32)
    kernels._step_status(torch.from_numpy(np.bitwise_or.reduce(rest[20 * B:24 * B].view(np.int32),
                                                               keepdims=True).copy()),
                         "quantise_steps")

    def objective(b, bits, got):
        if msssim:   # NaN (a NaN MS-SSIM): not better than anything, so +inf
            J = refine_objective_msssim(bits[b], got[b], lams[b], *shapes[b])
            return math.inf if math.isnan(J) else J
        return refine_objective(bits[b], got[b], lams[b])

    use, J, J_plain = [], [], []
    for b in range(B):
        jp = math.inf if bad_p else objective(b, bits_p, got_p)
        jb = math.inf if bad_b or kept[b] <= 0 else objective(b, bits_b, got_b)
        use.append(jb < jp)
        J.append(jb if use[b] else jp)
        J_plain.append(jp)
    if any(use):
        pick = torch.tensor(use).pin_memory().to(dev, non_blocking=True)
        y_hat = torch.where(pick.view(B, 1, 1, 1), st.best, st.plain)
    else:
        y_hat = st.plain
    if stats is not None:
        stats["refine_kept"] = [int(kept[b]) if use[b] else 0 for b in range(B)]
        stats["objective"], stats["objective_plain"] = J, J_plain
        stats["refine_iters"] = [iters] * B
        if msssim:
            stats["refine_distortion"] = ["ms-ssim"] * B
            stats["ms_ssim"] = [float(got_b[b] if use[b] else got_p[b]) for b in range(B)]
            stats["ms_ssim_plain"] = [float(got_p[b]) for b in range(B)]
    return y_hat


def compress_images(net, images, max_batch: int = 64,
                    streams_per_image: int = kernels.STREAMS_PER_IMAGE,
                    K: int = kernels.ENTROPY_K, step: Optional[int] = None, max_bytes=None,
                    bpp=None, stats: Optional[dict] = None, step_offsets=None,
                    block: int = DEFAULT_BLOCK, rdo=None, rdo_weights=None,
                    tile: Optional[int] = None, psnr=None, estimate: bool = DEFAULT_ESTIMATE,
                    msssim=None, refine=None, refine_lambda=None, refine_lr=None) -> List[bytes]:
    imgs = [as_u8_hwc(im) for im in images]
    request = rate_request(len(imgs), step, max_bytes, bpp, step_offsets, rdo, tile, psnr, msssim,
                           estimate, refine, refine_lambda, refine_lr)
    refine_msssim = (request is not None and request[0] == "refine"
                     and refine_objective_kind(request[3]) == "ms-ssim")
    if (request is not None and request[0] == "msssim") or refine_msssim:   # on the host, before the ingest
        sizes = [im.shape[:2] for im in imgs]
        kernels.check_msssim_shapes(sizes, [f"image {i} ({H}x{W})" for i, (H, W) in enumerate(sizes)])
    how = {} if rdo is None else {"rdo": rdo, "rdo_weights": rdo_weights}
    per_image = None
    if step_offsets is not None:
        per_image = checked_offsets([im.shape[:2] for im in imgs], step_offsets, block)
    device = next(net.parameters()).device
    fp, N, P = fingerprint(net), net.out_channel_N, streams_per_image
    blobs: List[Optional[bytes]] = [None] * len(imgs)
    budgets: List[Optional[int]] = [None] * len(imgs)
    if request is not None and request[0] == "budget":
        for i, (im, v) in enumerate(zip(imgs, request[1])):
            budgets[i] = int(math.floor(float(v) * im.shape[0] * im.shape[1] / 8)) if request[2] else int(v)
    reencodes = [0] * len(imgs)
    probes, sses = [0] * len(imgs), [None] * len(imgs)
    refined = {k: [None] * len(imgs) for k in ("refine_kept", "objective", "objective_plain",
                                               "refine_iters")
               + (("refine_distortion", "ms_ssim", "ms_ssim_plain") if refine_msssim else ())}
    for idx in group_by_canvas([im.shape[:2] for im in imgs], max_batch):
        group = [imgs[i] for i in idx]
        packed, offsets, shapes = upload_packed(group, device)
        x = kernels.image_ingest(packed, offsets, shapes, canvas(*shapes[0]))
        if request is None and tile is not None:   # compress's own ŷ, tiled, at the unit index
            enc = net.compress(x, streams_per_image=P, K=K, tile=tile)
            for i, (H, W), s in zip(idx, shapes, enc["strings"]):
                blobs[i] = pack_tile_header(P, N, K, UNIT_STEP, tile, H, W, fp) + s
            continue
        if request is None:
            enc = net.compress(x, streams_per_image=P, K=K)
            for i, (H, W), s in zip(idx, shapes, enc["strings"]):
                blobs[i] = pack_header(P, N, K, H, W, fp) + s
            continue
        # one analysis pass per batch, however many steps and re-encodes follow
        y = net.latents(x)
        # with step offsets: the batch's maps [B, mh, mw]; a step is then the BASE index, and a
        # blob also carries its map
        offs = None if per_image is None else np.stack([per_image[i] for i in idx])
        overhead = blob_overhead(P) + (0 if offs is None else offs[0].size)
        if tile is not None:
            overhead = tiled_blob_overhead(P, *shapes[0], tile)   # one canvas: one tile grid
        if request[0] == "refine":   # the refined ŷ, coded as the step's own
            _, s, iters, lams, lr = request
            got: dict = {}
            y_hat = refine_latents(net, y, [s] * len(idx), [lams[i] for i in idx], packed, offsets,
                                   shapes, iters, lr, got)
            enc = net._entropy_code(y_hat, net.bitEstimator.entropy_tables(K, step=s), P, K,
                                    tile=tile)
            for k, (i, (H, W), string) in enumerate(zip(idx, shapes, enc["strings"])):
                head = (pack_step_header(P, N, K, s, H, W, fp) if tile is None
                        else pack_tile_header(P, N, K, s, tile, H, W, fp))
                blobs[i] = head + string
                for name in refined:
                    refined[name][i] = got[name][k]
            continue
        if request[0] == "step":
            chosen = [request[1]] * len(idx)
        elif request[0] == "quality":
            targets = [QualityTarget(f"image {i} ({H}x{W})", request[1][i], H, W,
                                     sse_limit(H, W, request[1][i])) for i, (H, W) in zip(idx, shapes)]
            found = search_quality(quality_probe(net, y, packed, offsets, shapes), len(idx),
                                   quality_seeds(net, y) if estimate else None, targets)
            chosen = found.indices
            for k, i in enumerate(idx):
                probes[i], sses[i] = found.probes[k], found.sse[k]
        elif request[0] == "msssim":
            targets = [MsssimTarget(f"image {i} ({H}x{W})", request[1][i], H, W)
                       for i, (H, W) in zip(idx, shapes)]
            found = search_quality(msssim_probe(net, y, packed, offsets, shapes), len(idx), None,
                                   targets, msssim_passes, msssim_failure)
            chosen = found.indices
            for k, i in enumerate(idx):
                probes[i], sses[i] = found.probes[k], found.sse[k]
        else:
            est = (net.rate_sweep(y, latent=True, **how) if offs is None
                   else net.rate_sweep_offsets(y, offs, block)).cpu().numpy()
            chosen = []
            for k, i in enumerate(idx):
                try:
                    chosen.append(choose_step(est[k], budgets[i], overhead))
                except Iclr17Error:
                    chosen.append(STEPS - 1)   # no estimate fits: the coarsest step decides below

        def encode(ks, s):
            sel = y if len(ks) == len(idx) else y[torch.tensor(ks, device=device)]
            if tile is not None:
                enc = net.compress_latents(sel, s, streams_per_image=P, K=K, tile=tile, **how)
                return [pack_tile_header(P, N, K, s, tile, *shapes[k], fp) + string
                        for k, string in zip(ks, enc["strings"])]
            if offs is None:
                enc = net.compress_latents(sel, s, streams_per_image=P, K=K, **how)
                return [pack_step_header(P, N, K, s, *shapes[k], fp) + string
                        for k, string in zip(ks, enc["strings"])]
            emap = effective_indices(s, offs[ks])
            enc = net.compress_latents(sel, None, streams_per_image=P, K=K, step_map=emap,
                                       block=block)
            return [pack_map_header(P, N, K, s, block, *shapes[k], fp, m) + string
                    for k, m, string in zip(ks, emap, enc["strings"])]

        coded, again = encode_to_budget(chosen, [budgets[i] for i in idx], encode,
                                        [f"image {i} ({H}x{W})" for i, (H, W) in zip(idx, shapes)])
        for i, blob, n in zip(idx, coded, again):
            blobs[i], reencodes[i] = blob, n
    if stats is not None:
        stats["reencodes"] = reencodes
        if request is not None and request[0] == "quality":
            stats["probes"], stats["sse"] = probes, sses
        if request is not None and request[0] == "msssim":
            stats["probes"], stats["ms_ssim"] = probes, sses
        if request is not None and request[0] == "refine":
            stats.update(refined)
    return blobs


def decode_groups(net, blobs, max_batch: int, refs=None, recon=None, recon_strength=1.0):
    """``decompress_images``; with ``refs`` (the original uint8 images, one per blob) also each
    image's Σ (decoded − original)² → ([uint8 HWC arrays], [int] | None). ``recon`` /
    ``recon_strength``: ``recon_value``'s, for every blob of the call."""
    recon_value(recon, recon_strength)   # before any device use
    how_recon = {} if recon is None else {"recon": recon, "recon_strength": recon_strength}
    device = next(net.parameters()).device
    fp, N = fingerprint(net), net.out_channel_N
    parsed = [parse_blob(b, N, fp) for b in blobs]
    heads, steps = [h for h, _ in parsed], [s for _, s in parsed]
    starts = [s.payload if isinstance(s, StepMap) else HEADER.size for s in steps]
    for b, h, start in zip(blobs, heads, starts):
        # decompress reads the payload as 16-bit words and checks the counts; an odd rest cannot
        # even be read that way
        if len(b) < start + 4 * h.P or (len(b) - start) % 2:
            raise Iclr17Error(f"iclr17: codec: truncated stream ({len(b)} bytes)")
    out: List[Optional[np.ndarray]] = [None] * len(blobs)
    sses: Optional[List[Optional[int]]] = [None] * len(blobs) if refs is not None else None
    # a batch: one canvas, P, K and step; mapped blobs of one block edge batch whatever their
    # maps, tiled blobs of one step and tile edge together
    def kind(s):
        if isinstance(s, StepMap):
            return "map", s.block
        return ("tile", s.step, s.tile) if isinstance(s, TileInfo) else s
    keys = [canvas(h.H, h.W) + (h.P, h.K, kind(s)) for h, s in parsed]
    for idx in _group(keys, max_batch):
        h0, s0 = heads[idx[0]], steps[idx[0]]
        Hc, Wc = canvas(h0.H, h0.W)
        how = {"step": s0}
        if isinstance(s0, StepMap):
            how = {"step_map": np.stack([steps[i].indices for i in idx]), "block": s0.block}
        if isinstance(s0, TileInfo):
            how = {"step": s0.step, "tile": s0.tile}
        dec = net.decompress([blobs[i][starts[i]:] for i in idx], (Hc // 16, Wc // 16),
                             streams_per_image=h0.P, K=h0.K, device=device, **how, **how_recon)
        shapes = [(heads[i].H, heads[i].W) for i in idx]
        ref = None
        if refs is not None:
            group = [refs[i] for i in idx]
            if [g.shape[:2] for g in group] != shapes:
                raise Iclr17Error("iclr17: codec: a reference image's size differs from its stream's")
            ref, offsets, _ = upload_packed(group, device)
        else:
            offsets = [int(o) for o in np.cumsum([0] + [3 * H * W for H, W in shapes[:-1]])]
        dst, sse = kernels.image_egress(dec["x_hat"], offsets, shapes, ref)
        flat = dst.numpy()
        for k, (i, o, (H, W)) in enumerate(zip(idx, offsets, shapes)):
            out[i] = flat[o:o + 3 * H * W].reshape(H, W, 3).copy()
            if sses is not None:
                sses[i] = int(sse[k])
    return out, sses


def decode_region(net, blob, box, stats: Optional[dict] = None, recon=None,
                  recon_strength=1.0) -> np.ndarray:
    """``ImageCompressor.decompress_region``: the pixels ``box`` of one blob → uint8 [y1 − y0,
    x1 − x0, 3]. A tiled blob: the streams of ``region_window``'s tile rectangle are decoded into
    a compact latent (kernels.rans_decode_tiled), dequantised with the blob's step and synthesised
    as an image of its own; ``image_egress`` runs on the crop (from the 16-pixel grid line above
    and left of it: the egress takes canvases of multiples of 16). Any other blob is decoded
    whole and cropped. ``recon`` / ``recon_strength`` as ``decode_groups`` takes them: the compact
    latent is dequantised with the step's offsets (kernels.dequantise_recon)."""
    from . import chain
    rc = recon_value(recon, recon_strength)   # before any device use
    device = next(net.parameters()).device
    head, info = parse_blob(blob, net.out_channel_N, fingerprint(net))
    x0, y0, x1, y1 = _checked_box(head.H, head.W, box)
    if not isinstance(info, TileInfo):
        full = decode_groups(net, [blob], 1, recon=recon, recon_strength=recon_strength)[0][0]
        if stats is not None:
            stats["streams_decoded"] = stats["streams_total"] = head.P
        return np.ascontiguousarray(full[y0:y1, x0:x1])
    P, N, K, t = head.P, head.N, head.K, info.tile
    win = region_window(head.H, head.W, t, (x0, y0, x1, y1))
    r0, c0, r1, c1 = win.tiles
    Hc, Wc = canvas(head.H, head.W)
    # the rectangle's streams, in stream order, out of the blob's words
    flat = info.counts.reshape(-1)
    first = np.concatenate([[0], np.cumsum(flat)])
    th, tw = info.counts.shape[:2]
    picked = [(r * tw + c) * P + g for r in range(r0, r1) for c in range(c0, c1) for g in range(P)]
    words = np.frombuffer(bytes(blob[info.words:]), dtype="<u2")
    parts = [words[first[k]:first[k + 1]] for k in picked]
    off = np.concatenate([[0], np.cumsum([len(q) for q in parts])]).astype(np.int64)
    packed = np.concatenate(parts).view(np.int16).copy()
    y_hat = kernels.rans_decode_tiled(torch.from_numpy(packed).to(device),
                                      torch.from_numpy(off).to(device),
                                      net.bitEstimator.entropy_tables(K, step=info.step), 1,
                                      Hc // 16, Wc // 16, N, t, K, P, rect=win.tiles)
    if stats is not None:
        stats["streams_decoded"], stats["streams_total"] = len(picked), int(flat.size)
    if rc is None:
        y_deq = kernels.dequantise_step(y_hat, step_size(info.step))
    else:
        y_deq = kernels.dequantise_recon(y_hat, step_size(info.step),
                                         net.bitEstimator.recon_offsets(K, info.step, *rc), K)
    m = chain.MODES[kernels.precision()]
    clipped, _, _ = m.synthesis(net.Decoder, y_deq, m.latent_operand(y_deq), None, False, False,
                                None, False)
    dx, dy = win.offset
    X0, Y0 = dx // 16 * 16, dy // 16 * 16
    X1, Y1 = -(-(dx + x1 - x0) // 16) * 16, -(-(dy + y1 - y0) // 16) * 16
    shape = (dy - Y0 + y1 - y0, dx - X0 + x1 - x0)
    dst, _ = kernels.image_egress(clipped[:, :, Y0:Y1, X0:X1].contiguous(), [0], [shape])
    out = dst.numpy()[:3 * shape[0] * shape[1]].reshape(shape[0], shape[1], 3)
    return np.ascontiguousarray(out[dy - Y0:, dx - X0:])


def evaluate_images(net, images, want_msssim: bool = False, max_batch: int = 64,
                    step: Optional[int] = None, max_bytes=None, bpp=None, step_offsets=None,
                    block: int = DEFAULT_BLOCK, rdo=None, rdo_weights=None,
                    tile: Optional[int] = None, psnr=None,
                    estimate: bool = DEFAULT_ESTIMATE, recon=None, recon_strength=1.0,
                    msssim=None, refine=None, refine_lambda=None, refine_lr=None) -> List[dict]:
    # recon / recon_strength stand before the pinned tail (msssim, refine, refine_lambda,
    # refine_lr: DESIGN.md §0o); everything from step= on is meant to be passed by name
    rc = recon_value(recon, recon_strength)
    if rc is not None:   # the search and the objective assume bin centres
        for name, given in (("psnr", psnr is not None), ("msssim", msssim is not None),
                            ("refine", bool(refine_value(refine)))):
            if given:
                raise Iclr17Error(RECON_WITH[name])
    imgs = [as_u8_hwc(im) for im in images]
    stats: dict = {}
    blobs = compress_images(net, imgs, max_batch=max_batch, step=step, max_bytes=max_bytes, bpp=bpp,
                            step_offsets=step_offsets, block=block, rdo=rdo, rdo_weights=rdo_weights,
                            tile=tile, psnr=psnr, estimate=estimate, msssim=msssim, stats=stats,
                            refine=refine, refine_lambda=refine_lambda, refine_lr=refine_lr)
    want_msssim = want_msssim or msssim is not None
    recons, sses = decode_groups(net, blobs, max_batch, refs=imgs, recon=recon,
                                 recon_strength=recon_strength)
    device = next(net.parameters()).device
    res = []
    for im, blob, rec, sse in zip(imgs, blobs, recons, sses):
        H, W = im.shape[:2]
        r = {"bytes": len(blob), "bpp": 8 * len(blob) / (H * W), "sse_u8": sse,
             "psnr_u8": 10.0 * math.log10(255.0 ** 2 * 3 * H * W / sse) if sse else math.inf,
             "recon": rec, "step": parse_blob(blob)[1]}
        if isinstance(r["step"], StepMap):   # a mapped blob: its base index, and the map beside it
            r["step_map"], r["block"], r["step"] = r["step"].indices, r["step"].block, r["step"].base
        if isinstance(r["step"], TileInfo):  # a tiled blob: its ladder index, and the tile edge
            r["tile"], r["step"] = r["step"].tile, r["step"].step
        if want_msssim:
            r["ms_ssim"] = r["ms_ssim_db"] = None
            if kernels.query("iclr17_ms_ssim_workspace_size", 1, H, W):   # 0: too small for 5 levels
                def unit(a):
                    return (torch.from_numpy(a).to(device).permute(2, 0, 1).float() / 255)[None].contiguous()
                ms = float(kernels.ms_ssim(unit(rec), unit(im), data_range=1.0)[0])
                r["ms_ssim"] = ms
                r["ms_ssim_db"] = -10.0 * math.log10(1.0 - ms) if ms < 1.0 else math.inf
        for name in ("refine_kept", "objective", "objective_plain", "refine_iters"):
            if name in stats:
                r[name] = stats[name][len(res)]
        if recon is not None:   # "recon" is the decoded image: the mode goes by its own name
            r["recon_mode"], r["recon_strength"] = recon, float(recon_strength)
        if "refine_distortion" in stats:   # an MS-SSIM refinement: the judged values (with
            for name in ("refine_distortion", "ms_ssim", "ms_ssim_plain"):   # want_msssim the decode's
                r.setdefault(name, stats[name][len(res)])                    # own: the same bits)
        res.append(r)
    return res


# ------------------------------------------------------------------------------ command line
def _load_image(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))   # datasets.py:21


def _model(args):
    from .model import ImageCompressor, load_model
    if not torch.cuda.is_available():
        raise Iclr17Error("iclr17: codec: no ROCm GPU (MI355X / gfx950) — there is no CPU implementation")
    net = ImageCompressor(out_channel_N=args.N)
    load_model(net, args.weights)
    return net.to(torch.device("cuda:0")).eval()


def _boxes(texts: Sequence[str]) -> List[Tuple[int, int, int, int, int]]:
    """--roi X0,Y0,X1,Y1,OFF arguments as ``roi_offsets`` boxes."""
    boxes = []
    for t in texts:
        try:
            box = tuple(int(v) for v in t.split(","))
        except ValueError:
            box = ()
        if len(box) != 5:
            raise Iclr17Error(f"iclr17: codec: --roi takes X0,Y0,X1,Y1,OFF as five integers (got {t!r})")
        boxes.append(box)
    return boxes


def _region(text: str) -> Tuple[int, int, int, int]:
    """A --region X0,Y0,X1,Y1 argument as a ``decompress_region`` box."""
    try:
        box = tuple(int(v) for v in text.split(","))
    except ValueError:
        box = ()
    if len(box) != 4:
        raise Iclr17Error(f"iclr17: codec: --region takes X0,Y0,X1,Y1 as four integers (got {text!r})")
    return box


def build_parser() -> argparse.ArgumentParser:
    """The command line's parser (no device use)."""
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--weights", required=True, help="checkpoint (model.load_model)")
    common.add_argument("--N", type=int, default=192, help="channel count of the checkpoint")
    common.add_argument("--precision", choices=kernels.PRECISIONS, default=None)
    ap = argparse.ArgumentParser(prog="python -m iclr_17_compression_amd.codec",
                                 description="Code 8-bit RGB image files with the Ballé-2017 codec.")
    sub = ap.add_subparsers(dest="cmd", required=True)
    enc = sub.add_parser("encode", parents=[common], help="IN.png OUT.i17c")
    enc.add_argument("input")
    enc.add_argument("output")
    rate = enc.add_mutually_exclusive_group()
    rate.add_argument("--step", type=int, default=None, help="ladder index 0..31 (8: the unit step)")
    rate.add_argument("--max-bytes", type=int, default=None, help="byte budget of the output file")
    rate.add_argument("--bpp", type=float, default=None, help="budget in bits per pixel of the file")
    rate.add_argument("--psnr", type=float, default=None, metavar="T",
                      help="quality target in dB: the coarsest ladder index found whose 8-bit "
                           "decode reaches T (not with --rdo or --roi)")
    rate.add_argument("--msssim", type=float, default=None, metavar="T",
                      help="MS-SSIM target, 0 < T < 1: the coarsest ladder index found whose "
                           "8-bit decode reaches T (not with --rdo or --roi; both sides of the "
                           "image at least 161)")
    enc.add_argument("--roi", action="append", default=None, metavar="X0,Y0,X1,Y1,OFF",
                     help="a pixel box whose blocks get the ladder offset OFF (negative: finer); "
                          "repeatable, the finest offset wins where boxes overlap")
    enc.add_argument("--block", type=int, default=DEFAULT_BLOCK, choices=kernels.MAP_BLOCKS,
                     help="block edge of the step map in latent positions (16 pixels each)")
    enc.add_argument("--rdo", type=float, default=None, metavar="L",
                     help="rate-distortion optimised quantisation with lambda L >= 0 (alone: at "
                          "the unit step; not with --roi)")
    enc.add_argument("--tile", type=int, default=None, choices=kernels.TILES, metavar="T",
                     help="independent streams per tile of T x T latent positions (16 pixels "
                          "each; 8, 16, 32 or 64): parallel coding of a large image and region "
                          "decode (not with --roi)")
    _refine_arguments(enc, "--step or none (the unit step) and --tile")
    dec = sub.add_parser("decode", parents=[common], help="IN.i17c OUT.png")
    dec.add_argument("input")
    dec.add_argument("output")
    dec.add_argument("--region", default=None, metavar="X0,Y0,X1,Y1",
                     help="decode this pixel box alone (half-open); of a tiled stream only the "
                          "tiles it needs are decoded")
    _recon_arguments(dec)
    ev = sub.add_parser("eval", parents=[common], help="IMG...: one JSON line per image and a mean")
    ev.add_argument("images", nargs="+")
    ev.add_argument("--ms-ssim", action="store_true")
    ev.add_argument("--steps", default=None, help="ladder indices, e.g. 4,8,12: a row per image "
                                                  "and step, and a mean per step")
    ev.add_argument("--rdo", type=float, default=None, metavar="L",
                    help="rate-distortion optimised quantisation with lambda L >= 0")
    ev.add_argument("--psnr", type=float, default=None, metavar="T",
                    help="quality target in dB per image (not with --steps or --rdo)")
    ev.add_argument("--msssim", type=float, default=None, metavar="T",
                    help="MS-SSIM target per image (not with --steps, --rdo or --psnr)")
    _refine_arguments(ev, "--steps or none")
    _recon_arguments(ev)
    return ap


def _recon_arguments(parser) -> None:
    parser.add_argument("--recon", choices=[m for m in RECON_MODES if m], default=None, metavar="M",
                        help="where the decoder places a level in its bin: centre (the default), "
                             "centroid (the bin's mean under the rate model) or zero (the mean "
                             "for the zero bin alone); costs no bits, any stream decodes with it")
    parser.add_argument("--recon-strength", type=float, default=1.0, metavar="A",
                        help="0 <= A <= 1: the share of the way from the centre to the mean")


def _refine_arguments(parser, goes_with: str) -> None:
    parser.add_argument("--refine", type=int, default=None, metavar="K",
                        help="K gradient iterations of latent refinement: lower bits + lambda * SSE "
                             f"of this image, any decoder reads the result (with {goes_with}; "
                             "needs --refine-lambda)")
    parser.add_argument("--refine-lambda", type=float, default=None, metavar="L",
                        help="lambda of the refinement objective in the training loss's units "
                             "(lambda * mse + bpp)")
    parser.add_argument("--refine-lr", type=float, default=None, metavar="R",
                        help="Adam learning rate of the refinement in units of the quantiser "
                             f"step (default {DEFAULT_REFINE_LR})")
    parser.add_argument("--refine-distortion", choices=REFINE_DISTORTIONS, default="mse",
                        help="the distortion of the refinement objective: mse (lambda * mse + bpp) "
                             "or ms-ssim (lambda * (1 - MS-SSIM) + bpp; both sides of the image at "
                             f"least {kernels.MSSSIM_MIN_SIDE})")


def _refine_of(args) -> dict:
    lam = args.refine_lambda
    if lam is not None and args.refine_distortion == "ms-ssim":
        lam = msssim_lambda(lam)
    return {"refine": args.refine, "refine_lambda": lam, "refine_lr": args.refine_lr}


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    if getattr(args, "psnr", None) is not None:   # before the device is touched
        rate_request(1, step=getattr(args, "step", None), rdo=args.rdo, psnr=args.psnr,
                     step_offsets=[None] if getattr(args, "roi", None) else None)
        if getattr(args, "steps", None):
            raise Iclr17Error("iclr17: codec: step and psnr given together (at most one of step, "
                              "max_bytes, bpp, psnr)")
    if getattr(args, "msssim", None) is not None:   # the same, for the MS-SSIM target
        rate_request(1, step=getattr(args, "step", None), rdo=args.rdo,
                     psnr=getattr(args, "psnr", None), msssim=args.msssim,
                     step_offsets=[None] if getattr(args, "roi", None) else None)
        if getattr(args, "steps", None):
            raise Iclr17Error("iclr17: codec: step and msssim given together (at most one of step, "
                              "max_bytes, bpp, msssim)")
    if getattr(args, "refine", None) is not None:   # the same, for refinement
        with kernels.precision_scope(args.precision or kernels.precision()):
            rate_request(1, step=getattr(args, "step", None),
                         max_bytes=getattr(args, "max_bytes", None), bpp=getattr(args, "bpp", None),
                         rdo=args.rdo, psnr=args.psnr, msssim=args.msssim,
                         step_offsets=[None] if getattr(args, "roi", None) else None,
                         **_refine_of(args))
    if args.cmd != "encode":   # the same, for the reconstruction point
        how_recon = ({} if args.recon is None and args.recon_strength == 1.0 else
                     {"recon": args.recon, "recon_strength": args.recon_strength})
        if recon_value(args.recon, args.recon_strength) is not None:
            for name in ("psnr", "msssim", "refine"):
                if getattr(args, name, None):
                    raise Iclr17Error(RECON_WITH[name])
    net = _model(args)
    with kernels.precision_scope(args.precision or kernels.precision()):
        if args.cmd == "encode":
            image, roi = _load_image(args.input), {}
            if args.roi:
                roi = {"step_offsets": [roi_offsets(*image.shape[:2], _boxes(args.roi), args.block)],
                       "block": args.block}
            blob = net.compress_images([image], step=args.step, max_bytes=args.max_bytes,
                                       bpp=args.bpp, rdo=args.rdo, tile=args.tile,
                                       psnr=args.psnr, msssim=args.msssim, **roi,
                                       **_refine_of(args))[0]
            with open(args.output, "wb") as f:
                f.write(blob)
        elif args.cmd == "decode":
            from PIL import Image
            with open(args.input, "rb") as f:
                blob = f.read()
            if args.region is None:
                image = net.decompress_images([blob], **how_recon)[0]
            else:
                image = net.decompress_region(blob, _region(args.region), **how_recon)
            Image.fromarray(image).save(args.output, format="PNG")
        else:
            imgs = [_load_image(p) for p in args.images]
            steps = [int(t) for t in args.steps.split(",")] if args.steps else [None]
            for step in steps:
                rows = net.evaluate_images(imgs, want_msssim=args.ms_ssim, step=step,
                                           rdo=args.rdo, psnr=args.psnr, msssim=args.msssim,
                                           **_refine_of(args), **how_recon)
                tag = {} if step is None else {"step": step}
                if args.recon is not None:
                    tag["recon"] = args.recon
                    tag["recon_strength"] = args.recon_strength
                if args.psnr is not None:
                    tag["psnr"] = args.psnr
                if args.msssim is not None:
                    tag["msssim"] = args.msssim
                if args.rdo is not None:
                    tag["rdo"] = args.rdo
                if args.refine:
                    tag["refine"] = args.refine
                    if args.refine_distortion != "mse":
                        tag["refine_distortion"] = args.refine_distortion
                for p, im, r in zip(args.images, imgs, rows):
                    print(json.dumps({"name": p, **tag, "H": im.shape[0], "W": im.shape[1],
                                      "bytes": r["bytes"], "bpp": r["bpp"], "psnr_u8": r["psnr_u8"],
                                      "ms_ssim": r.get("ms_ssim"),
                                      **({} if args.psnr is None and args.msssim is None
                                         else {"index": r["step"]})}))
                ms = [r["ms_ssim"] for r in rows if r.get("ms_ssim") is not None]
                print(json.dumps({"name": "mean", **tag, "images": len(rows),
                                  "bpp": float(np.mean([r["bpp"] for r in rows])),
                                  "psnr_u8": float(np.mean([r["psnr_u8"] for r in rows])),
                                  "ms_ssim": float(np.mean(ms)) if ms else None}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
