"""The definition of rate–distortion optimised quantisation in plain numpy, the
inputs its tests share and their bars.

For one element of channel c at the step Δ (an fp32 ``codec.step_size`` value):

    t = y/Δ (IEEE fp32 divide),  r = rint(t) (half to even): quantise_step's own expressions
    candidates, in this order:  c0 = r;  c1 = r − sign(r) when r ≠ 0;  c2 = 0 when |r| ≥ 2
    J(v) = bits(v) + w_c·(v − t)²,  w_c = lam[c]·Δ·Δ evaluated left to right
    bits(v) = clamp(−log(F(v + ½) − F(v − ½) + 1e-10)/ln 2, 0, 50) on the step pack of Δ
    the pick: the first candidate of least J (a strict < moves the pick to a later candidate)
    ŷ = the pick,  y_deq = Δ·ŷ

``dtype=np.float32`` is the definition, op for op what the kernels evaluate (the step pack's row 0
is one fp32 product, the divisor ln 2 the fp32 value nearest to it); ``np.float64`` is its
evaluation without fp32 rounding ON THE SAME t, w and step pack, which are fp32 values in both.
Arrays are NHWC, the kernels' layout; the rate pack is the UNscaled [11, N] fp32 pack.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import backward_refs as R
from iclr_17_compression_amd import codec, synth
from oracle import codec_ref as oracle

REL = R.REL                  # the project's per-element bar: a cost J against float64
GRAD_REL = R.GRAD_REL        # sums over pixels: the synthesis gains
METRIC_REL = 1e-5            # the project's bar for a bit total (test_gpu_ratectl.py)
# The share of a case's elements that may be near ties: elements with more than one candidate
# within 2·REL·max J of the least cost, where an fp32 evaluation may pick either. A CPU run with the
# oracle's latents (N = 128, indices 2/8/14, λ in 0.25/1/4/16) and a margin of 4e-5·bits found at
# most 6 of 6144; with this margin the shared cases have at most 14 of 6144 (0.23 %).
NEAR_TIE_CAP = 0.005

DELTAS = np.array([codec.step_size(s) for s in range(codec.STEPS)], dtype=np.float32)
LN2_F32 = np.float32(0.693147182464599609375)      # float(math.log(2)) as the kernels hold it

# ------------------------------------------------------------------------------- inputs
# test_gpu_ratectl.latent_cases' recipe: synth.trained_like_state_dict(N, 1), smooth images on one
# 64×96 canvas → y [2,4,6,N] (N = 128: 3072 elements per image, less than one 4096-element chunk;
# N = 192: 4608, two chunks, the second ragged), and a 1×1 image → y [1,1,1,N].
SIZES = [(49, 83), (64, 96)]
INDICES = (2, 8, 14)
LAMBDAS = (0.25, 1.0, 16.0)


def smooth(seed, H, W):
    return np.ascontiguousarray(synth.smooth_image_u8(seed, H, W).transpose(1, 2, 0))


def images():
    """The two images of the 64×96 canvas, then the 1×1 image."""
    return [smooth(60 + k, H, W) for k, (H, W) in enumerate(SIZES)] + [smooth(70, 1, 1)]


def padded(im, Hc, Wc):
    """The ingest contract: ToTensor's /255, the image top left, edges replicated (CPU)."""
    H, W = im.shape[:2]
    x = torch.from_numpy(im).permute(2, 0, 1).float().div(255)[None]
    return F.pad(x, (0, Wc - W, 0, Hc - H), mode="replicate")


def batch(imgs):
    """Images of one canvas as the codec ingests them: fp32 [B,3,Hc,Wc] (CPU)."""
    Hc, Wc = codec.canvas(*imgs[0].shape[:2])
    return torch.cat([padded(im, Hc, Wc) for im in imgs])


def weights(N, kind):
    """Channel weights g [N] fp32: "unit", or "ramp", a non-uniform set between ¼ and 2."""
    if kind == "unit":
        return np.ones(N, dtype=np.float32)
    return (0.25 + 1.75 * ((np.arange(N) * 7) % 16) / 15.0).astype(np.float32)


def lam_of(rdo, g):
    """lam[c] = λ·g_c as one fp32 product."""
    return (np.float32(rdo) * np.asarray(g, dtype=np.float32)).astype(np.float32)


def pack_of(p, N, prefix="bitEstimator."):
    """The UNscaled rate pack [11, N] fp32 of an oracle parameter dict (common.h's rows:
    softplus(h), b, tanh(a) per layer, then softplus(h4), b4), for tests without a GPU."""
    rows = []
    for f in ("f1", "f2", "f3"):
        rows += [F.softplus(p[f"{prefix}{f}.h"]), p[f"{prefix}{f}.b"], torch.tanh(p[f"{prefix}{f}.a"])]
    rows += [F.softplus(p[prefix + "f4.h"]), p[prefix + "f4.b"]]
    return torch.stack([r.detach().float().reshape(N) for r in rows]).numpy()


def oracle_latents(N):
    """(parameter dict, pack, [y [2,4,6,N], y [1,1,1,N]]) from oracle.analysis on the shared
    images: what the GPU tests' latents are up to the transforms' rounding."""
    p = oracle.state_dict_to_torch(synth.trained_like_state_dict(N, 1))
    ims = images()
    with torch.no_grad():
        ys = [oracle.analysis(batch(ims[:2]), p), oracle.analysis(batch(ims[2:]), p)]
    return p, pack_of(p, N), [y.permute(0, 2, 3, 1).contiguous().numpy() for y in ys]


# --------------------------------------------------------------------------- definition
def element_bits(v, pack, d, dtype=np.float32):
    """bits(v) on the step pack of d: v [..., N] integer-valued, pack [11, N] fp32, d an fp32
    step. Row 0 of the step pack is ONE fp32 product in either dtype."""
    d = np.float32(d)
    sp0 = (pack[0].astype(np.float32) * d).astype(np.float32).astype(dtype)
    p = pack.astype(dtype)
    half = dtype(0.5)

    def cdf(x):
        t = x * sp0 + p[1]
        x = t + np.tanh(t) * p[2]
        for k in (1, 2):
            t = x * p[3 * k] + p[3 * k + 1]
            x = t + np.tanh(t) * p[3 * k + 2]
        return dtype(1.0) / (dtype(1.0) + np.exp(-(x * p[9] + p[10])))

    v = np.asarray(v).astype(dtype)
    prob = cdf(v + half) - cdf(v - half)
    ln2 = LN2_F32 if dtype is np.float32 else dtype(math.log(2.0))
    bits = (dtype(-1.0) * np.log(prob + dtype(1e-10))) / ln2
    out = np.clip(bits, dtype(0.0), dtype(50.0))
    assert out.dtype == dtype
    return out


def quotient(y, d):
    """t = y/Δ, the IEEE fp32 quotient."""
    t = np.asarray(y, dtype=np.float32) / np.float32(d)
    assert t.dtype == np.float32
    return t


def candidates(t):
    """t fp32 → (values [3, ...] fp32, valid [3, ...] bool): r, r − sign(r), 0 in this order."""
    r = np.rint(t)
    vals = np.stack([r, r - np.sign(r), np.zeros_like(r)])
    valid = np.stack([np.ones(r.shape, bool), r != 0, np.abs(r) >= 2])
    return vals, valid


def costs(t, pack, d, lam, dtype=np.float32):
    """(values, valid, bits, J), each [3, ...]: the candidates of every element of t (fp32 NHWC),
    their bits and costs in ``dtype``. w = lam·Δ·Δ is the fp32 value in either dtype. Entries of
    an invalid candidate are computed like the others and mean nothing."""
    d = np.float32(d)
    vals, valid = candidates(t)
    w = ((np.asarray(lam, dtype=np.float32) * d) * d).astype(np.float32).astype(dtype)
    bits = np.stack([element_bits(v, pack, d, dtype) for v in vals])
    with np.errstate(invalid="ignore", over="ignore"):
        e = vals.astype(dtype) - t.astype(dtype)
        J = bits + w * (e * e)
    assert J.dtype == dtype
    return vals, valid, bits, J


def first_least(J, valid):
    """Index [...] of the first valid candidate of least J: a strict < moves the pick on."""
    idx = np.zeros(J.shape[1:], dtype=np.int64)
    best = J[0].copy()
    for k in (1, 2):
        with np.errstate(invalid="ignore"):
            move = valid[k] & (J[k] < best)
        idx[move] = k
        best[move] = J[k][move]
    return idx


def take(a, idx):
    return np.take_along_axis(a, idx[None], axis=0)[0]


def quantise(y, pack, d, lam, dtype=np.float32):
    """The definition on a latent y (fp32 NHWC) → {"t", "r", "y_hat", "y_deq" (fp32), "bits_el"
    (the pick's bits, ``dtype``), "idx" (the picked candidate's number)}."""
    t = quotient(y, d)
    vals, valid, bits, J = costs(t, pack, d, lam, dtype)
    idx = first_least(J, valid)
    y_hat = take(vals, idx)
    return {"t": t, "r": vals[0], "y_hat": y_hat, "y_deq": np.float32(d) * y_hat,
            "bits_el": take(bits, idx), "idx": idx}


def cheapest(t, pack, d, dtype=np.float32):
    """What lam = 0 picks: the first valid candidate of least bits."""
    vals, valid, bits, _ = costs(t, pack, d, np.zeros(pack.shape[1], np.float32), dtype)
    return take(vals, first_least(bits, valid))


def exact_tie(t):
    """t sits exactly between two integers (rint's own tie)."""
    return np.abs(t - np.rint(t)) == np.float32(0.5)


def judge(t, y_hat, pack, d, lam):
    """A quantiser's picks ``y_hat`` on ITS OWN t against the definition in float64 →
    {"margin", "excess" (J64(pick) − min J64, per element), "near_tie" (more than one candidate
    within the margin of the least cost), "argmin" (the float64 pick), "is_candidate"}. The margin
    is 2·REL·max over the candidates of J64: two costs enter a comparison, each held to REL."""
    vals, valid, _, J = costs(t, pack, d, lam, np.float64)
    Jv = np.where(valid, J, np.nan)
    lo, hi = np.nanmin(Jv, axis=0), np.nanmax(Jv, axis=0)
    margin = 2.0 * REL * hi
    within = valid & (J <= lo + margin)
    hit = valid & (vals == y_hat[None])
    # the candidates of an element are distinct values, so at most one matches
    picked = np.where(hit.any(axis=0), np.where(hit, J, 0.0).sum(axis=0), np.inf)
    return {"margin": margin, "excess": picked - lo, "near_tie": within.sum(axis=0) > 1,
            "argmin": take(vals, first_least(J, valid)), "is_candidate": hit.any(axis=0)}
