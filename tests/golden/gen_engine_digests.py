"""Record the SHA-256 of every output buffer of the 8×8-tile engine's entry points, the halo
deconv3 entry points and the stand-alone GDN, for tests/test_gpu_engine_digests.py.

Run on a GPU, against the library of the commit that is the record (the parent of the change that
split csrc/engine_fp32.hip by kernel family and rewrote its host launch layer):

    ICLR17_LIB=/path/to/parent/libiclr17.so python tests/golden/gen_engine_digests.py

Inputs come from ``synth`` (trained-like weights, synthetic image): B = 2, N = 128 and 192, image
64 × 96, so the layer grids are 16×24, 8×12 and 4×6: partial 8×8 engine tiles, a partial second
16×16 halo block, unequal H and W. Activations and gradients are chained from the kernels' own
outputs. These kernels use no floating-point atomics, so every output is expected to be
bit-reproducible: every case runs twice and no fixture is written if a digest differs between the
two runs. The fixture holds digests and shapes only.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from iclr_17_compression_amd import kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

B, H, W = 2, 64, 96
CHANNELS = (128, 192)
SEED, IMAGE_SEED, NOISE_SEED = 1, 5, 7
FIXTURE = os.path.join(HERE, "g11_engine_digests.json")


def _record(out, name, values):
    """Digest every tensor of ``values`` (a tensor or a tuple with Nones): out[name][position] =
    "<dtype> <shape> <sha256>"."""
    if isinstance(values, torch.Tensor):
        values = (values,)
    assert name not in out, name
    out[name] = {}
    for i, t in enumerate(values):
        if t is None:
            continue
        a = t.detach().contiguous().cpu().numpy()
        out[name][str(i)] = (f"{a.dtype} {'x'.join(map(str, a.shape)) or 'scalar'} "
                             f"{hashlib.sha256(a.tobytes()).hexdigest()}")
    return values


def run(device, N):
    """Every case at channel count N → {case: {position: "dtype shape sha256"}}."""
    out = {}

    def rec(name, values):
        return _record(out, f"N{N}/{name}", values)

    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v)
                         for k, v in synth.trained_like_state_dict(N, SEED).items()})
    net = net.to(device).eval()
    enc, dec, k = net.Encoder, net.Decoder, kernels
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(IMAGE_SEED, B, H, W))).to(device)
    noise = torch.from_numpy(np.random.RandomState(NOISE_SEED).uniform(
        -0.5, 0.5, (B, N, H // 16, W // 16)).astype(np.float32)).to(device)
    rate, rtab = net.bitEstimator.packed(), net.bitEstimator.rate_table()
    w1, w2, w3, g1, g2 = enc.packed()
    d1, d2, d3, ig1, ig2 = dec.packed()
    g1x, g2x = enc.gdn1.effective_params_x6(), enc.gdn2.effective_params_x6()
    ig1x, ig2x = dec.igdn1.effective_params_x6(), dec.igdn2.effective_params_x6()
    b1, b2 = enc.conv1.bias, enc.conv2.bias
    e1, e2, e3 = dec.deconv1.bias, dec.deconv2.bias, dec.deconv3.bias

    # ---------------------------------------------------------------- fp32 forward layers
    h1, u1 = rec("conv1_gdn", k.conv1_gdn(x, w1, b1, *g1, N, want_pre=True))
    rec("conv1_gdn.nopre", k.conv1_gdn(x, w1, b1, *g1, N))
    h2, u2 = rec("conv2_gdn", k.conv2_gdn(h1, w2, b2, *g2, want_pre=True))
    rec("conv3", k.conv3(h2, w3))
    yh, bp, _ = rec("conv3_quant_rate.round", k.conv3_quant_rate(h2, w3, rate, want_y=True))
    rec("conv3_quant_rate.round_rtab", k.conv3_quant_rate(h2, w3, rate, rtab=rtab))
    yt, _, _ = rec("conv3_quant_rate.noise", k.conv3_quant_rate(h2, w3, rate, noise=noise,
                                                               want_y=True))
    v1, p1 = rec("deconv1_igdn", k.deconv_igdn(yh, d1, e1, *ig1, want_pre=True))
    v2, p2 = rec("deconv2_igdn", k.deconv_igdn(v1, d2, e2, *ig2, want_pre=True))
    rec("deconv2_igdn.nopre", k.deconv_igdn(v1, d2, e2, *ig2))
    rec("deconv3.plain", k.deconv3(v2, d3, e3))
    clipped, recon, _ = rec("deconv3.sse", k.deconv3(v2, d3, e3, x_ref=x, want_recon=True))
    rec("deconv3.sse_unclipped", k.deconv3(v2, d3, e3, x_ref=x, want_recon=True,
                                           sse_unclipped=True))
    rec("deconv3.sse_norecon", k.deconv3(v2, d3, e3, x_ref=x))

    # ------------------------------------------------------------------- x6 forward layers
    rec("split_planes", k.split_planes(h1))
    w3s = rec("split_packed", k.split_packed(w3, 25, N, N))[0]
    w1x = enc.packed_conv1_x6()
    rec("conv1_gdn_x6.gamma_fp32", k.conv1_gdn_x6(x, w1, b1, *g1, N, want_f32=True, want_pre=True))
    rec("conv1_gdn_x6.gamma_split", k.conv1_gdn_x6(x, w1, b1, *g1, N, want_f32=True,
                                                   want_pre=True, g6=g1x[2]))
    hs1, _, _ = rec("conv1x6_gdn", k.conv1x6_gdn(x, w1x, b1, g1x[0], g1x[2], N, want_f32=True,
                                                 want_pre=True))
    rec("conv1x6_gdn.split_only", k.conv1x6_gdn(x, w1x, b1, g1x[0], g1x[2], N))
    hs2, _, _ = rec("conv2_gdn_x6", k.conv2_gdn_x6(hs1, w2, b2, *g2x, want_f32=True, want_pre=True))
    for wname, ws in (("", None), ("w", w3s)):
        rec(f"conv3_quant_rate_x6{wname}.round",
            k.conv3_quant_rate_x6(hs2, w3, rate, want_y=True, w_split=ws))
        rec(f"conv3_quant_rate_x6{wname}.round_rtab",
            k.conv3_quant_rate_x6(hs2, w3, rate, rtab=rtab, w_split=ws))
        rec(f"conv3_quant_rate_x6{wname}.noise",
            k.conv3_quant_rate_x6(hs2, w3, rate, noise=noise, want_y=True, w_split=ws))
    _, bpx, _, yhs = k.conv3_quant_rate_x6(hs2, w3, rate, rtab=rtab, w_split=w3s)
    vs1, _, _ = rec("deconv1_igdn_x6", k.deconv_igdn_x6(yhs, d1, e1, *ig1x, want_f32=True,
                                                        want_pre=True))
    vs2, _, _ = rec("deconv2_igdn_x6", k.deconv_igdn_x6(vs1, d2, e2, *ig2x, want_f32=True,
                                                        want_pre=True))
    vs2c, _, _ = rec("deconv2_igdn_x6_cm", k.deconv_igdn_x6(vs1, d2, e2, *ig2x, chunk_major=True))
    rec("deconv2_igdn_x6.f32_only", k.deconv_igdn_x6(vs1, d2, e2, *ig2x, want_split=False,
                                                     want_f32=True))

    # ----------------------------------------------------------------- halo deconv3 kernels
    scale = 1.0 / (B * H * W)
    halo_cases = {
        "plain": {},
        "sse": {"x_ref": x, "want_recon": True},
        "sse_unclipped": {"x_ref": x, "want_recon": True, "sse_unclipped": True},
        "sse_norecon": {"x_ref": x},
        "recon": {"want_recon": True},
    }
    d3x = dec.packed_x6()
    for name, kw in halo_cases.items():
        rec(f"deconv3_x6.{name}", k.deconv3_x6(vs2, d3x, e3, **kw))
        rec(f"deconv3_x6_cm.{name}", k.deconv3_x6(vs2c, d3x, e3, **kw))
        rec(f"deconv3_x6_cm_bits.{name}", k.deconv3_x6(vs2c, d3x, e3, bits=(bpx, scale), **kw))
    d3b = dec.packed_bf16()[2]
    vb2 = k.to_bf16(v2)
    for name, kw in halo_cases.items():
        rec(f"deconv3_bf16.{name}", k.deconv3_bf16(vb2, d3b, e3, **kw))
        rec(f"deconv3_bf16_bits.{name}", k.deconv3_bf16(vb2, d3b, e3, bits=(bp, scale), **kw))
    # the h3 chain up to deconv2 (csrc/engine_h3.hip) makes deconv3_h3's input
    k.h3_chain_begin(device)
    w2h, w3h = enc.packed_h3()
    t, _ = k.conv1_gdn_h3(x, enc.packed_conv1_h3(), b1, *enc.gdn1.effective_params_h3(), N)
    t, _, _ = k.conv2_gdn_h3(t, w2h, b2, *enc.gdn2.effective_params_h3())
    _, bph, _, t = k.conv3_quant_rate_h3(t, w3h, rate, rtab=rtab)
    d1h, d2h, d3h = dec.packed_h3k()
    t, _, _ = k.deconv_igdn_h3(t, d1h, e1, *dec.igdn1.effective_params_h3(), int_in=True)
    vh2, _, _ = k.deconv_igdn_h3(t, d2h, e2, *dec.igdn2.effective_params_h3(), chunk_major=True)
    for name, kw in halo_cases.items():
        rec(f"deconv3_h3.{name}", k.deconv3_h3(vh2, d3h, e3, **kw))
        rec(f"deconv3_h3.{name}.bits", k.deconv3_h3(vh2, d3h, e3, bits=(bph, scale), **kw))
        rec(f"deconv3_h3.{name}.bits_per_image",
            k.deconv3_h3(vh2, d3h, e3, bits=(bph, scale), bits_per_image=True, **kw))

    # ------------------------------------------------------------ fused backward entry points
    # gradients chained from ∂(clipped − x): fp32 kernels first, then the x6 ones in both
    # gradient forms (fp32 + split, split only)
    g_recon = (recon - x).contiguous()
    g_bpp = torch.tensor(0.25, device=device)
    count = float(B * H * W)
    i2, i1 = dec.igdn2.effective_params_bwd(), dec.igdn1.effective_params_bwd()
    n2, n1 = enc.gdn2.effective_params_bwd(), enc.gdn1.effective_params_bwd()
    i2x, i1x = dec.igdn2.effective_params_bwd_x6(), dec.igdn1.effective_params_bwd_x6()
    n2x, n1x = enc.gdn2.effective_params_bwd_x6(), enc.gdn1.effective_params_bwd_x6()
    d3c, d2c, d1c = dec.packed_bwd(False)
    d3cx = dec.packed_bwd(True)[0]
    w3t, w2t = enc.packed_bwd()

    gv2 = rec("bwd_deconv3_igdn.fp32", k.bwd_deconv3_igdn(g_recon, d3c, p2, *i2))[0]
    gv1 = rec("bwd_deconv_igdn.fp32", k.bwd_deconv_igdn(gv2, d2c, p1, *i1))[0]
    gy = rec("bwd_deconv_rate.fp32", k.bwd_deconv_rate(gv1, d1c, yt, rate, g_bpp, count,
                                                       H // 16, W // 16))[0]
    rec("bwd_deconv_rate.fp32_norate", k.bwd_deconv_rate(gv1, d1c, None, None, None, count,
                                                         H // 16, W // 16))
    gu2 = rec("bwd_conv3_gdn.fp32", k.bwd_conv_gdn(gy, w3t, u2, *n2))[0]
    rec("bwd_conv2_gdn.fp32", k.bwd_conv_gdn(gu2, w2t, u1, *n1))

    for form, f32 in (("both", True), ("split", False)):
        kw = {"want_split": True, "want_f32": f32}
        r = rec(f"bwd_deconv3_igdn.x6_{form}",
                k.bwd_deconv3_igdn(g_recon, None, p2, *i2x[:3], w_split=d3cx, g6=i2x[3],
                                   g6t=i2x[4], **kw))
        rec(f"bwd_deconv3_igdn.x6gamma_{form}",   # fp32 contraction, x6 γ contractions
            k.bwd_deconv3_igdn(g_recon, d3c, p2, *i2x[:3], g6=i2x[3], g6t=i2x[4], **kw))
        r = rec(f"bwd_deconv_igdn.x6_{form}",
                k.bwd_deconv_igdn(None, d2c, p1, *i1x[:3], g_split=r[4], g6=i1x[3], g6t=i1x[4],
                                  **kw))
        gs1 = r[4]
        ry = rec(f"bwd_deconv_rate.x6_{form}",
                 k.bwd_deconv_rate(None, d1c, yt, rate, g_bpp, count, H // 16, W // 16,
                                   g_split=gs1, want_split=True))
        r = rec(f"bwd_conv3_gdn.x6_{form}",
                k.bwd_conv_gdn(None, w3t, u2, *n2x[:3], g_split=ry[2], g6=n2x[3], g6t=n2x[4], **kw))
        rec(f"bwd_conv2_gdn.x6_{form}",
            k.bwd_conv_gdn(None, w2t, u1, *n1x[:3], g_split=r[4], g6=n1x[3], g6t=n1x[4], **kw))
    rec("bwd_deconv_rate.x6_norate", k.bwd_deconv_rate(None, d1c, None, None, None, count,
                                                       H // 16, W // 16, g_split=gs1))
    rec("bwd_deconv_igdn.fp32_in_x6gamma",
        k.bwd_deconv_igdn(gv2, d2c, p1, *i1x[:3], g6=i1x[3], g6t=i1x[4], want_split=True))

    # --------------------------------------------------------------- stand-alone GDN / IGDN
    xn = u2.permute(0, 3, 1, 2)                      # [B, N, 8, 12] channels-last view
    gn = (h2 - 0.5 * u2).permute(0, 3, 1, 2)
    for lay, xx, gg in (("nhwc", xn, gn), ("nchw", xn.contiguous(), gn.contiguous())):
        for inv, (be, gp, gpt) in ((False, n2), (True, i1)):
            tag = f"{'igdn' if inv else 'gdn'}.{lay}"
            rec(f"gdn.{tag}", k.gdn(xx, be, gp, inv))
            rec(f"gdn_bwd.{tag}", k.gdn_backward(xx, gg, be, gp, gpt, inv))
    torch.cuda.synchronize(device)
    return out


def digests(device):
    out = {}
    with torch.no_grad():
        for N in CHANNELS:
            out.update(run(device, N))
    return out


def write_fixture(path, cases):
    """One line per case, so that a changed digest shows as one changed line."""
    head = {"B": B, "H": H, "W": W, "channels": list(CHANNELS)}
    with open(path, "w") as f:
        f.write("{" + json.dumps(head)[1:-1] + ', "digests": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(cases[k])}" for k in sorted(cases)))
        f.write("\n}}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    first, second = digests(dev), digests(dev)
    differing = sorted(key for key in first if first[key] != second.get(key))
    if differing or set(first) != set(second):
        print("NOT REPRODUCIBLE, no fixture written:", differing)
        sys.exit(1)
    write_fixture(args.out, first)
    print("wrote", args.out, os.path.getsize(args.out), "bytes,", len(first), "cases,",
          sum(len(v) for v in first.values()), "buffers")


if __name__ == "__main__":
    main()
