"""Record what ``kernels.deconv3_h3`` returns, for tests/test_gpu_chain.py.

Run on a GPU, at the commit whose wrapper is the record (the parent of the change that routed
``deconv3_h3`` through ``_deconv3_halo``):

    python tests/golden/gen_deconv3_h3.py [--out tests/golden/g10_deconv3_h3_n128.npz]

One B=1, 64×64, N=128 h3 chain of the trained-like model runs up to deconv2+IGDN2; its output
(deconv3's chunk-major h3 input) and conv3's bit partials are stored as the call's inputs, and
every non-None value ``deconv3_h3`` returns for them (x_ref = the image, want_recon) as
``<case>_<position>`` for the three ``bits`` cases, with ``<case>_len`` the tuple's length.
The weights are not stored: the test packs them from ``synth.trained_like_state_dict(128, 1)``.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from iclr_17_compression_amd import kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

N, SEED, IMAGE_SEED, SIZE = 128, 1, 5, 64
CASES = {"none": {}, "total": {"bits": True}, "per_image": {"bits": True, "bits_per_image": True}}


def model_and_image(device):
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v)
                         for k, v in synth.trained_like_state_dict(N, SEED).items()})
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(IMAGE_SEED, 1, SIZE, SIZE)))
    return net.to(device).eval(), x.to(device)


def inputs(device):
    """(net, x, deconv3's h3 input, conv3's bit partials) of the recorded chain."""
    net, x = model_and_image(device)
    enc, dec = net.Encoder, net.Decoder
    kernels.h3_chain_begin(device)
    w2h, w3h = enc.packed_h3()
    hs, _ = kernels.conv1_gdn_h3(x, enc.packed_conv1_h3(), enc.conv1.bias,
                                 *enc.gdn1.effective_params_h3(), N)
    hs, _, _ = kernels.conv2_gdn_h3(hs, w2h, enc.conv2.bias, *enc.gdn2.effective_params_h3())
    _, bp, _, yh = kernels.conv3_quant_rate_h3(hs, w3h, net.bitEstimator.packed(),
                                               rtab=net.bitEstimator.rate_table())
    d1, d2, _ = dec.packed_h3k()
    hs, _, _ = kernels.deconv_igdn_h3(yh, d1, dec.deconv1.bias, *dec.igdn1.effective_params_h3(),
                                      int_in=True)
    hs, _, _ = kernels.deconv_igdn_h3(hs, d2, dec.deconv2.bias, *dec.igdn2.effective_params_h3(),
                                      chunk_major=True)
    return net, x, hs, bp


def run_case(net, x, hs, bp, case):
    """``deconv3_h3`` on the stored inputs for one of CASES (a fresh chain: the flag is clear)."""
    kw = dict(CASES[case])
    if kw.pop("bits", False):
        kw["bits"] = (bp, 1.0 / (x.shape[0] * SIZE * SIZE))
    kernels.h3_chain_begin(x.device)
    return kernels.deconv3_h3(hs, net.Decoder.packed_h3k()[2], net.Decoder.deconv3.bias, x_ref=x,
                              want_recon=True, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "g10_deconv3_h3_n128.npz"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with torch.no_grad():
        net, x, hs, bp = inputs(dev)
        arrays = {"hs": hs.cpu().numpy(), "bits_partial": bp.cpu().numpy()}
        for case in CASES:
            out = run_case(net, x, hs, bp, case)
            arrays[f"{case}_len"] = np.int64(len(out))
            for i, t in enumerate(out):
                if t is not None:
                    arrays[f"{case}_{i}"] = t.cpu().numpy()
    assert all(np.isfinite(v).all() for k, v in arrays.items() if k != "hs")
    np.savez_compressed(args.out, **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes", sorted(arrays))


if __name__ == "__main__":
    main()
