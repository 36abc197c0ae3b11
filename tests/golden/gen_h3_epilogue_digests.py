"""Record the SHA-256 of every output buffer of the h3 engine's GDN / IGDN layers (conv1 + GDN1,
conv2 + GDN2, deconv + IGDN: csrc/engine_h3.hip, h3k_body's epilogue), for
tests/test_gpu_h3_epilogue.py.

Run on a GPU, against the library of the commit that is the record (the parent of the change that
made the epilogue's channel contraction one pass over the k-blocks):

    ICLR17_LIB=/path/to/parent/libiclr17.so python tests/golden/gen_h3_epilogue_digests.py

The cases, for N = 128 and 192, inputs from ``synth`` (trained-like weights, seed 1):
  conv1            image 2 × 3 × 80 × 112: output 20 × 28, ragged 16 × 16 tiles in both directions
  conv2.rows8      B = 3, input 40 × 56: 8-row tiles, ragged
  conv2.rows16     B = 64, input 64 × 64: 16-row tiles
  deconv.rows8.*   B = 3, latents 5 × 7: 8-row tiles, ragged
  deconv.rows16.*  B = 64, latents 16 × 16: 16-row tiles
                   (* = integer input with int_in or real input without, NHWC-16 or chunk-major-32
                   h3 output)
  conv1.zero       a zero image under a zero bias: every pixel all zeros (s_p = 1)
  conv1.tiny       the same with bias[5] = 1e-20: the pixels' largest x² is far below 2^-86
                   (s_p clamped at 2^100)
every one with the fp32, h3, x6 and pre-activation outputs. The kernels use no floating-point
atomics, so every output is bit-reproducible: every case runs twice and no fixture is written if a
digest differs between the two runs. The fixture holds digests and shapes only.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from iclr_17_compression_amd import kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

CHANNELS = (128, 192)
GROUPS = ("conv1", "conv2", "deconv")
SEED = 1
FIXTURE = os.path.join(HERE, "g12_h3_epilogue_digests.json")


def _digest(t):
    a = t.detach().contiguous().cpu().numpy()
    return f"{a.dtype} {'x'.join(map(str, a.shape))} {hashlib.sha256(a.tobytes()).hexdigest()}"


def _net(N, device):
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v)
                         for k, v in synth.trained_like_state_dict(N, SEED).items()})
    return net.to(device).eval()


def cases(device, N, group):
    """name → thunk returning the case's output tuple (h3, fp32, x6, pre)."""
    net = _net(N, device)
    enc, dec, k = net.Encoder, net.Decoder, kernels
    all_out = dict(want_f32=True, want_x6=True, want_pre=True)
    out = {}
    if group == "conv1":
        w1, g1 = enc.packed_conv1_h3(), enc.gdn1.effective_params_h3()
        x = torch.from_numpy(synth.to_unit_float(synth.image_u8(7, 2, 80, 112))).to(device)
        out["conv1"] = lambda: k.conv1_gdn_h3(x, w1, enc.conv1.bias, *g1, N, **all_out)
        zero = torch.zeros(1, 3, 64, 64, device=device)
        b0 = torch.zeros(N, device=device)
        b1 = b0.clone()
        b1[5] = 1e-20
        out["conv1.zero"] = lambda: k.conv1_gdn_h3(zero, w1, b0, *g1, N, **all_out)
        out["conv1.tiny"] = lambda: k.conv1_gdn_h3(zero, w1, b1, *g1, N, **all_out)
    elif group == "conv2":
        w2, g2 = enc.packed_h3()[0], enc.gdn2.effective_params_h3()
        for name, seed, (B, h, w) in (("rows8", 21, (3, 40, 56)), ("rows16", 33, (64, 64, 64))):
            a = k.h3_planes(torch.from_numpy(synth.normal_like(seed, (B, h, w, N), 0.7)).to(device),
                            cm=k.CONV_CM)
            out[f"conv2.{name}"] = (lambda a=a: k.conv2_gdn_h3(a, w2, enc.conv2.bias, *g2, **all_out))
    elif group == "deconv":
        wd, gd = dec.packed_h3k()[0], dec.igdn1.effective_params_h3()
        for name, (B, h, w) in (("rows8", (3, 5, 7)), ("rows16", (64, 16, 16))):
            real = torch.from_numpy(synth.normal_like(24, (B, h, w, N), 0.7))
            ints = torch.round(torch.from_numpy(synth.uniform(25, (B, h, w, N), -6, 6)))
            for int_in in (False, True):
                a = k.h3_planes((ints if int_in else real).to(device), cm=k.DECONV_CM)
                for cm in (False, True):
                    out[f"deconv.{name}.{'int' if int_in else 'real'}.{'cm32' if cm else 'cm16'}"] = (
                        lambda a=a, int_in=int_in, cm=cm: k.deconv_igdn_h3(
                            a, wd, dec.deconv1.bias, *gd, chunk_major=cm, int_in=int_in, **all_out))
    else:
        raise ValueError(group)
    return out


def digests(device, N, group):
    """{"N<N>/<case>": {position: "dtype shape sha256"}} for one channel count and case group."""
    got = {}
    with torch.no_grad():
        for name, thunk in cases(device, N, group).items():
            kernels.h3_chain_begin(device)
            values = thunk()
            assert all(v is not None for v in values) and len(values) == 4, name
            got[f"N{N}/{name}"] = {str(i): _digest(v) for i, v in enumerate(values)}
            assert int(kernels.h3_range_flag(device).item()) == 0, name
    return got


def all_digests(device):
    out = {}
    for N in CHANNELS:
        for group in GROUPS:
            out.update(digests(device, N, group))
    return out


def write_fixture(path, record):
    """One line per case, so that a changed digest shows as one changed line."""
    with open(path, "w") as f:
        f.write('{"channels": ' + json.dumps(list(CHANNELS)) + ', "digests": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(record[k])}" for k in sorted(record)))
        f.write("\n}}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    first, second = all_digests(dev), all_digests(dev)
    differing = sorted(key for key in first if first[key] != second.get(key))
    if differing or set(first) != set(second):
        print("NOT REPRODUCIBLE, no fixture written:", differing)
        sys.exit(1)
    write_fixture(args.out, first)
    print("wrote", args.out, os.path.getsize(args.out), "bytes,", len(first), "cases,",
          sum(len(v) for v in first.values()), "buffers")


if __name__ == "__main__":
    main()
