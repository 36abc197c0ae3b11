"""Record the SHA-256 of every forward output and every gradient of a training step, and the
ordered entry points it launches, in each precision mode, for tests/test_gpu_train_digests.py.

Run on a GPU, with the tree and the library of the commit that is the record (the parent of the
change that moved the training chain into chain.py and wrote each backward once):

    python tests/golden/gen_train_step_digests.py --commit <that commit's hash>

Only the public surface is used (ImageCompressor, forward_train, net(x, noise), net.Encoder(x),
net.Decoder(y), kernels.set_precision), so the same file runs on the recorded tree and on any later
one. Inputs come from ``synth`` (trained-like weights at seed 1, synthetic image, fixed noise):
B = 2, image 64 × 96, N = 128 and 192, so the layer grids are 16×24, 8×12 and 4×6: partial 8×8
engine tiles, a partial second halo block, unequal H and W. Per (mode, N) six cases reach every
branch of CodecTrainFn.backward and the two stand-alone Functions (``CASES``), each on a fresh net
with x.requires_grad.

Every case runs two consecutive steps on its net. Between them every parameter gets
``p.mul_(1.0)``: the values stay, the version counters move, so the second step repacks as a real
training step does. The second step's digests must equal the first's; its launches (the names
passed to ``kernels.call``) are the recorded sequence. The training kernels use no floating-point
atomics, so everything is expected to be bit-reproducible: the whole set runs twice and no fixture
is written if the two differ. The fixture holds digests, shapes and names only.

The recorded tree raised in the eight ``codec.ytilde`` cases: CodecTrainFn.backward unpacked four
values where synthesis_backward returned three (want_split=False). Those cases alone were
recorded with that unpack padded with None, a host-only change under which the other forty cases
were recorded again, bit for bit and launch for launch the same (the fixture's ``note``).
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

from iclr_17_compression_amd import _lib, kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

B, H, W = 2, 64, 96
CHANNELS = (128, 192)
MODES = ("h3", "x6", "fp32", "bf16")
CASES = ("codec.mse", "codec.clipped", "codec.ytilde", "codec.bpp", "encoder", "decoder")
SEED, IMAGE_SEED, NOISE_SEED, R_SEED, R2_SEED = 1, 5, 7, 13, 17
LAM = 0.01 * 255.0 ** 2
FIXTURE = os.path.join(HERE, "g13_train_step_digests.json")


def _digest(t):
    if t is None:
        return "None"
    a = t.detach().contiguous().cpu().numpy()
    return (f"{a.dtype} {'x'.join(map(str, a.shape)) or 'scalar'} "
            f"{hashlib.sha256(a.tobytes()).hexdigest()}")


def _step(net, case, x, noise, R, R2):
    """One forward + backward of ``case`` → {name: digest} of its outputs and gradients."""
    net.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    modules, inp = [net], x
    if case == "codec.mse":
        clipped, mse, bpp = net.forward_train(x, noise)
        outs = {"clipped": clipped, "mse": mse, "bpp": bpp}
        loss = LAM * mse + bpp
    elif case.startswith("codec."):
        clipped, y_tilde, bpp = net(x, noise)
        outs = {"clipped": clipped, "y_tilde": y_tilde, "bpp": bpp}
        loss = {"codec.clipped": lambda: (clipped * R).sum() + bpp,   # g_clipped only
                "codec.ytilde": lambda: (y_tilde * R2).sum() + bpp,   # g_ytilde: no split handed on
                "codec.bpp": lambda: bpp}[case]()                     # zero g_recon
    elif case == "encoder":
        modules = [net.Encoder]
        y = net.Encoder(x)
        outs = {"y": y}
        loss = (y * R2).sum()
    else:
        modules = [net.Decoder]
        with torch.no_grad():
            y_hat = torch.round(net.Encoder(x))
        inp = y_hat.requires_grad_()
        recon = net.Decoder(inp)
        outs = {"y_hat": y_hat, "recon": recon}
        loss = (recon * R).sum()
    loss.backward()
    torch.cuda.synchronize(x.device)
    out = {f"out.{k}": _digest(v) for k, v in outs.items()}
    out["grad.input"] = _digest(inp.grad)
    for m in modules:
        for n, p in m.named_parameters():
            out[f"grad.{n}"] = _digest(p.grad)
    return out


def run_case(device, mode, N, case, state, x, noise, R, R2):
    """Two steps of ``case`` on a fresh net → ({name: digest}, [entry points of the second])."""
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict(state)
    net = net.to(device).train()
    first = _step(net, case, x, noise, R, R2)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.0)
    launches, real = [], kernels.call

    def recording(name, *args):
        launches.append(name)
        return real(name, *args)

    kernels.call = recording
    try:
        second = _step(net, case, x, noise, R, R2)
    finally:
        kernels.call = real
    differing = sorted(k for k in first if first[k] != second.get(k))
    if differing or set(first) != set(second):
        raise AssertionError(f"{mode}/N{N}/{case}: the second step differs from the first in "
                             f"{differing}")
    return first, launches


def digests(device):
    """Every case → ({case: {name: digest}}, {case: [entry points]})."""
    out, seqs = {}, {}
    old = kernels.precision()
    try:
        for N in CHANNELS:
            state = {k: torch.from_numpy(v)
                     for k, v in synth.trained_like_state_dict(N, SEED).items()}
            x = torch.from_numpy(synth.to_unit_float(synth.image_u8(IMAGE_SEED, B, H, W))).to(device)
            shape = (B, N, H // 16, W // 16)
            noise = torch.from_numpy(synth.uniform(NOISE_SEED, shape, -0.5, 0.5)).to(device)
            R = torch.from_numpy(synth.uniform(R_SEED, (B, 3, H, W), -1.0, 1.0)).to(device)
            R2 = torch.from_numpy(synth.uniform(R2_SEED, shape, -1.0, 1.0)).to(device)
            for mode in MODES:
                kernels.set_precision(mode)
                for case in CASES:
                    key = f"{mode}/N{N}/{case}"
                    out[key], seqs[key] = run_case(device, mode, N, case, state, x, noise, R, R2)
    finally:
        kernels.set_precision(old)
    return out, seqs


def write_fixture(path, commit, cases, launches, note=""):
    """One line per case, so that a changed digest shows as one changed line."""
    with open(_lib.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()
    head = {"B": B, "H": H, "W": W, "channels": list(CHANNELS), "modes": list(MODES),
            "cases": list(CASES), "parent_commit": commit, "library_sha256": lib_hash,
            "note": note}
    lines = lambda d: ",\n".join(f"{json.dumps(k)}: {json.dumps(d[k])}" for k in sorted(d))  # noqa: E731
    with open(path, "w") as f:
        f.write("{" + json.dumps(head)[1:-1] + ', "digests": {\n' + lines(cases))
        f.write('\n}, "launches": {\n' + lines(launches) + "\n}}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the hash of the commit whose tree this runs")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--note", default="", help="stored in the file: how the tree differed, if it did")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    (first, seq1), (second, seq2) = digests(dev), digests(dev)
    differing = sorted(key for key in first if first[key] != second.get(key))
    if differing or set(first) != set(second) or seq1 != seq2:
        print("NOT REPRODUCIBLE, no fixture written:", differing,
              sorted(k for k in seq1 if seq1[k] != seq2.get(k)))
        sys.exit(1)
    write_fixture(args.out, args.commit, first, seq1, args.note)
    print("wrote", args.out, os.path.getsize(args.out), "bytes,", len(first), "cases,",
          sum(len(v) for v in first.values()), "tensors,", sum(len(v) for v in seq1.values()),
          "launches")


if __name__ == "__main__":
    main()
