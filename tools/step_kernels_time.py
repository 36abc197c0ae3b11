"""Cost and output hashes of the step-ladder kernels (csrc/ladder.h and the units on it:
ratectl.hip, stepmap.hip, rdoq.hip, quality.hip, steptrain.hip's forward) on the GPU, in one
process, warm: every arm once per round with the order rotating, HIP events around the entry point
on preallocated buffers (no host checks, no status read; a sweep's bracket includes its
reduce_partials). Made to compare two builds of libiclr17.so, selected per process with ICLR17_LIB
(diagnostic; needs a GPU). N = 192, y [64,16,16,192] (64 images of 256×256).

One JSON line per arm: the median, p10 and p90 in µs and the sha256 (16 hex digits) of every output
the arm writes.

    ICLR17_LIB=… python tools/step_kernels_time.py [--rounds 25] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from iclr_17_compression_amd import _lib, codec, kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=25)
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
N = 192
DELTAS = [codec.step_size(s) for s in range(codec.STEPS)]


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()[:16]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


net = ImageCompressor(out_channel_N=N)
net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
net = net.to(dev).eval()
p, call = kernels._p, _lib.call

with torch.no_grad():
    x = torch.stack([torch.from_numpy(synth.smooth_image_u8(300 + k, 256, 256)).float().div(255)
                     for k in range(64)]).to(dev)
    y = net.latents(x).contiguous()
    B, h, w, _ = y.shape
    n = y.numel()
    st = kernels._stream(y)
    pack = net.bitEstimator.packed()
    lam = net.synthesis_gains().contiguous()
    rng = np.random.default_rng(7)
    steps_dev = torch.tensor([DELTAS[s] for s in rng.integers(0, 32, B)], device=dev)
    noise = (torch.rand(B, N, h, w, device=dev, generator=torch.Generator(dev).manual_seed(3))
             - 0.5).contiguous()
    mh, mw = kernels.map_shape(h, w, 2)
    board = (np.add.outer(np.arange(mh), np.arange(mw)) % 2).astype(np.uint8)   # checkerboard
    idx2 = torch.from_numpy(np.broadcast_to(10 + 4 * board, (B, mh, mw)).copy()).to(dev)
    idx32 = torch.from_numpy(rng.permutation(B * mh * mw).reshape(B, mh, mw).astype(np.uint8)
                             % 32).to(dev)
    off = torch.from_numpy((3 * np.broadcast_to(board, (B, mh, mw)).astype(np.int8) - 1).copy()
                           ).to(dev)
    ladder = ctypes.cast((ctypes.c_float * 32)(*DELTAS), ctypes.c_void_p)
    d12 = ctypes.c_float(DELTAS[12])

    y_hat, y_deq = torch.empty_like(y), torch.empty_like(y)
    r12 = kernels.quantise_step(y, DELTAS[12])[0]
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    T = _lib.query("iclr17_rate_sweep_partials", h, w, N)
    partial = torch.empty(B * 32 * T, device=dev, dtype=torch.float64)
    table = torch.empty(B, 32, device=dev, dtype=torch.float64)
    bits = torch.empty(B, device=dev, dtype=torch.float64)

    def rdo(s):
        return lambda: call("iclr17_quantise_rdo", p(y), B, h, w, N, p(pack),
                            ctypes.c_float(DELTAS[s]), p(lam), p(y_hat), p(y_deq), p(partial),
                            p(bits), p(status), st)

    def step_map(idx):
        return lambda: call("iclr17_quantise_step_map", p(y), B, h, w, N, p(idx), 1, ladder,
                            p(y_hat), p(y_deq), p(status), st)

    pair, deq, sweep = (y_hat, y_deq), (y_deq,), (table,)
    arms = {   # name: (call, the tensors it writes)
        "quantise_step": (lambda: call("iclr17_quantise_step", p(y), n, d12, p(y_hat), p(y_deq),
                                       p(status), st), pair),
        "quantise_steps": (lambda: call("iclr17_quantise_steps", p(y), B, n // B, p(steps_dev),
                                        p(y_hat), p(y_deq), p(status), st), pair),
        "quantise_step_map 2 steps": (step_map(idx2), pair),
        "quantise_step_map 32 steps": (step_map(idx32), pair),
        "dequantise_step": (lambda: call("iclr17_dequantise_step", p(r12), n, d12, p(y_deq), st),
                            deq),
        "dequantise_step_map 32 steps": (
            lambda: call("iclr17_dequantise_step_map", p(r12), B, h, w, N, p(idx32), 1, ladder,
                         p(y_deq), st), deq),
        "quantise_rdo index 4": (rdo(4), pair + (bits,)),
        "quantise_rdo index 12": (rdo(12), pair + (bits,)),
        "rate_sweep": (lambda: call("iclr17_rate_sweep", p(y), B, h, w, N, p(pack), ladder, 32,
                                    p(partial), p(table), st), sweep),
        "rate_sweep_offsets": (lambda: call("iclr17_rate_sweep_offsets", p(y), B, h, w, N, p(pack),
                                            ladder, p(off), 1, p(partial), p(table), st), sweep),
        "rate_sweep_rdo": (lambda: call("iclr17_rate_sweep_rdo", p(y), B, h, w, N, p(pack), ladder,
                                        32, p(lam), p(partial), p(table), st), sweep),
        "distortion_sweep": (lambda: call("iclr17_distortion_sweep", p(y), B, h, w, N, p(lam),
                                          ladder, 32, p(partial), p(table), st), sweep),
        "step_noise_rate": (lambda: call("iclr17_step_noise_rate", p(y), p(noise), B, h, w, N,
                                         p(steps_dev), p(pack), p(y_hat), p(y_deq), p(partial),
                                         st), pair),
    }
    shas = {}
    for name, (fn, outs) in arms.items():   # warm, and the outputs' hashes
        fn()
        torch.cuda.synchronize()
        extra = (partial[:B * T],) if name == "step_noise_rate" else ()
        shas[name] = sha(*outs, *extra)
    assert int(status.item()) == 0
    names = list(arms)
    t = {name: [] for name in names}
    for r in range(args.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            t[name].append(timed(arms[name][0]))

lines = []
for name in names:
    s = sorted(t[name])
    lines.append(json.dumps({
        "arm": name, "lib": os.path.basename(_lib.LIB_PATH), "rounds": args.rounds,
        "median_us": round(1e3 * s[len(s) // 2], 2), "p10_us": round(1e3 * s[len(s) // 10], 2),
        "p90_us": round(1e3 * s[(9 * len(s)) // 10], 2), "sha256": shas[name]}))
    print(lines[-1], flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
