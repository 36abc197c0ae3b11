"""Cost of per-block quantiser steps (csrc/stepmap.hip, the mapped coder of
csrc/rans.hip, codec.py) on the GPU, in one process, warm, the arms alternating inside every round
(diagnostic; needs a GPU). 64 images of 256×256, N = 192, blocks of 2×2 latent positions (an 8×8
map per image, so that one image can hold all 32 steps):

  compress    compress_images(step=12), the single-step path, against step_offsets with a zero map
              and with checkerboards of 2, 8, 16 and 32 distinct steps; event brackets around the whole
              call, which ends in host work, so the host clock is given too
  decompress  decompress_images on the blobs of each arm
  sweep       kernels.rate_sweep against kernels.rate_sweep_offsets (zero and mixed offsets)
  coder       the entropy coder alone on the quantised latents of each map: rans_encode_map /
              rans_decode_map with the LDS table window against the same with every table row read
              from global memory, and the single-step rans_encode / rans_decode beside them

    python tools/stepmap_time.py [--rounds 30] [--codec-rounds 7] [--out profiles/stepmap_ab.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from iclr_17_compression_amd import codec, kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--codec-rounds", type=int, default=7)
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []
BASE, G, N, K, P = 12, 2, 192, kernels.ENTROPY_K, kernels.STREAMS_PER_IMAGE


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    lines.append(line)


def stats(ms):
    s = sorted(ms)
    return {"median_us": round(1e3 * s[len(s) // 2], 2), "p10_us": round(1e3 * s[len(s) // 10], 2),
            "p90_us": round(1e3 * s[(9 * len(s)) // 10], 2)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(arms, rounds, wall=None):
    """Every arm once per round, the order rotating by one each round → {name: [ms]}."""
    names = list(arms)
    t = {n: [] for n in names}
    for r in range(rounds):
        for n in names[r % len(names):] + names[:r % len(names)]:
            w0 = time.perf_counter()
            t[n].append(timed(arms[n]))
            if wall is not None:
                wall.setdefault(n, []).append(1e3 * (time.perf_counter() - w0))
    return t


def checkerboard(n):
    """An 8×8 offset map with n distinct values around 0 (n = 32: −12..19, every ladder index at
    base 12); n = 1: zeros."""
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    k = (5 * i + j) % n
    return (k - (12 if n == 32 else n // 2)).astype(np.int8)


net = ImageCompressor(out_channel_N=N)
net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
net = net.to(dev).eval()
imgs = [np.ascontiguousarray(synth.smooth_image_u8(300 + k, 256, 256).transpose(1, 2, 0))
        for k in range(64)]
DELTAS = [codec.step_size(s) for s in range(codec.STEPS)]
MAPS = {"zero map": 1, "2 steps": 2, "8 steps": 8, "16 steps": 16, "32 steps": 32}

with torch.no_grad():
    # ------------------------------------------------------------------ compress / decompress
    arms = {"step=12": lambda: net.compress_images(imgs, step=BASE)}
    for name, n in MAPS.items():
        arms[name] = (lambda off: lambda: net.compress_images(
            imgs, step=BASE, step_offsets=[off] * 64, block=G))(checkerboard(n))
    blobs = {name: fn() for name, fn in arms.items()}
    for name in MAPS:
        used = {int(e) for b in blobs[name] for e in np.unique(codec.parse_blob(b)[1].indices)}
        assert len(used) == MAPS[name], (name, used)
    for fn in arms.values():
        fn()
    wall = {}
    t = alternate(arms, args.codec_rounds, wall)
    for name in arms:
        emit({"arm": "compress", "what": name, "images": 64, "size": "256x256", "block": G,
              "rounds": args.codec_rounds, **stats(t[name]),
              "host_median_ms": round(sorted(wall[name])[len(wall[name]) // 2], 2),
              "bytes_total": sum(len(b) for b in blobs[name])})
    darms = {name: (lambda bl: lambda: net.decompress_images(bl))(blobs[name]) for name in arms}
    for fn in darms.values():
        fn()
    wall = {}
    t = alternate(darms, args.codec_rounds, wall)
    for name in darms:
        emit({"arm": "decompress", "what": name, "images": 64, "rounds": args.codec_rounds,
              **stats(t[name]), "host_median_ms": round(sorted(wall[name])[len(wall[name]) // 2], 2)})

    # ------------------------------------------------------------------ sweep
    x = torch.stack([torch.from_numpy(im).permute(2, 0, 1).float().div(255) for im in imgs]).to(dev)
    y = net.latents(x)
    pack = net.bitEstimator.packed()
    zero = torch.zeros(64, 8, 8, dtype=torch.int8)
    mixed = torch.from_numpy(np.broadcast_to(checkerboard(32), (64, 8, 8)).copy())
    sarms = {"rate_sweep": lambda: kernels.rate_sweep(y, pack, DELTAS),
             "rate_sweep_offsets, zero": lambda: kernels.rate_sweep_offsets(y, pack, DELTAS, zero, G),
             "rate_sweep_offsets, 32 offsets": lambda: kernels.rate_sweep_offsets(y, pack, DELTAS, mixed, G)}
    assert torch.equal(sarms["rate_sweep"](), sarms["rate_sweep_offsets, zero"]())
    for fn in sarms.values():
        fn()
    t = alternate(sarms, args.rounds)
    for name in sarms:
        emit({"arm": "sweep", "what": name, "shape": list(y.shape), "rounds": args.rounds,
              **stats(t[name])})

    # ------------------------------------------------------------------ coder: window vs global
    y12, _ = kernels.quantise_step(y, DELTAS[BASE])
    t12 = net.bitEstimator.entropy_tables(K, step=BASE)
    w12, o12 = kernels.rans_encode(y12, t12, K, P)
    carms = {"encode single-step": lambda: kernels.rans_encode(y12, t12, K, P),
             "decode single-step": lambda: kernels.rans_decode(w12, o12, t12, 64, 16, 16, N, K, P)}
    for name, n in MAPS.items():
        emap = codec.effective_indices(BASE, np.broadcast_to(checkerboard(n), (64, 8, 8)))
        tables, slots = net._map_tables(emap, K)
        yq, _ = kernels.quantise_step_map(y, emap, G, DELTAS)
        words, offs = kernels.rans_encode_map(yq, tables, slots, G, K, P, window=True)
        wg, og = kernels.rans_encode_map(yq, tables, slots, G, K, P, window=False)
        assert torch.equal(words, wg) and torch.equal(offs, og)
        for window, label in ((True, "window"), (False, "global")):
            carms[f"encode {name}, {label}"] = (lambda a: lambda: kernels.rans_encode_map(*a))(
                (yq, tables, slots, G, K, P, window))
            carms[f"decode {name}, {label}"] = (lambda a: lambda: kernels.rans_decode_map(*a))(
                (words, offs, tables, slots, G, 64, 16, 16, N, K, P, window))
    for fn in carms.values():
        fn()
    t = alternate(carms, args.rounds)
    for name in carms:
        emit({"arm": "coder", "what": name, "streams": 64 * P, "rounds": args.rounds, **stats(t[name])})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
