"""Cost of centroid reconstruction (csrc/recon.hip, codec.py) on the GPU, in one
process, warm, the arms alternating inside every round (diagnostic; needs a GPU). N = 192, K = 32:

  dequantise  kernels.dequantise_step against kernels.dequantise_recon on [64,16,16,192] (the
              table staged in LDS), and the mapped pair dequantise_step_map / dequantise_recon_map
              with all 32 ladder indices in every image (blocks of 2×2: an 8×8 map)
  offsets     kernels.recon_offsets for 1 step and for 32 steps
  decompress  decompress_images of 64 images of 256×256 at step=12: without recon, with it and a
              table made at every call (the cache cleared: cold), and with the cached table

    python tools/recon_time.py [--rounds 30] [--codec-rounds 7] [--out profiles/recon_ab.txt]
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
STEP, G, N, K = 12, 2, 192, kernels.ENTROPY_K


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


net = ImageCompressor(out_channel_N=N)
net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
net = net.to(dev).eval()
imgs = [np.ascontiguousarray(synth.smooth_image_u8(300 + k, 256, 256).transpose(1, 2, 0))
        for k in range(64)]
DELTAS = [codec.step_size(s) for s in range(codec.STEPS)]

with torch.no_grad():
    # ------------------------------------------------------------------ the dequantisers
    x = torch.stack([torch.from_numpy(im).permute(2, 0, 1).float().div(255) for im in imgs]).to(dev)
    y_hat, _ = kernels.quantise_step(net.latents(x), DELTAS[STEP])
    pack = net.bitEstimator.packed()
    one = kernels.recon_offsets(pack, N, K, [DELTAS[STEP]], "centroid", 1.0)[0]
    stack = kernels.recon_offsets(pack, N, K, DELTAS, "centroid", 1.0)
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    emap = np.broadcast_to(((5 * i + j) % 32).astype(np.uint8), (64, 8, 8)).copy()
    inside = float((y_hat.abs() <= K).float().mean())
    arms = {"dequantise_step": lambda: kernels.dequantise_step(y_hat, DELTAS[STEP]),
            "dequantise_recon": lambda: kernels.dequantise_recon(y_hat, DELTAS[STEP], one, K),
            "dequantise_step_map, 32 indices":
                lambda: kernels.dequantise_step_map(y_hat, emap, G, DELTAS),
            "dequantise_recon_map, 32 indices":
                lambda: kernels.dequantise_recon_map(y_hat, emap, G, DELTAS, stack, K)}
    for fn in arms.values():
        fn()
    t = alternate(arms, args.rounds)
    nbytes = 8 * y_hat.numel()
    for name in arms:
        s = stats(t[name])
        emit({"arm": "dequantise", "what": name, "shape": list(y_hat.shape), "rounds": args.rounds,
              **s, "latent_GB_per_s_at_median": round(nbytes / (s["median_us"] * 1e3), 1),
              "levels_inside_K": round(inside, 4)})

    # ------------------------------------------------------------------ the tables
    oarms = {"recon_offsets, 1 step": lambda: kernels.recon_offsets(pack, N, K, [DELTAS[STEP]],
                                                                    "centroid", 1.0),
             "recon_offsets, 32 steps": lambda: kernels.recon_offsets(pack, N, K, DELTAS,
                                                                      "centroid", 1.0),
             "recon_offsets, 32 steps, zero bin only": lambda: kernels.recon_offsets(
                 pack, N, K, DELTAS, "zero", 1.0)}
    for fn in oarms.values():
        fn()
    t = alternate(oarms, args.rounds)
    for name in oarms:
        emit({"arm": "offsets", "what": name, "N": N, "K": K, "rounds": args.rounds, **stats(t[name])})

    # ------------------------------------------------------------------ decompress_images
    blobs = net.compress_images(imgs, step=STEP)

    def cleared(**kw):
        # every table of the BitEstimator is made again: the coder's CDFs too, so the centre arm
        # of this group is the baseline of the cold one
        def run():
            net.bitEstimator._pack.invalidate()
            return net.decompress_images(blobs, **kw)
        return run

    groups = [{"centre": lambda: net.decompress_images(blobs),
               "centroid, cached table": lambda: net.decompress_images(blobs, recon="centroid"),
               "zero, cached table": lambda: net.decompress_images(blobs, recon="zero")},
              {"centre, cache cleared": cleared(),
               "centroid, cache cleared (cold)": cleared(recon="centroid"),
               "zero, cache cleared (cold)": cleared(recon="zero")}]
    for darms in groups:   # a group at a time: clearing the cache would make the cached arms cold
        for fn in darms.values():
            fn()
        wall = {}
        t = alternate(darms, args.codec_rounds, wall)
        for name in darms:
            emit({"arm": "decompress", "what": name, "images": 64, "size": "256x256", "step": STEP,
                  "rounds": args.codec_rounds, **stats(t[name]),
                  "host_median_ms": round(sorted(wall[name])[len(wall[name]) // 2], 2)})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
