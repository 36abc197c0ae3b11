"""Cost of rate control (csrc/ratectl.hip, codec.py) on the GPU, in one process, arms alternating
inside every round (diagnostic; needs a GPU):

  sweep    kernels.rate_sweep of y [64,16,16,192] at all 32 ladder steps (one launch pair) against
           the only way to get the same numbers before it: 32 × (rate_bits + reduce_partials) on
           latents quantised beforehand with the step packs made beforehand. HIP-event brackets,
           warm; median and p10–p90, and in how many of the alternating pairs the sweep lost.
  codec    compress_images of 64 images of 256×256 with a byte budget (half the plain size of each
           image) against the plain call; event brackets around the whole call, which ends in host
           work, so the host clock is given too.
  loop     how often the estimate-then-verify loop codes an image again, on the images of
           tests/test_gpu_ratectl.py at the budgets used there and on the 64 × 256² set.

    python tools/ratectl_time.py [--rounds 30] [--codec-rounds 5] [--out profiles/ratectl_ab.txt]
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
ap.add_argument("--codec-rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


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


def make_net(N):
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
    return net.to(dev).eval()


def smooth(seed, H, W):
    return np.ascontiguousarray(synth.smooth_image_u8(seed, H, W).transpose(1, 2, 0))


DELTAS = [codec.step_size(s) for s in range(codec.STEPS)]

with torch.no_grad():
    # ------------------------------------------------------------------ sweep
    net = make_net(192)
    imgs = [smooth(300 + k, 256, 256) for k in range(64)]
    x = torch.stack([torch.from_numpy(im).permute(2, 0, 1).float().div(255) for im in imgs]).to(dev)
    y = net.latents(x)
    pack = net.bitEstimator.packed()
    quantised = [kernels.quantise_step(y, d)[0].permute(0, 3, 1, 2) for d in DELTAS]
    packs = [kernels.pack_rate_step(pack, 192, d) for d in DELTAS]

    def fused():
        return kernels.rate_sweep(y, pack, DELTAS)

    def separate():
        return [kernels.reduce_partials(kernels.rate_bits(q, p))[0] for q, p in zip(quantised, packs)]

    want = torch.stack(separate(), dim=1)
    emit({"arm": "sweep", "shape": list(y.shape), "steps": len(DELTAS),
          "max_rel_vs_separate": float(((fused() - want).abs() / want.abs()).max())})
    for _ in range(3):
        fused(), separate()
    t = {"fused": [], "separate": []}
    lost = 0
    for r in range(args.rounds):
        order = (("fused", fused), ("separate", separate)) if r % 2 == 0 else \
            (("separate", separate), ("fused", fused))
        pair = {}
        for name, fn in order:
            pair[name] = timed(fn)
            t[name].append(pair[name])
        lost += pair["fused"] > pair["separate"]
    for name in t:
        emit({"arm": "sweep", "what": name, "rounds": args.rounds, **stats(t[name])})
    emit({"arm": "sweep", "pairs_lost_by_fused": int(lost), "of": args.rounds,
          "median_ratio_separate_over_fused":
              round(sorted(t["separate"])[args.rounds // 2] / sorted(t["fused"])[args.rounds // 2], 3)})

    # ------------------------------------------------------------------ codec
    plain_sizes = [len(b) for b in net.compress_images(imgs)]
    budgets = [n // 2 for n in plain_sizes]

    def plain():
        return net.compress_images(imgs)

    def budgeted():
        return net.compress_images(imgs, max_bytes=budgets)

    for _ in range(2):
        plain(), budgeted()
    t = {"plain": [], "budgeted": []}
    wall = {"plain": [], "budgeted": []}
    for r in range(args.codec_rounds):
        for name, fn in (("plain", plain), ("budgeted", budgeted))[::1 if r % 2 == 0 else -1]:
            w0 = time.perf_counter()
            t[name].append(timed(fn))
            wall[name].append(1e3 * (time.perf_counter() - w0))
    for name in t:
        emit({"arm": "codec", "what": name, "images": 64, "size": "256x256",
              "rounds": args.codec_rounds, **stats(t[name]),
              "host_median_ms": round(sorted(wall[name])[len(wall[name]) // 2], 2)})
    st = {}
    blobs = net.compress_images(imgs, max_bytes=budgets, stats=st)
    steps = [codec.parse_blob(b)[1] for b in blobs]
    emit({"arm": "loop", "set": "64 x 256x256 N=192, budget = half the plain size",
          "images": 64, "reencodes_total": int(sum(st["reencodes"])),
          "reencodes_max": int(max(st["reencodes"])), "steps_min_max": [min(steps), max(steps)]})

    # ------------------------------------------------------------------ loop, the test images
    mixed = [(49, 83), (64, 96), (50, 96), (64, 81)]
    test_imgs = [smooth(60 + k, H, W) for k, (H, W) in enumerate(mixed)]
    for N in (128, 192):
        net = make_net(N)
        sizes = [len(b) for b in net.compress_images(test_imgs)]
        for frac in ((5, 4), (3, 4), (1, 2)):
            st = {}
            b = [n * frac[0] // frac[1] for n in sizes]
            blobs = net.compress_images(test_imgs, max_bytes=b, stats=st)
            emit({"arm": "loop", "set": f"test images N={N}", "budget": f"{frac[0]}/{frac[1]} L",
                  "plain_bytes": sizes, "bytes": [len(x) for x in blobs],
                  "steps": [codec.parse_blob(x)[1] for x in blobs], "reencodes": st["reencodes"]})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
