"""Cost of rate–distortion optimised quantisation (csrc/rdoq.hip, codec.py) on the
GPU, in one process, warm, the arms alternating inside every round (diagnostic; needs a GPU).
N = 192, y [64,16,16,192] (64 images of 256×256), λ = 1 with the synthesis gains:

  quantise  iclr17_quantise_rdo against what it fuses, the parent's iclr17_quantise_step +
            iclr17_rate_bits + iclr17_reduce_partials at the same step (entry points on
            preallocated buffers: no host checks, no status read), and the plain quantiser alone
  sweep     iclr17_rate_sweep_rdo against iclr17_rate_sweep, all 32 steps
  compress  compress_images(step=12) with and without rdo; event brackets around the whole call,
            which ends in host work, so the host clock is given too

    python tools/rdo_time.py [--rounds 30] [--codec-rounds 7] [--out profiles/rdo_ab.txt]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from iclr_17_compression_amd import _lib, codec, kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--codec-rounds", type=int, default=7)
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []
STEP, N, RDO = 12, 192, 1.0


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
p = kernels._p

with torch.no_grad():
    x = torch.stack([torch.from_numpy(im).permute(2, 0, 1).float().div(255) for im in imgs]).to(dev)
    y = net.latents(x).contiguous()
    B, h, w, _ = y.shape
    pack = net.bitEstimator.packed()
    lam = (net.synthesis_gains() * RDO).contiguous()
    st = kernels._stream(y)

    # ------------------------------------------------------------------ quantise
    for s in (4, STEP):
        d = ctypes.c_float(DELTAS[s])
        sp = kernels.pack_rate_step(pack, N, DELTAS[s])
        T = _lib.query("iclr17_rate_sweep_rdo_partials", h, w, N)
        y_hat, y_deq = torch.empty_like(y), torch.empty_like(y)
        partial = torch.empty(B, T, device=dev, dtype=torch.float64)
        bits = torch.empty(B, device=dev, dtype=torch.float64)
        total = torch.empty((), device=dev, dtype=torch.float32)
        status = torch.zeros(1, device=dev, dtype=torch.int32)

        def plain_quantise():
            _lib.call("iclr17_quantise_step", p(y), y.numel(), d, p(y_hat), p(y_deq), p(status), st)

        def parent():
            plain_quantise()
            _lib.call("iclr17_rate_bits", p(y_hat), B, N, h, w, _lib.ICLR17_LAYOUT_NHWC, p(sp),
                      p(partial), st)
            _lib.call("iclr17_reduce_partials", p(partial), B, T, p(bits), p(total),
                      ctypes.c_double(1.0), st)

        def fused():
            _lib.call("iclr17_quantise_rdo", p(y), B, h, w, N, p(pack), d, p(lam), p(y_hat), p(y_deq),
                      p(partial), p(bits), p(status), st)

        parent()
        plain_bits, r = bits.clone(), y_hat.clone()
        fused()
        rdo_bits = bits.clone()
        moved = float((y_hat != r).float().mean())
        nonzero = float((r != 0).float().mean())
        far = float((r.abs() >= 2).float().mean())
        assert bool((rdo_bits <= plain_bits).all()) and int(status.item()) == 0
        arms = {"quantise_step alone": plain_quantise,
                "quantise_step + rate_bits + reduce_partials": parent, "quantise_rdo": fused}
        for fn in arms.values():
            fn()
        t = alternate(arms, args.rounds)
        for name in arms:
            emit({"arm": "quantise", "what": name, "shape": list(y.shape), "index": s, "lam": RDO,
                  "rounds": args.rounds, **stats(t[name]), "nonzero_share": round(nonzero, 4),
                  "abs_ge_2_share": round(far, 4), "moved_share": round(moved, 4),
                  "bits_plain": round(float(plain_bits.sum()), 1), "bits_rdo": round(float(rdo_bits.sum()), 1)})

    # ------------------------------------------------------------------ sweep
    T = _lib.query("iclr17_rate_sweep_partials", h, w, N)
    spartial = torch.empty(B * 32 * T, device=dev, dtype=torch.float64)
    sbits = torch.empty(B, 32, device=dev, dtype=torch.float64)
    arr = (ctypes.c_float * 32)(*DELTAS)
    steps = ctypes.cast(arr, ctypes.c_void_p)
    sarms = {"rate_sweep": lambda: _lib.call("iclr17_rate_sweep", p(y), B, h, w, N, p(pack), steps, 32,
                                             p(spartial), p(sbits), st),
             "rate_sweep_rdo": lambda: _lib.call("iclr17_rate_sweep_rdo", p(y), B, h, w, N, p(pack),
                                                 steps, 32, p(lam), p(spartial), p(sbits), st)}
    assert torch.equal(kernels.rate_sweep_rdo(y, pack, DELTAS, lam)[:, STEP],
                       kernels.quantise_rdo(y, pack, DELTAS[STEP], lam)[2])
    for fn in sarms.values():
        fn()
    t = alternate(sarms, args.rounds)
    for name in sarms:
        emit({"arm": "sweep", "what": name, "shape": list(y.shape), "steps": 32, "lam": RDO,
              "rounds": args.rounds, **stats(t[name])})

    # ------------------------------------------------------------------ compress
    carms = {"step=12": lambda: net.compress_images(imgs, step=STEP),
             "step=12, rdo=1": lambda: net.compress_images(imgs, step=STEP, rdo=RDO)}
    blobs = {name: fn() for name, fn in carms.items()}
    for fn in carms.values():
        fn()
    wall = {}
    t = alternate(carms, args.codec_rounds, wall)
    for name in carms:
        emit({"arm": "compress", "what": name, "images": 64, "size": "256x256",
              "rounds": args.codec_rounds, **stats(t[name]),
              "host_median_ms": round(sorted(wall[name])[len(wall[name]) // 2], 2),
              "bytes_total": sum(len(b) for b in blobs[name])})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
