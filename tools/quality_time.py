"""Cost and probe counts of quality targets (csrc/quality.hip, image_sse in
csrc/imageio.hip, codec.py) on the GPU, in one process, warm, the arms alternating inside every
round (diagnostic; needs a GPU).

  kernels   at y [64,16,16,192] / 64 images of 256×256, entry points on preallocated buffers:
            iclr17_quantise_steps against iclr17_quantise_step, iclr17_image_sse_u8 against
            iclr17_image_egress_u8 with a reference, iclr17_distortion_sweep against
            iclr17_rate_sweep (32 steps each), with the bytes each moves
  probe     one probe round of the 64 images (quantise_steps + synthesis + image_sse + one small
            transfer) against one evaluate_images(step=) trial, the host loop it replaces
  compress  compress_images(psnr=T), guided and bisecting, against compress_images(step=s) at the
            index found; event brackets around whole calls, host clock beside them
  probes    tests/golden/g9_weights_n192.npz on the synthetic Kodak-24 set at three targets:
            probes per image guided and bisecting, and how far the calibrated prediction's first
            guess lands from the index found

    python tools/quality_time.py [--rounds 30] [--codec-rounds 7] [--out profiles/quality_ab.txt]
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
N = 192
PORTRAIT = (3, 8, 9, 16, 17, 18)


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


def median(v):
    return sorted(v)[len(v) // 2]


# trained weights throughout: a target search on untrained ones meets a PSNR that barely moves
d = np.load(os.path.join(REPO, "tests", "golden", "g9_weights_n192.npz"))
net = ImageCompressor(out_channel_N=N)
net.load_state_dict({k: torch.from_numpy(d[k].astype(np.float32)) for k in d.files})
net = net.to(dev).eval()
imgs = [np.ascontiguousarray(synth.smooth_image_u8(300 + k, 256, 256).transpose(1, 2, 0))
        for k in range(64)]
DELTAS = [codec.step_size(s) for s in range(codec.STEPS)]
p = kernels._p

with torch.no_grad():
    packed, offsets, shapes = codec.upload_packed(imgs, dev)
    x = kernels.image_ingest(packed, offsets, shapes, (256, 256))
    y = net.latents(x).contiguous()
    B, h, w, _ = y.shape
    st = kernels._stream(y)
    pack = net.bitEstimator.packed()
    gains = net.synthesis_gains_raw()

    # ------------------------------------------------------------------ kernels
    y_hat, y_deq = torch.empty_like(y), torch.empty_like(y)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    steps_dev = torch.tensor([DELTAS[4 + k % 12] for k in range(B)], dtype=torch.float32, device=dev)
    d8 = ctypes.c_float(DELTAS[8])
    latent_bytes = 4 * y.numel()
    qarms = {
        "quantise_step (one step)": (lambda: _lib.call(
            "iclr17_quantise_step", p(y), y.numel(), d8, p(y_hat), p(y_deq), p(status), st), 3 * latent_bytes),
        "quantise_steps (a step per image)": (lambda: _lib.call(
            "iclr17_quantise_steps", p(y), B, y.numel() // B, p(steps_dev), p(y_hat), p(y_deq), p(status),
            st), 3 * latent_bytes),
        "quantise_steps, no y_hat (the probe's)": (lambda: _lib.call(
            "iclr17_quantise_steps", p(y), B, y.numel() // B, p(steps_dev), None, p(y_deq), p(status), st),
            2 * latent_bytes)}
    recon = net.decompress(net.compress_latents(y, 8)["strings"], (h, w), step=8)["x_hat"].contiguous()
    desc = kernels._image_desc("image_sse", packed.numel(), offsets, shapes, (256, 256)).to(dev)
    dst = torch.empty_like(packed)
    sse = torch.zeros(B, device=dev, dtype=torch.int64)
    pix = packed.numel()
    earms = {
        "image_egress_u8 with ref": (lambda: _lib.call(
            "iclr17_image_egress_u8", p(recon), p(desc), B, 256, 256, p(dst), p(packed), p(sse), p(status),
            st), 4 * recon.numel() + 2 * pix),
        "image_sse_u8": (lambda: _lib.call(
            "iclr17_image_sse_u8", p(recon), p(desc), B, 256, 256, p(packed), p(sse), p(status), st),
            4 * recon.numel() + pix)}
    T = _lib.query("iclr17_rate_sweep_partials", h, w, N)
    spartial = torch.empty(B * 32 * T, device=dev, dtype=torch.float64)
    sout = torch.empty(B, 32, device=dev, dtype=torch.float64)
    arr = (ctypes.c_float * 32)(*DELTAS)
    steps = ctypes.cast(arr, ctypes.c_void_p)
    sarms = {
        "rate_sweep, 32 steps": (lambda: _lib.call(
            "iclr17_rate_sweep", p(y), B, h, w, N, p(pack), steps, 32, p(spartial), p(sout), st),
            latent_bytes),
        "distortion_sweep, 32 steps": (lambda: _lib.call(
            "iclr17_distortion_sweep", p(y), B, h, w, N, p(gains), steps, 32, p(spartial), p(sout), st),
            latent_bytes)}
    for family, arms in (("quantise", qarms), ("sse", earms), ("sweep", sarms)):
        fns = {k: v[0] for k, v in arms.items()}
        for fn in fns.values():
            fn()
        t = alternate(fns, args.rounds)
        for name, (_, nbytes) in arms.items():
            s = stats(t[name])
            emit({"arm": "kernels", "family": family, "what": name, "images": B, "rounds": args.rounds,
                  **s, "bytes": nbytes, "GB_per_s": round(nbytes / (s["median_us"] * 1e-6) / 1e9, 1)})

    # ------------------------------------------------------------------ probe round vs a trial
    probe = codec.quality_probe(net, y, packed, offsets, shapes)
    members, idx8 = list(range(B)), [4 + k % 12 for k in range(B)]
    parms = {"one probe round (64 images, mixed indices)": lambda: probe(members, idx8),
             "one evaluate_images(step=8) trial": lambda: net.evaluate_images(imgs, step=8)}
    same = probe(members, [8] * B)
    assert same == [r["sse_u8"] for r in net.evaluate_images(imgs, step=8)]
    for fn in parms.values():
        fn()
    wall = {}
    t = alternate(parms, args.codec_rounds, wall)
    for name in parms:
        emit({"arm": "probe", "what": name, "images": B, "size": "256x256", "rounds": args.codec_rounds,
              **stats(t[name]), "host_median_ms": round(median(wall[name]), 2)})

    # ------------------------------------------------------------------ compress
    rows = net.evaluate_images(imgs, step=12)
    target = float(np.floor(2.0 * min(r["psnr_u8"] for r in rows)) / 2.0)   # every image reaches it
    st_g, st_b = {}, {}
    blobs = net.compress_images(imgs, psnr=target, stats=st_g, estimate=True)
    same = blobs == net.compress_images(imgs, psnr=target, stats=st_b, estimate=False)
    found = [codec.parse_blob(b)[1] for b in blobs]
    s_mid = int(np.median(found))
    carms = {"psnr=T, guided": lambda: net.compress_images(imgs, psnr=target, estimate=True),
             "psnr=T, bisection": lambda: net.compress_images(imgs, psnr=target, estimate=False),
             f"step={s_mid} (the median index found)": lambda: net.compress_images(imgs, step=s_mid)}
    for fn in carms.values():
        fn()
    wall = {}
    t = alternate(carms, args.codec_rounds, wall)
    for name in carms:
        emit({"arm": "compress", "what": name, "images": B, "size": "256x256", "target_db": round(target, 3),
              "indices_found": [min(found), s_mid, max(found)], "rounds": args.codec_rounds, **stats(t[name]),
              "host_median_ms": round(median(wall[name]), 2),
              "guided_equals_bisection": same,
              "probes_mean_guided": round(float(np.mean(st_g["probes"])), 3),
              "probes_mean_bisection": round(float(np.mean(st_b["probes"])), 3)})

    # ------------------------------------------------------------------ guided against bisection
    g9 = net
    kodak = [np.ascontiguousarray(synth.smooth_image_u8(100 + i, *((768, 512) if i in PORTRAIT
                                                                  else (512, 768))).transpose(1, 2, 0))
             for i in range(24)]
    ladder = {s: [r["psnr_u8"] for r in g9.evaluate_images(kodak, step=s)] for s in (4, 8, 12, 16)}
    emit({"arm": "probes", "weights": "g9_weights_n192.npz", "images": "kodak-synth 24",
          "mean_psnr_at_index": {str(s): round(float(np.mean(v)), 3) for s, v in ladder.items()}})
    for s_ref in (6, 10, 14):
        # a target every image can reach: the set's lowest PSNR at a reference index, rounded down
        rows = g9.evaluate_images(kodak, step=s_ref)
        target = float(np.floor(2.0 * min(r["psnr_u8"] for r in rows)) / 2.0)
        out = {}
        for name, estimate in (("guided", True), ("bisection", False)):
            stt = {}
            b = g9.compress_images(kodak, psnr=target, stats=stt, estimate=estimate)
            out[name] = ([codec.parse_blob(q)[1] for q in b], stt["probes"])
        # the calibrated prediction's first guess, per image, against the index found
        guesses = []
        for idx in codec.group_by_canvas([im.shape[:2] for im in kodak], 64):
            group = [kodak[i] for i in idx]
            pk, of, sh = codec.upload_packed(group, dev)
            yy = g9.latents(kernels.image_ingest(pk, of, sh, codec.canvas(*sh[0])))
            tg = [codec.QualityTarget(str(i), target, H, W, codec.sse_limit(H, W, target))
                  for i, (H, W) in zip(idx, sh)]
            res = codec.search_quality(codec.quality_probe(g9, yy, pk, of, sh), len(idx),
                                       codec.quality_seeds(g9, yy), tg)
            guesses += [(i, g, f) for i, g, f in zip(idx, res.guesses, res.indices)]
        miss = [abs(min(max(g, 0), 31) - f) for _, g, f in guesses if g is not None]
        emit({"arm": "probes", "target_db": target, "reference_index": s_ref,
              "indices_found_min_mean_max": [min(out["guided"][0]),
                                             round(float(np.mean(out["guided"][0])), 2),
                                             max(out["guided"][0])],
              "same_indices": out["guided"][0] == out["bisection"][0],
              "probes_guided_mean": round(float(np.mean(out["guided"][1])), 3),
              "probes_guided_max": max(out["guided"][1]),
              "probes_bisection_mean": round(float(np.mean(out["bisection"][1])), 3),
              "probes_bisection_max": max(out["bisection"][1]),
              "guess_miss_mean": round(float(np.mean(miss)), 3) if miss else None,
              "guess_miss_max": max(miss) if miss else None,
              "guess_exact_share": round(float(np.mean([m == 0 for m in miss])), 3) if miss else None})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
