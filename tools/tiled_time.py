"""Cost of tiled rANS streams (the tiled kernels of csrc/rans.hip, codec.py) on the
GPU, in one process, warm, the arms alternating inside every round (diagnostic; needs a GPU).
N = 192, one 2048×2048 and one 4096×3072 image from synth:

  compress    compress_images untiled with P = 1 (the path before tiles) and P = 4, and with
              tile = 8, 16, 32, 64; event brackets around the whole call, which ends in host work,
              so the host clock is given too
  decompress  decompress_images on the blobs of each arm
  coder       the entropy coder alone on the image's ŷ: rans_encode / rans_decode with P = 1 and 4
              against rans_encode_tiled / rans_decode_tiled at every tile edge with 1, 4, 8 and 16
              waves per workgroup (1: a table set staged per stream; more: one shared by that
              many streams)
  region      decompress_region of a 512×512 box against decompress_images of the same blob
  bytes       the blob of each tile edge against the untiled blob at steps 4, 8 and 12
  streams     the coder alone on 16 copies of the 2048×2048 ŷ at tile = 8 and 16: 4096 and 1024
              streams, more than the GPU holds one-wave workgroups at a time
  batch       64 images of 256×256 with and without tile = 16 (one tile per image); the tiled
              blob carries a ladder index, so the untiled call at step 8 (I17Q) stands beside it

    python tools/tiled_time.py [--rounds 15] [--codec-rounds 5] [--out profiles/tiled_ab.txt]
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
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--codec-rounds", type=int, default=5)
ap.add_argument("--sizes", default="2048x2048,4096x3072", help="HxW,... of the single images")
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []
N, K = 192, kernels.ENTROPY_K
WAVES = (1, 4, 8, 16)


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


def host_median(wall, name):
    return round(sorted(wall[name])[len(wall[name]) // 2], 2)


def image(seed, H, W):
    return np.ascontiguousarray(synth.smooth_image_u8(seed, H, W).transpose(1, 2, 0))


net = ImageCompressor(out_channel_N=N)
net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
net = net.to(dev).eval()
LAYOUTS = {"untiled P=1": {}, "untiled P=4": {"streams_per_image": 4}}
LAYOUTS.update({f"tile={t}": {"tile": t} for t in kernels.TILES})

with torch.no_grad():
    for k, size in enumerate(args.sizes.split(",")):
        H, W = (int(v) for v in size.split("x"))
        img = image(400 + k, H, W)
        h, w = H // 16, W // 16
        # ---------------------------------------------------------------- compress / decompress
        arms = {name: (lambda kw: lambda: net.compress_images([img], **kw))(kw)
                for name, kw in LAYOUTS.items()}
        blobs = {name: fn()[0] for name, fn in arms.items()}
        ref = net.decompress_images([blobs["untiled P=1"]])[0]
        for name, b in blobs.items():   # the same picture from every layout
            assert np.array_equal(net.decompress_images([b])[0], ref), name
        wall = {}
        t = alternate(arms, args.codec_rounds, wall)
        for name in arms:
            emit({"arm": "compress", "what": name, "size": size, "rounds": args.codec_rounds,
                  **stats(t[name]), "host_median_ms": host_median(wall, name),
                  "bytes": len(blobs[name])})
        darms = {name: (lambda b: lambda: net.decompress_images([b]))(blobs[name]) for name in arms}
        wall = {}
        t = alternate(darms, args.codec_rounds, wall)
        for name in darms:
            emit({"arm": "decompress", "what": name, "size": size, "rounds": args.codec_rounds,
                  **stats(t[name]), "host_median_ms": host_median(wall, name)})

        # ---------------------------------------------------------------- the coder alone
        x = kernels.image_ingest(*codec.upload_packed([img], dev), (H, W))
        y_hat, _ = kernels.quantise_step(net.latents(x), 1.0)
        cum = net.bitEstimator.entropy_tables(K)
        carms = {}
        for P in (1, 4):
            wd, of = kernels.rans_encode(y_hat, cum, K, P)
            carms[f"encode untiled P={P}"] = (lambda P: lambda: kernels.rans_encode(y_hat, cum, K, P))(P)
            carms[f"decode untiled P={P}"] = (lambda a: lambda: kernels.rans_decode(*a))(
                (wd, of, cum, 1, h, w, N, K, P))
        for tile in kernels.TILES:
            wd, of = kernels.rans_encode_tiled(y_hat, cum, tile, K, 1)
            assert torch.equal(kernels.rans_decode_tiled(wd, of, cum, 1, h, w, N, tile, K, 1), y_hat)
            for wv in WAVES:
                carms[f"encode tile={tile} waves={wv}"] = (lambda a: lambda: kernels.rans_encode_tiled(*a))(
                    (y_hat, cum, tile, K, 1, wv))
                carms[f"decode tile={tile} waves={wv}"] = (lambda a: lambda: kernels.rans_decode_tiled(*a))(
                    (wd, of, cum, 1, h, w, N, tile, K, 1, None, wv))
        for fn in carms.values():
            fn()
        t = alternate(carms, args.rounds)
        for name in carms:
            emit({"arm": "coder", "what": name, "size": size, "symbols": h * w * N,
                  "rounds": args.rounds, **stats(t[name])})

        # ---------------------------------------------------------------- region decode
        box = (W // 2 - 256, H // 2 - 256, W // 2 + 256, H // 2 + 256)
        rarms = {}
        for tile in kernels.TILES:
            b = blobs[f"tile={tile}"]
            st = {}
            got = net.decompress_region(b, box, stats=st)
            assert np.array_equal(got, ref[box[1]:box[3], box[0]:box[2]]), tile
            rarms[f"region tile={tile} ({st['streams_decoded']} of {st['streams_total']} streams)"] = \
                (lambda b: lambda: net.decompress_region(b, box))(b)
            rarms[f"full tile={tile}"] = (lambda b: lambda: net.decompress_images([b]))(b)
        wall = {}
        t = alternate(rarms, args.codec_rounds, wall)
        for name in rarms:
            emit({"arm": "region", "what": name, "size": size, "box": "512x512",
                  "rounds": args.codec_rounds, **stats(t[name]),
                  "host_median_ms": host_median(wall, name)})

        # ---------------------------------------------------------------- bytes
        for step in (4, 8, 12):
            base = len(net.compress_images([img], step=step)[0])
            row = {"arm": "bytes", "size": size, "step": step, "untiled": base,
                   "bpp_untiled": round(8 * base / (H * W), 4)}
            for tile in kernels.TILES:
                n = len(net.compress_images([img], step=step, tile=tile)[0])
                row[f"tile={tile}"] = n
                row[f"tile={tile} over"] = f"{100.0 * (n - base) / base:.2f}%"
            emit(row)
        # ---------------------------------------------------------------- many streams
        if k == 0:
            many = y_hat.expand(16, h, w, N).contiguous()
            sarms = {}
            for tile in (8, 16):
                wd, of = kernels.rans_encode_tiled(many, cum, tile, K, 1)
                for wv in WAVES:
                    sarms[f"encode 16 x tile={tile} waves={wv}"] = \
                        (lambda a: lambda: kernels.rans_encode_tiled(*a))((many, cum, tile, K, 1, wv))
                    sarms[f"decode 16 x tile={tile} waves={wv}"] = \
                        (lambda a: lambda: kernels.rans_decode_tiled(*a))(
                            (wd, of, cum, 16, h, w, N, tile, K, 1, None, wv))
            for fn in sarms.values():
                fn()
            t = alternate(sarms, args.rounds)
            for name in sarms:
                emit({"arm": "streams", "what": name, "size": "16 x " + size,
                      "symbols": 16 * h * w * N, "rounds": args.rounds, **stats(t[name])})
            del many, sarms, wd, of
        del x, y_hat
        torch.cuda.empty_cache()

    # -------------------------------------------------------------------- the batch case
    imgs = [image(300 + k, 256, 256) for k in range(64)]
    barms = {"64x256x256 untiled": lambda: net.compress_images(imgs),
             "64x256x256 untiled step=8": lambda: net.compress_images(imgs, step=8),
             "64x256x256 tile=16": lambda: net.compress_images(imgs, tile=16)}
    bl = {name: fn() for name, fn in barms.items()}
    for name in list(bl):
        barms["decode " + name] = (lambda b: lambda: net.decompress_images(b))(bl[name])
    for fn in barms.values():
        fn()
    wall = {}
    t = alternate(barms, args.codec_rounds, wall)
    for name in barms:
        emit({"arm": "batch", "what": name, "rounds": args.codec_rounds, **stats(t[name]),
              "host_median_ms": host_median(wall, name)})

    # the same 64 latents through the two coders alone: one stream per image either way
    x = torch.stack([torch.from_numpy(im).permute(2, 0, 1).float().div(255) for im in imgs]).to(dev)
    y_hat, _ = kernels.quantise_step(net.latents(x), 1.0)
    cum = net.bitEstimator.entropy_tables(K)
    wu, ou = kernels.rans_encode(y_hat, cum, K, 1)
    wt, ot = kernels.rans_encode_tiled(y_hat, cum, 16, K, 1)
    assert torch.equal(wu, wt) and torch.equal(ou, ot)   # one tile per image: the same words
    carms = {"encode 64 streams untiled": lambda: kernels.rans_encode(y_hat, cum, K, 1),
             "encode 64 streams tile=16": lambda: kernels.rans_encode_tiled(y_hat, cum, 16, K, 1),
             "decode 64 streams untiled": lambda: kernels.rans_decode(wu, ou, cum, 64, 16, 16, N, K, 1),
             "decode 64 streams tile=16": lambda: kernels.rans_decode_tiled(wt, ot, cum, 64, 16, 16, N,
                                                                            16, K, 1)}
    for fn in carms.values():
        fn()
    t = alternate(carms, args.rounds)
    for name in carms:
        emit({"arm": "batch coder", "what": name, "rounds": args.rounds, **stats(t[name])})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
