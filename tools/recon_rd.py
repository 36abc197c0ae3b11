"""Effect of centroid reconstruction on trained weights (diagnostic, needs a GPU):
tests/golden/g9_weights_n192.npz on the synthetic Kodak-24 set, ladder indices 4…16. Every index is
encoded once (``compress_images(step=s)``); the same blobs are then decoded at the bin centre, with
recon="centroid" and with recon="zero", each at strengths 0.25, 0.5, 0.75 and 1. Per index and arm:
the means over the 24 images of psnr_u8 and MS-SSIM of the 8-bit decode, and their differences
from the centre's at identical bytes; then a summary per arm and index range.

    python tools/recon_rd.py [--out profiles/recon_rd.txt] [--first 4] [--last 16]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from iclr_17_compression_amd import codec, kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--first", type=int, default=4)
ap.add_argument("--last", type=int, default=16)
ap.add_argument("--strengths", default="0.25,0.5,0.75,1")
args = ap.parse_args()
dev = torch.device("cuda:0")
PORTRAIT = (3, 8, 9, 16, 17, 18)
STRENGTHS = [float(v) for v in args.strengths.split(",")]
out = open(args.out, "w") if args.out else None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


d = np.load(os.path.join(REPO, "tests", "golden", "g9_weights_n192.npz"))
net = ImageCompressor(out_channel_N=192)
net.load_state_dict({k: torch.from_numpy(d[k].astype(np.float32)) for k in d.files})
net = net.to(dev).eval()
imgs = [np.ascontiguousarray(synth.smooth_image_u8(100 + i, *((768, 512) if i in PORTRAIT
                                                             else (512, 768))).transpose(1, 2, 0))
        for i in range(24)]
refs = [(torch.from_numpy(im).to(dev).permute(2, 0, 1).float() / 255)[None].contiguous() for im in imgs]
emit({"weights": "g9_weights_n192.npz", "images": "kodak-synth 24", "indices": [args.first, args.last],
      "strengths": STRENGTHS, "metric": "8-bit decode of the same blobs; differences from the centre"})


def measure(blobs, **kw):
    """Mean psnr_u8 and MS-SSIM of the blobs' decode under ``kw``."""
    recons, sses = codec.decode_groups(net, blobs, 64, refs=imgs, **kw)
    psnr, ms = [], []
    for im, rec, sse, ref in zip(imgs, recons, sses, refs):
        H, W = im.shape[:2]
        psnr.append(10.0 * math.log10(255.0 ** 2 * 3 * H * W / sse) if sse else math.inf)
        x = (torch.from_numpy(rec).to(dev).permute(2, 0, 1).float() / 255)[None].contiguous()
        ms.append(float(kernels.ms_ssim(x, ref, data_range=1.0)[0]))
    return float(np.mean(psnr)), float(np.mean(ms))


def db(ms):
    return -10.0 * math.log10(1.0 - ms)


table = {}
with torch.no_grad():
    for s in range(args.first, args.last + 1):
        blobs = net.compress_images(imgs, step=s)
        bpp = float(np.mean([8 * len(b) / (im.shape[0] * im.shape[1]) for b, im in zip(blobs, imgs)]))
        p0, m0 = measure(blobs)
        assert (p0, m0) == measure(blobs, recon="centre")
        emit({"index": s, "step": round(codec.step_size(s), 4), "arm": "centre", "bpp": round(bpp, 5),
              "psnr_u8": round(p0, 4), "ms_ssim": round(m0, 6), "ms_ssim_db": round(db(m0), 4)})
        for mode in ("centroid", "zero"):
            for a in STRENGTHS:
                p, m = measure(blobs, recon=mode, recon_strength=a)
                table[(mode, a, s)] = (p - p0, db(m) - db(m0))
                emit({"index": s, "arm": mode, "strength": a, "bpp": round(bpp, 5),
                      "psnr_u8": round(p, 4), "psnr_minus_centre_db": round(p - p0, 4),
                      "ms_ssim": round(m, 6), "ms_ssim_db_minus_centre": round(db(m) - db(m0), 4)})

for mode in ("centroid", "zero"):
    for a in STRENGTHS:
        for lo, hi in ((args.first, 8), (9, args.last)):
            rows = [table[(mode, a, s)] for s in range(lo, hi + 1) if (mode, a, s) in table]
            if rows:
                emit({"arm": mode, "strength": a, "summary": f"indices {lo}..{hi}",
                      "psnr_minus_centre_db": {"min": round(min(r[0] for r in rows), 4),
                                               "mean": round(float(np.mean([r[0] for r in rows])), 4),
                                               "max": round(max(r[0] for r in rows), 4)},
                      "ms_ssim_db_minus_centre": {"min": round(min(r[1] for r in rows), 4),
                                                  "mean": round(float(np.mean([r[1] for r in rows])), 4),
                                                  "max": round(max(r[1] for r in rows), 4)}})
if out:
    out.close()
