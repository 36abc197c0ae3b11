"""Rate–distortion effect of rate–distortion optimised quantisation on trained weights (DESIGN.md
§0j; diagnostic, needs a GPU): tests/golden/g9_weights_n192.npz on the synthetic Kodak-24 set,
ladder indices 4…16, plain rounding and λ in 0, 0.5, 2, 8, 32 with the synthesis gains. Per arm and
index the means over the 24 images of the real blobs' bpp, psnr_u8 and MS-SSIM (evaluate_images);
then, per RDO point, the plain curve's PSNR and MS-SSIM at the same bpp (linear in bpp between the
two neighbouring plain indices) and the difference: positive means RDO is above the plain curve.

    python tools/rdo_rd.py [--out profiles/rdo_rd.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from iclr_17_compression_amd import synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--first", type=int, default=4)
ap.add_argument("--last", type=int, default=16)
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []
LAMBDAS = (0.0, 0.5, 2.0, 8.0, 32.0)
PORTRAIT = (3, 8, 9, 16, 17, 18)


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    lines.append(line)


d = np.load(os.path.join(REPO, "tests", "golden", "g9_weights_n192.npz"))
net = ImageCompressor(out_channel_N=192)
net.load_state_dict({k: torch.from_numpy(d[k].astype(np.float32)) for k in d.files})
net = net.to(dev).eval()
imgs = [np.ascontiguousarray(synth.smooth_image_u8(100 + i, *((768, 512) if i in PORTRAIT
                                                             else (512, 768))).transpose(1, 2, 0))
        for i in range(24)]
g = net.synthesis_gains()
emit({"weights": "g9_weights_n192.npz", "images": "kodak-synth 24", "synthesis_gains": {
    "min": round(float(g.min()), 4), "max": round(float(g.max()), 4),
    "std": round(float(g.std()), 4)}})

curves = {}
for arm in (None,) + LAMBDAS:
    for s in range(args.first, args.last + 1):
        rows = net.evaluate_images(imgs, want_msssim=True, step=s,
                                   **({} if arm is None else {"rdo": arm}))
        point = {"bpp": float(np.mean([r["bpp"] for r in rows])),
                 "psnr_u8": float(np.mean([r["psnr_u8"] for r in rows])),
                 "ms_ssim": float(np.mean([r["ms_ssim"] for r in rows]))}
        curves.setdefault(arm, {})[s] = point
        emit({"arm": "plain" if arm is None else f"rdo={arm:g}", "index": s,
              "bpp": round(point["bpp"], 5), "psnr_u8": round(point["psnr_u8"], 4),
              "ms_ssim": round(point["ms_ssim"], 6)})

plain = sorted(curves[None].values(), key=lambda q: q["bpp"])
xs = [q["bpp"] for q in plain]
for lam in LAMBDAS:
    wins = []
    for s, q in curves[lam].items():
        if not xs[0] <= q["bpp"] <= xs[-1]:
            continue
        at = {k: float(np.interp(q["bpp"], xs, [u[k] for u in plain])) for k in ("psnr_u8", "ms_ssim")}
        row = {"arm": f"rdo={lam:g}", "index": s, "bpp": round(q["bpp"], 5),
               "bpp_saved_vs_plain_same_index": round(curves[None][s]["bpp"] - q["bpp"], 5),
               "psnr_minus_plain_curve_db": round(q["psnr_u8"] - at["psnr_u8"], 4),
               "ms_ssim_minus_plain_curve": round(q["ms_ssim"] - at["ms_ssim"], 6)}
        wins.append(row["psnr_minus_plain_curve_db"])
        emit(row)
    emit({"arm": f"rdo={lam:g}", "summary": "psnr minus the plain curve at equal bpp, over the "
          "indices inside the plain curve's range", "points": len(wins),
          "above": sum(v > 0 for v in wins), "mean_db": round(float(np.mean(wins)), 4),
          "min_db": round(min(wins), 4), "max_db": round(max(wins), 4)})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
