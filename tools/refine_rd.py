"""Rate–distortion effect of latent refinement on trained weights (diagnostic, needs
a GPU): tests/golden/g9_weights_n192.npz on the synthetic Kodak-24 set, ladder indices 4…16,
K in 0, 5, 20, 100 iterations with λ = 650.25/Δ² (the checkpoint's λ where the latent distortion of
the quantiser scales as it does at Δ = 1). Real blobs through ``evaluate_images``: per arm and index
the means over the 24 images of bpp, psnr_u8 and MS-SSIM and how many images kept a refined
latent; then, per refined point, the plain curve's PSNR and MS-SSIM at the same bpp (linear in bpp
between the two neighbouring plain indices) and the difference: positive means above the plain
curve.

First a small sweep chooses the learning rate (``refine_lr``, in units of Δ): index 8, K = 20, the
first six images, the candidate with the lowest mean objective relative to the plain one. The
table is then made with that value, and it is what codec.DEFAULT_REFINE_LR records.

``--distortion ms-ssim`` refines for bits + λ·H·W·(1 − MS-SSIM) with λ = L/Δ². The
sweep then chooses L and the learning rate together, on the same six images at index 8 with K = 20:
the pair whose refined point lies highest above those images' own plain curve in MS-SSIM at equal
bpp (objectives under different λ do not compare). The table is made as above.

    python tools/refine_rd.py [--out profiles/refine_rd.txt] [--first 4] [--last 16]
                              [--iters 0,5,20,100] [--lr R]
                              [--distortion ms-ssim [--lam L] [--lam-sweep 4,16,64,256]]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from iclr_17_compression_amd import codec, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--first", type=int, default=4)
ap.add_argument("--last", type=int, default=16)
ap.add_argument("--iters", default="0,5,20,100")
ap.add_argument("--lr", type=float, default=None, help="skip the sweep and use this value")
ap.add_argument("--sweep", default="0.001,0.003,0.01,0.03,0.1")
ap.add_argument("--distortion", choices=codec.REFINE_DISTORTIONS, default="mse",
                help="ms-ssim: the objective of DESIGN.md §0o, λ = L/Δ² with L from --lam-sweep")
ap.add_argument("--lam", type=float, default=None, help="ms-ssim: skip the sweep and use this L")
ap.add_argument("--lam-sweep", default="4,16,64,256")
args = ap.parse_args()
dev = torch.device("cuda:0")
ITERS = [int(v) for v in args.iters.split(",")]
LAMBDA = 650.25
MSSSIM = args.distortion == "ms-ssim"
PORTRAIT = (3, 8, 9, 16, 17, 18)
out = open(args.out, "w") if args.out else None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def lam_of(s):
    if MSSSIM:   # 1 − MS-SSIM of the quantiser's error scales with Δ² as the squared error does
        return codec.msssim_lambda(LAMBDA / codec.step_size(s) ** 2)
    return LAMBDA / codec.step_size(s) ** 2


d = np.load(os.path.join(REPO, "tests", "golden", "g9_weights_n192.npz"))
net = ImageCompressor(out_channel_N=192)
net.load_state_dict({k: torch.from_numpy(d[k].astype(np.float32)) for k in d.files})
net = net.to(dev).eval()
imgs = [np.ascontiguousarray(synth.smooth_image_u8(100 + i, *((768, 512) if i in PORTRAIT
                                                             else (512, 768))).transpose(1, 2, 0))
        for i in range(24)]
emit({"weights": "g9_weights_n192.npz", "images": "kodak-synth 24", "distortion": args.distortion,
      "lambda": "L / step^2 (L: the sweep below)" if MSSSIM else "650.25 / step^2", "iters": ITERS})

lr = args.lr
if MSSSIM:
    # λ and the learning rate together: index 8, K = 20, the first six images; the pair whose
    # refined point lies highest above those six images' own plain curve in MS-SSIM at equal bpp
    # (objectives under different λ do not compare)
    near = [net.evaluate_images(imgs[:6], want_msssim=True, step=s) for s in range(5, 12)]
    px = [float(np.mean([r["bpp"] for r in rows])) for rows in near][::-1]
    pm = [float(np.mean([r["ms_ssim"] for r in rows])) for rows in near][::-1]
    lams = [args.lam] if args.lam is not None else [float(v) for v in args.lam_sweep.split(",")]
    lrs = [lr] if lr is not None else [float(v) for v in args.sweep.split(",")]
    best = None
    for L in lams:
        for cand in lrs:
            rows = net.evaluate_images(imgs[:6], want_msssim=True, step=8, refine=20,
                                       refine_lambda=codec.msssim_lambda(L), refine_lr=cand)
            bpp = float(np.mean([r["bpp"] for r in rows]))
            ms = float(np.mean([r["ms_ssim"] for r in rows]))
            gain = ms - float(np.interp(bpp, px, pm))
            emit({"lambda_sweep": L, "lr_sweep": cand, "index": 8, "iters": 20, "images": 6,
                  "kept": sum(r["refine_kept"] > 0 for r in rows), "bpp": round(bpp, 5),
                  "ms_ssim": round(ms, 6), "ms_ssim_minus_plain_curve": round(gain, 6),
                  "psnr_u8": round(float(np.mean([r["psnr_u8"] for r in rows])), 4),
                  "mean_objective_over_plain": round(float(np.mean(
                      [r["objective"] / r["objective_plain"] for r in rows])), 6)})
            if px[0] <= bpp <= px[-1] and (best is None or gain > best[0]):
                best = (gain, L, cand)
    if best is None:
        sys.exit("no candidate landed inside the plain curve of indices 5..11")
    LAMBDA, lr = best[1], best[2]
    emit({"lambda_at_index_8": LAMBDA})
elif lr is None:
    best = None
    for cand in (float(v) for v in args.sweep.split(",")):
        rows = net.evaluate_images(imgs[:6], step=8, refine=20, refine_lambda=lam_of(8),
                                   refine_lr=cand)
        rel = float(np.mean([r["objective"] / r["objective_plain"] for r in rows]))
        emit({"lr_sweep": cand, "index": 8, "iters": 20, "images": 6,
              "mean_objective_over_plain": round(rel, 6),
              "kept": sum(r["refine_kept"] > 0 for r in rows),
              "bpp": round(float(np.mean([r["bpp"] for r in rows])), 5),
              "psnr_u8": round(float(np.mean([r["psnr_u8"] for r in rows])), 4)})
        if best is None or rel < best[0]:
            best = (rel, cand)
    lr = best[1]
emit({"refine_lr": lr, "default_in_codec_at_this_run": codec.DEFAULT_REFINE_LR})

curves = {}
for K in ITERS:
    for s in range(args.first, args.last + 1):
        rows = net.evaluate_images(imgs, want_msssim=True, step=s, refine=K,
                                   refine_lambda=lam_of(s), refine_lr=lr)
        point = {"bpp": float(np.mean([r["bpp"] for r in rows])),
                 "psnr_u8": float(np.mean([r["psnr_u8"] for r in rows])),
                 "ms_ssim": float(np.mean([r["ms_ssim"] for r in rows]))}
        curves.setdefault(K, {})[s] = point
        extra = {}
        if K:
            extra = {"kept": sum(r["refine_kept"] > 0 for r in rows),
                     "mean_objective_over_plain": round(float(np.mean(
                         [r["objective"] / r["objective_plain"] for r in rows])), 6)}
        emit({"arm": f"refine={K}", "index": s, "bpp": round(point["bpp"], 5),
              "psnr_u8": round(point["psnr_u8"], 4), "ms_ssim": round(point["ms_ssim"], 6), **extra})

if 0 in curves:
    plain = sorted(curves[0].values(), key=lambda q: q["bpp"])
    xs = [q["bpp"] for q in plain]
    for K in ITERS:
        if not K:
            continue
        wins, wins_ms = [], []
        for s, q in curves[K].items():
            if not xs[0] <= q["bpp"] <= xs[-1]:
                continue
            at = {k: float(np.interp(q["bpp"], xs, [u[k] for u in plain]))
                  for k in ("psnr_u8", "ms_ssim")}
            row = {"arm": f"refine={K}", "index": s, "bpp": round(q["bpp"], 5),
                   "bpp_saved_vs_plain_same_index": round(curves[0][s]["bpp"] - q["bpp"], 5),
                   "plain_curve_psnr_at_bpp": round(at["psnr_u8"], 4),
                   "psnr_minus_plain_curve_db": round(q["psnr_u8"] - at["psnr_u8"], 4),
                   "plain_curve_ms_ssim_at_bpp": round(at["ms_ssim"], 6),
                   "ms_ssim_minus_plain_curve": round(q["ms_ssim"] - at["ms_ssim"], 6)}
            wins.append(row["psnr_minus_plain_curve_db"])
            wins_ms.append(row["ms_ssim_minus_plain_curve"])
            emit(row)
        if wins:
            emit({"arm": f"refine={K}", "summary": "psnr minus the plain curve at equal bpp, over "
                  "the indices inside the plain curve's range", "points": len(wins),
                  "above": sum(v > 0 for v in wins), "mean_db": round(float(np.mean(wins)), 4),
                  "min_db": round(min(wins), 4), "max_db": round(max(wins), 4),
                  "mean_ms_ssim_diff": round(float(np.mean(wins_ms)), 6),
                  **({"ms_ssim_above": sum(v > 0 for v in wins_ms),
                      "min_ms_ssim_diff": round(min(wins_ms), 6),
                      "max_ms_ssim_diff": round(max(wins_ms), 6)} if MSSSIM else {})})
if out:
    out.close()
