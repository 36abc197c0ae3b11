"""Cost of latent refinement's pieces (diagnostic, needs a GPU): 64 images of
256×256, N = 192, synthetic weights, one process, warm, the arms of a round in rotating order, HIP
events around each arm, medians with p10–p90.

Per iteration: the training forward of the synthesis; its data gradient alone
(autograd.synthesis_latent_grad) against the full backward with the weight gradients
(autograd.synthesis_backward); the fused latent kernel (kernels.refine_step) against the sequence
of existing kernels it replaces (step_noise_rate_bwd for the rate derivative, adam_step,
quantise_steps, and step_noise_rate with zero noise as the per-image rate pass); the two small
kernels; for the MS-SSIM objective kernels.image_msssim_fwd_saved and
kernels.image_msssim_bwd against the Uniform pair on ready fp32 planes of the same size and against
the squared-error pair image_sse_device + refine_grad_recon. Then
``compress_images(step=8, refine=K)`` for K = 0, 5, 20 and both objectives, wall clock.

    python tools/refine_time.py [--rounds 15] [--precision h3] [--out profiles/refine_msssim_ab.txt]
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
from iclr_17_compression_amd import _lib, autograd, chain, codec, kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--precision", default=None, choices=("h3", "x6", "fp32"))
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
N, B, LAM = 192, 64, 650.25
mode = args.precision or kernels.precision()
lines = []


def emit(row):
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    s = sorted(ts)
    return {"median_ms": round(s[len(s) // 2], 4), "p10_ms": round(s[len(s) // 10], 4),
            "p90_ms": round(s[(9 * len(s)) // 10], 4)}


net = ImageCompressor(out_channel_N=N)
net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
net = net.to(dev).eval()
imgs = [np.ascontiguousarray(synth.smooth_image_u8(300 + k, 256, 256).transpose(1, 2, 0))
        for k in range(B)]

with torch.no_grad(), kernels.precision_scope(mode):
    packed, offsets, shapes = codec.upload_packed(imgs, dev)
    x = kernels.image_ingest(packed, offsets, shapes, (256, 256))
    y = net.latents(x).contiguous()
    _, h, w, _ = y.shape
    desc = kernels._image_desc("refine", packed.numel(), offsets, shapes, (256, 256)).to(dev)
    steps_dev = torch.full((B,), codec.step_size(8), device=dev)
    lam = torch.full((B,), LAM, device=dev, dtype=torch.float64)
    wt = (lam / 3.0).float()
    net._warm_packs(backward=True, mode=mode)
    net._warm_packs(mode=mode)
    m = chain.train_mode(mode)
    dec, pack = net.Decoder, net.bitEstimator.packed()
    y_hat, y_deq = kernels.quantise_steps(y, steps_dev)
    _, recon, _, saved = m.train_synthesis(dec, y_deq, None, None)
    g_recon = kernels.refine_grad_recon(recon, packed, desc, wt)
    g_y = autograd.synthesis_latent_grad(dec, saved, g_recon, mode=m.name).contiguous()
    full = autograd.synthesis_backward(dec, saved, g_recon, mode=m.name)[0]
    emit({"setup": f"{B} x 256x256, N={N}, precision {mode}, rounds {args.rounds}",
          "latent_grad_equals_full_backward": bool(torch.equal(g_y, full))})

    yy, mom, var = y.clone(), torch.zeros_like(y), torch.zeros_like(y)
    qh, qd, qd2 = y_hat.clone(), y_deq.clone(), torch.empty_like(y)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    status1 = torch.zeros(1, device=dev, dtype=torch.int32)
    partial = kernels.refine_bits_partials(y)
    ones = torch.ones(B, device=dev)
    zero_noise = torch.zeros(B, N, h, w, device=dev)
    g_buf = torch.empty_like(y)
    T = _lib.query("iclr17_step_rate_bwd_partials", h, w)
    rpart = torch.empty(B * T, 11, N, device=dev)
    adam_desc = torch.tensor([[yy.data_ptr(), g_buf.data_ptr(), mom.data_ptr(), var.data_ptr(),
                               yy.numel()]], dtype=torch.int64, device=dev)
    p, call, st = kernels._p, _lib.call, kernels._stream(y)
    best = torch.zeros_like(y)
    bJ = torch.full((B,), float("inf"), device=dev, dtype=torch.float64)
    bi = torch.zeros(B, device=dev, dtype=torch.int32)
    bb, bs = torch.zeros(B, device=dev, dtype=torch.float64), torch.zeros(B, device=dev, dtype=torch.int64)
    flag = torch.zeros(B, device=dev, dtype=torch.int32)
    bits = torch.rand(B, device=dev, dtype=torch.float64)
    sse = torch.ones(B, device=dev, dtype=torch.int64)

    def unfused():
        call("iclr17_step_noise_rate_bwd", p(qh), p(g_y), B, h, w, N, p(steps_dev), p(pack), p(ones),
             p(g_buf), p(rpart), st)
        call("iclr17_adam_step", p(adam_desc), 1, yy.numel(), ctypes.c_double(0.05),
             ctypes.c_double(0.9), ctypes.c_double(0.999), ctypes.c_double(1e-8), 1,
             ctypes.c_float(0.0), st)
        call("iclr17_quantise_steps", p(yy), B, yy.numel() // B, p(steps_dev), p(qh), p(qd),
             p(status1), st)
        call("iclr17_step_noise_rate", p(qd), p(zero_noise), B, h, w, N, p(steps_dev), p(pack),
             p(g_buf), p(qd2), p(partial), st)

    def keep():
        bJ.fill_(float("inf"))
        kernels.refine_keep(bits, sse, lam, status, None, qh, 1, bJ, bi, bb, bs, best, flag)

    # the MS-SSIM objective: the canvas pair against the Uniform pair on ready
    # fp32 planes of the same size (what ragged extents and the 8-bit conversion cost) and against
    # the SSE pair image_sse_device + refine_grad_recon (what an iteration gains in cost)
    ms_ws = kernels.image_msssim_grad_workspace(B, 256, 256, dev)
    ms_out = (torch.empty(B, device=dev), torch.empty(1, device=dev, dtype=torch.int32))
    ms_g = torch.full((B,), -8.0 * 256 * 256, device=dev)
    recon = recon.contiguous()
    ms_d = torch.empty_like(recon)
    X = (torch.round(recon.clamp(0, 1) * 255) / 255).contiguous()
    Y = x.contiguous()
    uni_ws = [None]

    def uniform_fwd():
        _, uni_ws[0] = kernels.ms_ssim_fwd_saved(X, Y, want_dy=False)

    arms = {
        "image_msssim_fwd_saved": lambda: kernels.image_msssim_fwd_saved(recon, packed, desc, ms_ws, ms_out),
        "image_msssim_bwd": lambda: kernels.image_msssim_bwd(recon, packed, desc, ms_ws, ms_g, ms_d),
        "ms_ssim_fwd_saved (ready fp32 planes, no dY)": uniform_fwd,
        "ms_ssim_bwd (ready fp32 planes, dx only)": lambda: kernels.ms_ssim_bwd(
            X, Y, uni_ws[0], ms_g, saved_dy=False, want_dy=False),
        "train_synthesis (forward)": lambda: m.train_synthesis(dec, y_deq, None, None),
        "synthesis_latent_grad": lambda: autograd.synthesis_latent_grad(dec, saved, g_recon, mode=m.name),
        "synthesis_backward (full)": lambda: autograd.synthesis_backward(dec, saved, g_recon, mode=m.name),
        "refine_step (fused)": lambda: kernels.refine_step(yy, steps_dev, pack, qh, qd, status, partial,
                                                           g_deq=g_y, m=mom, v=var, lr=0.05, t=1),
        "unfused: rate_bwd + adam + quantise + rate": unfused,
        "refine_step (iteration 0)": lambda: kernels.refine_step(yy, steps_dev, pack, qh, qd, status,
                                                                 partial),
        "refine_grad_recon": lambda: kernels.refine_grad_recon(recon, packed, desc, wt),
        "image_sse_device": lambda: kernels.image_sse_device(recon, None, None, packed, desc),
        "refine_keep (all kept)": keep,
    }
    names = list(arms)
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {name: [] for name in names}
    for r in range(args.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            t[name].append(timed(arms[name]))
    for name in names:
        emit({"arm": name, **stats(t[name])})
    med = {name: stats(t[name])["median_ms"] for name in names}
    emit({"saved_by_dropping_weight_gradients_ms":
          round(med["synthesis_backward (full)"] - med["synthesis_latent_grad"], 4),
          "fused_over_unfused": round(med["refine_step (fused)"]
                                      / med["unfused: rate_bwd + adam + quantise + rate"], 4)})
    emit({"msssim_pair_ms": round(med["image_msssim_fwd_saved"] + med["image_msssim_bwd"], 4),
          "uniform_pair_on_ready_planes_ms":
          round(med["ms_ssim_fwd_saved (ready fp32 planes, no dY)"]
                + med["ms_ssim_bwd (ready fp32 planes, dx only)"], 4),
          "sse_pair_ms": round(med["image_sse_device"] + med["refine_grad_recon"], 4)})

    for what, lam_of in (("mse", LAM), ("ms-ssim", codec.msssim_lambda(8.0))):
        for K in (0, 5, 20):
            if K == 0 and what != "mse":
                continue
            net.compress_images(imgs, step=8, refine=K, refine_lambda=lam_of)
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                net.compress_images(imgs, step=8, refine=K, refine_lambda=lam_of)
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            emit({"compress_images": f"step=8, refine={K}, {what}",
                  "wall_ms": [round(v, 2) for v in sorted(ts)]})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
