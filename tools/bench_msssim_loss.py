"""Times the differentiable MS-SSIM (losses.ms_ssim_diff, forward + backward) against the same
function composed of plain torch ops on the GPU (the reference's algorithm: depthwise conv2d,
avg_pool2d, pow, prod, differentiated by torch autograd), and an "ms-ssim" training step against
an "mse" one. Device events, warm-up, the two of each pair alternated in one process; prints one
JSON line. Only the image gradient that a training step needs (dX of the reconstruction) is asked.

    python tools/bench_msssim_loss.py [--batch 32] [--size 256] [--N 192] [--reps 30]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iclr_17_compression_amd import kernels, synth  # noqa: E402
from iclr_17_compression_amd.losses import ms_ssim_diff  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gauss(dev):
    t = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-(t ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dev)


def torch_ms_ssim(X, Y, g, w):
    """models/ms_ssim_torch.py:123-196 in torch ops, per image."""
    kw = g.reshape(1, 1, 1, -1).repeat(3, 1, 1, 1)
    kh = kw.transpose(2, 3)
    blur = lambda z: F.conv2d(F.conv2d(z, kw, groups=3), kh, groups=3)  # noqa: E731
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mcs, s = [], None
    for _ in range(5):
        mx, my = blur(X), blur(Y)
        mxx, myy, mxy = mx.pow(2), my.pow(2), mx * my
        vx, vy, cxy = blur(X * X) - mxx, blur(Y * Y) - myy, blur(X * Y) - mxy
        cs_map = (2 * cxy + c2) / (vx + vy + c2)
        s = (((2 * mxy + c1) / (mxx + myy + c1)) * cs_map).mean((1, 2, 3))
        mcs.append(cs_map.mean((1, 2, 3)))
        pad = (X.shape[2] % 2, X.shape[3] % 2)
        X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    mcs = torch.stack(mcs, dim=0)
    return torch.prod((mcs[:-1] ** w[:-1].unsqueeze(1)) * (s ** w[-1]), dim=0)


def timed(runs, reps, warmup):
    for k in runs:
        for _ in range(warmup):
            runs[k]()
    torch.cuda.synchronize()
    ev = {k: [] for k in runs}
    for _ in range(reps):
        for k in runs:   # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runs[k]()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for k in runs:
        ms = sorted(a.elapsed_time(b) for a, b in ev[k])
        out[k] = {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--N", type=int, default=192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_msssim_loss: needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(7, B, S, S))).to(dev)
    n = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    y = (x + 0.1 * n).clamp(0, 1)
    g, w = gauss(dev), torch.tensor(WEIGHTS, device=dev)

    def fused():
        Y = y.detach().requires_grad_(True)
        (1 - ms_ssim_diff(Y, x)).backward()
        return Y.grad

    def composed():
        Y = y.detach().requires_grad_(True)
        (1 - torch_ms_ssim(Y, x, g, w).mean()).backward()
        return Y.grad

    ga, gb = fused(), composed()
    agree = ((ga - gb).abs().max() / gb.abs().max()).item()
    res = {"loss_fwd_bwd": timed({"fused": fused, "torch_ops": composed}, a.reps, a.warmup)}

    net = ImageCompressor(out_channel_N=a.N)
    net.load_state_dict({k: torch.from_numpy(v)
                         for k, v in synth.trained_like_state_dict(a.N, 1).items()})
    net = net.to(dev).train()
    noise = torch.from_numpy(synth.uniform(4, (B, a.N, S // 16, S // 16), -0.5, 0.5)).to(dev)

    def step(distortion, lam):
        def run():
            net.zero_grad(set_to_none=True)
            _, d, bpp = net.forward_train(x, noise=noise, distortion=distortion)
            (lam * d + bpp).backward()
        return run

    res["train_step"] = timed({"ms-ssim": step("ms-ssim", 100.0), "mse": step("mse", 8192.0)},
                              a.reps, a.warmup)
    print(json.dumps({"tool": "bench_msssim_loss", "device": torch.cuda.get_device_name(0),
                      "precision": kernels.precision(), "batch": B, "size": S, "N": a.N,
                      "reps": a.reps, "grad_rel_diff_fused_vs_torch_ops": agree, **res}))


if __name__ == "__main__":
    main()
