"""Cost of the 8-bit image path (csrc/imageio.hip, codec.py) on the GPU, in one process, arms
alternating inside every round (diagnostic; needs a GPU):

  kernels  iclr17_image_ingest_u8 / iclr17_image_egress_u8 (pixels alone, and with the reference:
           pixels + SSE) against the torch compositions that were the only way to do this work before — the
           expressions of tests/test_gpu_image_io.py, batched, on the same device. HIP-event
           brackets per call; median, p10–p90 and GB/s over the algorithmic 15 bytes per pixel
           (3 uint8 + 3 fp32), and in how many of the alternating pairs the fused kernel lost.
  codec    compress_images + decompress_images on the Kodak-synth set with the G9 weights, in
           Mpix/s of true pixels, beside compress + decompress of the same canvases as fp32
           tensors already on the device (what the parent could do); host clock around a
           synchronise.

Workloads: 64 images of 256×256, and the Kodak-synth set with every image 5 rows and 7 columns
short of its canvas (18 of 507×761 on 512×768, 6 of 763×505 on 768×512), so padding is exercised.

    python tools/image_io_time.py [--rounds 50] [--codec-rounds 5] [--out profiles/image_io_ab.txt]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from iclr_17_compression_amd import _lib, codec, kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=50)
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


def kernel_arms(name, groups):
    """groups: [(B, H, W)] with one true size per group (so the torch arm can batch it)."""
    work = []
    for g, (B, H, W) in enumerate(groups):
        Hc, Wc = codec.canvas(H, W)
        u8 = torch.from_numpy(synth.image_u8(900 + g, B, H, W).reshape(-1)).to(dev)   # B·H·W·3 bytes
        offsets = [3 * H * W * b for b in range(B)]
        desc = torch.tensor([(o, H, W, 0) for o in offsets], dtype=torch.int64, device=dev)
        recon = torch.from_numpy(synth.uniform(910 + g, (B, 3, Hc, Wc), -0.2, 1.2)).to(dev)
        work.append((B, H, W, Hc, Wc, u8, desc, recon))
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = kernels._p

    def fused_ingest():
        for B, H, W, Hc, Wc, u8, desc, _ in work:
            out = torch.empty(B, 3, Hc, Wc, device=dev)
            _lib.call("iclr17_image_ingest_u8", P(u8), P(desc), B, Hc, Wc, P(out), st)

    def torch_ingest():
        for B, H, W, Hc, Wc, u8, _, _ in work:
            F.pad(u8.view(B, H, W, 3).permute(0, 3, 1, 2).float().div(255),
                  (0, Wc - W, 0, Hc - H), mode="replicate")

    def fused_egress(with_ref=True):
        for B, H, W, Hc, Wc, u8, desc, recon in work:
            dst = torch.empty_like(u8)
            sse = torch.empty(B, dtype=torch.int64, device=dev)
            status = torch.empty(1, dtype=torch.int32, device=dev)
            _lib.call("iclr17_image_egress_u8", P(recon), P(desc), B, Hc, Wc, P(dst),
                      P(u8) if with_ref else None, P(sse) if with_ref else None, P(status), st)

    def torch_egress(with_ref=True):
        for B, H, W, Hc, Wc, u8, _, recon in work:
            dst = torch.round(recon.clamp(0, 1) * 255).to(torch.uint8)[:, :, :H, :W]
            dst = dst.permute(0, 2, 3, 1).contiguous()
            (~torch.isfinite(recon[:, :, :H, :W])).any()
            if with_ref:
                ((dst.long() - u8.view(B, H, W, 3).long()) ** 2).sum((1, 2, 3))

    pixels = sum(B * H * W for B, H, W in groups)
    for what, fused, composed in (("ingest", fused_ingest, torch_ingest),
                                  ("egress", lambda: fused_egress(False), lambda: torch_egress(False)),
                                  ("egress+sse", fused_egress, torch_egress)):
        t = {"fused": [], "torch": []}
        for r in range(args.rounds + 5):
            a, b = timed(fused), timed(composed)
            if r >= 5:
                t["fused"].append(a)
                t["torch"].append(b)
        lost = sum(a > b for a, b in zip(t["fused"], t["torch"]))
        for arm in ("fused", "torch"):
            s = stats(t[arm])
            emit({"workload": name, "kernel": what, "arm": arm, **s, "pixels": pixels,
                  "GBps_15B_per_pixel": round(15 * pixels / (s["median_us"] * 1e-6) / 1e9, 1),
                  "rounds": args.rounds, "launch_groups": len(groups)})
        emit({"workload": name, "kernel": what, "fused_slower_in_pairs": lost, "pairs": args.rounds})


def codec_arms():
    d = np.load(os.path.join(REPO, "tests", "golden", "g9_weights_n192.npz"))
    net = ImageCompressor(out_channel_N=192)
    net.load_state_dict({k: torch.from_numpy(d[k].astype(np.float32)) for k in d.files})
    net = net.to(dev).eval()
    sizes = [(763, 505) if i in (3, 8, 9, 16, 17, 18) else (507, 761) for i in range(24)]
    imgs = [np.ascontiguousarray(synth.smooth_image_u8(100 + i, H, W).transpose(1, 2, 0))
            for i, (H, W) in enumerate(sizes)]
    tensors = []
    for idx in codec.group_by_canvas(sizes, 64):
        packed, offsets, shapes = codec.upload_packed([imgs[i] for i in idx], dev)
        tensors.append(kernels.image_ingest(packed, offsets, shapes, codec.canvas(*shapes[0])))
    true_px = sum(H * W for H, W in sizes)
    canvas_px = sum(t.shape[0] * t.shape[2] * t.shape[3] for t in tensors)

    def images_path():
        return net.decompress_images(net.compress_images(imgs))

    def tensor_path():
        for x in tensors:
            enc = net.compress(x)
            net.decompress(enc["strings"], enc["shape"])["x_hat"]

    t = {"images": [], "tensors": []}
    for r in range(args.codec_rounds + 2):
        for arm, fn in (("images", images_path), ("tensors", tensor_path)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                t[arm].append(time.perf_counter() - t0)
    for arm, px, note in (("images", true_px, "compress_images + decompress_images: uint8 files in, uint8 out"),
                          ("tensors", canvas_px, "compress + decompress of the padded fp32 batches on the device")):
        s = sorted(t[arm])
        med = s[len(s) // 2]
        emit({"workload": "kodak-synth 18x507x761 + 6x763x505, G9 weights", "path": arm, "what": note,
              "precision": kernels.precision(), "median_ms": round(1e3 * med, 2),
              "min_ms": round(1e3 * s[0], 2), "max_ms": round(1e3 * s[-1], 2), "pixels": px,
              "Mpix_per_s": round(px / med / 1e6, 2), "rounds": args.codec_rounds})


emit({"device": torch.cuda.get_device_name(0), "torch": torch.__version__})
kernel_arms("64 x 256x256", [(64, 256, 256)])
kernel_arms("kodak-synth 18 x 507x761 + 6 x 763x505", [(18, 507, 761), (6, 763, 505)])
codec_arms()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
