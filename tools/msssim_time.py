"""Cost of MS-SSIM targets (iclr17_image_msssim_u8 in csrc/msssim.hip, codec.py) on
the GPU, in one process, warm, the arms alternating inside every round (diagnostic; needs a GPU).

  kernel    64 uniform 256×256 images: iclr17_image_msssim_u8 (recon fp32 + packed uint8 originals,
            converted as level 0 is read) against iclr17_ms_ssim on a [64,3,256,256] fp32 pair (its
            planes are free), entry points on preallocated buffers, with the bytes each must move.
            With --parent-lib also the same iclr17_ms_ssim call into the library of the commit
            before, loaded beside this one.
  probe     one MS-SSIM probe round of the 64 images at mixed indices (quantise_steps + synthesis +
            image_msssim + one small transfer) against one
            evaluate_images(step=8, want_msssim=True) trial, the unit of the host loop it replaces
            (that path is the parent's, unchanged), and against a PSNR probe round
  compress  compress_images(msssim=T) against compress_images(step=L) at the median index found

    python tools/msssim_time.py [--rounds 30] [--codec-rounds 7] [--parent-lib OLD.so]
                                [--out profiles/msssim_target_ab.txt]
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
ap.add_argument("--parent-lib", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []
N = 192


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


# trained weights: on untrained ones MS-SSIM barely moves along the ladder
d = np.load(os.path.join(REPO, "tests", "golden", "g9_weights_n192.npz"))
net = ImageCompressor(out_channel_N=N)
net.load_state_dict({k: torch.from_numpy(d[k].astype(np.float32)) for k in d.files})
net = net.to(dev).eval()
imgs = [np.ascontiguousarray(synth.smooth_image_u8(300 + k, 256, 256).transpose(1, 2, 0))
        for k in range(64)]
p = kernels._p

with torch.no_grad():
    packed, offsets, shapes = codec.upload_packed(imgs, dev)
    x = kernels.image_ingest(packed, offsets, shapes, (256, 256))
    y = net.latents(x).contiguous()
    B, h, w, _ = y.shape
    st = kernels._stream(y)

    # ------------------------------------------------------------------ the kernel alone
    recon = net.decompress(net.compress_latents(y, 8)["strings"], (h, w), step=8)["x_hat"].contiguous()
    desc = kernels._image_desc("image_msssim", packed.numel(), offsets, shapes, (256, 256)).to(dev)
    nbytes = _lib.query("iclr17_image_msssim_workspace_size", B, 256, 256)
    assert nbytes == _lib.query("iclr17_ms_ssim_workspace_size", B, 256, 256)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    out = torch.empty(B, device=dev, dtype=torch.float32)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    # the planes the existing entry is given for free: what the new one converts to
    dst, _ = kernels.image_egress(recon, offsets, shapes)
    X = (dst.to(dev).view(B, 256, 256, 3).permute(0, 3, 1, 2).float() / 255).contiguous()
    Y = (packed.view(B, 256, 256, 3).permute(0, 3, 1, 2).float() / 255).contiguous()
    one = ctypes.c_float(1.0)
    plane = B * 3 * 256 * 256
    level = [plane // 4 ** l for l in range(5)]                # floats of X (or Y) per level
    # every level is read by its level kernel and (levels 0..3) by the pooling; levels 1..4 are
    # written once; X and Y, fp32
    planes_rw = 2 * 4 * (sum(level[1:]) + sum(level[1:4]) + sum(level[1:]))
    bytes_new = 2 * (4 * plane + plane) + planes_rw            # recon fp32 + bytes, read twice
    bytes_old = 2 * (2 * 4 * plane) + planes_rw                # X and Y fp32, read twice
    karms = {
        "iclr17_image_msssim_u8 (converts in flight)": (lambda: _lib.call(
            "iclr17_image_msssim_u8", p(recon), p(desc), B, 256, 256, p(packed), p(ws), nbytes, p(out),
            p(status), st), bytes_new),
        "iclr17_ms_ssim (fp32 planes given)": (lambda: _lib.call(
            "iclr17_ms_ssim", p(X), p(Y), B, 256, 256, one, p(ws), nbytes, p(out), st), bytes_old)}
    if args.parent_lib:
        old = ctypes.CDLL(args.parent_lib)
        old.iclr17_ms_ssim.restype, old.iclr17_ms_ssim.argtypes = _lib.SIGNATURES["iclr17_ms_ssim"]
        karms["iclr17_ms_ssim of the parent's library"] = (lambda: old.iclr17_ms_ssim(
            p(X), p(Y), B, 256, 256, one, p(ws), nbytes, p(out), st), bytes_old)
    results = {}
    for name, (fn, _) in karms.items():
        fn()
        torch.cuda.synchronize()
        results[name] = out.clone()
    names = list(karms)
    assert torch.equal(results[names[0]], results[names[1]]), "the two entries disagree"
    assert all(torch.equal(results[n], results[names[1]]) for n in names[2:]), "parent's library differs"
    t = alternate({k: v[0] for k, v in karms.items()}, args.rounds)
    for name, (_, nb) in karms.items():
        s = stats(t[name])
        emit({"arm": "kernel", "what": name, "images": B, "size": "256x256", "rounds": args.rounds, **s,
              "bytes": nb, "GB_per_s": round(nb / (s["median_us"] * 1e-6) / 1e9, 1),
              "values_equal": True})

    # ------------------------------------------------------------------ probe round vs a trial
    members, mixed = list(range(B)), [4 + k % 12 for k in range(B)]
    probe = codec.msssim_probe(net, y, packed, offsets, shapes)
    sse_probe = codec.quality_probe(net, y, packed, offsets, shapes)
    trial = net.evaluate_images(imgs, step=8, want_msssim=True)
    assert probe(members, [8] * B) == [r["ms_ssim"] for r in trial]
    parms = {"one MS-SSIM probe round (64 images, mixed indices)": lambda: probe(members, mixed),
             "one PSNR probe round (64 images, mixed indices)": lambda: sse_probe(members, mixed),
             "one evaluate_images(step=8, want_msssim=True) trial":
                 lambda: net.evaluate_images(imgs, step=8, want_msssim=True),
             "one evaluate_images(step=8) trial (no MS-SSIM)": lambda: net.evaluate_images(imgs, step=8)}
    for fn in parms.values():
        fn()
    wall = {}
    t = alternate(parms, args.codec_rounds, wall)
    for name in parms:
        emit({"arm": "probe", "what": name, "images": B, "size": "256x256", "rounds": args.codec_rounds,
              **stats(t[name]), "host_median_ms": round(median(wall[name]), 2)})

    # ------------------------------------------------------------------ compress
    row12 = [r["ms_ssim"] for r in net.evaluate_images(imgs, step=12, want_msssim=True)]
    target = float(np.floor(1000.0 * min(row12)) / 1000.0)     # every image reaches it
    stt = {}
    blobs = net.compress_images(imgs, msssim=target, stats=stt)
    found = [codec.parse_blob(b)[1] for b in blobs]
    s_mid = int(np.median(found))
    carms = {"msssim=T": lambda: net.compress_images(imgs, msssim=target),
             f"step={s_mid} (the median index found)": lambda: net.compress_images(imgs, step=s_mid)}
    for fn in carms.values():
        fn()
    wall = {}
    t = alternate(carms, args.codec_rounds, wall)
    for name in carms:
        emit({"arm": "compress", "what": name, "images": B, "size": "256x256", "target": target,
              "indices_found": [min(found), s_mid, max(found)], "rounds": args.codec_rounds,
              **stats(t[name]), "host_median_ms": round(median(wall[name]), 2),
              "probes_mean": round(float(np.mean(stt["probes"])), 3), "probes_max": max(stt["probes"])})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
