#!/usr/bin/env python3
"""Throughput bench of the Ballé-2017 codec hot path on MI355X (BASELINE.json metric).

One step = encode+decode of one batch of synthetic 256×256×3 images per GPU, N = 192:
    conv1+GDN → conv2+GDN → conv3+round+rate → deconv1+IGDN → deconv2+IGDN → deconv3+clamp
    → deterministic per-batch bit reduction (bpp)
with inputs already resident in HBM. Images shard by batch across ranks (no collective in the
data path; "weak" scaling). Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the line. --full adds what the
headline does not need (the bf16 and x6 legs, the per-layer pass and its roofline, the CPU
baseline); --dump-outputs DIR writes the last timed step's results as DIR/<name>.npy.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--full] [--dump-outputs DIR]
    torchrun --nproc-per-node N bench.py --gpus N ...
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import platform
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from iclr_17_compression_amd import kernels, synth  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

METRIC = "Mpixels/s encode+decode at 1/2/4/8 GPU; bpp & PSNR parity on Kodak"
FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 dense peak
BF16_MFMA_PEAK_TFLOPS = 2516.6  # 256 CU x 4 SIMD x 1024 FLOP/clk (16x16x32 bf16, 16 cyc) x 2.4 GHz
X6_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 6   # fp32-equivalent: 6 bf16 part products per MAC
X6_LAYERS = ("conv1_gdn1", "conv2_gdn2", "conv3_quant_rate", "deconv1_igdn1", "deconv2_igdn2",
             "deconv3_clamp")   # every contraction of the x6 eval chain
H3_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 3   # fp32-equivalent: 3 fp16 part products per MAC
# the layers of the h3 eval chain whose contractions run in the h3 form (all of them)
H3_LAYERS = ("conv1_gdn1", "conv2_gdn2", "conv3_quant_rate", "deconv1_igdn1", "deconv2_igdn2",
             "deconv3_clamp")


# the JSON line's "dtype": the arithmetic the contractions compute in (every mode accumulates in
# fp32; the epilogues — GDN square roots, quantiser, rate — are fp32)
DTYPE = {"h3": "h3", "x6": "f32", "fp32": "f32", "bf16": "bf16"}
DTYPE_NOTE = {
    "h3": "h3: fp32 operands rounded to 22 significant bits (two fp16 parts), fp32 accumulate",
    "x6": "f32: fp32 operands split exactly (24 significant bits) into three bf16 parts, fp32 accumulate",
    "fp32": "f32: exact-f32 MFMA products",
    "bf16": "bf16 operands, fp32 accumulate",
}

PRECISION_NOTE = {
    "h3": ("h3: fp32 operands as two fp16 parts (22 significant bits, power-of-two scaled), 3 part "
           "products per MAC on v_mfma_f32_*_f16 with fp32 accumulate for every convolution and "
           "GDN contraction"),
    "x6": ("x6: fp32 operands split exactly into 3 bf16 parts, 6 part products on "
           "v_mfma_f32_16x16x32_bf16, fp32 accumulate (every contraction)"),
    "bf16": "bf16: bf16 activations and weights, one bf16 product per MAC, fp32 accumulate and epilogues",
    "fp32": "fp32 (exact-f32 MFMA products)",
}


def layer_peak(prec: str, k: str):
    """(peak TFLOP/s, basis) of layer k's main contraction in precision mode prec."""
    if prec == "bf16":
        return BF16_MFMA_PEAK_TFLOPS, "bf16 dense MFMA peak (one bf16 product per MAC)"
    if prec == "h3" and k in H3_LAYERS:
        return H3_PEAK_TFLOPS, "bf16/f16 dense MFMA peak / 3 (h3: three fp16 part products per fp32 MAC)"
    if prec in ("x6", "h3") and k in X6_LAYERS:
        return X6_PEAK_TFLOPS, "bf16 dense MFMA peak / 6 (bf16x6: six bf16 part products per fp32 MAC)"
    return FP32_MFMA_PEAK_TFLOPS, "fp32 MFMA dense peak (exact-f32 products)"
HBM_PEAK_GBS = 8000.0

LAYERS = ("conv1_gdn1", "conv2_gdn2", "conv3_quant_rate", "deconv1_igdn1", "deconv2_igdn2",
          "deconv3_clamp", "bits_reduce")


def layer_flops(N: int, H: int, W: int) -> dict:
    """Algorithmic FLOPs per image (2·MAC) of each fused kernel."""
    h1, w1, h2, w2, h3, w3 = H // 4, W // 4, H // 8, W // 8, H // 16, W // 16
    mac = {
        "conv1_gdn1": h1 * w1 * N * 3 * 81 + h1 * w1 * N * N,
        "conv2_gdn2": h2 * w2 * N * N * 25 + h2 * w2 * N * N,
        "conv3_quant_rate": h3 * w3 * N * N * 25,
        "deconv1_igdn1": h3 * w3 * N * N * 25 + h2 * w2 * N * N,
        "deconv2_igdn2": h2 * w2 * N * N * 25 + h1 * w1 * N * N,
        "deconv3_clamp": h1 * w1 * N * 3 * 81,
        "bits_reduce": 0,
    }
    return {k: 2.0 * v for k, v in mac.items()}


def layer_bytes(N: int, H: int, W: int, act: int = 4) -> dict:
    """Algorithmic HBM bytes per image of each fused kernel (NHWC activations of `act` bytes per
    element — fp32 4, the bf16 mode 2 — read once and written once, the fp32 image and
    reconstruction; weights amortised over the batch and ignored)."""
    h1, w1, h2, w2, h3, w3 = H // 4, W // 4, H // 8, W // 8, H // 16, W // 16
    f = 4
    return {
        "conv1_gdn1": f * 3 * H * W + act * h1 * w1 * N,
        "conv2_gdn2": act * (h1 * w1 * N + h2 * w2 * N),
        "conv3_quant_rate": act * (h2 * w2 * N + h3 * w3 * N),
        "deconv1_igdn1": act * (h3 * w3 * N + h2 * w2 * N),
        "deconv2_igdn2": act * (h2 * w2 * N + h1 * w1 * N),
        "deconv3_clamp": act * h1 * w1 * N + f * 3 * H * W,
        "bits_reduce": 0,
    }


class Step:
    """The fused forward of ImageCompressor.forward (model.py:47-80), layer by layer, with
    optional HIP-event brackets on the launching stream for per-kernel timing."""

    def __init__(self, net: ImageCompressor, x: torch.Tensor):
        self.net, self.x = net, x
        B, _, H, W = x.shape
        self.scale = 1.0 / (B * H * W)
        self.N = net.out_channel_N
        self.enc = net.Encoder.packed()
        self.dec = net.Decoder.packed()
        self.d3x6 = net.Decoder.packed_x6()
        self.dh3 = net.Decoder.packed_h3k()
        self.eh3 = net.Encoder.packed_h3()
        self.w1h3 = net.Encoder.packed_conv1_h3()
        self.eg3 = [net.Encoder.gdn1.effective_params_h3(), net.Encoder.gdn2.effective_params_h3()]
        self.gh3 = [net.Decoder.igdn1.effective_params_h3(), net.Decoder.igdn2.effective_params_h3()]
        self.rate = net.bitEstimator.packed()
        gdns = (net.Encoder.gdn1, net.Encoder.gdn2, net.Decoder.igdn1, net.Decoder.igdn2)
        self.w1x6 = net.Encoder.packed_conv1_x6()
        self.w3s = net.Encoder.packed_w3_split()   # x6 conv3's pre-split weights
        self.g6 = [m.effective_params_x6() for m in gdns]
        self.ebf = net.Encoder.packed_bf16()
        self.dbf = net.Decoder.packed_bf16()
        self.gbf = [m.effective_params_bf16() for m in gdns]
        self.rtab = net.bitEstimator.rate_table()

    def __call__(self, events=None):
        for _ in self.layers(events):
            pass
        return self.out

    def layers(self, events=None):
        """The step as a generator: yields after each layer's launch (SplitStep interleaves the
        batch parts layer by layer); the outputs land in self.out."""
        net, N = self.net, self.N
        w1, w2, w3, g1, g2 = self.enc
        d1, d2, d3, q1, q2 = self.dec
        ev = (lambda i: events[i].record()) if events is not None else (lambda i: None)
        ev(0)
        if kernels.precision() == "bf16":
            (w1b, w2b, w3b), (d1b, d2b, d3b), (e1, e2, e3, e4) = self.ebf, self.dbf, self.gbf
            h = kernels.conv1_gdn_bf16(self.x, w1b, net.Encoder.conv1.bias, *e1, N)
            ev(1)
            yield
            h = kernels.conv2_gdn_bf16(h, w2b, net.Encoder.conv2.bias, *e2)
            ev(2)
            yield
            y_hat, partial, _, ybf = kernels.conv3_quant_rate_bf16(h, w3b, self.rate, self.rtab)
            ev(3)
            yield
            h = kernels.deconv_igdn_bf16(ybf, d1b, net.Decoder.deconv1.bias, *e3)
            ev(4)
            yield
            h = kernels.deconv_igdn_bf16(h, d2b, net.Decoder.deconv2.bias, *e4)
            ev(5)
            yield
            # bpp's reduction (model.py:71-78) inside deconv3's kernel (ImageCompressor.forward)
            clipped, _, _, bpp = kernels.deconv3_bf16(h, d3b, net.Decoder.deconv3.bias,
                                                      bits=(partial, self.scale))
        elif kernels.precision() == "h3":
            # ImageCompressor.forward in the h3 form: every layer (and GDN contraction) on three
            # fp16 part products per MAC; the chain's range flag cleared first (deconv3 makes the
            # results NaN when a value did not fit the form)
            kernels.h3_chain_begin(self.x.device)
            e1, e2 = self.eg3
            (w2h, w3h), (x1, x2, x3) = self.eh3, self.dh3
            hs, _ = kernels.conv1_gdn_h3(self.x, self.w1h3, net.Encoder.conv1.bias, *e1, N)
            ev(1)
            yield
            hs, _, _ = kernels.conv2_gdn_h3(hs, w2h, net.Encoder.conv2.bias, *e2)
            ev(2)
            yield
            y_hat, partial, _, yh = kernels.conv3_quant_rate_h3(hs, w3h, self.rate, rtab=self.rtab)
            ev(3)
            yield
            h3, h4 = self.gh3
            hs, _, _ = kernels.deconv_igdn_h3(yh, x1, net.Decoder.deconv1.bias, *h3, int_in=True)
            ev(4)
            yield
            hs, _, _ = kernels.deconv_igdn_h3(hs, x2, net.Decoder.deconv2.bias, *h4, chunk_major=True)
            ev(5)
            yield
            clipped, _, _, bpp = kernels.deconv3_h3(hs, x3, net.Decoder.deconv3.bias,
                                                    bits=(partial, self.scale))
        elif kernels.precision() == "x6":
            e1, e2, e3, e4 = self.g6
            hs, _, _ = kernels.conv1x6_gdn(self.x, self.w1x6, net.Encoder.conv1.bias, e1[0], e1[2],
                                           N)
            ev(1)
            yield
            hs, _, _ = kernels.conv2_gdn_x6(hs, w2, net.Encoder.conv2.bias, *e2)
            ev(2)
            yield
            y_hat, partial, _, ys = kernels.conv3_quant_rate_x6(hs, w3, self.rate, rtab=self.rtab,
                                                                w_split=self.w3s)
            ev(3)
            yield
            # Synthesis_net_17.decode's x6 path
            hs, _, _ = kernels.deconv_igdn_x6(ys, d1, net.Decoder.deconv1.bias, *e3)
            ev(4)
            yield
            hs, _, _ = kernels.deconv_igdn_x6(hs, d2, net.Decoder.deconv2.bias, *e4, chunk_major=True)
            ev(5)
            yield
            clipped, _, _, bpp = kernels.deconv3_x6(hs, self.d3x6, net.Decoder.deconv3.bias,
                                                    bits=(partial, self.scale))
        else:
            h = kernels.conv1_gdn(self.x, w1, net.Encoder.conv1.bias, g1[0], g1[1], N)
            ev(1)
            yield
            h = kernels.conv2_gdn(h, w2, net.Encoder.conv2.bias, g2[0], g2[1])
            ev(2)
            yield
            y_hat, partial = kernels.conv3_quant_rate(h, w3, self.rate, rtab=self.rtab)
            ev(3)
            yield
            h = kernels.deconv_igdn(y_hat, d1, net.Decoder.deconv1.bias, q1[0], q1[1])
            ev(4)
            yield
            h = kernels.deconv_igdn(h, d2, net.Decoder.deconv2.bias, q2[0], q2[1])
            ev(5)
            yield
            clipped, _, _ = kernels.deconv3(h, d3, net.Decoder.deconv3.bias)
            bpp = None
        ev(6)
        self.last_partial = partial
        if bpp is None:   # the separate reduction kernel (fp32 chain)
            _, bpp = kernels.reduce_partials(partial, self.scale, per_image=False)
        ev(7)
        self.out = (clipped, y_hat, bpp)
        yield


class SplitStep:
    """The eval step with the batch split into n parts launched on n HIP streams: the images are
    independent (no exchange), so one part's phase-locked prologue / epilogue bursts can overlap
    another part's main loops. Same kernels, same per-image results as Step."""

    def __init__(self, net: ImageCompressor, x: torch.Tensor, n: int):
        B = x.shape[0]
        if n < 2 or B % n:
            raise SystemExit(f"--streams {n}: the batch ({B}) must split evenly into >= 2 parts")
        self.parts = [Step(net, xs.contiguous()) for xs in x.chunk(n)]
        self.side = [torch.cuda.Stream(device=x.device) for _ in range(n - 1)]

    def __call__(self):
        main = torch.cuda.current_stream()
        for s in self.side:
            s.wait_stream(main)
        # layer-interleaved launch order (part 0 layer 1, part 1 layer 1, part 0 layer 2, ...):
        # each stream's next kernel is queued while the other's runs (tools/streams_eval.py:
        # interleaved beat one part's whole chain after the other's)
        active = [(st, p.layers()) for st, p in zip([main] + self.side, self.parts)]
        while active:
            nxt = []
            for st, g in active:
                with torch.cuda.stream(st):
                    try:
                        next(g)
                        nxt.append((st, g))
                    except StopIteration:
                        pass
            active = nxt
        for s in self.side:
            main.wait_stream(s)
        return [p.out for p in self.parts]


def train_flops(N: int, H: int, W: int) -> float:
    """Algorithmic FLOPs of one training step per image: forward + input gradients (no conv1
    dgrad) + weight gradients + GDN backward (two channel contractions + the parameter GEMM)."""
    h1, w1, h2, w2, h3, w3 = H // 4, W // 4, H // 8, W // 8, H // 16, W // 16
    conv = {"c1": h1 * w1 * N * 243, "c2": h2 * w2 * N * N * 25, "c3": h3 * w3 * N * N * 25,
            "d1": h3 * w3 * N * N * 25, "d2": h2 * w2 * N * N * 25, "d3": h1 * w1 * N * 243}
    gdn = {"g1": h1 * w1 * N * N, "g2": h2 * w2 * N * N, "q1": h2 * w2 * N * N, "q2": h1 * w1 * N * N}
    fwd = sum(conv.values()) + sum(gdn.values())
    dgrad = sum(v for k, v in conv.items() if k != "c1")
    wgrad = sum(conv.values())
    gdn_bwd = 3 * sum(gdn.values())
    return 2.0 * (fwd + dgrad + wgrad + gdn_bwd)


def run_train(args, net, x, world, dev):
    """C3/C4: fused training step (forward_train + backward + bucketed all-reduce over RCCL +
    ±5 clamp + Adam), λ = 0.01·255² (train_lambda 650.25)."""
    from iclr_17_compression_amd import dist as idist
    from iclr_17_compression_amd.optim import FusedAdam
    net.train()
    params = list(net.parameters())
    opt = FusedAdam(params, lr=1e-4, grad_clip=5)   # ±5 clamp + Adam in one launch
    lam = 0.01 * 255.0 ** 2
    B, _, S, _ = x.shape

    reducer = idist.GradAllReducer(params).attach(net)   # all-reduce overlapped with backward
    loader, data_info = None, None
    if args.train_dir:   # the data path inside the timed region: decode pool → GPU transform
        from iclr_17_compression_amd import data
        paths = make_train_dir(args.train_dir, idist.rank())
        loader = data.TrainLoader(paths, B, S, 7, dev, idist.rank(), world,
                                  workers=args.workers, prefetch=args.prefetch,
                                  cache=not args.stream_data)
        data_info = {"images": len(paths), "workers": args.workers, "prefetch": args.prefetch,
                     "source": ("decoded images resident in HBM (decoded once), crop/resample "
                                "on the GPU" if loader.store is not None else
                                "streamed: worker decode + crop, pinned upload, GPU resample")}
        # the loader alone (no training consuming it): one epoch after a warm-up epoch
        for _ in loader.epoch(0):
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for xb in loader.epoch(1):
            n += xb.shape[0]
        torch.cuda.synchronize()
        data_info["loader_crops_per_s"] = round(n / (time.perf_counter() - t0), 1)
        print(f"data path alone: {data_info['loader_crops_per_s']} crops/s", file=sys.stderr, flush=True)

        def batches():
            e = 2
            while True:
                yield from loader.epoch(e)
                e += 1
        it = batches()

    def step():
        xb = next(it) if loader is not None else x
        opt.zero_grad(set_to_none=True)
        _, mse, bpp = net.forward_train(xb)
        (lam * mse + bpp).backward()
        reducer.finish()
        opt.step()
        return bpp

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        bpp = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = idist.max_over_ranks(time.perf_counter() - t0, dev)
    ms = elapsed / args.steps * 1e3
    if args.dump_outputs and idist.rank() == 0:   # before --full's overlap legs step any further
        dump_outputs(args.dump_outputs, {"bpp": bpp.reshape(1)})
    comm = (allreduce_overlap(args, net, params, opt, reducer, step, ms, dev)
            if world > 1 and args.full else None)
    if loader is not None:
        loader.close()
        data_info["step_crops_per_s"] = round(B * args.steps / elapsed, 1)
    flops = train_flops(args.N, S, S) * B
    tflops = flops / (ms * 1e-3) / 1e12
    x6t = kernels.precision() in ("x6", "h3")   # the backward runs the x6 kernels in both
    h3t = kernels.precision() == "h3"           # h3: the forward runs the codec's h3 kernels
    tpeak = X6_PEAK_TFLOPS if x6t else FP32_MFMA_PEAK_TFLOPS
    return {
        "metric": "Mpixels/s training (fwd+bwd+Adam), " + METRIC,
        "value": round(world * B * S * S * args.steps / elapsed / 1e6, 2),
        "unit": "Mpix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "h3 fwd / f32 bwd" if h3t else "f32",
        "data": "synthetic (splitmix64 uint8/255 images, seeded trained-like weights)",
        "config": {"workload": f"train step, {B} x {S}x{S}x3 crops per GPU, N={args.N}, lambda=0.01",
                   "N": args.N, "batch_per_gpu": B, "global_batch": B * world,
                   "precision": ("h3: forward (the codec's kernels, three fp16 part products per "
                                 "MAC); x6: input gradients, weight gradients and GDN γ gradients "
                                 "(bias/β/rate-parameter sums and Adam in fp32)" if h3t else
                                 "x6: forward, input gradients, weight gradients and GDN γ "
                                 "gradients (bias/β/rate-parameter sums and Adam in fp32)"
                                 if x6t else "exact-f32"),
                   "parallelism": f"dp{world} ({'RCCL' if os.environ.get('ICLR17_DIST_BACKEND', 'nccl') == 'nccl' else 'gloo'} "
                                  "bucketed grad all-reduce overlapped with the backward)"},
        "roofline": {"bound": "mfma", "kernel": "whole training step", "achieved": round(tflops, 2),
                     "peak": round(tpeak, 1), "unit": "TFLOP/s",
                     "peak_basis": ("bf16 dense MFMA peak / 6 (most of the step runs x6; the "
                                    "h3 forward's FLOPs are priced the same)" if x6t
                                    else "fp32 MFMA dense peak"),
                     "frac": round(tflops / tpeak, 4), "traffic": None,
                     "flop_per_step": flops},
        "bpp_last": round(bpp.item(), 6),
        **({"data_path": data_info} if data_info else {}),
        **({"allreduce": comm} if comm else {}),
    }


def _timed_loop(fn, steps: int, dev) -> float:
    """ms per call of fn over `steps` calls, barrier + synchronize brackets, max over ranks."""
    from iclr_17_compression_amd import dist as idist
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    return idist.max_over_ranks(time.perf_counter() - t0, dev) / steps * 1e3


def allreduce_overlap(args, net, params, opt, reducer, step, step_ms: float, dev) -> dict:
    """C4: how much of the gradient all-reduce the backward hides. Measured after the timed
    region, over as many steps: (1) the bucketed all-reduce of one step's gradients alone
    (the reducer's own buckets, nothing else running), (2) the same training step with the
    reducer detached (no all-reduce: each rank keeps its own gradient). exposed = step −
    no-all-reduce step; overlapped fraction = 1 − exposed / all-reduce time. The parameters and
    the Adam moments are restored after (2), so the ranks leave it with the replicas in sync."""
    keys = [torch.zeros_like(p) for p in params]   # stand-ins with no .grad of their own
    grads = [torch.ones_like(p) for p in params]

    def ar_only():
        reducer.launch(keys, grads)
        reducer.wait()

    ar_ms = _timed_loop(ar_only, args.steps, dev)
    # (2) applies Adam to each rank's own (un-averaged) gradient: snapshot what it changes
    snap = [p.detach().clone() for p in params]
    snap_state = {p: {k: v.clone() for k, v in opt.state[p].items()} for p in params if opt.state[p]}
    net._grad_reducer = None
    reducer_finish = reducer.finish
    reducer.finish = lambda: None
    try:
        local_ms = _timed_loop(step, args.steps, dev)
    finally:
        reducer.finish = reducer_finish
        reducer.attach(net)
        with torch.no_grad():
            for p, s in zip(params, snap):
                p.copy_(s)
            for p, st in snap_state.items():
                for k, v in st.items():
                    opt.state[p][k].copy_(v)
        for p in params:   # drop the last un-averaged gradients (the copies bumped the version
            p.grad = None  # counters, so the weight packs rebuild on next use)
    exposed = max(0.0, step_ms - local_ms)
    return {"bucket_mb": reducer.bucket_bytes / 2 ** 20,
            "grad_bytes": sum(p.numel() * 4 for p in params),
            "allreduce_alone_ms": round(ar_ms, 4), "step_without_allreduce_ms": round(local_ms, 4),
            "exposed_ms": round(exposed, 4),
            "overlapped_fraction": round(min(1.0, max(0.0, 1.0 - exposed / ar_ms)), 4) if ar_ms > 0 else None,
            "method": "all-reduce alone and the step without it, timed after the timed region "
                      "over as many steps (barrier + synchronize brackets, max over ranks)"}


def make_train_dir(spec: str, rank: int):
    """--train-dir: a directory of images, or "png:N" / "jpg:N" — N synthetic photos (768×512 and
    512×768, shifted and flipped variants of 16 smooth synthetic images) encoded by PIL into a
    temporary directory once per rank."""
    kind, _, n = spec.partition(":")
    if kind not in ("png", "jpg") or not n.isdigit():
        return sorted(glob.glob(os.path.join(spec, "*.*")))
    import tempfile
    from PIL import Image
    n = int(n)
    d = os.path.join(tempfile.gettempdir(), f"iclr17_bench_{kind}_{n}_{rank}")
    os.makedirs(d, exist_ok=True)
    base = {}
    paths = []
    for i in range(n):
        p = os.path.join(d, f"img{i:04d}.{kind}")
        if not os.path.exists(p):
            portrait = i % 4 == 0
            k = (i % 16, portrait)
            if k not in base:
                H, W = (768, 512) if portrait else (512, 768)
                base[k] = synth.smooth_image_u8(5000 + i % 16, H, W).transpose(1, 2, 0)
            img = np.roll(base[k], (37 * i) % 251, axis=1)
            img = np.ascontiguousarray(img[::-1] if (i // 16) % 2 else img)
            Image.fromarray(img).save(p, **({"compress_level": 1} if kind == "png" else {"quality": 95}))
        paths.append(p)
        if i % 64 == 63:
            print(f"make_train_dir: {i + 1}/{n}", file=sys.stderr, flush=True)
    return paths


KODAK_PORTRAIT = (3, 8, 9, 16, 17, 18)   # kodim04/09/10/17/18/19: 512 wide x 768 tall


def kodak_synth_images(meta):
    """The G5 synthetic Kodak-24 set (tests/golden/gen_goldens.py: smooth_image_u8(100+i))."""
    out = []
    for row in meta["images"]:
        x = synth.to_unit_float(synth.smooth_image_u8(meta["image_seed_base"] + row["index"],
                                                      row["height"], row["width"]))
        out.append(torch.from_numpy(x)[None])
    return out


KODAK_ORDERS = {"g9": "g9s_reference_orders_n192.json"}   # tests/golden/gen_g9s.py

KODAK_SETS = {   # --kodak-set: fixture, description of the weights
    "g9": ("g9_kodak24_synth_n192_trained.json",
           "N=192 weights trained to lambda=0.01 (tests/golden/g9_weights_n192.npz)"),
    "g5": ("g5_kodak24_synth_n192.json", "seeded trained-like N=192 weights (synth.py)"),
}


def kodak_rank_images(rank: int, world: int):
    """This rank's Kodak-24 images (C2 at N GPUs): the 18 landscape images split by shard_range,
    the 6 portrait ones by the reversed rank order, so the ranks with fewer landscape images take
    the portrait ones (8 ranks: 3 images each)."""
    from iclr_17_compression_amd import dist as idist
    land = [i for i in range(24) if i not in KODAK_PORTRAIT]
    lo, hi = idist.shard_range(len(land), rank, world)
    plo, phi = idist.shard_range(len(KODAK_PORTRAIT), world - 1 - rank, world)
    return land[lo:hi], list(KODAK_PORTRAIT)[plo:phi]


def kodak_table(rows: dict, ncols: int, dev) -> np.ndarray:
    """The [24, ncols] per-image table from every rank's rows {image index: values}: each rank
    fills its own rows, the others stay exact zeros, and one all-reduce (sum) assembles it — the
    result does not depend on the summation order."""
    from iclr_17_compression_amd import dist as idist
    table = torch.zeros(24, ncols, dtype=torch.float64, device=dev)
    for i, vals in rows.items():
        table[i] = torch.tensor(vals, dtype=torch.float64)
    if idist.world() > 1:
        dist.all_reduce(table, op=dist.ReduceOp.SUM)
    return table.cpu().numpy()


def run_kodak(args, dev):
    """C2 (BASELINE configs[1]): Kodak-24 encode/decode at N=192 with testKodak's per-image
    metrics (bpp, PSNR, MS-SSIM on the GPU), synthetic Kodak images (no network); parity against
    the reference's own values: G9 (default; weights trained to λ = 0.01, PSNR ≈ 27 dB) or G5
    (seeded trained-like weights, a degenerate 6.6 dB point). At N ranks the 24 images are
    sharded (kodak_rank_images; images are independent, no collective in the data path) and the
    per-image metrics come back with one fixed-order sum at the end."""
    from iclr_17_compression_amd import dist as idist
    world, rank = idist.world(), idist.rank()
    fixture, weights_note = KODAK_SETS[args.kodak_set]
    meta = json.load(open(os.path.join(REPO, "tests", "golden", fixture)))
    net = ImageCompressor(out_channel_N=meta["N"])
    if "weights" in meta:
        d = np.load(os.path.join(REPO, "tests", "golden", meta["weights"]))
        net.load_state_dict({k: torch.from_numpy(d[k].astype(np.float32)) for k in d.files})
    else:
        net.load_state_dict({k: torch.from_numpy(v) for k, v in
                             synth.trained_like_state_dict(meta["N"], meta["weight_seed"]).items()})
    net = net.to(dev).eval()
    imgs = kodak_synth_images(meta)
    groups = [g for g in kodak_rank_images(rank, world) if g]
    batches = [torch.cat([imgs[i] for i in g]).to(dev) for g in groups]

    def step():   # the two orientations on concurrent streams (ImageCompressor.evaluate_many)
        return tuple(net.evaluate_many(batches, want_msssim=True))

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            evs = step()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = idist.max_over_ranks(time.perf_counter() - t0, dev)
    # per-image metrics and the reference-latent match: rows of this rank's images, summed over
    # ranks (every other rank contributes exact zeros, so the sum is order-independent)
    keys = ("bpp", "psnr", "ms_ssim")
    rows = {}
    for ev, g in zip(evs, groups):
        for j, i in enumerate(g):
            rows[i] = [ev[k][j].item() for k in keys] + [0.0]
    yfix = {"g9": "g9_y_hat_n192.npz"}.get(args.kodak_set)
    if yfix:   # ŷ against the reference's own committed latents (tests/golden/gen_yhat.py)
        yd = np.load(os.path.join(REPO, "tests", "golden", yfix))
        with torch.no_grad():
            for i in rows:
                ev = net.evaluate(imgs[i].to(dev))
                ref = torch.from_numpy(yd[f"yhat_{i:02d}"].astype(np.float32)).to(dev)
                rows[i][len(keys)] = float((ev["y_hat"] != ref).sum().item())
    t = kodak_table(rows, len(keys) + 1, dev)
    if args.dump_outputs and rank == 0:   # the last timed step's per-image bpp / PSNR / MS-SSIM
        dump_outputs(args.dump_outputs, {"per_image_metrics": torch.from_numpy(t[:, :len(keys)].copy())})
    per = {i: {k: float(t[i, c]) for c, k in enumerate(keys)} for i in range(24)}
    rel = {k: max(abs(per[i][k] - meta["images"][i][k]) / abs(meta["images"][i][k]) for i in range(24))
           for k in keys}
    parity = {"max_rel_" + k: v for k, v in rel.items()}
    if yfix:
        parity["latent_flips_vs_reference_y_hat"] = int(t[:, len(keys)].sum())
        parity["images_with_the_reference_latents"] = int((t[:, len(keys)] == 0).sum())
    if args.kodak_set in KODAK_ORDERS:   # the bar: the reference's own cross-order spread (G8s/G9s)
        orders = json.load(open(os.path.join(REPO, "tests", "golden", KODAK_ORDERS[args.kodak_set])))
        sp = orders["set_spread_fp32"]
        parity["reference_cross_order_spread"] = {
            "max_rel_" + k: sp["rel_d" + k] for k in keys}
        parity["reference_cross_order_flips"] = orders["total_flips_vs_default"]
        parity["reference_images_with_flips_max"] = orders["max_images_with_flips_fp32"]
        parity["bar"] = {"max_rel_" + k: max(1e-5, sp["rel_d" + k] + 1e-6) for k in keys}
    pixels = 24 * 512 * 768 * args.steps
    return {
        "metric": "Mpixels/s Kodak-24 encode+decode with per-image bpp/PSNR/MS-SSIM (C2)",
        "value": round(pixels / elapsed / 1e6, 2), "unit": "Mpix/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": DTYPE[kernels.precision()],
        "data": f"synthetic Kodak-24 (18 x 512x768 + 6 x 768x512, smooth_image_u8), {weights_note}",
        "config": {"workload": "Kodak-24 eval: encode, round, rate, decode, clamp, per-image bpp/PSNR/MS-SSIM",
                   "N": meta["N"], "precision": kernels.precision(),
                   "parallelism": f"dp{world} (the 24 images sharded by rank, metrics summed at the end)"},
        f"parity_vs_reference_{args.kodak_set.upper()}": parity,
        "dataset_average": {k: sum(per[i][k] for i in range(24)) / 24 for k in keys},
    }


def run_codec(args, dev):
    """§8 f4: the codec with a REAL bitstream. One step = analysis + round (fused kernels) →
    rANS encode of ŷ (+ stream offsets, pack) → rANS decode → synthesis + clamp; the bitstream
    stays in HBM. Reports the entropy-coder kernels' own rates and the real vs the estimated
    (reference model.py:71-78) bits."""
    N, S, B = args.N, args.size, args.batch
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(0, B, S, S))).to(dev)
    cum = net.bitEstimator.entropy_tables()
    h = w = S // 16
    t_enc, t_dec = [], []

    def step(timed=False):
        q = net.encode_latents(x)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        words, offsets = kernels.rans_encode(q["y_hat"], cum)
        e1.record()
        y = kernels.rans_decode(words, offsets, cum, B, h, w, N)
        e2.record()
        split = kernels.split_planes(y) if kernels.precision() == "x6" else None
        yh3 = kernels.h3_planes(y, cm=kernels.DECONV_CM) if kernels.precision() == "h3" else None
        clipped, _, _ = net.Decoder.decode(y, want_recon=False, y_split=split, y_integral=True,
                                           y_h3=yh3)
        if timed:
            t_enc.append((e0, e1))
            t_dec.append((e1, e2))
        return q, words, y, clipped

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            q, words, y, clipped = step(timed=True)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"y_hat": y, "clipped": clipped})
        if not torch.equal(y, q["y_hat"]):
            raise SystemExit("codec bench: decoded latents differ from the encoded ones")
        bits, _ = kernels.reduce_partials(q["bits_partial"])
    enc_ms = sorted(a.elapsed_time(b) for a, b in t_enc)[len(t_enc) // 2]
    dec_ms = sorted(a.elapsed_time(b) for a, b in t_dec)[len(t_dec) // 2]
    syms = B * h * w * N
    real_bits = 16.0 * words.numel() + 32.0 * B * kernels.STREAMS_PER_IMAGE   # + the length header
    est_bits = float(bits.sum().item())
    return {
        "metric": "Mpixels/s encode+decode through a real rANS bitstream (SURVEY 8f row 4)",
        "value": round(B * S * S * args.steps / elapsed / 1e6, 2), "unit": "Mpix/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": DTYPE[kernels.precision()] + " transforms, u32 rANS state",
        "data": "synthetic (splitmix64 uint8/255 images, seeded trained-like weights)",
        "config": {"workload": f"image -> bitstream -> image, {B} x {S}x{S}x3, N={N}",
                   "precision": kernels.precision(), "K": kernels.ENTROPY_K,
                   "streams_per_image": kernels.STREAMS_PER_IMAGE},
        "entropy_coder": {"encode_ms": round(enc_ms, 4), "decode_ms": round(dec_ms, 4),
                          "encode_Msym_per_s": round(syms / enc_ms / 1e3, 1),
                          "decode_Msym_per_s": round(syms / dec_ms / 1e3, 1),
                          "real_bpp": round(real_bits / (B * S * S), 5),
                          "estimated_bpp": round(est_bits / (B * S * S), 5),
                          "real_over_estimated": round(real_bits / est_bits, 5)},
    }


def run_encdec(args, dev):
    """The separate encode / decode path (NewTests/testReconSeperateEandD.py:67-68,
    train_decoder_new.py:66-105): y = net.Encoder(x), ŷ = torch.round(y), x̂ = net.Decoder(ŷ),
    through the nn.Module surface, each half timed with HIP events on the current stream."""
    N, S, B = args.N, args.size, args.batch
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(0, B, S, S))).to(dev)
    t_enc, t_dec = [], []

    def step(timed=False):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        y_hat = torch.round(net.Encoder(x))
        e1.record()
        recon = net.Decoder(y_hat)
        e2.record()
        if timed:
            t_enc.append((e0, e1))
            t_dec.append((e1, e2))
        return y_hat, recon

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y_hat, recon = step(timed=True)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"y_hat": y_hat, "recon": recon})
        _, fwd_yhat, _ = net(x)
        same = bool(torch.equal(y_hat, fwd_yhat))
    enc_ms = float(np.mean([a.elapsed_time(b) for a, b in t_enc]))
    dec_ms = float(np.mean([a.elapsed_time(b) for a, b in t_dec]))
    px = B * S * S
    return {
        "metric": "Mpixels/s separate encode (Encoder) + decode (Decoder) through the module surface",
        "value": round(px * args.steps / elapsed / 1e6, 2), "unit": "Mpix/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": DTYPE[kernels.precision()],
        "data": "synthetic (splitmix64 uint8/255 images, seeded trained-like weights)",
        "config": {"workload": f"round(Encoder(x)) then Decoder, {B} x {S}x{S}x3, N={N}",
                   "precision": kernels.precision()},
        "encode_ms": round(enc_ms, 4), "decode_ms": round(dec_ms, 4),
        "encode_Mpix_per_s": round(px / enc_ms / 1e3, 1), "decode_Mpix_per_s": round(px / dec_ms / 1e3, 1),
        "round_encoder_equals_forward_latents": same,
    }


def cpu_threads() -> tuple:
    """(threads used, cores in this process's affinity mask): every affinity core, unless the
    box's CPU share is pinned by OMP_NUM_THREADS (16 on the GPU pool, whose affinity mask shows
    the whole machine)."""
    aff = len(os.sched_getaffinity(0))
    omp = os.environ.get("OMP_NUM_THREADS", "")
    return (min(aff, int(omp)) if omp.isdigit() and int(omp) > 0 else aff), aff


def cpu_baseline(N: int, H: int, W: int, budget_s: float) -> dict:
    """The oracle (op-for-op restatement of the reference forward, bit-identical to it on the
    build host) timed on this host's cores on a bounded sample."""
    from oracle import codec_ref as oracle
    cores, aff = cpu_threads()
    torch.set_num_threads(cores)
    sd = oracle.state_dict_to_torch(synth.trained_like_state_dict(N, 1))
    B = 4
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(99, B, H, W)))
    with torch.no_grad():
        oracle.codec_forward(x[:1], sd)  # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            oracle.codec_forward(x, sd)
            n += 1
            if time.perf_counter() - t0 > budget_s:
                break
        dt = time.perf_counter() - t0
    return {"value": round(n * B * H * W / dt / 1e6, 4), "unit": "Mpix/s", "cores": cores,
            "affinity_cores": aff, "kind": "port",
            "sample": f"{n} x eval forward of B={B} {H}x{W} images, N={N}, fp32 torch CPU, "
                      f"{cores} threads ({dt:.1f} s, {platform.processor() or platform.machine()})"}


def cpu_baseline_train(N: int, S: int, budget_s: float) -> dict:
    """The training step of the reference on the CPU: the oracle's rd_loss (model.py:47-80 with
    the uniform-noise quantiser, λ·MSE + bpp) forward + autograd backward + torch Adam with the
    ±5 gradient clamp (train.py:115-120), timed on a bounded sample of B=2 crops."""
    from oracle import codec_ref as oracle
    cores, aff = cpu_threads()
    torch.set_num_threads(cores)
    sd = oracle.state_dict_to_torch(synth.trained_like_state_dict(N, 2))
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-4)
    B = 2
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(98, B, S, S)))
    lam = 0.01 * 255.0 ** 2

    def step(i):
        noise = torch.from_numpy(synth.uniform(500 + i, (B, N, S // 16, S // 16), -0.5, 0.5))
        opt.zero_grad(set_to_none=True)
        loss, _, _ = oracle.rd_loss(x, params, noise, lam)
        loss.backward()
        for p in params.values():
            p.grad.clamp_(-5, 5)
        opt.step()

    step(0)   # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        step(n + 1)
        n += 1
        if time.perf_counter() - t0 > budget_s:
            break
    dt = time.perf_counter() - t0
    return {"value": round(n * B * S * S / dt / 1e6, 5), "unit": "Mpix/s", "cores": cores,
            "affinity_cores": aff, "kind": "port",
            "sample": f"{n} x train step (fwd + autograd bwd + Adam) of B={B} {S}x{S} crops, "
                      f"N={N}, fp32 torch CPU, {cores} threads ({dt:.1f} s)"}


DUMP_BUDGET = 64 * 10 ** 6 - 4096   # array bytes of one --dump-outputs (64 MB less the .npy headers)


def dump_outputs(d: str, outputs: dict) -> None:
    """--dump-outputs: every tensor of `outputs` as d/<name>.npy, float32 (float64 stays). When
    they exceed DUMP_BUDGET together, each array larger than an equal share of it is written as
    a 1-D sample of its flattened elements, at sorted indices drawn with a fixed seed (the same
    indices for the same shape, so two builds' dumps compare element for element)."""
    os.makedirs(d, exist_ok=True)

    def size(t):
        return t.numel() * (8 if t.dtype == torch.float64 else 4)
    total = sum(size(t) for t in outputs.values())
    share = DUMP_BUDGET // max(len(outputs), 1)
    for name, t in outputs.items():
        t = t.detach()
        if total > DUMP_BUDGET and size(t) > share:
            n = share // (8 if t.dtype == torch.float64 else 4)
            idx = np.sort(np.random.default_rng(0).integers(0, t.numel(), n))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        t = t if t.dtype == torch.float64 else t.float()
        np.save(os.path.join(d, name + ".npy"), t.cpu().numpy())


def lib_sha() -> str:
    import hashlib
    from iclr_17_compression_amd import _lib
    return hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]


def profile_layers(N: int, S: int, B: int, prec: str) -> dict:
    """Per bench layer, the rocprof trace mean (ms) of its kernel from the committed summary of
    THIS library build (profiles/*_traffic.json, tools/profile_round.sh), or {}."""
    sha = lib_sha()
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "*_traffic.json")), reverse=True):
        d = json.load(open(f))
        if (d.get("precision") == prec and d.get("workload") == {"N": N, "S": S, "B": B}
                and d.get("lib_sha256") == sha):
            return {k: e["mean_ms"] for k, e in d.get("layers", {}).items() if e.get("mean_ms")}
    return {}


def pmc_traffic(layer: str, N: int, S: int, B: int, prec: str):
    """HBM bytes per launch of `layer` from a committed PMC summary (profiles/*_traffic.json, made
    by tools/profile_round.sh — counters cannot be collected inside this process). Only a summary
    of THIS library build (SHA-256 of the loaded libiclr17.so), this precision and this workload
    counts; otherwise (None, reason)."""
    sha = lib_sha()
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "*_traffic.json")))
    seen = []
    for f in reversed(files):
        d = json.load(open(f))
        if d.get("precision") != prec or d.get("workload") != {"N": N, "S": S, "B": B}:
            continue
        seen.append(f"{os.path.basename(f)}@{d.get('lib_sha256')}")
        e = d.get("layers", {}).get(layer, {})
        if d.get("lib_sha256") == sha and "traffic_bytes" in e:
            return e["traffic_bytes"], (f"profiles/{os.path.basename(f)} (lib {sha}, kernel "
                                        f"{e.get('kernel')}, trace mean {e.get('mean_ms', 0):.4f} ms)"), e.get("mean_ms")
    why = (f"no PMC summary of this build (lib {sha}) for {prec} {layer} at N={N} S={S} B={B}"
           + (f"; summaries of other builds: {', '.join(seen[:3])}" if seen else ""))
    return None, why, None


CLOCK_RAMP_S = 0.3   # the GPU clock ramps over the first ~50 ms of load (tools/warm_probe.py)


def time_eval(net, x, args, world, dev, per_layer: bool = True, ramp: bool = False) -> dict:
    """W warm-up steps, then K timed steps between barrier + synchronize brackets; "outputs" is
    what the last timed step returned. per_layer (--full) adds a second pass of K steps with
    HIP-event brackets per layer on the launching stream (outside the wall-clock region, so the
    brackets cannot perturb it). ramp: CLOCK_RAMP_S of the same step before the warm-up, so that
    the timed region starts at steady clocks when no other leg has run before it (--full: the
    bf16 leg has). Elapsed is the max over ranks."""
    step = Step(net, x)
    streams = args.bf16_streams if kernels.precision() == "bf16" else args.streams
    with torch.no_grad():
        split = SplitStep(net, x, streams) if streams > 1 else None
        run = split or step
        if ramp:
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < CLOCK_RAMP_S:
                run()
                torch.cuda.synchronize()
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        if args.graph:
            # the step's launches captured once into a HIP graph (torch.cuda.CUDAGraph on ROCm):
            # each replay submits the whole chain at once (no per-kernel host launch, shorter
            # gaps between dependent kernels); outputs land in the graph's own memory pool
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run()   # SplitStep: the side streams fork from / join the capture stream
            graph.replay()
            torch.cuda.synchronize()
            run = graph.replay
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            run()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        # the last timed step's results (a graph replays into the tensors of its capture); split
        # over streams: the parts' images and latents joined, one bpp per part
        outs = [p.out for p in split.parts] if split else [step.out]
        clipped, y_hat = (torch.cat([o[i] for o in outs]) for i in (0, 1))
        bpps = torch.stack([o[2].reshape(()) for o in outs])
        res = {"bpp": bpps.mean(), "clipped": clipped, "y_hat": y_hat,
               "outputs": {"clipped": clipped, "y_hat": y_hat, "bpp": bpps}}
        if per_layer:
            if run is not step:   # the one-stream step of the per-layer pass, warm
                for _ in range(3):
                    step()
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(8)] for _ in range(args.steps)]
            for i in range(args.steps):
                clipped, y_hat, bpp = step(evs[i])
            torch.cuda.synchronize()
            B, _, H, W = x.shape
            bits, _ = kernels.reduce_partials(step.last_partial)
            res.update({"bpp": bpp, "clipped": clipped, "y_hat": y_hat,
                        "bpp_img": (bits / (H * W)).double(),
                        "per_layer_ms": {name: float(np.mean([evs[i][j].elapsed_time(evs[i][j + 1])
                                                              for i in range(args.steps)]))
                                         for j, name in enumerate(LAYERS)}})
    t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    res["elapsed"] = t.item()
    return res


def roofline(per_layer_ms: dict, prec: str, N: int, S: int, B: int):
    """(dominant layer, per-layer table, roofline object) of one eval pass."""
    flops, bytes_ = layer_flops(N, S, S), layer_bytes(N, S, S, 2 if prec == "bf16" else 4)
    dominant = max(LAYERS, key=lambda k: per_layer_ms[k])
    achieved = flops[dominant] * B / (per_layer_ms[dominant] * 1e-3) / 1e12
    layers = {k: {"ms": round(per_layer_ms[k], 4),
                  "tflops": round(flops[k] * B / (per_layer_ms[k] * 1e-3) / 1e12, 2) if flops[k] else None,
                  "gbs": round(bytes_[k] * B / (per_layer_ms[k] * 1e-3) / 1e9, 1) if bytes_[k] else None}
              for k in LAYERS}
    peak, note = layer_peak(prec, dominant)
    prof = profile_layers(N, S, B, prec)
    for k in LAYERS:
        if flops[k]:
            pk = layer_peak(prec, k)[0]
            layers[k]["peak"] = round(pk, 1)
            layers[k]["frac"] = round(flops[k] * B / (per_layer_ms[k] * 1e-3) / 1e12 / pk, 4)
            if prof.get(k):   # the same fraction from the SHA-matched rocprof trace mean
                layers[k]["profile_mean_ms"] = round(prof[k], 4)
                layers[k]["frac_from_profile"] = round(flops[k] * B / (prof[k] * 1e-3) / 1e12 / pk, 4)
    # per-layer T_roof = max(F / P_peak, bytes / BW_peak) and the whole chain's
    # Σ T_roof / Σ T_measured (P_peak the mode's MFMA peak, BW_peak the HBM peak)
    t_roof = {}
    for k in LAYERS:
        if not flops[k]:
            continue
        p = layer_peak(prec, k)[0]
        t_mfma = flops[k] * B / (p * 1e12) * 1e3
        t_hbm = bytes_[k] * B / (HBM_PEAK_GBS * 1e9) * 1e3
        t_roof[k] = max(t_mfma, t_hbm)
        layers[k]["t_roof_ms"] = round(t_roof[k], 4)
        layers[k]["roof_bound"] = "mfma" if t_mfma >= t_hbm else "hbm"
    measured = sum(per_layer_ms[k] for k in t_roof)
    traffic, src, prof_ms = pmc_traffic(dominant, N, S, B, prec)
    roof = {"bound": "mfma", "kernel": dominant, "achieved": round(achieved, 2), "peak": round(peak, 1),
            "unit": "TFLOP/s", "peak_basis": note, "frac": round(achieved / peak, 4),
            "duration": "hip_events: mean over the K steps on the launching stream "
                        f"({per_layer_ms[dominant]:.4f} ms)",
            "frac_of_bf16_dense_peak": round(achieved / BF16_MFMA_PEAK_TFLOPS, 4),
            "traffic": traffic, "traffic_source": src if traffic is not None else None,
            "chain_roofline_frac": round(sum(t_roof.values()) / measured, 4)}
    if prof_ms:   # the SHA-matched rocprof trace mean of the same kernel, and the fraction it gives
        roof["profile_mean_ms"] = round(prof_ms, 4)
        roof["frac_from_profile"] = round(flops[dominant] * B / (prof_ms * 1e-3) / 1e12 / peak, 4)
    if traffic is None:
        roof["traffic_null_reason"] = src
    return dominant, layers, roof


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n: int, argv) -> int:
    """`python bench.py --gpus N` without torchrun: start N fresh interpreters, one per GPU (rank r
    on GPU r), with torchrun's environment (RANK / LOCAL_RANK / WORLD_SIZE, MASTER_ADDR
    127.0.0.1, a free MASTER_PORT). The parent has made no HIP call: it only waits, forwards the
    children's output (rank 0 prints the JSON line) and returns the first failing exit status,
    ending the other ranks when one fails."""
    import subprocess
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), GROUP_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env))
    rc = 0
    while procs:
        time.sleep(0.2)
        for p in list(procs):
            code = p.poll()
            if code is None:
                continue
            procs.remove(p)
            if code != 0 and rc == 0:
                rc = code
                print(f"bench: a rank exited with status {code}; stopping the others",
                      file=sys.stderr, flush=True)
                for q in procs:
                    q.terminate()
    return rc if rc >= 0 else 1


def check_world(args, world: int, backend: str, ndev: int) -> None:
    """--gpus must be the process count, and (RCCL) one process per visible GPU."""
    if world > 1 and args.gpus != world:
        raise SystemExit(f"bench: --gpus {args.gpus} but WORLD_SIZE {world}")
    if backend == "nccl" and not args.dry_run and args.gpus > ndev:
        raise SystemExit(f"bench: --gpus {args.gpus} but only {ndev} GPUs are visible "
                         "(one process per GPU over RCCL)")


def rank_layout(dev, backend: str) -> dict:
    """Per-rank device ids (all-gathered) and the RCCL communicator's size, for the JSON line."""
    world = idist_world()
    mine = dev.index if dev.type == "cuda" else -1
    ids = [mine]
    if world > 1:
        t = torch.tensor([mine], dtype=torch.int64, device=dev)
        out = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(out, t)
        ids = [int(o.item()) for o in out]
    return {"dist_backend": backend if world > 1 else None,
            "rccl_world_size": world if (world > 1 and backend == "nccl") else None,
            "rank_devices": ids}


def idist_world() -> int:
    return dist.get_world_size() if dist.is_initialized() else 1


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="strong scaling: images over all GPUs, split evenly by rank (C5: 64 at "
                         "--size 2048); overrides --batch")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch, rendezvous, barrier and max-over-ranks only (no kernels): checks "
                         "the multi-rank plumbing on a host without a GPU")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--N", type=int, default=192)
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: eval — the bf16 and x6 legs, "
                         "the per-layer pass with its roofline, the CPU baseline; train — the CPU "
                         "baseline and (N > 1) the all-reduce overlap")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy "
                         "(float32; at most 64 MB in all, a fixed seeded sample of a larger array)")
    ap.add_argument("--cpu-budget", type=float, default=15.0)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU leg")
    ap.add_argument("--kodak-set", choices=tuple(KODAK_SETS), default="g9",
                    help="kodak mode: the operating point (g9 trained, g5 trained-like)")
    ap.add_argument("--train-dir", default="",
                    help='train mode: images for the data path in the timed step ("png:N": N synthetic PNGs)')
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--stream-data", action="store_true",
                    help="train-dir: decode every epoch instead of keeping decoded images in HBM")
    ap.add_argument("--prefetch", type=int, default=4)
    ap.add_argument("--no-bf16-leg", action="store_true",
                    help="x6 eval: skip the bf16 throughput-mode leg reported as bf16_mode")
    ap.add_argument("--no-x6-leg", action="store_true",
                    help="h3 eval: skip the x6 (full fp32 operand) leg reported as x6_mode")
    ap.add_argument("--streams", type=int, default=1,
                    help="eval: split the batch over this many HIP streams in the timed region "
                         "(independent images; per-layer timings stay one stream)")
    ap.add_argument("--bf16-streams", type=int, default=1,
                    help="the same for the bf16 leg / --precision bf16")
    ap.add_argument("--graph", action="store_true",
                    help="eval: replay the timed steps from one HIP graph instead of launching them "
                         "kernel by kernel (slower than eager: bf16 12 %% in round 4, profiles/r04_ab_streams.log; x6 4 %% in round 3)")
    ap.add_argument("--mode", choices=("eval", "train", "kodak", "codec", "encdec"), default="eval")
    ap.add_argument("--precision", choices=kernels.PRECISIONS, default=None,
                    help="inference contraction mode (default: ICLR17_PRECISION or x6)")
    args = ap.parse_args()
    if os.environ.get("ICLR17_HANG_DUMP"):   # diagnostic: periodic stack dumps to stderr
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["ICLR17_HANG_DUMP"]), repeat=True)
    if args.precision:
        kernels.set_precision(args.precision)

    # one process per GPU over RCCL ("nccl"). ICLR17_DIST_BACKEND=gloo rehearses the multi-rank
    # path with several ranks sharing the GPUs there are (device = local rank mod device count)
    backend = os.environ.get("ICLR17_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()   # counts devices without initialising HIP on this image
    if args.dry_run and ndev == 0 and backend == "nccl":
        backend = "gloo"   # RCCL needs a device; the plumbing dry run falls back to gloo on CPU
    if "WORLD_SIZE" not in os.environ:
        check_world(args, 1, backend, ndev)
        if args.gpus > 1:   # no torchrun: start the N ranks here, before any HIP call
            raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    check_world(args, world, backend, ndev)
    if backend == "nccl" and world > 1 and local >= ndev:
        raise SystemExit(f"bench: LOCAL_RANK {local} but only {ndev} GPUs (one process per GPU)")
    local = local % max(ndev, 1)
    if args.dry_run:
        dev = torch.device("cuda", local) if ndev else torch.device("cpu")
    else:
        dev = torch.device("cuda", local)
    if world > 1:
        if dev.type == "cuda":
            torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    layout = rank_layout(dev, backend)
    if args.global_batch:
        if args.global_batch % world:
            raise SystemExit(f"bench: --global-batch {args.global_batch} is not a multiple of {world} ranks")
        args.batch = args.global_batch // world
    if args.dry_run:
        from iclr_17_compression_amd import dist as idist
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        if world > 1:
            dist.barrier()
        elapsed = idist.max_over_ranks(time.perf_counter() - t0, dev)
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "batch_per_gpu": args.batch,
                              "global_batch": args.batch * world,
                              "scaling": "strong" if args.global_batch else "weak",
                              "barrier_s": elapsed, **layout}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return

    if args.mode == "kodak":   # all ranks: the 24 images are sharded
        res = run_kodak(args, dev)
        res.update(layout)
        if rank == 0:
            print(json.dumps(res), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    if args.mode in ("codec", "encdec"):
        if rank == 0:
            run = {"kodak": run_kodak, "codec": run_codec, "encdec": run_encdec}[args.mode]
            print(json.dumps(run(args, dev)), flush=True)
        return
    N, S, B = args.N, args.size, args.batch
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
    net = net.to(dev).eval()
    # each rank encodes its own shard of the global batch (images are independent)
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(1000 + rank, B, S, S))).to(dev)
    if args.mode == "train":
        result = run_train(args, net, x, world, dev)
        result.update(layout)
        if args.global_batch:
            result["scaling"] = "strong"
        if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:   # the CPU leg: N=1 only
            result["cpu_baseline"] = cpu_baseline_train(N, min(S, 256), args.cpu_budget)
        if rank == 0:
            print(json.dumps(result), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    prec = kernels.precision()
    rb = None
    if args.full and prec in ("x6", "h3") and not args.no_bf16_leg:
        # the bf16 throughput-mode leg runs first (reported as bf16_mode below). Its step is 4x
        # shorter and the GPU clock ramps over the first ~50 ms of load (tools/warm_probe.py:
        # bf16 0.567 → 0.465 ms, x6 2.49 → 2.06 ms per step), so it warms for at least 100 steps
        # before its timed region; the headline's timed region then starts at steady clocks. It
        # runs at every rank count (max over ranks, whole-job rate) so that 1- and N-GPU
        # headlines start from the same clock state.
        kernels.set_precision("bf16")
        try:
            rb = time_eval(net, x, argparse.Namespace(**{**vars(args), "warmup": max(args.warmup, 100)}),
                           world, dev)
        finally:
            kernels.set_precision(prec)
    # a plain run has no leg before the headline: it ramps the clock on the headline's own step
    r = time_eval(net, x, args, world, dev, per_layer=args.full, ramp=not args.full)
    kernels.check_finite("bench bpp", r["bpp"])   # h3: NaN when an activation did not fit the form
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, r["outputs"])
    rx = None
    if args.full and prec == "h3" and not args.no_x6_leg:
        # the x6 mode (full fp32 operands: an exact three-part bf16 split, six products per MAC)
        # on the same batch after the headline, so that a full-fp32-operand rate stays timed on
        # the driver's box next to the h3 one (reported as x6_mode below)
        kernels.set_precision("x6")
        try:
            rx = time_eval(net, x, args, world, dev)
        finally:
            kernels.set_precision(prec)
    nstreams = args.bf16_streams if prec == "bf16" else args.streams
    elapsed, bpp = r["elapsed"], r["bpp"]
    pixels = world * B * S * S * args.steps
    value = pixels / elapsed / 1e6
    ms_per_step = elapsed / args.steps * 1e3
    flops = layer_flops(N, S, S)
    total_flops = sum(flops.values()) * B
    result = {
        "metric": METRIC,
        "value": round(value, 2),
        "unit": "Mpix/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "strong" if args.global_batch else "weak",
        "vs_baseline": None,
        "dtype": DTYPE[prec],
        "dtype_note": DTYPE_NOTE[prec],
        "data": "synthetic (splitmix64 uint8/255 images, seeded trained-like weights)",
        **layout,
        "config": {"workload": (f"eval encode+decode (round quantiser + rate), {B} x {S}x{S}x3 images per GPU"
                                + (f" ({args.global_batch} over {world} GPUs)" if args.global_batch else "")
                                + f", N={N}"),
                   "N": N, "image": f"{S}x{S}x3", "batch_per_gpu": B, "global_batch": B * world,
                   "quant": "round",
                   "precision": PRECISION_NOTE[prec],
                   "parallelism": f"dp{world} (images sharded by rank, no data-path collective)",
                   "launch": ("hipGraph replay of the whole step" if args.graph else
                              "eager (kernel by kernel)" + (f", batch split over {nstreams} HIP streams"
                                                            if nstreams > 1 else ""))},
        "whole_step_tflops": round(total_flops / (ms_per_step * 1e-3) / 1e12, 2),
        "bpp_last": round(bpp.item(), 6),
    }
    if args.full:   # the per-layer pass: the dominant kernel's roofline and the layer table
        bytes_ = layer_bytes(N, S, S, 2 if prec == "bf16" else 4)
        dominant, layers, roof = roofline(r["per_layer_ms"], prec, N, S, B)
        result["roofline"] = {**roof, "algorithmic_bytes_per_launch": bytes_[dominant] * B,
                              "flop_per_launch": flops[dominant] * B,
                              "whole_step_tflops": result.pop("whole_step_tflops")}
        result["layers"] = layers
    if rb is not None:
        # the bf16 throughput mode on the same batch: rate, roofline, and its deviation from the
        # parity mode's (fp32-accurate) results — latent flips, Δbpp, ΔPSNR
        dom_b, layers_b, roof_b = roofline(rb["per_layer_ms"], "bf16", N, S, B)
        flips = int((rb["y_hat"] != r["y_hat"]).sum().item())

        def psnr(c):
            return (10 * torch.log10(1.0 / ((c - x) ** 2).mean(dim=(1, 2, 3)))).double()
        result["bf16_mode"] = {
            "value": round(pixels / rb["elapsed"] / 1e6, 2), "unit": "Mpix/s",
            "warmup": max(args.warmup, 100),
            "ms_per_step": round(rb["elapsed"] / args.steps * 1e3, 4), "dtype": "bf16",
            "streams": args.bf16_streams,
            "roofline": {k: roof_b[k] for k in ("kernel", "achieved", "peak", "frac", "duration",
                                                  "profile_mean_ms", "frac_from_profile", "traffic",
                                                  "traffic_source", "traffic_null_reason",
                                                  "chain_roofline_frac")
                         if k in roof_b},
            "layers": layers_b,
            "vs_parity_mode": {"parity_mode": prec, "latent_flip_rate": flips / r["y_hat"].numel(),
                      "max_abs_dbpp_per_image": float((rb["bpp_img"] - r["bpp_img"]).abs().max()),
                      "max_abs_dpsnr_db_per_image": float((psnr(rb["clipped"]) - psnr(r["clipped"])).abs().max())},
        }
    if rx is not None:
        dom_x, layers_x, roof_x = roofline(rx["per_layer_ms"], "x6", N, S, B)
        result["x6_mode"] = {
            "value": round(pixels / rx["elapsed"] / 1e6, 2), "unit": "Mpix/s",
            "ms_per_step": round(rx["elapsed"] / args.steps * 1e3, 4), "dtype": DTYPE["x6"],
            "dtype_note": DTYPE_NOTE["x6"],
            "roofline": {k: roof_x[k] for k in ("kernel", "achieved", "peak", "peak_basis", "frac",
                                                  "duration", "profile_mean_ms", "frac_from_profile",
                                                  "traffic", "traffic_source", "traffic_null_reason",
                                                  "chain_roofline_frac")
                         if k in roof_x},
            "layers": layers_x,
            "vs_headline": {"latent_flips": int((rx["y_hat"] != r["y_hat"]).sum().item()),
                            "latents": r["y_hat"].numel(),
                            "max_abs_rel_dbpp_per_image": float(((rx["bpp_img"] - r["bpp_img"]).abs()
                                                                 / r["bpp_img"].abs()).max())},
        }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:   # the CPU leg: N=1 only
        # per-pixel cost is size-independent: the sample is 256² images at any --size
        result["cpu_baseline"] = cpu_baseline(N, min(S, 256), min(S, 256), args.cpu_budget)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
