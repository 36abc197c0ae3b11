"""Cost of a training step along the quantiser-step ladder (csrc/steptrain.hip) on
the GPU, in one process, arms alternating inside every round (diagnostic; needs a GPU):

  unstepped   forward_train(x) and the backward of λ·mse + bpp: CodecTrainFn, the rate term fused
              into conv3's epilogue (forward) and deconv1's input-gradient epilogue (backward)
  stepped     forward_train(x, steps=random ladder indices) and the backward of
              mean(λ_b·mse_b + bpp_b): StepTrainFn, the quantiser / rate part as kernels of its own

B = 32 images of 256×256, N = 192, the h3 mode; HIP-event brackets around forward + backward,
warm; median and p10–p90 of both arms, their ratio, and in how many of the alternating pairs the
stepped step was the slower one. The optimiser step is the same in both arms and left out.

    python tools/steptrain_time.py [--rounds 30] [--out profiles/steptrain_ab.txt]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from iclr_17_compression_amd import kernels, synth, train  # noqa: E402
from iclr_17_compression_amd.model import ImageCompressor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--channels", type=int, default=192)
ap.add_argument("--precision", default="h3")
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []
LAM = 8192.0


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    lines.append(line)


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 3), "p10_ms": round(s[len(s) // 10], 3),
            "p90_ms": round(s[(9 * len(s)) // 10], 3)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kernels.set_precision(args.precision)
N, B = args.channels, args.batch
net = ImageCompressor(out_channel_N=N)
net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
net = net.to(dev).train()
x = torch.from_numpy(synth.to_unit_float(synth.image_u8(7, B, args.size, args.size))).to(dev)
noise = net._latent_noise(x)
round_no = [0]


def unstepped():
    _, mse, bpp = net.forward_train(x, noise=noise)
    net.zero_grad(set_to_none=True)
    (LAM * mse + bpp).backward()


def stepped():
    # new random steps every call, as the training loop draws them (host work inside the bracket)
    round_no[0] += 1
    st = train.sample_steps(0, 31, B, round_no[0], 0, 234)
    lams = torch.tensor(train.step_lambdas(LAM, st), dtype=torch.float32)
    _, dist, bpp = net.forward_train(x, noise=noise, steps=st)
    net.zero_grad(set_to_none=True)
    torch.mean(lams.to(dev, non_blocking=True) * dist + bpp).backward()


for _ in range(3):
    unstepped(), stepped()
torch.cuda.synchronize()
kernels.check_finite("warm-up gradients", *[p.grad for p in net.parameters()])
t = {"unstepped": [], "stepped": []}
lost = 0
for r in range(args.rounds):
    order = (("unstepped", unstepped), ("stepped", stepped))[::1 if r % 2 == 0 else -1]
    pair = {}
    for name, fn in order:
        pair[name] = timed(fn)
        t[name].append(pair[name])
    lost += pair["stepped"] > pair["unstepped"]
emit({"what": "training step, forward + backward", "batch": B, "size": args.size, "N": N,
      "precision": args.precision, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)})
for name in t:
    emit({"arm": name, **stats(t[name])})
med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
emit({"median_ratio_stepped_over_unstepped": round(med["stepped"] / med["unstepped"], 4),
      "pairs_lost_by_stepped": int(lost), "of": args.rounds})

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
