"""GPU tests of training along the quantiser-step ladder: the three kernels of
csrc/steptrain.hip against torch's fp32 operations (bitwise where the definition is one rounded
operation, and against the existing rate kernels), and ``forward_train(steps=…)`` against the
stepped reference of tests/step_refs.py in every training precision.

Every figure is printed before it is asserted (run with -s to read them).
"""
import functools
import json
import logging
import math
import os
import re

import pytest
import torch

import backward_refs as R
import step_refs as S
from iclr_17_compression_amd import chain, codec, kernels, synth, train
from iclr_17_compression_amd.model import ImageCompressor
from oracle import codec_ref as oracle

pytestmark = pytest.mark.gpu


def nhwc(t, device):
    return t.permute(0, 2, 3, 1).contiguous().to(device)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def rate_pack(rate, device):
    return kernels.pack_rate([rate[k].to(device) for k in S.RATE_ORDER])


def make(N, seed, device):
    sd = synth.trained_like_state_dict(N, seed)
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(device).train(), oracle.state_dict_to_torch(sd)


@pytest.fixture(params=["h3", "x6", "fp32"])
def precision(request):
    old = kernels.precision()
    kernels.set_precision(request.param)
    yield request.param
    kernels.set_precision(old)


# ------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape", S.KERNEL_SHAPES + S.EXTRA_SHAPES)
def test_step_noise_rate_forward(device, shape):
    """z and ỹ are torch's fp32 y/Δ + u and Δ·z bit for bit; the per-image bits are exactly what
    rate_bits sums over that image's z with the step pack of its Δ."""
    B, h, w, C = shape
    c = S.kernel_case(shape)
    y, noise = nhwc(c["y"], device), c["noise"].to(device)
    d = S.deltas(c["steps"]).to(device)
    pack = rate_pack(c["rate"], device)
    z, y_deq, part = kernels.step_noise_rate(y, noise, d.view(-1), pack)
    z_ref = y / d + nhwc(c["noise"], device)
    assert torch.equal(z, z_ref)
    assert torch.equal(y_deq, d * z_ref)
    bits, _ = kernels.reduce_partials(part)
    assert part.shape == (B, -(-h * w * C // 4096))
    for b, s in enumerate(c["steps"]):
        sp = kernels.pack_rate_step(pack, C, codec.step_size(s))
        ref, _ = kernels.reduce_partials(kernels.rate_bits(z[b:b + 1].permute(0, 3, 1, 2), sp))
        print(f"bits[{b}] step {s}: {bits[b].item()!r} vs rate_bits {ref[0].item()!r}")
        assert bits[b].item() == ref[0].item(), (b, s)
    # reproducible
    z2, q2, part2 = kernels.step_noise_rate(y, noise, d.view(-1), pack)
    assert torch.equal(z, z2) and torch.equal(y_deq, q2) and torch.equal(part, part2)


@pytest.mark.parametrize("shape", S.KERNEL_SHAPES)
def test_step_noise_rate_backward(device, shape):
    """∂L/∂y and the rate-parameter gradients (the kernel's partials through rate_param_grads)
    against the reference with the rate term of the fp32 definition, at step_refs' bars."""
    B, h, w, C = shape
    c = S.kernel_case(shape)
    d = S.deltas(c["steps"])
    pack = rate_pack(c["rate"], device)
    z, _ = S.quantise(c["y"], c["noise"], d)          # the forward test holds the kernel to these
    g_y, part = kernels.step_noise_rate_backward(nhwc(z, device), nhwc(c["g_deq"], device),
                                                 d.view(-1).to(device), pack,
                                                 c["g_bits"].to(device))
    assert part.shape == (B * -(-h * w // 16), 11, C)
    grads = kernels.rate_param_grads(part, [c["rate"][k].to(device) for k in S.RATE_ORDER])
    dz, pg = S.rate_term_fp32(z, c["rate"], c["steps"], c["g_bits"])
    ref = S.quantise_backward(c["g_deq"].double(), dz.double(), d.double())
    e = R.global_err(nchw(g_y), ref)
    print(f"g_y {shape}: {e:.2e} (bar {S.BARS['g_y']:.1e})")
    errs = {k: R.global_err(g.reshape(-1), r.reshape(-1)) for k, g, r in zip(S.RATE_ORDER, grads, pg)}
    print("rate params", {k: f"{v:.2e}" for k, v in errs.items()})
    assert e <= S.BARS["g_y"]
    bad = {k: v for k, v in errs.items() if not v <= S.BARS["rate_params"]}
    assert not bad, bad
    g2, part2 = kernels.step_noise_rate_backward(nhwc(z, device), nhwc(c["g_deq"], device),
                                                 d.view(-1).to(device), pack,
                                                 c["g_bits"].to(device))
    assert torch.equal(g_y, g2) and torch.equal(part, part2)


@pytest.mark.parametrize("shape", S.EXTRA_SHAPES)
def test_kernels_do_not_depend_on_the_channel_count(device, shape):
    """Channel counts other than the codec's (7: less than a wave; 300: a backward thread owns two
    channels) against the 192- and 128-channel runs on the same per-channel data: every channel
    is a model of its own and every output element and partial row entry depends on one channel
    only, so z, ỹ, ∂L/∂y and the partials of a channel are the same bits whatever C is and
    whichever thread owns it. (The bits of a channel count of its own are held to rate_bits by the
    forward test.) The distance of ∂L/∂y to the fp32 definition is printed, not asserted: see
    step_refs.EXTRA_SHAPES."""
    B, h, w, C = shape
    c = S.kernel_case(shape)
    d = S.deltas(c["steps"])
    dd, gb = d.view(-1).to(device), c["g_bits"].to(device)

    def run(y, noise, g_deq, rate):
        pack = rate_pack(rate, device)
        z, y_deq, _ = kernels.step_noise_rate(nhwc(y, device), noise.to(device), dd, pack)
        g_y, part = kernels.step_noise_rate_backward(z, nhwc(g_deq, device), dd, pack, gb)
        return z, y_deq, g_y, part

    full = run(c["y"], c["noise"], c["g_deq"], c["rate"])
    for lo, hi, N in ((0, min(C, 192), 192), (192, C, 128)):
        n = hi - lo
        if n <= 0:
            continue
        wide = [torch.cat([t[:, lo:hi], torch.zeros(B, N - n, h, w)], dim=1)
                for t in (c["y"], c["noise"], c["g_deq"])]
        ref = run(*wide, R.rate_params(N))
        for name, a, b in zip(("z", "y_deq", "g_y", "partials"), full, ref):
            assert torch.equal(a[..., lo:hi], b[..., :n]), (name, lo, hi)
    dz, _ = S.rate_term_fp32(full[0].permute(0, 3, 1, 2).cpu(), c["rate"], c["steps"], c["g_bits"])
    e = R.global_err(nchw(full[2]), S.quantise_backward(c["g_deq"].double(), dz.double(), d.double()))
    print(f"g_y {shape}: {e:.2e} from the fp32 definition")


@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (2, 16, 48), (4, 32, 16)])
def test_grad_recon_images_constant_vector_is_grad_recon(device, B, H, W):
    """One weight for every image is grad_recon's scalar weight: G/B per image (B a power of two,
    so (G/B)/(3HW) and G/(B·3HW) are the same fp32 value) gives the same bits, with and without
    the clamp gradient; different weights scale their images."""
    recon = R.uniform(81, (B, 3, H, W), -0.2, 1.2).to(device)
    x = R.uniform(82, (B, 3, H, W), 0.0, 1.0).to(device)
    g_clip = R.normal(83, (B, 3, H, W)).to(device)
    G = torch.tensor(0.7310585975646973, device=device)
    vec = (G / B).repeat(B)
    for gc in (None, g_clip):
        assert torch.equal(kernels.grad_recon_images(recon, x, vec, gc),
                           kernels.grad_recon(recon, x, G, gc))
    assert torch.equal(kernels.grad_recon_images(recon, x, None, g_clip),
                       kernels.grad_recon(recon, x, None, g_clip))
    wts = torch.arange(1, B + 1, device=device, dtype=torch.float32)
    got = kernels.grad_recon_images(recon, x, wts, g_clip).cpu()
    ref = S.grad_recon_images(recon.cpu().double(), x.cpu().double(), wts.cpu().double(),
                              g_clip.cpu().double())
    assert R.global_err(got, ref) <= R.BARS["grad_recon"]["global"]


# ------------------------------------------------------------------------------ the chain
def chain_inputs():
    B, _, H, W = S.CHAIN_SHAPE
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(3, B, H, W)))
    noise = torch.from_numpy(synth.uniform(4, (B, S.CHAIN_N, H // 16, W // 16), -0.5, 0.5))
    return x, noise


@functools.lru_cache(maxsize=None)
def chain_reference():
    """The fp32 stepped reference's per-image results and the autograd of its loss, computed
    once for the three precisions (read-only)."""
    sd = oracle.state_dict_to_torch(synth.trained_like_state_dict(S.CHAIN_N, S.CHAIN_SEED))
    x, noise = chain_inputs()
    sdp = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out = S.forward(x, sdp, noise, S.CHAIN_STEPS)
    S.loss(out, train.step_lambdas(S.CHAIN_LAM, S.CHAIN_STEPS)).backward()
    return (out["mse"].detach(), out["bpp"].detach(), {k: v.grad for k, v in sdp.items()})


def stepped_step(net, x, noise, steps, lams=None, distortion="mse"):
    lams = train.step_lambdas(S.CHAIN_LAM, steps) if lams is None else lams
    clipped, dist, bpp = net.forward_train(x, noise=noise, steps=steps, distortion=distortion)
    loss = torch.mean(torch.tensor(lams, device=x.device, dtype=torch.float32) * dist + bpp)
    net.zero_grad()
    loss.backward()
    return clipped, dist, bpp, {k: p.grad.clone() for k, p in net.named_parameters()}


def test_chain_against_stepped_reference(device, precision):
    """dist[B], bpp[B] and all 30 gradients of mean(λ_b·mse_b + bpp_b) with steps (2, 8, 19)
    against the fp32 stepped reference's autograd: tests/test_gpu_backward.py's comparator and
    bar for the unstepped step (max|Δ| ≤ 1e-4 · max|ref| per tensor)."""
    net, _ = make(S.CHAIN_N, S.CHAIN_SEED, device)
    x, noise = chain_inputs()
    r_mse, r_bpp, r_grads = chain_reference()
    _, dist, bpp, grads = stepped_step(net, x.to(device), noise.to(device), S.CHAIN_STEPS)
    assert dist.shape == bpp.shape == (x.shape[0],) and dist.dtype == bpp.dtype == torch.float32
    e_mse = ((dist.cpu().double() - r_mse.double()).abs() / r_mse.double().abs()).max().item()
    e_bpp = ((bpp.cpu().double() - r_bpp.double()).abs() / r_bpp.double().abs()).max().item()
    errs = {k: R.global_err(g, r_grads[k]) for k, g in grads.items()}
    print(f"{precision}: mse {e_mse:.2e} bpp {e_bpp:.2e} (bar {S.BARS['mse']:.1e}); "
          f"max grad err {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert len(errs) == 30
    assert e_mse <= S.BARS["mse"] and e_bpp <= S.BARS["bpp"]
    bad = {k: e for k, e in errs.items() if not e < S.GRAD_REL}
    assert not bad, bad


def test_unit_step_is_the_unstepped_forward(device, precision):
    """Every image at index 8: z (= ỹ, Δ = 1) is the unstepped training forward's ỹ bit for bit
    for the same noise, and the mean of bpp_b its bpp."""
    net, _ = make(S.CHAIN_N, S.CHAIN_SEED, device)
    x, noise = (t.to(device) for t in chain_inputs())
    B = x.shape[0]
    with torch.no_grad():
        m = chain.train_mode(precision)
        feats = m.train_analysis(net.Encoder, x)
        y = net.Encoder.y_nhwc(x, m.name, feats=feats)
        ones = torch.ones(B, device=device)
        z, y_deq, _ = kernels.step_noise_rate(y, noise, ones, net.bitEstimator.packed())
    _, y_tilde, bpp0 = net(x, noise=noise)
    assert torch.equal(z.permute(0, 3, 1, 2), y_tilde) and torch.equal(z, y_deq)
    _, _, bpp = net.forward_train(x, noise=noise, steps=8)
    e = abs(bpp.double().sum().item() / B - bpp0.item()) / bpp0.item()
    print(f"{precision}: mean bpp_b vs bpp {e:.2e}")
    assert e <= S.REL


def test_stepped_step_is_reproducible(device, precision):
    net, _ = make(S.CHAIN_N, S.CHAIN_SEED, device)
    x, noise = (t.to(device) for t in chain_inputs())
    a = stepped_step(net, x, noise, S.CHAIN_STEPS)
    b = stepped_step(net, x, noise, S.CHAIN_STEPS)
    for i in range(3):
        assert torch.equal(a[i], b[i]), i
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_batch_independence(device):
    """The gradients of the mean loss over B = 4 are the average of those of its two B = 2
    halves run with the same steps and noise (no image's step leaks into another's)."""
    net, _ = make(S.CHAIN_N, S.CHAIN_SEED, device)
    B, H, W = 4, 32, 48
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(13, B, H, W))).to(device)
    noise = torch.from_numpy(synth.uniform(14, (B, S.CHAIN_N, H // 16, W // 16), -0.5, 0.5)).to(device)
    steps = (0, 19, 8, 31)
    _, dist, bpp, full = stepped_step(net, x, noise, steps)
    halves = [stepped_step(net, x[i:i + 2], noise[i:i + 2], steps[i:i + 2]) for i in (0, 2)]
    errs = {k: R.global_err((halves[0][3][k] + halves[1][3][k]) / 2, full[k]) for k in full}
    print(f"max {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert max(errs.values()) <= S.GRAD_REL, errs
    for i, hv in zip((0, 2), halves):
        assert R.global_err(hv[1], dist[i:i + 2]) <= S.REL
        assert R.global_err(hv[2], bpp[i:i + 2]) <= S.REL


@pytest.mark.parametrize("where", ["encoder", "decoder"])
def test_h3_overflow_is_a_nan_distortion(device, where):
    """tests/test_gpu_h3_range.py's overflowing inputs: an activation that does not fit the h3
    form, in the analysis or in the synthesis half, ends in a NaN distortion of the stepped step
    (the latent between the halves is made without clearing the chain's range flag)."""
    old = kernels.precision()
    kernels.set_precision("h3")
    try:
        net, _ = make(192, 1, device)
        x = torch.from_numpy(synth.to_unit_float(synth.image_u8(5, 2, 64, 96))).to(device)
        with torch.no_grad():
            if where == "encoder":
                net.Encoder.conv1.bias[0] = 1e4
                net.Encoder.gdn1.gamma[0].zero_()
                net.Encoder.gdn1.beta[0] = 0.0
            else:
                net.Decoder.deconv1.bias[0] = 1e4
        _, dist, _ = net.forward_train(x, steps=[3, 12])
        assert kernels.h3_range_overflowed(device)
        assert bool(torch.isnan(dist).all()), dist
    finally:
        kernels.set_precision(old)


def test_ms_ssim_distortion(device):
    """distortion="ms-ssim" with steps: [B] distortions in (0, 1), finite gradients everywhere."""
    net, _ = make(S.CHAIN_N, S.CHAIN_SEED, device)
    B, H, W = 2, 176, 176
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(15, B, H, W))).to(device)
    _, dist, bpp, grads = stepped_step(net, x, None, (4, 14), lams=[64.0, 8.0],
                                       distortion="ms-ssim")
    assert dist.shape == bpp.shape == (B,)
    assert bool(((dist > 0) & (dist < 1)).all()) and bool(torch.isfinite(bpp).all())
    assert len(grads) == 30
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()) and g.abs().max() > 0, k


def test_train_driver_with_steps(device, tmp_path, caplog):
    """train.main with "steps": [lo, hi]: two synthetic steps along the ladder log finite batch
    means and change the parameters of all three modules."""
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"batch_size": 2, "print_freq": 1, "cal_step": 1,
                               "out_channel_N": 128, "train_lambda": 100, "steps": [2, 20]}))
    caplog.set_level(logging.INFO, logger="ImageCompression")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert train.main(["--config", str(cfg), "--synthetic", "--max-steps", "2", "-n", "s"]) == 0
    finally:
        os.chdir(cwd)
    lines = [ln for ln in caplog.text.splitlines() if "Step [" in ln]
    assert len(lines) == 2 and "Step [2/2" in lines[1]
    for ln in lines:
        fields = dict(re.findall(r"\| (Total Loss|PSNR|Bpp|MSE) (\S+) ", ln))
        assert set(fields) == {"Total Loss", "PSNR", "Bpp", "MSE"}, ln
        assert all(math.isfinite(float(v)) for v in fields.values()), ln
    ck = tmp_path / "checkpoints" / "s"
    before = torch.load(ck / "iter_0.pth.tar", map_location="cpu", weights_only=True)
    after = torch.load(ck / "iter_2.pth.tar", map_location="cpu", weights_only=True)
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    weights = {k for k in before if k.endswith(".weight")}
    assert len(before) == 30 and weights <= changed, weights - changed
    assert any(k.startswith("bitEstimator.") for k in changed)
    assert all(torch.isfinite(v).all() for v in after.values())
