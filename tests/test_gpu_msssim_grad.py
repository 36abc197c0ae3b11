"""The differentiable MS-SSIM / SSIM (losses.py → autograd.MsSsimFn / SsimFn → csrc/msssim.hip)
and MS-SSIM as the training distortion, on the GPU.

Inputs: x = a synthetic image batch, y = clamp(x + σ·randn, 0, 1) with σ ∈ {0.05, 0.2}. (At
σ ≤ 0.01 the fp32 reference's own gradient is off by ~1e-3 of max|g| through cancellation, and
independent random pairs can have cs means ≤ 0, NaN in the reference too.)

Truth: a float64 restatement of oracle.ms_ssim / oracle.ssim_and_cs (the reference's fp32 window
and weights, widened), differentiated by torch's CPU autograd. Bar: the error of the fp32 oracle's
own CPU autograd against that truth, max|Δ| / max|g|, measured in the same test; the GPU's error
may be at most 4× it (a different but equally valid summation order, and the FMA filter).
Measured on an MI355X (GPU error / fp32-oracle error, worst over the cases of a test): see
DESIGN.md, "Differentiable MS-SSIM".
"""
import functools
import json
import logging
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from iclr_17_compression_amd import kernels, synth
from iclr_17_compression_amd.losses import MSSSIMLoss, ms_ssim_diff, ssim_diff
from iclr_17_compression_amd.model import ImageCompressor
from oracle import codec_ref as oracle

pytestmark = pytest.mark.gpu

GRAD_REL = 1e-4   # the project's per-tensor bar on a training step's gradients
FACTOR = 4.0


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@functools.lru_cache(maxsize=None)
def pair(seed, B, H, W, sigma):
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(seed, B, H, W)))
    n = torch.randn(x.shape, generator=torch.Generator().manual_seed(1000 + seed))
    return x, (x + sigma * n).clamp(0, 1)


def ssim_and_cs64(X, Y):
    return oracle.ssim_and_cs(X, Y, oracle.gauss_window().to(X.dtype), 1.0)


def ms_ssim_any(X, Y):
    """oracle.ms_ssim in X's dtype (float64: the truth), the fp32 window and weights widened."""
    w = torch.tensor(oracle.MSSSIM_WEIGHTS, dtype=torch.float32).to(X.dtype)
    mcs, s = [], None
    for _ in range(5):
        s, cs = ssim_and_cs64(X, Y)
        mcs.append(cs)
        pad = (X.shape[2] % 2, X.shape[3] % 2)
        X = F.avg_pool2d(X, kernel_size=2, padding=pad)
        Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    mcs = torch.stack(mcs, dim=0)
    return torch.prod((mcs[:-1] ** w[:-1].unsqueeze(1)) * (s ** w[-1]), dim=0)


def cpu_grads(fn, x, y, dtype):
    X = x.detach().clone().to(dtype).requires_grad_(True)   # clone: the shared inputs stay as they are
    Y = y.detach().clone().to(dtype).requires_grad_(True)
    fn(X, Y).backward()
    return X.grad, Y.grad


def gpu_grads(fn, x, y, device, need=(True, True)):
    X = x.detach().clone().to(device).requires_grad_(need[0])
    Y = y.detach().clone().to(device).requires_grad_(need[1])
    fn(X, Y).backward()
    return X.grad, Y.grad


def check_against_truth(tag, gpu_fn, ref_fn, x, y, device):
    """dX and dY of gpu_fn on the GPU against ref_fn in float64; bar 4× the fp32 CPU error."""
    t = cpu_grads(ref_fn, x, y, torch.float64)
    o = cpu_grads(ref_fn, x, y, torch.float32)
    g = gpu_grads(gpu_fn, x, y, device)
    for name, tt, oo, gg in zip(("dX", "dY"), t, o, g):
        assert torch.isfinite(tt).all() and tt.abs().max() > 0
        e_ref, e_gpu = rel_err(oo, tt), rel_err(gg, tt)
        print(f"{tag} {name}: gpu {e_gpu:.3e}  fp32 oracle {e_ref:.3e}  ratio {e_gpu / e_ref:.2f}")
        assert e_gpu <= FACTOR * e_ref, (tag, name, e_gpu, e_ref)


def test_value_is_the_evaluation_kernels(device):
    x, y = pair(1, 2, 177, 183, 0.05)
    xd, yd = x.to(device), y.to(device).requires_grad_(True)
    want = kernels.ms_ssim(yd.detach(), xd)
    got = ms_ssim_diff(yd, xd, size_average=False)
    assert got.requires_grad and torch.equal(got.detach(), want)
    assert torch.equal(ms_ssim_diff(yd.detach(), xd, size_average=False), want)   # no-grad route
    assert torch.equal(ms_ssim_diff(yd, xd).detach(), want.mean())
    assert torch.equal(MSSSIMLoss()(yd, xd).detach(), 1 - want.mean())
    s, cs = ssim_diff(yd, xd, size_average=False, full=True)
    ws, wcs = kernels.ssim(yd.detach(), xd)
    assert torch.equal(s.detach(), ws) and torch.equal(cs.detach(), wcs)


@pytest.mark.parametrize("size_average", [False, True])
@pytest.mark.parametrize("sigma", [0.05, 0.2])
@pytest.mark.parametrize("B,H,W", [(1, 176, 208), (2, 177, 183)])
def test_ms_ssim_gradients(device, B, H, W, sigma, size_average):
    x, y = pair(2, B, H, W, sigma)
    wts = torch.tensor([0.5, 1.5][:B])
    if size_average:
        gpu_fn = lambda X, Y: 1.5 * ms_ssim_diff(X, Y, size_average=True)   # noqa: E731
        ref_fn = lambda X, Y: 1.5 * ms_ssim_any(X, Y).mean()                # noqa: E731
    else:
        gpu_fn = lambda X, Y: (ms_ssim_diff(X, Y, size_average=False) * wts.to(X.device)).sum()  # noqa: E731
        ref_fn = lambda X, Y: (ms_ssim_any(X, Y) * wts.to(X.dtype)).sum()   # noqa: E731
    check_against_truth(f"ms_ssim {B}x3x{H}x{W} σ={sigma} avg={size_average}", gpu_fn, ref_fn,
                        x, y, device)


def test_partial_needs(device):
    x, y = pair(2, 2, 177, 183, 0.2)
    wts = torch.tensor([0.5, 1.5], device=device)
    fn = lambda X, Y: (ms_ssim_diff(X, Y, size_average=False) * wts).sum()   # noqa: E731
    dx, dy = gpu_grads(fn, x, y, device)
    dx1, none_y = gpu_grads(fn, x, y, device, need=(True, False))
    none_x, dy1 = gpu_grads(fn, x, y, device, need=(False, True))
    assert none_x is None and none_y is None
    assert torch.equal(dx1, dx) and torch.equal(dy1, dy)
    sfn = lambda X, Y: sum((t * wts).sum() for t in ssim_diff(X, Y, size_average=False, full=True))  # noqa: E731
    x, y = pair(3, 2, 28, 20, 0.2)
    dx, dy = gpu_grads(sfn, x, y, device)
    dx1, none_y = gpu_grads(sfn, x, y, device, need=(True, False))
    none_x, dy1 = gpu_grads(sfn, x, y, device, need=(False, True))
    assert none_x is None and none_y is None
    assert torch.equal(dx1, dx) and torch.equal(dy1, dy)


@pytest.mark.parametrize("a,c", [(1.0, 0.0), (0.0, 1.0), (1.0, 0.7)])
@pytest.mark.parametrize("sigma", [0.05, 0.2])
@pytest.mark.parametrize("B,H,W", [(1, 11, 11), (1, 12, 75), (2, 28, 20)])
def test_ssim_gradients(device, B, H, W, sigma, a, c):
    """Upstream gradients on ssim alone, cs alone (the other's gradient is then absent, not
    zero) and both."""
    x, y = pair(3, B, H, W, sigma)
    wts = torch.tensor([0.5, 1.5][:B])

    def combine(s, cs, w):
        terms = ([a * (s * w).sum()] if a else []) + ([c * (cs * w).sum()] if c else [])
        return sum(terms)

    gpu_fn = lambda X, Y: combine(*ssim_diff(X, Y, size_average=False, full=True), wts.to(X.device))  # noqa: E731
    ref_fn = lambda X, Y: combine(*ssim_and_cs64(X, Y), wts.to(X.dtype))   # noqa: E731
    check_against_truth(f"ssim {B}x3x{H}x{W} σ={sigma} g=({a},{c})", gpu_fn, ref_fn, x, y, device)


def test_backward_is_deterministic(device):
    x, y = pair(2, 2, 177, 183, 0.05)
    fn = lambda X, Y: 1 - ms_ssim_diff(X, Y)   # noqa: E731
    a, b = gpu_grads(fn, x, y, device), gpu_grads(fn, x, y, device)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    x, y = pair(3, 2, 28, 20, 0.05)
    fn = lambda X, Y: sum(ssim_diff(X, Y, full=True))   # noqa: E731
    a, b = gpu_grads(fn, x, y, device), gpu_grads(fn, x, y, device)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------- training step
LAM = 100.0


def make(N, seed, device):
    sd = synth.trained_like_state_dict(N, seed)
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(device).train(), oracle.state_dict_to_torch(sd)


def step_inputs(N):
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(3, 2, 176, 176)))
    noise = torch.from_numpy(synth.uniform(4, (2, N, 11, 11), -0.5, 0.5))
    return x, noise


def oracle_step(N, dtype):
    sd = oracle.state_dict_to_torch(synth.trained_like_state_dict(N, 2))
    x, noise = step_inputs(N)
    sdp = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    clipped, _, bpp, _, _ = oracle.codec_forward(x.to(dtype), sdp, training=True,
                                                 noise=noise.to(dtype))
    ms = oracle.ms_ssim(clipped, x) if dtype == torch.float32 else ms_ssim_any(clipped, x.to(dtype))
    dist = 1 - ms.mean()
    loss = LAM * dist + bpp
    loss.backward()
    grads = {k: v.grad for k, v in sdp.items()}
    assert len(grads) == 30 and all(g is not None and torch.isfinite(g).all() for g in grads.values())
    return loss.item(), dist.item(), bpp.item(), grads


@functools.lru_cache(maxsize=None)
def reference_step(N):
    """The fp32 oracle's MS-SSIM training step on the CPU (the reference), and per tensor the
    fp32 oracle's own gradient error against the same graph in float64; once per N."""
    ref = oracle_step(N, torch.float32)
    truth = oracle_step(N, torch.float64)
    own = {k: rel_err(ref[3][k], truth[3][k]) for k in truth[3]}
    return (*ref, own, truth[3])


@pytest.fixture(params=["h3", "x6", "fp32"])
def precision(request):
    old = kernels.precision()
    kernels.set_precision(request.param)
    yield request.param
    kernels.set_precision(old)


@pytest.mark.parametrize("N", [128, 192])
def test_msssim_train_step_all_grads(device, precision, N):
    """loss = 100·(1 − MS-SSIM(clipped, x)) + bpp at B=2, 176×176 against the fp32 oracle's CPU
    autograd: the loss terms within 1e-5 relative, all 30 gradients within GRAD_REL = 1e-4 per
    tensor. The level-0 cs means of these weights are 0.006-0.010 and 48 % of the pixels are
    clipped, so the loss is ill-conditioned; where a tensor misses 1e-4 its bar is 4× the fp32
    oracle's own error on that tensor against the same graph in float64. Measured on an MI355X:
    at N=128 every tensor is within 5.1e-5 of the fp32 oracle in every mode. At N=192 the fp32
    oracle itself is 2.5e-4 to 2.4e-3 from float64 on the 19 encoder / decoder tensors
    (Decoder.deconv3.weight 2.4e-3); the fp32 and x6 modes differ from it by that much (worst
    2.44e-3, 1.00× its own error) and are within 4.6e-5 / 8.7e-5 of float64; the h3 mode lands on
    the fp32 oracle's side (within 1.4e-5 of it except Decoder.deconv3.bias at 1.38e-4, where the
    oracle's own error is 1.7e-3)."""
    net, _ = make(N, 2, device)
    x, noise = step_inputs(N)
    clipped, dist, bpp = net.forward_train(x.to(device), noise=noise.to(device),
                                           distortion="ms-ssim")
    loss = LAM * dist + bpp
    net.zero_grad()
    loss.backward()
    r_loss, r_dist, r_bpp, r_grads, own, t_grads = reference_step(N)
    print(f"N={N} {precision}: 1-ms {dist.item():.7f} vs {r_dist:.7f}, bpp {bpp.item():.6f} vs "
          f"{r_bpp:.6f}, loss {loss.item():.6f} vs {r_loss:.6f}")
    errs = {k: rel_err(p.grad, r_grads[k]) for k, p in net.named_parameters()}
    vs64 = {k: rel_err(p.grad, t_grads[k]) for k, p in net.named_parameters()}
    for k in errs:
        print(f"  {k}: vs fp32 oracle {errs[k]:.2e}  fp32 oracle's own {own[k]:.2e}  "
              f"vs float64 {vs64[k]:.2e}")
    print(f"  worst: vs fp32 oracle {max(errs.values()):.2e}, vs float64 {max(vs64.values()):.2e}")
    assert dist.item() == pytest.approx(r_dist, rel=1e-5)
    assert bpp.item() == pytest.approx(r_bpp, rel=1e-5)
    assert loss.item() == pytest.approx(r_loss, rel=1e-5)
    bad = {k: (e, own[k]) for k, e in errs.items() if not (e < GRAD_REL or e <= FACTOR * own[k])}
    assert len(errs) == 30 and not bad, bad


def test_default_distortion_is_the_mse_step(device):
    """forward_train(x) and forward_train(x, distortion="mse") are the same step, bitwise."""
    N = 128
    net, _ = make(N, 2, device)
    x = torch.from_numpy(synth.to_unit_float(synth.image_u8(3, 2, 64, 64))).to(device)
    noise = torch.from_numpy(synth.uniform(4, (2, N, 4, 4), -0.5, 0.5)).to(device)
    runs = []
    for kw in ({}, {"distortion": "mse"}):
        net.zero_grad()
        clipped, mse, bpp = net.forward_train(x, noise=noise, **kw)
        (8192 * mse + bpp).backward()
        runs.append((clipped, mse, bpp, {k: p.grad.clone() for k, p in net.named_parameters()}))
    for i in range(3):
        assert torch.equal(runs[0][i], runs[1][i])
    for k in runs[0][3]:
        assert torch.equal(runs[0][3][k], runs[1][3][k]), k
    with pytest.raises(kernels.Iclr17Error, match="distortion"):
        net.forward_train(x, noise=noise, distortion="psnr")


def test_train_driver_msssim(device, tmp_path, caplog):
    """train.main with "distortion": "ms-ssim": two synthetic steps log finite values with the
    MS-SSIM field and change the parameters."""
    from iclr_17_compression_amd import train
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"batch_size": 2, "print_freq": 1, "cal_step": 1,
                               "out_channel_N": 128, "train_lambda": 100,
                               "distortion": "ms-ssim"}))
    caplog.set_level(logging.INFO, logger="ImageCompression")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert train.main(["--config", str(cfg), "--synthetic", "--max-steps", "2", "-n", "m"]) == 0
    finally:
        os.chdir(cwd)
    lines = [ln for ln in caplog.text.splitlines() if "Step [" in ln]
    assert len(lines) == 2 and "Step [2/2" in lines[1]
    for ln in lines:
        fields = dict(re.findall(r"\| (Total Loss|PSNR|Bpp|MSE|MS-SSIM) (\S+) ", ln))
        assert set(fields) == {"Total Loss", "PSNR", "Bpp", "MSE", "MS-SSIM"}, ln
        assert all(math.isfinite(float(v)) for v in fields.values()), ln
    ck = tmp_path / "checkpoints" / "m"
    before = torch.load(ck / "iter_0.pth.tar", map_location="cpu", weights_only=True)
    after = torch.load(ck / "iter_2.pth.tar", map_location="cpu", weights_only=True)
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    weights = {k for k in before if k.endswith(".weight")}
    assert len(before) == 30 and len(weights) == 6 and weights <= changed, weights - changed
    assert any(k.startswith("bitEstimator.") for k in changed)
    assert all(torch.isfinite(v).all() for v in after.values())
