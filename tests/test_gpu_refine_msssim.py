"""Latent refinement for MS-SSIM on the GPU: the saving forward and the backward of
MS-SSIM over a canvas batch (csrc/msssim.hip) against the Uniform gradient path on each image alone,
bit for bit; refine_keep_msssim against the host's arithmetic; and
``compress_images(refine_lambda=msssim_lambda(…))`` against its contract, recomputed from the blobs
alone. The weights are synthetic: nothing here is a statement about quality.

Every figure is printed before it is asserted (run with -s to read them)."""
import numpy as np
import pytest
import torch

import rdo_refs as R
import refine_refs as F
from iclr_17_compression_amd import codec, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor

pytestmark = pytest.mark.gpu

# One canvas, 176×272 (tests/test_gpu_msssim_target.py's): odd and even sizes at every level;
# Ho = 151 gives 10 row tiles and 166 gives 11; Wo = 256 gives 4 column tiles and 257 gives 5.
CANVAS = (176, 272)
SIZES = [(161, 161), (176, 272), (170, 267), (175, 266)]
G = [0.75, -1.5, 2250.0, -0.03125 * 3]          # distinct upstream gradients, two of them negative


def unit(a, device):
    """evaluate_images' conversion of an 8-bit HWC image: [1,3,H,W] fp32, /255 on the device."""
    return (torch.from_numpy(np.ascontiguousarray(a)).to(device).permute(2, 0, 1).float() / 255)[None].contiguous()


def pack(images):
    sizes = [im.size for im in images]
    offsets = [int(o) for o in np.cumsum([0] + sizes[:-1])]
    return (torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])), offsets,
            [im.shape[:2] for im in images])


def same_bits(a, b):
    """fp32 tensors equal as bit patterns: −0.0 is not +0.0, NaN equals the same NaN."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run(recon, ref, offsets, shapes, g, device):
    """fwd_saved + bwd of one canvas batch → (values, status, d_recon)."""
    B, _, Hc, Wc = recon.shape
    desc = kernels._image_desc("test", ref.numel(), offsets, shapes, (Hc, Wc)).to(device)
    ws = kernels.image_msssim_grad_workspace(B, Hc, Wc, device)
    values, status = kernels.image_msssim_fwd_saved(recon, ref, desc, ws)
    d = kernels.image_msssim_bwd(recon, ref, desc, ws, torch.tensor(g, dtype=torch.float32, device=device))
    return values.clone(), int(status.item()), d


@pytest.fixture(scope="module")
def case(device):
    """test_gpu_msssim_target.py's case: recon random fp32 in [−0.1, 1.1] (the gate fires), 1e30 in
    the padding, the originals recon's own 8-bit image ± 20 levels. The reference gradient comes
    from the Uniform gradient path, one image at a time, once: X_b = the egress bytes · fl(1/255),
    Y_b = the original · fl(1/255), ms_ssim_fwd_saved and ms_ssim_bwd with g_b, then the gate in
    torch on recon's own values; zeros (+0.0) on the rest of the canvas."""
    Hc, Wc = CANVAS
    recon = synth.uniform(41, (len(SIZES), 3, Hc, Wc), -0.1, 1.1)
    refs = []
    for b, (H, W) in enumerate(SIZES):
        own = np.rint(np.clip(recon[b, :, :H, :W], 0.0, 1.0) * np.float32(255.0)).astype(np.int64)
        noise = synth.image_u8(50 + b, 1, H, W)[0].astype(np.int64) % 41 - 20
        refs.append(np.ascontiguousarray(np.clip(own + noise, 0, 255).astype(np.uint8).transpose(1, 2, 0)))
        recon[b, :, H:, :] = 1e30
        recon[b, :, :, W:] = 1e30
    recon = torch.from_numpy(recon).to(device)
    ref, offsets, shapes = pack(refs)
    assert any(o % 4 for o in offsets)                      # natural, unaligned byte offsets
    dst, _ = kernels.image_egress(recon, offsets, shapes)
    want = torch.zeros_like(recon)
    gated = 0
    for b, (o, (H, W), r) in enumerate(zip(offsets, shapes, refs)):
        out8 = dst.numpy()[o:o + 3 * H * W].reshape(H, W, 3)
        X, Y = unit(out8, device), unit(r, device)
        _, ws = kernels.ms_ssim_fwd_saved(X, Y, want_dy=False)
        gb = torch.tensor([G[b]], dtype=torch.float32, device=device)
        d, _ = kernels.ms_ssim_bwd(X, Y, ws, gb, saved_dy=False, want_dy=False)
        v = recon[b, :, :H, :W]
        shut = ((v < 0) & (d[0] > 0)) | ((v > 1) & (d[0] < 0))
        gated += int(shut.sum())
        want[b, :, :H, :W] = torch.where(shut, torch.zeros_like(d[0]), d[0])
    assert gated > 0 and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    return recon, refs, ref.to(device), offsets, shapes, want


# ------------------------------------------------------------------ 1, 2. value and gradient
def test_value_is_image_msssim(device, case):
    recon, refs, ref, offsets, shapes, _ = case
    values, status, _ = run(recon, ref, offsets, shapes, G, device)
    want = kernels.image_msssim(recon, offsets, shapes, ref)
    print("fwd_saved:", [f"{float(v):.9g}" for v in values.cpu()], "image_msssim:",
          [f"{float(v):.9g}" for v in want])
    assert values.dtype == torch.float32 and status == 0
    assert torch.equal(values.cpu(), want)


def test_gradient_bit_for_bit(device, case):
    recon, refs, ref, offsets, shapes, want = case
    _, _, d = run(recon, ref, offsets, shapes, G, device)
    for b, (H, W) in enumerate(shapes):
        inside = d[b, :, :H, :W]
        print(f"image {b} {H}x{W}: max |d| {float(inside.abs().max()):.3e}, "
              f"differing elements {int((inside != want[b, :, :H, :W]).sum())}")
        assert torch.equal(inside, want[b, :, :H, :W])
        # the rest of the canvas: +0.0 exactly, whatever recon's padding holds
        assert int(d[b, :, H:, :].contiguous().view(torch.int32).abs().max() if H < CANVAS[0] else 0) == 0
        assert int(d[b, :, :, W:].contiguous().view(torch.int32).abs().max() if W < CANVAS[1] else 0) == 0
    assert same_bits(d, want)


# ------------------------------------------------------------------ 3. batch independence
def test_batch_independence_and_determinism(device, case):
    recon, refs, ref, offsets, shapes, want = case
    values, _, d = run(recon, ref, offsets, shapes, G, device)
    again_v, _, again = run(recon, ref, offsets, shapes, G, device)
    assert same_bits(again, d) and same_bits(again_v, values)
    order = [3, 1, 0, 2]
    ref_o, offsets_o, shapes_o = pack([refs[b] for b in order])
    v_o, st_o, d_o = run(recon[order].contiguous(), ref_o.to(device), offsets_o, shapes_o,
                         [G[b] for b in order], device)
    assert st_o == 0 and same_bits(v_o, values[order]) and same_bits(d_o, d[order])
    for b in range(len(SIZES)):
        ref_1, offsets_1, shapes_1 = pack([refs[b]])
        v_1, st_1, d_1 = run(recon[b:b + 1].contiguous(), ref_1.to(device), offsets_1, shapes_1,
                             [G[b]], device)
        assert st_1 == 0 and same_bits(v_1, values[b:b + 1]) and same_bits(d_1, d[b:b + 1]), b


# ------------------------------------------------------------------ 4. padding and status
def test_padding_and_status(device, case):
    recon, refs, ref, offsets, shapes, want = case
    values, _, d = run(recon, ref, offsets, shapes, G, device)
    H, W = shapes[2]
    pad = recon.clone()
    pad[2, :, H:, :] = float("nan")
    pad[2, :, :, W:] = float("inf")
    pad[0, :, shapes[0][0]:, :] = float("-inf")
    v_p, st_p, d_p = run(pad, ref, offsets, shapes, G, device)
    assert st_p == 0 and same_bits(v_p, values) and same_bits(d_p, d)
    inside = recon.clone()
    inside[2, 1, H - 1, W - 1] = float("nan")     # the last pixel of the image's own region
    v_i, st_i, d_i = run(inside, ref, offsets, shapes, G, device)
    assert st_i == 1
    others = [0, 1, 3]
    assert same_bits(v_i[others], values[others]) and same_bits(d_i[others], d[others])
    assert int(d_i[2, :, H:, :].contiguous().view(torch.int32).abs().max()) == 0
    assert int(d_i[2, :, :, W:].contiguous().view(torch.int32).abs().max()) == 0
    # the status is cleared by the next call
    assert run(recon, ref, offsets, shapes, G, device)[1] == 0


# ------------------------------------------------------------------ 5. shared kernels unchanged
# The fp32 bits of kernels.ms_ssim_bwd's dx (g = [1, −0.375], no dY) on the pair below: eight fixed
# elements of the flattened [2,3,176,192] tensor, the sum of all bit patterns and their sum weighted
# by (index mod 65521) + 1, both modulo 2^64. From a run of the commit before ssim_level_bwd_kernel
# became a body over the extent sources (its library built from that commit's sources, on an
# MI355X): the shared kernels keep the existing entries' results.
PARENT_DX_AT = [0, 1, 191, 33600, 33791, 101383, 181305, 202751]
PARENT_DX_BITS = [0x308CCE58, 0x308C1153, 0x31983EE1, 0x30FBF49B, 0x3010888E, 0x2DBD2E80,
                  0xB7A41E14, 0xAF0F2AC8]
PARENT_DX_SUM = 0x16BB5486C1595
PARENT_DX_WEIGHTED = 0xB117F2B271B584A7
PARENT_VALUE_BITS = [0x3F78EE43, 0x3F7863C4]


def test_existing_ms_ssim_bwd_unchanged(device):
    x = synth.uniform(5, (2, 3, 176, 192))
    y = np.clip(x + np.float32(0.25) * (synth.uniform(6, x.shape) - np.float32(0.5)), 0.0, 1.0)
    assert x.dtype == y.dtype == np.float32
    xt, yt = torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)
    g = torch.tensor([1.0, -0.375], dtype=torch.float32, device=device)
    out, ws = kernels.ms_ssim_fwd_saved(xt, yt, want_dy=False)
    dx, _ = kernels.ms_ssim_bwd(xt, yt, ws, g, saved_dy=False, want_dy=False)
    w = dx.cpu().numpy().view(np.uint32).reshape(-1).astype(np.uint64)
    at = (np.arange(w.size, dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)
    got = ([int(w[i]) for i in PARENT_DX_AT], int(w.sum(dtype=np.uint64)), int((w * at).sum(dtype=np.uint64)))
    print("dx bits:", [hex(v) for v in got[0]], hex(got[1]), hex(got[2]))
    assert [int(v) for v in out.cpu().numpy().view(np.uint32)] == PARENT_VALUE_BITS
    assert got == (PARENT_DX_BITS, PARENT_DX_SUM, PARENT_DX_WEIGHTED)


# ------------------------------------------------------------------ 6. refine_keep_msssim
def levels(seed, shape):
    """Integer-valued fp32 latents."""
    return torch.round(torch.from_numpy(np.random.default_rng(seed).normal(0.0, 4.0, shape).astype(np.float32)))


def test_refine_keep_msssim(device):
    """B = 4: improved, equal (not copied), worse, NaN MS-SSIM (not copied); then a quantiser status
    and a reconstruction status, which keep nothing. J is codec.refine_objective_msssim's, exactly."""
    B = 4
    lam = [8.0, 8.0, 100.0, 8.0]
    sizes = [(161, 177), (176, 192), (169, 180), (161, 161)]
    bits = [1000.0, 2000.0, 3000.0, 4000.0]
    ms = [float(np.float32(v)) for v in (0.9123, 0.8765, 0.95, float("nan"))]
    J = [codec.refine_objective_msssim(b, m, l, H, W) for b, m, l, (H, W) in zip(bits, ms, lam, sizes)]
    assert J[0] == 1000.0 + (8.0 * float(161 * 177)) * (1.0 - ms[0]) and np.isnan(J[3])
    best_J0 = [float(np.nextafter(J[0], np.inf)), J[1], float(np.nextafter(J[2], -np.inf)), 1e30]

    def on(v, dt):
        return torch.tensor(v, dtype=dt, device=device)

    y_hat = levels(5, (B, 3, 4, 128)).to(device)
    old = levels(6, (B, 3, 4, 128)).to(device)

    def keep(qstatus=(0, 0, 0, 0), rstatus=0):
        st = {"best_J": on(best_J0, torch.float64), "best_iter": on([0, 1, 2, 0], torch.int32),
              "best_bits": on([1.0, 2.0, 3.0, 4.0], torch.float64),
              "best_ms": on([0.1, 0.2, 0.3, 0.4], torch.float32), "best": old.clone(),
              "flag": on([9, 9, 9, 9], torch.int32)}
        kernels.refine_keep_msssim(on(bits, torch.float64), on(ms, torch.float32),
                                   on(lam, torch.float64),
                                   on([float(H * W) for H, W in sizes], torch.float64),
                                   on(list(qstatus), torch.int32), on([rstatus], torch.int32), y_hat,
                                   5, st["best_J"], st["best_iter"], st["best_bits"], st["best_ms"],
                                   st["best"], st["flag"])
        return st

    st = keep()
    print("J", J, "best_J", st["best_J"].tolist())
    assert st["flag"].tolist() == [1, 0, 0, 0]
    assert st["best_J"].tolist() == [J[0], best_J0[1], best_J0[2], 1e30]     # J[0]: the host's, exactly
    assert st["best_iter"].tolist() == [5, 1, 2, 0]
    assert st["best_bits"].tolist() == [1000.0, 2.0, 3.0, 4.0]
    assert st["best_ms"].tolist() == [ms[0]] + [float(np.float32(v)) for v in (0.2, 0.3, 0.4)]
    assert torch.equal(st["best"][0], y_hat[0]) and torch.equal(st["best"][1:], old[1:])   # only the flagged
    for kw in ({"qstatus": (2, 0, 0, 0)}, {"rstatus": 1}):
        st = keep(**kw)
        assert st["flag"].tolist() == [0, 0, 0, 0] and torch.equal(st["best"], old)
        assert st["best_J"].tolist() == best_J0 and st["best_iter"].tolist() == [0, 1, 2, 0]


# ------------------------------------------------------------------ 7-9. the loop and the codec
TARGET_SIZES = [(161, 177), (176, 192), (169, 180)]       # one canvas, 176×192
ITERS = 5
# chosen on these synthetic weights from λ ∈ {8, 64, 512} × refine_lr ∈ {0.05, 0.2} at K = 5 (every
# pair kept a refined latent for every image; test_refined_blobs' docstring has the figures)
LAMBDA, LR = 64.0, 0.05


@pytest.fixture(scope="module")
def net(device):
    n = ImageCompressor(out_channel_N=F.E2E_N)
    sd = synth.trained_like_state_dict(F.E2E_N, F.E2E_SEED)
    n.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return n.to(device).eval()


@pytest.fixture(scope="module")
def images():
    return [R.smooth(30 + k, H, W) for k, (H, W) in enumerate(TARGET_SIZES)]


@pytest.fixture(params=["h3", "x6", "fp32"])
def precision(request):
    with kernels.precision_scope(request.param):
        yield request.param


def image_bits(y_hat_nhwc, pack_, step):
    """The existing per-image estimate: rate_bits of ŷ on the step pack of Δ."""
    sp = kernels.pack_rate_step(pack_, y_hat_nhwc.shape[3], codec.step_size(step))
    per, _ = kernels.reduce_partials(kernels.rate_bits(y_hat_nhwc.permute(0, 3, 1, 2), sp))
    return per[0].item()


def blob_objective(net, blob, image, lam, device):
    """J of a blob from the blob alone: its decoded ŷ through the existing rate estimate, its
    decoded pixels through kernels.ms_ssim of the image alone against its original."""
    head, step = codec.parse_blob(blob)
    Hc, Wc = codec.canvas(head.H, head.W)
    dec = net.decompress([blob[codec.HEADER.size:]], (Hc // 16, Wc // 16), streams_per_image=head.P,
                         K=head.K, step=step)
    bits = image_bits(dec["y_hat"].permute(0, 2, 3, 1).contiguous(), net.bitEstimator.packed(), step)
    pixels = net.decompress_images([blob])[0]
    ms = float(kernels.ms_ssim(unit(pixels, device), unit(image, device))[0])
    return codec.refine_objective_msssim(bits, ms, lam, head.H, head.W), bits, ms, pixels


def test_refined_blobs(device, net, images, precision):
    """The contract, recomputed from the blobs alone. λ = 64, refine_lr = 0.05, K = 5 on the
    synthetic N = 128 weights at index 8. Observed on an MI355X: refine_kept = [5, 5, 5] in h3, x6
    and fp32; MS-SSIM 0.037 / 0.043 / 0.034 → 0.091 / 0.107 / 0.092 and the estimated bits 0.3–0.5 %
    lower (these weights are untrained: the values say that the gradient's sign and scale are
    right, nothing about quality). λ ∈ {8, 64, 512} × refine_lr ∈ {0.05, 0.2} all kept [5, 5, 5]."""
    lam = codec.msssim_lambda(LAMBDA)
    kw = {"step": F.E2E_STEP}
    plain = net.compress_images(images, **kw)
    assert net.compress_images(images, refine=0, refine_lambda=lam, **kw) == plain
    kw.update(refine=ITERS, refine_lambda=lam, refine_lr=LR)
    stats = {}
    blobs = net.compress_images(images, stats=stats, **kw)
    assert net.compress_images(images, **kw) == blobs
    assert stats["refine_distortion"] == ["ms-ssim"] * 3 and stats["refine_iters"] == [ITERS] * 3
    rows = net.evaluate_images(images, want_msssim=True, **kw)
    decoded = net.decompress_images(blobs)
    for i, (blob, im) in enumerate(zip(blobs, images)):
        assert blob[:4] == b"I17Q" and codec.parse_blob(blob)[1] == F.E2E_STEP
        J, bits, ms, pixels = blob_objective(net, blob, im, LAMBDA, device)
        Jp, bits_p, ms_p, _ = blob_objective(net, plain[i], im, LAMBDA, device)
        print(f"{precision} image {i}: kept {stats['refine_kept'][i]}, J {J!r} (bits {bits!r}, ms {ms!r}) "
              f"plain {Jp!r} (bits {bits_p!r}, ms {ms_p!r})")
        assert stats["objective"][i] == J and stats["objective_plain"][i] == Jp
        assert J <= Jp
        assert stats["ms_ssim"][i] == ms == rows[i]["ms_ssim"] and stats["ms_ssim_plain"][i] == ms_p
        assert 0 <= stats["refine_kept"][i] <= ITERS
        assert (blob == plain[i]) == (stats["refine_kept"][i] == 0)
        assert np.array_equal(decoded[i], pixels)           # decompress_images: the judged decode
        assert rows[i]["objective"] == J and rows[i]["refine_distortion"] == "ms-ssim"
        assert rows[i]["ms_ssim_plain"] == ms_p and rows[i]["bytes"] == len(blob)
    assert max(stats["refine_kept"]) > 0
    # a plain λ of the same call reports exactly today's keys
    stats = {}
    net.compress_images(images, stats=stats, step=F.E2E_STEP, refine=1, refine_lambda=LAMBDA)
    assert sorted(stats) == sorted(["reencodes", "refine_kept", "objective", "objective_plain",
                                    "refine_iters"])


def test_diverging_run_is_the_plain_blob(device, net, images, precision):
    stats = {}
    blobs = net.compress_images(images, step=F.E2E_STEP, refine=ITERS,
                                refine_lambda=codec.msssim_lambda(LAMBDA), refine_lr=1e6, stats=stats)
    assert blobs == net.compress_images(images, step=F.E2E_STEP)
    assert stats["refine_kept"] == [0, 0, 0]
    assert stats["objective"] == stats["objective_plain"] and stats["ms_ssim"] == stats["ms_ssim_plain"]


def test_lambda_zero_lowers_the_estimated_bits(device, net, images, precision):
    plain = net.compress_images(images, step=F.E2E_STEP)
    stats = {}
    blobs = net.compress_images(images, step=F.E2E_STEP, refine=ITERS,
                                refine_lambda=codec.msssim_lambda(0), refine_lr=LR, stats=stats)
    for i, im in enumerate(images):
        _, bits, _, _ = blob_objective(net, blobs[i], im, 0.0, device)
        _, bits_p, _, _ = blob_objective(net, plain[i], im, 0.0, device)
        print(f"{precision} image {i}: bits {bits!r} plain {bits_p!r} kept {stats['refine_kept'][i]}")
        assert bits <= bits_p and stats["objective"][i] == bits
    assert max(stats["refine_kept"]) > 0


def test_loop_has_no_host_synchronisation(device, net, images, precision):
    """codec.refine_loop with the MS-SSIM objective under torch's sync debug mode, after one run
    that builds the packed layouts; the second run gives the first one's bits."""
    ims = images[:2]
    packed, offsets, shapes = codec.upload_packed(ims, device)
    Hc, Wc = codec.canvas(*shapes[0])
    y = net.latents(kernels.image_ingest(packed, offsets, shapes, (Hc, Wc)))
    desc = kernels._image_desc("refine", packed.numel(), offsets, shapes, (Hc, Wc)).to(device)
    steps = torch.tensor([codec.step_size(8), codec.step_size(11)], device=device)
    lam = torch.tensor([LAMBDA, 8.0], dtype=torch.float64, device=device)
    area = torch.tensor([float(H * W) for H, W in shapes], dtype=torch.float64, device=device)
    g = (-(lam * area)).float()
    net._warm_packs(backward=True, mode=precision)
    net._warm_packs(mode=precision)
    args = (net, y, steps, lam, g, packed, desc, 3, LR, precision)
    first = codec.refine_loop(*args, area=area)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = codec.refine_loop(*args, area=area)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert second.best_iter.min().item() >= 0 and bool(torch.isfinite(second.best_J).all())
    assert second.best_sse.dtype == torch.float32               # the best iterate's MS-SSIM
    q_hat, _ = kernels.quantise_steps(y, steps)
    assert torch.equal(second.plain, q_hat)                   # iteration 0 is the plain quantiser
