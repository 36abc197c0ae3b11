"""Latent refinement on the GPU (csrc/refine.hip and the layers above it): the three
kernels against the existing kernels (bit for bit), torch expressions and the float64 references
of tests/refine_refs.py, and ``compress_images(refine=…)`` against its contract, recomputed from
the blobs alone. The weights are synthetic: nothing here is a statement about quality.

Every figure is printed before it is asserted (run with -s to read them)."""
import numpy as np
import pytest
import torch

import backward_refs as R
import refine_refs as F
import step_refs as S
from iclr_17_compression_amd import codec, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor

pytestmark = pytest.mark.gpu


def nhwc(t, device):
    return t.permute(0, 2, 3, 1).contiguous().to(device)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def rate_pack(rate, device):
    return kernels.pack_rate([rate[k].to(device) for k in S.RATE_ORDER])


def image_bits(y_hat_nhwc, pack, indices):
    """The existing per-image estimate: rate_bits of image b's ŷ on the step pack of its Δ."""
    C = y_hat_nhwc.shape[3]
    out = []
    for b, s in enumerate(indices):
        sp = kernels.pack_rate_step(pack, C, codec.step_size(s))
        per, _ = kernels.reduce_partials(kernels.rate_bits(y_hat_nhwc[b:b + 1].permute(0, 3, 1, 2), sp))
        out.append(per[0].item())
    return out


# ------------------------------------------------------------------ 1. refine_grad_recon
def test_refine_grad_recon(device):
    """B = 2 on a 32×48 canvas: a ragged 17×33 image and a full one, both at odd byte offsets.
    Bit for bit torch's fp32 wt·(2·(recon − ref/255)); exact zeros on the padding."""
    ims = [np.ascontiguousarray(synth.image_u8(31 + k, 1, H, W)[0].transpose(1, 2, 0))
           for k, (H, W) in enumerate(((17, 33), (32, 48)))]
    offsets = [1, 2 + ims[0].size]          # 1 and 1685: a byte of slack before each image
    assert all(o % 2 == 1 for o in offsets)
    flat = np.zeros(offsets[1] + ims[1].size + 3, dtype=np.uint8)
    for o, im in zip(offsets, ims):
        flat[o:o + im.size] = im.reshape(-1)
    ref = torch.from_numpy(flat).to(device)
    shapes = [im.shape[:2] for im in ims]
    desc = kernels._image_desc("refine", ref.numel(), offsets, shapes, (32, 48)).to(device)
    recon = R.uniform(41, (2, 3, 32, 48), -0.2, 1.2).to(device)
    wt = torch.tensor([650.25 / 3.0, 0.75], dtype=torch.float32, device=device)
    g = kernels.refine_grad_recon(recon, ref, desc, wt)
    want = torch.zeros_like(recon)
    for b, im in enumerate(ims):
        H, W = im.shape[:2]
        # ref/255 is the ingest's IEEE division; torch divides by a scalar on the GPU by
        # multiplying with its reciprocal, so the quotient is taken on the host
        x = (torch.from_numpy(im).permute(2, 0, 1).float() / 255).to(device)
        want[b, :, :H, :W] = wt[b] * (2.0 * (recon[b, :, :H, :W] - x))
    assert torch.equal(g, want)
    assert bool((g[0, :, 17:, :] == 0).all()) and bool((g[0, :, :, 33:] == 0).all())
    assert torch.equal(kernels.refine_grad_recon(recon, ref, desc, wt), g)
    ref64 = F.grad_recon(recon.double().cpu(), ims, wt.double().cpu())
    print(f"grad_recon vs float64: {R.global_err(g, ref64):.2e}")


# ------------------------------------------------------------------ 2. refine_step
def step_inputs(shape, device):
    c = F.step_case(shape)
    t = {k: nhwc(c[k], device) for k in ("y", "g_deq", "m", "v")}
    t["steps"] = S.deltas(F.STEP_INDICES).view(-1).to(device)
    t["pack"] = rate_pack(c["rate"], device)
    return t


def run_step(t, step, sel=slice(None), y=None, g_out=True):
    """One refine_step on copies → dict of everything it wrote."""
    y = (t["y"] if y is None else y)[sel].clone()
    steps = t["steps"][sel].contiguous()
    B = y.shape[0]
    y_hat, _ = kernels.quantise_steps(t["y"][sel].contiguous(), steps)   # ŷ of the iterate before
    m, v = t["m"][sel].clone(), t["v"][sel].clone()
    out = {"y_hat_in": y_hat.clone(), "y_deq": torch.empty_like(y),
           "status": torch.full((B,), 7, device=y.device, dtype=torch.int32),
           "partial": kernels.refine_bits_partials(y),
           "g": torch.empty_like(y) if g_out else None}
    kernels.refine_step(y, steps, t["pack"], y_hat, out["y_deq"], out["status"], out["partial"],
                        g_deq=t["g_deq"][sel].contiguous(), m=m, v=v, lr=F.LR, t=step,
                        g_out=out["g"])
    out.update(y=y, m=m, v=v, y_hat=y_hat)
    out["bits"], _ = kernels.reduce_partials(out["partial"])
    return out


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("shape", F.STEP_SHAPES)
def test_refine_step(device, shape, step):
    B, h, w, C = shape
    t = step_inputs(shape, device)
    o = run_step(t, step)
    assert o["partial"].shape == (B, -(-h * w * C // 4096))
    # the gradient: the existing kernel's, bit for bit
    ones = torch.ones(B, device=device)
    g_ref, _ = kernels.step_noise_rate_backward(o["y_hat_in"], t["g_deq"], t["steps"], t["pack"], ones)
    assert torch.equal(o["g"], g_ref)
    # Adam: the float64 evaluation fed the kernel's own g
    d = S.deltas(F.STEP_INDICES, torch.float64)
    ref = F.latent_iteration(None, None, nchw(t["y"]).double(), nchw(t["m"]).double(),
                             nchw(t["v"]).double(), d, None, F.LR, step, g=nchw(o["g"]).double())
    errs = {k: R.global_err(nchw(o[k]), ref[k]) for k in ("m", "v", "y")}
    print(f"refine_step {shape} t={step}:", {k: f"{e:.2e}" for k, e in errs.items()}, f"(bar {F.REL:.0e})")
    assert all(e <= F.REL for e in errs.values()), errs
    # the next iterate: the existing quantiser and the existing estimate, bit for bit
    q_hat, q_deq = kernels.quantise_steps(o["y"], t["steps"])
    assert torch.equal(o["y_hat"], q_hat) and torch.equal(o["y_deq"], q_deq)
    assert not bool(torch.equal(o["y_hat"], o["y_hat_in"]))       # the step moved some level
    want = image_bits(o["y_hat"], t["pack"], F.STEP_INDICES)
    print("bits", o["bits"].tolist(), "rate_bits", want)
    assert o["bits"].tolist() == want
    assert o["status"].tolist() == [0] * B
    # reproducible, without g_out the same, and an image alone as in its batch
    again = run_step(t, step, g_out=False)
    for k in ("y", "m", "v", "y_hat", "y_deq", "partial", "status"):
        assert torch.equal(o[k], again[k]), k
    for b in range(B):
        alone = run_step(t, step, sel=slice(b, b + 1))
        for k in ("y", "m", "v", "y_hat", "y_deq", "partial", "status", "g"):
            assert torch.equal(o[k][b:b + 1], alone[k]), (k, b)


@pytest.mark.parametrize("shape", F.STEP_SHAPES)
def test_refine_step_iteration_zero(device, shape):
    """Without a gradient: ``quantise_steps`` and the estimate of y as it stands; y untouched."""
    t = step_inputs(shape, device)
    y = t["y"].clone()
    y_hat, y_deq = torch.empty_like(y), torch.empty_like(y)
    status = torch.full((shape[0],), 7, device=device, dtype=torch.int32)
    partial = kernels.refine_bits_partials(y)
    kernels.refine_step(y, t["steps"], t["pack"], y_hat, y_deq, status, partial)
    q_hat, q_deq = kernels.quantise_steps(t["y"], t["steps"])
    assert torch.equal(y, t["y"]) and torch.equal(y_hat, q_hat) and torch.equal(y_deq, q_deq)
    bits, _ = kernels.reduce_partials(partial)
    assert bits.tolist() == image_bits(q_hat, t["pack"], F.STEP_INDICES)
    assert status.tolist() == [0, 0]


def test_refine_step_status_bits(device):
    """A NaN in image 0 and a level beyond ±32767 in image 1 set their image's status bits and
    change no other element."""
    shape = F.STEP_SHAPES[0]
    t = step_inputs(shape, device)
    clean = run_step(t, 1)
    bad = t["y"].clone()
    bad[0, 2, 3, 5] = float("nan")
    bad[1, 4, 6, 191] = 1e9
    o = run_step(t, 1, y=bad)
    assert o["status"].tolist() == [1, 2]                         # ST_NAN, ST_RANGE
    mask = torch.ones_like(bad, dtype=torch.bool)
    mask[0, 2, 3, 5] = mask[1, 4, 6, 191] = False
    for k in ("y", "m", "v", "y_hat", "y_deq", "g"):
        assert torch.equal(o[k][mask], clean[k][mask]), k
    assert bool(torch.isnan(o["y_hat"][0, 2, 3, 5])) and float(o["y_hat"][1, 4, 6, 191]) > 32767
    # iteration 0 flags the same
    y_hat, y_deq = torch.empty_like(bad), torch.empty_like(bad)
    status = torch.zeros(2, device=device, dtype=torch.int32)
    kernels.refine_step(bad, t["steps"], t["pack"], y_hat, y_deq, status,
                        kernels.refine_bits_partials(bad))
    assert status.tolist() == [1, 2]


# ------------------------------------------------------------------ 3. refine_keep
def test_refine_keep(device):
    """B = 4: improved, equal (not copied), worse, NaN (not copied); then a quantiser status and
    a reconstruction status, which keep nothing."""
    B, per = 4, 3 * 4 * 128
    lam = [650.25, 650.25, 100.0, 650.25]
    bits = [1000.0, 2000.0, 3000.0, float("nan")]
    sse = [5000, 6000, 7000, 8000]
    J = [F.objective(b, s, l) for b, s, l in zip(bits, sse, lam)]
    best_J0 = [J[0] + 1e-9, J[1], J[2] - 1e-9, 1e30]

    def on(v, dt):
        return torch.tensor(v, dtype=dt, device=device)

    y_hat = torch.round(R.normal(5, (B, 3, 4, 128), 4.0)).to(device)
    old = torch.round(R.normal(6, (B, 3, 4, 128), 4.0)).to(device)

    def run(qstatus=(0, 0, 0, 0), rstatus=0):
        st = {"best_J": on(best_J0, torch.float64), "best_iter": on([0, 1, 2, 0], torch.int32),
              "best_bits": on([1.0, 2.0, 3.0, 4.0], torch.float64),
              "best_sse": on([10, 20, 30, 40], torch.int64), "best": old.clone(),
              "flag": on([9, 9, 9, 9], torch.int32)}
        kernels.refine_keep(on(bits, torch.float64), on(sse, torch.int64), on(lam, torch.float64),
                            on(list(qstatus), torch.int32), on([rstatus], torch.int32), y_hat, 5,
                            st["best_J"], st["best_iter"], st["best_bits"], st["best_sse"],
                            st["best"], st["flag"])
        return st

    st = run()
    kept, new_J = F.keep(bits, sse, lam, (0, 0, 0, 0), 0, best_J0)
    assert kept == [True, False, False, False] and new_J == [J[0], best_J0[1], best_J0[2], 1e30]
    assert st["flag"].tolist() == [int(k) for k in kept]
    assert st["best_J"].tolist() == new_J
    assert st["best_iter"].tolist() == [5, 1, 2, 0]
    assert st["best_bits"].tolist() == [1000.0, 2.0, 3.0, 4.0]
    assert st["best_sse"].tolist() == [5000, 20, 30, 40]
    assert torch.equal(st["best"][0], y_hat[0]) and torch.equal(st["best"][1:], old[1:])
    for kw in ({"qstatus": (2, 0, 0, 0)}, {"rstatus": 1}):
        st = run(**kw)
        assert st["flag"].tolist() == [0, 0, 0, 0] and torch.equal(st["best"], old)
        assert st["best_J"].tolist() == best_J0 and st["best_iter"].tolist() == [0, 1, 2, 0]


# ------------------------------------------------------------------ 4. the codec
@pytest.fixture(scope="module")
def net(device):
    n = ImageCompressor(out_channel_N=F.E2E_N)
    sd = synth.trained_like_state_dict(F.E2E_N, F.E2E_SEED)
    n.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return n.to(device).eval()


@pytest.fixture(params=["h3", "x6", "fp32"])
def precision(request):
    with kernels.precision_scope(request.param):
        yield request.param


def blob_objective(net, blob, image, lam, tile=None):
    """J of a blob from the blob alone: its decoded ŷ through the existing rate estimate, its
    decoded pixels against the original in numpy."""
    head, info = codec.parse_blob(blob)
    step = info.step if tile else info
    Hc, Wc = codec.canvas(head.H, head.W)
    dec = net.decompress([blob[codec.HEADER.size:]], (Hc // 16, Wc // 16), streams_per_image=head.P, K=head.K,
                         step=step, **({"tile": tile} if tile else {}))
    y_hat = dec["y_hat"].permute(0, 2, 3, 1).contiguous()
    bits = image_bits(y_hat, net.bitEstimator.packed(), [step])[0]
    pixels = net.decompress_images([blob])[0]
    sse = int(((pixels.astype(np.int64) - image.astype(np.int64)) ** 2).sum())
    return F.objective(bits, sse, lam), bits, sse


@pytest.mark.parametrize("tile", [None, 8])
def test_refined_blobs(device, net, precision, tile):
    ims = F.e2e_images()
    kw = {"step": F.E2E_STEP, "tile": tile}
    plain = net.compress_images(ims, **kw)
    assert net.compress_images(ims, refine=0, **kw) == plain
    assert net.compress_images(ims, refine=0, refine_lambda=F.E2E_LAMBDA, **kw) == plain
    # three iterations move a level only with a learning rate above the default
    kw.update(refine=F.E2E_ITERS, refine_lambda=F.E2E_LAMBDA, refine_lr=F.LR)
    stats = {}
    blobs = net.compress_images(ims, stats=stats, **kw)
    assert net.compress_images(ims, **kw) == blobs
    decoded = net.decompress_images(blobs)
    for i, (blob, im) in enumerate(zip(blobs, ims)):
        head, info = codec.parse_blob(blob)
        assert blob[:4] == (b"I17T" if tile else b"I17Q")
        assert (info.step, info.tile) == (F.E2E_STEP, tile) if tile else info == F.E2E_STEP
        assert (head.H, head.W) == im.shape[:2] == decoded[i].shape[:2]
        J, bits, sse = blob_objective(net, blob, im, F.E2E_LAMBDA, tile)
        Jp, bits_p, sse_p = blob_objective(net, plain[i], im, F.E2E_LAMBDA, tile)
        print(f"{precision} tile={tile} image {i}: kept {stats['refine_kept'][i]}, J {J!r} "
              f"(bits {bits!r}, sse {sse}) plain {Jp!r} (bits {bits_p!r}, sse {sse_p})")
        assert stats["objective"][i] == J
        assert stats["objective_plain"][i] == Jp
        assert J <= Jp
        assert stats["refine_iters"][i] == F.E2E_ITERS
        assert 0 <= stats["refine_kept"][i] <= F.E2E_ITERS
        assert (blob == plain[i]) == (stats["refine_kept"][i] == 0)
    rows = net.evaluate_images(ims, **kw)
    assert [r["objective"] for r in rows] == stats["objective"]
    assert [r["bytes"] for r in rows] == [len(b) for b in blobs]
    # the default learning rate: the same contract
    kw["refine_lr"] = None
    stats = {}
    for blob, im, J, Jp in zip(net.compress_images(ims, stats=stats, **kw), ims, stats["objective"],
                               stats["objective_plain"]):
        assert blob_objective(net, blob, im, F.E2E_LAMBDA, tile)[0] == J <= Jp


def test_lambda_zero_lowers_the_estimated_bits(device, net, precision):
    ims = F.e2e_images()
    plain = net.compress_images(ims, step=F.E2E_STEP)
    stats = {}
    blobs = net.compress_images(ims, step=F.E2E_STEP, refine=F.E2E_ITERS, refine_lambda=0,
                                refine_lr=F.LR, stats=stats)
    for i, im in enumerate(ims):
        _, bits, _ = blob_objective(net, blobs[i], im, 0.0)
        _, bits_p, _ = blob_objective(net, plain[i], im, 0.0)
        print(f"{precision} image {i}: bits {bits!r} plain {bits_p!r} kept {stats['refine_kept'][i]}")
        assert bits <= bits_p and stats["objective"][i] == bits


def test_diverging_run_is_the_plain_blob(device, net, precision):
    """refine_lr = 1e6: every iterate leaves the coder's range, none is kept, nothing faults, and
    the blobs are the plain ones byte for byte."""
    ims = F.e2e_images()
    stats = {}
    blobs = net.compress_images(ims, step=F.E2E_STEP, refine=F.E2E_ITERS,
                                refine_lambda=F.E2E_LAMBDA, refine_lr=1e6, stats=stats)
    assert blobs == net.compress_images(ims, step=F.E2E_STEP)
    assert stats["refine_kept"] == [0, 0, 0]
    assert stats["objective"] == stats["objective_plain"]


def test_loop_has_no_host_synchronisation(device, net, precision):
    """codec.refine_loop under torch's sync debug mode (it raises on any synchronising call), after
    one run that builds the packed layouts; the second run gives the first one's bits."""
    ims = F.e2e_images()[:2]
    ims = [ims[1], np.ascontiguousarray(ims[1][::-1])]        # two images of one canvas
    packed, offsets, shapes = codec.upload_packed(ims, device)
    x = kernels.image_ingest(packed, offsets, shapes, (64, 64))
    y = net.latents(x)
    desc = kernels._image_desc("refine", packed.numel(), offsets, shapes, (64, 64)).to(device)
    steps = torch.tensor([codec.step_size(8), codec.step_size(11)], device=device)
    lam = torch.tensor([F.E2E_LAMBDA, 100.0], dtype=torch.float64, device=device)
    wt = (lam / 3.0).float()
    net._warm_packs(backward=True, mode=precision)
    net._warm_packs(mode=precision)
    args = (net, y, steps, lam, wt, packed, desc, F.E2E_ITERS, codec.DEFAULT_REFINE_LR, precision)
    first = codec.refine_loop(*args)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = codec.refine_loop(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert second.best_iter.min().item() >= 0 and bool(torch.isfinite(second.best_J).all())
    q_hat, _ = kernels.quantise_steps(y, steps)
    assert torch.equal(second.plain, q_hat)                   # iteration 0 is the plain quantiser
