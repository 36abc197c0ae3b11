"""Quality targets on the GPU (csrc/quality.hip, image_sse in csrc/imageio.hip and the layers above
them): the three kernels against the existing ones and the definition, and the
codec's contract against a brute-force sweep of the ladder. The weights are synthetic: nothing
here is a statement about quality."""
import math

import numpy as np
import pytest
import torch

import rdo_refs as R
from iclr_17_compression_amd import codec, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor

pytestmark = pytest.mark.gpu

DELTAS = [codec.step_size(s) for s in range(codec.STEPS)]
MIXED = [(49, 83), (64, 96), (50, 96), (64, 81)]    # one canvas, 64×96 (test_gpu_ratectl.py)
SWEEP_REL = 1e-5                                    # the project's sweep bar


def make_net(N, device):
    n = ImageCompressor(out_channel_N=N)
    n.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
    return n.to(device).eval()


@pytest.fixture(scope="module")
def nets(device):
    made = {}

    def get(N):
        if N not in made:
            net = make_net(N, device)
            ims = R.images()
            with kernels.precision_scope("x6"):
                ys = [net.latents(R.batch(ims[:2]).to(device)), net.latents(R.batch(ims[2:]).to(device))]
            assert [tuple(y.shape) for y in ys] == [(2, 4, 6, N), (1, 1, 1, N)]
            made[N] = (net, ys)
        return made[N]
    return get


def steps_on(device, indices):
    return torch.tensor([DELTAS[s] for s in indices], dtype=torch.float32, device=device)


# ------------------------------------------------------------------ 1. quantise_steps
def status_of_step(y, d):
    """quantise_step's status bits of one image, read off what it raises."""
    try:
        kernels.quantise_step(y, d)
    except kernels.Iclr17Error as e:
        return (1 if "a latent is NaN" in str(e) else 0) | (2 if "> 32767" in str(e) else 0)
    return 0


@pytest.mark.parametrize("N", [128, 192])
def test_quantise_steps_equals_quantise_step(device, nets, N):
    _, ys = nets(N)
    for y, indices in ((ys[0], (3, 17)), (ys[0], (31, 0)), (ys[1], (11,))):
        sd = steps_on(device, indices)
        y_hat, y_deq = kernels.quantise_steps(y, sd)
        none, y_deq2 = kernels.quantise_steps(y, sd, want_hat=False)
        assert none is None and torch.equal(y_deq2, y_deq)
        assert y_hat.shape == y_deq.shape == y.shape and y_hat.dtype == torch.float32
        for b, s in enumerate(indices):
            one_hat, one_deq = kernels.quantise_step(y[b:b + 1].contiguous(), DELTAS[s])
            assert torch.equal(y_hat[b:b + 1], one_hat) and torch.equal(y_deq[b:b + 1], one_deq)
    # the status word: a NaN in one image, a range overflow in the other, each alone and together
    y = ys[0]
    for bad0, bad1 in ((float("nan"), None), (None, 8192.0), (float("nan"), float("-inf")),
                       (8192.0, None)):
        bad = y.clone()
        if bad0 is not None:
            bad[0, 3, 5, N - 1] = bad0
        if bad1 is not None:
            bad[1, 0, 0, 0] = bad1
        indices = (0, 0)     # Δ = 0.25: 8192 / 0.25 = 32768 > 32767
        want = status_of_step(bad[0:1].contiguous(), DELTAS[0]) | status_of_step(bad[1:2].contiguous(),
                                                                                DELTAS[0])
        y_hat, y_deq, status = kernels.quantise_steps_device(bad, steps_on(device, indices))
        assert int(status.item()) == want != 0
        ref = np.rint(bad.cpu().numpy() / np.float32(DELTAS[0]))
        assert np.array_equal(y_hat.cpu().numpy(), ref, equal_nan=True)
        assert np.array_equal(y_deq.cpu().numpy(), np.float32(DELTAS[0]) * ref, equal_nan=True)
        text = "a latent is NaN" if want & 1 else "> 32767"
        with pytest.raises(kernels.Iclr17Error, match=text):
            kernels.quantise_steps(bad, steps_on(device, indices))
    # a coarse step for the image that overflows at the fine one: no status
    bad = y.clone()
    bad[1, 0, 0, 0] = 8192.0
    kernels.quantise_steps(bad, steps_on(device, (0, 8)))
    for steps in (torch.tensor([1.0, 0.0]), torch.tensor([1.0, float("nan")]),
                  torch.tensor([1.0, float("inf")]), torch.tensor([1.0, -2.0])):
        with pytest.raises(kernels.Iclr17Error, match="not finite and positive"):
            kernels.quantise_steps(y, steps.to(device))
    with pytest.raises(kernels.Iclr17Error, match="step sizes for a batch"):
        kernels.quantise_steps(y, torch.ones(3, device=device))


# ------------------------------------------------------------------ 2. image_sse
def u8_image(seed, H, W):
    return np.ascontiguousarray(synth.image_u8(seed, 1, H, W)[0].transpose(1, 2, 0))


def packed(images):
    sizes = [im.size for im in images]
    offsets = [int(o) for o in np.cumsum([0] + sizes[:-1])]
    return torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])), offsets, \
        [im.shape[:2] for im in images]


def recon_batch(shapes, canvas, seed):
    """fp32 [B,3,Hc,Wc] in [−0.2, 1.2] with rounding ties (k + ½)/255 and exact 0, 1, −0.0 in each
    image's own region (test_gpu_image_io.py's recipe)."""
    Hc, Wc = canvas
    r = synth.uniform(seed, (len(shapes), 3, Hc, Wc), -0.2, 1.2)
    ties = np.concatenate([(np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255.0),
                           np.array([0.0, 1.0, -0.0], dtype=np.float32)])
    for b, (H, W) in enumerate(shapes):
        region = r[b, 1, :H, :W].reshape(-1)
        n = min(region.size, ties.size)
        region[:n] = ties[:n]
        r[b, 1, :H, :W] = region.reshape(H, W)
    return torch.from_numpy(r)


SSE_CASES = [(MIXED, (64, 96)), ([(20, 261)], (32, 272)), ([(19, 261), (32, 258), (17, 272)], (32, 272)),
             ([(1, 1)], (16, 16))]


@pytest.mark.parametrize("shapes,canvas", SSE_CASES, ids=["mixed", "20x261", "wide3", "1x1"])
def test_image_sse_equals_the_egress_sums(device, shapes, canvas):
    recon = recon_batch(shapes, canvas, 33).to(device)
    ref, offsets, shp = packed([u8_image(80 + k, H, W) for k, (H, W) in enumerate(shapes)])
    assert len(shapes) < 3 or any(o % 4 for o in offsets)     # natural, unaligned byte offsets
    ref = ref.to(device)
    _, _, want_sse, want_status = kernels.image_egress_device(recon, offsets, shp, ref)
    buf, sse, status, spare = kernels.image_sse_device(recon, offsets, shp, ref)
    assert buf.numel() == 8 * len(shapes) + 8 and sse.dtype == torch.int64
    assert torch.equal(sse, want_sse) and int(status.item()) == int(want_status.item()) == 0
    assert int(spare.item()) == 0 and int(sse.min()) > 0
    assert torch.equal(kernels.image_sse(recon, offsets, shp, ref), want_sse.cpu())
    assert torch.equal(kernels.image_sse(recon, offsets, shp, ref), want_sse.cpu())   # again
    # the CPU contract of the egress, for the sums themselves
    for b, (H, W) in enumerate(shapes):
        got8 = torch.round(recon[b, :, :H, :W].cpu().clamp(0, 1) * 255).permute(1, 2, 0).long()
        o = offsets[b]
        r8 = ref.cpu()[o:o + 3 * H * W].reshape(H, W, 3).long()
        assert int(((got8 - r8) ** 2).sum()) == int(sse[b])
    # non-finite values: in the padding they are never looked at, inside an image they set the
    # status exactly as the egress's
    H, W = shapes[-1]
    pad = recon.clone()
    if H < canvas[0]:
        pad[-1, :, H:, :] = float("nan")
    if W < canvas[1]:
        pad[-1, :, :, W:] = float("inf")
    _, sse_p, status_p, _ = kernels.image_sse_device(pad, offsets, shp, ref)
    assert torch.equal(sse_p, want_sse) and int(status_p.item()) == 0
    for bad in (float("nan"), float("-inf")):
        inside = recon.clone()
        inside[-1, 2, H - 1, W - 1] = bad          # the last pixel of the last image's own region
        _, _, e_sse, e_status = kernels.image_egress_device(inside, offsets, shp, ref)
        _, s_sse, s_status, _ = kernels.image_sse_device(inside, offsets, shp, ref)
        assert int(s_status.item()) == int(e_status.item()) == 1 and torch.equal(s_sse, e_sse)
        for precision, text in (("h3", "does not fit the h3 form"), ("x6", "non-finite reconstruction")):
            with kernels.precision_scope(precision):
                with pytest.raises(kernels.Iclr17Error, match=text):
                    kernels.image_sse(inside, offsets, shp, ref)


# ------------------------------------------------------------------ 3. distortion_sweep
def sweep_reference(y, w, q_of):
    """The definition in float64 on the GPU's own fp32 q: Σ w_c·(Δ·q − v)² per image and step."""
    v = y.cpu().numpy().astype(np.float64)
    out = np.empty((y.shape[0], len(q_of)))
    for s, (d, q) in enumerate(q_of):
        e = np.float64(np.float32(d)) * q.astype(np.float64) - v
        out[:, s] = (w.astype(np.float64) * e * e).sum(axis=(1, 2, 3))
    return out


@pytest.mark.parametrize("N", [128, 192])
def test_distortion_sweep(device, nets, N):
    net, ys = nets(N)
    ramp = R.weights(N, "ramp")
    worst = 0.0
    for y in ys:
        q_of = [(d, kernels.quantise_step(y, d)[0].cpu().numpy()) for d in DELTAS]
        for w in (ramp, np.ones(N, dtype=np.float32)):
            got = kernels.distortion_sweep(y, torch.from_numpy(w).to(device), DELTAS)
            assert got.dtype == torch.float64 and tuple(got.shape) == (y.shape[0], 32)
            want = sweep_reference(y, w, q_of)
            rel = np.abs(got.cpu().numpy() - want) / want
            worst = max(worst, float(rel.max()))
            assert torch.equal(kernels.distortion_sweep(y, torch.from_numpy(w).to(device), DELTAS), got)
            for b in range(y.shape[0]):                      # an image alone: its row of the batch
                alone = kernels.distortion_sweep(y[b:b + 1].contiguous(), torch.from_numpy(w).to(device),
                                                 DELTAS)
                assert torch.equal(alone[0], got[b])
            for s in (0, 8, 31):                             # S = 1: the column of S = 32
                one = kernels.distortion_sweep(y, torch.from_numpy(w).to(device), [DELTAS[s]])
                assert tuple(one.shape) == (y.shape[0], 1) and torch.equal(one[:, 0], got[:, s])
        # unit weights: the direct sum from quantise_step's outputs. y_deq is Δ·q rounded to fp32
        # where the sweep's fma is not: per element |δ| ≤ 2^-24·|y_deq|, so by Cauchy–Schwarz the
        # sums differ by at most 2·√(Σe²·Σδ²) + Σδ², relative to Σe², beyond the sweep's own bar
        unit = kernels.distortion_sweep(y, torch.ones(N, device=device), DELTAS).cpu().numpy()
        v = y.cpu().numpy().astype(np.float64)
        for s, d in enumerate(DELTAS):
            deq = kernels.quantise_step(y, d)[1].cpu().numpy().astype(np.float64)
            direct = ((deq - v) ** 2).sum(axis=(1, 2, 3))
            delta2 = ((2.0 ** -24 * np.abs(deq)) ** 2).sum(axis=(1, 2, 3))
            bound = SWEEP_REL + (2.0 * np.sqrt(direct * delta2) + delta2) / direct
            assert (np.abs(unit[:, s] - direct) / direct <= bound).all(), (s, unit[:, s], direct)
        zero = kernels.distortion_sweep(y, torch.zeros(N, device=device), DELTAS)
        assert torch.equal(zero, torch.zeros_like(zero))
    print(f"distortion_sweep N={N}: worst relative error against float64 {worst:.3e} (bar {SWEEP_REL:g})")
    assert worst <= SWEEP_REL
    # the model's entry: the default weights are the unnormalised gains, and synthesis_gains is
    # still their division by the mean
    g = net.synthesis_gains_raw()
    assert torch.equal(net.synthesis_gains(), (g / g.mean()).contiguous())
    assert torch.equal(net.distortion_sweep(ys[0]), kernels.distortion_sweep(ys[0], g, DELTAS))
    assert torch.equal(net.distortion_sweep(ys[0], steps=[4, 9], weights=ramp),
                       kernels.distortion_sweep(ys[0], torch.from_numpy(ramp).to(device),
                                                [DELTAS[4], DELTAS[9]]))
    for bad in (torch.full((N,), float("nan")), -torch.ones(N), torch.ones(N + 1)):
        with pytest.raises(kernels.Iclr17Error, match="weights must"):
            kernels.distortion_sweep(ys[0], bad.to(device), DELTAS)
    with pytest.raises(kernels.Iclr17Error, match="0 steps|33 steps"):
        kernels.distortion_sweep(ys[0], g, DELTAS + [1.0])


# ------------------------------------------------------------------ 4. the codec's contract
@pytest.fixture(scope="module")
def mixed_images():
    return [R.smooth(90 + k, H, W) for k, (H, W) in enumerate(MIXED)]


@pytest.fixture(scope="module")
def ladders(device, nets, mixed_images):
    """Brute force, once per (N, precision): sse_u8 of every image at every ladder index from the
    real codec path, evaluate_images(step=i)."""
    made = {}

    def get(N, precision):
        if (N, precision) not in made:
            net, _ = nets(N)
            with kernels.precision_scope(precision):
                rows = [net.evaluate_images(mixed_images, step=i) for i in range(codec.STEPS)]
            made[N, precision] = np.array([[r["sse_u8"] for r in row] for row in rows]).T   # [image, index]
        return made[N, precision]
    return get


def psnr_of(sse, H, W):
    return 10.0 * math.log10(255.0 ** 2 * 3 * H * W / sse)


def targets_between(table, shapes, which):
    """Per image a target halfway (in dB) between the measured PSNRs of two neighbouring indices
    j, j + 1 of which j passes and j + 1 fails: the ``which``-th such pair of three spread over
    the ladder. Nothing is fixed in advance. The SSE of these synthetic weights is not monotone
    along the ladder, and a search that measures index 0 failing raises by its contract, so only
    pairs with SSE(0) ≤ SSE(j) are taken: index 0 then passes whatever else does."""
    out = []
    for row, (H, W) in zip(table, shapes):
        pairs = [j for j in range(codec.STEPS - 1) if 0 < row[0] <= row[j] < row[j + 1]]
        assert pairs, "the SSE never rises above its value at index 0 along the ladder"
        j = pairs[min(len(pairs) - 1, which * len(pairs) // 3)]
        out.append(0.5 * (psnr_of(row[j], H, W) + psnr_of(row[j + 1], H, W)))
    return out


def check_contract(net, images, table, targets, blobs, stats):
    for k, (im, T, blob) in enumerate(zip(images, targets, blobs)):
        H, W = im.shape[:2]
        limit = codec.sse_limit(H, W, T)
        head, s = codec.parse_blob(blob)
        if isinstance(s, codec.TileInfo):
            s = s.step
        passes = table[k] <= limit
        assert passes[s] and (s == codec.STEPS - 1 or not passes[s + 1]), (k, s, T)
        if not passes[int(passes.sum()):].any():          # the pass row is a prefix
            assert s == int(passes.sum()) - 1
        assert stats["sse"][k] == int(table[k][s])
        assert 1 <= stats["probes"][k] <= codec.MAX_PROBES
    assert stats["reencodes"] == [0] * len(images)


@pytest.mark.parametrize("precision", ["x6", "h3", "fp32"])
@pytest.mark.parametrize("N", [128, 192])
def test_codec_contract(device, nets, mixed_images, ladders, N, precision):
    net, _ = nets(N)
    table = ladders(N, precision)
    shapes = [im.shape[:2] for im in mixed_images]
    print(f"N={N} {precision}: PSNR along the ladder, image 0: "
          + " ".join(f"{psnr_of(e, *shapes[0]):.2f}" for e in table[0]))
    with kernels.precision_scope(precision):
        for which in range(3):
            targets = targets_between(table, shapes, which)
            for estimate in (True, False):
                stats = {}
                blobs = net.compress_images(mixed_images, psnr=targets, stats=stats, estimate=estimate)
                check_contract(net, mixed_images, table, targets, blobs, stats)
                print(f"  targets {[round(t, 2) for t in targets]} estimate={estimate}: indices "
                      f"{[codec.parse_blob(b)[1] for b in blobs]} probes {stats['probes']}")
                if not estimate:
                    assert max(stats["probes"]) <= 6
                one = {}      # an image's probes depend on that image alone, guided or not
                assert net.compress_images(mixed_images, psnr=targets, stats=one, estimate=estimate,
                                           max_batch=1) == blobs and one == stats
        targets = targets_between(table, shapes, 1)
        stats = {}
        blobs = net.compress_images(mixed_images, psnr=targets, stats=stats)
        found = [codec.parse_blob(b)[1] for b in blobs]
        # the blob of step=s, byte for byte; the real decode's SSE; independence of the batch
        rows = net.evaluate_images(mixed_images, psnr=targets)
        for k, (im, s, T) in enumerate(zip(mixed_images, found, targets)):
            assert [blobs[k]] == net.compress_images([im], step=s)
            assert rows[k]["step"] == s and rows[k]["sse_u8"] == stats["sse"][k]
            assert rows[k]["sse_u8"] <= codec.sse_limit(*im.shape[:2], T)
            alone_stats = {}
            assert net.compress_images([im], psnr=T, stats=alone_stats) == [blobs[k]]
            assert alone_stats["probes"] == [stats["probes"][k]]
            assert alone_stats["sse"] == [stats["sse"][k]]
        one_stats = {}
        assert net.compress_images(mixed_images, psnr=targets, max_batch=1, stats=one_stats) == blobs
        assert one_stats == stats
        # tile: the layout alone
        tiled = net.compress_images(mixed_images, psnr=targets, tile=8)
        for k, (im, s) in enumerate(zip(mixed_images, found)):
            assert [tiled[k]] == net.compress_images([im], step=s, tile=8)
        # a scalar target, and 1 dB: the coarsest index
        stats1 = {}
        low = net.compress_images(mixed_images, psnr=1, stats=stats1)
        assert [codec.parse_blob(b)[1] for b in low] == [codec.STEPS - 1] * 4
        assert max(stats1["probes"]) <= codec.MAX_PROBES
        # unreachable: above what index 0 gives, and (the SSE need not be monotone) above what
        # any index gives
        k = int(np.argmax(table.min(axis=1)))
        if table[k].min() > 0:
            top = psnr_of(table[k].min(), *shapes[k])
            with pytest.raises(kernels.Iclr17Error,
                               match=rf"image 0 \({shapes[k][0]}x{shapes[k][1]}\) cannot reach"):
                net.compress_images([mixed_images[k]], psnr=top + 0.5)
            with pytest.raises(kernels.Iclr17Error, match=rf"image {k} .*cannot reach"):
                net.compress_images(mixed_images, psnr=[1.0] * k + [top + 0.5] + [1.0] * (3 - k))
        # decoding: mixed with plain and stepped blobs
        plain = net.compress_images(mixed_images[:2])
        stepped = net.compress_images(mixed_images[2:], step=5)
        mix = [blobs[0], plain[0], tiled[1], stepped[0], blobs[3], plain[1]]
        out = net.decompress_images(mix)
        want = [net.decompress_images([b])[0] for b in mix]
        assert all(np.array_equal(a, b) for a, b in zip(out, want))
        assert np.array_equal(out[0], rows[0]["recon"]) and np.array_equal(out[4], rows[3]["recon"])


def test_codec_raises(device, nets, mixed_images):
    net, _ = nets(128)
    for kw, text in (({"rdo": 1.0}, "psnr with rdo.*is not built"),
                     ({"step_offsets": [None] * 4}, "psnr with step_offsets.*is not built"),
                     ({"step": 8}, "step and psnr given together"),
                     ({"bpp": 1.0}, "bpp and psnr given together")):
        with pytest.raises(kernels.Iclr17Error, match=text):
            net.compress_images(mixed_images, psnr=30.0, **kw)
        with pytest.raises(kernels.Iclr17Error, match=text):
            net.evaluate_images(mixed_images, psnr=30.0, **kw)
    with pytest.raises(kernels.Iclr17Error, match="psnr must be"):
        net.compress_images(mixed_images, psnr=float("nan"))
    stats = {}
    net.compress_images(mixed_images, step=8, stats=stats)      # without psnr: stats as before
    assert sorted(stats) == ["reencodes"]


def test_command_line(device, nets, mixed_images, ladders, tmp_path, capsys):
    import json

    from PIL import Image
    net, _ = nets(128)
    img = mixed_images[1]
    T = targets_between(ladders(128, kernels.precision()), [im.shape[:2] for im in mixed_images], 1)[1]
    src, out, back = tmp_path / "in.png", tmp_path / "out.i17c", tmp_path / "back.png"
    ckpt = tmp_path / "iter_0.pth.tar"
    Image.fromarray(img).save(src)
    torch.save(net.state_dict(), ckpt)
    common = ["--weights", str(ckpt), "--N", "128"]
    for flags, kw in ((["--psnr", repr(T)], {"psnr": T}), (["--psnr", repr(T), "--tile", "8"],
                                                           {"psnr": T, "tile": 8})):
        assert codec.main(["encode", str(src), str(out), *common, *flags]) == 0
        blob = net.compress_images([img], **kw)[0]
        assert out.read_bytes() == blob and blob[:4] == (b"I17T" if "tile" in kw else b"I17Q")
        assert codec.main(["decode", str(out), str(back), *common]) == 0
        with Image.open(back) as im:
            assert np.array_equal(np.asarray(im), net.decompress_images([blob])[0])
    capsys.readouterr()
    assert codec.main(["eval", str(src), *common, "--psnr", repr(T)]) == 0
    rows = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    want = net.evaluate_images([img], psnr=T)[0]
    assert [r["name"] for r in rows] == [str(src), "mean"] and rows[0]["psnr"] == T
    assert rows[0]["index"] == want["step"] and rows[0]["bytes"] == want["bytes"]
    assert rows[0]["psnr_u8"] == want["psnr_u8"] >= T
