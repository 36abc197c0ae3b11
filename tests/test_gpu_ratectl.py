"""Rate control on the GPU (csrc/ratectl.hip and the layers above it): the fused rate sweep against
the existing rate kernels and against float64, the step quantiser bit for bit, the unit step
against the plain codec path, round trips along the ladder, byte budgets and the bf16 mode.
The weights are synthetic: nothing here is a statement about quality away from the unit step."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iclr_17_compression_amd import codec, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor

pytestmark = pytest.mark.gpu

METRIC_REL = 1e-5                                   # the project's bar for a bit total
MIXED = [(49, 83), (64, 96), (50, 96), (64, 81)]    # one canvas, 64×96 (test_gpu_image_io.py)
ALL_STEPS = list(range(codec.STEPS))
DELTAS = [codec.step_size(s) for s in ALL_STEPS]


def smooth(seed, H, W):
    return np.ascontiguousarray(synth.smooth_image_u8(seed, H, W).transpose(1, 2, 0))


def padded(im, Hc, Wc):
    """The ingest contract: ToTensor's /255, the image top left, edges replicated (CPU)."""
    H, W = im.shape[:2]
    x = torch.from_numpy(im).permute(2, 0, 1).float().div(255)[None]
    return F.pad(x, (0, Wc - W, 0, Hc - H), mode="replicate")


def to_u8(x_hat):
    """The egress contract on a CPU tensor [..., 3, H, W]: half-to-even of clamp·255."""
    return torch.round(x_hat.clamp(0, 1) * 255).to(torch.uint8)


def make_net(N, device):
    n = ImageCompressor(out_channel_N=N)
    n.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
    return n.to(device).eval()


@pytest.fixture(scope="module")
def nets(device):
    made = {}

    def get(N):
        if N not in made:
            made[N] = make_net(N, device)
        return made[N]
    return get


@pytest.fixture(scope="module")
def images():
    """The mixed 64×96-canvas group, then a 1×1 image."""
    return [smooth(60 + k, H, W) for k, (H, W) in enumerate(MIXED)] + [smooth(70, 1, 1)]


def batch(imgs, device):
    """Images of one canvas as the codec ingests them: fp32 [B,3,Hc,Wc] on the device."""
    Hc, Wc = codec.canvas(*imgs[0].shape[:2])
    return torch.cat([padded(im, Hc, Wc) for im in imgs]).to(device)


def latent_cases(net, images, device):
    """y of shape [2,4,6,N] (two images of the 64×96 canvas) and [1,1,1,N] (the 1×1 image)."""
    with kernels.precision_scope("x6"):
        return [net.latents(batch(images[:2], device)), net.latents(batch(images[4:], device))]


def separate_bits(y, net, s):
    """The existing kernels' figure for step s: float64 [B] and the pieces it was made from."""
    N = y.shape[3]
    y_hat, _ = kernels.quantise_step(y, DELTAS[s])
    pack = kernels.pack_rate_step(net.bitEstimator.packed(), N, DELTAS[s])
    per, _ = kernels.reduce_partials(kernels.rate_bits(y_hat.permute(0, 3, 1, 2), pack))
    return per, y_hat, pack


# ------------------------------------------------------------------ 1. sweep = existing kernels
@pytest.mark.parametrize("N", [128, 192])
def test_sweep_equals_the_existing_kernels(device, nets, images, N):
    net = nets(N)
    cases = latent_cases(net, images, device)
    assert [tuple(y.shape) for y in cases] == [(2, 4, 6, N), (1, 1, 1, N)]
    for y in cases:
        sweep = kernels.rate_sweep(y, net.bitEstimator.packed(), DELTAS)
        assert sweep.dtype == torch.float64 and tuple(sweep.shape) == (y.shape[0], 32)
        want = torch.stack([separate_bits(y, net, s)[0] for s in ALL_STEPS], dim=1)
        rel = ((sweep - want).abs() / want.abs()).max().item()
        print(f"sweep vs rate_bits N={N} {tuple(y.shape)}: max rel {rel:.3e}")
        assert rel <= 1e-12
        assert torch.equal(kernels.rate_sweep(y, net.bitEstimator.packed(), DELTAS), sweep)
        for s in (0, 8, 31):   # S = 1: a column of the full sweep
            one = kernels.rate_sweep(y, net.bitEstimator.packed(), [DELTAS[s]])
            assert tuple(one.shape) == (y.shape[0], 1)
            assert ((one[:, 0] - want[:, s]).abs() <= 1e-12 * want[:, s].abs()).all()
        # the model-level entry: ladder indices, the latent or the image
        assert torch.equal(net.rate_sweep(y), sweep)
        assert torch.equal(net.rate_sweep(y, steps=[4, 9]), sweep[:, [4, 9]])
    with kernels.precision_scope("x6"):
        assert torch.equal(net.rate_sweep(batch(images[:2], device)),
                           kernels.rate_sweep(cases[0], net.bitEstimator.packed(), DELTAS))
    for bad in ([], DELTAS + [1.0]):
        with pytest.raises(kernels.Iclr17Error, match="steps"):
            kernels.rate_sweep(cases[0], net.bitEstimator.packed(), bad)
    with pytest.raises(kernels.Iclr17Error, match="not finite and positive"):
        kernels.rate_sweep(cases[0], net.bitEstimator.packed(), [1.0, 0.0])


# ------------------------------------------------------------------ 2. sweep vs float64
def bits_f64(y_hat, pack):
    """Σ element_bits per image in numpy float64: y_hat [B,h,w,N] (the GPU's ŷ), pack [11,N]."""
    z = y_hat.astype(np.float64)
    p = pack.astype(np.float64)

    def cdf(v):
        for k in range(3):
            t = v * p[3 * k] + p[3 * k + 1]
            v = t + np.tanh(t) * p[3 * k + 2]
        return 1.0 / (1.0 + np.exp(-(v * p[9] + p[10])))

    prob = cdf(z + 0.5) - cdf(z - 0.5)
    bits = np.clip(-np.log(prob + 1e-10) / math.log(2.0), 0.0, 50.0)
    return bits.reshape(bits.shape[0], -1).sum(axis=1)


def test_sweep_against_float64(device, nets, images):
    net = nets(128)
    for y in latent_cases(net, images, device):
        sweep = kernels.rate_sweep(y, net.bitEstimator.packed(), DELTAS).cpu().numpy()
        want = np.empty_like(sweep)
        for s in ALL_STEPS:
            _, y_hat, pack = separate_bits(y, net, s)
            want[:, s] = bits_f64(y_hat.cpu().numpy(), pack.cpu().numpy().reshape(11, -1))
        rel = np.abs(sweep - want) / np.abs(want)
        print(f"sweep vs float64 {tuple(y.shape)}: max rel {rel.max():.3e} at step "
              f"{int(rel.max(axis=0).argmax())}; per step {np.array2string(rel.max(axis=0), precision=1)}")
        assert rel.max() <= METRIC_REL


# ------------------------------------------------------------------ 3. the quantiser is exact
def near_tie(v):
    """Where a value lies within 1e-3 of a rounding tie (n + ½)·Δ_s of any of the 32 steps."""
    v = np.asarray(v).astype(np.float64)
    bad = np.zeros(v.shape, bool)
    for d in DELTAS:
        u = v / d
        bad |= np.abs(u - (np.floor(u) + 0.5)) * d < 1e-3
    return bad


def tie_free(shape, seed, lo, hi):
    """fp32 values in [lo, hi) none of which is ``near_tie``: violators are drawn again until
    none is left."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(lo, hi, size=shape).astype(np.float32)
    bad = near_tie(y)
    while bad.any():
        y[bad] = rng.uniform(lo, hi, size=int(bad.sum())).astype(np.float32)
        bad = near_tie(y)
    return y


def test_quantise_is_exact(device):
    y = tie_free((3, 5, 7, 128), 5, -60.0, 60.0)   # 13440 elements: 53 workgroups, the last partial
    y.reshape(-1)[:6] = [0.0, -0.0, 8191.6, -8191.6, 1e-30, -1e-30]   # |ŷ| = 32766 at Δ = 0.25
    assert not near_tie(y).any()
    yd = torch.from_numpy(y).to(device)
    for s, d in enumerate(DELTAS):
        d32 = np.float32(d)
        y_hat, y_deq = kernels.quantise_step(yd, d)
        want = np.rint(y / d32)
        assert want.dtype == np.float32
        assert np.array_equal(y_hat.cpu().numpy().view(np.uint32), want.view(np.uint32)), s
        assert np.array_equal(y_deq.cpu().numpy().view(np.uint32), (d32 * want).view(np.uint32)), s
        assert torch.equal(kernels.dequantise_step(y_hat, d), y_deq)
    one = torch.from_numpy(tie_free((1, 1, 1, 128), 6, -9.0, 9.0)).to(device)
    assert np.array_equal(kernels.quantise_step(one, DELTAS[3])[0].cpu().numpy(),
                          np.rint(one.cpu().numpy() / np.float32(DELTAS[3])))
    for value, text in ((float("nan"), "a latent is NaN"), (8192.0, "> 32767"),
                        (float("-inf"), "> 32767")):
        bad = yd.clone()
        bad[2, 4, 6, 127] = value   # the last element
        with pytest.raises(kernels.Iclr17Error, match=text):
            kernels.quantise_step(bad, 0.25)
    assert float(kernels.quantise_step(yd.clone().fill_(8191.75), 0.25)[0].max()) == 32767.0
    with pytest.raises(kernels.Iclr17Error, match="not finite and positive"):
        kernels.quantise_step(yd, 0.0)


# ------------------------------------------------------------------ 3b. one body, three sources
def test_step_sources_agree(device, nets):
    """The quantiser has one body and three step sources (a scalar, a step per image, the ladder
    at a block's index) and the rate sweep two (its steps, the ladder at a clamped offset): on one
    input they give the same bits, and the same errors."""
    big = tie_free((3, 5, 7, 128), 5, -60.0, 60.0)   # 13440 elements: the last workgroup is
    one = tie_free((1, 1, 1, 128), 6, -9.0, 9.0)     # partial, the maps of 4 and 16 are ragged
    for y_np, index in ((big, (0, 8, 31)), (one, (8,))):
        y = torch.from_numpy(y_np).to(device)
        B, h, w, _ = y.shape
        deltas = torch.tensor([DELTAS[s] for s in index], device=device, dtype=torch.float32)
        hat_b, deq_b = kernels.quantise_steps(y, deltas)
        maps = {g: np.stack([np.full(kernels.map_shape(h, w, g), s, np.uint8) for s in index])
                for g in (1, 4, 16)}
        mapped = {g: kernels.quantise_step_map(y, maps[g], g, DELTAS) for g in maps}
        for b, s in enumerate(index):
            hat, deq = kernels.quantise_step(y[b], DELTAS[s])
            for got_hat, got_deq in [(hat_b, deq_b)] + list(mapped.values()):
                assert torch.equal(got_hat[b].view(torch.int32), hat.view(torch.int32)), (b, s)
                assert torch.equal(got_deq[b].view(torch.int32), deq.view(torch.int32)), (b, s)
            assert torch.equal(kernels.dequantise_step(hat, DELTAS[s]).view(torch.int32),
                               deq.view(torch.int32))
        for g in maps:
            assert torch.equal(kernels.dequantise_step_map(hat_b, maps[g], g, DELTAS)
                               .view(torch.int32), deq_b.view(torch.int32)), g

    # the same refusal through every source: Δ = 0.25 as a scalar, per image and as ladder entry 5
    y = torch.from_numpy(big).to(device)
    ladder = list(DELTAS)
    ladder[5] = 0.25
    quarter = torch.full((3,), 0.25, device=device)
    fives = np.full((3,) + kernels.map_shape(5, 7, 4), 5, np.uint8)
    for value in (float("nan"), 8192.0):
        bad = y.clone()
        bad[2, 4, 6, 127] = value   # the last element
        said = []
        for name, run in (("quantise_step", lambda: kernels.quantise_step(bad, 0.25)),
                          ("quantise_steps", lambda: kernels.quantise_steps(bad, quarter)),
                          ("quantise_step_map",
                           lambda: kernels.quantise_step_map(bad, fives, 4, ladder))):
            with pytest.raises(kernels.Iclr17Error) as err:
                run()
            head = f"iclr17: {name}: "
            assert str(err.value).startswith(head), str(err.value)
            said.append(str(err.value)[len(head):])
        assert said[0] and said.count(said[0]) == 3, said
        assert ("NaN" if value != value else "> 32767") in said[0]

    # one offset c for a whole image: row s of the offset sweep is row clamp(s + c) of rate_sweep
    pack = nets(128).bitEstimator.packed()
    rows = kernels.rate_sweep(y, pack, DELTAS)
    for c in (-3, 5):
        for g in (1, 4):
            off = np.full((3,) + kernels.map_shape(5, 7, g), c, np.int8)
            got = kernels.rate_sweep_offsets(y, pack, DELTAS, off, g)
            want = rows[:, [min(max(s + c, 0), 31) for s in ALL_STEPS]]
            assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (c, g)


def test_step_pack_and_its_cache(device, nets):
    net = make_net(128, device)   # its own: a parameter changes below
    be = net.bitEstimator
    base = be.packed().cpu().numpy().reshape(11, 128)
    got = be.step_packed(5)
    assert be.step_packed(5) is got
    want = base.copy()
    want[0] = base[0] * np.float32(DELTAS[5])
    assert np.array_equal(got.cpu().numpy().reshape(11, 128).view(np.uint32), want.view(np.uint32))
    assert torch.equal(be.step_packed(codec.UNIT_STEP), be.packed())
    tables = be.entropy_tables(32, step=5)
    assert be.entropy_tables(32, step=5) is tables
    assert torch.equal(tables, kernels.entropy_tables(got, 128, 32))
    assert torch.equal(be.entropy_tables(32, step=codec.UNIT_STEP), be.entropy_tables(32))
    with torch.no_grad():
        be.f1.h[0, 3, 0, 0] += 0.5
    fresh = be.step_packed(5)
    assert fresh is not got and not torch.equal(fresh, got)
    assert torch.equal(fresh, kernels.pack_rate_step(be.packed(), 128, DELTAS[5]))
    assert not torch.equal(be.entropy_tables(32, step=5), tables)


# ------------------------------------------------------------------ 4. the unit step
@pytest.mark.parametrize("N,precision", [(128, "x6"), (128, "h3"), (192, "h3")])
def test_unit_step_ties_the_new_path_to_the_old(device, nets, images, N, precision):
    net = nets(N)
    with kernels.precision_scope(precision):
        plain = net.compress_images(images)
        unit = net.compress_images(images, step=codec.UNIT_STEP)
        for p, u in zip(plain, unit):
            assert p[:4] == b"I17C" and u[:4] == b"I17Q"
            head, step = codec.parse_blob(u, N=N, fingerprint=codec.fingerprint(net))
            assert step == codec.UNIT_STEP and head == codec.parse_header(p)
            assert u[codec.HEADER.size:] == p[codec.HEADER.size:]
        for a, b in zip(net.decompress_images(unit), net.decompress_images(plain)):
            assert np.array_equal(a, b)
        assert net.compress_images(images) == plain   # the plain path writes what it wrote


# ------------------------------------------------------------------ 5. round trips
@pytest.mark.parametrize("precision", ["x6", "h3"])
@pytest.mark.parametrize("P", [1, 4])
def test_round_trip_along_the_ladder(device, nets, images, precision, P):
    net = nets(128)
    group = images[:2]
    with kernels.precision_scope(precision):
        x = batch(group, device)
        y = net.latents(x)
        for s in (0, 5, 13, 31):
            blobs = net.compress_images(group, step=s, streams_per_image=P)
            y_hat, y_deq = kernels.quantise_step(y, DELTAS[s])
            for b in blobs:
                head, step = codec.parse_blob(b)
                assert step == s and head.P == P
            dec = net.decompress([b[codec.HEADER.size:] for b in blobs], (4, 6),
                                 streams_per_image=P, step=s)
            assert torch.equal(dec["y_hat"], y_hat.permute(0, 3, 1, 2))
            with torch.no_grad():   # the eval forward; with autograd on the training kernels run
                want = to_u8(net.Decoder(y_deq.permute(0, 3, 1, 2).contiguous()).clamp(0, 1).cpu())
            for k, (im, got) in enumerate(zip(group, net.decompress_images(blobs))):
                H, W = im.shape[:2]
                assert got.dtype == np.uint8 and got.shape == (H, W, 3)
                assert np.array_equal(got, want[k, :, :H, :W].permute(1, 2, 0).numpy()), (s, k)


@pytest.mark.parametrize("precision", ["x6", "h3"])
def test_mixed_blobs_and_batch_independence(device, nets, images, precision):
    net = nets(128)
    with kernels.precision_scope(precision):
        per_step = {s: net.compress_images(images, step=s) for s in (5, 13, 31)}
        plain = net.compress_images(images)
        mixed = [plain[0], per_step[5][1], per_step[31][2], per_step[13][3], per_step[5][4],
                 plain[1], per_step[13][0]]
        alone = [net.decompress_images([b])[0] for b in mixed]
        for a, b in zip(net.decompress_images(mixed), alone):
            assert np.array_equal(a, b)
        for a, b in zip(net.decompress_images(mixed, max_batch=2), alone):
            assert np.array_equal(a, b)
        # a blob's bytes do not depend on its batch
        assert net.compress_images(images, step=5, max_batch=1) == per_step[5]
        assert net.compress_images(images[1:2], step=13) == per_step[13][1:2]
        rows = net.evaluate_images(images[:2], step=13)
        assert [r["step"] for r in rows] == [13, 13]
        assert [r["bytes"] for r in rows] == [len(b) for b in per_step[13][:2]]
        assert np.array_equal(rows[1]["recon"], net.decompress_images(per_step[13][1:2])[0])
        assert net.evaluate_images(images[:1])[0]["step"] is None


# ------------------------------------------------------------------ 6. budgets
@pytest.mark.parametrize("N", [128, 192])
def test_budgets(device, nets, images, N):
    net = nets(N)
    img = images[1]                     # the 64×96 image
    overhead = codec.blob_overhead(1)
    L = len(net.compress_images([img])[0])
    assert L // 2 > overhead + 300      # the halved budget is well above the floor
    est = net.rate_sweep(batch([img], device)).cpu().numpy()[0]
    chosen = []
    for budget in (5 * L // 4, 3 * L // 4, L // 2):
        stats = {}
        blob = net.compress_images([img], max_bytes=budget, stats=stats)[0]
        s = codec.parse_blob(blob)[1]
        print(f"N={N} L={L} budget {budget}: step {s}, {len(blob)} bytes, estimate "
              f"{math.ceil(est[s] / 8) + overhead}, re-encodes {stats['reencodes']}")
        assert len(blob) <= budget
        assert blob == net.compress_images([img], step=s)[0]
        if s > 0:
            finer = net.compress_images([img], step=s - 1)[0]
            assert len(finer) > budget or math.ceil(est[s - 1] / 8) + overhead > budget
        chosen.append(s)
    assert chosen[0] < chosen[1] < chosen[2]
    # per-image budgets in one mixed batch: per-image steps, each what the image gets alone
    group = images[:4]
    sizes = [len(b) for b in net.compress_images(group)]
    budgets = [5 * sizes[0] // 4, sizes[1] // 2, 3 * sizes[2] // 4, sizes[3] // 2]
    blobs = net.compress_images(group, max_bytes=budgets)
    steps = [codec.parse_blob(b)[1] for b in blobs]
    assert all(len(b) <= m for b, m in zip(blobs, budgets)) and len(set(steps)) > 1
    for im, m, b in zip(group, budgets, blobs):
        assert net.compress_images([im], max_bytes=m) == [b]
    rows = net.evaluate_images(group, max_bytes=budgets)
    assert [r["step"] for r in rows] == steps and [r["bytes"] for r in rows] == [len(b) for b in blobs]
    # bpp is a budget of ⌊bpp·H·W/8⌋ bytes on the true size
    assert net.compress_images(group, bpp=2.0) == net.compress_images(
        group, max_bytes=[2 * H * W // 8 for H, W in MIXED])
    assert net.compress_images(group[:2], bpp=[3.0, 1.5]) == net.compress_images(
        group[:2], max_bytes=[3 * 49 * 83 // 8, 3 * 64 * 96 // 16])
    with pytest.raises(kernels.Iclr17Error, match="image 1 .* budget of 100 bytes: the coarsest step gives"):
        net.compress_images(group[:2], max_bytes=[10 ** 6, 100])


# ------------------------------------------------------------------ 7. sizes along the ladder
def test_sizes_fall_along_the_ladder(device, nets, images):
    net = nets(128)
    sizes = [len(net.compress_images(images[1:2], step=s)[0]) for s in (4, 8, 12, 16)]
    print("bytes at steps 4, 8, 12, 16:", sizes)
    assert sizes[0] > sizes[1] > sizes[2] > sizes[3]


def test_command_line(device, nets, images, tmp_path, capsys):
    import json

    from PIL import Image
    net, img = nets(128), images[1]
    src, out, back = tmp_path / "in.png", tmp_path / "out.i17c", tmp_path / "back.png"
    ckpt = tmp_path / "iter_0.pth.tar"
    Image.fromarray(img).save(src)
    torch.save(net.state_dict(), ckpt)
    common = ["--weights", str(ckpt), "--N", "128"]
    for flags, kw in ((["--step", "13"], {"step": 13}), (["--max-bytes", "1500"], {"max_bytes": 1500}),
                      (["--bpp", "2.0"], {"bpp": 2.0})):
        assert codec.main(["encode", str(src), str(out), *common, *flags]) == 0
        blob = net.compress_images([img], **kw)[0]
        assert out.read_bytes() == blob and blob[:4] == b"I17Q"
        assert codec.main(["decode", str(out), str(back), *common]) == 0
        with Image.open(back) as im:
            assert np.array_equal(np.asarray(im), net.decompress_images([blob])[0])
    with pytest.raises(SystemExit):   # argparse: the options exclude each other
        codec.main(["encode", str(src), str(out), *common, "--step", "8", "--bpp", "1.0"])
    capsys.readouterr()
    assert codec.main(["eval", str(src), str(src), *common, "--steps", "4,12"]) == 0
    rows = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    assert [(r["name"], r["step"]) for r in rows] == [
        (str(src), 4), (str(src), 4), ("mean", 4), (str(src), 12), (str(src), 12), ("mean", 12)]
    want = net.evaluate_images([img], step=12)[0]
    assert rows[3]["bytes"] == want["bytes"] and rows[3]["psnr_u8"] == want["psnr_u8"]
    assert rows[5]["images"] == 2 and rows[5]["bpp"] == pytest.approx(want["bpp"], rel=1e-12)


# ------------------------------------------------------------------ 8. bf16
def test_bf16_round_trip(device, nets, images):
    net = nets(128)
    group = images[:2]
    with kernels.precision_scope("bf16"):
        y = net.latents(batch(group, device))
        for s in (5, 13):
            blobs = net.compress_images(group, step=s)
            dec = net.decompress([b[codec.HEADER.size:] for b in blobs], (4, 6), step=s)
            assert torch.equal(dec["y_hat"], kernels.quantise_step(y, DELTAS[s])[0].permute(0, 3, 1, 2))
            first = net.decompress_images(blobs)
            for a, b in zip(first, net.decompress_images(blobs, max_batch=1)):
                assert np.array_equal(a, b)
            assert net.compress_images(group, step=s, max_batch=1) == blobs
