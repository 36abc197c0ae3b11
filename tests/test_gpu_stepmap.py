"""Per-block quantiser steps on the GPU (csrc/stepmap.hip, the mapped coder of
csrc/rans.hip and the layers above): the mapped quantiser bit for bit against torch, the coder word
for word against the oracle with a table row per symbol, constant maps against the single-step
path, batch independence, the offset sweep against rate_sweep (exactly) and float64, budgeted ROI
encodes and corrupt blobs. The shapes are the smallest at which each path can go wrong. The weights
are synthetic: nothing here is a statement about quality."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stepmap_refs as R
from iclr_17_compression_amd import codec, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor
from oracle import rans_ref

pytestmark = pytest.mark.gpu

METRIC_REL = 1e-5                                   # rate_sweep's standing bar
LADDER = [codec.step_size(s) for s in range(codec.STEPS)]
MIXED = [(49, 83), (64, 96), (50, 96), (64, 81)]    # one canvas, 64×96: latent 4×6

# name: (B, h, w, g, N, P, K, distinct indices wanted)
CASES = {
    "1x1": (1, 1, 1, 1, 128, 1, 32, 1),
    # HW = 9 < 64: a rANS block spans 8 channels; 9 table sets leave a window of 27 < 32 channels
    "3x3": (1, 3, 3, 1, 128, 4, 32, 9),
    # ragged blocks on both edges, three images with three maps, escapes (K = 4) in mapped regions
    "5x7": (3, 5, 7, 4, 128, 1, 4, 4),
    # all 32 indices in one image: a window of 7 of the stream's 32 channels
    "8x4": (1, 8, 4, 1, 128, 4, 32, 32),
    # the defaults N = 192, P = 1, K = 32 with 16 table sets: a window of 15 of 192 channels
    "16x16": (1, 16, 16, 4, 192, 1, 32, 16),
    # the defaults with all 32 indices in one image: 1.6 MB of tables, a window of 7 channels
    "8x8": (1, 8, 8, 1, 192, 1, 32, 32),
}


def smooth(seed, H, W):
    return np.ascontiguousarray(synth.smooth_image_u8(seed, H, W).transpose(1, 2, 0))


def padded(im, Hc, Wc):
    H, W = im.shape[:2]
    x = torch.from_numpy(im).permute(2, 0, 1).float().div(255)[None]
    return F.pad(x, (0, Wc - W, 0, Hc - H), mode="replicate")


def to_u8(x_hat):
    return torch.round(x_hat.clamp(0, 1) * 255).to(torch.uint8)


def batch(imgs, device):
    Hc, Wc = codec.canvas(*imgs[0].shape[:2])
    return torch.cat([padded(im, Hc, Wc) for im in imgs]).to(device)


@pytest.fixture(scope="module")
def nets(device):
    made = {}

    def get(N):
        if N not in made:
            n = ImageCompressor(out_channel_N=N)
            n.load_state_dict({k: torch.from_numpy(v)
                               for k, v in synth.trained_like_state_dict(N, 1).items()})
            made[N] = n.to(device).eval()
        return made[N]
    return get


@pytest.fixture(scope="module")
def images():
    """The mixed 64×96-canvas group, then a 1×1 image."""
    return [smooth(60 + k, H, W) for k, (H, W) in enumerate(MIXED)] + [smooth(70, 1, 1)]


@pytest.fixture(scope="module")
def cases(device, nets):
    """Per case, made once: y (CPU and device), the index map, the definition's ŷ and Δ·ŷ, the
    stacked tables of the indices the map uses and the map as slots."""
    made = {}

    def get(name):
        if name in made:
            return made[name]
        B, h, w, g, N, P, K, distinct = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        mh, mw = -(-h // g), -(-w // g)
        idx = np.empty((B, mh * mw), np.uint8)
        for b in range(B):   # `distinct` different indices per image where the map has room
            pool = rng.permutation(32)[:distinct]
            if pool.min() > 3:
                pool[0] = b % 4   # a fine step in every image: |ŷ| beyond K, so escapes
            idx[b] = np.resize(pool, mh * mw)
            assert len(np.unique(idx[b])) == min(distinct, mh * mw)
        idx = idx.reshape(B, mh, mw)
        y = rng.uniform(-40.0, 40.0, size=(B, h, w, N)).astype(np.float32)
        flat = y.reshape(-1)
        flat[:8] = [0.0, -0.0, 0.5, 1.5, -2.5, 1e-30, 39.99, -39.99][:flat.size]
        y = torch.from_numpy(y)
        y_hat, y_deq = R.quantise(y, idx, g)
        used = [int(e) for e in np.unique(idx)]
        lut = np.zeros(32, np.uint8)
        lut[used] = np.arange(len(used))
        tables = torch.stack([nets(N).bitEstimator.entropy_tables(K, step=e) for e in used])
        made[name] = dict(y=y, yd=y.to(device), idx=idx, y_hat=y_hat, y_deq=y_deq, tables=tables,
                          slots=lut[idx], used=used)
        return made[name]
    return get


def bits_equal(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


# ------------------------------------------------------------------ 1. the quantiser is exact
@pytest.mark.parametrize("name", list(CASES))
def test_quantise_map_is_the_definition(device, cases, name):
    B, h, w, g, N, P, K, _ = CASES[name]
    c = cases(name)
    y_hat, y_deq = kernels.quantise_step_map(c["yd"], c["idx"], g, LADDER)
    assert bits_equal(y_hat, c["y_hat"]) and bits_equal(y_deq, c["y_deq"])
    assert bits_equal(kernels.dequantise_step_map(y_hat, c["idx"], g, LADDER), c["y_deq"])
    # the map as a torch tensor, on the host or the device
    for m in (torch.from_numpy(c["idx"]), torch.from_numpy(c["idx"]).to(device)):
        assert bits_equal(kernels.quantise_step_map(c["yd"], m, g, LADDER)[0], c["y_hat"])
    # a constant map is quantise_step
    for s in (0, 8, 31):
        const = np.full_like(c["idx"], s)
        for got, want in zip(kernels.quantise_step_map(c["yd"], const, g, LADDER),
                             kernels.quantise_step(c["yd"], LADDER[s])):
            assert bits_equal(got, want)


def test_quantise_map_rejections(device, cases):
    c = cases("5x7")
    yd, idx = c["yd"], c["idx"]
    for value, text in ((float("nan"), "a latent is NaN"), (float("inf"), "> 32767")):
        bad = yd.clone()
        bad[2, 4, 6, 127] = value   # the last element
        with pytest.raises(kernels.Iclr17Error, match=text):
            kernels.quantise_step_map(bad, idx, 4, LADDER)
    for m, g, text in ((idx[:2], 4, "indices must be integers of shape [3, 2, 2]"),
                       (idx, 2, "indices must be integers of shape [3, 3, 4]"),
                       (idx.astype(np.float32), 4, "indices must be integers"),
                       (idx.astype(np.int64) + 32, 4, "indices must lie in 0..31"),
                       (idx.astype(np.int64) - 32, 4, "indices must lie in 0..31"),
                       (idx, 3, "block edge 3")):
        for fn in (kernels.quantise_step_map, kernels.dequantise_step_map):
            with pytest.raises(kernels.Iclr17Error) as err:
                fn(yd, m, g, LADDER)
            assert text in str(err.value)
    with pytest.raises(kernels.Iclr17Error, match="31 ladder steps"):
        kernels.quantise_step_map(yd, idx, 4, LADDER[:31])
    with pytest.raises(kernels.Iclr17Error, match="not finite and positive"):
        kernels.quantise_step_map(yd, idx, 4, [0.0] + LADDER[1:])


# ------------------------------------------------------------------ 2. the coder, word for word
@pytest.mark.parametrize("name", list(CASES))
def test_words_equal_the_oracle_and_decode_returns_the_latent(device, cases, name):
    B, h, w, g, N, P, K, _ = CASES[name]
    c = cases(name)
    y_hat = c["y_hat"].to(device)
    S = len(c["used"])
    assert (c["y_hat"].abs() > K).any()   # escapes in the mapped regions
    cum = c["tables"].cpu().numpy().astype(np.int64).reshape(S * N, 2 * K + 3)
    coded = {}
    for window in (True, False, None):
        words, offsets = kernels.rans_encode_map(y_hat, c["tables"], c["slots"], g, K, P,
                                                 window=window)
        coded[window] = (words, offsets)
        for wdec in (True, False):
            back = kernels.rans_decode_map(words, offsets, c["tables"], c["slots"], g, B, h, w, N,
                                           K, P, window=wdec)
            assert torch.equal(back.cpu(), c["y_hat"] + 0.0), (window, wdec)   # −0 codes as 0
    for window in (False, None):   # the two table sources write the same words
        assert torch.equal(coded[window][0], coded[True][0])
        assert torch.equal(coded[window][1], coded[True][1])
    words = coded[True][0].cpu().numpy().view(np.uint16)
    off = coded[True][1].cpu().numpy()
    assert off.shape == (B * P + 1,) and off[0] == 0 and off[-1] == words.size
    yh = c["y_hat"].numpy()
    for b in range(B):
        for grp in range(P):
            values, rows = R.stream_symbols(yh[b], c["slots"][b], g, N, P, grp)
            want = rans_ref.encode_stream(values, rows, cum, K)
            s = b * P + grp
            assert words[off[s]:off[s + 1]].tolist() == want, (b, grp)
    # a slot outside the stacked tables, and tables of another shape
    with pytest.raises(kernels.Iclr17Error, match=f"slots must lie in 0..{S - 1}"):
        kernels.rans_encode_map(y_hat, c["tables"], c["slots"].astype(np.int64) + S, g, K, P)
    with pytest.raises(kernels.Iclr17Error, match="stacked tables must be an int32 GPU tensor"):
        kernels.rans_encode_map(y_hat, c["tables"][0], c["slots"], g, K, P)
    with pytest.raises(kernels.Iclr17Error, match="a latent is not integer-valued"):
        kernels.rans_encode_map(y_hat + 0.25, c["tables"], c["slots"], g, K, P)


def test_decode_map_reports_corrupt_words(device, cases):
    B, h, w, g, N, P, K, _ = CASES["8x4"]
    c = cases("8x4")
    words, offsets = kernels.rans_encode_map(c["y_hat"].to(device), c["tables"], c["slots"], g, K, P)
    short = offsets.clone()
    short[-1] -= 1
    with pytest.raises(kernels.Iclr17Error, match="ran past its words|did not end in the initial state"):
        kernels.rans_decode_map(words, short, c["tables"], c["slots"], g, B, h, w, N, K, P)
    with pytest.raises(kernels.Iclr17Error, match="offsets do not match"):
        kernels.rans_decode_map(words, offsets[:-1], c["tables"], c["slots"], g, B, h, w, N, K, P)


# ------------------------------------------------------------------ 3. constant maps
@pytest.mark.parametrize("precision", ["x6", "h3"])
def test_constant_map_is_the_single_step_blob(device, nets, images, precision):
    net = nets(128)
    n = len(images)
    with kernels.precision_scope(precision):
        for s in (5, 13):
            stepped = net.compress_images(images, step=s)
            decoded = net.decompress_images(stepped)
            variants = [
                (net.compress_images(images, step=s, step_offsets=[None] * n), s, 4),
                (net.compress_images(images, step=s, step_offsets=[None] * n, block=1), s, 1),
                (net.compress_images(images, step_offsets=[
                    np.full(codec.map_shape(*im.shape[:2], 2), s - 8) for im in images], block=2), 8, 2)]
            for blobs, base, g in variants:
                for q, m, im in zip(stepped, blobs, images):
                    assert q[:4] == b"I17Q" and m[:4] == b"I17M"
                    head, smap = codec.parse_blob(m, N=128, fingerprint=codec.fingerprint(net))
                    assert head == codec.parse_blob(q)[0]
                    assert (smap.base, smap.block) == (base, g)
                    assert smap.indices.shape == codec.map_shape(*im.shape[:2], g)
                    assert (smap.indices == s).all()
                    assert m[smap.payload:] == q[codec.HEADER.size:]
                for a, b in zip(net.decompress_images(blobs), decoded):
                    assert np.array_equal(a, b)
        # offsets alone: the unit step, and still a mapped blob
        unit = net.compress_images(images, step=codec.UNIT_STEP)
        for q, m in zip(unit, net.compress_images(images, step_offsets=[None] * n)):
            smap = codec.parse_blob(m)[1]
            assert m[:4] == b"I17M" and smap.base == 8 and (smap.indices == 8).all()
            assert m[smap.payload:] == q[codec.HEADER.size:]
        assert net.compress_images(images, step=5) == net.compress_images(images, step=5)


# ------------------------------------------------------------------ 4. batches and round trips
@pytest.mark.parametrize("precision", ["x6", "h3"])
def test_round_trip_and_batch_independence(device, nets, images, precision):
    net = nets(128)
    rng = np.random.default_rng(11)
    g, base = 2, 10
    offs = [rng.integers(-12, 13, size=codec.map_shape(*im.shape[:2], g)) for im in images]
    offs[2] = None
    with kernels.precision_scope(precision):
        blobs = net.compress_images(images, step=base, step_offsets=offs, block=g)
        for i, (im, off) in enumerate(zip(images, offs)):
            assert net.compress_images([im], step=base, step_offsets=[off], block=g) == [blobs[i]]
        assert net.compress_images(images, step=base, step_offsets=offs, block=g, max_batch=2) == blobs
        # the stream's map is clamp(base + offset), and the payload decodes to the definition's ŷ
        group = images[:4]
        y = net.latents(batch(group, device))
        emap = np.stack([R.effective(base, np.zeros((2, 3), int) if o is None else o)
                         for o in offs[:4]]).astype(np.uint8)
        parsed = [codec.parse_blob(b) for b in blobs[:4]]
        for (head, smap), m in zip(parsed, emap):
            assert (smap.base, smap.block) == (base, g) and np.array_equal(smap.indices, m)
        y_hat, y_deq = kernels.quantise_step_map(y, emap, g, LADDER)
        dec = net.decompress([b[s.payload:] for b, (_, s) in zip(blobs, parsed)], (4, 6),
                             step_map=emap, block=g)
        assert torch.equal(dec["y_hat"], y_hat.permute(0, 3, 1, 2))
        with torch.no_grad():
            want = to_u8(net.Decoder(y_deq.permute(0, 3, 1, 2).contiguous()).clamp(0, 1).cpu())
        decoded = net.decompress_images(blobs)
        for k, (im, got) in enumerate(zip(group, decoded)):
            H, W = im.shape[:2]
            assert got.dtype == np.uint8 and got.shape == (H, W, 3)
            assert np.array_equal(got, want[k, :, :H, :W].permute(1, 2, 0).numpy()), k
        # all three kinds of blob in one call, each decoding to what it decodes to alone
        mixed = [blobs[0], net.compress_images(images[1:2])[0], blobs[3],
                 net.compress_images(images[2:3], step=13)[0], blobs[4], blobs[1],
                 net.compress_images(images[:1], step=base, step_offsets=[offs[0][:1, :2]], block=4)[0]]
        alone = [net.decompress_images([b])[0] for b in mixed]
        for batchsize in (64, 2):
            for a, b in zip(net.decompress_images(mixed, max_batch=batchsize), alone):
                assert np.array_equal(a, b)
        assert np.array_equal(alone[0], decoded[0]) and np.array_equal(alone[4], decoded[4])
        rows = net.evaluate_images(group, step=base, step_offsets=offs[:4], block=g)
        assert [r["step"] for r in rows] == [base] * 4 and [r["block"] for r in rows] == [g] * 4
        assert [r["bytes"] for r in rows] == [len(b) for b in blobs[:4]]
        assert all(np.array_equal(r["step_map"], m) for r, m in zip(rows, emap))
        assert np.array_equal(rows[1]["recon"], decoded[1])


# ------------------------------------------------------------------ 5. the offset sweep
def sweep_inputs(net, images, device, N):
    """(y, block edge) pairs: the 64×96-canvas group's latent [4,4,6,N], a 1×1 latent, and a
    16×16 latent of 12 sweep chunks at N = 192."""
    rng = np.random.default_rng(5)
    with kernels.precision_scope("x6"):
        ys = [(net.latents(batch(images[:4], device)), 4), (net.latents(batch(images[:4], device)), 1),
              (net.latents(batch(images[4:], device)), 1)]
    big = net.latents(batch([smooth(80, 256, 256)], device))
    assert tuple(big.shape) == (1, 16, 16, N)
    return ys + [(big, 4), (big + torch.from_numpy(
        rng.normal(0, 0.3, size=tuple(big.shape)).astype(np.float32)).to(device), 8)]


@pytest.mark.parametrize("N", [128, 192])
def test_sweep_offsets_equal_rate_sweep(device, nets, images, N):
    net = nets(N)
    pack = net.bitEstimator.packed()
    for y, g in sweep_inputs(net, images, device, N):
        B, h, w, _ = y.shape
        mh, mw = kernels.map_shape(h, w, g)
        sweep = kernels.rate_sweep(y, pack, LADDER)
        zero = kernels.rate_sweep_offsets(y, pack, LADDER, np.zeros((B, mh, mw), np.int8), g)
        assert zero.dtype == torch.float64 and tuple(zero.shape) == (B, 32)
        assert torch.equal(zero, sweep), (tuple(y.shape), g)
        # one offset per image: the shifted, clamped row, exactly
        for consts in ([-3, 5, -31, 31], [1, -1, 12, -12]):
            cs = np.array(consts[:B])
            off = np.broadcast_to(cs[:, None, None], (B, mh, mw))
            got = kernels.rate_sweep_offsets(y, pack, LADDER, off, g)
            rows = np.clip(np.arange(32)[None, :] + cs[:, None], 0, 31)
            want = torch.gather(sweep, 1, torch.from_numpy(rows).to(device))
            assert torch.equal(got, want), (tuple(y.shape), g, consts)
        assert torch.equal(net.rate_sweep_offsets(y, np.zeros((B, mh, mw), int), g), sweep)
    y, g = sweep_inputs(net, images, device, N)[0]
    for off, text in ((np.zeros((4, 1, 3), int), "offsets must be integers of shape [4, 1, 2]"),
                      (np.full((4, 1, 2), 32), "offsets must lie in -31..31"),
                      (np.zeros((4, 1, 2)), "offsets must be integers")):
        with pytest.raises(kernels.Iclr17Error) as err:
            kernels.rate_sweep_offsets(y, pack, LADDER, off, g)
        assert text in str(err.value)


@pytest.mark.parametrize("N", [128, 192])
def test_sweep_offsets_against_float64(device, nets, images, N):
    net = nets(N)
    pack = net.bitEstimator.packed()
    rng = np.random.default_rng(6)
    for y, g in sweep_inputs(net, images, device, N):
        B, h, w, _ = y.shape
        off = rng.integers(-12, 13, size=(B,) + kernels.map_shape(h, w, g))
        got = kernels.rate_sweep_offsets(y, pack, LADDER, off, g).cpu().numpy()
        want = R.sweep_f64(y.cpu().numpy(), pack.cpu().numpy().reshape(11, N), off, g)
        rel = np.abs(got - want) / np.abs(want)
        print(f"offset sweep vs float64 N={N} {tuple(y.shape)} g={g}: max rel {rel.max():.3e} at "
              f"base {int(rel.max(axis=0).argmax())}")
        assert rel.max() <= METRIC_REL
        assert torch.equal(kernels.rate_sweep_offsets(y, pack, LADDER, off, g).cpu(),
                           torch.from_numpy(got))   # reproducible


# ------------------------------------------------------------------ 6. budgets
@pytest.mark.parametrize("N", [128, 192])
def test_budgeted_roi_encode(device, nets, images, N):
    net = nets(N)
    img, g = images[1], 2                      # the 64×96 image: latent 4×6, a 2×3 map
    off = np.array([[-4, 0, 0], [0, 0, 3]])
    overhead = codec.blob_overhead(1) + off.size
    L = len(net.compress_images([img])[0])
    assert L // 2 > overhead + 300
    y = net.latents(batch([img], device))
    est = net.rate_sweep_offsets(y, off[None], g).cpu().numpy()[0]
    sizes = [math.ceil(b / 8) + overhead for b in est]
    bases = []
    for budget in (5 * L // 4, 3 * L // 4, L // 2):
        stats = {}
        blob = net.compress_images([img], max_bytes=budget, step_offsets=[off], block=g, stats=stats)[0]
        head, smap = codec.parse_blob(blob, N=N, fingerprint=codec.fingerprint(net))
        first = min(s for s in range(32) if sizes[s] <= budget)
        print(f"N={N} L={L} budget {budget}: base {smap.base} (first {first}), {len(blob)} bytes, "
              f"estimate {sizes[smap.base]}, re-encodes {stats['reencodes']}")
        assert len(blob) <= budget and blob[:4] == b"I17M"
        # the first base is the finest whose estimate fits; the loop only moves coarser from it
        assert smap.base == first + stats["reencodes"][0]
        assert smap.block == g and np.array_equal(smap.indices, R.effective(smap.base, off))
        assert blob == net.compress_images([img], step=smap.base, step_offsets=[off], block=g)[0]
        if stats["reencodes"][0]:
            finer = net.compress_images([img], step=smap.base - 1, step_offsets=[off], block=g)[0]
            assert len(finer) > budget
        dec = net.decompress([blob[smap.payload:]], (4, 6), step_map=smap.indices[None], block=g)
        want = kernels.quantise_step_map(y, smap.indices[None], g, LADDER)[0]
        assert torch.equal(dec["y_hat"], want.permute(0, 3, 1, 2))
        bases.append(smap.base)
    assert bases[0] < bases[1] < bases[2]
    # per-image budgets and maps in one batch: each image gets what it gets alone
    group = images[:4]
    offs = [off, None, -off, np.full((2, 3), 6)]
    budgets = [3 * L // 4, L // 2, L, 2 * L // 3]
    blobs = net.compress_images(group, max_bytes=budgets, step_offsets=offs, block=g)
    assert all(len(b) <= m for b, m in zip(blobs, budgets))
    assert len({codec.parse_blob(b)[1].base for b in blobs}) > 1
    for im, m, o, b in zip(group, budgets, offs, blobs):
        assert net.compress_images([im], max_bytes=m, step_offsets=[o], block=g) == [b]
    assert net.compress_images(group[:2], bpp=[3.0, 1.5], step_offsets=offs[:2], block=g) == \
        net.compress_images(group[:2], max_bytes=[3 * 49 * 83 // 8, 3 * 64 * 96 // 16],
                            step_offsets=offs[:2], block=g)
    with pytest.raises(kernels.Iclr17Error, match="image 1 .* budget of 100 bytes: the coarsest step gives"):
        net.compress_images(group[:2], max_bytes=[10 ** 6, 100], step_offsets=offs[:2], block=g)


# ------------------------------------------------------------------ 7. corrupt blobs, command line
def test_corrupt_blobs_raise(device, nets, images):
    net = nets(128)
    off = np.array([[-4, 0, 0], [0, 0, 3]])
    blob = net.compress_images(images[1:2], step=10, step_offsets=[off], block=2)[0]
    smap = codec.parse_blob(blob)[1]
    assert smap.payload == 28 + 6 and np.array_equal(net.decompress_images([blob])[0],
                                                     net.decompress_images([blob, blob])[1])
    for bad, text in ((blob[:30] + b"\x20" + blob[31:], "quantiser step 32 in the stream's step map"),
                      (blob[:33] + b"\xff" + blob[34:], "quantiser step 255 in the stream's step map"),
                      (blob[:11] + b"\x05" + blob[12:], "step-map block of 2^5"),
                      (blob[:31], "truncated step map (3 of 6 bytes)"),
                      (blob[:36], "truncated stream (36 bytes)"),
                      (blob[:-1], "truncated stream"),
                      (blob[:-2], "stream lengths do not match the payload"),
                      (blob[:20], "truncated header")):
        with pytest.raises(kernels.Iclr17Error) as err:
            net.decompress_images([bad])
        assert text in str(err.value), text


def test_command_line_roi(device, nets, images, tmp_path):
    from PIL import Image
    net, img = nets(128), images[1]
    src, out, back = tmp_path / "in.png", tmp_path / "out.i17c", tmp_path / "back.png"
    ckpt = tmp_path / "iter_0.pth.tar"
    Image.fromarray(img).save(src)
    torch.save(net.state_dict(), ckpt)
    common = ["--weights", str(ckpt), "--N", "128"]
    boxes = [(10, 5, 40, 30, -4), (60, 0, 96, 64, 3)]
    roi = ["--roi", "10,5,40,30,-4", "--roi", "60,0,96,64,3"]
    for flags, kw, g in (([], {}, 4), (["--step", "13", "--block", "2"], {"step": 13}, 2),
                         (["--bpp", "2.0", "--block", "1"], {"bpp": 2.0}, 1)):
        assert codec.main(["encode", str(src), str(out), *common, *roi, *flags]) == 0
        blob = net.compress_images([img], step_offsets=[codec.roi_offsets(64, 96, boxes, g)],
                                   block=g, **kw)[0]
        assert out.read_bytes() == blob and blob[:4] == b"I17M"
        assert len(np.unique(codec.parse_blob(blob)[1].indices)) > 1
        assert codec.main(["decode", str(out), str(back), *common]) == 0
        with Image.open(back) as im:
            assert np.array_equal(np.asarray(im), net.decompress_images([blob])[0])
    with pytest.raises(kernels.Iclr17Error, match="--roi takes X0,Y0,X1,Y1,OFF"):
        codec.main(["encode", str(src), str(out), *common, "--roi", "1,2,3"])
