"""Centroid reconstruction on the GPU (csrc/recon.hip and the layers above): the
offset tables against the float64 definition, both dequantisers bit for bit against numpy and, with
a zero table, against the dequantisers they stand beside, batch independence, and the decode
surface byte for byte — every blob kind in one call, the region decode, evaluate_images' rows.
The shapes are the smallest at which each path can go wrong. The weights are synthetic: nothing
here is a statement about quality."""
import math

import numpy as np
import pytest
import torch

import recon_refs as C
from iclr_17_compression_amd import codec, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor

pytestmark = pytest.mark.gpu

LADDER = [codec.step_size(s) for s in range(codec.STEPS)]
MIXED = [(49, 83), (64, 96), (50, 96), (64, 81)]    # one canvas, 64×96: latent 4×6
INDICES = (0, 8, 13, 31)
OFFSET_BAR = 1e-6     # of a level: fp32 storage ≤ 3e-8, libm differences / p ≤ 2e-8


def smooth(seed, H, W):
    return np.ascontiguousarray(synth.smooth_image_u8(seed, H, W).transpose(1, 2, 0))


def to_u8(x_hat):
    return torch.round(x_hat.clamp(0, 1) * 255).to(torch.uint8)


def bits_equal(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), np.asarray(b).view(np.int32))


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
    return [smooth(60 + k, H, W) for k, (H, W) in enumerate(MIXED)]


def pack_of(net):
    """The device's own fp32 rate pack on the host, [11, N]: the values the kernel reads."""
    return net.bitEstimator.packed().cpu().numpy().reshape(11, net.out_channel_N)


def levels(rng, shape, K):
    """ŷ with 0, ±1, ±K, ±(K + 1), ±32767 among random levels a little beyond ±K."""
    y = rng.integers(-K - 2, K + 3, size=shape).astype(np.float32)
    special = [0, 1, -1, K, -K, K + 1, -K - 1, 32767, -32767]
    flat = y.reshape(-1)
    at = rng.permutation(flat.size)[:4 * len(special)]
    flat[at] = np.resize(np.array(special, np.float32), at.size)
    return y


def random_tables(rng, *shape):
    return rng.uniform(-0.5, 0.5, size=shape).astype(np.float32)


# ------------------------------------------------------------------ 1. the tables
@pytest.mark.parametrize("N,K", [(128, 4), (128, 32), (192, 4), (192, 32)])
def test_offsets_against_float64(device, nets, N, K):
    net = nets(N)
    pack = pack_of(net)
    with np.errstate(over="ignore"):
        full, prob = zip(*[C.full_offsets(pack, K, e) for e in INDICES])
    low = np.stack(prob) < C.P_MIN
    steps = [LADDER[e] for e in INDICES]
    worst = 0.0
    for mode in ("centroid", "zero"):
        for a in (1.0, 0.5):
            got = kernels.recon_offsets(net.bitEstimator.packed(), N, K, steps, mode, a)
            assert got.shape == (4, N, 2 * K + 1) and got.dtype == torch.float32
            got = got.cpu().numpy()
            want = np.stack([C.table_of(f, K, mode, a) for f in full])
            assert np.abs(got).max() <= 0.5 * a
            if mode == "zero":
                assert not got[:, :, np.arange(2 * K + 1) != K].any()
            assert not got[low].any()                    # low-p entries are switched off
            worst = max(worst, np.abs(got.astype(np.float64) - want).max())
    print(f"recon_offsets N={N} K={K}: max |kernel − float64| = {worst:.3e} of a level")
    assert worst <= OFFSET_BAR
    zero = kernels.recon_offsets(net.bitEstimator.packed(), N, K, steps, "centroid", 0.0)
    assert not zero.any()
    again = kernels.recon_offsets(net.bitEstimator.packed(), N, K, steps[1:2], "zero", 0.5)
    assert torch.equal(again[0], torch.from_numpy(got[1]).to(device))   # a step alone: the same row


def test_offsets_are_cached_on_the_parameters(device, nets):
    be = nets(128).bitEstimator
    a = be.recon_offsets(4, 12, "centroid", 0.5)
    assert a.shape == (128, 9) and be.recon_offsets(4, 12, "centroid", 0.5) is a
    assert be.recon_offsets(4, 12, "centroid", 1.0) is not a
    s = be.stacked_recon_offsets(4, [3, 12], "centroid", 0.5)
    assert be.stacked_recon_offsets(4, [3, 12], "centroid", 0.5) is s and torch.equal(s[1], a)
    assert be.stacked_recon_offsets(4, [3, 12], "zero", 0.5) is not s
    with torch.no_grad():
        be.f1.b.add_(0.0)       # an in-place touch of a parameter: the version moves
    assert be.recon_offsets(4, 12, "centroid", 0.5) is not a


# ------------------------------------------------------------------ 2. a zero table
def test_zero_table_is_the_plain_dequantiser(device):
    rng = np.random.default_rng(1)
    for shape, K, g in (((2, 5, 7, 128), 4, 4), ((1, 3, 3, 192), 32, 1), ((1, 3, 3, 192), 64, 2)):
        B, h, w, N = shape
        y = torch.from_numpy(levels(rng, shape, K)).to(device)
        zero = torch.zeros(N, 2 * K + 1, device=device)
        for e in (3, 12):
            assert torch.equal(kernels.dequantise_recon(y, LADDER[e], zero, K),
                               kernels.dequantise_step(y, LADDER[e]))
        idx = rng.integers(0, 32, size=(B,) + kernels.map_shape(h, w, g)).astype(np.uint8)
        got = kernels.dequantise_recon_map(y, idx, g, LADDER, zero.expand(32, -1, -1).contiguous(), K)
        assert torch.equal(got, kernels.dequantise_step_map(y, idx, g, LADDER))


# ------------------------------------------------------------------ 3. one step, bit for bit
@pytest.mark.parametrize("shape,K", [((2, 5, 7, 128), 4), ((2, 5, 7, 128), 32),
                                     ((1, 3, 3, 192), 4), ((1, 3, 3, 192), 32),
                                     ((1, 3, 3, 192), 64)])   # K = 64: 99 KB, the global path
def test_dequantise_recon_is_the_definition(device, shape, K):
    rng = np.random.default_rng(K + shape[3])
    N = shape[3]
    y = levels(rng, shape, K)
    table = random_tables(rng, N, 2 * K + 1)
    for e in (5, 12, 31):
        got = kernels.dequantise_recon(torch.from_numpy(y).to(device), LADDER[e],
                                       torch.from_numpy(table).to(device), K)
        assert bits_equal(got, C.dequantise(y, table, K, e)), e
    odd = y.copy()      # what no decoder produces is still read inside the table, or not at all
    odd.reshape(-1)[:6] = [np.inf, -np.inf, np.nan, -0.0, K + 0.5, -K - 0.5]
    got = kernels.dequantise_recon(torch.from_numpy(odd).to(device), LADDER[12],
                                   torch.from_numpy(table).to(device), K).cpu().numpy()
    want = C.dequantise(odd, table, K, 12)
    assert np.array_equal(got, want, equal_nan=True)
    assert got.reshape(-1)[:2].tolist() == [np.inf, -np.inf] and math.isnan(got.reshape(-1)[2])


# ------------------------------------------------------------------ 4. a step per block
# (B, h, w, g, N, K, distinct indices): ragged blocks and three maps; all 32 indices in one image
MAPPED = {"5x7": (3, 5, 7, 4, 128, 4, 4), "8x8": (1, 8, 8, 1, 192, 32, 32)}


@pytest.mark.parametrize("name", list(MAPPED))
def test_dequantise_recon_map_is_the_definition(device, name):
    B, h, w, g, N, K, distinct = MAPPED[name]
    rng = np.random.default_rng(len(name) + N)
    mh, mw = kernels.map_shape(h, w, g)
    idx = np.stack([np.resize(rng.permutation(32)[:distinct], mh * mw) for _ in range(B)])
    idx = idx.reshape(B, mh, mw).astype(np.uint8)
    used = [int(e) for e in np.unique(idx)]
    assert len(used) >= distinct
    lut = np.zeros(32, np.uint8)
    lut[used] = np.arange(len(used))
    y = levels(rng, (B, h, w, N), K)
    tables = random_tables(rng, len(used), N, 2 * K + 1)       # one per slot
    by_index = np.zeros((32, N, 2 * K + 1), np.float32)
    by_index[used] = tables
    yd, td = torch.from_numpy(y).to(device), torch.from_numpy(tables).to(device)
    got = kernels.dequantise_recon_map(yd, lut[idx], g, [LADDER[e] for e in used], td, K)
    assert bits_equal(got, C.dequantise_map(y, idx, g, by_index, K))
    # a constant map is the one-step path
    e = used[-1]
    const = np.full((B, mh, mw), lut[e], np.uint8)
    assert torch.equal(kernels.dequantise_recon_map(yd, const, g, [LADDER[s] for s in used], td, K),
                       kernels.dequantise_recon(yd, LADDER[e], td[lut[e]], K))
    with pytest.raises(kernels.Iclr17Error, match="slots must lie in"):
        kernels.dequantise_recon_map(yd, np.full((B, mh, mw), len(used), np.uint8), g,
                                     [LADDER[s] for s in used], td, K)


def test_an_image_alone_equals_the_image_in_its_batch(device):
    rng = np.random.default_rng(9)
    B, h, w, g, N, K = 3, 5, 7, 4, 128, 4
    y = torch.from_numpy(levels(rng, (B, h, w, N), K)).to(device)
    tables = torch.from_numpy(random_tables(rng, 32, N, 2 * K + 1)).to(device)
    idx = rng.integers(0, 32, size=(B,) + kernels.map_shape(h, w, g)).astype(np.uint8)
    one = kernels.dequantise_recon(y, LADDER[12], tables[12], K)
    mapped = kernels.dequantise_recon_map(y, idx, g, LADDER, tables, K)
    for b in range(B):
        assert torch.equal(kernels.dequantise_recon(y[b:b + 1], LADDER[12], tables[12], K), one[b:b + 1])
        assert torch.equal(kernels.dequantise_recon_map(y[b:b + 1], idx[b:b + 1], g, LADDER, tables, K),
                           mapped[b:b + 1])


# ------------------------------------------------------------------ 5. the decode surface
def test_decompress_images_end_to_end(device, nets, images):
    net, K = nets(128), kernels.ENTROPY_K
    with kernels.precision_scope("x6"):
        plain = net.compress_images(images)
        stepped = net.compress_images(images, step=12)
        for blobs, step, e in ((stepped, 12, 12), (plain, None, 8)):   # a plain blob: index 8
            assert blobs[0][:4] == (b"I17C" if step is None else b"I17Q")
            y_hat = net.decompress([b[codec.HEADER.size:] for b in blobs], (4, 6), step=step)["y_hat"]
            y_hat = y_hat.permute(0, 2, 3, 1).contiguous().cpu().numpy()
            table = net.bitEstimator.recon_offsets(K, e, "zero", 1.0).cpu().numpy()
            with np.errstate(over="ignore"):
                ref = C.offsets(pack_of(net), K, [e], "zero", 1.0)[0]
            assert np.abs(table.astype(np.float64) - ref).max() <= OFFSET_BAR and table[:, K].any()
            y_deq = torch.from_numpy(C.dequantise(y_hat, table, K, e)).to(device)
            with torch.no_grad():
                want = to_u8(net.Decoder(y_deq.permute(0, 3, 1, 2).contiguous()).clamp(0, 1).cpu())
            got = net.decompress_images(blobs, recon="zero")
            for k, (im, g) in enumerate(zip(images, got)):
                H, W = im.shape[:2]
                assert g.dtype == np.uint8 and g.shape == (H, W, 3)
                assert np.array_equal(g, want[k, :, :H, :W].permute(1, 2, 0).numpy()), (step, k)
        # None and "centre" are the call without the argument
        base = net.decompress_images(stepped)
        for kw in ({"recon": None}, {"recon": "centre"}, {"recon": "centre", "recon_strength": 0.5},
                   {"recon": None, "recon_strength": 0.0}):
            for a, b in zip(net.decompress_images(stepped, **kw), base):
                assert np.array_equal(a, b)
        assert any(not np.array_equal(a, b)
                   for a, b in zip(net.decompress_images(stepped, recon="zero"), base))
        # strength 0 moves nothing
        for a, b in zip(net.decompress_images(stepped, recon="centroid", recon_strength=0.0), base):
            assert np.array_equal(a, b)
        # all four kinds of blob in one call, each decoding to what it decodes to alone
        offs = np.array([[-3, 2]])
        mixed = [plain[0], stepped[1],
                 net.compress_images(images[2:3], step=12, step_offsets=[offs])[0],
                 net.compress_images(images[3:4], step=12, tile=8)[0], stepped[0],
                 net.compress_images(images[:1], step=10, step_offsets=[None], block=2)[0]]
        assert [b[:4] for b in mixed[:4]] == [b"I17C", b"I17Q", b"I17M", b"I17T"]
        for kw in ({"recon": "centroid"}, {"recon": "zero", "recon_strength": 0.5}):
            alone = [net.decompress_images([b], **kw)[0] for b in mixed]
            for batchsize in (64, 2):
                for a, b in zip(net.decompress_images(mixed, max_batch=batchsize, **kw), alone):
                    assert np.array_equal(a, b)
        # the mapped blob against the definition: blocks at indices 9 and 14
        head, smap = codec.parse_blob(mixed[2])
        assert sorted(np.unique(smap.indices)) == [9, 14]
        dec = net.decompress([mixed[2][smap.payload:]], (4, 6), step_map=smap.indices[None], block=4)
        y_hat = dec["y_hat"].permute(0, 2, 3, 1).contiguous().cpu().numpy()
        by_index = np.zeros((32, 128, 2 * K + 1), np.float32)
        for e in (9, 14):
            by_index[e] = net.bitEstimator.recon_offsets(K, e, "centroid", 1.0).cpu().numpy()
        y_deq = torch.from_numpy(C.dequantise_map(y_hat, smap.indices[None], 4, by_index, K)).to(device)
        with torch.no_grad():
            want = to_u8(net.Decoder(y_deq.permute(0, 3, 1, 2).contiguous()).clamp(0, 1).cpu())
        H, W = images[2].shape[:2]
        got = net.decompress_images([mixed[2]], recon="centroid")[0]
        assert np.array_equal(got, want[0, :, :H, :W].permute(1, 2, 0).numpy())


def test_region_decode_is_the_crop(device, nets):
    net = nets(128)
    im = smooth(90, 200, 328)       # canvas 208×336: latent 13×21, 2×3 tiles of 8, ragged
    H, W = im.shape[:2]
    boxes = {"four-tile corner": (100, 110, 150, 140), "padded edge": (W - 37, H - 21, W, H)}
    with kernels.precision_scope("x6"):
        blob = net.compress_images([im], step=12, tile=8)[0]
        assert blob[:4] == b"I17T"
        centre = net.decompress_images([blob])[0]
        for kw in ({"recon": "centroid"}, {"recon": "zero", "recon_strength": 0.5}):
            full = net.decompress_images([blob], **kw)[0]
            assert not np.array_equal(full, centre)
            for name, (x0, y0, x1, y1) in boxes.items():
                stats = {}
                got = net.decompress_region(blob, (x0, y0, x1, y1), stats=stats, **kw)
                assert np.array_equal(got, full[y0:y1, x0:x1]), (kw, name)
                assert stats["streams_decoded"] <= stats["streams_total"] == 6
        x0, y0, x1, y1 = boxes["four-tile corner"]
        assert np.array_equal(net.decompress_region(blob, (x0, y0, x1, y1), recon="centre"),
                              centre[y0:y1, x0:x1])
        # a blob that is not tiled is decoded whole with the same arguments
        q = net.compress_images([im], step=12)[0]
        assert np.array_equal(net.decompress_region(q, (x0, y0, x1, y1), recon="centroid"),
                              net.decompress_images([q], recon="centroid")[0][y0:y1, x0:x1])


def test_evaluate_images_rows(device, nets, images):
    net = nets(128)
    with kernels.precision_scope("x6"):
        rows = net.evaluate_images(images, step=12, recon="centroid")
        plain = net.evaluate_images(images, step=12)
        blobs = net.compress_images(images, step=12)
        decoded = net.decompress_images(blobs, recon="centroid")
    for r, p, im, blob, dec in zip(rows, plain, images, blobs, decoded):
        H, W = im.shape[:2]
        assert r["bytes"] == p["bytes"] == len(blob) and r["step"] == 12     # the same bits
        assert (r["recon_mode"], r["recon_strength"]) == ("centroid", 1.0)
        assert "recon_mode" not in p
        assert np.array_equal(r["recon"], dec)
        sse = int(((r["recon"].astype(np.int64) - im.astype(np.int64)) ** 2).sum())
        assert r["sse_u8"] == sse
        assert r["psnr_u8"] == 10.0 * math.log10(255.0 ** 2 * 3 * H * W / sse)
    assert any(r["sse_u8"] != p["sse_u8"] for r, p in zip(rows, plain))
    for kw in ({"psnr": 30.0}, {"msssim": 0.9}, {"step": 12, "refine": 2, "refine_lambda": 650.25}):
        with pytest.raises(kernels.Iclr17Error, match="is not built"):
            net.evaluate_images(images[:1], recon="zero", **kw)
