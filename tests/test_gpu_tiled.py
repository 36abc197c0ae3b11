"""Tiled rANS streams on the GPU (the tiled kernels of csrc/rans.hip and the layers
above): every tile's words against the oracle's encode_stream of its sequence, decode bit for bit
(whole and by rectangle, at every workgroup shape), the tiled blob against the untiled one of the
same step (latents and decoded bytes), RDO, region decode against the crop of the full decode,
batches and mixed kinds, budgets with the tile overhead, corrupt words and the command line.

Shapes: 200×328 images travel on a 208×336 canvas, a latent of 13×21; at t = 8 that is 2×3 tiles,
ragged in both directions, the corner tile 5×5 (25 symbols per channel: a 64-symbol block spans
channels). 40×24 gives a latent of 3×2, smaller than one tile. The weights are synthetic: nothing
here is a statement about quality."""
import numpy as np
import pytest
import torch

from iclr_17_compression_amd import codec, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor
from oracle import rans_ref

pytestmark = pytest.mark.gpu

SIZES = [(200, 328), (193, 321), (208, 336)]     # one canvas, 208×336
SMALL = (40, 24)
CORRUPT = "ran past its words|did not end in the initial state"


def smooth(seed, H, W):
    return np.ascontiguousarray(synth.smooth_image_u8(seed, H, W).transpose(1, 2, 0))


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
    """Three images of one canvas, then the one smaller than a tile."""
    return [smooth(90 + k, H, W) for k, (H, W) in enumerate(SIZES)] + [smooth(99, *SMALL)]


def latents_of(net, blob):
    """The decoded ŷ (NCHW) of one blob of any stepped or tiled kind."""
    head, info = codec.parse_blob(blob)
    Hc, Wc = codec.canvas(head.H, head.W)
    how = {"step": info.step, "tile": info.tile} if isinstance(info, codec.TileInfo) else {"step": info}
    return net.decompress([blob[codec.HEADER.size:]], (Hc // 16, Wc // 16),
                          streams_per_image=head.P, K=head.K, **how)["y_hat"]


# ------------------------------------------------------------------ 1. the coder, word for word
# name: (B, h, w, t, N, P, K)
WORD_CASES = {
    "13x21-t8-P2-K4": (2, 13, 21, 8, 128, 2, 4),      # ragged both ways, escapes everywhere
    "13x21-t8-P1": (1, 13, 21, 8, 192, 1, 32),        # the defaults
    "13x21-t16-P1": (1, 13, 21, 16, 128, 1, 32),      # 1×2 tiles, 13×16 and 13×5
    "3x2-t8-P2": (2, 3, 2, 8, 128, 2, 32),            # smaller than one tile: 6 symbols per channel
    "9x9-t8-P1": (1, 9, 9, 8, 128, 1, 32),            # tiles of 8×8, 8×1, 1×8 and 1×1 positions
}


def word_case(name, device, net):
    B, h, w, t, N, P, K = WORD_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    y = np.rint(rng.laplace(0.0, 3.0, size=(B, h, w, N))).astype(np.float32)
    y[rng.random(y.shape) < 0.01] = 40.0             # beyond ±K at K = 32 as well
    y[0, 0, 0, :4] = [-32767.0, 32767.0, -(K + 1), K + 1]
    y[:, :, :, 5] = 0.0                              # a channel all zero in every tile
    y[0, -min(h, 5):, -min(w, 5):, 7] = 0.0          # and one all zero inside the corner tile only
    assert (np.abs(y) > K).any()
    cum = net.bitEstimator.entropy_tables(K)
    return y, torch.from_numpy(y).to(device), cum, cum.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("name", list(WORD_CASES))
def test_tile_words_equal_the_oracle_and_decode_returns_the_latent(device, nets, name):
    B, h, w, t, N, P, K = WORD_CASES[name]
    y, yd, cum, cum_np = word_case(name, device, nets(N))
    th, tw = kernels.tile_grid(h, w, t)
    cpg = N // P
    words_d, off_d = kernels.rans_encode_tiled(yd, cum, t, K, P)
    words, off = words_d.cpu().numpy().view(np.uint16), off_d.cpu().numpy()
    assert off.shape == (B * th * tw * P + 1,) and off[0] == 0 and off[-1] == words.size
    s = 0
    for b in range(B):
        for r in range(th):
            for c in range(tw):
                tile = y[b, r * t:(r + 1) * t, c * t:(c + 1) * t]      # ragged at the edges
                for g in range(P):
                    chans = np.arange(g * cpg, (g + 1) * cpg)
                    values = tile[:, :, chans].transpose(2, 0, 1).reshape(-1)   # (channel, row, column)
                    rows = np.repeat(chans, tile.shape[0] * tile.shape[1])
                    want = rans_ref.encode_stream(values.astype(np.int64).tolist(), rows.tolist(), cum_np, K)
                    assert words[off[s]:off[s + 1]].tolist() == want, (b, r, c, g)
                    s += 1
    # every workgroup shape writes the same words and decodes them to the latent, bit for bit
    for waves in kernels.TILE_WAVES:
        wv, ov = kernels.rans_encode_tiled(yd, cum, t, K, P, waves=waves)
        assert torch.equal(wv, words_d) and torch.equal(ov, off_d), waves
        back = kernels.rans_decode_tiled(words_d, off_d, cum, B, h, w, N, t, K, P, waves=waves)
        assert torch.equal(back, yd), waves
    # a rectangle of tiles alone, from its own streams, into the compact window it covers
    for rect in {(0, 0, 1, 1), (th - 1, tw - 1, th, tw), (0, tw - 1, th, tw), (th - 1, 0, th, tw)}:
        r0, c0, r1, c1 = rect
        picked = [((b * th + r) * tw + c) * P + g for b in range(B) for r in range(r0, r1)
                  for c in range(c0, c1) for g in range(P)]
        parts = [words[off[k]:off[k + 1]] for k in picked]
        sub_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        sub = torch.from_numpy(np.concatenate(parts).view(np.int16).copy()).to(device)
        win = kernels.rans_decode_tiled(sub, torch.from_numpy(sub_off).to(device), cum, B, h, w, N,
                                        t, K, P, rect=rect)
        assert torch.equal(win, yd[:, r0 * t:r1 * t, c0 * t:c1 * t].contiguous()), rect


def test_tiled_coder_rejections(device, nets):
    B, h, w, t, N, P, K = WORD_CASES["13x21-t8-P2-K4"]
    y, yd, cum, _ = word_case("13x21-t8-P2-K4", device, nets(N))
    words, off = kernels.rans_encode_tiled(yd, cum, t, K, P)
    with pytest.raises(kernels.Iclr17Error, match="a latent is not integer-valued"):
        kernels.rans_encode_tiled(yd + 0.25, cum, t, K, P)
    with pytest.raises(kernels.Iclr17Error, match="tile edge 4"):
        kernels.rans_encode_tiled(yd, cum, 4, K, P)
    with pytest.raises(kernels.Iclr17Error, match="not divisible into 3 streams"):
        kernels.rans_encode_tiled(yd, cum, t, K, 3)
    with pytest.raises(kernels.Iclr17Error, match="3 waves per workgroup"):
        kernels.rans_encode_tiled(yd, cum, t, K, P, waves=3)
    with pytest.raises(kernels.Iclr17Error, match="the tables must be an int32 GPU tensor"):
        kernels.rans_encode_tiled(yd, cum[:, :-1], t, K, P)
    for rect in ((0, 0, 3, 3), (1, 1, 1, 2), (-1, 0, 1, 1), (0, 0, 2, 4)):
        with pytest.raises(kernels.Iclr17Error, match="is not inside the 2x3 tiles"):
            kernels.rans_decode_tiled(words, off, cum, B, h, w, N, t, K, P, rect=rect)
    with pytest.raises(kernels.Iclr17Error, match="offsets do not match the 24 streams"):
        kernels.rans_decode_tiled(words, off[:-1], cum, B, h, w, N, t, K, P)
    with pytest.raises(kernels.Iclr17Error, match="offsets do not match the 4 streams"):
        kernels.rans_decode_tiled(words, off, cum, B, h, w, N, t, K, P, rect=(0, 0, 1, 1))


def test_decode_tiled_reports_corrupt_words(device, nets):
    """Data only: the pointers, the lengths and the geometry stay those of the good stream."""
    B, h, w, t, N, P, K = WORD_CASES["13x21-t8-P1"]
    y, yd, cum, _ = word_case("13x21-t8-P1", device, nets(N))
    words, off = kernels.rans_encode_tiled(yd, cum, t, K, P)
    o = off.cpu().numpy()
    for at in (int(o[3]) + 1, int(o[5]) + 200, int(o[-1]) - 1):   # a final state, two payload words
        bad = words.clone()
        bad[at] ^= 0x1234
        with pytest.raises(kernels.Iclr17Error, match=CORRUPT):
            kernels.rans_decode_tiled(bad, off, cum, B, h, w, N, t, K, P)
    # a last stream one word short, as test_decode_map_reports_corrupt_words has it
    short = off.clone()
    short[-1] -= 1
    with pytest.raises(kernels.Iclr17Error, match=CORRUPT):
        kernels.rans_decode_tiled(words, short, cum, B, h, w, N, t, K, P)


# ------------------------------------------------------------------ 2. the same picture
@pytest.mark.parametrize("precision", ["x6", "h3"])
def test_tiled_blob_is_the_untiled_picture(device, nets, images, precision):
    net = nets(128)
    fp = codec.fingerprint(net)
    with kernels.precision_scope(precision):
        for s, t, P in ((5, 8, 1), (13, 8, 2), (8, 16, 1)):
            stepped = net.compress_images(images, step=s, streams_per_image=P)
            tiled = net.compress_images(images, step=s, streams_per_image=P, tile=t)
            decoded = net.decompress_images(stepped)
            for q, b, im in zip(stepped, tiled, images):
                head, info = codec.parse_blob(b, N=128, fingerprint=fp)
                assert q[:4] == b"I17Q" and b[:4] == b"I17T"
                assert head == codec.parse_blob(q)[0] and (info.step, info.tile) == (s, t)
                assert info.counts.shape == codec.tile_shape(*im.shape[:2], t) + (P,)
                assert len(b) == info.words + 2 * int(info.counts.sum())
                assert torch.equal(latents_of(net, b), latents_of(net, q))
            for a, want in zip(net.decompress_images(tiled), decoded):
                assert np.array_equal(a, want)
        # tile alone: index 8 and compress's own ŷ, the plain blob's latents
        plain = net.compress_images(images)
        alone = net.compress_images(images, tile=8)
        assert alone == net.compress_images(images, step=codec.UNIT_STEP, tile=8)
        for c, b in zip(plain, alone):
            head, info = codec.parse_blob(b)
            assert c[:4] == b"I17C" and (info.step, info.tile) == (8, 8)
            Hc, Wc = codec.canvas(head.H, head.W)
            ref = net.decompress([c[codec.HEADER.size:]], (Hc // 16, Wc // 16))["y_hat"]
            assert torch.equal(latents_of(net, b), ref)
        # one tile holds the whole latent: the untiled blob's words behind another header
        one = net.compress_images(images[3:], step=5, tile=8)[0]
        assert one[28:] == net.compress_images(images[3:], step=5)[0][28:]
        rows = net.evaluate_images(images[:2], step=13, tile=8)
        assert [(r["step"], r["tile"]) for r in rows] == [(13, 8)] * 2
        assert [r["bytes"] for r in rows] == [len(b) for b in net.compress_images(images[:2], step=13, tile=8)]


@pytest.mark.parametrize("N", [128, 192])
def test_tiled_rdo_levels_are_the_untiled_ones(device, nets, images, N):
    net = nets(N)
    for kw in ({"rdo": 0.02}, {"rdo": 0.05, "step": 11}):
        plain = net.compress_images(images, **kw)
        tiled = net.compress_images(images, tile=8, **kw)
        for q, b in zip(plain, tiled):
            assert q[:4] == b"I17Q" and b[:4] == b"I17T"
            assert torch.equal(latents_of(net, b), latents_of(net, q))
        moved = any(not torch.equal(latents_of(net, q), latents_of(net, u))
                    for q, u in zip(plain, net.compress_images(images, step=kw.get("step", 8))))
        assert moved   # the optimisation did choose other levels: the equality above says something
    y = net.latents(torch.cat([torch.from_numpy(images[2]).permute(2, 0, 1).float().div(255)[None]]).to(device))
    a = net.compress_latents(y, 9, rdo=0.03, tile=8)
    b = net.compress_latents(y, 9, rdo=0.03)
    assert torch.equal(a["y_hat"], b["y_hat"]) and torch.equal(a["est_bits"], b["est_bits"])


# ------------------------------------------------------------------ 3. region equals crop
def region_boxes(H, W):
    return {"inside one tile": (20, 30, 90, 100),
            "four-tile corner": (100, 110, 150, 140),
            "right edge": (W - 37, 50, W, 90),
            "bottom edge": (140, H - 21, 200, H),
            "bottom right": (W - 5, H - 5, W, H),
            "1x1": (131, 127, 132, 128),
            "1x1 origin": (0, 0, 1, 1),
            "whole": (0, 0, W, H)}


@pytest.mark.parametrize("precision", ["x6", "h3", "fp32"])
def test_region_decode_equals_the_crop(device, nets, images, precision):
    net = nets(128)
    with kernels.precision_scope(precision):
        for im, kw in ((images[0], {"step": 6, "tile": 8}), (images[1], {"tile": 8, "streams_per_image": 2}),
                       (images[1], {"step": 12, "tile": 16}), (images[3], {"step": 4, "tile": 8})):
            H, W = im.shape[:2]
            blob = net.compress_images([im], **kw)[0]
            full = net.decompress_images([blob])[0]
            t, P = kw["tile"], kw.get("streams_per_image", 1)
            th, tw = codec.tile_shape(H, W, t)
            boxes = region_boxes(H, W) if H > 100 else {"whole": (0, 0, W, H), "1x1": (W - 1, H - 1, W, H),
                                                        "inner": (3, 5, 20, 33)}
            for name, box in boxes.items():
                x0, y0, x1, y1 = box
                stats = {}
                got = net.decompress_region(blob, box, stats=stats)
                assert got.dtype == np.uint8 and got.shape == (y1 - y0, x1 - x0, 3)
                assert np.array_equal(got, full[y0:y1, x0:x1]), (precision, kw, name)
                r0, c0, r1, c1 = codec.region_window(H, W, t, box).tiles
                assert stats == {"streams_decoded": (r1 - r0) * (c1 - c0) * P,
                                 "streams_total": th * tw * P}, name
                if name == "inside one tile" and t == 8:
                    assert stats["streams_decoded"] == P < stats["streams_total"] == 6 * P
        # a blob that is not tiled is decoded whole: the call always works
        for blob in (net.compress_images(images[:1])[0], net.compress_images(images[:1], step=11)[0],
                     net.compress_images(images[:1], step_offsets=[None])[0]):
            stats = {}
            got = net.decompress_region(blob, (100, 110, 150, 140), stats=stats)
            assert np.array_equal(got, net.decompress_images([blob])[0][110:140, 100:150])
            assert stats == {"streams_decoded": 1, "streams_total": 1}


@pytest.mark.parametrize("precision", ["x6", "h3"])
def test_region_decode_at_192_channels(device, nets, images, precision):
    net = nets(192)
    with kernels.precision_scope(precision):
        blob = net.compress_images(images[:1], step=7, tile=8)[0]
        full = net.decompress_images([blob])[0]
        for box in region_boxes(200, 328).values():
            x0, y0, x1, y1 = box
            assert np.array_equal(net.decompress_region(blob, box), full[y0:y1, x0:x1]), box


# ------------------------------------------------------------------ 4. batches, kinds, budgets
def test_batch_independence_and_mixed_kinds(device, nets, images):
    net = nets(128)
    blobs = net.compress_images(images, step=10, tile=8)
    for i, im in enumerate(images):
        assert net.compress_images([im], step=10, tile=8) == [blobs[i]]
    assert net.compress_images(images, step=10, tile=8, max_batch=2) == blobs
    decoded = net.decompress_images(blobs)
    mixed = [blobs[0], net.compress_images(images[1:2])[0], blobs[3],
             net.compress_images(images[2:3], step=13)[0], blobs[1],
             net.compress_images(images[:1], step=9, step_offsets=[None], block=2)[0],
             net.compress_images(images[2:3], step=10, tile=16)[0],
             net.compress_images(images[2:3], step=11, tile=8)[0], blobs[2]]
    assert {b[:4] for b in mixed} == {b"I17C", b"I17Q", b"I17M", b"I17T"}
    alone = [net.decompress_images([b])[0] for b in mixed]
    for batchsize in (64, 2):
        for a, b in zip(net.decompress_images(mixed, max_batch=batchsize), alone):
            assert np.array_equal(a, b)
    for k, i in ((0, 0), (2, 3), (4, 1), (8, 2)):
        assert np.array_equal(alone[k], decoded[i])
    # the tile edge changes the layout alone
    assert np.array_equal(alone[6], decoded[2])


@pytest.mark.parametrize("N", [128, 192])
def test_budget_counts_the_tile_overhead(device, nets, images, N):
    net = nets(N)
    img = images[0]
    H, W = img.shape[:2]
    overhead = codec.tiled_blob_overhead(1, H, W, 8)
    assert overhead == 28 + 6 * 260
    L = len(net.compress_images([img], tile=8)[0])
    picked = []
    for budget in (5 * L // 4, 3 * L // 4, overhead + (L - overhead) // 3):
        stats = {}
        blob = net.compress_images([img], max_bytes=budget, tile=8, stats=stats)[0]
        info = codec.parse_blob(blob)[1]
        untiled = codec.parse_blob(net.compress_images([img], max_bytes=budget)[0])[1]
        print(f"N={N} L={L} budget {budget}: step {info.step} (untiled {untiled}), {len(blob)} bytes, "
              f"re-encodes {stats['reencodes']}")
        assert blob[:4] == b"I17T" and len(blob) <= budget
        assert info.step >= untiled   # 5 more streams to pay for: never a finer step
        assert blob == net.compress_images([img], step=info.step, tile=8)[0]
        if info.step:   # the next finer step does not fit, or the estimate said so
            finer = net.compress_images([img], step=info.step - 1, tile=8)[0]
            est = net.rate_sweep(net.latents(kernels.image_ingest(
                *codec.upload_packed([img], device), codec.canvas(H, W))), latent=True)[0]
            assert len(finer) > budget or int(np.ceil(float(est[info.step - 1]) / 8)) + overhead > budget
        picked.append(info.step)
    assert picked[0] < picked[1] < picked[2]
    # a budget below the overhead itself cannot be met at any step
    with pytest.raises(kernels.Iclr17Error, match="does not fit its budget of 1500 bytes"):
        net.compress_images([img], max_bytes=1500, tile=8)
    group = images[:3]
    budgets = [3 * L // 4, L, 2 * L // 3]
    blobs = net.compress_images(group, max_bytes=budgets, tile=8)
    assert all(len(b) <= m for b, m in zip(blobs, budgets))
    for im, m, b in zip(group, budgets, blobs):
        assert net.compress_images([im], max_bytes=m, tile=8) == [b]
    assert net.compress_images(group[:1], bpp=2.0, tile=8) == \
        net.compress_images(group[:1], max_bytes=200 * 328 * 2 // 8, tile=8)


# ------------------------------------------------------------------ 5. corrupt blobs, command line
def test_corrupt_payload_words_raise(device, nets, images):
    net = nets(128)
    blob = net.compress_images(images[:1], step=9, tile=8)[0]
    info = codec.parse_blob(blob)[1]
    first = info.words + 2 * np.concatenate([[0], np.cumsum(info.counts.reshape(-1))])
    # data bytes only: a final state of the first stream, the last word of the tile at (1, 2)
    for at, box in ((int(first[0]) + 3, (20, 30, 90, 100)), (int(first[6]) - 1, (290, 160, 300, 170))):
        bad = blob[:at] + bytes([blob[at] ^ 0x5A]) + blob[at + 1:]
        assert codec.parse_blob(bad)[1].counts.tolist() == info.counts.tolist()
        with pytest.raises(kernels.Iclr17Error, match=CORRUPT):
            net.decompress_images([bad])
        with pytest.raises(kernels.Iclr17Error, match=CORRUPT):
            net.decompress_region(bad, box)
    # a region that does not touch the corrupt tile still decodes, to the good blob's pixels
    good = net.decompress_images([blob])[0]
    assert np.array_equal(net.decompress_region(bad, (20, 30, 90, 100)), good[30:100, 20:90])


def test_command_line_tile_and_region(device, nets, images, tmp_path):
    from PIL import Image
    net, img = nets(128), images[0]
    src, out, back = tmp_path / "in.png", tmp_path / "out.i17c", tmp_path / "back.png"
    ckpt = tmp_path / "iter_0.pth.tar"
    Image.fromarray(img).save(src)
    torch.save(net.state_dict(), ckpt)
    common = ["--weights", str(ckpt), "--N", "128"]
    for flags, kw in ((["--tile", "8"], {"tile": 8}), (["--tile", "16", "--step", "12"], {"tile": 16, "step": 12}),
                      (["--tile", "8", "--bpp", "1.5", "--rdo", "0.02"], {"tile": 8, "bpp": 1.5, "rdo": 0.02})):
        assert codec.main(["encode", str(src), str(out), *common, *flags]) == 0
        blob = net.compress_images([img], **kw)[0]
        assert out.read_bytes() == blob and blob[:4] == b"I17T"
        full = net.decompress_images([blob])[0]
        assert codec.main(["decode", str(out), str(back), *common]) == 0
        with Image.open(back) as im:
            assert np.array_equal(np.asarray(im), full)
        assert codec.main(["decode", str(out), str(back), *common, "--region", "100,110,150,140"]) == 0
        with Image.open(back) as im:
            assert np.array_equal(np.asarray(im), full[110:140, 100:150])
    with pytest.raises(kernels.Iclr17Error, match="--region takes X0,Y0,X1,Y1"):
        codec.main(["decode", str(out), str(back), *common, "--region", "1,2,3"])
    with pytest.raises(kernels.Iclr17Error, match="tiled step maps are not built"):
        codec.main(["encode", str(src), str(out), *common, "--tile", "8", "--roi", "0,0,50,50,-2"])
