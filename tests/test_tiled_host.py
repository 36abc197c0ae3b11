"""Tiled rANS streams, the host side, without a GPU: the I17T container next to
the untouched I17C, I17Q and I17M ones, the overhead a budget counts, rate_request with ``tile``,
every corrupt-blob rejection (all before any device use: the model here lives on the CPU),
region_window against a brute-force dependency probe of a CPU synthesis with the three layers'
geometry, and the host-side argument checks of the new entry points."""
import ctypes
import re
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iclr_17_compression_amd import _lib, codec, kernels
from iclr_17_compression_amd.model import ImageCompressor

P16 = ctypes.c_void_p(16)   # a non-null pointer that no check dereferences
FP = 0x0123456789ABCDEF


def tiled_blob(P=2, N=192, K=32, step=13, tile=8, H=200, W=328, fp=FP, counts=None):
    """A well-formed I17T blob with made-up words: 200×328 → canvas 208×336, latent 13×21, 2×3
    tiles at t = 8."""
    th, tw = codec.tile_shape(H, W, tile)
    if counts is None:
        counts = 128 + np.arange(th * tw * P)
    counts = np.asarray(counts, dtype="<u4")
    words = (np.arange(int(counts.sum())) % 65536).astype("<u2")
    return codec.pack_tile_header(P, N, K, step, tile, H, W, fp) + counts.tobytes() + words.tobytes()


# ------------------------------------------------------------------------------ container
def test_tile_header_bytes_and_round_trip():
    assert codec.TILE_HEADER.size == 28 == codec.HEADER.size
    assert codec.tile_shape(200, 328, 8) == (2, 3)
    head = codec.pack_tile_header(P=2, N=192, K=32, step=13, tile=8, H=200, W=328, fingerprint=FP)
    assert head == struct.pack("<4sBBHHBBIIQ", b"I17T", 1, 2, 192, 32, 13, 3, 200, 328, FP)
    for t, lg, shape in ((8, 3, (2, 3)), (16, 4, (1, 2)), (32, 5, (1, 1)), (64, 6, (1, 1))):
        b = codec.pack_tile_header(1, 128, 4, 0, t, 200, 328, FP)
        assert b[11] == lg and codec.tile_shape(200, 328, t) == shape
    blob = tiled_blob()
    h, info = codec.parse_tile_header(blob, N=192, fingerprint=FP)
    assert h == codec.Header(P=2, N=192, K=32, H=200, W=328, fingerprint=FP)
    assert (info.step, info.tile, info.words) == (13, 8, 28 + 4 * 12)
    assert info.counts.shape == (2, 3, 2) and info.counts.dtype == np.int64
    assert info.counts.reshape(-1).tolist() == list(range(128, 140))   # (tile row, tile column, group)
    h2, info2 = codec.parse_blob(blob, N=192, fingerprint=FP)
    assert h2 == h and info2[:2] == (13, 8) and np.array_equal(info2.counts, info.counts)
    # a latent smaller than one tile: one stream per group
    small = tiled_blob(P=1, H=40, W=24, counts=[130])
    assert codec.parse_blob(small)[1].counts.shape == (1, 1, 1)
    for kw, text in (({"step": 32}, "quantiser step index"), ({"tile": 4}, "tile edge 4"),
                     ({"tile": 128}, "tile edge 128"), ({"tile": True}, "tile edge True"),
                     ({"P": 0}, "header field out of range")):
        args = dict(P=1, N=192, K=32, step=8, tile=8, H=200, W=328, fingerprint=FP)
        args.update(kw)
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            codec.pack_tile_header(**args)


def test_other_headers_are_unchanged():
    assert codec.pack_header(4, 192, 32, 333, 500, FP) == \
        struct.pack("<4sBBHHxxIIQ", b"I17C", 1, 4, 192, 32, 333, 500, FP)
    assert codec.pack_step_header(4, 192, 32, 13, 333, 500, FP) == \
        struct.pack("<4sBBHHBxIIQ", b"I17Q", 1, 4, 192, 32, 13, 333, 500, FP)
    m = (np.arange(48).reshape(6, 8) % 32).astype(np.uint8)
    assert codec.pack_map_header(4, 192, 32, 13, 4, 333, 500, FP, m) == \
        struct.pack("<4sBBHHBBIIQ", b"I17M", 1, 4, 192, 32, 13, 2, 333, 500, FP) + m.tobytes()
    plain = codec.pack_header(1, 192, 32, 49, 83, FP) + b"\0" * 8
    assert codec.parse_blob(plain) == (codec.Header(1, 192, 32, 49, 83, FP), None)
    stepped = codec.pack_step_header(1, 192, 32, 5, 49, 83, FP) + b"\0" * 8
    assert codec.parse_blob(stepped) == (codec.Header(1, 192, 32, 49, 83, FP), 5)
    assert codec.blob_overhead(1) == 28 + 260 and codec.blob_overhead(4) == 28 + 4 * 260


def test_tiled_overhead():
    # header + per stream a count and 64 final states
    assert codec.tiled_blob_overhead(1, 200, 328, 8) == 28 + 2 * 3 * 260
    assert codec.tiled_blob_overhead(2, 200, 328, 8) == 28 + 2 * 3 * 2 * 260
    assert codec.tiled_blob_overhead(1, 200, 328, 16) == 28 + 1 * 2 * 260
    assert codec.tiled_blob_overhead(1, 2048, 2048, 16) == 28 + 64 * 260
    assert codec.tiled_blob_overhead(4, 4096, 3072, 64) == 28 + 4 * 3 * 4 * 260
    # one tile: the untiled blob's
    assert codec.tiled_blob_overhead(3, 40, 24, 8) == codec.blob_overhead(3)
    with pytest.raises(_lib.Iclr17Error, match="tile edge 12"):
        codec.tiled_blob_overhead(1, 200, 328, 12)


def test_rate_request_with_tile():
    assert codec.rate_request(2, tile=8) is None                       # the layout, not the rate
    assert codec.rate_request(2, step=5, tile=16) == ("step", 5)
    assert codec.rate_request(2, max_bytes=900, tile=32) == ("budget", [900, 900], False)
    assert codec.rate_request(2, bpp=[1.0, 2.0], tile=64) == ("budget", [1.0, 2.0], True)
    assert codec.rate_request(1, rdo=0.5, tile=8) == ("step", codec.UNIT_STEP)
    for t in (4, 0, 12, 128, True, 8.0, "8"):
        with pytest.raises(_lib.Iclr17Error, match="tile must be one of"):
            codec.rate_request(1, tile=t)
    for kw in ({}, {"step": 5}, {"max_bytes": 900}):
        with pytest.raises(_lib.Iclr17Error, match="tiled step maps are not built"):
            codec.rate_request(1, step_offsets=[None], tile=8, **kw)
    with pytest.raises(_lib.Iclr17Error, match="step and bpp given together"):
        codec.rate_request(1, step=3, bpp=1.0, tile=8)
    # the surface refuses it before any device use as well
    net = ImageCompressor(128).eval()
    img = np.zeros((40, 24, 3), np.uint8)
    with pytest.raises(_lib.Iclr17Error, match="tiled step maps are not built"):
        net.compress_images([img], tile=8, step_offsets=[None])
    with pytest.raises(_lib.Iclr17Error, match="tile must be one of"):
        net.compress_images([img], tile=12)
    with pytest.raises(_lib.Iclr17Error, match="tiled step maps are not built"):
        net.compress_latents(torch.zeros(1, 3, 2, 128), None, step_map=np.zeros((1, 1, 1), int), tile=8)


def test_corrupt_tiled_blobs_are_rejected_on_the_host():
    net = ImageCompressor(128).eval()          # on the CPU: whatever reached the device would raise
    fp = codec.fingerprint(net)                # "ROCm GPU", not the texts below
    good = tiled_blob(N=128, fp=fp)
    table_end = 28 + 4 * 12

    def field(offset, raw):
        return good[:offset] + raw + good[offset + len(raw):]

    cases = ((field(11, b"\x02"), "tiles of 2^2 latent positions"),
             (field(11, b"\x07"), "tiles of 2^7 latent positions"),
             (field(11, b"\xff"), "tiles of 2^255 latent positions"),
             (field(10, b"\x20"), "quantiser step 32 in the stream"),
             (good[:table_end - 1], "truncated tile count table (47 of 48 bytes)"),
             (good[:28], "truncated tile count table (0 of 48 bytes)"),
             (good[:27], "truncated header"),
             (good[:-2], "the tile counts sum to 1602 words, the stream holds 1601"),
             (good + b"\0\0", "the tile counts sum to 1602 words, the stream holds 1603"),
             (field(28, struct.pack("<I", 127)), "the tile counts sum to 1601 words"),
             (good[:-1], "truncated stream"),
             (good + b"\0", "truncated stream"),
             (field(20, struct.pack("<Q", fp ^ 1)), "fingerprint mismatch"),
             (field(6, struct.pack("<H", 192)), "the stream is for N=192, the model has N=128"),
             (field(4, b"\x02"), "unknown version 2"),
             # a finer tile in the header asks for a longer table than a coarser blob holds
             (tiled_blob(N=128, fp=fp, tile=16)[:11] + b"\x03" + tiled_blob(N=128, fp=fp, tile=16)[12:],
              "the tile counts sum to"))
    for blob, text in cases:
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            codec.parse_blob(blob, N=128, fingerprint=fp)
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            net.decompress_images([good[:0] + blob])
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            net.decompress_region(blob, (0, 0, 8, 8))
    # a well-formed blob passes the host checks and only then asks for the device
    with pytest.raises(_lib.Iclr17Error, match="ROCm GPU|GPU tensor"):
        net.decompress_images([good])
    for box, ok in (((0, 0, 328, 200), True), ((327, 199, 328, 200), True), ((0, 0, 329, 200), False),
                    ((0, 0, 328, 201), False), ((-1, 0, 5, 5), False), ((5, 5, 5, 9), False),
                    ((0, 0, 8), False), ((0.0, 0, 8, 8), False), (None, False)):
        with pytest.raises(_lib.Iclr17Error, match="ROCm GPU|GPU tensor" if ok else "a region is"):
            net.decompress_region(good, box)


# ------------------------------------------------------------------------------ region_window
class Synthesis:
    """The synthesis transform's geometry on the CPU in float64, random weights, a small N:
    deconv 5×5/s2/p2/op1, pointwise nonlinearity, the same again, deconv 9×9/s4/p4/op3. The
    nonlinearity mixes channels and not positions, as IGDN does."""

    def __init__(self, N=3, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.w1 = torch.randn(N, N, 5, 5, generator=g, dtype=torch.float64)
        self.w2 = torch.randn(N, N, 5, 5, generator=g, dtype=torch.float64)
        self.w3 = torch.randn(N, 3, 9, 9, generator=g, dtype=torch.float64)
        self.gamma = torch.rand(N, N, 1, 1, generator=g, dtype=torch.float64)

    def igdn(self, x):
        return x * torch.sqrt(1.0 + F.conv2d(x * x, self.gamma))

    def __call__(self, y):
        x = self.igdn(F.conv_transpose2d(y, self.w1, stride=2, padding=2, output_padding=1))
        x = self.igdn(F.conv_transpose2d(x, self.w2, stride=2, padding=2, output_padding=1))
        return F.conv_transpose2d(x, self.w3, stride=4, padding=4, output_padding=3)


def region_boxes(H, W):
    """Boxes with every residue of x0, x1, y0 and y1 mod 16, the image corners, 1×1 boxes and the
    whole image."""
    boxes = []
    for r in range(16):
        x0, x1 = 32 + r, 64 + (5 * r + 3) % 16 + (16 if r > 8 else 0)
        y0, y1 = 16 + (7 * r + 1) % 16, 48 + r
        boxes.append((x0, y0, min(x1, W), min(y1, H)))
    assert {b[0] % 16 for b in boxes} == {b[2] % 16 for b in boxes} == set(range(16))
    assert {b[1] % 16 for b in boxes} == {b[3] % 16 for b in boxes} == set(range(16))
    boxes += [(0, 0, 9, 7), (W - 9, 0, W, 7), (0, H - 7, 9, H), (W - 9, H - 7, W, H),
              (0, 0, 1, 1), (W - 1, H - 1, W, H), (37, 29, 38, 30), (48, 32, 49, 33),
              (47, 31, 48, 32), (0, 0, W, H), (16, 16, 32, 32)]
    return boxes


def test_region_window_against_brute_force():
    H, W, t = 72, 120, 8                 # canvas 80×128: latent 5×8
    h, w = 5, 8
    syn = Synthesis()
    g = torch.Generator().manual_seed(1)
    y = torch.randn(1, 3, h, w, generator=g, dtype=torch.float64)
    base = syn(y)
    assert tuple(base.shape) == (1, 3, 16 * h, 16 * w)
    for box in region_boxes(H, W):
        x0, y0, x1, y1 = box
        win = codec.region_window(H, W, t, box)
        i0, j0, i1, j1 = win.latent
        assert 0 <= i0 < i1 <= h and 0 <= j0 < j1 <= w
        # the issue's bound: at most one position up and left of the box's own, two down and right
        assert i0 >= y0 // 16 - 1 and j0 >= x0 // 16 - 1
        assert i1 - 1 <= (y1 - 1) // 16 + 2 and j1 - 1 <= (x1 - 1) // 16 + 2
        # sufficient: every position outside the rectangle perturbed at once, no pixel moves
        outside = torch.ones(h, w, dtype=torch.bool)
        outside[i0:i1, j0:j1] = False
        noise = torch.randn(1, 3, h, w, generator=g, dtype=torch.float64)
        moved = syn(y + noise * outside)
        assert torch.equal(moved[..., y0:y1, x0:x1], base[..., y0:y1, x0:x1]), box
        if outside.any():
            assert not torch.equal(moved, base)
        # tight: each edge row and column of the rectangle reaches some pixel of the box
        for name, edge in (("top", (slice(i0, i0 + 1), slice(j0, j1))),
                           ("bottom", (slice(i1 - 1, i1), slice(j0, j1))),
                           ("left", (slice(i0, i1), slice(j0, j0 + 1))),
                           ("right", (slice(i0, i1), slice(j1 - 1, j1)))):
            only = torch.zeros(h, w, dtype=torch.bool)
            only[edge] = True
            moved = syn(y + noise * only)
            assert not torch.equal(moved[..., y0:y1, x0:x1], base[..., y0:y1, x0:x1]), (box, name)
        # the tiles cover the rectangle and no tile is idle; the offset places the box
        r0, c0, r1, c1 = win.tiles
        assert (r0, c0, r1, c1) == (i0 // t, j0 // t, (i1 - 1) // t + 1, (j1 - 1) // t + 1)
        assert win.offset == (x0 - 16 * t * c0, y0 - 16 * t * r0)


def test_region_window_values_and_rejections():
    # 200×328: canvas 208×336, latent 13×21, 2×3 tiles at t = 8
    assert codec.region_window(200, 328, 8, (0, 0, 16, 16)) == ((0, 0, 3, 3), (0, 0, 1, 1), (0, 0))
    assert codec.region_window(200, 328, 8, (16, 16, 32, 32)) == ((0, 0, 4, 4), (0, 0, 1, 1), (16, 16))
    # a box straddling the four-tile corner at pixel (128, 128)
    assert codec.region_window(200, 328, 8, (120, 120, 136, 136)) == \
        ((6, 6, 11, 11), (0, 0, 2, 2), (120, 120))
    # inside tile (1, 2): latent rows 8.., columns 16..
    assert codec.region_window(200, 328, 8, (290, 160, 300, 170)) == \
        ((9, 17, 13, 21), (1, 2, 2, 3), (290 - 256, 160 - 128))
    assert codec.region_window(200, 328, 8, (0, 0, 328, 200)) == ((0, 0, 13, 21), (0, 0, 2, 3), (0, 0))
    assert codec.region_window(200, 328, 16, (0, 0, 328, 200)).tiles == (0, 0, 1, 2)
    assert codec.region_window(40, 24, 8, (23, 39, 24, 40)) == ((1, 0, 3, 2), (0, 0, 1, 1), (23, 39))
    for box in ((0, 0, 329, 200), (0, 0, 0, 10), (10, 10, 5, 20), (-1, 0, 5, 5), (0, 0, 5), "box",
                (0, 0, 5.0, 5), (0, 0, True, 5)):
        with pytest.raises(_lib.Iclr17Error, match="a region is"):
            codec.region_window(200, 328, 8, box)
    with pytest.raises(_lib.Iclr17Error, match="tile edge 4"):
        codec.region_window(200, 328, 4, (0, 0, 8, 8))


# ------------------------------------------------------------------------------ entry points
def test_tiled_entry_points_reject_bad_arguments_on_the_host():
    q = _lib.query
    assert q("iclr17_rans_tiled_capacity", 192, 1, 3) == 128 + 2 * 192 * 64
    assert q("iclr17_rans_tiled_capacity", 192, 2, 6) == 128 + 2 * 96 * 4096
    assert q("iclr17_rans_tiled_capacity", 192, 5, 3) == 0 == q("iclr17_rans_tiled_capacity", 192, 1, 2)
    assert q("iclr17_rans_tiled_capacity", 192, 1, 7) == 0
    assert q("iclr17_rans_tiled_streams", 13, 21, 2, 3) == 12
    assert q("iclr17_rans_tiled_streams", 128, 128, 1, 4) == 64
    assert q("iclr17_rans_tiled_streams", 13, 21, 1, 2) == 0 == q("iclr17_rans_tiled_streams", 0, 21, 1, 3)

    def enc(B=1, h=13, w=21, N=192, P=1, lg=3, K=32, waves=0, words=10 ** 9, p=P16):
        return [p, B, h, w, N, P, lg, p, K, waves, p, words, p, p, None]

    def dec(B=1, h=13, w=21, N=192, P=1, lg=3, rect=(0, 0, 2, 3), K=32, waves=0, elems=10 ** 9,
            total=10 ** 6, p=P16):
        return [p, total, p, B, h, w, N, P, lg, *rect, p, K, waves, p, elems, p, None]

    for name, args, cases in (
            ("iclr17_rans_encode_tiled", enc, (
                ({"lg": 2}, "log2 of the tile edge is not 3..6"), ({"lg": 7}, "log2 of the tile edge"),
                ({"B": 0}, "bad shape"), ({"h": 0}, "bad shape"), ({"P": 5}, "bad shape"),
                ({"p": None}, "bad arguments"), ({"K": 0}, "bad arguments"),
                ({"K": 100}, "tables of 155904 bytes exceed LDS"),
                ({"waves": 3}, "3 waves per workgroup"), ({"waves": 32}, "32 waves per workgroup"),
                ({"words": 6 * 24704 - 1}, "scratch of 148223 words < 148224"))),
            ("iclr17_rans_decode_tiled", dec, (
                ({"lg": 2}, "log2 of the tile edge is not 3..6"), ({"B": 0}, "bad shape"),
                ({"P": 5}, "bad shape"), ({"p": None}, "bad arguments"), ({"total": -1}, "bad arguments"),
                ({"rect": (0, 0, 3, 3)}, "the tile rectangle is not inside the tile grid"),
                ({"rect": (1, 0, 2, 3)}, "the tile rectangle is not inside the tile grid"),
                ({"rect": (0, 3, 1, 1)}, "the tile rectangle is not inside the tile grid"),
                ({"rect": (0, -1, 1, 1)}, "the tile rectangle is not inside the tile grid"),
                ({"rect": (0, 0, 0, 1)}, "the tile rectangle is not inside the tile grid"),
                ({"waves": 5}, "5 waves per workgroup"),
                ({"K": 100}, "tables of 155904 bytes exceed LDS"),
                # the window of tiles (1, 2): 5 × 5 positions
                ({"rect": (1, 2, 1, 1), "elems": 25 * 192 - 1}, "output of 4799 elements < 4800"),
                ({"elems": 13 * 21 * 192 - 1}, "output of 52415 elements < 52416")))):
        for kw, text in cases:
            with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
                _lib.call(name, *args(**kw))
            assert text in _lib.last_error()
    # the Python layer checks before it allocates or launches: CPU tensors never get that far
    cum = torch.zeros(192, 67, dtype=torch.int32)
    with pytest.raises(_lib.Iclr17Error, match="ROCm GPU"):
        kernels.rans_encode_tiled(torch.zeros(1, 13, 21, 192), cum, 8)
    with pytest.raises(_lib.Iclr17Error, match="tile edge 12"):
        kernels.tile_grid(13, 21, 12)
    with pytest.raises(_lib.Iclr17Error, match="the tables must be an int32 GPU tensor"):
        kernels.rans_decode_tiled(torch.zeros(4, dtype=torch.int16), torch.zeros(7, dtype=torch.int64),
                                  cum, 1, 13, 21, 192, 8)
    assert kernels.tile_grid(13, 21, 8) == (2, 3) and kernels.tile_grid(128, 128, 64) == (2, 2)
