"""Per-block quantiser steps, the host side, without a GPU: the I17M container next
to the untouched I17C and I17Q ones, roi_offsets, the clamp to the ladder, rate_request with
step_offsets, the budget loop over base indices with a stand-in coder, the references of
tests/stepmap_refs.py against the entropy-coder oracle, and the host-side argument checks of the
new entry points."""
import ctypes
import re
import struct

import numpy as np
import pytest
import torch

import stepmap_refs as R
from iclr_17_compression_amd import _lib, codec, kernels
from iclr_17_compression_amd.model import ImageCompressor
from oracle import rans_ref

P16 = ctypes.c_void_p(16)   # a non-null pointer that no check dereferences
FP = 0x0123456789ABCDEF


# ------------------------------------------------------------------------------ container
def test_map_header_round_trip():
    assert codec.map_shape(333, 500, 4) == (6, 8)        # canvas 336×512: latent 21×32
    m = (np.arange(48).reshape(6, 8) % 32).astype(np.uint8)
    blob = codec.pack_map_header(P=4, N=192, K=32, base=13, block=4, H=333, W=500, fingerprint=FP,
                                 indices=m)
    assert codec.MAP_HEADER.size == 28 == codec.HEADER.size == codec.STEP_HEADER.size
    assert blob == struct.pack("<4sBBHHBBIIQ", b"I17M", 1, 4, 192, 32, 13, 2, 333, 500, FP) + m.tobytes()
    head, smap = codec.parse_map_header(blob + b"payload", N=192, fingerprint=FP)
    assert head == codec.Header(P=4, N=192, K=32, H=333, W=500, fingerprint=FP)
    assert (smap.base, smap.block, smap.payload) == (13, 4, 28 + 48)
    assert smap.indices.dtype == np.uint8 and np.array_equal(smap.indices, m)
    head2, smap2 = codec.parse_blob(blob, N=192, fingerprint=FP)
    assert head2 == head and np.array_equal(smap2.indices, m) and smap2[:2] == (13, 4)
    # every block edge, ragged maps, the 1×1 image
    for g, shape in ((1, (21, 32)), (2, (11, 16)), (8, (3, 4)), (16, (2, 2))):
        assert codec.map_shape(333, 500, g) == shape
        z = np.full(shape, 31, np.uint8)
        b = codec.pack_map_header(1, 128, 4, 0, g, 333, 500, FP, z)
        assert b[11] == g.bit_length() - 1 and len(b) == 28 + z.size
        assert codec.parse_map_header(b)[1].block == g
    one = codec.pack_map_header(1, 128, 32, 8, 4, 1, 1, FP, np.zeros((1, 1), np.int64))
    assert one[28:] == b"\0" and codec.parse_map_header(one)[1].indices.shape == (1, 1)


def test_map_header_rejections():
    m = np.full((1, 2), 5, np.uint8)                     # 49×83: canvas 64×96, latent 4×6, g = 4
    good = codec.pack_map_header(1, 192, 32, 5, 4, 49, 83, FP, m) + b"\0" * 8

    def field(offset, raw):
        return good[:offset] + raw + good[offset + len(raw):]

    for blob, text in ((field(0, b"I17Q"), "bad magic"),
                       (field(4, b"\x02"), "unknown version 2"),
                       (field(10, b"\x20"), "quantiser step 32 in the stream"),
                       (field(11, b"\x05"), "step-map block of 2^5"),
                       (field(11, b"\xff"), "step-map block of 2^255"),
                       (field(28, b"\x20"), "quantiser step 32 in the stream's step map"),
                       (field(29, b"\xff"), "quantiser step 255 in the stream's step map"),
                       (good[:29], "truncated step map (1 of 2 bytes)"),
                       (good[:28], "truncated step map (0 of 2 bytes)"),
                       (good[:27], "truncated header"),
                       (field(12, struct.pack("<I", 0)), "must be at least 1x1")):
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            codec.parse_map_header(blob, N=192, fingerprint=FP)
        if not text.startswith("bad magic"):
            with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
                codec.parse_blob(blob, N=192, fingerprint=FP)
    # a finer block edge in the header asks for a longer map than the blob holds
    with pytest.raises(_lib.Iclr17Error, match=re.escape("truncated step map (10 of 24 bytes)")):
        codec.parse_map_header(field(11, b"\x00"))
    with pytest.raises(_lib.Iclr17Error, match="the stream is for N=192, the model has N=128"):
        codec.parse_map_header(good, N=128, fingerprint=FP)
    with pytest.raises(_lib.Iclr17Error, match="fingerprint mismatch"):
        codec.parse_map_header(good, N=192, fingerprint=FP ^ 1)
    for kw, text in (({"base": 32}, "quantiser step index"), ({"block": 3}, "block edge 3"),
                     ({"block": 32}, "block edge 32"),
                     ({"indices": np.full((1, 2), 32)}, "ladder indices 0..31"),
                     ({"indices": np.full((2, 2), 3)}, "ladder indices 0..31"),
                     ({"indices": np.full((1, 2), 3.0)}, "ladder indices 0..31")):
        args = {"P": 1, "N": 192, "K": 32, "base": 5, "block": 4, "H": 49, "W": 83,
                "fingerprint": FP, "indices": m, **kw}
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            codec.pack_map_header(**args)


def test_plain_and_stepped_blobs_parse_as_before():
    plain = codec.pack_header(2, 128, 32, 49, 83, FP)
    stepped = codec.pack_step_header(2, 128, 32, 31, 49, 83, FP)
    assert plain == struct.pack("<4sBBHHxxIIQ", b"I17C", 1, 2, 128, 32, 49, 83, FP)
    assert stepped == struct.pack("<4sBBHHBxIIQ", b"I17Q", 1, 2, 128, 32, 31, 49, 83, FP)
    head = codec.Header(P=2, N=128, K=32, H=49, W=83, fingerprint=FP)
    assert codec.parse_blob(plain + b"xx", N=128, fingerprint=FP) == (head, None)
    assert codec.parse_blob(stepped + b"xx", N=128, fingerprint=FP) == (head, 31)
    mapped = codec.pack_map_header(2, 128, 32, 31, 4, 49, 83, FP, np.zeros((1, 2), np.uint8))
    for parse, blob in ((codec.parse_header, mapped), (codec.parse_step_header, mapped),
                        (codec.parse_map_header, plain), (codec.parse_map_header, stepped)):
        with pytest.raises(_lib.Iclr17Error, match="bad magic"):
            parse(blob)


# ------------------------------------------------------------------------------ offsets
def test_roi_offsets():
    # 100×150: canvas 112×160, latent 7×10; g = 4 → 2×3 blocks of 64×64 pixels, ragged both ways
    assert codec.map_shape(100, 150, 4) == (2, 3)
    z = codec.roi_offsets(100, 150, [], 4)
    assert z.shape == (2, 3) and z.dtype.kind == "i" and not z.any()
    assert np.array_equal(codec.roi_offsets(100, 150, [(0, 0, 1, 1, -4)]), [[-4, 0, 0], [0, 0, 0]])
    # a box's far edge is exclusive: x1 = 64 stays in column 0, 65 reaches column 1
    assert np.array_equal(codec.roi_offsets(100, 150, [(10, 10, 64, 64, -4)]), [[-4, 0, 0], [0, 0, 0]])
    assert np.array_equal(codec.roi_offsets(100, 150, [(10, 10, 65, 65, -4)]), [[-4, -4, 0], [-4, -4, 0]])
    # the ragged last block (pixels 128..159 of the canvas) and a box that leaves the image
    assert np.array_equal(codec.roi_offsets(100, 150, [(140, 70, 10 ** 6, 10 ** 6, 3)]),
                          [[0, 0, 0], [0, 0, 3]])
    assert not codec.roi_offsets(100, 150, [(200, 0, 300, 50, 3), (5, 5, 5, 9, 3), (-9, -9, 0, 0, 3)]).any()
    # overlaps: the most negative offset wins, whatever the order; a positive one beats no box
    boxes = [(0, 0, 150, 100, 6), (60, 0, 70, 10, -2), (0, 0, 10, 10, -5), (0, 0, 10, 10, 2)]
    want = [[-5, -2, 6], [6, 6, 6]]
    assert np.array_equal(codec.roi_offsets(100, 150, boxes), want)
    assert np.array_equal(codec.roi_offsets(100, 150, boxes[::-1]), want)
    # a box with offset 0 over a positive one: 0 is the finer of the two
    assert np.array_equal(codec.roi_offsets(64, 64, [(0, 0, 64, 64, 5), (0, 0, 64, 64, 0)], 1),
                          np.zeros((4, 4)))
    # other block edges
    assert codec.roi_offsets(100, 150, [(0, 0, 17, 16, -1)], 1).nonzero()[0].size == 2
    assert codec.roi_offsets(100, 150, [(0, 0, 1, 1, -1)], 16).shape == (1, 1)
    for bad, text in (([(0, 0, 1, 1)], "a box is"), ([(0, 0, 1, 1, 0.5)], "offset is an integer")):
        with pytest.raises(_lib.Iclr17Error, match=text):
            codec.roi_offsets(100, 150, bad)
    with pytest.raises(_lib.Iclr17Error, match="block edge 5"):
        codec.roi_offsets(100, 150, [], 5)


def test_effective_indices_clamp_at_both_ends():
    off = np.array([[-40, -9, -8, 0, 23, 24, 100]])
    assert codec.effective_indices(8, off).tolist() == [[0, 0, 0, 8, 31, 31, 31]]
    assert codec.effective_indices(0, off).tolist() == [[0, 0, 0, 0, 23, 24, 31]]
    assert codec.effective_indices(31, off).tolist() == [[0, 22, 23, 31, 31, 31, 31]]
    assert codec.effective_indices(8, off).dtype == np.uint8
    assert np.array_equal(R.effective(8, off), codec.effective_indices(8, off))
    with pytest.raises(_lib.Iclr17Error, match="quantiser step index"):
        codec.effective_indices(32, off)
    # offsets are cut to −31..31 on the way in: the clamp gives the same indices
    got = codec.checked_offsets([(49, 83)], [np.array([[-1000, 1000]])], 4)[0]
    assert got.dtype == np.int8 and got.tolist() == [[-31, 31]]
    for base in (0, 8, 31):
        assert np.array_equal(codec.effective_indices(base, got),
                              codec.effective_indices(base, [[-1000, 1000]]))


def test_rate_request_with_step_offsets():
    off = [np.zeros((1, 2), np.int8)] * 2
    assert codec.rate_request(2) is None
    assert codec.rate_request(2, step_offsets=off) == ("step", codec.UNIT_STEP)
    assert codec.rate_request(2, step=3, step_offsets=off) == ("step", 3)
    assert codec.rate_request(2, max_bytes=500, step_offsets=off) == ("budget", [500, 500], False)
    assert codec.rate_request(2, bpp=[0.5, 1.0], step_offsets=off) == ("budget", [0.5, 1.0], True)
    net = ImageCompressor(128).eval()   # on the host: nothing below may reach a kernel
    img = np.zeros((49, 83, 3), np.uint8)
    for kw, text in (({"step": 8, "max_bytes": 1000}, "step and max_bytes given together"),
                     ({"step": 8, "bpp": 1.0}, "step and bpp given together"),
                     ({"max_bytes": 1000, "bpp": 1.0}, "max_bytes and bpp given together"),
                     ({"step": 32}, "quantiser step index"),
                     ({"max_bytes": [1, 2, 3]}, "max_bytes has 3 values for 2 images"),
                     ({"step_offsets": off[:1]}, "step_offsets has 1 entries for 2 images"),
                     ({"step_offsets": [None, np.zeros((2, 2), np.int8)]},
                      "step_offsets[1] must be integers of shape [1, 2] for a 49x83 image with block 4"),
                     ({"step_offsets": [np.zeros((1, 2)), None]}, "step_offsets[0] must be integers"),
                     ({"block": 2}, "step_offsets[0] must be integers of shape [2, 3]"),
                     ({"block": 3}, "block edge 3")):
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            net.compress_images([img, img], **{"step_offsets": off, **kw})
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            net.evaluate_images([img, img], **{"step_offsets": off, **kw})


# ------------------------------------------------------------------------------ budget rule
def test_budget_loop_moves_the_base_and_counts_the_map():
    """compress_images' budget path with a map, the coder a stand-in: choose_step and
    encode_to_budget as they are, the overhead grown by the map's bytes, encode(ks, s) coding at
    BASE s."""
    offs = np.array([[[-4, 0], [0, 2]], [[0, 0], [0, 0]]])             # two images, 2×2 maps
    overhead = codec.blob_overhead(1) + offs[0].size
    assert overhead == 28 + 4 + 256 + 4
    calls = []

    def words(k, s):   # bytes of rANS words of image k at base s: falls with the base
        return (3000, 2000)[k] - 60 * s

    def encode(ks, s):
        calls.append((tuple(ks), s))
        blobs = []
        for k in ks:
            emap = codec.effective_indices(s, offs[k])
            head = codec.pack_map_header(1, 128, 32, s, 4, 100, 100, FP, emap)
            blobs.append(head + bytes(4 + 256 + words(k, s)))
        return blobs

    est = [[8.0 * (words(k, s) - 130) for s in range(32)] for k in range(2)]   # 130 bytes too low
    budgets = [2380, 1500]
    chosen = [codec.choose_step(est[k], budgets[k], overhead) for k in range(2)]
    # the finest base whose estimate fits, the map's 4 bytes counted: estimate + overhead is
    # 3162 − 60·s for image 0, and without the map's bytes (3158 − 60·s) base 13 would have fitted
    assert chosen == [14, 12]
    assert codec.choose_step(est[0], budgets[0], codec.blob_overhead(1)) == 13
    blobs, again = codec.encode_to_budget(chosen, budgets, encode, ["image 0", "image 1"])
    # the blobs are 3292 − 60·s and 2292 − 60·s bytes: two bases coarser each
    assert again == [2, 2] and [len(b) for b in blobs] == [2332, 1452]
    assert calls == [((0,), 14), ((1,), 12), ((0,), 15), ((1,), 13), ((0,), 16), ((1,), 14)]
    for k, blob in enumerate(blobs):
        smap = codec.parse_blob(blob)[1]
        assert smap.base == (16, 14)[k] and len(blob) <= budgets[k]
        assert np.array_equal(smap.indices, np.clip(smap.base + offs[k], 0, 31))
    # at base 31 a blob that still does not fit raises, naming the image
    with pytest.raises(_lib.Iclr17Error, match=re.escape(
            "image 1 does not fit its budget of 400 bytes: the coarsest step gives 432")):
        codec.encode_to_budget([30, 30], [10 ** 6, 400], encode, ["image 0", "image 1"])


# ------------------------------------------------------------------------------ references
def test_refs_rows_round_trip_through_the_oracle():
    """stream_symbols' rows drive the oracle's coder through a 5×7 latent whose g = 1 map holds
    all 32 slots, with escapes (K = 2): decode returns the values."""
    rng = np.random.default_rng(3)
    h, w, N, P, K, S = 5, 7, 4, 2, 2, 32
    y_hat = rng.integers(-6, 7, size=(h, w, N)).astype(np.float32)
    slots = (np.arange(h * w).reshape(h, w) % S).astype(np.uint8)
    assert len(np.unique(slots)) == S
    cum = np.zeros((S * N, 2 * K + 3), np.int64)
    for r in range(S * N):   # any valid tables: positive frequencies summing to 2^16
        f = rng.integers(1, 1000, size=2 * K + 2)
        f[rng.integers(0, 2 * K + 2)] += (1 << 16) - f.sum()
        cum[r, 1:] = np.cumsum(f)
    assert (np.diff(cum, axis=1) > 0).all() and (cum[:, -1] == 1 << 16).all()
    for grp in range(P):
        values, rows = R.stream_symbols(y_hat, slots, 1, N, P, grp)
        assert len(values) == len(rows) == h * w * N // P and max(abs(v) for v in values) > K
        assert rows[0] == slots[0, 0] * N + grp * 2 and rows[1] == slots[0, 1] * N + grp * 2
        words = rans_ref.encode_stream(values, rows, cum, K)
        assert rans_ref.decode_stream(words, rows, cum, K) == values


def test_refs_quantise_and_positions():
    m = np.arange(4).reshape(1, 2, 2)
    pos = R.per_position(m, 5, 7, 4)      # ragged: rows 4.. and columns 4.. are the last blocks
    assert pos.shape == (1, 5, 7)
    assert pos[0, 3].tolist() == [0, 0, 0, 0, 1, 1, 1] and pos[0, 4].tolist() == [2, 2, 2, 2, 3, 3, 3]
    y = torch.tensor([0.5, 1.5, 2.5, -0.75]).view(1, 1, 1, 4)
    y_hat, y_deq = R.quantise(y, np.array([[[8]]]), 4)            # Δ = 1: halves go to even
    assert y_hat.view(-1).tolist() == [0.0, 2.0, 2.0, -1.0] and torch.equal(y_deq, y_hat)
    y_hat, y_deq = R.quantise(y, np.array([[[0]]]), 1)            # Δ = 0.25
    assert y_hat.view(-1).tolist() == [2.0, 6.0, 10.0, -3.0]
    assert y_deq.view(-1).tolist() == [0.5, 1.5, 2.5, -0.75]


# ------------------------------------------------------------------------------ entry points
def rejects(text, name, *args):
    with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
        _lib.call(name, *args)
    assert text in _lib.last_error()


def ladder(*override):
    v = [codec.step_size(s) for s in range(32)]
    for i, x in override:
        v[i] = x
    return ctypes.cast((ctypes.c_float * 32)(*v), ctypes.c_void_p)


NULL = object()   # stands for a NULL ladder where None means "the default"


def pick(st):
    return ladder() if st is None else None if st is NULL else st


def test_entry_points_validate_without_gpu():
    # every check below fires on the host before a kernel could be launched
    def quant(y=P16, B=2, h=4, w=6, N=128, idx=P16, lg=2, st=None, y_hat=P16, y_deq=P16, status=P16):
        return ["iclr17_quantise_step_map", y, B, h, w, N, idx, lg, pick(st), y_hat, y_deq,
                status, None]

    def dequant(y_hat=P16, B=2, h=4, w=6, N=128, idx=P16, lg=2, st=None, y_deq=P16):
        return ["iclr17_dequantise_step_map", y_hat, B, h, w, N, idx, lg, pick(st), y_deq, None]

    def sweep(y=P16, B=2, h=4, w=6, N=128, rp=P16, st=None, off=P16, lg=2, partial=P16, bits=P16):
        return ["iclr17_rate_sweep_offsets", y, B, h, w, N, rp, pick(st), off, lg, partial,
                bits, None]

    for what, entry, ptrs in (("quantise_step_map", quant, ("y", "idx", "y_hat", "y_deq", "status")),
                              ("dequantise_step_map", dequant, ("y_hat", "idx", "y_deq")),
                              ("rate_sweep_offsets", sweep, ("y", "rp", "off", "partial", "bits"))):
        for p in ptrs:
            rejects(f"{what}: null pointer", *entry(**{p: None}))
        rejects(f"{what}: null pointer", *entry(st=NULL))
        rejects(f"{what}: bad shape B=0 h=4 w=6 N=128", *entry(B=0))
        rejects(f"{what}: bad shape B=2 h=-1 w=6 N=128", *entry(h=-1))
        rejects(f"{what}: bad shape B=2 h=4 w=0 N=128", *entry(w=0))
        rejects(f"{what}: bad shape B=2 h=4 w=6 N=0", *entry(N=0))
        rejects(f"{what}: log2 of the block edge is 5 (0..4)", *entry(lg=5))
        rejects(f"{what}: log2 of the block edge is -1 (0..4)", *entry(lg=-1))
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rejects(f"{what}: step 7 (", *entry(st=ladder((7, bad))))
            assert "is not finite and positive" in _lib.last_error()
    rejects("rate_sweep_offsets: N=4096 needs", *sweep(N=4096))

    def enc(y=P16, B=2, h=4, w=6, N=128, P=1, cum=P16, S=3, K=32, slots=P16, lg=2, window=1,
            scratch=P16, words=10 ** 9, lengths=P16, status=P16):
        return ["iclr17_rans_encode_map", y, B, h, w, N, P, cum, S, K, slots, lg, window, scratch,
                words, lengths, status, None]

    def dec(words=P16, offsets=P16, B=2, h=4, w=6, N=128, P=1, cum=P16, S=3, K=32, slots=P16, lg=2,
            window=1, y=P16, status=P16):
        return ["iclr17_rans_decode_map", words, offsets, B, h, w, N, P, cum, S, K, slots, lg,
                window, y, status, None]

    for what, entry, ptrs in (("rans_encode_map", enc, ("y", "cum", "slots", "scratch", "lengths", "status")),
                              ("rans_decode_map", dec, ("words", "offsets", "cum", "slots", "y", "status"))):
        for kw in [{p: None} for p in ptrs] + [{"B": 0}, {"h": 0}, {"w": -2}, {"N": 0}, {"P": 0},
                                               {"P": 3}, {"K": 0}, {"K": 1025}]:
            rejects(f"{what}: bad arguments", *entry(**kw))
        rejects(f"{what}: S=0 table sets (1..32)", *entry(S=0))
        rejects(f"{what}: S=33 table sets (1..32)", *entry(S=33))
        rejects(f"{what}: log2 of the block edge is 5 (0..4)", *entry(lg=5))
        rejects(f"{what}: log2 of the block edge is -1 (0..4)", *entry(lg=-1))
    cap = _lib.query("iclr17_rans_capacity", 4, 6, 128, 1)
    rejects(f"rans_encode_map: scratch of {2 * cap - 1} words < {2 * cap}", *enc(words=2 * cap - 1))


def test_wrapper_checks_precede_any_device_use():
    y = torch.zeros(2, 4, 6, 128)   # host tensors: never uploaded
    rp = torch.zeros(11 * 128)
    steps = [codec.step_size(s) for s in range(32)]
    m = np.zeros((2, 1, 2), np.uint8)
    cum = torch.zeros(1, 128, 67, dtype=torch.int32)
    for fn in (lambda: kernels.quantise_step_map(y, m, 4, steps),
               lambda: kernels.dequantise_step_map(y, m, 4, steps),
               lambda: kernels.rate_sweep_offsets(y, rp, steps, m, 4),
               lambda: kernels.rans_encode_map(y, cum, m, 4)):
        with pytest.raises(_lib.Iclr17Error, match="ROCm GPU"):
            fn()
    with pytest.raises(_lib.Iclr17Error, match="stacked tables must be an int32 GPU tensor"):
        kernels.rans_decode_map(torch.zeros(4, dtype=torch.int16), torch.zeros(3, dtype=torch.int64),
                                cum, m, 4, 2, 4, 6, 128)
    assert kernels.map_shape(5, 7, 4) == (2, 2) and kernels.map_shape(16, 16, 16) == (1, 1)
    for bad in (0, 3, 32, True, None):
        with pytest.raises(_lib.Iclr17Error, match="block edge"):
            kernels.map_shape(5, 7, bad)
