"""Rate control's host side, without a GPU: the quantiser-step ladder, the I17Q container header
next to the untouched I17C one, the budget rule's pure choice, the host-side validation of the
entry points of csrc/ratectl.hip, and the argument errors of compress_images."""
import ctypes
import re
import struct

import numpy as np
import pytest
import torch

from iclr_17_compression_amd import _lib, codec, kernels
from iclr_17_compression_amd.model import ImageCompressor

P16 = ctypes.c_void_p(16)   # a non-null pointer that no check dereferences
FP = 0x0123456789ABCDEF


# ------------------------------------------------------------------------------ ladder
def test_ladder():
    assert codec.STEPS == 32 and codec.UNIT_STEP == 8
    sizes = [codec.step_size(s) for s in range(32)]
    assert sizes[8] == 1.0 and sizes[0] == 0.25
    assert 53.8 < sizes[31] < 53.9
    for s in range(28):
        assert sizes[s + 4] == 2.0 * sizes[s]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    for d in sizes:
        assert float(np.float32(d)) == d
    # the four mantissas are the fp32 values nearest to 2^(k/4)
    for k in range(4):
        assert sizes[8 + k] == float(np.float32(2.0 ** (k / 4)))
    assert codec.step_size(np.int64(5)) == sizes[5]
    for bad in (-1, 32, 100, 8.0, "8", None, True):
        with pytest.raises(_lib.Iclr17Error, match="quantiser step index"):
            codec.step_size(bad)


# ------------------------------------------------------------------------------ container
def test_step_header_round_trip():
    blob = codec.pack_step_header(P=4, N=192, K=32, step=13, H=333, W=500, fingerprint=FP)
    assert len(blob) == 28 == codec.STEP_HEADER.size == codec.HEADER.size
    assert blob == struct.pack("<4sBBHHBxIIQ", b"I17Q", 1, 4, 192, 32, 13, 333, 500, FP)
    head, step = codec.parse_step_header(blob + b"payload", N=192, fingerprint=FP)
    assert head == codec.Header(P=4, N=192, K=32, H=333, W=500, fingerprint=FP) and step == 13
    assert codec.parse_step_header(blob) == (head, 13)   # without a model to compare against
    # but for the magic and the step byte, the plain header of the same fields
    plain = codec.pack_header(4, 192, 32, 333, 500, FP)
    assert blob[4:10] == plain[4:10] and blob[11:] == plain[11:] and plain[10:12] == b"\0\0"
    assert blob[10] == 13
    unit = codec.pack_step_header(1, 128, 32, codec.UNIT_STEP, 49, 83, FP)
    assert unit[:4] == b"I17Q" and unit[10] == 8


def test_step_header_rejections():
    good = codec.pack_step_header(1, 192, 32, 5, 49, 83, FP)

    def field(offset, raw):
        return good[:offset] + raw + good[offset + len(raw):]

    for blob, text in ((field(0, b"PNG\x00"), "bad magic"),
                       (field(0, b"I17C"), "bad magic"),
                       (field(4, b"\x02"), "unknown version 2"),
                       (field(4, b"\x00"), "unknown version 0"),
                       (field(10, b"\x20"), "quantiser step 32 in the stream"),
                       (field(10, b"\xff"), "quantiser step 255 in the stream"),
                       (good[:27], "truncated header"),
                       (b"", "truncated header"),
                       (field(12, struct.pack("<I", 0)), "must be at least 1x1"),
                       (field(16, struct.pack("<I", 0)), "must be at least 1x1")):
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            codec.parse_step_header(blob, N=192, fingerprint=FP)
    with pytest.raises(_lib.Iclr17Error, match=re.escape("the stream is for N=192, the model has N=128")):
        codec.parse_step_header(good, N=128, fingerprint=FP)
    with pytest.raises(_lib.Iclr17Error, match="fingerprint mismatch"):
        codec.parse_step_header(good, N=192, fingerprint=FP ^ 1)
    for step in (-1, 32):
        with pytest.raises(_lib.Iclr17Error, match="quantiser step index"):
            codec.pack_step_header(1, 192, 32, step, 49, 83, FP)
    for H, W in ((0, 8), (8, 0)):
        with pytest.raises(_lib.Iclr17Error, match=re.escape("must be at least 1x1")):
            codec.pack_step_header(1, 192, 32, 5, H, W, FP)


def test_parse_blob_dispatches_and_parse_header_is_unchanged():
    plain = codec.pack_header(2, 128, 32, 49, 83, FP)
    stepped = codec.pack_step_header(2, 128, 32, 31, 49, 83, FP)
    head = codec.Header(P=2, N=128, K=32, H=49, W=83, fingerprint=FP)
    assert codec.parse_blob(plain + b"xx", N=128, fingerprint=FP) == (head, None)
    assert codec.parse_blob(stepped + b"xx", N=128, fingerprint=FP) == (head, 31)
    assert codec.parse_blob(stepped) == (head, 31)
    assert codec.parse_header(plain) == head
    with pytest.raises(_lib.Iclr17Error, match=re.escape("bad magic b'I17Q' (not an I17C stream)")):
        codec.parse_header(stepped)
    with pytest.raises(_lib.Iclr17Error, match="bad magic"):
        codec.parse_blob(b"PNG\x00" + plain[4:])
    with pytest.raises(_lib.Iclr17Error, match="truncated header"):
        codec.parse_blob(stepped[:20])
    with pytest.raises(_lib.Iclr17Error, match="truncated header"):
        codec.parse_blob(b"I1")
    with pytest.raises(_lib.Iclr17Error, match="quantiser step 32 in the stream"):
        codec.parse_blob(stepped[:10] + b"\x20" + stepped[11:])
    with pytest.raises(_lib.Iclr17Error, match="unknown version 2"):   # version 2 stays foreign
        codec.parse_blob(plain[:4] + b"\x02" + plain[5:])


# ------------------------------------------------------------------------------ budget rule
def test_choose_step():
    overhead = codec.blob_overhead(1)
    assert overhead == 28 + 4 + 256 and codec.blob_overhead(4) == 28 + 16 + 1024
    row = [8.0 * (3200 - 100 * s) for s in range(32)]   # 3200, 3100, … 100 bytes of words
    assert codec.choose_step(row, 10 ** 6, overhead) == 0
    assert codec.choose_step(row, 2000 + overhead, overhead) == 12
    assert codec.choose_step(row, 2000 + overhead - 1, overhead) == 13
    assert codec.choose_step(row, 100 + overhead, overhead) == 31
    # bits round up to whole bytes
    assert codec.choose_step([8.0 * 10 + 1, 8.0 * 10], 10 + overhead, overhead) == 1
    assert codec.choose_step([8.0 * 10 - 7, 8.0 * 10], 10 + overhead, overhead) == 0
    # ties: the finer index
    assert codec.choose_step([900.0, 800.0, 800.0, 800.0], 100 + overhead, overhead) == 1
    # nothing fits
    with pytest.raises(_lib.Iclr17Error, match=re.escape(f"no quantiser step fits {99 + overhead} bytes")):
        codec.choose_step(row, 99 + overhead, overhead)
    with pytest.raises(_lib.Iclr17Error, match="no quantiser step fits 100 bytes"):
        codec.choose_step(row, 100, overhead)
    # a non-monotone row is scanned 0 → 31: the first index that fits, not the best later one
    bumpy = [8.0 * b for b in (500, 90, 300, 80, 10)]
    assert codec.choose_step(bumpy, 100 + overhead, overhead) == 1
    assert codec.choose_step(bumpy, 85 + overhead, overhead) == 3
    assert codec.choose_step(np.asarray(bumpy), 300 + overhead, overhead) == 1


def test_encode_to_budget_moves_coarser_until_the_blob_fits():
    # blob length of image k at index s; the coder stands in for the GPU
    size = {0: lambda s: 1000 - 10 * s, 1: lambda s: 2000 - 50 * s, 2: lambda s: 900 - 10 * s}
    calls = []

    def encode(members, s):
        calls.append((tuple(members), s))
        return [bytes(size[k](s)) for k in members]

    labels = ["image 7 (5x5)", "image 8 (5x5)", "image 9 (5x5)"]
    # image 0 fits at once; image 1 (first pick 3, an estimate that was too low) needs index 6;
    # image 2 has no budget
    blobs, again = codec.encode_to_budget([3, 3, 5], [970, 1700, None], encode, labels)
    assert [len(b) for b in blobs] == [970, 1700, 850] and again == [0, 3, 0]
    # grouped by index, members ascending; only the image that did not fit is coded again
    assert calls == [((0, 1), 3), ((2,), 5), ((1,), 4), ((1,), 5), ((1,), 6)]
    calls.clear()
    blobs, again = codec.encode_to_budget([30, 0], [699, 10 ** 6], encode, labels)
    assert [len(b) for b in blobs] == [690, 2000] and again == [1, 0]
    with pytest.raises(_lib.Iclr17Error, match=re.escape(
            "image 7 (5x5) does not fit its budget of 689 bytes: the coarsest step gives 690")):
        codec.encode_to_budget([30, 0], [689, 10 ** 6], encode, labels)
    assert codec.encode_to_budget([], [], encode, []) == ([], [])


# ------------------------------------------------------------------------------ entry points
def rejects(text, name, *args):
    with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
        _lib.call(name, *args)
    assert text in _lib.last_error()


def test_entry_points_validate_without_gpu():
    # every check below fires on the host before a kernel could be launched
    F = ctypes.c_float
    one = (ctypes.c_float * 1)(1.0)

    def steps(*v):
        return ctypes.cast((ctypes.c_float * len(v))(*v), ctypes.c_void_p)

    def sweep(y=P16, B=2, h=4, w=6, N=128, rp=P16, st=None, S=1, partial=P16, bits=P16):
        st = ctypes.cast(one, ctypes.c_void_p) if st is None else st
        return ["iclr17_rate_sweep", y, B, h, w, N, rp, st, S, partial, bits, None]

    for kw in ({"y": None}, {"rp": None}, {"partial": None}, {"bits": None}):
        rejects("rate_sweep: null pointer", *sweep(**kw))
    with pytest.raises(_lib.Iclr17Error, match="rate_sweep: null pointer"):
        _lib.call("iclr17_rate_sweep", P16, 2, 4, 6, 128, P16, None, 1, P16, P16, None)
    rejects("rate_sweep: bad shape B=0 h=4 w=6 N=128", *sweep(B=0))
    rejects("rate_sweep: bad shape B=2 h=-1 w=6 N=128", *sweep(h=-1))
    rejects("rate_sweep: bad shape B=2 h=4 w=0 N=128", *sweep(w=0))
    rejects("rate_sweep: bad shape B=2 h=4 w=6 N=0", *sweep(N=0))
    rejects("rate_sweep: S=0 steps (1..32)", *sweep(S=0))
    rejects("rate_sweep: S=33 steps (1..32)", *sweep(S=33, st=steps(*[1.0] * 33)))
    rejects("rate_sweep: S=-1 steps (1..32)", *sweep(S=-1))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rejects("rate_sweep: step 1 (", *sweep(S=3, st=steps(0.5, bad, 2.0)))
        assert "is not finite and positive" in _lib.last_error()
    rejects("rate_sweep: N=4096 needs", *sweep(N=4096))
    assert _lib.query("iclr17_rate_sweep_partials", 16, 16, 192) == 12
    assert _lib.query("iclr17_rate_sweep_partials", 1, 1, 128) == 1
    assert _lib.query("iclr17_rate_sweep_partials", 4, 6, 192) == 2
    assert _lib.query("iclr17_rate_sweep_partials", 0, 6, 192) == 0
    # the sweep's chunks are rate_bits' own
    assert (_lib.query("iclr17_rate_sweep_partials", 16, 16, 192)
            == _lib.query("iclr17_rate_bits_partials", 192, 16, 16))

    def quant(y=P16, n=100, d=1.0, y_hat=P16, y_deq=P16, status=P16):
        return ["iclr17_quantise_step", y, n, F(d), y_hat, y_deq, status, None]

    def dequant(y_hat=P16, n=100, d=1.0, y_deq=P16):
        return ["iclr17_dequantise_step", y_hat, n, F(d), y_deq, None]

    def pack(rp=P16, N=128, d=1.0, out=P16):
        return ["iclr17_pack_rate_step", rp, N, F(d), out, None]

    for what, entry, ptrs, size in (("quantise_step", quant, ("y", "y_hat", "y_deq", "status"), "n"),
                                    ("dequantise_step", dequant, ("y_hat", "y_deq"), "n"),
                                    ("pack_rate_step", pack, ("rp", "out"), "N")):
        for p in ptrs:
            rejects(f"{what}: null pointer", *entry(**{p: None}))
        rejects(f"{what}: bad shape {size}=0", *entry(**{size: 0}))
        rejects(f"{what}: bad shape {size}=-5", *entry(**{size: -5}))
        for bad in (0.0, -0.25, float("nan"), float("inf")):
            rejects(f"{what}: the step ", *entry(d=bad))
            assert "is not finite and positive" in _lib.last_error()


def test_wrapper_checks_precede_any_device_use():
    y = torch.zeros(1, 2, 2, 128)   # host tensors: never uploaded
    rp = torch.zeros(11 * 128)
    for fn in (lambda: kernels.quantise_step(y, 1.0), lambda: kernels.dequantise_step(y, 1.0),
               lambda: kernels.pack_rate_step(rp, 128, 1.0), lambda: kernels.rate_sweep(y, rp, [1.0])):
        with pytest.raises(_lib.Iclr17Error, match="ROCm GPU"):
            fn()


# ------------------------------------------------------------------------------ compress_images
def test_compress_images_argument_errors():
    net = ImageCompressor(128).eval()   # on the host: nothing below may reach a kernel
    img = np.zeros((5, 7, 3), np.uint8)
    for kw, text in (({"step": 8, "max_bytes": 1000}, "step and max_bytes given together"),
                     ({"step": 8, "bpp": 1.0}, "step and bpp given together"),
                     ({"max_bytes": 1000, "bpp": 1.0}, "max_bytes and bpp given together"),
                     ({"step": 8, "max_bytes": 1000, "bpp": 1.0}, "given together"),
                     ({"step": 32}, "quantiser step index"),
                     ({"step": -1}, "quantiser step index"),
                     ({"max_bytes": [1000, 2000, 3000]}, "max_bytes has 3 values for 2 images"),
                     ({"bpp": [1.0]}, "bpp has 1 values for 2 images"),
                     ({"max_bytes": 0}, "max_bytes must be finite and positive"),
                     ({"bpp": float("nan")}, "bpp must be finite and positive")):
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            net.compress_images([img, img], **kw)
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            net.evaluate_images([img, img], **kw)
    assert codec.rate_request(2) is None
    assert codec.rate_request(2, step=np.int64(4)) == ("step", 4)
    assert codec.rate_request(2, max_bytes=500) == ("budget", [500, 500], False)
    assert codec.rate_request(2, bpp=[0.5, 1.0]) == ("budget", [0.5, 1.0], True)
