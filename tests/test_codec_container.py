"""The image-file codec's host side (iclr_17_compression_amd/codec.py): the 28-byte container
header and its rejections, the weights fingerprint, canvases and batching, and the host-side
validation of the two image entry points and their wrappers — all without a GPU. The contract
is the codec module's own (the reference has neither padding nor a bitstream)."""
import ctypes
import re
import struct

import pytest
import torch

from iclr_17_compression_amd import _lib, codec, kernels
from iclr_17_compression_amd.model import ImageCompressor

P16 = ctypes.c_void_p(16)   # a non-null pointer that no check dereferences
FP = 0x0123456789ABCDEF


def test_header_round_trip():
    blob = codec.pack_header(P=4, N=192, K=32, H=333, W=500, fingerprint=FP)
    assert len(blob) == 28 == codec.HEADER.size
    assert blob == struct.pack("<4sBBHHxxIIQ", b"I17C", 1, 4, 192, 32, 333, 500, FP)
    h = codec.parse_header(blob + b"payload", N=192, fingerprint=FP)
    assert h == codec.Header(P=4, N=192, K=32, H=333, W=500, fingerprint=FP)
    assert codec.parse_header(blob) == h   # without a model to compare against


def test_header_rejections():
    good = codec.pack_header(1, 192, 32, 49, 83, FP)

    def field(offset, raw):
        return good[:offset] + raw + good[offset + len(raw):]

    for blob, text in ((field(0, b"PNG\x00"), "bad magic"),
                       (field(4, b"\x02"), "unknown version 2"),
                       (good[:27], "truncated header"),
                       (b"", "truncated header"),
                       (field(12, struct.pack("<I", 0)), "must be at least 1x1"),
                       (field(16, struct.pack("<I", 0)), "must be at least 1x1")):
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            codec.parse_header(blob, N=192, fingerprint=FP)
    with pytest.raises(_lib.Iclr17Error, match=re.escape("the stream is for N=192, the model has N=128")):
        codec.parse_header(good, N=128, fingerprint=FP)
    with pytest.raises(_lib.Iclr17Error, match="fingerprint mismatch"):
        codec.parse_header(good, N=192, fingerprint=FP ^ 1)
    for H, W in ((0, 8), (8, 0)):
        with pytest.raises(_lib.Iclr17Error, match=re.escape("must be at least 1x1")):
            codec.pack_header(1, 192, 32, H, W, FP)


def test_fingerprint_is_stable_and_follows_the_weights():
    import hashlib
    torch.manual_seed(0)
    net = ImageCompressor(128).eval()
    fp = codec.fingerprint(net)
    assert fp == codec.fingerprint(net) and 0 <= fp < 2 ** 64
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(sd[k].numpy().astype("<f4").tobytes())
    assert fp == int.from_bytes(h.digest()[:8], "little")
    twin = ImageCompressor(128).eval()
    twin.load_state_dict(sd)
    assert codec.fingerprint(twin) == fp
    with torch.no_grad():
        net.Decoder.deconv3.weight[5, 1, 2, 3] += 2.0 ** -10   # one element of one tensor
    changed = codec.fingerprint(net)
    assert changed != fp and codec.fingerprint(net) == changed
    net.load_state_dict(sd)                                    # the original weights back
    assert codec.fingerprint(net) == fp == codec.fingerprint(twin)


def test_canvas():
    assert codec.canvas(1, 1) == (16, 16)
    assert codec.canvas(16, 16) == (16, 16)
    assert codec.canvas(17, 31) == (32, 32)
    assert codec.canvas(512, 768) == (512, 768)
    with pytest.raises(_lib.Iclr17Error, match="at least 1x1"):
        codec.canvas(0, 5)


def test_group_by_canvas():
    shapes = [(49, 83), (60, 64), (64, 96), (50, 90), (1, 1), (64, 64), (16, 16), (49, 83)] * 3
    for max_batch in (1, 2, 5, 64):
        groups = codec.group_by_canvas(shapes, max_batch)
        assert sorted(i for g in groups for i in g) == list(range(len(shapes)))
        for g in groups:
            assert 1 <= len(g) <= max_batch
            assert len({codec.canvas(*shapes[i]) for i in g}) == 1
    kodak = [(512, 768)] * 18 + [(768, 512)] * 6
    kodak = kodak[:7] + kodak[18:] + kodak[7:18]   # portraits in between, as in the real set
    groups = codec.group_by_canvas(kodak, 64)
    assert len(groups) == 2 and sorted(map(len, groups)) == [6, 18]
    assert len(codec.group_by_canvas(kodak, 8)) == 3 + 1
    with pytest.raises(_lib.Iclr17Error, match="max_batch"):
        codec.group_by_canvas(kodak, 0)


def test_image_entry_points_validate_without_gpu():
    # every check below fires on the host before a kernel could be launched
    def ingest(src=P16, desc=P16, B=2, Hc=64, Wc=96, out=P16):
        return ["iclr17_image_ingest_u8", src, desc, B, Hc, Wc, out, None]

    def egress(recon=P16, desc=P16, B=2, Hc=64, Wc=96, dst=P16, ref=None, sse=None, status=P16):
        return ["iclr17_image_egress_u8", recon, desc, B, Hc, Wc, dst, ref, sse, status, None]

    def rejects(text, args):
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            _lib.call(*args)
        assert text in _lib.last_error()

    for what, entry in (("image_ingest", ingest), ("image_egress", egress)):
        rejects("bad shape B=0 H=64 W=96", entry(B=0))
        rejects("bad shape B=-3 H=64 W=96", entry(B=-3))
        rejects("image height/width must be multiples of 16 (got 250x96)", entry(Hc=250))
        rejects("image height/width must be multiples of 16 (got 64x40)", entry(Wc=40))
        rejects("bad shape B=2 H=0 W=96", entry(Hc=0))
        rejects(f"{what}: null pointer", entry(desc=None))
    rejects("image_ingest: null pointer", ingest(src=None))
    rejects("image_ingest: null pointer", ingest(out=None))
    rejects("image_egress: null pointer", egress(recon=None))
    rejects("image_egress: null pointer", egress(dst=None))
    rejects("image_egress: null pointer", egress(status=None))
    rejects("image_egress: sse required with ref", egress(ref=P16))


def test_wrapper_descriptor_checks_precede_any_device_use():
    src = torch.zeros(3 * 49 * 83 + 3 * 64 * 96, dtype=torch.uint8)   # a host tensor: never uploaded
    offsets, shapes = [0, 3 * 49 * 83], [(49, 83), (64, 96)]
    for text, kw in (("image 1 is 65x96, outside the canvas 64x96", {"shapes": [(49, 83), (65, 96)]}),
                     ("image 0 is 49x97, outside the canvas 64x96", {"shapes": [(49, 97), (64, 96)]}),
                     ("image 0 is 0x83, outside the canvas 64x96", {"shapes": [(0, 83), (64, 96)]}),
                     ("image 1 (bytes 12202..30634) lies outside the buffer of 30633 bytes",
                      {"offsets": [0, 3 * 49 * 83 + 1]}),
                     ("image 0 (bytes -1..", {"offsets": [-1, 3 * 49 * 83]}),
                     ("1 offsets for 2 images", {"offsets": [0]}),
                     ("multiples of 16", {"canvas": (64, 90)})):
        args = {"offsets": offsets, "shapes": shapes, "canvas": (64, 96), **kw}
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            kernels.image_ingest(src, args["offsets"], args["shapes"], args["canvas"])
    with pytest.raises(_lib.Iclr17Error, match="1-D uint8"):
        kernels.image_ingest(src.float(), offsets, shapes, (64, 96))
    # sound descriptors: the only thing left to object to is that the bytes are not on a GPU
    with pytest.raises(_lib.Iclr17Error, match="ROCm GPU"):
        kernels.image_ingest(src, offsets, shapes, (64, 96))
