"""Centroid reconstruction, the host side, without a GPU: recon_value, the surface
raising before any device use, the RECON_WITH texts, the command line and the host-side argument
checks of the three entry points of csrc/recon.hip."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

from iclr_17_compression_amd import _lib, codec, kernels
from iclr_17_compression_amd._lib import Iclr17Error
from iclr_17_compression_amd.model import ImageCompressor

P16 = ctypes.c_void_p(16)   # a non-null pointer that no check dereferences


def test_recon_value():
    assert codec.RECON_MODES == (None, "centre", "centroid", "zero")
    assert codec.recon_value(None) is None and codec.recon_value("centre", 0.25) is None
    assert codec.recon_value("centroid") == ("centroid", 1.0)
    assert codec.recon_value("zero", 0) == ("zero", 0.0)
    assert codec.recon_value("zero", np.float32(0.5)) == ("zero", 0.5)
    assert codec.recon_value("centroid", np.int64(1)) == ("centroid", 1.0)
    for bad in ("center", "CENTROID", "", 0, 1, True, b"zero", ("zero",)):
        with pytest.raises(Iclr17Error, match="recon must be one of"):
            codec.recon_value(bad)
    for bad in (True, False, "1", None, [1.0], 1j):
        with pytest.raises(Iclr17Error, match="recon_strength must be a real number"):
            codec.recon_value("centroid", bad)
    for bad in (-0.001, 1.001, float("nan"), float("inf"), -float("inf"), 2):
        for mode in ("centroid", None):     # checked whatever the mode
            with pytest.raises(Iclr17Error, match=r"recon_strength must be finite and in \[0, 1\]"):
                codec.recon_value(mode, bad)


def test_not_built_texts():
    assert set(codec.RECON_WITH) == {"psnr", "msssim", "refine"}
    for k, text in codec.RECON_WITH.items():
        assert text.startswith(f"iclr17: codec: recon with {k}: ") and "is not built" in text


def test_surface_raises_before_any_device_use():
    net = ImageCompressor(out_channel_N=128).eval()     # a CPU model: a device use would raise
    im = np.zeros((20, 20, 3), np.uint8)
    blob = codec.pack_step_header(1, 128, 32, 12, 20, 20, codec.fingerprint(net)) + b"\0" * 8
    for call in (lambda **kw: net.decompress([b"\0" * 8], (2, 2), step=12, **kw),
                 lambda **kw: net.decompress_images([blob], **kw),
                 lambda **kw: net.decompress_region(blob, (0, 0, 4, 4), **kw),
                 lambda **kw: net.evaluate_images([im], step=12, **kw)):
        with pytest.raises(Iclr17Error, match="recon must be one of"):
            call(recon="mean")
        with pytest.raises(Iclr17Error, match="recon_strength must be finite"):
            call(recon="zero", recon_strength=1.5)
        with pytest.raises(Iclr17Error, match="recon_strength must be a real number"):
            call(recon="centroid", recon_strength=True)
    for kw, name in (({"psnr": 30.0}, "psnr"), ({"msssim": 0.9}, "msssim"),
                     ({"step": 12, "refine": 3, "refine_lambda": 650.25}, "refine")):
        for mode in ("centroid", "zero"):
            with pytest.raises(Iclr17Error) as e:
                net.evaluate_images([im], recon=mode, **kw)
            assert str(e.value) == codec.RECON_WITH[name]
    # "centre", None and refine=0 are the call without them: these get as far as the device
    for kw in ({"recon": "centre", "psnr": 30.0}, {"recon": "zero", "step": 12, "refine": 0}):
        with pytest.raises(RuntimeError, match="GPU") as e:   # torch's, or the package's own
            net.evaluate_images([im], **kw)
        assert "recon" not in str(e.value)


def test_signatures():
    for fn in (ImageCompressor.decompress, ImageCompressor.decompress_images,
               ImageCompressor.decompress_region, codec.decode_groups, codec.decode_region):
        ps = inspect.signature(fn).parameters
        assert list(ps)[-2:] == ["recon", "recon_strength"], fn
        assert ps["recon"].default is None and ps["recon_strength"].default == 1.0
    # evaluate_images' last four names are pinned: the two stand right before them,
    # and every name up to ``estimate`` keeps its position
    for fn in (ImageCompressor.evaluate_images, codec.evaluate_images):
        ps = inspect.signature(fn).parameters
        assert list(ps)[-7:] == ["estimate", "recon", "recon_strength", "msssim", "refine",
                                 "refine_lambda", "refine_lr"], fn
        assert ps["recon"].default is None and ps["recon_strength"].default == 1.0
    assert "recon" not in inspect.signature(codec.compress_images).parameters


def test_command_line():
    ap = codec.build_parser()
    a = ap.parse_args(["decode", "in.i17c", "out.png", "--weights", "w"])
    assert (a.recon, a.recon_strength) == (None, 1.0)
    a = ap.parse_args(["decode", "in.i17c", "out.png", "--weights", "w", "--recon", "zero",
                       "--recon-strength", "0.5", "--region", "0,0,8,8"])
    assert (a.recon, a.recon_strength, a.region) == ("zero", 0.5, "0,0,8,8")
    a = ap.parse_args(["eval", "a.png", "--weights", "w", "--steps", "10,12", "--recon", "centroid"])
    assert (a.recon, a.recon_strength, a.steps) == ("centroid", 1.0, "10,12")
    assert ap.parse_args(["eval", "a.png", "--weights", "w", "--recon", "centre"]).recon == "centre"
    with pytest.raises(SystemExit):
        ap.parse_args(["decode", "in.i17c", "out.png", "--weights", "w", "--recon", "mean"])
    with pytest.raises(SystemExit):     # the encoder has no such option
        ap.parse_args(["encode", "in.png", "out.i17c", "--weights", "w", "--recon", "zero"])
    # main raises on the host, before it looks for a device
    with pytest.raises(Iclr17Error, match="recon_strength must be finite"):
        codec.main(["decode", "in.i17c", "out.png", "--weights", "w", "--recon", "zero",
                    "--recon-strength", "2"])
    with pytest.raises(Iclr17Error) as e:
        codec.main(["eval", "a.png", "--weights", "w", "--recon", "zero", "--psnr", "30"])
    assert str(e.value) == codec.RECON_WITH["psnr"]


# ------------------------------------------------------------------------------ wrappers
def test_wrapper_checks_precede_any_device_use():
    y = torch.zeros(2, 4, 6, 128)   # host tensors: never uploaded
    rp = torch.zeros(11 * 128)
    off = torch.zeros(128, 65)
    with pytest.raises(Iclr17Error, match="ROCm GPU"):
        kernels.recon_offsets(rp, 128, 32, [1.0], "centroid")
    with pytest.raises(Iclr17Error, match="ROCm GPU"):
        kernels.dequantise_recon(y, 1.0, off)
    with pytest.raises(Iclr17Error, match="ROCm GPU"):
        kernels.dequantise_recon_map(y, np.zeros((2, 1, 2), np.uint8), 4, [1.0], off[None])
    assert kernels.RECON_MODES == {"centroid": 0, "zero": 1}


# ------------------------------------------------------------------------------ entry points
def rejects(text, name, *args):
    with pytest.raises(Iclr17Error, match=re.escape(text)):
        _lib.call(name, *args)
    assert text in _lib.last_error()


def floats(*v):
    return ctypes.cast((ctypes.c_float * len(v))(*v), ctypes.c_void_p)


def test_entry_points_validate_without_gpu():
    # every check below fires on the host before a kernel could be launched
    def offsets(rp=P16, N=128, K=32, st=(1.0, 2.0), S=2, mode=0, a=1.0, off=P16):
        return ["iclr17_recon_offsets", rp, N, K, None if st is None else floats(*st), S, mode,
                ctypes.c_float(a), off, None]

    for p in ("rp", "off", "st"):
        rejects("recon_offsets: null pointer", *offsets(**{p: None}))
    rejects("recon_offsets: bad shape N=0", *offsets(N=0))
    rejects("recon_offsets: K=0 (1..1024)", *offsets(K=0))
    rejects("recon_offsets: K=1025 (1..1024)", *offsets(K=1025))
    rejects("recon_offsets: S=0 steps (1..32)", *offsets(S=0))
    rejects("recon_offsets: S=33 steps (1..32)", *offsets(S=33))
    rejects("recon_offsets: mode 2", *offsets(mode=2))
    rejects("recon_offsets: mode -1", *offsets(mode=-1))
    for bad in (-0.5, 1.5, float("nan"), float("inf")):
        rejects("recon_offsets: strength ", *offsets(a=bad))
        assert "is not in [0, 1]" in _lib.last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rejects("recon_offsets: step 1 (", *offsets(st=(1.0, bad)))
        assert "is not finite and positive" in _lib.last_error()

    def one(y=P16, B=2, h=4, w=6, N=128, d=1.0, off=P16, K=32, out=P16):
        return ["iclr17_dequantise_recon", y, B, h, w, N, ctypes.c_float(d), off, K, out, None]

    def mapped(y=P16, B=2, h=4, w=6, N=128, slots=P16, lg=2, st=(1.0, 2.0), off=P16, S=2, K=32,
               out=P16):
        return ["iclr17_dequantise_recon_map", y, B, h, w, N, slots, lg,
                None if st is None else floats(*st), off, S, K, out, None]

    for what, entry, ptrs in (("dequantise_recon", one, ("y", "off", "out")),
                              ("dequantise_recon_map", mapped, ("y", "slots", "st", "off", "out"))):
        for p in ptrs:
            rejects(f"{what}: null pointer", *entry(**{p: None}))
        rejects(f"{what}: bad shape B=0 h=4 w=6 N=128", *entry(B=0))
        rejects(f"{what}: bad shape B=2 h=-1 w=6 N=128", *entry(h=-1))
        rejects(f"{what}: bad shape B=2 h=4 w=0 N=128", *entry(w=0))
        rejects(f"{what}: bad shape B=2 h=4 w=6 N=0", *entry(N=0))
        rejects(f"{what}: K=0 (1..1024)", *entry(K=0))
        rejects(f"{what}: K=1025 (1..1024)", *entry(K=1025))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rejects("dequantise_recon: the step ", *one(d=bad))
        assert "is not finite and positive" in _lib.last_error()
        rejects("dequantise_recon_map: step 0 (", *mapped(st=(bad, 1.0)))
    rejects("dequantise_recon_map: log2 of the block edge is 5 (0..4)", *mapped(lg=5))
    rejects("dequantise_recon_map: log2 of the block edge is -1 (0..4)", *mapped(lg=-1))
    rejects("dequantise_recon_map: S=0 steps (1..32)", *mapped(S=0))
    rejects("dequantise_recon_map: S=33 steps (1..32)", *mapped(S=33))
