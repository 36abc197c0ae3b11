"""The C-ABI library: loads on a GPU-less host, exports every entry point include/iclr17.h
declares, and its host-side validation rejects bad arguments before any launch."""
import ctypes
import os
import re

import pytest
import torch

from iclr_17_compression_amd import _lib, kernels

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iclr17.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(iclr17_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_exports_every_declared_symbol():
    lib = _lib.load()
    names = declared_functions()
    assert len(names) >= 20
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    # the Python binding declares a signature for every entry point, and nothing else
    assert sorted(_lib.SIGNATURES) == names


def test_version_and_size_queries():
    lib = _lib.load()
    assert lib.iclr17_version() >= 1
    assert _lib.query("iclr17_packed_weight_size", _lib.ICLR17_W_CONV5, 192) == 25 * 192 * 192
    assert _lib.query("iclr17_packed_weight_size", _lib.ICLR17_W_CONV1, 128) == 256 * 128
    assert _lib.query("iclr17_packed_weight_size", _lib.ICLR17_W_DECONV9, 192) == 9 * 192 * 48
    assert _lib.query("iclr17_packed_weight_size", _lib.ICLR17_W_CONV1_X6, 192) == 256 * 192
    assert _lib.query("iclr17_rate_partials_per_image", 256, 256, 192) == 4 * 2   # 96-column tiles
    assert _lib.query("iclr17_rate_partials_per_image", 256, 256, 128) == 4 * 2   # 64-column tiles
    assert _lib.query("iclr17_output_partials_per_image", 256, 256) == 64
    assert _lib.query("iclr17_rate_bits_partials", 192, 16, 16) == 12
    # x6 conv3: noise mode on < 256 tiles·images runs 48-column tiles (4 partials per tile)
    R, Q = _lib.ICLR17_QUANT_ROUND, _lib.ICLR17_QUANT_NOISE
    assert _lib.query("iclr17_conv3_x6_partials_per_image", 32, 256, 256, 192, R) == 4 * 2
    assert _lib.query("iclr17_conv3_x6_partials_per_image", 32, 256, 256, 192, Q) == 4 * 4
    assert _lib.query("iclr17_conv3_x6_partials_per_image", 64, 256, 256, 192, Q) == 4 * 2
    assert _lib.query("iclr17_conv3_x6_partials_per_image", 2, 256, 256, 128, Q) == 4 * 2
    # h3 engine: 8×16 tiles (2 per 256² image) × 64-channel output slices
    assert _lib.query("iclr17_conv3_h3_partials_per_image", 64, 256, 256, 192, R) == 2 * 3
    assert _lib.query("iclr17_conv3_h3_partials_per_image", 32, 256, 256, 192, Q) == 2 * 3
    assert _lib.query("iclr17_conv3_h3_partials_per_image", 1, 2048, 2048, 192, R) == 128 * 3
    assert _lib.query("iclr17_conv3_h3_partials_per_image", 64, 256, 256, 128, R) == 2 * 2
    assert _lib.query("iclr17_conv3_h3_partials_per_image", 2, 256, 512, 128, Q) == 4 * 2
    assert _lib.query("iclr17_conv3_h3_partials_per_image", 2, 40, 256, 128, Q) == 0


def test_argument_validation_without_gpu():
    # every check below fires on the host before a kernel could be launched
    with pytest.raises(_lib.Iclr17Error, match="multiples of 16"):
        _lib.call("iclr17_analysis_conv1_gdn", ctypes.c_void_p(16), 1, 250, 256, 192,
                  *[ctypes.c_void_p(16)] * 5, None, None)
    with pytest.raises(_lib.Iclr17Error, match="unsupported"):
        _lib.call("iclr17_analysis_conv2_gdn", ctypes.c_void_p(16), 1, 256, 256, 96,
                  *[ctypes.c_void_p(16)] * 5, None, None)
    with pytest.raises(_lib.Iclr17Error, match="null pointer"):
        _lib.call("iclr17_synthesis_deconv3", None, 1, 256, 256, 192, *[None] * 6, 0, None)
    with pytest.raises(_lib.Iclr17Error, match="quant mode"):
        _lib.call("iclr17_analysis_conv3_quant_rate", ctypes.c_void_p(16), 1, 256, 256, 192,
                  ctypes.c_void_p(16), 1, None, ctypes.c_void_p(16), None, None,
                  ctypes.c_void_p(16), ctypes.c_void_p(16), None)
    assert "quant mode" in _lib.last_error()
    # every entry point of csrc/engine_fp32.hip and csrc/deconv3_halo.hip, each rejection with the
    # message text it had before those files' host layers were rewritten
    for name, (what, kind, args) in ENGINE_ENTRIES.items():
        def rejects(text, **kw):
            with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
                _lib.call(name, *args(**kw))
            assert text in _lib.last_error(), name
        if kind == "image":
            rejects("image height/width must be multiples of 16 (got 250x256)", H=250)
            rejects("image height/width must be multiples of 16 (got 256x40)", W=40)
            rejects("bad shape B=0 H=256 W=256", B=0)
            rejects("channel count N=96 unsupported (128, 192)", N=96)
        else:
            rejects(f"{what}: bad shape", H=0)
            rejects(f"{what}: bad shape", W=-8)
            rejects(f"{what}: bad shape", B=0)
            rejects("channel count N=96 unsupported", N=96)
        rejects(f"{what}: null pointer", p=None)
        if "quant_rate" in name:
            rejects(f"{what}: bad quant mode 1 / missing noise", q=_lib.ICLR17_QUANT_NOISE)
            rejects(f"{what}: bad quant mode 7 / missing noise", q=7)
        if "synthesis_deconv3" in name:
            rejects(f"{what}: sse_partial required with x", x=P16)
            rejects(f"{what}: the unclipped SSE needs the recon output", unclipped=1)
        if name.endswith("_bits") or name.endswith("_h3"):
            rejects(f"{what}: bits fold needs the partials, their count and a total", fold=P16)
    for name, what in (("iclr17_gdn", "gdn"), ("iclr17_gdn_bwd", "gdn_bwd")):
        def gdn_args(B=1, C=192, H=8, W=8, layout=_lib.ICLR17_LAYOUT_NHWC, p=P16):
            head = [p, p] if what == "gdn_bwd" else [p]
            tail = [p, p, p, p, p, None] if what == "gdn_bwd" else [p, p, p]
            return [*head, B, C, H, W, layout, 0, *tail, None]
        for text, kw in ((f"{what}: bad shape", {"H": 0}), (f"{what}: bad shape", {"B": -1}),
                         (f"{what}: C=96 unsupported (128, 192)", {"C": 96}),
                         (f"{what}: bad layout 5", {"layout": 5}),
                         (f"{what}: null pointer", {"p": None})):
            with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
                _lib.call(name, *gdn_args(**kw))
    with pytest.raises(_lib.Iclr17Error, match="not a positive multiple of 8"):
        _lib.call("iclr17_split_planes", P16, 12, P16, None)
    with pytest.raises(_lib.Iclr17Error, match="split_planes: null pointer"):
        _lib.call("iclr17_split_planes", None, 16, P16, None)
    for bad in ((None, 25, 192, 192, P16), (P16, 0, 192, 192, P16), (P16, 25, 100, 192, P16),
                (P16, 25, 192, 0, P16), (P16, 25, 192, 192, None)):
        with pytest.raises(_lib.Iclr17Error, match="split_packed: bad arguments"):
            _lib.call("iclr17_split_packed", *bad, None)


P16 = ctypes.c_void_p(16)   # a non-null pointer that no check dereferences


def _entry(what, kind, build):
    """An entry point's arguments with every check passing, but for the keyword overrides:
    B, H, W (the image, or the grid h × w), N, p (every required pointer), q and noise (conv3's
    quantiser), x / unclipped / fold (deconv3's optional SSE input, SSE form and bits fold)."""
    def args(B=1, H=256, W=256, N=192, p=P16, q=_lib.ICLR17_QUANT_ROUND, x=None, unclipped=0,
             fold=None):
        bits = [fold, 4 if fold else 0, None, None, ctypes.c_double(1.0)]
        return build(B, H, W, N, p, q, x, unclipped, bits)
    return what, kind, args


def _deconv3(bits=False, flag=False):
    def build(B, H, W, N, p, q, x, unclipped, fold):
        tail = (fold if bits else []) + ([None] if flag else [])
        return [p, B, H, W, N, p, p, x, p, None, None, unclipped, *tail, None]
    return build


def _bwd_gdn(B, H, W, N, p, q, x, unclipped, fold):   # bwd_deconv_igdn, bwd_conv_gdn
    return [p, None, B, H, W, N, p, p, p, p, p, None, None, p, None, p, None, None, None]


ENGINE_ENTRIES = {
    "iclr17_analysis_conv1_gdn": _entry("conv1_gdn", "image", lambda B, H, W, N, p, *_:
                                        [p, B, H, W, N, p, p, p, p, p, None, None]),
    "iclr17_analysis_conv2_gdn": _entry("conv2_gdn", "image", lambda B, H, W, N, p, *_:
                                        [p, B, H, W, N, p, p, p, p, p, None, None]),
    "iclr17_analysis_conv3_quant_rate": _entry(
        "conv3_quant_rate", "image", lambda B, H, W, N, p, q, *_:
        [p, B, H, W, N, p, q, None, p, None, None, p, p, None]),
    "iclr17_analysis_conv3": _entry("conv3", "image", lambda B, H, W, N, p, *_:
                                    [p, B, H, W, N, p, p, None]),
    "iclr17_synthesis_deconv3": _entry("deconv3", "image", _deconv3()),
    "iclr17_synthesis_deconv3_x6": _entry("deconv3_x6", "image", _deconv3()),
    "iclr17_synthesis_deconv3_x6_cm": _entry("deconv3_x6", "image", _deconv3()),
    "iclr17_synthesis_deconv3_x6_cm_bits": _entry("deconv3_x6", "image", _deconv3(bits=True)),
    "iclr17_synthesis_deconv3_h3": _entry("deconv3_h3", "image", _deconv3(bits=True, flag=True)),
    "iclr17_synthesis_deconv3_bf16": _entry("deconv3_bf16", "image", _deconv3()),
    "iclr17_synthesis_deconv3_bf16_bits": _entry("deconv3_bf16", "image", _deconv3(bits=True)),
    "iclr17_analysis_conv1_gdn_x6": _entry("conv1_gdn_x6", "image", lambda B, H, W, N, p, *_:
                                           [p, B, H, W, N, p, p, p, p, None, p, None, None, None]),
    "iclr17_analysis_conv1x6_gdn": _entry("conv1x6_gdn", "image", lambda B, H, W, N, p, *_:
                                          [p, B, H, W, N, p, p, p, p, p, None, None, None]),
    "iclr17_analysis_conv2_gdn_x6": _entry("conv2_gdn_x6", "image", lambda B, H, W, N, p, *_:
                                           [p, B, H, W, N, p, p, p, p, p, p, None, None, None]),
    "iclr17_analysis_conv3_quant_rate_x6": _entry(
        "conv3_quant_rate_x6", "image", lambda B, H, W, N, p, q, *_:
        [p, B, H, W, N, p, q, None, p, None, None, p, None, p, None]),
    "iclr17_analysis_conv3_quant_rate_x6w": _entry(
        "conv3_quant_rate_x6w", "image", lambda B, H, W, N, p, q, *_:
        [p, B, H, W, N, p, p, q, None, p, None, None, p, None, p, None]),
    "iclr17_bwd_deconv3_igdn": _entry(
        "bwd_deconv3_igdn", "image", lambda B, H, W, N, p, *_:
        [p, B, H, W, N, p, None, p, p, p, p, None, None, p, None, p, None, None, None]),
    "iclr17_synthesis_deconv_igdn": _entry("deconv_igdn", "grid", lambda B, H, W, N, p, *_:
                                           [p, B, H, W, N, p, p, p, p, p, None, None]),
    "iclr17_synthesis_deconv_igdn_x6": _entry(
        "deconv_igdn_x6", "grid", lambda B, H, W, N, p, *_:
        [p, B, H, W, N, p, p, p, p, p, p, None, None, None]),
    "iclr17_synthesis_deconv_igdn_x6_cm": _entry(
        "deconv_igdn_x6", "grid", lambda B, H, W, N, p, *_:
        [p, B, H, W, N, p, p, p, p, p, p, None, None, None]),
    "iclr17_bwd_deconv_igdn": _entry("bwd_deconv_igdn", "grid", _bwd_gdn),
    "iclr17_bwd_conv_gdn": _entry("bwd_conv_gdn", "grid", _bwd_gdn),
    "iclr17_bwd_deconv_rate": _entry(
        "bwd_deconv_rate", "grid", lambda B, H, W, N, p, *_:
        [p, None, B, H, W, N, p, None, None, None, ctypes.c_float(1.0), p, None, None, None]),
}


def test_cpu_tensors_fail_loudly():
    from iclr_17_compression_amd.model import ImageCompressor
    net = ImageCompressor(128).eval()
    with pytest.raises(_lib.Iclr17Error, match="ROCm GPU"):
        net(torch.rand(1, 3, 32, 32))
    with pytest.raises(_lib.Iclr17Error, match="ROCm GPU"):
        kernels.gdn(torch.rand(1, 128, 4, 4), torch.zeros(128), torch.zeros(128 * 128), False)


def test_msssim_window_matches_reference():
    """csrc/msssim.hip embeds the reference's fp32 Gaussian window (ms_ssim_torch.py:5-18) as hex
    constants; they must equal the oracle's (reference-identical) window bit for bit."""
    import re
    from oracle import codec_ref as oracle
    text = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "msssim.hip")).read()
    block = text[text.index("c_gauss[WIN] = {"):]
    block = block[:block.index("};")]
    consts = [float.fromhex(h[:-1]) for h in re.findall(r"-?0x[0-9a-fp.+-]+f", block)]
    assert consts == oracle.gauss_window().tolist()
