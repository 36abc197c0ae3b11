"""The h3 engine's narrow-activation main loop (csrc/engine_h3.hip, NARROW) and the chain's wide
word that selects it (include/iclr17.h, iclr17_h3_range_words).

A layer whose input holds only |x| < 1024 puts the 2^11 factor of the hi·hi part product on the
step's one activation fragment instead of the weight fragments. Both forms form the same exact
fp16 × fp16 products in the same order, so their results must be bit-identical — checked here per
layer three ways on the smallest shapes every layer accepts (64×64 images: conv1 out 16², conv2
out 8², ŷ 4²): the narrow form (B = 1, ordinary input, wide word clear), the general form picked
by the wide word (B = 2 with a value of 1500 in image 1: image 0 must not change), and the general
form forced by a one-word flag (nothing past word 0 is read or written then). conv1 splits the
image in its own kernel and keeps the general form; it is here as a producer of the
wide word and for the batch independence of its outputs.
"""
import contextlib

import pytest
import torch

from iclr_17_compression_amd import _lib, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor
from oracle import codec_ref as oracle

pytestmark = pytest.mark.gpu

WIDE = 1500.0   # ≥ 1024 (wide), an integer below 2048 (exact in the hi plane), far below 2^22


@contextlib.contextmanager
def one_word_flag(device):
    """The library told that a range flag is one int: the general form everywhere."""
    kernels.h3_range_flag(device)   # the module's own (two-word) setting happens first
    _lib.call("iclr17_h3_range_words", 1)
    try:
        yield
    finally:
        _lib.call("iclr17_h3_range_words", 2)


_nets = {}


def net_for(N, device):
    if N not in _nets:
        net = ImageCompressor(out_channel_N=N)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
        _nets[N] = net.to(device).eval()
    return _nets[N]


def image(seed, B, H, W):
    return torch.from_numpy(synth.to_unit_float(synth.image_u8(seed, B, H, W)))


def img0(t):
    """Image 0 of an output: planes first for the h3 / x6 forms ([P][B][…]), batch first otherwise."""
    return t[:, 0] if t.dtype == torch.int16 else t[0]


def layer_cases(N, device):
    """name → (inputs(B): fp32 input tensors, image 1 holding one wide value; run(inputs): outputs).
    run() turns activations into the h3 form itself, so the producers see the values."""
    net = net_for(N, device)
    enc, dec = net.Encoder, net.Decoder
    w2h, w3h = enc.packed_h3()
    x1, x2 = dec.packed_h3k()[:2]
    g1, g2 = enc.gdn1.effective_params_h3(), enc.gdn2.effective_params_h3()
    i1, i2 = dec.igdn1.effective_params_h3(), dec.igdn2.effective_params_h3()
    rate, rtab = net.bitEstimator.packed(), net.bitEstimator.rate_table()

    def act(seed, h, w, integer=False):
        def make(B):
            if integer:
                a = torch.round(torch.from_numpy(synth.uniform(seed, (2, h, w, N), -6, 6)))
            else:
                a = torch.from_numpy(synth.normal_like(seed, (2, h, w, N), 0.7))
            a[1, h // 2, w // 3, 5] = -WIDE
            return a[:B].contiguous().to(device)
        return make

    def img(B):
        x = image(7, 2, 64, 64)
        x[1, 1, 30, 41] = WIDE
        return x[:B].contiguous().to(device)

    noise = torch.from_numpy(synth.uniform(9, (2, N, 4, 4), -0.5, 0.5)).to(device)
    return {
        "conv1": (img, lambda x: kernels.conv1_gdn_h3(x, enc.packed_conv1_h3(), enc.conv1.bias, *g1, N,
                                                      want_f32=True, want_x6=True, want_pre=True)),
        "conv2": (act(21, 16, 16), lambda a: kernels.conv2_gdn_h3(
            kernels.h3_planes(a, cm=kernels.CONV_CM), w2h, enc.conv2.bias, *g2, want_f32=True,
            want_x6=True, want_pre=True)),
        "conv3_round": (act(22, 8, 8), lambda a: kernels.conv3_quant_rate_h3(
            kernels.h3_planes(a, cm=kernels.CONV_CM), w3h, rate, want_y=True, rtab=rtab)),
        "conv3_noise": (act(23, 8, 8), lambda a: kernels.conv3_quant_rate_h3(
            kernels.h3_planes(a, cm=kernels.CONV_CM), w3h, rate, noise[:a.shape[0]].contiguous(),
            want_y=True)),
        "deconv1": (act(24, 4, 4), lambda a: kernels.deconv_igdn_h3(
            kernels.h3_planes(a, cm=kernels.DECONV_CM), x1, dec.deconv1.bias, *i1, want_f32=True,
            want_x6=True, want_pre=True)),
        "deconv1_int_in": (act(25, 4, 4, integer=True), lambda a: kernels.deconv_igdn_h3(
            kernels.h3_planes(a, cm=kernels.DECONV_CM), x1, dec.deconv1.bias, *i1, want_f32=True,
            int_in=True)),
        "deconv2_chunk_major": (act(26, 8, 8), lambda a: kernels.deconv_igdn_h3(
            kernels.h3_planes(a, cm=kernels.DECONV_CM), x2, dec.deconv2.bias, *i2, want_f32=True,
            chunk_major=True)),
    }


LAYERS = ["conv1", "conv2", "conv3_round", "conv3_noise", "deconv1", "deconv1_int_in",
          "deconv2_chunk_major"]


@pytest.mark.parametrize("N", [128, 192])
@pytest.mark.parametrize("layer", LAYERS)
def test_narrow_and_general_forms_bit_equal(device, N, layer):
    inputs, run = layer_cases(N, device)[layer]
    flag, wide = kernels.h3_range_flag(device), kernels.h3_wide_flag(device)
    with torch.no_grad():
        kernels.h3_chain_begin(device)
        narrow = [t for t in run(inputs(1)) if t is not None]
        assert int(flag.item()) == 0
        assert int(wide.item()) == 0          # ordinary input and output: the narrow form ran
        kernels.h3_chain_begin(device)
        both = [t for t in run(inputs(2)) if t is not None]
        assert int(flag.item()) == 0          # 1500 is wide, not out of range
        if layer != "conv1":                  # conv1 reads the image, no h3 input: it keeps the
            assert int(wide.item()) == 1      # general form; elsewhere the input's producer set
                                              # the word: the general form ran
        with one_word_flag(device):
            kernels.h3_chain_begin(device)
            general = [t for t in run(inputs(1)) if t is not None]
            assert int(flag.item()) == 0 and int(wide.item()) == 0   # word 1 untouched
    assert len(narrow) == len(both) == len(general) >= 2
    for a, b, g in zip(narrow, both, general):
        assert bool(torch.isfinite(a.float()).all()) or a.dtype == torch.int16
        assert torch.equal(img0(a), img0(b)), layer
        assert a.shape == g.shape and torch.equal(a, g), layer


def test_wide_threshold_through_h3_planes(device):
    """|x| < 1024 leaves the wide word clear, 1024 sets it, and so does 2047.9, whose hi part
    rounds to 32 (hi·2^11 would not fit fp16): its consumer runs the general form and gives the
    finite result of the one-word flag's general form."""
    N = 128
    net = net_for(N, device)
    enc = net.Encoder
    w2h, g2 = enc.packed_h3()[0], enc.gdn2.effective_params_h3()
    flag, wide = kernels.h3_range_flag(device), kernels.h3_wide_flag(device)
    base = torch.from_numpy(synth.normal_like(41, (1, 16, 16, N), 0.7))

    def with_peak(v):
        a = base.clone()
        a[0, 9, 3, 77] = v
        return a.to(device)

    def conv2(a):
        return kernels.conv2_gdn_h3(kernels.h3_planes(a, cm=kernels.CONV_CM), w2h, enc.conv2.bias, *g2,
                                    want_f32=True)

    with torch.no_grad():
        for v, expect in ((1023.9, 0), (-1023.9, 0), (1024.0, 1), (-1024.0, 1), (2047.9, 1)):
            kernels.h3_chain_begin(device)
            s = kernels.h3_planes(with_peak(v), cm=kernels.CONV_CM)
            assert int(wide.item()) == expect, v
            kernels.h3_chain_begin(device)
            kernels.h3_planes(with_peak(v).reshape(-1))   # the flat form's kernel
            assert int(wide.item()) == expect and int(flag.item()) == 0, v
        hi = s[0].view(torch.float16).float().abs().max().item()
        assert hi == 32.0                     # 2047.9·2^-6 rounds up to 32
        kernels.h3_chain_begin(device)
        h3w, f32w, _ = conv2(with_peak(2047.9))
        assert int(wide.item()) == 1 and int(flag.item()) == 0
        with one_word_flag(device):
            h3g, f32g, _ = conv2(with_peak(2047.9))
    assert bool(torch.isfinite(f32w).all())
    assert torch.equal(f32w, f32g) and torch.equal(h3w, h3g)


def test_one_word_and_null_flag_write_nothing_past_word_0(device, monkeypatch):
    """With a one-word flag the library takes the general form — the input holds 3000, whose hi
    part (46.9) times 2^11 overflows fp16, so the narrow form would give NaN — and leaves the int
    after the flag alone; with a null flag it runs the general form and writes no flag at all."""
    N = 128
    net = net_for(N, device)
    enc = net.Encoder
    w2h, g2 = enc.packed_h3()[0], enc.gdn2.effective_params_h3()
    a = torch.from_numpy(synth.normal_like(42, (1, 16, 16, N), 0.7))
    a[0, 4, 11, 3] = 3000.0
    a = a.to(device)
    flag, wide = kernels.h3_range_flag(device), kernels.h3_wide_flag(device)

    def conv2():
        return kernels.conv2_gdn_h3(kernels.h3_planes(a, cm=kernels.CONV_CM), w2h, enc.conv2.bias, *g2,
                                    want_f32=True)

    with torch.no_grad():
        kernels.h3_chain_begin(device)
        ref = conv2()                          # two words: wide set, the general form
        assert int(wide.item()) == 1 and int(flag.item()) == 0
        with one_word_flag(device):
            kernels.h3_chain_begin(device)
            wide.fill_(-7)                     # the guard element after the one-word flag
            one = conv2()
            assert int(wide.item()) == -7 and int(flag.item()) == 0
            # the range flag itself still works with one word
            kernels.h3_planes(torch.full((4,), 2.0 ** 23, device=device))
            assert int(flag.item()) == 1 and int(wide.item()) == -7
        kernels.h3_chain_begin(device)
        monkeypatch.setattr(kernels, "h3_range_flag", lambda dev: None)
        null = conv2()
        monkeypatch.undo()
        assert int(wide.item()) == 0 and int(flag.item()) == 0
    assert bool(torch.isfinite(ref[1]).all())
    for r, o, n in zip(ref[:2], one[:2], null[:2]):
        assert torch.equal(r, o) and torch.equal(r, n)


def test_chain_narrow_equals_general_and_oracle(device):
    """The whole h3 chain at 64×64, B = 2: the narrow forms ran (the wide word stays clear), ŷ, the
    clipped image and bpp equal the general forms' bit for bit, and they meet the chain's bars
    against the CPU oracle (latents bit-identical, bpp 1e-5 relative, reconstruction 1e-4)."""
    N = 192
    net = net_for(N, device)
    x = image(0, 2, 64, 64)
    old = kernels.precision()
    kernels.set_precision("h3")
    try:
        with torch.no_grad():
            clipped, y_hat, bpp = net(x.to(device))
            assert int(kernels.h3_wide_flag(device).item()) == 0
            assert int(kernels.h3_range_flag(device).item()) == 0
            with one_word_flag(device):
                clipped_g, y_hat_g, bpp_g = net(x.to(device))
    finally:
        kernels.set_precision(old)
    assert torch.equal(y_hat, y_hat_g) and torch.equal(clipped, clipped_g) and torch.equal(bpp, bpp_g)
    sd = oracle.state_dict_to_torch(synth.trained_like_state_dict(N, 1))
    r_clipped, r_yhat, r_bpp, _, _ = oracle.codec_forward(x, sd)
    assert int((y_hat.cpu() != r_yhat).sum()) == 0
    assert abs(bpp.item() - r_bpp.item()) <= 1e-5 * abs(r_bpp.item())
    assert (clipped.cpu() - r_clipped).abs().max().item() < 1e-4
