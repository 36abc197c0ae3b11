"""One forward chain per precision mode (iclr_17_compression_amd/chain.py), carried modes and the
scoped x6 fall-back.

Every comparison is of bit patterns: the entries compared launch the same kernels with the same
arguments. Shapes: B=2, 64×96 (two 16-row × three 16-column tiles at the latent-side layers,
non-square so an H/W swap shows), trained-like weights at N=192, one case also at N=128.
"""
import os
import sys

import numpy as np
import pytest
import torch

from iclr_17_compression_amd import chain, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor

pytestmark = pytest.mark.gpu

LAM = 0.01 * 255.0 ** 2


def _net(N, device):
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
    return net.to(device).eval()


def _image(device):
    return torch.from_numpy(synth.to_unit_float(synth.image_u8(5, 2, 64, 96))).to(device)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


@pytest.fixture
def default_mode():
    """Sets the process default for a test and puts the old one back (with the real
    kernels.set_precision, whatever the test patched in)."""
    real, old = kernels.set_precision, kernels.precision()
    yield real
    real(old)


# ------------------------------------------------------------ the fall-back leaves the default
@pytest.mark.parametrize("entry", ["evaluate", "compress"])
def test_x6_fallback_never_sets_the_default(device, default_mode, monkeypatch, entry):
    default_mode("h3")
    net = _net(192, device)
    with torch.no_grad():   # the overflow model of test_gpu_h3_range._encoder_overflow
        net.Encoder.conv1.bias[0] = 1e4
        net.Encoder.gdn1.gamma[0].zero_()
        net.Encoder.gdn1.beta[0] = 0.0
    x = _image(device)

    def refuse(mode):
        raise AssertionError(f"library code called set_precision({mode!r})")

    monkeypatch.setattr(kernels, "set_precision", refuse)
    with torch.no_grad():
        if entry == "evaluate":
            res = net.evaluate(x, h3_overflow="x6")
            assert bool(torch.isfinite(res["bpp"]).all())   # the x6 rerun's results came back
        else:
            res = net.compress(x)
            assert len(res["strings"]) == 2 and all(len(s) > 4 for s in res["strings"])
        assert kernels.h3_range_overflowed(device)   # the h3 chain did overflow
    assert kernels.precision() == "h3"


# ------------------------------------------------------------ each h3 training entry begins a chain
def test_h3_training_entries_begin_their_own_chain(device, default_mode):
    """A training step, Encoder(x) with grad and Decoder(ŷ) with grad in h3 each begin their own
    chain: run right after an h3 eval chain that overflowed the range on the same stream (its flag
    still set), every output and gradient of the three is finite."""
    default_mode("h3")
    bad = _net(192, device)
    with torch.no_grad():   # the overflow model of test_gpu_h3_range._encoder_overflow
        bad.Encoder.conv1.bias[0] = 1e4
        bad.Encoder.gdn1.gamma[0].zero_()
        bad.Encoder.gdn1.beta[0] = 0.0
    net = _net(192, device).train()
    x = _image(device)
    noise = torch.from_numpy(synth.uniform(11, (2, 192, 4, 6), -0.5, 0.5).astype(np.float32)).to(device)
    with torch.no_grad():
        y_hat = torch.round(net.Encoder(x))

    def overflow():
        with torch.no_grad():
            bad.evaluate(x)
        assert kernels.h3_range_overflowed(device)

    def finite(outs, modules, inp):
        torch.cuda.synchronize()
        named = [(f"out{i}", o) for i, o in enumerate(outs)] + [("input", inp.grad)]
        named += [(n, p.grad) for m in modules for n, p in m.named_parameters()]
        for n, t in named:
            assert t is not None and bool(torch.isfinite(t).all()), n

    overflow()
    net.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    clipped, mse, bpp = net.forward_train(xg, noise)
    (LAM * mse + bpp).backward()
    finite((clipped, mse, bpp), [net], xg)

    overflow()
    net.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    y = net.Encoder(xg)
    y.sum().backward()
    finite((y,), [net.Encoder], xg)

    overflow()
    net.zero_grad(set_to_none=True)
    yg = y_hat.clone().requires_grad_(True)
    recon = net.Decoder(yg)
    recon.sum().backward()
    finite((recon,), [net.Decoder], yg)


# ------------------------------------------------------------ backward in the forward's mode
def _codec_loss(net, x, noise):
    _, mse, bpp = net.forward_train(x, noise)
    return LAM * mse + bpp


def _encoder_loss(net, x, noise):
    return net.Encoder(x).sum()


def _decoder_loss(net, x, noise):
    return net.Decoder(x).sum()


def _grads(net, modules, x, noise, loss_fn, set_precision, backward_mode=None):
    net.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    loss = loss_fn(net, x, noise)
    if backward_mode is not None:
        set_precision(backward_mode)
    loss.backward()
    torch.cuda.synchronize()
    named = [(n, p.grad) for m in modules for n, p in m.named_parameters()] + [("input", x.grad)]
    assert all(g is not None for _, g in named), [n for n, g in named if g is None]
    return [(n, g.clone()) for n, g in named]


@pytest.mark.parametrize("what", ["codec", "encoder", "decoder"])
@pytest.mark.parametrize("mode", ["h3", "x6", "fp32"])
def test_backward_runs_in_the_forwards_mode(device, default_mode, mode, what):
    """The gradients of a forward in ``mode`` do not depend on the process default at backward
    time: all parameters' and the input's are bitwise those of a run with the mode constant."""
    other = "x6" if mode == "fp32" else "fp32"
    net = _net(192, device).train()
    x = _image(device)
    noise = torch.from_numpy(synth.uniform(11, (2, 192, 4, 6), -0.5, 0.5).astype(np.float32)).to(device)
    if what == "codec":
        modules, loss_fn, inp = [net], _codec_loss, x
    elif what == "encoder":
        modules, loss_fn, inp = [net.Encoder], _encoder_loss, x
    else:
        modules, loss_fn = [net.Decoder], _decoder_loss
        default_mode(mode)
        with torch.no_grad():
            inp = torch.round(net.Encoder(x))
    default_mode(mode)
    ref = _grads(net, modules, inp, noise, loss_fn, default_mode)
    default_mode(mode)
    got = _grads(net, modules, inp, noise, loss_fn, default_mode, backward_mode=other)
    assert len(ref) == len(got) == sum(len(list(m.parameters())) for m in modules) + 1
    if what == "codec":
        assert len(ref) == 31
    for (n, a), (_, b) in zip(ref, got):
        assert _bits_equal(a, b), n


# ------------------------------------------------------------ one chain, every entry
@pytest.mark.parametrize("mode,N", [("h3", 192), ("x6", 192), ("fp32", 192), ("bf16", 192), ("h3", 128)])
def test_every_entry_runs_the_same_chain(device, default_mode, mode, N):
    default_mode(mode)
    net = _net(N, device)
    x = _image(device)
    B, _, H, W = x.shape
    with torch.no_grad():
        clipped, y_hat, bpp = net(x)
        run = net.run(x, x_ref_sse=True, want_y=True)
        ev = net.evaluate(x, want_y=True)
        y = net.Encoder(x)
        recon = net.Decoder(y_hat)
        run_bits = run.get("bits_per_image")
        if run_bits is None:
            run_bits, _ = kernels.reduce_partials(run["bits_partial"])
        _, run_bpp = kernels.reduce_partials(run["bits_partial"], 1.0 / (B * H * W), per_image=False)
        sse, _ = kernels.reduce_partials(run["sse_partial"])
    assert (run.get("bits_per_image") is not None) == (mode == "h3")
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()  # noqa: E731
    # ŷ: forward, run, evaluate, round(Encoder)
    assert _bits_equal(y_hat, nchw(run["y_hat"]))
    assert _bits_equal(y_hat, ev["y_hat"])
    assert _bits_equal(y_hat, torch.round(y))
    # y: run, evaluate, Encoder
    assert _bits_equal(ev["y"], nchw(run["y"]))
    assert _bits_equal(ev["y"], y)
    # the reconstruction: forward, run, evaluate, Decoder(ŷ)
    assert _bits_equal(clipped, run["clipped"])
    assert _bits_equal(clipped, ev["clipped"])
    assert _bits_equal(clipped, recon.clamp(0.0, 1.0))
    # the rate and the distortion
    assert _bits_equal(bpp, run_bpp)
    assert _bits_equal(ev["bpp"], run_bits / (H * W))
    assert _bits_equal(ev["mse"], sse / (3 * H * W))
    assert bool(torch.isfinite(ev["bpp"]).all()) and bool(torch.isfinite(bpp))


def test_latent_operand_is_the_decoders_input(device, default_mode):
    """decode() on the operand chain.MODES[mode].latent_operand makes is Decoder(y), in each mode."""
    net = _net(192, device)
    default_mode("h3")
    with torch.no_grad():
        y = torch.round(net.Encoder(_image(device)))
        y_nhwc = net.Decoder.to_nhwc(y)
        for mode in kernels.PRECISIONS:
            default_mode(mode)
            m = chain.MODES[mode]
            operand = {} if m.operand is None else {m.operand: m.latent_operand(y_nhwc)}
            _, recon, _ = net.Decoder.decode(y_nhwc, **operand)
            assert _bits_equal(recon, net.Decoder(y)), mode
            assert bool(torch.isfinite(recon).all()), mode


# ------------------------------------------------------------ deconv3_h3 through _deconv3_halo
def test_deconv3_h3_returns_are_the_recorded_ones(device, default_mode, golden_dir):
    """Every value ``deconv3_h3`` returns, for bits=None, bits=(p, s) and with bits_per_image, is
    bitwise what the wrapper returned before it went through ``_deconv3_halo``
    (tests/golden/gen_deconv3_h3.py recorded them at that commit)."""
    sys.path.insert(0, golden_dir)
    try:
        import gen_deconv3_h3 as gen
    finally:
        sys.path.remove(golden_dir)
    default_mode("h3")
    g = np.load(os.path.join(golden_dir, "g10_deconv3_h3_n128.npz"))
    net, x = gen.model_and_image(device)
    hs = torch.from_numpy(g["hs"]).to(device)
    bp = torch.from_numpy(g["bits_partial"]).to(device)
    with torch.no_grad():
        for case in gen.CASES:
            out = gen.run_case(net, x, hs, bp, case)
            assert len(out) == int(g[f"{case}_len"]) == {"none": 3, "total": 4, "per_image": 5}[case]
            for i, t in enumerate(out):
                assert t is not None, (case, i)   # x_ref and want_recon are given: nothing is None
                assert _bits_equal(t.cpu(), torch.from_numpy(g[f"{case}_{i}"])), (case, i)
