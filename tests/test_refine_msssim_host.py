"""The host side of latent refinement for MS-SSIM (codec.py): the λ that carries the
objective, what ``rate_request`` accepts and rejects, the size rule, the host twin of the device's
J and the command line. No GPU."""
import inspect
import math

import numpy as np
import pytest

from iclr_17_compression_amd import _lib, codec, kernels
from iclr_17_compression_amd._lib import Iclr17Error
from iclr_17_compression_amd.model import ImageCompressor


def test_msssim_lambda_keeps_its_type():
    lam = codec.msssim_lambda(8.0)
    assert isinstance(lam, codec.MsssimLambda) and isinstance(lam, float) and lam == 8.0
    assert isinstance(codec.refine_lambda_value(lam), codec.MsssimLambda)
    assert type(codec.refine_lambda_value(8.0)) is float
    assert isinstance(codec.msssim_lambda(np.float32(2.0)), codec.MsssimLambda)
    assert isinstance(codec.msssim_lambda(lam), codec.MsssimLambda)
    assert codec.msssim_lambda(0) == 0.0 and "msssim_lambda" in repr(lam)
    req = codec.rate_request(2, step=5, refine=3, refine_lambda=lam)
    assert req == ("refine", 5, 3, [8.0, 8.0], codec.DEFAULT_REFINE_LR)
    assert all(isinstance(v, codec.MsssimLambda) for v in req[3])
    req = codec.rate_request(2, refine=1, refine_lambda=[codec.msssim_lambda(1), codec.msssim_lambda(2.5)])
    assert req[:3] == ("refine", codec.UNIT_STEP, 1) and req[3] == [1.0, 2.5]
    assert codec.refine_objective_kind(req[3]) == "ms-ssim"
    assert codec.refine_objective_kind([1.0, 2.0]) == "mse"


@pytest.mark.parametrize("bad,why", [(True, "real number"), ("1", "real number"),
                                     (-1.0, "finite and >= 0"), (math.nan, "finite and >= 0"),
                                     (math.inf, "finite and >= 0"), (1e39, "finite and >= 0")])
def test_msssim_lambda_rejects_what_refine_lambda_value_rejects(bad, why):
    with pytest.raises(Iclr17Error, match=f"refine_lambda must be .*{why}"):
        codec.msssim_lambda(bad)
    if isinstance(bad, float):      # made without the check: rate_request's own rejects it
        with pytest.raises(Iclr17Error, match=f"refine_lambda must be .*{why}"):
            codec.rate_request(1, refine=1, refine_lambda=codec.MsssimLambda(bad))
        with pytest.raises(Iclr17Error, match=f"refine_lambda must be .*{why}"):
            codec.rate_request(2, refine=1, refine_lambda=[codec.msssim_lambda(1.0), codec.MsssimLambda(bad)])


def test_mixed_objectives_raise():
    for mixed in ([codec.msssim_lambda(8.0), 8.0], [1.0, codec.msssim_lambda(2.0)]):
        with pytest.raises(Iclr17Error) as e:
            codec.rate_request(2, step=8, refine=2, refine_lambda=mixed)
        assert str(e.value) == codec.REFINE_MIXED_OBJECTIVES and "mixes plain and MS-SSIM" in str(e.value)
        with pytest.raises(Iclr17Error):
            codec.refine_objective_kind(mixed)


def test_small_image_raises_naming_it_before_any_device_work():
    """The net is on the CPU and holds no device: the size rule speaks first."""
    net = ImageCompressor(out_channel_N=128)
    ims = [np.zeros((176, 192, 3), np.uint8), np.zeros((160, 192, 3), np.uint8)]
    with pytest.raises(Iclr17Error, match=r"image 1 \(160x192\) is 160x192, too small"):
        codec.compress_images(net, ims, step=8, refine=2, refine_lambda=codec.msssim_lambda(8.0))
    with pytest.raises(Iclr17Error, match=r"image 0 \(161x100\) is 161x100, too small"):
        net.evaluate_images([np.zeros((161, 100, 3), np.uint8)], refine=1,
                            refine_lambda=codec.msssim_lambda(1.0))


@pytest.mark.parametrize("kw", [{}, {"step": 8}, {"step": 3, "tile": 8}, {"bpp": 0.5},
                                {"rdo": 0.1, "step": 9}, {"psnr": 30.0}, {"msssim": 0.9},
                                {"max_bytes": [500, 900]}])
def test_plain_requests_are_todays(kw):
    want = codec.rate_request(2, **kw)
    assert codec.rate_request(2, refine=0, refine_lambda=codec.msssim_lambda(8.0), **kw) == want
    plain = codec.rate_request(2, step=5, refine=3, refine_lambda=650.25)
    assert plain == ("refine", 5, 3, [650.25, 650.25], codec.DEFAULT_REFINE_LR)
    assert all(type(v) is float for v in plain[3])


@pytest.mark.parametrize("name,value", [("max_bytes", 900), ("bpp", 0.5), ("psnr", 30.0),
                                        ("msssim", 0.9), ("rdo", 0.1),
                                        ("step_offsets", [None, None])])
def test_pairs_that_raise_still_raise(name, value):
    with pytest.raises(Iclr17Error) as e:
        codec.rate_request(2, refine=2, refine_lambda=codec.msssim_lambda(8.0), **{name: value})
    assert str(e.value) == codec.REFINE_WITH[name]


def test_bf16_still_raises():
    with kernels.precision_scope("bf16"):
        with pytest.raises(Iclr17Error) as e:
            codec.rate_request(1, step=8, refine=1, refine_lambda=codec.msssim_lambda(8.0))
        assert str(e.value) == codec.REFINE_IN_BF16


def test_signatures_still_end_in_the_three_keywords():
    for fn, before in ((codec.rate_request, "estimate"), (codec.compress_images, "msssim"),
                       (codec.evaluate_images, "msssim"),
                       (ImageCompressor.compress_images, "msssim"),
                       (ImageCompressor.evaluate_images, "msssim")):
        names = list(inspect.signature(fn).parameters)
        assert names[-4:] == [before, "refine", "refine_lambda", "refine_lr"], fn


def test_refine_objective_msssim():
    f = codec.refine_objective_msssim
    assert f(100.0, 1.0, 8.0, 161, 177) == 100.0
    assert f(10.0, 0.5, 2.0, 4, 8) == 10.0 + 2.0 * 32.0 * 0.5 == 42.0
    ms = float(np.float32(0.9123))              # an fp32 value, widened
    assert f(1.5, np.float32(0.9123), 8.0, 161, 177) == 1.5 + (8.0 * float(161 * 177)) * (1.0 - ms)
    assert f(1.5, ms, 0.0, 161, 177) == 1.5
    assert math.isnan(f(1.5, math.nan, 8.0, 161, 177))
    # H·W times train.py's λ·(1 − MS-SSIM) + bpp
    H, W, bits, lam = 176, 192, 5000.0, 8.0
    assert f(bits, ms, lam, H, W) == pytest.approx(H * W * (lam * (1.0 - ms) + bits / (H * W)), rel=1e-14)


def test_command_line():
    ap = codec.build_parser()
    a = ap.parse_args(["encode", "in.png", "out.i17c", "--weights", "w", "--step", "6", "--refine",
                       "20", "--refine-lambda", "8", "--refine-distortion", "ms-ssim"])
    assert (a.refine, a.refine_lambda, a.refine_distortion) == (20, 8.0, "ms-ssim")
    got = codec._refine_of(a)
    assert isinstance(got["refine_lambda"], codec.MsssimLambda) and got["refine_lambda"] == 8.0
    a = ap.parse_args(["encode", "in.png", "out.i17c", "--weights", "w", "--refine", "2",
                       "--refine-lambda", "8"])
    assert a.refine_distortion == "mse" and type(codec._refine_of(a)["refine_lambda"]) is float
    a = ap.parse_args(["eval", "a.png", "--weights", "w", "--refine", "5", "--refine-lambda", "100",
                       "--refine-distortion", "ms-ssim"])
    assert a.refine_distortion == "ms-ssim"
    a = ap.parse_args(["eval", "a.png", "--weights", "w"])
    assert a.refine_distortion == "mse" and codec._refine_of(a)["refine_lambda"] is None
    with pytest.raises(SystemExit):
        ap.parse_args(["encode", "in.png", "out.i17c", "--weights", "w", "--refine-distortion", "psnr"])
    with pytest.raises(SystemExit):
        ap.parse_args(["decode", "a", "b", "--weights", "w", "--refine-distortion", "ms-ssim"])
    # the pairs that raise do so before the device is touched
    tail = ["--refine", "3", "--refine-lambda", "1", "--refine-distortion", "ms-ssim"]
    with pytest.raises(Iclr17Error, match="refine with bpp"):
        codec.main(["encode", "in.png", "out.i17c", "--weights", "w", "--bpp", "0.5"] + tail)
    with pytest.raises(Iclr17Error, match="refine with rdo"):
        codec.main(["eval", "in.png", "--weights", "w", "--rdo", "0.5"] + tail)
    with pytest.raises(Iclr17Error, match="refine without refine_lambda"):
        codec.main(["encode", "in.png", "out.i17c", "--weights", "w", "--refine", "3",
                    "--refine-distortion", "ms-ssim"])
    with pytest.raises(Iclr17Error, match="bf16 precision mode"):
        codec.main(["encode", "in.png", "out.i17c", "--weights", "w", "--precision", "bf16"] + tail)


def test_new_entries_are_bound():
    for name in ("iclr17_image_msssim_grad_workspace_size", "iclr17_image_msssim_u8_fwd_saved",
                 "iclr17_image_msssim_u8_bwd", "iclr17_refine_keep_msssim"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert _lib.query("iclr17_image_msssim_grad_workspace_size", 4, 176, 272) > \
        _lib.query("iclr17_image_msssim_workspace_size", 4, 176, 272) > 0
    assert _lib.query("iclr17_image_msssim_grad_workspace_size", 1, 160, 272) == 0
    assert lib.iclr17_refine_keep_msssim is not None
    for fn in ("image_msssim_grad_workspace", "image_msssim_fwd_saved", "image_msssim_bwd",
               "refine_keep_msssim"):
        assert callable(getattr(kernels, fn))
