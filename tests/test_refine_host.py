"""The host side of latent refinement (codec.py, "Latent refinement"): what
``rate_request`` accepts and rejects, the value checks and the command line. No GPU."""
import inspect
import math

import numpy as np
import pytest

from iclr_17_compression_amd import codec, kernels
from iclr_17_compression_amd._lib import Iclr17Error
from iclr_17_compression_amd.model import ImageCompressor

LAM = 650.25


def test_refine_request():
    assert codec.rate_request(2, step=5, refine=3, refine_lambda=LAM) == \
        ("refine", 5, 3, [LAM, LAM], codec.DEFAULT_REFINE_LR)
    assert codec.rate_request(2, refine=7, refine_lambda=[1, 2.5], refine_lr=0.2) == \
        ("refine", codec.UNIT_STEP, 7, [1.0, 2.5], 0.2)
    assert codec.rate_request(1, refine=1, refine_lambda=np.float32(2.0), tile=16)[0] == "refine"
    assert codec.rate_request(1, refine=1, refine_lambda=0)[3] == [0.0]


@pytest.mark.parametrize("kw", [{}, {"step": 8}, {"step": 3, "tile": 8}, {"bpp": 0.5},
                                {"rdo": 0.1, "step": 9}, {"psnr": 30.0}, {"msssim": 0.9},
                                {"step_offsets": [None, None]}, {"max_bytes": [500, 900]}])
def test_refine_zero_and_none_build_todays_request(kw):
    want = codec.rate_request(2, **kw)
    assert codec.rate_request(2, refine=0, **kw) == want
    assert codec.rate_request(2, refine=None, **kw) == want
    # λ and the learning rate are still checked, and change nothing
    assert codec.rate_request(2, refine=0, refine_lambda=LAM, refine_lr=0.1, **kw) == want


@pytest.mark.parametrize("name,value", [("max_bytes", 900), ("bpp", 0.5), ("psnr", 30.0),
                                        ("msssim", 0.9), ("rdo", 0.1),
                                        ("step_offsets", [None, None])])
def test_refine_with_another_option_raises_naming_the_pair(name, value):
    with pytest.raises(Iclr17Error) as e:
        codec.rate_request(2, refine=2, refine_lambda=LAM, **{name: value})
    assert str(e.value) == codec.REFINE_WITH[name]
    said = "step_offsets / a step map" if name == "step_offsets" else name
    assert f"refine with {said}:" in str(e.value) and "not built" in str(e.value)


def test_refine_without_lambda_and_in_bf16():
    with pytest.raises(Iclr17Error) as e:
        codec.rate_request(1, step=8, refine=1)
    assert str(e.value) == codec.REFINE_NEEDS_LAMBDA and "refine without refine_lambda" in str(e.value)
    with kernels.precision_scope("bf16"):
        with pytest.raises(Iclr17Error) as e:
            codec.rate_request(1, step=8, refine=1, refine_lambda=LAM)
        assert str(e.value) == codec.REFINE_IN_BF16 and "refine in the bf16 precision mode" in str(e.value)
        assert codec.rate_request(1, step=8, refine=0, refine_lambda=LAM) == ("step", 8)
    for mode in ("h3", "x6", "fp32"):
        with kernels.precision_scope(mode):
            assert codec.rate_request(1, refine=1, refine_lambda=LAM)[0] == "refine"


@pytest.mark.parametrize("bad", [True, False, -1, 1.0, 2.5, "3", np.float32(2), [1]])
def test_refine_value(bad):
    with pytest.raises(Iclr17Error, match="refine must be an integer >= 0"):
        codec.rate_request(1, refine=bad, refine_lambda=LAM)


def test_refine_value_accepts():
    assert codec.refine_value(None) == 0 and codec.refine_value(0) == 0
    assert codec.refine_value(np.int64(4)) == 4


@pytest.mark.parametrize("bad,why", [(True, "real number"), ("1", "real number"),
                                     (-1.0, "finite and >= 0"), (math.nan, "finite and >= 0"),
                                     (math.inf, "finite and >= 0"), (1e39, "finite and >= 0")])
def test_refine_lambda_value(bad, why):
    with pytest.raises(Iclr17Error, match=f"refine_lambda must be .*{why}"):
        codec.rate_request(1, refine=1, refine_lambda=bad)
    with pytest.raises(Iclr17Error, match=f"refine_lambda must be .*{why}"):
        codec.rate_request(2, refine=1, refine_lambda=[1.0, bad])


def test_refine_lambda_length():
    with pytest.raises(Iclr17Error, match="refine_lambda has 3 values for 2 images"):
        codec.rate_request(2, refine=1, refine_lambda=[1.0, 2.0, 3.0])


@pytest.mark.parametrize("bad", [True, "0.1", 0, 0.0, -0.1, math.nan, math.inf])
def test_refine_lr_value(bad):
    with pytest.raises(Iclr17Error, match="refine_lr must be"):
        codec.rate_request(1, refine=1, refine_lambda=LAM, refine_lr=bad)


def test_default_lr_and_objective():
    assert codec.refine_lr_value(None) == codec.DEFAULT_REFINE_LR > 0
    assert codec.refine_objective(100.0, 0, LAM) == 100.0
    assert codec.refine_objective(10.0, 65025 * 3, 2.0) == 12.0
    assert codec.refine_objective(1.5, 7, LAM) == 1.5 + (LAM / 3.0) * 7.0 / 65025.0


def test_new_keywords_come_last():
    """refine and its two companions are appended: no existing parameter changes position."""
    for fn, before in ((codec.rate_request, "estimate"), (codec.compress_images, "msssim"),
                       (codec.evaluate_images, "msssim"),
                       (ImageCompressor.compress_images, "msssim"),
                       (ImageCompressor.evaluate_images, "msssim")):
        names = list(inspect.signature(fn).parameters)
        assert names[-4:] == [before, "refine", "refine_lambda", "refine_lr"], fn


def test_command_line():
    ap = codec.build_parser()
    a = ap.parse_args(["encode", "in.png", "out.i17c", "--weights", "w", "--step", "6", "--refine",
                       "20", "--refine-lambda", "650.25", "--refine-lr", "0.1", "--tile", "16"])
    assert (a.refine, a.refine_lambda, a.refine_lr, a.step, a.tile) == (20, 650.25, 0.1, 6, 16)
    a = ap.parse_args(["encode", "in.png", "out.i17c", "--weights", "w"])
    assert (a.refine, a.refine_lambda, a.refine_lr) == (None, None, None)
    a = ap.parse_args(["eval", "a.png", "b.png", "--weights", "w", "--steps", "4,8", "--refine", "5",
                       "--refine-lambda", "100"])
    assert (a.refine, a.refine_lambda, a.refine_lr) == (5, 100.0, None)
    with pytest.raises(SystemExit):
        ap.parse_args(["decode", "a", "b", "--weights", "w", "--refine", "3"])
    # the pairs that raise do so before the device is touched
    with pytest.raises(Iclr17Error, match="refine with bpp"):
        codec.main(["encode", "in.png", "out.i17c", "--weights", "w", "--bpp", "0.5", "--refine",
                    "3", "--refine-lambda", "1"])
    with pytest.raises(Iclr17Error, match="refine with rdo"):
        codec.main(["eval", "in.png", "--weights", "w", "--rdo", "0.5", "--refine", "3",
                    "--refine-lambda", "1"])
    with pytest.raises(Iclr17Error, match="refine without refine_lambda"):
        codec.main(["encode", "in.png", "out.i17c", "--weights", "w", "--refine", "3"])
    with pytest.raises(Iclr17Error, match="bf16 precision mode"):
        codec.main(["encode", "in.png", "out.i17c", "--weights", "w", "--refine", "3",
                    "--refine-lambda", "1", "--precision", "bf16"])
