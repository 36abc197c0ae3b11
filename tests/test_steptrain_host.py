"""The host side of training along the quantiser-step ladder, no GPU needed:
train.py's step sampling, per-image λ and config keys, forward_train's host checks of ``steps``,
and the argument validation of the three entry points of csrc/steptrain.hip.
"""
import ctypes
import json
import re

import pytest
import torch

from iclr_17_compression_amd import _lib, codec, train
from iclr_17_compression_amd.model import ImageCompressor

P16 = ctypes.c_void_p(16)


# ------------------------------------------------------------------------------ sample_steps
def test_sample_steps_deterministic_and_in_range():
    a = train.sample_steps(3, 17, 64, global_step=5, rank=0, seed=234)
    assert a == train.sample_steps(3, 17, 64, global_step=5, rank=0, seed=234)
    assert len(a) == 64 and all(isinstance(s, int) and 3 <= s <= 17 for s in a)
    assert train.sample_steps(9, 9, 4, 1, 0, 0) == [9] * 4
    # inclusive at both ends, and uniform enough that every index of a small range turns up
    many = train.sample_steps(0, 31, 4096, 1, 0, 0)
    assert set(many) == set(range(32))
    counts = [many.count(s) for s in range(32)]
    assert min(counts) > 128 - 60 and max(counts) < 128 + 60   # mean 128, σ ≈ 11


def test_sample_steps_differ_across_ranks_steps_and_seeds():
    base = train.sample_steps(0, 31, 32, global_step=7, rank=0, seed=1)
    assert base != train.sample_steps(0, 31, 32, global_step=7, rank=1, seed=1)
    assert base != train.sample_steps(0, 31, 32, global_step=8, rank=0, seed=1)
    assert base != train.sample_steps(0, 31, 32, global_step=7, rank=0, seed=2)
    # rank and step do not alias: (rank 1, step 0) is not (rank 0, step 1)
    assert train.sample_steps(0, 31, 32, 0, 1, 1) != train.sample_steps(0, 31, 32, 1, 0, 1)


# ------------------------------------------------------------------------------ step_lambdas
def test_step_lambdas_exact_values():
    lam = 8192
    got = train.step_lambdas(lam, [8, 0, 16, 12, 9])
    assert got[0] == lam                       # Δ = 1 at the unit step: exactly lam
    assert got[1] == lam * 16.0                # Δ = 1/4
    assert got[2] == lam / 16.0                # Δ = 4
    assert got[3] == lam / 4.0                 # Δ = 2
    d9 = codec.step_size(9)
    assert got[4] == lam / d9 ** 2
    assert train.step_lambdas(lam, [8, 0, 31], "constant") == [float(lam)] * 3
    assert train.step_lambdas(lam, [3, 20]) == train.step_lambdas(lam, [3, 20], "inverse-square")
    with pytest.raises(ValueError, match="step_lambda"):
        train.step_lambdas(lam, [8], "linear")
    with pytest.raises(_lib.Iclr17Error, match="quantiser step index"):
        train.step_lambdas(lam, [32])


# ------------------------------------------------------------------------------ parse_config
def _cfg(tmp_path, **keys):
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(keys))
    return str(path)


def test_parse_config_accepts_steps(tmp_path):
    cfg = train.parse_config(_cfg(tmp_path, steps=[4, 20]))
    assert cfg["steps"] == [4, 20] and cfg["step_lambda"] == "inverse-square"
    cfg = train.parse_config(_cfg(tmp_path, steps=[0, 31], step_lambda="constant"))
    assert cfg["step_lambda"] == "constant"
    assert train.parse_config(_cfg(tmp_path, steps=[8, 8]))["steps"] == [8, 8]
    # absent: today's config, nothing added
    plain = train.parse_config(_cfg(tmp_path, train_lambda=512))
    assert "steps" not in plain and "step_lambda" not in plain
    assert plain == {**train.parse_config(""), "train_lambda": 512}


@pytest.mark.parametrize("bad", [[4], [4, 20, 21], [20, 4], [-1, 4], [0, 32], [1.0, 4], [True, 4],
                                 "4-20", 8, None, ["4", "20"]])
def test_parse_config_rejects_malformed_steps(tmp_path, bad):
    with pytest.raises(ValueError, match=re.escape("config: steps must be [lo, hi]")):
        train.parse_config(_cfg(tmp_path, steps=bad))


def test_parse_config_rejects_malformed_step_lambda(tmp_path):
    with pytest.raises(ValueError, match="config: step_lambda must be one of"):
        train.parse_config(_cfg(tmp_path, steps=[4, 20], step_lambda="linear"))
    with pytest.raises(ValueError, match="config: step_lambda needs steps"):
        train.parse_config(_cfg(tmp_path, step_lambda="constant"))


# ------------------------------------------------------------------------------ forward_train
def test_forward_train_checks_steps_before_any_device_use():
    """Wrong length, range or type raise on the host: the image here is a CPU tensor, which the
    first device check would reject with another message."""
    net = ImageCompressor(out_channel_N=128).train()
    x = torch.zeros(2, 3, 32, 32)
    for steps, text in (([8], "1 steps for a batch of 2"),
                        ([8, 8, 8], "3 steps for a batch of 2"),
                        (torch.tensor([1, 2, 3]), "3 steps for a batch of 2"),
                        ([8, 32], "quantiser step index 32"),
                        ([-1, 8], "quantiser step index -1"),
                        (32, "quantiser step index 32"),
                        ([8.0, 8], "quantiser step index 8.0"),
                        (torch.tensor([8.0, 8.0]), "steps must be an integer tensor"),
                        (True, "steps must be an int, a sequence or an integer tensor")):
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            net.forward_train(x, steps=steps)
    with pytest.raises(_lib.Iclr17Error, match="requires a gradient is not supported"):
        net.forward_train(x.clone().requires_grad_(True), steps=[8, 8])
    with pytest.raises(_lib.Iclr17Error, match="distortion must be"):
        net.forward_train(x, steps=[8, 8], distortion="psnr")
    # valid steps get as far as the device check
    for steps in (8, [0, 31], torch.tensor([3, 4]), torch.tensor([3, 4], dtype=torch.int32)):
        with pytest.raises(_lib.Iclr17Error, match="runs only on a ROCm GPU"):
            net.forward_train(x, steps=steps)


# ------------------------------------------------------------------------------ the C ABI
def _fwd(B=1, h=4, w=4, N=192, p=P16, **null):
    a = {k: p for k in ("y", "noise", "steps", "rate", "z", "deq", "part")}
    a.update(null)
    return [a["y"], a["noise"], B, h, w, N, a["steps"], a["rate"], a["z"], a["deq"], a["part"], None]


def _bwd(B=1, h=4, w=4, N=192, p=P16, **null):
    a = {k: p for k in ("z", "g", "steps", "rate", "gbits", "gy", "part")}
    a.update(null)
    return [a["z"], a["g"], B, h, w, N, a["steps"], a["rate"], a["gbits"], a["gy"], a["part"], None]


def test_argument_validation_without_gpu():
    """Every check of the three entries fires on the host before a kernel could be launched."""
    for name, what, args, ptrs in (
            ("iclr17_step_noise_rate", "step_noise_rate", _fwd,
             ("y", "noise", "steps", "rate", "z", "deq", "part")),
            ("iclr17_step_noise_rate_bwd", "step_noise_rate_bwd", _bwd,
             ("z", "g", "steps", "rate", "gbits", "gy", "part"))):
        def rejects(text, **kw):
            with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
                _lib.call(name, *args(**kw))
            assert text in _lib.last_error(), name
        for k in ptrs:
            rejects(f"{what}: null pointer", **{k: None})
        rejects(f"{what}: bad shape B=0 h=4 w=4 N=192", B=0)
        rejects(f"{what}: bad shape B=1 h=0 w=4 N=192", h=0)
        rejects(f"{what}: bad shape B=1 h=4 w=-3 N=192", w=-3)
        rejects(f"{what}: bad shape B=1 h=4 w=4 N=0", N=0)
        # any N ≥ 1 whose 11·N floats fit the LDS; beyond that, reported as rate_sweep reports it
        rejects(f"{what}: N=1500 needs 66000 bytes of LDS", N=1500)
    assert _lib.query("iclr17_step_rate_bwd_partials", 16, 16) == 16
    assert _lib.query("iclr17_step_rate_bwd_partials", 5, 7) == 3
    assert _lib.query("iclr17_step_rate_bwd_partials", 1, 1) == 1
    assert _lib.query("iclr17_step_rate_bwd_partials", 0, 4) == 0

    def recon(B=2, per=3 * 16 * 16, r=P16, x=P16, out=P16):
        return [r, x, P16, None, B, per, out, None]
    for kw in ({"r": None}, {"x": None}, {"out": None}):
        with pytest.raises(_lib.Iclr17Error, match="grad_recon_images: null pointer"):
            _lib.call("iclr17_grad_recon_images", *recon(**kw))
    with pytest.raises(_lib.Iclr17Error, match=re.escape("grad_recon_images: bad shape B=0")):
        _lib.call("iclr17_grad_recon_images", *recon(B=0))
    with pytest.raises(_lib.Iclr17Error, match=re.escape("bad shape B=2 per_image=0")):
        _lib.call("iclr17_grad_recon_images", *recon(per=0))
