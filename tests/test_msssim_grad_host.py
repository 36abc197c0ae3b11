"""The differentiable MS-SSIM / SSIM surface without a GPU: the public names, the argument
checks, the C ABI's workspace query and host-side validation, the training driver's config key
and ImageCompressor.forward_train's ``distortion`` argument."""
import ctypes
import json

import pytest
import torch

from iclr_17_compression_amd import _lib

P = ctypes.c_void_p(256)   # a non-null pointer the host-side checks never dereference


def test_losses_module_exposes_the_three_names():
    import iclr_17_compression_amd as pkg
    from iclr_17_compression_amd import losses
    for name in ("ms_ssim_diff", "ssim_diff", "MSSSIMLoss"):
        assert callable(getattr(losses, name))
        assert getattr(pkg, name) is getattr(losses, name)
    assert isinstance(losses.MSSSIMLoss(data_range=1.0), torch.nn.Module)


def test_reference_argument_checks_fire():
    """ms_ssim_torch.py:102-112 / :140-150 come first, as ValueError, in the reference's order."""
    from iclr_17_compression_amd.losses import MSSSIMLoss, ms_ssim_diff, ssim_diff
    x = torch.rand(1, 3, 176, 176)
    for fn in (ms_ssim_diff, ssim_diff, MSSSIMLoss()):
        with pytest.raises(ValueError, match="4-d"):
            fn(x[0], x[0])
        with pytest.raises(ValueError, match="same dtype"):
            fn(x, x.double())
        with pytest.raises(ValueError, match="same dimensions"):
            fn(x, x[:, :, :170])


def test_cpu_tensors_raise():
    """A differentiable function does not silently move devices."""
    from iclr_17_compression_amd.losses import MSSSIMLoss, ms_ssim_diff, ssim_diff
    x = torch.rand(1, 3, 176, 176, requires_grad=True)
    y = torch.rand(1, 3, 176, 176)
    for fn in (ms_ssim_diff, ssim_diff, MSSSIMLoss()):
        with pytest.raises(_lib.Iclr17Error, match="CUDA"):
            fn(x, y)
        with pytest.raises(_lib.Iclr17Error, match="CUDA"):
            fn(y, y)


def test_grad_workspace_query():
    q = lambda *a: _lib.query("iclr17_ssim_grad_workspace_size", *a)  # noqa: E731
    # 160 → 80 → 40 → 20 → 10 < the 11-tap window; 161 → 81 → 41 → 21 → 11
    assert q(1, 160, 160, 0, 1) == 0 and q(1, 160, 160, 1, 1) == 0
    assert q(1, 161, 161, 0, 1) > 0
    assert q(1, 161, 161, 1, 1) >= q(1, 161, 161, 0, 1)
    assert q(1, 161, 160, 1, 1) == 0 and q(0, 161, 161, 1, 1) == 0
    # single-scale: one level, the window alone bounds the size
    assert q(1, 10, 11, 1, 0) == 0
    assert q(2, 11, 11, 1, 0) >= q(2, 11, 11, 0, 0) > 0
    # the derivative maps are counted: 3 (dX only) or 4 planes-of-every-image per level
    assert q(1, 161, 161, 1, 1) - q(1, 161, 161, 0, 1) == \
        4 * 3 * sum((n - 10) ** 2 for n in (161, 81, 41, 21, 11))


def test_backward_entries_validate_on_the_host():
    need = _lib.query("iclr17_ssim_grad_workspace_size", 1, 176, 176, 1, 1)
    with pytest.raises(_lib.Iclr17Error, match="null pointer"):
        _lib.call("iclr17_ms_ssim_bwd", None, P, 1, 176, 176, 1, P, need, P, P, P, None)
    with pytest.raises(_lib.Iclr17Error, match="null pointer"):   # no gradient
        _lib.call("iclr17_ms_ssim_bwd", P, P, 1, 176, 176, 1, P, need, None, P, P, None)
    with pytest.raises(_lib.Iclr17Error, match="null pointer"):   # no output
        _lib.call("iclr17_ms_ssim_bwd", P, P, 1, 176, 176, 1, P, need, P, None, None, None)
    with pytest.raises(_lib.Iclr17Error, match="workspace too small"):
        _lib.call("iclr17_ms_ssim_bwd", P, P, 1, 176, 176, 1, P, need - 1, P, P, P, None)
    with pytest.raises(_lib.Iclr17Error, match="saved no dY"):
        _lib.call("iclr17_ms_ssim_bwd", P, P, 1, 176, 176, 0, P, need, P, P, P, None)
    with pytest.raises(_lib.Iclr17Error, match="too small for 5 levels"):
        _lib.call("iclr17_ms_ssim_bwd", P, P, 1, 160, 160, 1, P, need, P, P, P, None)
    with pytest.raises(_lib.Iclr17Error, match="too small for 5 levels"):
        _lib.call("iclr17_ms_ssim_fwd_saved", P, P, 1, 160, 160, 1.0, 1, P, need, P, None)
    with pytest.raises(_lib.Iclr17Error, match="workspace too small"):
        _lib.call("iclr17_ms_ssim_fwd_saved", P, P, 1, 176, 176, 1.0, 1, P, need - 1, P, None)
    need1 = _lib.query("iclr17_ssim_grad_workspace_size", 2, 28, 20, 1, 0)
    with pytest.raises(_lib.Iclr17Error, match="null pointer"):   # neither g_ssim nor g_cs
        _lib.call("iclr17_ssim_bwd", P, P, 2, 28, 20, 1, P, need1, None, None, P, P, None)
    with pytest.raises(_lib.Iclr17Error, match="workspace too small"):
        _lib.call("iclr17_ssim_bwd", P, P, 2, 28, 20, 1, P, need1 - 1, P, None, P, None, None)
    with pytest.raises(_lib.Iclr17Error, match="null pointer"):
        _lib.call("iclr17_ssim_fwd_saved", P, P, 2, 28, 20, 1.0, 1, P, need1, P, None, None)


def test_evaluation_entry_points_name_the_differentiable_ones():
    from iclr_17_compression_amd.models import ms_ssim
    x = torch.rand(1, 3, 176, 176, requires_grad=True)
    with pytest.raises(_lib.Iclr17Error, match="no backward.*ms_ssim_diff"):
        ms_ssim(x, x.detach(), data_range=1.0)


def test_parse_config_distortion(tmp_path):
    from iclr_17_compression_amd import train
    assert train.parse_config("").get("distortion", "mse") == "mse"
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps({"distortion": "ms-ssim", "train_lambda": 100}))
    cfg = train.parse_config(str(p))
    assert cfg["distortion"] == "ms-ssim" and cfg["train_lambda"] == 100
    p.write_text(json.dumps({"distortion": "psnr"}))
    with pytest.raises(ValueError, match="distortion"):
        train.parse_config(str(p))


def test_forward_train_rejects_an_unknown_distortion_before_the_device():
    from iclr_17_compression_amd.model import ImageCompressor
    net = ImageCompressor(128).train()
    with pytest.raises(_lib.Iclr17Error, match="distortion"):
        net.forward_train(torch.rand(1, 3, 32, 32), distortion="psnr")
