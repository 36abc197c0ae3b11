"""Differentiable MS-SSIM / SSIM on the GPU kernels, and MS-SSIM as a training loss.

The reference's models/ms_ssim_torch.py is plain torch and so differentiable; its ``MS_SSIM``
exists to be used as a loss. The reference-named evaluation entry points (``models.ms_ssim``,
``models.ssim``, ``MS_SSIM``) stay evaluation-only here and refuse inputs that require grad;
these are the differentiable ones:

* ``ms_ssim_diff(X, Y, data_range=1.0, size_average=True)``
* ``ssim_diff(X, Y, data_range=1.0, size_average=True, full=False)``
* ``MSSSIMLoss(data_range=1.0)``: ``1 − mean MS-SSIM``

Values are bitwise those of ``kernels.ms_ssim`` / ``kernels.ssim``; the backward runs in
``csrc/msssim.hip`` (autograd.MsSsimFn / SsimFn), with fixed-order sums, so gradients are bitwise
reproducible. The default window (11 taps, σ = 1.5) and the 5 default level weights only. Inputs
are CUDA float32 [B,3,H,W] tensors on one device: a differentiable function does not move
tensors between devices, so CPU tensors raise ``Iclr17Error``.

As in the reference, nothing is clamped: an image pair whose mean cs of some level (or ssim of the
last) is ≤ 0 has a NaN MS-SSIM and NaN gradients. Pairs of an image and its reconstruction are far
from that; independent random images are not.
"""
from __future__ import annotations

import torch

from . import kernels
from ._lib import Iclr17Error
from .autograd import MsSsimFn, SsimFn

__all__ = ["ms_ssim_diff", "ssim_diff", "MSSSIMLoss"]


def _check(X, Y, what):
    """ms_ssim_torch.py:102-112 / :140-150 in the reference's order, then device and dtype."""
    if not (isinstance(X, torch.Tensor) and isinstance(Y, torch.Tensor)):
        raise Iclr17Error(f"iclr17: {what} takes two torch.Tensors")
    if len(X.shape) != 4:
        raise ValueError('Input images must 4-d tensor.')
    if not X.type() == Y.type():
        raise ValueError('Input images must have the same dtype.')
    if not X.shape == Y.shape:
        raise ValueError('Input images must have the same dimensions.')
    if not X.is_cuda or X.device != Y.device:
        raise Iclr17Error(f"iclr17: {what} takes CUDA tensors on one device (got {X.device} and "
                          f"{Y.device}); it runs only on a ROCm GPU (MI355X / gfx950) and does not "
                          "move its inputs")
    if X.dtype != torch.float32:
        raise Iclr17Error(f"iclr17: {what} takes float32 images (got {X.dtype})")


def _needs_grad(X, Y):
    return torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad)


def ms_ssim_diff(X, Y, data_range=1.0, size_average=True):
    """MS-SSIM of [B,3,H,W] image batches (ms_ssim_torch.py:123-196), differentiable in X and Y:
    the batch mean (0-dim) with ``size_average``, else per image [B]."""
    _check(X, Y, "ms_ssim_diff")
    if _needs_grad(X, Y):
        v = MsSsimFn.apply(X, Y, float(data_range))
    else:
        v = kernels.ms_ssim(X.contiguous(), Y.contiguous(), float(data_range))
    return v.mean() if size_average else v


def ssim_diff(X, Y, data_range=1.0, size_average=True, full=False):
    """Single-scale SSIM (ms_ssim_torch.py:86-120), differentiable in X and Y; with ``full`` also
    the cs means, differentiable too."""
    _check(X, Y, "ssim_diff")
    if _needs_grad(X, Y):
        s, cs = SsimFn.apply(X, Y, float(data_range))
    else:
        s, cs = kernels.ssim(X.contiguous(), Y.contiguous(), float(data_range))
    if size_average:
        s, cs = s.mean(), cs.mean()
    return (s, cs) if full else s


class MSSSIMLoss(torch.nn.Module):
    """``1 − mean MS-SSIM(X, Y)``: the distortion term of λ·(1 − MS-SSIM) + bpp."""

    def __init__(self, data_range=1.0):
        super().__init__()
        self.data_range = data_range

    def forward(self, X, Y):
        return 1 - ms_ssim_diff(X, Y, data_range=self.data_range, size_average=True)
