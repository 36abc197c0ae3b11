"""Factorised entropy model — surface of the reference models/bitEstimator.py:6-42.

``Bitparm`` / ``BitEstimator`` keep the reference parameters (h, b, a of shape (1, C, 1, 1);
the final layer has no ``a``) and init; forwards run gfx950 elementwise kernels.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import kernels
from ..packcache import PackCache


class Bitparm(nn.Module):
    def __init__(self, channel, final=False):
        super().__init__()
        self.final = final
        self.h = nn.Parameter(torch.nn.init.normal_(torch.empty(channel).view(1, -1, 1, 1), 0, 0.01))
        self.b = nn.Parameter(torch.nn.init.normal_(torch.empty(channel).view(1, -1, 1, 1), 0, 0.01))
        if not final:
            self.a = nn.Parameter(torch.nn.init.normal_(torch.empty(channel).view(1, -1, 1, 1), 0, 0.01))
        else:
            self.a = None

    def forward(self, x):
        # bitEstimator.py:20-25
        from ..autograd import BitparmFn, needs_grad
        ps = [p for p in (self.h, self.b, self.a) if p is not None]
        if needs_grad(x, ps):
            return BitparmFn.apply(x, self, *ps)
        return kernels.bitparm(x, self.h, self.b, self.a)


class BitEstimator(nn.Module):
    def __init__(self, channel):
        super().__init__()
        self.f1 = Bitparm(channel)
        self.f2 = Bitparm(channel)
        self.f3 = Bitparm(channel)
        self.f4 = Bitparm(channel, True)
        self.channel = channel
        self._pack = PackCache()

    def params_in_order(self):
        return [self.f1.h, self.f1.b, self.f1.a, self.f2.h, self.f2.b, self.f2.a,
                self.f3.h, self.f3.b, self.f3.a, self.f4.h, self.f4.b]

    def packed(self, force: bool = False):
        """Per-channel table [11][C]: softplus(h_k), b_k, tanh(a_k) (k=1..3), softplus(h4), b4."""
        ps = self.params_in_order()
        return self._pack.get("rate", ps, lambda: kernels.pack_rate(ps), force=force)

    def rate_table(self, force: bool = False):
        """element_bits for the integer latents −32..32 per channel ([C, 65]; the round-mode
        quantiser epilogue looks them up), cached like the packed parameters."""
        ps = self.params_in_order()
        return self._pack.get("rtab", ps, lambda: kernels.rate_table(self.packed(force), self.channel),
                              force=force)

    def step_packed(self, step: int):
        """The packed table of ladder step ``step`` (codec.step_size): row 0 · Δ, made on the
        device from ``packed()`` and cached like it."""
        from ..codec import step_size
        d = step_size(step)
        ps = self.params_in_order()
        return self._pack.get(f"rate_s{step}", ps,
                              lambda: kernels.pack_rate_step(self.packed(), self.channel, d))

    def entropy_tables(self, K: int = kernels.ENTROPY_K, step: Optional[int] = None):
        """Quantised CDFs for the entropy coder (cached like the packed parameters); with
        ``step`` those of ŷ = rint(y/Δ_step), from ``step_packed(step)``."""
        ps = self.params_in_order()
        if step is not None:
            return self._pack.get(
                f"cdf{K}_s{step}", ps,
                lambda: kernels.entropy_tables(self.step_packed(step), self.channel, K))
        return self._pack.get(f"cdf{K}", ps,
                              lambda: kernels.entropy_tables(self.packed(), self.channel, K),
                              )

    def stacked_tables(self, K: int, steps):
        """``entropy_tables(K, step=s)`` of the ladder steps ``steps`` (ascending, distinct)
        stacked as int32 [S, C, 2K + 3] for the mapped entropy coder. The last stack is kept (one
        per K, not one per set of steps: a stack is up to 32 table sets), so a run of calls with
        the same steps stacks once."""
        ps = self.params_in_order()
        steps = tuple(int(s) for s in steps)

        def build():
            return steps, torch.stack([self.entropy_tables(K, step=s) for s in steps])

        kept = self._pack.get(f"cdf{K}_map", ps, build)
        if kept[0] != steps:
            kept = self._pack.get(f"cdf{K}_map", ps, build, force=True)
        return kept[1]

    def recon_offsets(self, K: int, step: int, mode: str, strength: float = 1.0):
        """The reconstruction offsets of ladder step ``step`` (kernels.recon_offsets: fp32
        [C, 2K + 1], ``mode`` "centroid" or "zero"), cached like ``entropy_tables``."""
        from ..codec import step_size
        ps = self.params_in_order()
        return self._pack.get(
            f"recon{K}_s{step}_{mode}_{float(strength)!r}", ps,
            lambda: kernels.recon_offsets(self.packed(), self.channel, K, [step_size(step)], mode,
                                          strength)[0])

    def stacked_recon_offsets(self, K: int, steps, mode: str, strength: float = 1.0):
        """``recon_offsets`` of the ladder steps ``steps`` (ascending, distinct) as fp32
        [S, C, 2K + 1], from one launch, for the mapped dequantiser. The last stack is kept, as
        ``stacked_tables`` keeps its."""
        from ..codec import step_size
        ps = self.params_in_order()
        want = (tuple(int(s) for s in steps), mode, float(strength))

        def build():
            return want, kernels.recon_offsets(self.packed(), self.channel, K,
                                               [step_size(s) for s in want[0]], mode, strength)

        kept = self._pack.get(f"recon{K}_map", ps, build)
        if kept[0] != want:
            kept = self._pack.get(f"recon{K}_map", ps, build, force=True)
        return kept[1]

    def forward(self, x):
        # bitEstimator.py:38-42
        from ..autograd import BitEstimatorFn, needs_grad
        if needs_grad(x, self.params_in_order()):
            return BitEstimatorFn.apply(x, self, *self.params_in_order())
        return kernels.bit_estimator(x, self.packed(), self.channel)
