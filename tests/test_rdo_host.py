"""The host side of rate–distortion optimised quantisation, without a GPU: the
``rdo`` option's checks, what it selects, the budget rule driven with a stand-in coder, and the
entry points' argument checks."""
import ctypes
import re

import numpy as np
import pytest
import torch

from iclr_17_compression_amd import _lib, codec, kernels
from iclr_17_compression_amd.model import ImageCompressor

P16 = ctypes.c_void_p(16)   # a non-null pointer that no check dereferences
FP = 0x0123456789ABCDEF


# ------------------------------------------------------------------------------ the option
def test_rdo_value():
    for good in (0, 0.0, 0.25, 1, 16.0, np.float32(2.0), np.int64(3)):
        assert codec.rdo_value(good) == float(good)
    for bad in (True, False, np.bool_(True), "1", None, [1.0], 1j):
        with pytest.raises(_lib.Iclr17Error, match="rdo must be a real number"):
            codec.rdo_value(bad)
    for bad in (-1, -1e-30, float("nan"), float("inf"), -float("inf"), 1e39):
        with pytest.raises(_lib.Iclr17Error, match="rdo must be finite and >= 0"):
            codec.rdo_value(bad)


def test_rate_request_with_rdo():
    assert codec.rate_request(2) is None
    # alone: the unit step, as step_offsets alone
    assert codec.rate_request(2, rdo=1.0) == ("step", codec.UNIT_STEP)
    assert codec.rate_request(2, rdo=0) == ("step", codec.UNIT_STEP)
    assert codec.rate_request(2, step=3, rdo=0.5) == ("step", 3)
    assert codec.rate_request(2, max_bytes=500, rdo=0.5) == ("budget", [500, 500], False)
    assert codec.rate_request(2, bpp=[0.5, 1.0], rdo=2) == ("budget", [0.5, 1.0], True)
    off = [np.zeros((1, 2), np.int8)] * 2
    with pytest.raises(_lib.Iclr17Error, match="per-block rate–distortion optimised quantisation "
                                               "is not built"):
        codec.rate_request(2, step=3, step_offsets=off, rdo=1.0)
    for bad in (True, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.Iclr17Error, match="rdo must be"):
            codec.rate_request(2, step=3, rdo=bad)


def test_public_calls_check_rdo_before_any_device_use():
    net = ImageCompressor(128).eval()   # on the host: nothing below may reach a kernel
    img = np.zeros((49, 83, 3), np.uint8)
    off = [np.zeros((1, 2), np.int8)] * 2
    for kw, text in (({"rdo": True}, "rdo must be a real number"),
                     ({"rdo": -0.5}, "rdo must be finite and >= 0"),
                     ({"rdo": float("nan"), "step": 4}, "rdo must be finite and >= 0"),
                     ({"rdo": float("inf"), "max_bytes": 900}, "rdo must be finite and >= 0"),
                     ({"rdo": 1.0, "step_offsets": off}, "is not built"),
                     ({"rdo": 1.0, "step": 8, "bpp": 1.0}, "step and bpp given together"),
                     ({"rdo": 1.0, "step": 32}, "quantiser step index")):
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            net.compress_images([img, img], **kw)
        with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
            net.evaluate_images([img, img], **kw)
    y = torch.zeros(2, 4, 6, 128)
    with pytest.raises(_lib.Iclr17Error, match="is not built"):
        net.compress_latents(y, None, step_map=np.zeros((2, 1, 2), np.uint8), rdo=1.0)
    for bad, text in ((True, "real number"), (-1, "finite and >= 0")):
        with pytest.raises(_lib.Iclr17Error, match=text):
            net.compress_latents(y, 8, rdo=bad, rdo_weights=np.ones(128, np.float32))
        with pytest.raises(_lib.Iclr17Error, match=text):
            net.rate_sweep(y, latent=True, rdo=bad, rdo_weights=np.ones(128, np.float32))
    with pytest.raises(_lib.Iclr17Error, match=re.escape("rdo_weights must have shape [128]")):
        net.compress_latents(y, 8, rdo=1.0, rdo_weights=np.ones(127, np.float32))


# ------------------------------------------------------------------------------ budget rule
def test_budget_loop_with_rdo_estimates():
    """compress_images' budget path with ``rdo``, the coder a stand-in: choose_step and
    encode_to_budget as they are, driven by the optimised levels' (smaller) estimates; the blobs
    are ordinary I17Q ones."""
    overhead = codec.blob_overhead(1)
    calls = []

    def words(k, s, rdo):   # bytes of rANS words of image k at index s: fewer with rdo
        return (3000, 2000)[k] - 60 * s - (90 if rdo else 0)

    def encode(ks, s):
        calls.append((tuple(ks), s))
        return [codec.pack_step_header(1, 128, 32, s, 100, 100, FP) + bytes(4 + 256 + words(k, s, True))
                for k in ks]

    est = {rdo: [[8.0 * (words(k, s, rdo) - 70) for s in range(32)] for k in range(2)]
           for rdo in (False, True)}                                    # 70 bytes too low
    budgets = [2380, 1500]
    plain = [codec.choose_step(est[False][k], budgets[k], overhead) for k in range(2)]
    chosen = [codec.choose_step(est[True][k], budgets[k], overhead) for k in range(2)]
    # estimate + overhead is 3218 − 60·s (3128 − 60·s with rdo) for image 0, 1000 less for image 1
    assert overhead == 288 and plain == [14, 12] and chosen == [13, 11]
    blobs, again = codec.encode_to_budget(chosen, budgets, encode, ["image 0", "image 1"])
    # the blobs are 3198 − 60·s and 2198 − 60·s bytes: the estimate's index is 38 bytes over, the
    # next fits
    assert again == [1, 1] and [len(b) for b in blobs] == [2358, 1478]
    assert calls == [((0,), 13), ((1,), 11), ((0,), 14), ((1,), 12)]
    for k, blob in enumerate(blobs):
        assert blob[:4] == codec.STEP_MAGIC and len(blob) <= budgets[k]
        head, step = codec.parse_blob(blob)
        assert step == (14, 12)[k] and head.N == 128
    with pytest.raises(_lib.Iclr17Error, match=re.escape(
            "image 1 does not fit its budget of 300 bytes: the coarsest step gives 338")):
        codec.encode_to_budget([30, 30], [10 ** 6, 300], encode, ["image 0", "image 1"])


# ------------------------------------------------------------------------------ entry points
def rejects(text, name, *args):
    with pytest.raises(_lib.Iclr17Error, match=re.escape(text)):
        _lib.call(name, *args)
    assert text in _lib.last_error()


def steps_arg(*values):
    return ctypes.cast((ctypes.c_float * len(values))(*values), ctypes.c_void_p)


def test_entry_points_validate_without_gpu():
    # every check below fires on the host before a kernel could be launched
    def quant(y=P16, B=2, h=4, w=6, N=128, rp=P16, step=1.0, lam=P16, y_hat=P16, y_deq=P16,
              partial=P16, bits=P16, status=P16):
        return ["iclr17_quantise_rdo", y, B, h, w, N, rp, ctypes.c_float(step), lam, y_hat, y_deq,
                partial, bits, status, None]

    def sweep(y=P16, B=2, h=4, w=6, N=128, rp=P16, st=(1.0, 2.0), S=2, lam=P16, partial=P16,
              bits=P16):
        return ["iclr17_rate_sweep_rdo", y, B, h, w, N, rp, None if st is None else steps_arg(*st),
                S, lam, partial, bits, None]

    for what, entry, ptrs in (
            ("quantise_rdo", quant, ("y", "rp", "lam", "y_hat", "y_deq", "partial", "bits", "status")),
            ("rate_sweep_rdo", sweep, ("y", "rp", "st", "lam", "partial", "bits"))):
        for p in ptrs:
            rejects(f"{what}: null pointer", *entry(**{p: None}))
        rejects(f"{what}: bad shape B=0 h=4 w=6 N=128", *entry(B=0))
        rejects(f"{what}: bad shape B=2 h=-1 w=6 N=128", *entry(h=-1))
        rejects(f"{what}: bad shape B=2 h=4 w=0 N=128", *entry(w=0))
        rejects(f"{what}: bad shape B=2 h=4 w=6 N=0", *entry(N=0))
        rejects(f"{what}: N=4096", *entry(N=4096))
        assert "of LDS" in _lib.last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rejects("quantise_rdo: the step ", *quant(step=bad))
        assert "is not finite and positive" in _lib.last_error()
        rejects("rate_sweep_rdo: step 1 (", *sweep(st=(1.0, bad)))
        assert "is not finite and positive" in _lib.last_error()
    rejects("rate_sweep_rdo: S=0 steps (1..32)", *sweep(S=0))
    rejects("rate_sweep_rdo: S=33 steps (1..32)", *sweep(st=(1.0,) * 33, S=33))
    # the codec's own shapes fit: all 32 steps at N = 192 (and the partial counts are rate_sweep's)
    for h, w, N in ((4, 6, 128), (4, 6, 192), (1, 1, 192), (32, 48, 192)):
        assert (_lib.query("iclr17_rate_sweep_rdo_partials", h, w, N)
                == _lib.query("iclr17_rate_sweep_partials", h, w, N) == -(-h * w * N // 4096))


def test_wrapper_checks_precede_any_device_use():
    y = torch.zeros(2, 4, 6, 128)   # host tensors: never uploaded
    rp = torch.zeros(11 * 128)
    lam = torch.ones(128)
    for fn in (lambda: kernels.quantise_rdo(y, rp, 1.0, lam),
               lambda: kernels.rate_sweep_rdo(y, rp, [1.0, 2.0], lam)):
        with pytest.raises(_lib.Iclr17Error, match="ROCm GPU"):
            fn()
