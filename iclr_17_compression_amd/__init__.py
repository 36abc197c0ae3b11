"""iclr_17_compression_amd — MI355X-native (gfx950) Ballé-2017 codec hot path.

Drop-in for the reference's model.py / models/ surface (Yuval-H/iclr_17_compression):

    from iclr_17_compression_amd.model import ImageCompressor, save_model, load_model
    from iclr_17_compression_amd.models import GDN, BitEstimator, Analysis_net_17, Synthesis_net_17

All compute runs in libiclr17.so (hand-written HIP kernels, C ABI in include/iclr17.h).

The differentiable MS-SSIM / SSIM and the MS-SSIM training loss (losses.py):

    from iclr_17_compression_amd import ms_ssim_diff, ssim_diff, MSSSIMLoss
"""
__version__ = "0.1.0"

__all__ = ["ms_ssim_diff", "ssim_diff", "MSSSIMLoss"]


def __getattr__(name):
    # resolved on first use, so importing the package alone loads nothing more than before
    if name in __all__:
        from . import losses
        return getattr(losses, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
