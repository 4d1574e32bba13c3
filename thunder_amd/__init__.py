"""thunder_amd -- MI355X (gfx950) particle-filter expectation / Fourier-insert engine.

Drop-in for THUNDER's GPU plugin surface (gpu/interface/Interface.h): the
kernels live in libthunder_amd.so behind the C-ABI of include/thunder_amd.h;
this package is the thin torch/ctypes front end used by the tests and bench.
"""
from ._lib import ThxError, lib  # noqa: F401
from .build import LIB as LIBRARY_PATH  # noqa: F401

__all__ = ["lib", "ThxError", "LIBRARY_PATH", "average_halves", "refresh_projectee"]


def __getattr__(name):
    # the torch front end of the round's last stage, imported on first use
    if name in ("average_halves", "refresh_projectee"):
        from . import reference
        return getattr(reference, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
