"""MI355X-native Gaussian-Shading watermark hot path (embed / DDIM step / extract) behind the reference's own
Python interface.  The directory name is fixed by the build contract and is not an importable identifier; import it
through the `gswm_amd` loader module at the repo root:

    import gswm_amd
    from gswm_amd import gs_insert, extract          # drop-in twins of the reference's modules
    from gswm_amd import codec                        # batch-first device API over the C ABI (include/gswm.h)
    from gswm_amd import trace                        # registry of issued messages: which user made this image, and how sure
    from gswm_amd import tamper                       # which tiles of an image still carry the watermark; the tile-weighted vote
    from gswm_amd import soft                         # the soft-decision vote: every element weighted by its reliability level
    from gswm_amd import detect                       # a keyring instead of a registry: which key is this image under, and what does it say
    from gswm_amd import align                        # the same through flips, quarter turns and lattice shifts of the image
    from gswm_amd import ecc                          # error-corrected payloads: a convolutional code under the votes, read by one Viterbi launch
"""
from . import _native  # noqa: F401
from . import codec  # noqa: F401

__all__ = ["codec", "gs_insert", "extract", "comfy", "ddim", "dist", "distortions", "trace", "tamper", "soft", "detect", "align", "ecc"]


def __getattr__(name):  # lazy sub-modules (keep `import gswm_amd` light)
    if name in __all__:
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError(name)
