"""volsurfs_amd — MI355X-native (gfx950) K-shell layered-mesh render hot path.

Host-side mirror of the reference's operator surface for the hot path named in
BASELINE.json; all compute is in libvolsurfs_hip.so (hand-written
HIP, C-ABI in include/volsurfs_hip.h).  There is no CPU fallback.
"""
from . import _lib  # noqa: F401

_MESH_SMOOTH = ("smooth_mesh", "smooth_shells", "smooth_meshes", "SmoothReport")

__all__ = ["_lib", *_MESH_SMOOTH]


def __getattr__(name):
    """The smoothing stage's names, imported on first use: importing the package alone still loads neither torch nor
    the library."""
    if name in _MESH_SMOOTH:
        from . import mesh_smooth
        return getattr(mesh_smooth, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
