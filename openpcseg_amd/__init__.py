"""openpcseg_amd -- MI355X (gfx950) native sparse-voxel hot path behind the torchsparse 1.4
operator API that PJLab-ADG/OpenPCSeg's segmentors call.

    import openpcseg_amd
    openpcseg_amd.install_as_torchsparse()   # `import torchsparse` now resolves to this package
    openpcseg_amd.fuse(model)                # optional: block fusion for the reference's unmodified segmentors (block_fusion.py)
    openpcseg_amd.freeze(model)              # optional: inference mode, BatchNorm folded into the convolutions (inference.py)
"""
from .sparse import SparseTensor, PointTensor, cat, fapply, get_kernel_offsets, make_ntuple  # noqa: F401
from .compat import install_as_torchsparse, install_reference_aliases  # noqa: F401
from . import optim  # noqa: F401  (FusedSGD, LossScaler: the training-step tail on the device)


def fuse(model, criterion=True, glue=True, forward=True):
    """Block fusion for an unmodified reference segmentor (openpcseg_amd/block_fusion.py)."""
    from .block_fusion import fuse as _fuse
    return _fuse(model, criterion=criterion, glue=glue, forward=forward)


def unfuse(model):
    from .block_fusion import unfuse as _unfuse
    return _unfuse(model)


def freeze(model):
    """Inference mode: fold every BatchNorm of the package's blocks into its convolution (openpcseg_amd/inference.py)."""
    from .inference import freeze as _freeze
    return _freeze(model)


def unfreeze(model):
    from .inference import unfreeze as _unfreeze
    return _unfreeze(model)


__version__ = "0.1.0"
