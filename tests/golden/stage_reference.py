"""Where the reference's Python sources are read from, for the tests and make_golden.py that import them.

They are read in place, never copied into this repository: the tests that import the reference's segmentors skip where its tree
is absent. Nothing under openpcseg_amd/ reads the reference.
"""
import os

REF = "/root/reference"


def reference_root():
    """Where the reference's Python sources can be imported from, or None where its tree is absent."""
    return REF if os.path.isdir(os.path.join(REF, "pcseg")) else None


TS_ZIP = os.path.join(REF, "package", "torchsparse.zip")
TS_FUNCTIONAL = ["hash", "query", "count", "voxelize", "devoxelize", "conv"]   # TS:torchsparse/nn/functional/<name>.py


def functional_source(name):
    """Source text of the reference's torchsparse/nn/functional/<name>.py, read from the reference's zip; None where it is absent."""
    if not os.path.isfile(TS_ZIP):
        return None
    import zipfile
    with zipfile.ZipFile(TS_ZIP) as z:
        return z.read("torchsparse/torchsparse/nn/functional/%s.py" % name).decode()
