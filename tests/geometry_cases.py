"""Convolution geometries outside the set the shipped models use (kernel volume above 27, even kernels at stride 1, dilation,
strides that leave output rows without a pair, negative coordinates): the case table shared by tests/golden/make_golden.py
(`geometry` sub-command -> tests/golden/geometry_golden.npz, outputs of the reference) and the tests that read the fixture."""
import os

import numpy as np

# name, kernel_size, stride, tensor stride of the input level, dilation
CASES = [("k5s1", 5, 1, 1, 1), ("k4s1", 4, 1, 1, 1), ("k2s1", 2, 1, 1, 1), ("k3d2", 3, 1, 1, 2), ("k3d3", 3, 1, 1, 3),
         ("k323", (3, 2, 3), 1, 1, 1), ("k531", (5, 3, 1), 1, 1, 1),
         ("k4s2", 4, 2, 1, 1), ("k5s2", 5, 2, 1, 1), ("k3s3", 3, 3, 1, 1), ("k5s3", 5, 3, 1, 1), ("k3s212", 3, (2, 1, 2), 1, 1),
         ("k2s2_l2", 2, 2, 2, 1), ("k3s2_l2", 3, 2, 2, 1), ("k3d2_l2", 3, 1, 2, 2),
         ("k442", (4, 4, 2), 1, 1, 1), ("k553", (5, 5, 3), 1, 1, 1), ("k211", (2, 1, 1), 1, 1, 1)]
# the same on the scene shifted to negative coordinates (the fast spdownsample branch truncates toward zero, the general one
# compares with the coordinate minimum)
NEG_CASES = [("k2s2", 2, 2, 1, 1), ("k3s2", 3, 2, 1, 1), ("k4s2", 4, 2, 1, 1), ("k3s1", 3, 1, 1, 1), ("k5s1", 5, 1, 1, 1)]
# (case, transposed, cin, cout) of the stored ConvolutionFunction vectors conv_<case>_<N|T>_{x,w,y,gy,gx,gw}
CONV_CASES = [("k5s1", False, 8, 12), ("k4s2", False, 4, 4), ("k4s2", True, 4, 4), ("k3s3", False, 8, 12), ("k3s3", True, 12, 8),
              ("k2s1", False, 4, 8), ("k3d2", False, 4, 8)]

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tup3(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


def volume(ks):
    return int(np.prod(tup3(ks)))


def is_strided(stride):
    return any(s != 1 for s in tup3(stride))


def case(name, table=CASES):
    return next(c for c in table if c[0] == name)


def load():
    """(ops_golden.npz, geometry_golden.npz)"""
    return np.load(os.path.join(GOLDEN_DIR, "ops_golden.npz")), np.load(os.path.join(GOLDEN_DIR, "geometry_golden.npz"))


def input_coords(ops, tensor_stride):
    """Input level of a case: the golden scene, or its k2 s2 downsample for the cases at tensor stride 2."""
    return ops["scene_coords"] if tensor_stride == 1 else ops["ds_k2s2"]


def negative_scene(ops):
    """The golden scene shifted by -(max // 2) per spatial axis: about half of every axis is negative."""
    c = ops["scene_coords"].copy()
    c[:, :3] -= c[:, :3].max(axis=0, keepdims=True) // 2
    return c
