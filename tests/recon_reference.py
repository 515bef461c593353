"""Plain float64 NumPy for the three passes of the ReconBlock gate (include/pcseg_hip.h, the pcs_recon_gate_* section;
R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:337-384).

a3 = the three conv outputs (n, c); stat3 = 3 x (mean | invstd), 6c; gamma3 / beta3 = 3 x c or None:

    forward    out = x * ((s0 + s1) + s2),  s_k = 1 / (1 + exp(-bn_k(a_k))),  bn_k(a) = (a - mean_k) * invstd_k * gamma_k + beta_k
    bwd_stats  g_k = dy * x * s_k * (1 - s_k);  sums2 = 3 x [sum g_k | sum g_k * xhat_k],  xhat_k = (a_k - mean_k) * invstd_k
    bwd_apply  dx_gate = dy * ((s0 + s1) + s2);  da_k = (g_k - S_k0 / count - xhat_k * S_k1 / count) * invstd_k * gamma_k
"""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def terms(a3, stat3, gamma3=None, beta3=None):
    """-> per branch (s_k, xhat_k, invstd_k * gamma_k)."""
    stat3, gamma3, beta3 = _f64(stat3), _f64(gamma3), _f64(beta3)
    c = np.asarray(a3[0]).shape[1]
    out = []
    for k, a in enumerate(a3):
        a = _f64(a)
        mean, invstd = stat3[2 * k * c:(2 * k + 1) * c], stat3[(2 * k + 1) * c:(2 * k + 2) * c]
        sc = invstd * (gamma3[k * c:(k + 1) * c] if gamma3 is not None else 1.0)
        xhat = (a - mean) * invstd
        t = (a - mean) * sc + (beta3[k * c:(k + 1) * c] if beta3 is not None else 0.0)
        out.append((1.0 / (1.0 + np.exp(-t)), xhat, sc))
    return out


def forward(a3, x, stat3, gamma3=None, beta3=None):
    (s0, _, _), (s1, _, _), (s2, _, _) = terms(a3, stat3, gamma3, beta3)
    return _f64(x) * ((s0 + s1) + s2)


def grads_of_gates(dy, x, a3, stat3, gamma3=None, beta3=None):
    """-> [g_0, g_1, g_2]."""
    p = _f64(dy) * _f64(x)
    return [p * s * (1.0 - s) for s, _, _ in terms(a3, stat3, gamma3, beta3)]


def bwd_stats(dy, x, a3, stat3, gamma3=None, beta3=None):
    parts = []
    for g, (_, xhat, _) in zip(grads_of_gates(dy, x, a3, stat3, gamma3, beta3), terms(a3, stat3, gamma3, beta3)):
        parts += [g.sum(0), (g * xhat).sum(0)]
    return np.concatenate(parts)


def bwd_apply(dy, x, a3, stat3, gamma3, beta3, sums2, count):
    """-> (dx_gate, [da_0, da_1, da_2])."""
    s2 = _f64(sums2)
    c = np.asarray(x).shape[1]
    count = float(count) if count > 0 else 1.0
    tr = terms(a3, stat3, gamma3, beta3)
    da = []
    for k, (g, (_, xhat, sc)) in enumerate(zip(grads_of_gates(dy, x, a3, stat3, gamma3, beta3), tr)):
        da.append((g - s2[2 * k * c:(2 * k + 1) * c] / count - xhat * (s2[(2 * k + 1) * c:(2 * k + 2) * c] / count)) * sc)
    return _f64(dy) * ((tr[0][0] + tr[1][0]) + tr[2][0]), da
