"""Exact restatement of the mapper's global-point rule (no GPU, no BLAS).

csrc/grid_kernels.hip rounds a global point as the reference's per-point
``3x3 @ 3x1`` NumPy product rounds it on the fixtures' build host:

    gx = fma(c, x, -s * y) + px        gy = fma(s, x, c * y) + py

with c, s = np.cos / np.sin of the heading.  ``global_points_exact`` spells the
fused multiply-add with rational arithmetic (one rounding of c x + t, t the
already rounded second product), so it gives the same doubles on every host,
whatever its NumPy or BLAS build.
"""
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    """round(a b + c) with a single rounding (float(Fraction) rounds to nearest even)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def global_points_exact(poses, scans):
    """List of (m_i, 2) float64, one per scan."""
    out = []
    for pose, pts in zip(np.asarray(poses, dtype=np.float64), scans):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
        c, s = float(np.cos(pose[2])), float(np.sin(pose[2]))
        px, py = float(pose[0]), float(pose[1])
        g = np.zeros(pts.shape)
        for j, (x, y) in enumerate(pts.tolist()):
            g[j, 0] = fma(c, x, -s * y) + px
            g[j, 1] = fma(s, x, c * y) + py
        out.append(g)
    return out


def global_points_rational(poses, scans):
    """The same points with NO rounding at all, as Fractions: [(gx, gy), ...]
    per scan.  Only meaningful where cos and sin are exact (heading 0)."""
    out = []
    for pose, pts in zip(np.asarray(poses, dtype=np.float64), scans):
        c, s = Fraction(float(np.cos(pose[2]))), Fraction(float(np.sin(pose[2])))
        px, py = Fraction(float(pose[0])), Fraction(float(pose[1]))
        out.append([(c * Fraction(x) - s * Fraction(y) + px, s * Fraction(x) + c * Fraction(y) + py)
                    for x, y in np.asarray(pts, dtype=np.float64).reshape(-1, 2).tolist()])
    return out
