"""Formula-built triangle meshes for the STL-correction tests and scripts/stlcorr_probe.py (no mesh library needed)."""
import math

import numpy as np


def tube_triangles(centre, axis, half_len, radius, sections, rings, phase=0.0):
    """(2 * sections * rings, 3, 3) vertices: the side of a cylinder about `axis` through `centre`, `sections` x `rings`
    quads split in two, outward winding."""
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    a = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(u, a)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    th = phase + 2.0 * math.pi * np.arange(sections + 1) / sections
    circle = radius * (np.cos(th)[:, None] * e1 + np.sin(th)[:, None] * e2)                  # (sections + 1, 3)
    t = (2.0 * np.arange(rings + 1) / rings - 1.0) * half_len
    p = np.asarray(centre, dtype=np.float64) + t[:, None, None] * u + circle[None, :, :]   # (rings + 1, sections + 1, 3)
    lo0, lo1, hi0, hi1 = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    tri = np.stack([np.stack([lo0, lo1, hi1], axis=2), np.stack([lo0, hi1, hi0], axis=2)], axis=2)
    return np.ascontiguousarray(tri.reshape(-1, 3, 3))


def subdivisions(triangles, dx, max_subdiv):
    """n per triangle as voxel_bc_correction.py:70-77 takes it"""
    span = np.max((triangles.max(axis=1) - triangles.min(axis=1)) / dx, axis=1)
    n = np.where(span > 1.0, np.ceil(span), 1.0)
    return np.clip(n, 1, max_subdiv).astype(np.int64)
