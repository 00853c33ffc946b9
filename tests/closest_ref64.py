"""Brute-force float64 distance from points to a triangle mesh (no project import): what tests/test_closest_point.py holds closest_point to.

The distance to a triangle is written differently from the kernel's region classification: the point is projected onto the triangle's plane and, where the
projection lies inside (three signed areas against the normal), the distance is the plane's; otherwise it is the smallest of the distances to the three edge
segments.  Faces whose float64 cross product is exactly zero are skipped, as the contract skips them (their distance is +inf)."""
import numpy as np


def _segment_d2(p, a, b):
    ab, ap = b - a, p - a
    den = (ab * ab).sum(-1)
    t = np.clip((ap * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
    d = ap - t[..., None] * ab
    return (d * d).sum(-1)


def face_distances(verts, faces, pts):
    """(B, F) float64 distances of every point to every face; +inf for a zero-area face"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    p = np.asarray(pts, np.float64)[:, None, :]
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    ap = p - a
    with np.errstate(over="ignore", invalid="ignore"):
        wb = (np.cross(ap, c - a) * n).sum(-1) / nn1          # weight of vertex 1
        wc = (np.cross(b - a, ap) * n).sum(-1) / nn1          # weight of vertex 2
        inside = (wb >= 0) & (wc >= 0) & (wb + wc <= 1)
        plane = (ap * n).sum(-1) ** 2 / nn1
        edges = np.minimum(np.minimum(_segment_d2(p, a, b), _segment_d2(p, b, c)), _segment_d2(p, c, a))
        d2 = np.where(inside, np.minimum(plane, edges), edges)
    return np.where(ok, np.sqrt(d2), np.inf)


def closest_ref(verts, faces, pts, slack, chunk=256):
    """-> dict: 'dist' (B,) the distance to the mesh, 'argmin' (B,) the face that attains it (the lowest index among exact ties), 'near' (B, F) bool: the faces
    within `slack` of the minimum, 'runner_up' (B,) the smallest distance among the OTHER faces (+inf for a mesh of one face)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    B, F = pts.shape[0], np.asarray(faces).shape[0]
    out = {"dist": np.empty(B), "argmin": np.empty(B, np.int64), "near": np.empty((B, F), bool), "runner_up": np.empty(B)}
    for s in range(0, B, chunk):
        d = face_distances(verts, faces, pts[s:s + chunk])
        k = d.argmin(1)
        best = d[np.arange(d.shape[0]), k]
        out["dist"][s:s + chunk], out["argmin"][s:s + chunk] = best, k
        out["near"][s:s + chunk] = d <= best[:, None] + slack
        d[np.arange(d.shape[0]), k] = np.inf
        out["runner_up"][s:s + chunk] = d.min(1)
    return out


def rebuild(verts, faces, tri, bary):
    """the point (1 - b1 - b2) p0 + b1 p1 + b2 p2 in float64"""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    t, b = np.asarray(tri, np.int64), np.asarray(bary, np.float64)
    p0, p1, p2 = v[f[t, 0]], v[f[t, 1]], v[f[t, 2]]
    return (1.0 - b[:, :1] - b[:, 1:]) * p0 + b[:, :1] * p1 + b[:, 1:] * p2
