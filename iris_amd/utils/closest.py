"""Closest point on the scene's mesh: the BVH the rays traverse, walked by a distance query (iris_amd/csrc/iris_closest.h; the contract: DESIGN.md
section 5c-17).  The reference has no counterpart: its materials are functions of the position alone.  Here it is what takes a position to the triangle and
barycentrics a texture lookup needs (model/texture.py)."""
import torch

from .. import _lib as L


def closest_point(scene, xs):
    """xs (B, 3) float32 on the scene's device -> (tri (B,) int64, bary (B, 2) float32, pos (B, 3) float32, dist2 (B,) float32).

    tri is the ORIGINAL face index of the closest triangle (a long triangle that the BVH holds through several presplit references reports its own index, and
    one answer).  bary = (b1, b2) as ray_intersect's uvs: pos = (1 - b1 - b2) p0 + b1 p1 + b2 p2, b1, b2 >= 0, b1 + b2 <= 1.  dist2 is the squared distance
    as the kernel computed it.  The closest point of a triangle is the vertex / edge / interior classification in float32; the winner is the lexicographic
    minimum of (dist2, original index); triangles whose float32 cross product is exactly zero are skipped, as no ray can hit them.  A mesh with no other
    triangle, and a query point that is not finite, give tri = -1, dist2 = +inf and zeros.  B = 0 launches nothing.  No backward pass: an input that
    requires grad raises."""
    L.no_autograd("closest_point", xs)
    xs = L.require_gpu(xs, torch.float32, "xs").detach().reshape(-1, 3)
    if L.device_index(xs.device) != L.device_index(scene.device):
        raise L.IrisError(f"closest_point: xs is on {xs.device}, the scene on {scene.device}")
    B, dev = xs.shape[0], xs.device
    tri = torch.empty(B, device=dev, dtype=torch.int64)
    bary = torch.empty(B, 2, device=dev, dtype=torch.float32)
    pos = torch.empty(B, 3, device=dev, dtype=torch.float32)
    dist2 = torch.empty(B, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        L.check(L.lib().iris_closest_point(scene.handle, L.ptr(xs), B, L.ptr(tri), L.ptr(bary), L.ptr(pos), L.ptr(dist2), L.stream()))
    return tri, bary, pos, dist2
