"""closest_point on the GPU (iris_amd/csrc/iris_closest.h, iris_amd/utils/closest.py) against the brute-force float64 distances of tests/closest_ref64.py.

Tolerance, derived and not measured: S = the largest absolute coordinate among the mesh's vertices and the call's query points, eps = 64 * 2^-24 * S (the
operation count of the float32 closest-point arithmetic).  Every case prints its largest distance error in units of 2^-24 S next to the 64 it is allowed.

Per case: |sqrt(dist2) - d_ref| <= eps; the point rebuilt in float64 from (tri, bary) within eps of pos and within d_ref + eps of the query; barycentrics in
range; tri among the reference's faces within 2 eps of the minimum (a zero-area face is never among them: its reference distance is +inf); where the
reference's runner-up is more than 2 eps behind, tri IS the reference's argmin; two calls give the same bits.

The last check must not be vacuous.  For the sets drawn inside the bounding box and ON the surface the test asserts, from the reference alone, that at least 90 %
of the points qualify.  Where it cannot hold the INPUT says why:
  * vertices, edge midpoints and the icosphere's centre are ties by construction: set check only;
  * a point OUTSIDE a closed convex mesh lies, with a probability that grows with its distance, in the region of an edge or a vertex, where the faces that share
    it tie exactly: the sets "up to ten extents outside" are held to the set check, and to the argmin wherever the reference separates the faces;
  * for the same reason the icosphere's inside-the-box set keeps the draws inside the sphere (the box's corners are outside the mesh: 15 % of a plain draw ties);
  * the icosphere translated by 1000 has eps = 3.8e-3, a fortieth of an edge: its inside-the-box set is drawn within 0.05 below the faces' centroids and its
    on-surface rays are aimed near them, where the runner-up is an inradius (0.04) away;
  * the two domino scenes span 10 and 40 decades (S = 3.6e10 and 2.1e31): every face lies within eps of every point at their low end, where the stack is deepest.
    They are run for the traversal (no fault, the spill part of the stack, one answer) and are ALSO held to a one-sided bound that is not vacuous there:
    sqrt(dist2) <= d_ref + 64 * 2^-24 * max(|query|, |vertices of the reference's face|, d_ref), which the nearest face's own float32 evaluation meets unless
    the traversal pruned it."""
import functools

import numpy as np
import pytest
import torch

import closest_ref64 as C
import deep_scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _cube(lo=0.0, hi=1.0):
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts float32 (V, 3), faces int32 (F, 3), number of REAL faces)"""
    from iris_amd.utils.lights import icosphere
    if name == "one":
        return np.array([[0.25, -0.5, 0.125], [1.5, 0.25, 0.0], [0.0, 1.0, 0.75]], np.float32), np.array([[0, 1, 2]], np.int32), 1
    if name == "cube":
        return (*_cube(), 12)
    if name in ("ico", "ico_far", "ico_degenerate"):
        v, f = icosphere(3)
        v, f = v.astype(np.float32), np.asarray(f, np.int32)
        if name == "ico_far":
            v = (v.astype(np.float64) + 1000.0).astype(np.float32)
        if name == "ico_degenerate":                                   # eight zero-area faces at radius 1.5, coordinates in eighths: every cross product is exactly 0
            a = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * np.float32(0.875)
            b, m = a + np.float32([0.25, 0, 0]), a + np.float32([0.125, 0, 0])
            n0 = len(v)
            v = np.concatenate([v, a, b, m])
            ia, ib, im = n0 + np.arange(8), n0 + 8 + np.arange(8), n0 + 16 + np.arange(8)
            deg = np.stack([ia, np.where(np.arange(8) % 3 == 0, ia, np.where(np.arange(8) % 3 == 1, ib, im)), np.where(np.arange(8) % 3 == 0, ia, ib)], 1)
            deg[1] = (ia[1], ib[1], ib[1]); deg[2] = (ia[2], im[2], ib[2])          # (a, b, b) and three collinear points; deg[0] is a single point, thrice
            return v, np.concatenate([f, deg.astype(np.int32)]), len(f)
        return v, f, len(f)
    if name == "cube_long":                                            # the cube and, as face 12, one triangle 100 units long: the presplit makes several references of it
        v, f = _cube()
        v = np.concatenate([v, np.float32([[-50, 3, 0.2], [50, 3, 0.2], [0, 3, 1.2]])])
        return v, np.concatenate([f, np.int32([[8, 9, 10]])]), 13
    v, f = deep_scenes.scene(name)
    return v, f, len(f)


@functools.lru_cache(maxsize=None)
def scene(name):
    from iris_amd.utils.path_tracing import Scene
    v, f, _ = mesh(name)
    return Scene(v, f, device=torch.device(DEV))


def _edges(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(np.sort(e, 1), axis=0)


def _surface(name, n, rng, aim=None):
    """positions returned by ray_intersect: rays from half a unit above random points of random faces, aimed at them"""
    from iris_amd.utils.path_tracing import ray_intersect
    v, f, real = mesh(name)
    face = rng.integers(0, real, n)
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    if aim is not None:                                              # near the centroid: (1/3, 1/3) +- aim
        b = 1.0 / 3.0 + (rng.random((n, 2)) - 0.5) * 2 * aim
    p0, p1, p2 = (v[f[face, k]].astype(np.float64) for k in range(3))
    target = (1 - b.sum(1, keepdims=True)) * p0 + b[:, :1] * p1 + b[:, 1:] * p2
    nrm = np.cross(p1 - p0, p2 - p0)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o = torch.from_numpy((target + 0.5 * nrm).astype(np.float32)).to(DEV)
    d = torch.from_numpy(np.ascontiguousarray(-nrm, np.float32)).to(DEV)
    pos, _, _, _, valid = ray_intersect(scene(name), o, d)
    assert int(valid.sum()) == n
    return pos.cpu().numpy()


@functools.lru_cache(maxsize=None)
def points(name, kind, n):
    v, f, real = mesh(name)
    rng = np.random.default_rng([ord(c) for c in name + "/" + kind] + [n])
    lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
    ext = (hi - lo).max()
    if kind == "box":
        if name == "ico_far":                                        # within 0.05 below the faces, near their centroids (see the module docstring)
            face = rng.integers(0, real, n)
            p0, p1, p2 = (v[f[face, k]].astype(np.float64) for k in range(3))
            nrm = np.cross(p1 - p0, p2 - p0)
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            p = (p0 + p1 + p2) / 3 - nrm * rng.uniform(0.005, 0.05, (n, 1)) + rng.uniform(-0.01, 0.01, (n, 3))
        elif name in ("flat60", "accepted"):                         # x across every decade of the dominoes up to 1e3 (beyond, float32 squares of 'accepted' overflow)
            x = np.exp(rng.uniform(np.log(lo[0] * 0.5), np.log(min(hi[0] * 1.5, 1e3 if name == "accepted" else np.inf)), n))
            p = np.stack([x, rng.uniform(-0.2, 1.2, n), rng.uniform(-0.2, 1.2, n)], 1)
        else:
            p = rng.uniform(lo, hi, (4 * n + 16, 3))
            if name == "ico":                                        # the part of the box INSIDE the sphere: its corners are outside the mesh (see the module docstring)
                p = p[np.linalg.norm(p, axis=1) < 0.95]
            p = p[:n]
            assert len(p) == n
    elif kind == "outside":                                          # up to ten extents beyond the box, in every direction
        p = rng.uniform(lo - 10 * ext, hi + 10 * ext, (n, 3))
    elif kind == "surface":
        return _surface(name, n, rng, aim=0.05 if name == "ico_far" else None)
    elif kind == "vertex":
        p = v[np.unique(f[:real])]
    elif kind == "edge":
        e = _edges(f[:real])
        p = (v[e[:, 0]] + v[e[:, 1]]) * np.float32(0.5)
    elif kind == "centre":
        c = (lo + hi) / 2
        p = np.concatenate([c[None], c[None] + rng.uniform(-1e-5, 1e-5, (n - 1, 3)) * max(1.0, np.abs(c).max())])
    elif kind == "long":                                             # nearest to the long triangle of cube_long: beside it, all along it
        p = np.stack([rng.uniform(-45, 45, n), rng.uniform(2.5, 4.0, n), rng.uniform(0.0, 1.0, n)], 1)
    elif kind == "degenerate":                                       # within 0.06 of the zero-area faces, 0.4 from the sphere
        a = v[len(v) - 24:len(v) - 16].astype(np.float64)
        p = a[rng.integers(0, 8, n)] + np.concatenate([rng.uniform(0, 0.25, (n, 1)), rng.uniform(-0.04, 0.04, (n, 2))], 1)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(p, np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, kind, n):
    v, f, _ = mesh(name)
    p = points(name, kind, n)
    S = max(float(np.abs(v).max()), float(np.abs(p).max()))
    eps = 64 * U * S
    return S, eps, C.closest_ref(v, f, p, slack=2 * eps)


def run(name, kind, n, share=None):
    from iris_amd.utils.closest import closest_point
    v, f, real = mesh(name)
    p = points(name, kind, n)
    S, eps, ref = reference(name, kind, n)
    x = torch.from_numpy(p).to(DEV)
    tri, bary, pos, dist2 = closest_point(scene(name), x)
    again = closest_point(scene(name), x)
    for a, b in zip((tri, bary, pos, dist2), again):
        assert torch.equal(a.view(torch.int64 if a.dtype == torch.int64 else torch.int32), b.view(torch.int64 if b.dtype == torch.int64 else torch.int32))
    assert tri.dtype == torch.int64 and tri.shape == (len(p),) and bary.shape == (len(p), 2) and pos.shape == (len(p), 3) and dist2.shape == (len(p),)
    tri, bary, pos, dist2 = tri.cpu().numpy(), bary.cpu().numpy(), pos.cpu().numpy().astype(np.float64), dist2.cpu().numpy().astype(np.float64)
    assert (tri >= 0).all() and (tri < real).all(), "no face, or a zero-area one"
    d = np.sqrt(dist2)
    err = np.abs(d - ref["dist"])
    qualifies = ref["runner_up"] - ref["dist"] > 2 * eps
    print(f"{name}/{kind}/{len(p)}: S = {S:.4g}, largest |sqrt(dist2) - d_ref| = {err.max() / (U * S):.3g} x 2^-24 S (allowed 64), "
          f"{qualifies.mean() * 100:.1f} % of the points have a runner-up more than 2 eps behind")
    assert err.max() <= eps
    b64 = bary.astype(np.float64)
    assert (bary >= 0).all() and (b64.sum(1) <= 1.0).all()
    q = C.rebuild(v, f, tri, bary)
    assert np.linalg.norm(q - pos, axis=1).max() <= eps
    assert (np.linalg.norm(q - p.astype(np.float64), axis=1) <= ref["dist"] + eps).all()
    assert ref["near"][np.arange(len(p)), tri].all()
    if share is not None:
        assert qualifies.mean() >= share, "the argmin check would be vacuous: change the input"
    assert (tri[qualifies] == ref["argmin"][qualifies]).all()
    return tri, ref, d


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_sizes_inside_the_icosphere(n):
    run("ico", "box", n, share=0.9 if n > 1 else None)


@pytest.mark.parametrize("name, kind, n, share", [
    ("one", "box", 65, 0.9), ("one", "outside", 65, 0.9), ("one", "surface", 65, 0.9), ("one", "vertex", 3, None), ("one", "edge", 3, None),
    ("cube", "box", 4097, 0.9), ("cube", "outside", 4097, None), ("cube", "surface", 4097, 0.9), ("cube", "vertex", 8, None), ("cube", "edge", 18, None),
    ("ico", "outside", 4097, None), ("ico", "surface", 4097, 0.9), ("ico", "vertex", 642, None), ("ico", "edge", 1920, None), ("ico", "centre", 64, None),
    ("ico_far", "box", 4097, 0.9), ("ico_far", "outside", 4097, None), ("ico_far", "surface", 4097, 0.9), ("ico_far", "vertex", 642, None),
    ("ico_far", "centre", 64, None),
    ("cube_long", "box", 4097, 0.9), ("cube_long", "surface", 4097, 0.9),
])
def test_meshes_and_point_sets(name, kind, n, share):
    run(name, kind, n, share)


def test_long_triangle_reports_its_own_index_through_every_reference():
    info = scene("cube_long").info()
    assert info["n_leaf_records"] > info["n_triangles"] == 13, "the presplit made no references: the input does not test them"
    tri, ref, _ = run("cube_long", "long", 4097, share=0.9)
    assert (ref["argmin"] == 12).mean() > 0.9
    assert (tri[ref["argmin"] == 12] == 12).all()


def test_zero_area_faces_are_skipped():
    v, f, real = mesh("ico_degenerate")
    p = points("ico_degenerate", "degenerate", 4097)
    a = v[len(v) - 24:len(v) - 16].astype(np.float64)
    seg = np.abs(p[:, None, 1:].astype(np.float64) - a[None, :, 1:]).max(-1).min(1)
    assert real == 1280 and len(f) == 1288 and seg.max() <= 0.05                     # every point is nearer to a zero-area face than the sphere (0.4 away)
    tri, ref, d = run("ico_degenerate", "degenerate", 4097)
    assert d.min() > 0.3 and (tri < 1280).all()


@pytest.mark.parametrize("name", ["flat60", "accepted"])
def test_deep_trees(name):
    """the stack's spill part (3 entries per level on the first descent) on the deepest trees the library takes, and the one-sided bound of the module docstring"""
    info = scene(name).info()
    lds = deep_scenes.stack_sizes()["plain"]
    assert 3 * info["depth"] > lds, "the tree is too shallow to leave the LDS part of the stack"
    v, f, _ = mesh(name)
    tri, ref, d = run(name, "box", 4097)
    p = points(name, "box", 4097).astype(np.float64)
    local = np.maximum(np.maximum(np.abs(p).max(1), np.abs(v[f[ref["argmin"]]].astype(np.float64)).max((1, 2))), ref["dist"])
    over = (d - ref["dist"]) / (U * local)
    print(f"{name}: largest (sqrt(dist2) - d_ref) in units of 2^-24 max(|query|, |face|, d_ref): {over.max():.3g} (allowed 64)")
    assert (over <= 64).all()


def test_contract_edges():
    from iris_amd import _lib as L
    from iris_amd.utils.closest import closest_point
    from iris_amd.utils.path_tracing import Scene
    sc = scene("cube")
    out = closest_point(sc, torch.zeros(0, 3, device=DEV))
    assert [tuple(t.shape) for t in out] == [(0,), (0, 2), (0, 3), (0,)]
    x = torch.tensor([[0.5, 0.5, 2.0], [float("nan"), 0, 0], [0, float("inf"), 0], [0.25, 0.5, 0.5], [0, 0, -float("inf")]], device=DEV)
    tri, bary, pos, dist2 = closest_point(sc, x)
    assert tri.tolist()[1:3] == [-1, -1] and tri[4] == -1 and tri[0] >= 0 and tri[3] >= 0
    assert bool(torch.isinf(dist2[[1, 2, 4]]).all()) and not bool(bary[[1, 2, 4]].any()) and not bool(pos[[1, 2, 4]].any())
    assert abs(dist2[0].item() - 1.0) <= 1e-6 and np.allclose(pos[0].tolist(), [0.5, 0.5, 1.0], atol=1e-6) and abs(dist2[3].item() - 0.0625) <= 1e-6
    with pytest.raises(L.IrisError, match="requires grad"):
        closest_point(sc, torch.rand(4, 3, device=DEV, requires_grad=True))
    with pytest.raises(L.IrisError):
        closest_point(sc, torch.rand(4, 3))
    flat = Scene(np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]]), np.int32([[0, 1, 2], [1, 1, 3]]), device=torch.device(DEV))      # no triangle with an area
    tri, bary, pos, dist2 = closest_point(flat, torch.rand(65, 3, device=DEV))
    assert bool((tri == -1).all()) and bool(torch.isinf(dist2).all()) and not bool(bary.any()) and not bool(pos.any())
    f32 = Scene(*mesh("cube")[:2], device=torch.device(DEV), layout=L.BVH4_F32)
    with pytest.raises(L.IrisError, match="quantised node table"):
        closest_point(f32, torch.rand(4, 3, device=DEV))
