"""Tiny scenes whose 4-wide BVH is tall and one-sided, rays whose traversal stack outgrows its LDS part on them, and the host replay that says how deep each ray's
stack gets (tools/stack_replay: the library's own builder + the kernels' push rule, no GPU).  No project import: test_deep_stack_cpu.py asserts what the GPU tests
of test_deep_stack.py rely on, and both take the stack sizes from the replay, never from a typed-in number.

"Dominoes": triangle i lies in the plane x = x_i = x0 * ratio^i.  The binned SAH peels a few far triangles off per level, and the 4-wide collapse keeps a tree whose
every node is "some leaves plus one subtree of nearer triangles".  A ray towards +x descends into the near subtree first with t = inf and leaves up to three siblings
on its stack per level; a ray towards -x meets the leaves first and stays at a few entries."""
import json
import os
import re
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "iris_amd", "csrc")
REPLAY_SRC = os.path.join(REPO, "tools", "stack_replay", "stack_replay.cpp")
DEEP, SHALLOW, MID, RANDOM = 0, 1, 2, 3

# name -> (n, ratio, x0, cone).  The first three are traced by every kernel test; "accepted" is the deepest tree iris_scene_create takes, "refused" the one it must not.
SCENES = {
    "flat60": (60, 1.5, 1.0, False),
    "cone60": (60, 1.5, 1.0, True),
    "accepted": (230, 1.5, 1e-9, False),
    "refused": (200, 2.0, 1e-30, False),
}
TRACED = ("flat60", "cone60", "accepted")
# what the stand-alone program must survive besides: one triangle, coincident dominoes, ratio 1 (every domino in one plane), and the cone whose box areas overflow
# float32 (coordinates up to 2^119 are finite, their products are not: the builder used to die of std::bad_alloc on it)
DEGENERATE = {
    "one": (1, 1.5, 1.0, False),
    "coincident": (2, 1.0, 1.0, True),
    "ratio1": (40, 1.0, 1.0, False),
    "overflow": (120, 2.0, 1.0, True),
}


def dominoes(n, ratio, x0, cone):
    """(verts (3n, 3) float32, faces (n, 3) int32).  Flat: (x_i,0,0) (x_i,1,0) (x_i,0,1); cone: (x_i,0,0) (x_i,x_i,0) (x_i,0,x_i), self-similar about the origin."""
    x = (np.float64(x0) * np.float64(ratio) ** np.arange(n)).astype(np.float32).astype(np.float64)
    s = x if cone else np.ones(n)
    v = np.zeros((n, 3, 3))
    v[:, :, 0] = x[:, None]
    v[:, 1, 1] = s
    v[:, 2, 2] = s
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def scene(name):
    return dominoes(*{**SCENES, **DEGENERATE}[name])


def rays(name, n=16384, seed=0):
    """(o, d, kind) float32 / float32 / int8 for a scene: 3/8 DEEP rays (from the low-x end towards +x, inside every box; half aimed at the first domino, half past
    every hypotenuse: those miss everything and run the whole depth-first traversal), 3/8 SHALLOW (the same lines, reversed from beyond the far end), 1/8 MID (origins
    between two consecutive dominoes, either way along such a line: every stack size in between) and 1/8 RANDOM.  Directions are unit vectors."""
    nd, ratio, x0, cone = {**SCENES, **DEGENERATE}[name]
    rng = np.random.default_rng(seed)
    x = np.float64(x0) * np.float64(ratio) ** np.arange(nd)
    kind = np.full(n, RANDOM, np.int8)
    kind[: 3 * n // 8] = DEEP
    kind[3 * n // 8: 6 * n // 8] = SHALLOW
    kind[6 * n // 8: 7 * n // 8] = MID
    if n < 8:
        kind[:] = DEEP
    # a line through the scene: (a, b) are the cone's slopes or the flat scene's (y, z); a + b < 1 meets the triangles, a + b > 1 passes them inside their boxes
    # (half of the deep and of the mid rays miss; of the shallow ones a quarter: under the F32 rule a reversed ray that misses everything keeps most of the tree
    #  on its stack -- every box is entered at once --, and a quarter of all rays has to stay shallow under either rule)
    ab = rng.uniform(0.05, 0.95, size=(16 * n + 64, 2))
    ab = ab[np.abs(ab.sum(1) - 1.0) > 0.05]
    i = np.arange(n)
    want_hit = np.where(kind == SHALLOW, i % 4 != 3, i % 2 == 0)
    hits, misses = ab[ab.sum(1) < 1.0], ab[ab.sum(1) > 1.0]
    assert len(hits) >= n and len(misses) >= n
    ab = np.where(want_hit[:, None], hits[:n], misses[:n])
    start = np.where(kind == DEEP, 0.5 * x[0], 1.5 * x[-1])
    gap = rng.integers(0, max(nd - 1, 1), size=n)
    mid = np.sqrt(x[gap] * x[np.minimum(gap + 1, nd - 1)])
    start = np.where(kind == MID, mid, start)
    sign = np.where(kind == DEEP, 1.0, -1.0)
    sign = np.where(kind == MID, np.where(rng.random(n) < 0.75, 1.0, -1.0), sign)
    if cone:
        o = start[:, None] * np.concatenate([np.ones((n, 1)), ab], 1)
        d = sign[:, None] * np.concatenate([np.ones((n, 1)), ab], 1)
    else:
        o = np.concatenate([start[:, None], ab], 1)
        tilt = rng.uniform(-0.04, 0.04, size=(n, 2)) / x[-1]               # stays inside the unit square all the way
        d = np.concatenate([sign[:, None], tilt], 1)
    r = kind == RANDOM
    lo = np.log(x[0] * 0.5), np.log(x[-1] * 1.5)
    ext = np.exp(rng.uniform(lo[0], lo[1], size=n))
    ro = np.stack([ext, rng.uniform(-0.2, 1.2, n) * (ext if cone else 1.0), rng.uniform(-0.2, 1.2, n) * (ext if cone else 1.0)], 1)
    rd = rng.normal(size=(n, 3))
    o[r], d[r] = ro[r], rd[r]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), kind


def mixed_order(kind):
    """a permutation that spreads every kind evenly: deep and shallow rays alternate in the lanes of one wave (the first ray is a deep one)"""
    kind = np.asarray(kind)
    frac = np.zeros(len(kind))
    for k in np.unique(kind):
        m = kind == k
        frac[m] = (np.arange(m.sum()) + (0.0 if k == DEEP else 0.5)) / m.sum()
    return np.argsort(frac, kind="stable")


def blocked_order(kind):
    """a permutation with whole waves of each kind (as rays() lays them out for multiples of 512 rays)"""
    return np.argsort(np.asarray(kind), kind="stable")


def header_int(header, name):
    """`constexpr int NAME = value` or `#define NAME value` of a header under iris_amd/csrc, as test_jpeg.py reads kPngMaxImages"""
    src = open(os.path.join(CSRC, header)).read()
    m = re.search(r"(?:constexpr\s+int\s+|,\s*|#define\s+)" + name + r"\s*=?\s*(\d+)", src)
    assert m, (header, name)
    return int(m.group(1))


def stack_sizes():
    """the LDS parts of the three stack sizes and the capacity, from the headers"""
    lds, spill = header_int("iris_trace.h", "kStackLds"), header_int("iris_trace.h", "kStackSpill")
    return {"plain": lds, "bake_tile": header_int("iris_bake.h", "IRIS_TILE_STACK"), "pt_tile": header_int("iris_pt.h", "kPtTileStack"), "capacity": lds + spill}


def thresholds():
    s = stack_sizes()
    return sorted({s[k] - 3 for k in ("plain", "bake_tile", "pt_tile")} | {s[k] for k in ("plain", "bake_tile", "pt_tile")})


def build_replay(out_dir, sanitize=False):
    exe = os.path.join(str(out_dir), "stack_replay_san" if sanitize else "stack_replay")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", *flags, "-I", CSRC, REPLAY_SRC, os.path.join(CSRC, "bvh_build.cpp"), "-lpthread", "-o", exe], check=True, timeout=600)
    return exe


def replay(exe, work_dir, verts, faces, o, d, max_leaf=4, presplit=8.0):
    """run the host program -> its JSON (depth, n_leaf_records, per-ray maximal stack size under the Q8 and the F32 push rule, per-ray hit)"""
    tag = "%d_%d" % (os.getpid(), replay.calls)
    replay.calls += 1
    sp, rp = os.path.join(str(work_dir), "scene_%s.bin" % tag), os.path.join(str(work_dir), "rays_%s.bin" % tag)
    verts, faces = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    o, d = np.ascontiguousarray(o, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    with open(sp, "wb") as f:
        f.write(np.array([len(verts), len(faces)], np.int32).tobytes() + verts.tobytes() + faces.tobytes())
    with open(rp, "wb") as f:
        f.write(np.array([len(o)], np.int32).tobytes() + o.tobytes() + d.tobytes())
    out = subprocess.run([exe, sp, rp, str(int(max_leaf)), repr(float(presplit))], check=True, capture_output=True, text=True, timeout=600).stdout
    res = json.loads(out)
    for k in ("max_q8", "max_f32", "hit_q8", "hit_f32"):
        if k in res:
            res[k] = np.asarray(res[k], np.int64)
    return res


replay.calls = 0
