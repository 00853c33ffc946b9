"""What tests/test_deep_stack.py relies on, asserted without a GPU: the domino scenes of tests/deep_scenes.py really force tall one-sided trees out of the
builder as it is today, and their ray sets really hold rays on either side of every branch the traversal stacks take when they leave their LDS part.  The stack
sizes come from tools/stack_replay (the library's builder + the kernels' push rule on the host), the thresholds from iris_trace.h, iris_bake.h and iris_pt.h.
A change to the builder that flattens these trees fails HERE, not silently on the GPU.

Maximal stack sizes that occur (16 384 rays per scene, as the replay of this revision prints them; the test prints today's).  At max_leaf 4, default presplit:
  flat60   (depth 11): Q8 and F32 0-14, 17, 21-25, 33
  cone60   (depth 17): Q8 0-20, 22-25, 28-34, 36-38, 45-49             F32 0-24, 28-34, 36-38, 44-49
  accepted (depth 29): Q8 0-12, 14, 76-78, 80, 85                      F32 0-9, 11-13, 61, 62, 64, 65, 67, 68, 70, 76-78, 80, 85
and over the family with its four builds (max_leaf 1 and 4, presplit off and on):
  Q8  0-26, 28-39, 45-50, 76-80, 82, 85, 87           F32 0-26, 28-39, 44-50, 61-70, 72, 76-80, 82, 85, 87
so every threshold T in {7, 9, 10, 12, 21, 24} (LDS_DEPTH - 3 and LDS_DEPTH of the three stack sizes) has rays at T, just below it and just above it.

The issue behind these tests bounds a ray's maximum by 3 * (depth - 1); its own table (33 entries at depth 11, 85 at depth 29) contradicts that.  What holds by
construction, and what iris_scene_create's refusal 3 * depth + 4 > capacity relies on, is 3 * depth: every internal node on the path from the root leaves at most
three siblings.  That is the bound asserted here."""
import collections

import numpy as np
import pytest

import deep_scenes as ds

N_RAYS = 16384
BUILDS = [(4, 8.0), (1, 8.0), (4, 0.0), (1, 0.0)]        # (bvh_max_leaf, presplit): 1 and 4, off and the default


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ds.build_replay(tmp_path_factory.mktemp("stack_replay"))


@pytest.fixture(scope="module")
def family(exe, tmp_path_factory):
    """(scene, max_leaf, presplit) -> replay of the scene's 16 384 rays"""
    tmp = tmp_path_factory.mktemp("replays")
    out = {}
    for name in ds.TRACED:
        v, f = ds.scene(name)
        o, d, kind = ds.rays(name, N_RAYS)
        for leaf, ps in BUILDS:
            out[name, leaf, ps] = dict(ds.replay(exe, tmp, v, f, o, d, leaf, ps), kind=kind)
    return out


def test_thresholds_come_from_the_headers():
    s = ds.stack_sizes()
    assert s["pt_tile"] < s["bake_tile"] < s["plain"] < s["capacity"] and len(ds.thresholds()) == 6


def test_each_scene_mixes_deep_and_shallow_rays(family):
    s = ds.stack_sizes()
    for (name, leaf, ps), r in family.items():
        assert r["buildable"] and r["quantised"] and r["rays"] == N_RAYS
        for rule in ("max_q8", "max_f32"):
            m = r[rule]
            hist = sorted(collections.Counter(m.tolist()).items())
            print(f"{name} max_leaf {leaf} presplit {ps} {rule}: depth {r['depth']}, {r['n_leaf_records']} leaf records, (maximal stack size, rays) {hist}")
            assert (m > s["plain"]).mean() >= 0.25, (name, leaf, ps, rule)
            assert (m <= s["pt_tile"] - 1).mean() >= 0.25, (name, leaf, ps, rule)
            w = m[ds.mixed_order(r["kind"])].reshape(-1, 64)                     # every wave of the mixed interleaving holds both kinds ...
            assert ((w > s["plain"]).any(1) & (w <= s["pt_tile"] - 1).any(1)).all(), (name, leaf, ps, rule)
            assert m.max() <= 3 * r["depth"], (name, leaf, ps, rule)             # (see the module docstring)
            assert m.max() + 4 <= s["capacity"]
        w = r["max_q8"][ds.blocked_order(r["kind"])].reshape(-1, 64)             # ... and the blocked one has whole waves of each
        assert (w > s["plain"]).all(1).any() and (w <= s["pt_tile"] - 1).all(1).any(), (name, leaf, ps)
        np.testing.assert_array_equal(r["hit_q8"], r["hit_f32"])                  # the closest hit does not depend on the order of the visits
        assert 0.3 < (r["hit_q8"] >= 0).mean() < 0.8                              # hits and misses both


def test_every_threshold_has_rays_on_either_side(family):
    for rule in ("max_q8", "max_f32"):
        seen = np.unique(np.concatenate([r[rule] for r in family.values()]))
        print(rule, "maximal stack sizes that occur over the family:", seen.tolist())
        for t in ds.thresholds():
            assert (seen <= t).any() and (seen > t).any(), (rule, t)
            # and close by: a maximum within two entries below and within three above, so that a wave's ballot really changes sides there
            assert ((seen > t - 3) & (seen <= t)).any() and ((seen > t) & (seen <= t + 3)).any(), (rule, t, seen.tolist())


def test_small_ray_counts_keep_a_deep_ray(family):
    """the GPU tests trace the first 1, 63, 64, 65 and 257 rays of the mixed order"""
    s = ds.stack_sizes()
    for (name, leaf, ps), r in family.items():
        m = r["max_q8"][ds.mixed_order(r["kind"])]
        assert m[0] > s["plain"]
        for n in (63, 64, 65, 257):
            assert (m[:n] > s["plain"]).any() and (m[:n] <= s["pt_tile"] - 1).any()


def test_capacity_scenes(exe, tmp_path, family):
    cap = ds.stack_sizes()["capacity"]
    for leaf, ps in BUILDS:
        d = family["accepted", leaf, ps]["depth"]
        assert cap - 8 <= 3 * d + 4 <= cap, (leaf, ps, d)
        assert family["accepted", leaf, ps]["max_q8"].max() >= cap - 12          # the one place a stack comes within a dozen entries of the capacity
    v, f = ds.scene("refused")
    o, d, _ = ds.rays("refused", 64)
    for leaf, ps in BUILDS:
        r = ds.replay(exe, tmp_path, v, f, o, d, leaf, ps)
        assert 3 * r["depth"] + 4 > cap, (leaf, ps, r["depth"])


def test_replay_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined (stand-alone: nothing is preloaded), over the whole family and the degenerate inputs -- one triangle,
    two coincident dominoes, ratio 1, and the cone whose box areas overflow float32, which build_wide_bvh used to answer with std::bad_alloc."""
    san = ds.build_replay(tmp_path, sanitize=True)
    for name in list(ds.SCENES) + list(ds.DEGENERATE):
        v, f = ds.scene(name)
        o, d, _ = ds.rays(name, 512)
        for leaf, ps in BUILDS:
            r = ds.replay(san, tmp_path, v, f, o, d, leaf, ps)        # (check=True: a sanitizer report ends the program with a failure)
            if name == "overflow":
                assert r == {"buildable": False, "n_nodes": 0}
            else:
                assert r["buildable"] and r["depth"] >= 1 and len(r["max_f32"]) == 512


def test_oracle_trees_fit_the_oracle_stack(oracle_mod):
    """oracle/iris_oracle.c intersect_bvh keeps 128 stack entries, one per level of its binary tree, and orc_scene_create refuses a deeper tree (Scene raises):
    the scenes traced through the oracle's BVH are far below that, and the two larger ones build as well (they are only ever traced by brute force)."""
    for name in ds.SCENES:
        d = oracle_mod.Scene(*ds.scene(name)).depth()
        print(name, "oracle tree depth", d)
        assert 1 <= d <= 128
        assert d <= 64 or name not in ("flat60", "cone60")
