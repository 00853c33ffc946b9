#!/usr/bin/env python3
"""The pre-bake stages' pass over one view (iris_amd/utils/gbuffer.py pool_view, iris_amd/csrc/iris_prebake.h) on one MI355X -> profiles/prebake_1080p.json.

Scene: the bench scene (tools/synth.room, --tris 1 000 000) and ONE 1080p view (tools/synth.camera) with a seeded 8-bit photograph, an EmorCRF of 1024 knots
with non-zero weights, the voxel grid of --voxel_num 256 built from that view.  In the same process, the arms taking turns call by call (per-call HIP event
times; --warmup calls, then the median and the half distance between the 16th and 84th percentile of --steps calls):

  fused_*      pool_view for each of the three passes of bake_slf (bounds, occupancy, voxel pool through the response model's inverse) and for the triangle
               pool of extract_emitters (raw 8-bit values): one launch on the device-resident 8-bit photograph
  composed_*   what each replaces, rebuilt here from the public primitives: cameras.view_rays + ray_intersect + boolean mask + EmorCRF.inverse +
               VoxelSLF.scatter_add / voxel_histogram / scatter_add_rows, on the device-resident FLOAT photograph (the earlier path uploaded the host's u / 255)
  trace_only   pool_view with no sink: ray generation and closest hit alone -> trace_share_of_fused_*, the part of a pass that storing the hits would save
  host_decode_png_ms, upload_u8_ms, upload_f32_ms   the photograph's way to the device (host clock around a synchronise): PIL decode of a 1080p PNG, and the
               upload of 6.2 MB (8-bit, what the commands send) against 24.9 MB (float32, what the composition needs)
  fused_per_lane_*   the same launch with one set of atomics per hit (iris_debug_set("pool_combine", 0)) instead of the default, which sums a wave's equal
               destinations first: the arm that decides which of the two forms is the default
Before anything is timed every fused pass, in both forms, is compared with its composition on fresh sinks (counts, histogram, bounds exact; means to rtol 2e-5,
atol 1e-6).  There is no earlier measurement of either side: no time here is an acceptance threshold.
"""
import argparse, json, os, statistics, sys, tempfile, time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def interleaved_ms(arms, steps, warmup):
    """arms: {name: fn} -> {name: [ms per call]}, the arms taking turns call by call"""
    import torch
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(steps):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def host_ms(fn, steps, warmup):
    import torch
    out = []
    for k in range(warmup + steps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def med(ms):
    return round(statistics.median(ms), 4)


def half_spread(ms):
    s = sorted(ms)
    return round((s[min(len(s) - 1, int(round(0.84 * (len(s) - 1))))] - s[int(round(0.16 * (len(s) - 1)))]) / 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--img_hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--voxel_num", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "prebake_1080p.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from iris_amd import _lib as L
    from iris_amd import slf_bake as sb
    from iris_amd.model.crf import EmorCRF
    from iris_amd.model.slf import VoxelSLF
    from iris_amd.utils import cameras, stage
    from iris_amd.utils.gbuffer import pool_view, scatter_add_rows, voxel_histogram
    from iris_amd.utils.path_tracing import Scene, ray_intersect
    from iris_amd.utils.texture import write_png
    from tools import synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_prebake needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    hw = tuple(args.img_hw)
    n = hw[0] * hw[1]
    room = synth.room(0, args.tris)
    scene = Scene(room["vertices"], room["faces"], device=dev)
    n_tri = len(room["faces"])
    K, c2w = synth.camera(hw[0], hw[1], 0)
    view = {"kind": "real", "K": K, "c2w": c2w}
    photo = np.random.default_rng(0).integers(0, 256, (hw[0], hw[1], 3)).astype(np.uint8)
    photo_f = (photo.astype(np.float64) / 255.0).astype(np.float32)                  # the host's u / 255
    img_u8, img_f = torch.from_numpy(photo).to(dev), torch.from_numpy(photo_f).to(dev).reshape(-1, 3)
    s = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (j + 1)) * 0.05 for j in range(3)]))
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    crf.to(dev)
    exposure = 0.8
    batch = {"camera": view, "img_hw": hw, "image": img_u8, "exposure": exposure}
    vmin, vmax = (float(x) for x in sb.scene_bounds(scene, [batch], "real", dev))
    mask = sb.visible_voxels(scene, [batch], vmin, vmax, args.voxel_num, dev) > 0
    tables = (crf.grid, crf.get_inv_crf())

    class Sinks:
        def __init__(self):
            self.bounds = torch.tensor([1000.0, 0.0], device=dev)
            self.hist = torch.zeros(args.voxel_num, args.voxel_num, args.voxel_num, device=dev)
            self.vslf = VoxelSLF(mask, vmin, vmax)
            self.tri_sum, self.tri_count = torch.zeros(n_tri, 3, device=dev), torch.zeros(n_tri, device=dev)

    def hits():
        xs, ds = cameras.view_rays(view, hw, dev)
        pos, _, _, idx, valid = ray_intersect(scene, xs, ds)
        return pos, idx, valid

    def composed(s):
        def bounds():
            pos, _, valid = hits()
            p = pos[valid]
            s.bounds[0] = torch.minimum(s.bounds[0], p.min()); s.bounds[1] = torch.maximum(s.bounds[1], p.max())

        def occupancy():
            pos, _, valid = hits()
            voxel_histogram(pos[valid], vmin, vmax, args.voxel_num, s.hist)

        def voxel_pool():
            pos, _, valid = hits()
            s.vslf.scatter_add(pos[valid], crf.inverse(img_f, exposure)[valid])

        def triangle_pool():
            _, idx, valid = hits()
            scatter_add_rows(img_f[valid], idx[valid], s.tri_sum, s.tri_count)
        return {"bounds": bounds, "occupancy": occupancy, "voxel_pool": voxel_pool, "triangle_pool": triangle_pool}

    def fused(s):
        cam = {"camera": view, "img_hw": hw}
        return {"bounds": lambda: pool_view(scene, bounds=s.bounds, **cam),
                "occupancy": lambda: pool_view(scene, hist=s.hist, voxel_range=(vmin, vmax), **cam),
                "voxel_pool": lambda: pool_view(scene, vslf=s.vslf, image=img_u8, crf_tables=tables, exposure=exposure, **cam),
                "triangle_pool": lambda: pool_view(scene, tri_sum=s.tri_sum, tri_count=s.tri_count, image=img_u8, **cam)}

    # same results first, on fresh sinks
    a, b = Sinks(), Sinks()
    for fn in list(fused(a).values()) + list(composed(b).values()):
        fn()
    torch.cuda.synchronize()
    mean = lambda t, c: (t / c.clamp_min(1).unsqueeze(-1).to(t.dtype)).cpu().numpy()
    same = {"bounds": bool((a.bounds == b.bounds).all()), "hist": bool(torch.equal(a.hist, b.hist)), "voxel_count": bool(torch.equal(a.vslf.count, b.vslf.count)),
            "triangle_count": bool(torch.equal(a.tri_count, b.tri_count)),
            "voxel_mean": bool(np.allclose(mean(a.vslf.radiance, a.vslf.count), mean(b.vslf.radiance, b.vslf.count), rtol=2e-5, atol=1e-6)),
            "triangle_mean": bool(np.allclose(mean(a.tri_sum, a.tri_count), mean(b.tri_sum, b.tri_count), rtol=2e-5, atol=1e-6))}
    hit_pixels = int(a.hist.sum())
    assert all(same.values()), same

    def per_lane(fn):
        def call():
            L.debug_set("pool_combine", 0)
            try:
                fn()
            finally:
                L.debug_set("pool_combine", -1)
        return call

    c = Sinks()                                           # the per-lane arm against the same composition, before it is timed
    for fn in fused(c).values():
        per_lane(fn)()
    torch.cuda.synchronize()
    same["per_lane_counts"] = bool(torch.equal(c.hist, b.hist) and torch.equal(c.vslf.count, b.vslf.count) and torch.equal(c.tri_count, b.tri_count))
    same["per_lane_means"] = bool(np.allclose(mean(c.vslf.radiance, c.vslf.count), mean(b.vslf.radiance, b.vslf.count), rtol=2e-5, atol=1e-6)
                                  and np.allclose(mean(c.tri_sum, c.tri_count), mean(b.tri_sum, b.tri_count), rtol=2e-5, atol=1e-6))
    assert all(same.values()), same

    arms = {"trace_only": lambda: pool_view(scene, camera=view, img_hw=hw)}
    for k, fn in fused(a).items():
        arms["fused_" + k] = fn
    for k, fn in fused(c).items():
        if k != "bounds":                                 # (the bounds have one form)
            arms["fused_per_lane_" + k] = per_lane(fn)
    for k, fn in composed(b).items():
        arms["composed_" + k] = fn
    ms = interleaved_ms(arms, args.steps, args.warmup)

    tmp = tempfile.mkdtemp()
    png = os.path.join(tmp, "photo.png")
    write_png(png, photo)
    pinned_note = "pageable host memory, as torch.from_numpy gives it"
    rows = {k: {"ms": med(v), "half_spread_ms": half_spread(v)} for k, v in ms.items()}
    for k in ("bounds", "occupancy", "voxel_pool", "triangle_pool"):
        rows["fused_" + k]["trace_share"] = round(rows["trace_only"]["ms"] / rows["fused_" + k]["ms"], 4)
        rows["fused_" + k]["composed_over_fused"] = round(rows["composed_" + k]["ms"] / rows["fused_" + k]["ms"], 3)
        if k != "bounds":
            rows["fused_" + k]["per_lane_over_combined"] = round(rows["fused_per_lane_" + k]["ms"] / rows["fused_" + k]["ms"], 3)
    host = {"host_decode_png_ms": med(host_ms(lambda: stage.read_photograph(png, hw), 5, 1)),
            "upload_u8_ms": med(host_ms(lambda: torch.from_numpy(photo).to(dev), args.steps, args.warmup)),
            "upload_f32_ms": med(host_ms(lambda: torch.from_numpy(photo_f).to(dev), args.steps, args.warmup)),
            "note": "host clock around a synchronise; " + pinned_note + "; the PNG holds seeded noise (it does not compress: a photograph decodes faster)"}
    res = {"what": "one 1080p view of the bench scene through the pre-bake passes: pool_view (one launch) against the composition it replaces, interleaved; per-call HIP "
                   "event medians (ms)",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "tris": n_tri, "img_hw": list(hw), "voxel_num": args.voxel_num, "voxels_seen": int(mask.sum()),
           "hit_pixels": hit_pixels, "pixels": n, "steps": args.steps, "warmup": args.warmup, "same_results": same, "rows": rows, "photograph": host,
           "bake_slf_three_passes_ms": {"fused": round(sum(rows["fused_" + k]["ms"] for k in ("bounds", "occupancy", "voxel_pool")), 4),
                                        "composed": round(sum(rows["composed_" + k]["ms"] for k in ("bounds", "occupancy", "voxel_pool")), 4)},
           "wave_combining": "fused_* combine a wave's equal destinations before the atomic (the default); fused_per_lane_* issue one set of atomics per hit "
                             "(iris_debug_set pool_combine 0), as the composition's scatter kernels do",
           "not_measured": "the composition with its primary hits stored across the three passes (the removed cache= path); kernel times by profiler"}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
