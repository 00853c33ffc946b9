#!/usr/bin/env python3
"""The texture export stage (iris_amd/utils/texture.py, iris_amd/csrc/iris_texture.h) on one MI355X -> profiles/texture_export.json.

  stages     a synthetic mesh of --faces (1 M) small triangles under grid_atlas, at 2048^2 and 4096^2: the UV raster, the resolve and the quantiser over the whole
             texture (per-call HIP event times: warm-up calls, then the median of --steps calls), and the whole bake_textures with an NGPBRDF
             (init_parameters(1337)) at chunk_size 160000 (host clock around a synchronise), with the share of it that the network's calls take
             (HIP events around every material_net call of one bake)
  classes    the same atlas plus two wall triangles that cover a quarter of the texture each (last in the face list): iris_uv_raster's default split against
             every triangle in the small class (iris_debug_uv_raster), in the same process, interleaved call by call.  `spread_ms` is the larger of the two
             arms' half distance between the 16th and the 84th percentile of their calls: the default must not be slower than the forced-small arm by more.
  threshold  where the classes cross: grid atlases of 200 .. 200 000 faces at 2048^2 (bounding boxes of ~42 000 .. ~42 texels), every triangle through the
             small class and every triangle through the large class, interleaved.  The built-in constant kUvSmallMaxTexels sits between the largest box at
             which the small class is not slower and the smallest at which the large class is.
There is no earlier implementation to compare with: no time here is an acceptance threshold.  Every arm's ids are compared with the default's in the run.
"""
import argparse, json, os, re, statistics, sys, time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def event_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


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


def med(ms):
    return round(statistics.median(ms), 4)


def half_spread(ms):
    s = sorted(ms)
    return round((s[min(len(s) - 1, int(round(0.84 * (len(s) - 1))))] - s[int(round(0.16 * (len(s) - 1)))]) / 2, 4)


def synthetic_mesh(F, seed=0):
    """F small triangles scattered in [-1, 1]^3, every face with its own vertices"""
    import numpy as np
    g = np.random.default_rng(seed)
    c = g.uniform(-0.95, 0.95, (F, 1, 3)).astype(np.float32)
    v = (c + g.uniform(-0.01, 0.01, (F, 3, 3)).astype(np.float32)).reshape(-1, 3)
    return v, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=1000000)
    ap.add_argument("--res", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--steps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--class_steps", type=int, default=9, help="calls per arm of the class comparison (the forced-small arm walks a quarter of the texture in ONE lane)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "texture_export.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from iris_amd import _lib as L
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.utils import texture as T
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    src = open(os.path.join(REPO, "iris_amd", "csrc", "iris_texture.h")).read()
    threshold = int(re.search(r"kUvSmallMaxTexels\s*=\s*(\d+)", src).group(1))
    F = args.faces
    v, f = synthetic_mesh(F)
    net = NGPBRDF(-1.0, 1.0).init_parameters(seed=1337).to(dev)
    res = {"what": "texture export on one MI355X: per-call HIP event medians (ms) of the UV raster, resolve and quantiser over the whole texture; bake_textures end to end "
                   "(host clock) with the network's share; the raster's two triangle classes compared",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "faces": F, "steps": args.steps, "warmup": args.warmup, "class_steps": args.class_steps,
           "class_threshold_texels": threshold, "stages": {}, "classes": {}, "threshold_sweep": {}}
    for r in args.res:
        vt, ft = T.grid_atlas(F, r)
        m = T.UVMesh(vt, ft, v, f, r, device=dev)
        ids = m.raster()
        n = r * r
        alb, rough = torch.rand(n, 3, device=dev), torch.rand(n, device=dev)
        img_a, img_rm = torch.empty(r, r, 3, dtype=torch.uint8, device=dev), torch.empty(r, r, 3, dtype=torch.uint8, device=dev)
        st = {"covered_share": round(float((ids >= 0).float().mean()), 4)}
        st["raster_ms"] = med(event_ms(lambda: m.raster(), args.steps, args.warmup))
        st["resolve_ms"] = med(event_ms(lambda: m.resolve(ids, bary=False), args.steps, args.warmup))
        st["quantize_ms"] = med(event_ms(lambda: T.quantize_into(alb, rough, rough, ids, 0, img_a, img_rm), args.steps, args.warmup))
        del alb, rough
        marks = []

        def timed_net(x):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = net(x); e1.record()
            marks.append((e0, e1))
            return out
        walls = []
        for k in range(args.warmup + 5):
            marks.clear()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            T.bake_textures(timed_net if k >= args.warmup else net, m.vt, m.ft, m.v, m.f, r, 160000, device=dev)
            torch.cuda.synchronize(); walls.append((time.perf_counter() - t0) * 1e3)
        st["bake_textures_ms"] = med(walls[args.warmup:])
        st["network_ms_last_bake"] = round(sum(a.elapsed_time(b) for a, b in marks), 3)
        st["bake_ms_last_bake"] = round(walls[-1], 3)
        st["network_share"] = round(st["network_ms_last_bake"] / walls[-1], 4)
        st["note"] = "bake_textures is handed device tensors: its input checks are reductions on the device with three scalar read-backs, part of the wall time"
        res["stages"][str(r)] = st
        del m, ids, img_a, img_rm

        # the two classes: the atlas plus two wall triangles of a quarter of the texture each, last in the list
        wall_vt = np.float32([[0, 0], [1, 0], [0, 0.5], [1, 1], [0, 1], [1, 0.5]])
        vt2 = np.concatenate([vt, wall_vt]); ft2 = np.concatenate([ft, np.int32([[3 * F, 3 * F + 1, 3 * F + 2], [3 * F + 3, 3 * F + 4, 3 * F + 5]])])
        v2 = np.concatenate([v, np.float32([[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [1, 1, 1], [-1, 1, 1], [1, -1, 1]])])
        f2 = np.concatenate([f, np.int32([[3 * F, 3 * F + 1, 3 * F + 2], [3 * F + 3, 3 * F + 4, 3 * F + 5]])])
        m2 = T.UVMesh(vt2, ft2, v2, f2, r, device=dev)
        want = m2.raster()
        assert torch.equal(m2.raster(T.RASTER_ALL_SMALL), want) and torch.equal(m2.raster(T.RASTER_AUTO), want)
        ms = interleaved_ms({"default": lambda: m2.raster(), "all_small": lambda: m2.raster(T.RASTER_ALL_SMALL)}, args.class_steps, 1)
        spread = max(half_spread(ms["default"]), half_spread(ms["all_small"]))
        res["classes"][str(r)] = {"default_ms": med(ms["default"]), "all_small_ms": med(ms["all_small"]), "spread_ms": spread,
                                  "default_half_spread_ms": half_spread(ms["default"]), "all_small_half_spread_ms": half_spread(ms["all_small"]),
                                  "covered_share": round(float((want >= 0).float().mean()), 4),
                                  "default_not_slower_than_all_small": bool(med(ms["default"]) <= med(ms["all_small"]) + spread)}
        del m2, want
    # where the classes cross
    r = 2048
    for Fs in (200, 2000, 20000, 50000, 100000, 200000):
        vs, fs = synthetic_mesh(Fs, 1)
        vt, ft = T.grid_atlas(Fs, r)
        ms_ = T.UVMesh(vt, ft, vs, fs, r, device=dev)
        want = ms_.raster()
        assert torch.equal(ms_.raster(T.RASTER_ALL_SMALL), want) and torch.equal(ms_.raster(T.RASTER_ALL_LARGE), want)
        G = int(np.ceil(np.sqrt((Fs + 1) // 2)))
        ms = interleaved_ms({"all_small": lambda: ms_.raster(T.RASTER_ALL_SMALL), "all_large": lambda: ms_.raster(T.RASTER_ALL_LARGE), "default": lambda: ms_.raster()},
                            args.steps, args.warmup)
        res["threshold_sweep"][str(Fs)] = {"box_texels": int(round((r / G) ** 2)), "all_small_ms": med(ms["all_small"]), "all_large_ms": med(ms["all_large"]),
                                           "default_ms": med(ms["default"]), "spread_ms": max(half_spread(x) for x in ms.values())}
        del ms_, want
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
