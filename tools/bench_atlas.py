#!/usr/bin/env python3
"""The area-proportional atlas and the seam dilation (iris_amd.utils.texture.area_atlas / dilate_into, iris_amd/csrc/iris_atlas.h) on one MI355X
-> profiles/atlas_area.json.  The mesh is the benchmark's room (tools/synth.room, seed 1, 1.0 M triangles), the texture 4096^2.

  arms       taking turns call by call, host clock around a device synchronise: area_atlas from host arrays (upload included) and from device tensors;
             grid_atlas plus the upload of its vt / ft (what the grid stand-in costs before the same bake); the numpy restatement (tests/atlas_ref.py) on the same
             host, --ref_steps times.  `half_spread_ms` is half the distance between the 16th and the 84th percentile of an arm's calls.
  kernels    per-launch HIP event medians: measure, classes (one probe, at the chosen j), the stable sort that ranks (torch), place; and the stages of one
             area_atlas call as L.StageTimer sees them (event to event on the stream, so `classes` holds the host's small read after every probe)
  dilate     dilate_into at n = 2 on the two 4096^2 images under the area atlas (HIP events)
  texels     the report of area_atlas, and how many faces cover how many texels (the rasteriser's ids) under grid_atlas and under area_atlas, with the quantiles
             of texels per unit of sqrt(D_j) * area
Descriptive: no time here is an acceptance threshold.  The device's vt is compared with the restatement's in the run.
"""
import argparse, json, os, statistics, sys, time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def med(ms):
    return round(statistics.median(ms), 4)


def half_spread(ms):
    s = sorted(ms)
    return round((s[min(len(s) - 1, int(round(0.84 * (len(s) - 1))))] - s[int(round(0.16 * (len(s) - 1)))]) / 2, 4)


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


def wall_ms(fn):
    import torch
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def texel_table(ids, F, share):
    """ids (R, R) int32 on the device, share (F) float64 numpy: each face's sqrt(D) * area -> faces per power-of-two bucket of covered texels, and quantiles"""
    import numpy as np
    import torch
    n = torch.bincount(ids[ids >= 0].to(torch.int64), minlength=F).cpu().numpy()
    buckets = {"0": int((n == 0).sum())}
    b = 1
    while b <= n.max():
        buckets[f"{b}..{2 * b - 1}"] = int(((n >= b) & (n < 2 * b)).sum())
        b *= 2
    ok = share > 0
    ratio = n[ok] / share[ok]
    q = {f"p{p}": float(np.percentile(ratio, p)) for p in (1, 5, 25, 50, 75, 95, 99)}
    return {"faces_by_texels": buckets, "texels_min": int(n.min()), "texels_max": int(n.max()), "covered_share": round(float((ids >= 0).float().mean()), 4),
            "texels_per_share_quantiles": q}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1000000); ap.add_argument("--scene-seed", type=int, default=1)
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=15); ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--ref_steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "atlas_area.json"))
    args = ap.parse_args()
    import ctypes as C
    import numpy as np
    import torch
    import atlas_ref as A
    from iris_amd import _lib as L
    from iris_amd.utils import texture as T
    from tools import synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_atlas needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    room = synth.room(args.scene_seed, args.tris)
    v, f = np.ascontiguousarray(room["vertices"], np.float32), np.ascontiguousarray(room["faces"], np.int32)
    F, R = f.shape[0], args.res
    v_d, f_d = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    res = {"what": "area_atlas and dilate_into on one MI355X: the benchmark's room at one texture size; wall-clock medians (ms) of the interleaved arms, per-launch HIP "
                   "event medians, the atlas report and the texels per face under the two built-in atlases.  Descriptive: no threshold hangs on a number here",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "faces": F, "vertices": int(v.shape[0]), "tex_res": R, "steps": args.steps, "warmup": args.warmup,
           "ref_steps": args.ref_steps}

    # the result, once, against the restatement
    vt, ft, report = T.area_atlas(v_d, f_d, R)
    t0 = time.perf_counter(); want_vt, want_ft, want_rep = A.area_atlas_ref(v, f, R); first_ref_ms = (time.perf_counter() - t0) * 1e3
    res["equals_restatement"] = bool(np.array_equal(vt.cpu().numpy().view(np.int32), want_vt.view(np.int32)) and report == want_rep)
    res["report"] = report

    # the arms
    def grid_arm():
        g_vt, g_ft = T.grid_atlas(F, R)
        return torch.from_numpy(g_vt).to(dev), torch.from_numpy(g_ft).to(dev)
    arms = {"area_atlas_host_inputs": lambda: T.area_atlas(v, f, R, device=dev), "area_atlas_device_inputs": lambda: T.area_atlas(v_d, f_d, R),
            "grid_atlas_plus_upload": grid_arm}
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    ms = {k: [] for k in arms}
    ms["numpy_restatement"] = [first_ref_ms]
    for step in range(args.steps):
        for k, fn in arms.items():
            ms[k].append(wall_ms(fn))
        if step + 1 < args.ref_steps:
            t0 = time.perf_counter(); A.area_atlas_ref(v, f, R); ms["numpy_restatement"].append((time.perf_counter() - t0) * 1e3)
    res["arms_ms"] = {k: {"median": med(x), "half_spread_ms": half_spread(x), "calls": len(x)} for k, x in ms.items()}

    # the launches, one by one
    lib = L.lib()
    S = torch.empty(F, dtype=torch.float64, device=dev); corner = torch.empty(F, dtype=torch.uint8, device=dev); k = torch.empty(F, dtype=torch.uint8, device=dev)
    hist = torch.empty(16, dtype=torch.int64, device=dev); out_vt = torch.empty(3 * F, 2, device=dev)
    L.check(lib.iris_atlas_measure(L.ptr(v_d), v.shape[0], L.ptr(f_d), F, L.ptr(S), L.ptr(corner), L.stream()))
    L.check(lib.iris_atlas_classes(L.ptr(S), F, report["j"], R, L.ptr(k), L.ptr(hist), L.stream()))
    h = (C.c_int64 * 14)(*hist.cpu().tolist()[:14])
    order = torch.sort(k, stable=True)[1]
    kern = {"measure": lambda: L.check(lib.iris_atlas_measure(L.ptr(v_d), v.shape[0], L.ptr(f_d), F, L.ptr(S), L.ptr(corner), L.stream())),
            "classes_one_probe": lambda: L.check(lib.iris_atlas_classes(L.ptr(S), F, report["j"], R, L.ptr(k), L.ptr(hist), L.stream())),
            "rank_torch_stable_sort": lambda: torch.sort(k, stable=True),
            "place": lambda: L.check(lib.iris_atlas_place(L.ptr(k), L.ptr(corner), L.ptr(order), F, R, h, L.ptr(out_vt), L.stream()))}
    res["kernels_ms"] = {name: med(event_ms(fn, args.steps, args.warmup)) for name, fn in kern.items()}
    assert torch.equal(out_vt.view(torch.int32), vt.view(torch.int32))
    with L.StageTimer() as timer:
        T.area_atlas(v_d, f_d, R)
    res["stages_ms_one_call"] = {name: round(x, 4) for name, x in timer.ms().items()}
    res["stages_note"] = "event to event on the stream: 'classes' sums the probes of the bisection and holds the host's read of 16 counters after each"

    # texels per face under the two atlases, and the dilation
    share = np.sqrt(report["D_j"]) * np.sqrt(A.measure(v, f)[0]) / 2
    m = T.UVMesh(vt, ft, v_d, f_d, R)
    ids = m.raster()
    res["texels_area_atlas"] = texel_table(ids, F, share)
    g_vt, g_ft = grid_arm()
    res["texels_grid_atlas"] = texel_table(T.UVMesh(g_vt, g_ft, v_d, f_d, R).raster(), F, share)
    img_a = torch.randint(0, 256, (R, R, 3), dtype=torch.uint8, device=dev); img_rm = torch.randint(0, 256, (R, R, 3), dtype=torch.uint8, device=dev)
    res["dilate_n2_ms"] = med(event_ms(lambda: T.dilate_into(ids, img_a, img_rm, 2), args.steps, args.warmup))
    res["dilate_uncovered_share"] = round(float((ids < 0).float().mean()), 4)

    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
