#!/usr/bin/env python3
"""End-to-end wall clock of the bake_shading CLI (reference: bake_shading.py as run by scripts/*/train.sh): the bench workload written
to disk in the reference's file formats and ScanNet++ layout (data/<scene>/scans/scene.ply, data/<scene>/psdf/{train_test_lists,transforms_all}.json, vslf.npz, emitter.pth), then `python -m iris_amd.bake_shading` over a
sequence of 1080p views -- mesh load + BVH build, per view rays / primary hits / 7-lobe bake / denoise, 13 EXR files per view.
bench.py times the path with inputs resident in HBM; this is the number a user of the CLI sees.  One JSON line per configuration.

    python tools/bench_cli.py [--views 8] [--tris 1000000] [--out /tmp/iris_cli] [--configs zip:atrous:host,zip:atrous:device,none:atrous] [--repeat 2]

A configuration is compression:denoise[:exr_encoder] (encoder host by default); --repeat runs the whole list that many times, alternating.
"""
import argparse
import json
import os
import shutil
import struct
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def write_ply(path, v, f):
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                  "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f))).encode())
        fh.write(np.ascontiguousarray(v, "<f4").tobytes())
        rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", 3)])
        rec["n"] = 3; rec["i"] = f
        fh.write(rec.tobytes())


def usable_cpus():
    """what this process may actually run on: its affinity mask and the cgroup's CPU quota (cpu.max; bench.py's cpu_baseline reads the same)"""
    try:
        aff = len(os.sched_getaffinity(0))
    except Exception:     # noqa
        aff = None
    cpu_max, quota = None, None
    for f in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            cpu_max = open(f).read().strip(); break
        except Exception:     # noqa
            pass
    try:
        q, per = cpu_max.split()[:2]
        quota = None if q == "max" else round(float(q) / float(per), 2)
    except Exception:     # noqa
        pass
    return {"sched_getaffinity": aff, "cgroup_cpu_max": cpu_max, "cgroup_cpus": quota}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--slf-res", type=int, default=256)
    ap.add_argument("--out", type=str, default="/tmp/iris_cli")
    ap.add_argument("--configs", type=str, default="zip:atrous,none:atrous,none:none")
    ap.add_argument("--repeat", type=int, default=1, help="passes over --configs (alternated: A B C A B C ...)")
    args = ap.parse_args()
    from tools import synth
    shutil.rmtree(args.out, ignore_errors=True)
    SCENE = "bench0room"                                               # the ScanNet++ layout the reference's scripts run on: <root>/data/<scene>/{scans/scene.ply, psdf/*.json}
    scene_dir = os.path.join(args.out, "data", SCENE, "scans"); os.makedirs(scene_dir)
    psdf_dir = os.path.join(args.out, "data", SCENE, "psdf"); os.makedirs(psdf_dir)
    t0 = time.time()
    room = synth.room(1, args.tris)
    v, f = room["vertices"].astype(np.float32), room["faces"].astype(np.int32)
    write_ply(os.path.join(scene_dir, "scene.ply"), v, f)
    slf = synth.slf_for(v, f, H=args.slf_res)
    emi = synth.emitters_for(v, f, room["is_emitter"])
    from iris_amd.model.slf import VoxelSLF
    vs = VoxelSLF(torch.from_numpy(slf["mask"]), float(slf["voxel_min"]), float(slf["voxel_max"]))
    vs.radiance[:] = torch.from_numpy(slf["radiance"])
    slf_path, emi_path = os.path.join(args.out, "vslf.npz"), os.path.join(args.out, "emitter.pth")
    torch.save({"mask": torch.from_numpy(slf["mask"]), "voxel_min": float(slf["voxel_min"]), "voxel_max": float(slf["voxel_max"]), "weight": vs.state_dict()}, slf_path)
    torch.save({"is_emitter": torch.from_numpy(emi["is_emitter"]), "emitter_vertices": torch.from_numpy(emi["emitter_vertices"]),
                "emitter_area": torch.from_numpy(emi["emitter_area"]), "emitter_normal": torch.zeros(len(emi["emitter_area"]), 3),
                "emitter_radiance": torch.from_numpy(emi["emitter_radiance"])}, emi_path)
    H, W = args.height, args.width
    names, frames, K0 = [], [], None
    for i in range(args.views):
        K, c2w = synth.camera(H, W, (i * 32) // args.views, n_views=32)
        K0 = np.asarray(K, np.float64)
        m = np.eye(4); m[:3, :4] = np.asarray(c2w, np.float64); m[:3, 1:3] *= -1          # OpenCV -> the OpenGL convention transforms_all.json stores
        names.append("DSC%05d.JPG" % i)
        frames.append({"file_path": "images/" + names[-1], "transform_matrix": m.tolist()})
    json.dump({"train": names, "test": []}, open(os.path.join(psdf_dir, "train_test_lists.json"), "w"))
    json.dump({"fl_x": float(K0[0, 0]), "fl_y": float(K0[1, 1]), "cx": float(K0[0, 2]), "cy": float(K0[1, 2]), "h": H, "w": W, "frames": frames[::-1]},        # (stored out of order: the LIST decides)
              open(os.path.join(psdf_dir, "transforms_all.json"), "w"))
    print("# dataset written in %.1f s: %d triangles, %d views of %dx%d" % (time.time() - t0, len(f), args.views, W, H), file=sys.stderr)

    for cfg in args.configs.split(",") * max(1, args.repeat):
        comp, den, enc = (cfg.split(":") + ["host"])[:3]
        out_dir = os.path.join(args.out, "shading_" + cfg.replace(":", "_"))
        # scripts/scannetpp/bathroom2/train.sh:49-54's argument list (+ the two additions under test)
        cmd = [sys.executable, "-m", "iris_amd.bake_shading", "--dataset_root", args.out, "--scene", SCENE, "--dataset", "scannetpp", "--res_scale", "1.0",
               "--slf_path", slf_path, "--emitter_path", emi_path, "--output", out_dir, "--compression", comp, "--denoise", den, "--exr_encoder", enc]
        t = time.time()
        r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        dt = time.time() - t
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            raise SystemExit("bake_shading failed")
        inner = [l for l in r.stdout.splitlines() if l.startswith("[bake_shading]")]
        n_files = sum(len(fs) for _, _, fs in os.walk(out_dir))
        size = sum(os.path.getsize(os.path.join(d, x)) for d, _, fs in os.walk(out_dir) for x in fs)
        from iris_amd import bake_shading as bs
        rays = args.views * H * W * (bs.SPP_DIFFUSE + sum(bs.SPPS_SPECULAR))     # upper bound: every pixel valid
        print(json.dumps({"config": {"compression": comp, "denoise": den, "views": args.views, "image": [W, H], "triangles": int(len(f)), "exr_encoder": enc, "host_cpus": os.cpu_count(), "usable_cpus": usable_cpus(), "command": "python -m iris_amd.bake_shading --dataset_root R --scene S --dataset scannetpp --res_scale 1.0 --slf_path ... --emitter_path ... --output ... (scripts/scannetpp/bathroom2/train.sh:49-54)"},
                          "wall_s": round(dt, 2), "s_per_view_incl_startup": round(dt / args.views, 3), "cli_report": inner[-1] if inner else None,
                          "files": n_files, "bytes_written": size, "upper_bound_Mrays_per_s": round(rays / dt / 1e6, 1)}), flush=True)
        shutil.rmtree(out_dir, ignore_errors=True)
    shutil.rmtree(args.out, ignore_errors=True)


if __name__ == "__main__":
    main()
