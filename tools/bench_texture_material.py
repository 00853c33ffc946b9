#!/usr/bin/env python3
"""What the material costs at the primary hits of one 1080p view, network against exported textures, on the bench scene (the room of bench.py:
seed 1, 1 M triangles, SLF H = 256; the network is NGPBRDF with random parameters, the textures are that network baked with --atlas area at --tex_res, --dilate 2).
The positions are the 2 073 600 primary-hit positions of view 0 (ray_intersect's; a miss contributes the origin it returns).  ONE process, the arms interleaved,
per-call HIP events, medians over --repeats passes after one warm-up pass:
  ngp              NGPBRDF.forward(positions)
  closest_point    utils.closest.closest_point(scene, positions)
  sample_textures  the fetch alone at closest_point's (tri, bary), the tables already on the device
  baked            BakedTextureBRDF.forward(positions): closest triangle, UV and fetch in one launch
  intersect        ray_intersect of the view's rays (iris_intersect on the same count), for scale
Writes profiles/texture_material.json and prints it as one JSON line.  Needs the GPU.  No threshold is set and none is claimed: the reason for the texture
material is that the exported asset can be rendered at all; which of the two is faster is reported either way."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000); ap.add_argument("--height", type=int, default=1080); ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--tex_res", type=int, default=4096); ap.add_argument("--dilate", type=int, default=2); ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "texture_material.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture_material needs the GPU")
    import bench
    from iris_amd import _lib as L
    from iris_amd.model.texture import BakedTextureBRDF
    from iris_amd.utils import texture as T
    from iris_amd.utils.closest import closest_point
    from iris_amd.utils.dataset import real_ldr
    from iris_amd.utils.path_tracing import ray_intersect
    from tools import synth
    from tools.bench_pt_single import ngp_material
    dev = torch.device("cuda:0")
    t0 = time.time()
    room, slf, _, scene, _ = bench.build_workload(SimpleNamespace(scene_seed=1, tris=args.tris, slf_res=256, layout=0, long_walls=False), dev)
    net = ngp_material(slf, dev).to(dev)
    H, W = args.height, args.width
    K, c2w = synth.camera(H, W, 0, n_views=32)
    rays_o, rays_d = real_ldr.to_world(real_ldr.get_direction(K, (H, W)), c2w, False, device=dev)[:2]
    rays_o, rays_d = rays_o.contiguous(), torch.nn.functional.normalize(rays_d, dim=-1).contiguous()
    pos, _, _, _, valid = ray_intersect(scene, rays_o, rays_d)
    v, f = room["vertices"], room["faces"]
    vt, ft, report = T.area_atlas(v, f, args.tex_res, device=dev)
    albedo, rm = T.bake_textures(net, vt, ft, v, f, args.tex_res, device=dev, dilate=args.dilate)
    baked = BakedTextureBRDF(scene, ft, vt, albedo, rm)
    tri, bary, _, dist2 = closest_point(scene, pos)
    torch.cuda.synchronize()
    print("# workload, atlas and bake in %.1f s" % (time.time() - t0), file=sys.stderr, flush=True)

    arms = {
        "ngp": lambda: net(pos),
        "closest_point": lambda: closest_point(scene, pos),
        "sample_textures": lambda: baked.sample(tri, bary),
        "baked": lambda: baked(pos),
        "intersect": lambda: ray_intersect(scene, rays_o, rays_d),
    }
    times = {k: [] for k in arms}
    with torch.no_grad():
        for rep in range(args.repeats + 1):                    # pass 0 warms every arm up
            for name, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1))
        one, two = baked(pos), baked.sample(tri, bary)
        same = all(torch.equal(one[k], two[k]) for k in one)
        want = net(pos)
        hit = valid.reshape(-1)
        psnr = {k: float(-10 * torch.log10(((want[k].reshape(one[k].shape)[hit] - one[k][hit]).double() ** 2).mean())) for k in one}
    n = int(pos.shape[0])
    result = {"device": torch.cuda.get_device_name(0), "build": L.build_id(), "triangles": int(scene.info()["n_triangles"]), "bvh_depth": int(scene.info()["depth"]),
              "positions": n, "primary_hits": int(valid.sum()), "tex_res": args.tex_res, "dilate": args.dilate, "atlas": {k: report[k] for k in ("j", "used", "histogram")},
              "repeats": args.repeats, "largest_sqrt_dist2_of_a_hit": float(dist2[hit].max().sqrt()),
              "one_launch_equals_two_calls": bool(same), "psnr_db_textures_against_network_at_the_hits": psnr,
              "ms": {k: {"median": median(t), "min": min(t), "max": max(t)} for k, t in times.items()},
              "positions_per_s": {k: n / (median(t) * 1e-3) for k, t in times.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
