#!/usr/bin/env python3
"""Measurements for the render stage on the bench scene (1.0 M-triangle room; material = the reference's NGPBRDF with random parameters,
--material stub for the closed-form stand-in): one 1080p view, spp 32, HIP events, everything in ONE process.
  fused     render_intrinsics: iris_render_primary + the material network + iris_render_intrinsics per chunk of pixels, with a stage table
  composed  the same six maps from the calls the package had before the stage existed, as render.py:178-220 writes them: torch jitter, repeat_interleave,
            ray_intersect, the network, BaseBRDF.sample_specular (kept for g0, g1 alone), eval_emitter, VoxelSLF.forward, three mask assignments, six
            reshape().mean(1) -- in the same pixel chunks (the reference holds a whole view at once: 66 M samples x ~400 B of intermediates)
  view      render_view: the path-traced image + the intrinsics + denoiser + CRF, per view
Writes profiles/render_bench.json and prints it as one JSON line."""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch


def composed_intrinsics(scene, emitter, material_net, rays_o, rays_d, dxdu, dydv, spp, out, chunk):
    """render.py:178-220 out of the public calls: ray_intersect, sample_specular, eval_emitter, VoxelSLF.forward and torch glue"""
    import torch.nn.functional as NF
    from iris_amd.model.brdf import BaseBRDF
    from iris_amd.utils.path_tracing import ray_intersect
    brdf, dev = BaseBRDF(), rays_o.device
    for b0 in range(0, rays_o.shape[0], chunk):
        b1 = min(b0 + chunk, rays_o.shape[0])
        du, dv = torch.rand(2, b1 - b0, spp, 1, device=dev)
        ds = NF.normalize(rays_d[b0:b1, None] + dxdu[b0:b1, None] * du + dydv[b0:b1, None] * dv, dim=-1).reshape(-1, 3)
        xs = rays_o[b0:b1].repeat_interleave(spp, dim=0)
        positions, normals, _, tri, valid = ray_intersect(scene, xs, ds)
        mat = material_net(positions)
        albedo_, metallic_, roughness_ = mat["albedo"], mat["metallic"].clone(), mat["roughness"].clone()
        kd_ = albedo_ * (1 - metallic_)
        ks_ = 0.04 * (1 - metallic_) + albedo_ * metallic_
        _, _, g0, g1 = brdf.sample_specular(torch.rand(len(metallic_), 2, device=dev), -ds, normals, roughness_)
        a_prime_ = g0 * ks_ + g1 + kd_
        emission_ = emitter.eval_emitter(positions, ds, tri)[0]
        slf_ = emitter(positions)
        keep = torch.logical_and(valid, emission_.sum(-1) == 0)
        kd_[~keep] = 1.0; a_prime_[~keep] = 1.0; roughness_[~keep] = 1.0; metallic_[~keep] = 0.0
        for k, x, c in (("kd", kd_, 3), ("a_prime", a_prime_, 3), ("roughness", roughness_, 1), ("metallic", metallic_, 1), ("emission", emission_, 3), ("slf", slf_, 3)):
            out[k][b0:b1] += x.reshape(-1, spp, c).mean(1)
    return out


def timed(fn, repeats):
    """median of `repeats` HIP-event timings of fn() in ms, after one warm-up call"""
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=32); ap.add_argument("--tris", type=int, default=1_000_000); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--material", choices=["ngp", "stub"], default="ngp"); ap.add_argument("--indir_depth", type=int, default=5)
    ap.add_argument("--no-view", action="store_true", help="skip the render_view measurement")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "render_bench.json"))
    args = ap.parse_args()
    import bench
    from iris_amd import _lib as L_
    from iris_amd.render import render_view
    from iris_amd.utils.dataset import real_ldr
    from iris_amd.utils.render import CHUNK_SAMPLES, MAPS, new_maps, render_intrinsics
    from tools import synth
    from tools.bench_pt_single import GpuStub, ngp_material
    from tools.bench_refine import TimedMaterial
    dev = torch.device("cuda:0")
    ns = argparse.Namespace(scene_seed=1, tris=args.tris, slf_res=256, layout=0)
    room, slf, emi, scene, emitter = bench.build_workload(ns, dev)
    emitter = emitter.to(dev) if hasattr(emitter, "to") else emitter
    H, W, spp = 1080, 1920, args.spp
    K, c2w = synth.camera(H, W, 0)
    rays = real_ldr.to_world(real_ldr.get_direction(K, (H, W)), c2w, True, K, device=dev)
    net = ngp_material(slf, dev) if args.material == "ngp" else GpuStub()
    B, chunk = H * W, max(1, CHUNK_SAMPLES // spp)
    maps = new_maps(B, dev)
    fused_ms, fused_all = timed(lambda: render_intrinsics(scene, emitter, net, *rays, spp, out=maps), args.repeats)
    with L_.StageTimer() as tm:
        render_intrinsics(scene, emitter, net, *rays, spp, out=maps)
    stages = {k: round(v, 3) for k, v in sorted(tm.ms().items(), key=lambda kv: -kv[1])}
    maps2 = new_maps(B, dev)
    comp_ms, comp_all = timed(lambda: composed_intrinsics(scene, emitter, net, *rays, spp, maps2, chunk), args.repeats)
    N = B * spp
    row = {"case": f"one {W} x {H} view of the bench room ({args.tris} triangles), spp {spp}: {N} samples per round, chunks of {chunk} pixels; material {args.material}",
           "fused_intrinsics": {"ms": round(fused_ms, 2), "all_ms": [round(x, 2) for x in fused_all], "Msamples_per_s": round(N / fused_ms / 1e3, 1), "stages_ms": stages,
                                "kernel_GB_per_s_at_69_B_per_sample": round(N * 69 / max(stages.get("intrinsics kernel", float("nan")), 1e-9) / 1e6, 1)},
           "composed_from_public_calls": {"ms": round(comp_ms, 2), "all_ms": [round(x, 2) for x in comp_all], "Msamples_per_s": round(N / comp_ms / 1e3, 1)},
           "composed_over_fused": round(comp_ms / fused_ms, 3)}
    if not args.no_view:
        t = TimedMaterial(net)
        view_ms, view_all = timed(lambda: render_view(scene, emitter, t, None, rays, (H, W), spp, spp, args.indir_depth), 1)
        row["render_view"] = {"ms_per_view": round(view_ms, 1), "SPP": spp, "spp": spp, "indir_depth": args.indir_depth, "denoiser": "atrous", "crf": "none (no EMoR file on the bench box)"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(row, fh, indent=1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
