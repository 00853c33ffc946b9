#!/usr/bin/env python3
"""Measurements for the trainers' validation (iris_amd/utils/validation.py, iris_amd/csrc/iris_validate.h) on the bench scene (the
1.0 M-triangle room; material = the reference's NGPBRDF with random parameters) with views of 1080 x 1920, everything in ONE process, HIP events, the
arms of a comparison interleaved call by call after warm-up calls of each; median, minimum and maximum of --steps calls.

  loss         kd_validation_loss (fused HIP, both launches and the float64 epilogue) of a stack of --views views, in the ldr and the synthetic mode,
               beside the reference's lines (train_brdf_crf.py:459-494) run as torch operations on the device, one view at a time as Lightning runs them
  intrinsics   validation_intrinsics (iris_render_primary + the material network + iris_val_intrinsics) of one view at --spp, beside its composition from
               the public calls as train_brdf_crf.py:372-396 writes it, in the same pixel chunks
  evaluate     ValidationSet.evaluate per view, split into its three parts: the trace (once, at construction), the material network, the metric

The fused loss must agree with the torch lines to the float32 mean's error, or nothing is written.  The measurement runs in a fresh child process under
`timeout`; its one JSON line goes to --out (default profiles/validation_1080p.json)."""
import argparse, json, os, statistics, subprocess, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 1080, 1920


def torch_loss(albedo_net, metallic_net, valid, rgb_or_kd, emission):
    """train_brdf_crf.py:459-494 for one view on the device; emission None: the real layouts' branch"""
    import torch
    import torch.nn.functional as NF
    emission_mask_gt = torch.ones_like(metallic_net) if emission is None else emission.mean(-1, keepdim=True) == 0
    albedo_ = albedo_net[valid] * (1 - metallic_net[valid])
    albedo = torch.zeros(len(valid), 3, device=valid.device)
    albedo[valid] = albedo_
    albedo_gt = rgb_or_kd.pow(1 / 2.2).clamp(0, 1) if emission is None else rgb_or_kd
    loss_c = NF.mse_loss(albedo_gt * emission_mask_gt, albedo * emission_mask_gt)
    return loss_c, -10.0 * torch.log10(loss_c.clamp_min(1e-5))


def composed_intrinsics(scene, emitter, material_net, rays_o, rays_d, dxdu, dydv, spp, out, chunk):
    """train_brdf_crf.py:372-396 out of the public calls: ray_intersect, the network, eval_emitter and torch glue"""
    import torch
    import torch.nn.functional as NF
    from iris_amd.utils.path_tracing import ray_intersect
    dev = rays_o.device
    for b0 in range(0, rays_o.shape[0], chunk):
        b1 = min(b0 + chunk, rays_o.shape[0])
        du, dv = torch.rand(2, b1 - b0, spp, 1, device=dev)
        ds = NF.normalize(rays_d[b0:b1, None] + dxdu[b0:b1, None] * du + dydv[b0:b1, None] * dv, dim=-1).reshape(-1, 3)
        xs = rays_o[b0:b1].repeat_interleave(spp, dim=0)
        positions, _, _, tri, valid = ray_intersect(scene, xs, ds)
        mat = material_net(positions)
        emission_ = emitter.eval_emitter(positions, ds, tri)[0]
        keep = (valid.unsqueeze(-1) * (emission_.sum(-1, keepdim=True) == 0))
        for k, x, c in (("albedo", mat["albedo"] * keep, 3), ("roughness", mat["roughness"].reshape(-1, 1) * keep, 1),
                        ("metallic", mat["metallic"].reshape(-1, 1) * keep, 1), ("emission", emission_, 3)):
            out[k][b0:b1] += x.reshape(-1, spp, c).mean(1)
    return out


def interleaved(arms, steps, warmup):
    """{name: fn} -> {name: [ms per call]}: HIP events around every call, the arms taking turns"""
    import torch
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(steps):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return ms


def summary(ms):
    return {name: {"ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]} for name, v in ms.items()}


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import bench
    from iris_amd import _lib as L
    from iris_amd.utils.dataset import real_ldr
    from iris_amd.utils.path_tracing import ray_intersect
    from iris_amd.utils.render import CHUNK_SAMPLES
    from iris_amd.utils.validation import ValidationSet, kd_validation_loss, new_maps, validation_intrinsics
    from tools import synth
    from tools.bench_pt_single import ngp_material
    if not torch.cuda.is_available():
        raise SystemExit("bench_validation needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    ns = argparse.Namespace(scene_seed=1, tris=args.tris, slf_res=256, layout=0)
    room, slf, emi, scene, emitter = bench.build_workload(ns, dev)
    emitter = emitter.to(dev) if hasattr(emitter, "to") else emitter
    net = ngp_material(slf, dev)
    V, hw = args.views, H * W
    views = []
    for i in range(V):
        K, c2w = synth.camera(H, W, i)
        views.append(dict(kind="real", K=np.asarray(K, np.float32), c2w=np.asarray(c2w, np.float32)[:3, :4]))
    g = torch.Generator().manual_seed(2024)
    codes = torch.randint(0, 256, (V, H, W, 3), generator=g, dtype=torch.uint8)
    diffcol = torch.rand(V, H, W, 3, generator=g)
    emit = (torch.rand(V, H, W, 1, generator=g) < 0.1).float() * torch.rand(V, H, W, 3, generator=g)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    vs = ValidationSet(views, (H, W), codes, np.ones(V, np.float32), scene, device=dev)          # (warm-up of the trace)
    e0.record()
    vs = ValidationSet(views, (H, W), codes, np.ones(V, np.float32), scene, device=dev)
    e1.record(); torch.cuda.synchronize()
    construct_ms = e0.elapsed_time(e1)
    syn = ValidationSet(views[:1], (H, W), codes[:1], np.ones(1, np.float32), scene, diffcol=diffcol[:1], emit=emit[:1], device=dev)
    diffcol, emit = diffcol.to(dev).reshape(V, hw, 3), emit.to(dev).reshape(V, hw, 3)

    # ---- the loss: the fused stack beside the reference's lines per view
    with torch.no_grad():
        mat = net(vs.positions.reshape(-1, 3))
    albedo, metallic = mat["albedo"].reshape(V, hw, 3).contiguous(), mat["metallic"].reshape(V, hw, 1).contiguous()
    rgb = vs.codes.to(torch.float32) / 255
    arms = {"fused_ldr": lambda: kd_validation_loss(albedo, metallic, vs.valid, codes=vs.codes, img_hw=(H, W)),
            "torch_ldr": lambda: [torch_loss(albedo[i], metallic[i], vs.valid[i], rgb[i], None) for i in range(V)],
            "fused_synthetic": lambda: kd_validation_loss(albedo, metallic, vs.valid, gt=diffcol, emit=emit, img_hw=(H, W)),
            "torch_synthetic": lambda: [torch_loss(albedo[i], metallic[i], vs.valid[i], diffcol[i], emit[i]) for i in range(V)],
            "fused_ldr_N1": lambda: kd_validation_loss(albedo[:1], metallic[:1], vs.valid[:1], codes=vs.codes[:1], img_hw=(H, W))}
    agree = {}
    for mode in ("ldr", "synthetic"):
        fused = arms["fused_" + mode]()["loss"].cpu().numpy()
        ref = np.array([float(l) for l, _ in arms["torch_" + mode]()], np.float64)
        bound = fused * 3 * hw * 2.0 ** -24 + (2 * np.sqrt(fused) * 2.0 ** -23 + 2.0 ** -46 if mode == "ldr" else 0.0)
        agree[mode] = {"fused": fused.tolist(), "torch_float32": ref.tolist(), "max_difference_over_bound": float((np.abs(fused - ref) / bound).max())}
        if not (np.abs(fused - ref) <= bound).all():
            raise SystemExit(f"bench_validation: the fused {mode} loss {fused.tolist()} and the torch lines {ref.tolist()} differ by more than the float32 mean's error; nothing written")
    loss_ms = summary(interleaved(arms, args.steps, args.warmup))
    for mode in ("ldr", "synthetic"):
        f, t = loss_ms["fused_" + mode], loss_ms["torch_" + mode]
        loss_ms["torch_over_fused_" + mode] = round(t["ms"] / f["ms"], 3)
        loss_ms["fused_beats_torch_beyond_the_spread_" + mode] = bool(f["min_max_ms"][1] < t["min_max_ms"][0])

    # ---- the intrinsics of one view
    K, c2w = synth.camera(H, W, 0)
    rays = real_ldr.to_world(real_ldr.get_direction(K, (H, W)), c2w, True, K, device=dev)
    spp, chunk = args.spp, max(1, CHUNK_SAMPLES // args.spp)
    maps, maps2 = new_maps(hw, dev), new_maps(hw, dev)
    arms = {"fused": lambda: validation_intrinsics(scene, emitter, net, *rays, spp, out=maps),
            "composed": lambda: composed_intrinsics(scene, emitter, net, *rays, spp, maps2, chunk)}
    intr_ms = summary(interleaved(arms, args.intrinsics_steps, 1))
    intr_ms["composed_over_fused"] = round(intr_ms["composed"]["ms"] / intr_ms["fused"]["ms"], 3)
    with L.StageTimer() as tm:
        validation_intrinsics(scene, emitter, net, *rays, spp, out=maps)
    intr_ms["fused_stages_ms"] = {k: round(v, 3) for k, v in sorted(tm.ms().items(), key=lambda kv: -kv[1])}

    # ---- evaluate, per view, by part
    o, d = rays[0], torch.nn.functional.normalize(rays[1], dim=-1)
    pos1, valid1 = vs.positions[:1].reshape(hw, 3), vs.valid[:1]

    def network():
        with torch.no_grad():
            return net(pos1)
    m1 = network()
    a1, me1 = m1["albedo"].contiguous(), m1["metallic"].contiguous()
    arms = {"trace": lambda: ray_intersect(scene, o, d), "network": network,
            "metric": lambda: kd_validation_loss(a1, me1, valid1, codes=vs.codes[:1], img_hw=(H, W)),
            "evaluate_all_views": lambda: vs.evaluate(None, net), "evaluate_synthetic_one_view": lambda: syn.evaluate(None, net)}
    eval_ms = summary(interleaved(arms, args.steps, args.warmup))
    eval_ms["evaluate_per_view_ms"] = round(eval_ms["evaluate_all_views"]["ms"] / V, 4)
    a, b = vs.evaluate(None, net), vs.evaluate(None, net)
    out = {"what": f"the trainers' validation on {V} views of {W} x {H} of the bench room ({args.tris} triangles), NGPBRDF with random parameters: medians of per-call "
                   "HIP event times in one process, the arms of a comparison interleaved call by call",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "views": V, "H": H, "W": W, "steps": args.steps, "warmup": args.warmup,
           "loss": loss_ms, "loss_agreement": agree, "loss_bytes_read_ldr": V * hw * (12 + 4 + 1 + 3), "loss_bytes_read_synthetic": V * hw * (12 + 4 + 1 + 12 + 12),
           "intrinsics": dict(intr_ms, spp=spp, steps=args.intrinsics_steps, samples=hw * spp, chunk_pixels=chunk),
           "evaluate": dict(eval_ms, construct_all_views_ms=round(construct_ms, 3), two_calls_equal_bits=bool(torch.equal(a["val/loss"], b["val/loss"]))),
           "note": "call times include the host's launches, allocations and the float64 epilogue; the torch arms run the reference's lines per view, as Lightning "
                   "does; construct_all_views_ms is ray generation + the trace + the uploads of all views, paid once per run; one run on one box"}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--intrinsics_steps", type=int, default=5); ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--views", type=int, default=4); ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--timeout", type=int, default=480, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "validation_1080p.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"]
    for k in ("steps", "warmup", "intrinsics_steps", "spp", "views", "tris"):
        cmd += ["--" + k, str(getattr(args, k))]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stdout.write(p.stdout)
        raise SystemExit(f"bench_validation: the measurement ended with status {p.returncode}; nothing written")
    line = lines[-1][len("RESULT "):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
