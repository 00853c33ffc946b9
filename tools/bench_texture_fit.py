#!/usr/bin/env python3
"""What one step of the texture fit costs, on the bench scene (the room of bench.py: seed 1, 1 M triangles, SLF H = 256; the network is NGPBRDF
with random parameters; the textures are that network baked with --atlas area at --tex_res, --dilate 2) at --points surface points per step, drawn
area-proportionally (utils.texture.surface_draw).  ONE process, the arms interleaved, per-call HIP events, medians over --repeats passes after one warm-up pass:
  draw           surface_draw's (face, bary) of one step
  target         the positions and NGPBRDF.forward at them (what the fit is fitted to)
  fetch          TextureBRDF.sample under no_grad: iris_texture_sample_f32
  backward       iris_texture_sample_f32_bwd alone, into a gradient buffer that is not zeroed in between (twenty float atomics per point)
  zero           zeroing that buffer
  adam           FusedAdam.step on the (H, W, 5) texels
  fit_step       utils.texture.fit_step: target, fetch, loss, backward, Adam
  torch_step     the same step with the fetch composed from torch operations (four gathers, the lerps; autograd's index_put_(accumulate=True)) and torch.optim.Adam
Also: the backward's atomic bytes per second (20 adds of 4 bytes per point) against the chip-wide rate of about 1.3 TB/s for well-shaped float atomics; how many of
a wave's 256 taps share a texel with another tap of the wave (what summing in the wave before the atomic could save); and export's --verify PSNR before and
after --fit_steps steps at --fit_lr.  The network has RANDOM parameters, white noise at the scale of the atlas's texels: the PSNR pair says nothing about a trained
network.  Writes profiles/texture_fit.json and prints it as one JSON line.  Needs the GPU.  No threshold is set and none is claimed."""
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

ATOMIC_RATE = 1.3e12            # bytes per second of float atomic adds, chip-wide, for 256-byte wave-instructions spread over many rows


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def torch_fetch(texels, ft, vt, face, bary):
    """the fetch's arithmetic in torch operations -> (B, 5); differentiable with respect to texels through the four gathers"""
    H, W = texels.shape[:2]
    b1, b2 = bary[:, :1], bary[:, 1:]
    i = ft[face].long()
    uv = ((1.0 - b1) - b2) * vt[i[:, 0]] + b1 * vt[i[:, 1]] + b2 * vt[i[:, 2]]
    x, y = (uv[:, 0] * W - 0.5).clamp(0, W - 1), (uv[:, 1] * H - 0.5).clamp(0, H - 1)
    x0, y0 = x.floor(), y.floor()
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    flat = texels.reshape(H * W, 5)
    t00, t01, t10, t11 = flat[y0 * W + x0], flat[y0 * W + x1], flat[y1 * W + x0], flat[y1 * W + x1]
    top, bot = t00 + fx * (t01 - t00), t10 + fx * (t11 - t10)
    out = top + fy * (bot - top)
    return torch.cat([out[:, :3], out[:, 3:4].clamp(min=0.02), out[:, 4:]], 1), (y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000); ap.add_argument("--tex_res", type=int, default=4096); ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--points", type=int, default=1 << 20); ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--fit_steps", type=int, default=200); ap.add_argument("--fit_lr", type=float, default=5e-3); ap.add_argument("--verify", type=int, default=1 << 20)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "texture_fit.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture_fit needs the GPU")
    import bench
    from iris_amd import _lib as L
    from iris_amd.model.texture import BakedTextureBRDF, TextureBRDF
    from iris_amd.utils import export as E, texture as T
    from iris_amd.utils.optim import FusedAdam
    from tools.bench_pt_single import ngp_material
    dev = torch.device("cuda:0")
    t0 = time.time()
    room, slf, _, scene, _ = bench.build_workload(SimpleNamespace(scene_seed=1, tris=args.tris, slf_res=256, layout=0, long_walls=False), dev)
    net = ngp_material(slf, dev).to(dev)
    v, f = room["vertices"], room["faces"]
    vt, ft, report = T.area_atlas(v, f, args.tex_res, device=dev)
    albedo, rm = T.bake_textures(net, vt, ft, v, f, args.tex_res, device=dev, dilate=args.dilate)
    tex = TextureBRDF(scene, ft, vt, albedo, rm)
    v_d, f_d = T._upload(v, torch.float32, dev).reshape(-1, 3), T._upload(f, torch.int64, dev).reshape(-1, 3)
    draw = T.surface_draw(v, f, args.points, 0, dev)
    face, bary = draw(0)
    B = int(face.shape[0])
    torch.cuda.synchronize()
    print("# workload, atlas and bake in %.1f s" % (time.time() - t0), file=sys.stderr, flush=True)

    def positions(face, bary):
        b1, b2 = bary[:, :1], bary[:, 1:]
        p0, p1, p2 = (v_d[f_d[face, k]] for k in range(3))
        return ((1.0 - b1 - b2) * p0 + b1 * p1) + b2 * p2

    # ---- the timing arms work on copies: the fit below starts from the baked texels
    timed = TextureBRDF(scene, ft, vt, albedo, rm)
    opt = FusedAdam([timed.texels], lr=args.fit_lr)
    g = torch.randn(B, 5, device=dev) * (2.0 / (5 * B))
    ga, gr, gm = g[:, :3].contiguous(), g[:, 3].contiguous(), g[:, 4].contiguous()
    grad = torch.zeros_like(timed.texels)
    timed.texels.grad = torch.randn_like(timed.texels) * 1e-6
    t_param = torch.nn.Parameter(timed.texels.detach().clone())
    t_opt = torch.optim.Adam([t_param], lr=args.fit_lr)

    def backward_only():
        L.check(L.lib().iris_texture_sample_f32_bwd(L.ptr(face), L.ptr(bary), B, *timed._args(timed.texels), L.ptr(ga), L.ptr(gr), L.ptr(gm), L.ptr(grad), L.stream()))

    def no_grad_fetch():
        with torch.no_grad():
            timed.sample(face, bary)

    def target():
        with torch.no_grad():
            net(positions(face, bary))

    def torch_step():
        with torch.no_grad():
            want = net(positions(face, bary))
            want = torch.cat([want["albedo"].reshape(-1, 3), want["roughness"].reshape(-1, 1), want["metallic"].reshape(-1, 1)], 1)
        got, _ = torch_fetch(t_param, timed.ft, timed.vt, face, bary)
        loss = ((got - want) ** 2).mean()
        t_opt.zero_grad(set_to_none=True)
        loss.backward()
        t_opt.step()

    arms = {
        "draw": lambda: draw(1),
        "target": target,
        "fetch": no_grad_fetch,
        "backward": backward_only,
        "zero": lambda: grad.zero_(),
        "adam": lambda: opt.step(),
        "fit_step": lambda: T.fit_step(net, timed, opt, v_d, f_d, face, bary),
        "torch_step": torch_step,
    }
    times = {k: [] for k in arms}
    for rep in range(args.repeats + 1):                        # pass 0 warms every arm up
        for name, fn in arms.items():
            if name == "adam" and timed.texels.grad is None:
                timed.texels.grad = torch.randn_like(timed.texels) * 1e-6
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1))
    # the torch fetch agrees with the kernel (a check of the arm, not of the kernel: tests/test_texture_fit.py is that)
    with torch.no_grad():
        a = timed.sample(face, bary)
        b, taps = torch_fetch(timed.texels, timed.ft, timed.vt, face, bary)
        torch_arm_max_diff = float((torch.cat([a["albedo"], a["roughness"], a["metallic"]], 1) - b).abs().max())
        # taps of a wave (64 consecutive points x 4) that fall on a texel another tap of the wave also falls on
        n_w = B // 64
        ids = torch.stack(taps, 1)[:n_w * 64].reshape(n_w, 256).sort(dim=1)[0]
        shared = float((ids[:, 1:] == ids[:, :-1]).float().sum() / ids.numel())
    del timed, opt, t_param, t_opt, grad
    torch.cuda.empty_cache()

    # ---- --verify before and after the fit, at export's own points
    def psnr(albedo_img, rm_img):
        _, _, pos = E.verify_points(v, f, args.verify)
        pos = torch.from_numpy(pos).to(dev)
        with torch.no_grad():
            want, got = net(pos), BakedTextureBRDF(scene, ft, vt, albedo_img, rm_img)(pos)
        return {k: E._psnr(want[k].reshape(got[k].shape), got[k]) for k in ("albedo", "roughness", "metallic")}
    before = psnr(albedo, rm)
    t0 = time.time()
    fit = T.fit_textures(net, tex, v, f, args.fit_steps, args.points, args.fit_lr, seed=0)
    torch.cuda.synchronize()
    fit_seconds = time.time() - t0
    after = psnr(*tex.to_images())
    rounded_only = psnr(*TextureBRDF(scene, ft, vt, albedo, rm).to_images())          # (the baked bytes themselves: to_images is the identity on them)

    ms = {k: {"median": median(t), "min": min(t), "max": max(t)} for k, t in times.items()}
    atomic_bytes = B * 20 * 4
    result = {"device": torch.cuda.get_device_name(0), "build": L.build_id(), "triangles": int(scene.info()["n_triangles"]), "tex_res": args.tex_res,
              "dilate": args.dilate, "atlas": {k: report[k] for k in ("j", "used", "histogram")}, "points": B, "repeats": args.repeats, "ms": ms,
              "backward_atomic_bytes": atomic_bytes, "backward_atomic_bytes_per_s": atomic_bytes / (ms["backward"]["median"] * 1e-3),
              "chip_wide_atomic_rate_bytes_per_s": ATOMIC_RATE, "backward_share_of_the_chip_wide_rate": atomic_bytes / (ms["backward"]["median"] * 1e-3) / ATOMIC_RATE,
              "share_of_a_waves_taps_on_a_texel_shared_in_the_wave": shared, "torch_arm_largest_difference_from_the_kernel": torch_arm_max_diff,
              "fit": {"steps": args.fit_steps, "lr": args.fit_lr, "first_loss": fit["first_loss"], "last_loss": fit["last_loss"], "seconds": fit_seconds},
              "verify_points": args.verify, "psnr_db_before_the_fit": before, "psnr_db_after_the_fit": after, "psnr_db_of_the_baked_bytes_through_to_images": rounded_only,
              "note": "the network has random parameters: the PSNR pair says nothing about a trained network"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
