#!/usr/bin/env python3
"""The trainers' pixel batch (iris_amd.utils.dataset.PixelSet.gather: one iris_pixel_batch launch on 8-bit stores and a camera table) against the
reference's layout held on the same GPU, in one process: ``index_select`` on the float (N,16) table [rays_x | rays_d | dxdu | dydv | segmentation |
rgb] (utils/dataset/real_ldr.py:351-354), on the (N,3) albedo table and on the (N,1) exposure table (:386), sliced as __getitem__ does (:418-427).

Shape: --views (default 16) real views of 1080 x 1920 pixels, random ids without repetition; B = 8192 (the trainers' batch: latency-bound, a time
per call with the host's launches) and B = 2^21 (about one view: bandwidth-bound).  Timed under HIP events: one window over the steps after a
warm-up; each arm twice, the fused one around the other, so that the spread of the same code in one process stands beside the ratio.
Also reported: resident bytes per pixel of both layouts (without the shading cache, which neither arm reads here: 39 floats per pixel in the
reference's table, a 160-B row in ShadingCache).
Writes one JSON object (and prints it): --out, default profiles/pixel_batches.json.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

H, W = 1080, 1920


def timed(fn, steps, warmup):
    """ms per call: one event window over `steps` calls, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pixel_batches.json"))
    args = ap.parse_args()
    from iris_amd import _lib as L
    from iris_amd.utils.dataset import PixelSet
    dev = torch.device("cuda:0")
    V, hw = args.views, H * W
    n = V * hw
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    views = []
    for v in range(V):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        views.append(dict(kind="real", K=np.array([[1400.0 + v, 0, 960.0], [0, 1400.0 - v, 540.0], [0, 0, 1]], np.float32),
                          c2w=np.hstack([q, rng.normal(size=(3, 1))]).astype(np.float32)))
    rgb = torch.randint(0, 256, (n, 3), device=dev, dtype=torch.uint8, generator=g)
    albedo = torch.randint(0, 256, (n, 3), device=dev, dtype=torch.uint8, generator=g)
    seg = torch.randint(0, 200, (n,), device=dev, dtype=torch.int32, generator=g)
    exposure = (0.5 + rng.random(V)).astype(np.float32)
    ps = PixelSet(views, (H, W), rgb, segmentation=seg, int_albedo=albedo, exposure=exposure, batch_size=8192, device=dev)

    # the reference's layout, built from the set's own values view by view
    table = torch.empty(n, 16, device=dev, dtype=torch.float32)
    for v in range(V):
        s = slice(v * hw, (v + 1) * hw)
        table[s, :12] = torch.cat(ps.view_rays(v), 1)
        table[s, 12] = seg[s].float()
        table[s, 13:] = (rgb[s].double() / 255.0).float()
    albedo_f = torch.cat([(albedo[v * hw:(v + 1) * hw].double() / 255.0).float() for v in range(V)])
    exposure_f = torch.from_numpy(exposure).to(dev).view(-1, 1, 1).repeat(1, hw, 1).view(-1, 1)

    def reference(idx):
        tmp = table.index_select(0, idx)
        return dict(rays=tmp[..., :12], segmentation=tmp[..., 12], rgbs=tmp[..., 13:16], int_albedo=albedo_f.index_select(0, idx),
                    exposure=exposure_f.index_select(0, idx))

    out = {"what": "pixel batch: PixelSet.gather (one iris_pixel_batch launch, 8-bit stores + camera table) vs index_select on the reference's float tables "
                   "(N,16), (N,3), (N,1) on the same GPU", "box": torch.cuda.get_device_name(0), "build": L.build_id(), "views": V, "img_hw": [H, W],
           "resident_bytes_per_pixel": {"pixel_set": round((ps.rgb.nbytes + ps.int_albedo.nbytes + ps.segmentation.nbytes + ps.exposure.nbytes +
                                                            ps.cameras.nbytes) / n, 4),
                                        "reference_layout": (table.nbytes + albedo_f.nbytes + exposure_f.nbytes) / n},
           "note": "ms per batch under HIP events, host launches included; each arm twice, the fused one around the torch one"}
    perm = torch.randperm(n, device=dev, generator=g)
    for B, steps, warmup in ((8192, 2000, 200), (1 << 21, 50, 10)):
        idx = perm[:B].contiguous()
        a, b = ps.gather(idx), reference(idx)
        same = all(torch.equal(a[k] if k != "segmentation" else a[k].float(), b[k]) for k in b)
        f1 = timed(lambda: ps.gather(idx), steps, warmup)
        t1, t2 = timed(lambda: reference(idx), steps, warmup), timed(lambda: reference(idx), steps, warmup)
        f2 = timed(lambda: ps.gather(idx), steps, warmup)
        out["B=%d" % B] = {"pixel_set_ms_per_batch": [round(f1, 4), round(f2, 4)], "index_select_ms_per_batch": [round(t1, 4), round(t2, 4)],
                           "index_select_over_pixel_set": round(min(t1, t2) / max(f1, f2), 2), "steps": steps, "warmup": warmup, "same_values": bool(same)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
