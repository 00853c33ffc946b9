#!/usr/bin/env python3
"""tests/golden/render_intrinsics.npz: the intrinsics half of the reference's render loop (render.py:178-220) run through THE REFERENCE'S OWN functions.

Runs only in the build container (imports the reference through the stub modules of tools/make_goldens.py; torch-CPU).  The loop body is replayed call by call --
torch.rand (recorded), NF.normalize, ray_intersect (the oracle's brute-force closest hit patched in: utils/path_tracing.py:30-43 is Mitsuba / OptiX),
material_net(positions), material_net.sample_specular, emitter_net.eval_emitter, emitter_net(positions), the masked defaults and the reshape().mean(1) sums --
for two rounds of spp = 5, once in float32 and once, on the SAME recorded per-sample inputs, in float64 (torch.set_default_dtype(torch.float64), modules .double()).

Scene: the box room of make_goldens.py with the wall x = 4 removed (primary rays leave through it), its ceiling light in view, and two more emitter triangles
hanging in the room whose radiance rows sum to zero -- (0,0,0) and (1,-1,0) -- which the reference therefore treats as surfaces (render.py:202); the smooth H = 32
SLF with the voxels y < 0.6 emptied (a visible part of the wall y = 0 has no radiance cache); a 24 x 16 camera.  Material: tests/stub_material.EdgeStubMaterial
(roughness reaches 0.02 and 1.0, metallic 0 and 1).

Stored: the scene, SLF and emitter tables, the rays, per round every per-sample input of iris_render_intrinsics (positions, normals, wo, e0, valid_next, material
rows, u2) and the jitter draws, the six accumulated float32 maps and the same maps from the float64 run.  Asserted while writing: misses, kept surfaces, real
emitters, zero-sum emitters and empty voxels each make up at least 1 % of the samples, and the float32 and float64 runs classify every sample identically (keep
mask, voxel row); if they do not, change --seed so that no discontinuity sits on a rounding.

    python tools/make_render_golden.py [--seed 11]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
SPP, ROUNDS, H_IMG, W_IMG, H_SLF = 5, 2, 16, 24, 32
MAPS = ("kd", "a_prime", "roughness", "metallic", "emission", "slf")


def render_room():
    """make_goldens.box_room() without the wall x = X, plus two triangles hanging in the room at x = 3 (facing the camera)"""
    from make_goldens import box_room
    v, f = box_room()
    f = np.asarray([t for t in f.tolist() if t not in ([1, 5, 6], [1, 6, 2])], np.int32)          # 10 wall triangles + the 2 of the ceiling light
    n = len(v)
    extra_v = np.asarray([(3.0, 0.3, 0.7), (3.0, 1.3, 0.7), (3.0, 0.8, 1.7), (3.0, 1.7, 0.7), (3.0, 2.7, 0.7), (3.0, 2.2, 1.7)], np.float32)
    extra_f = np.asarray([(n, n + 1, n + 2), (n + 3, n + 4, n + 5)], np.int32)
    return np.concatenate([v, extra_v]), np.concatenate([f, extra_f])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=11)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as NF
    from make_goldens import _stub_modules, smooth_radiance, surface_mask
    _stub_modules()
    sys.path.insert(0, REF)
    os.chdir(REF)
    from model.brdf import BaseBRDF
    from model.slf import VoxelSLF
    from model.emitter import SLFEmitter
    import utils.path_tracing as rpt
    from utils.dataset import real_ldr
    from stub_material import EdgeStubMaterial
    import oracle
    oracle.build()

    verts, faces = render_room()
    osc = oracle.Scene(verts, faces)

    def ray_intersect_patch(scene, xs, ds):
        p, n, uv, idx, valid = osc.ray_intersect(xs.detach().numpy().astype(np.float32), ds.detach().numpy().astype(np.float32), brute=True)
        return (torch.from_numpy(p), torch.from_numpy(n), torch.from_numpy(uv), torch.from_numpy(idx), torch.from_numpy(valid))
    rpt.ray_intersect = ray_intersect_patch

    # SLF: surface voxels with the smooth radiance of the other fixtures; y < 0.6 emptied
    vmin, vmax = -0.23, 4.21              # (no face of the room lies on a voxel boundary: the ceiling light at z = 2.55 would with -0.2 .. 4.2)
    mask = surface_mask(verts, faces, H_SLF, vmin, vmax)
    yc = (np.arange(H_SLF) + 0.5) / H_SLF * (vmax - vmin) + vmin
    mask[:, yc < 0.6, :] = False
    slf = VoxelSLF(torch.from_numpy(mask), vmin, vmax)
    kk, jj, ii = np.where(mask)
    slf.radiance[:] = torch.from_numpy(smooth_radiance((np.stack([ii, jj, kk], -1) + 0.5) / H_SLF * (vmax - vmin) + vmin))
    # emitters: the ceiling light (10, 9, 8) and the two zero-sum triangles
    n_face = len(faces)
    is_emitter = torch.zeros(n_face, dtype=torch.bool); is_emitter[-4:] = True
    ev = torch.from_numpy(verts[faces[-4:]])
    area = torch.cross(ev[:, 1] - ev[:, 0], ev[:, 2] - ev[:, 0], dim=-1).norm(dim=-1) / 2.0
    rad = torch.zeros(n_face, 3)
    rad[0] = rad[1] = torch.tensor([10.0, 9.0, 8.0]); rad[2] = torch.tensor([0.0, 0.0, 0.0]); rad[3] = torch.tensor([1.0, -1.0, 0.0])
    tmp = tempfile.mkdtemp()
    ep, sp = os.path.join(tmp, "emitter.pth"), os.path.join(tmp, "vslf.npz")
    torch.save({"is_emitter": is_emitter, "emitter_vertices": ev, "emitter_area": area, "emitter_normal": torch.zeros(4, 3), "emitter_radiance": rad}, ep)
    torch.save({"mask": torch.from_numpy(mask), "voxel_min": vmin, "voxel_max": vmax, "weight": slf.state_dict()}, sp)
    emitter_net = SLFEmitter(ep, sp)

    class RefStub(BaseBRDF):                # the reference's NGPBRDF is a BaseBRDF with a forward(position) (model/brdf.py:213-260)
        def forward(self, x):
            return EdgeStubMaterial()(x)
    material_net = RefStub()

    # camera near the wall x = 0, looking along +x and up: the ceiling light, the open side, the wall y = 0 and the two triangles
    K = torch.tensor([[0.45 * W_IMG, 0, W_IMG / 2], [0, 0.45 * W_IMG, H_IMG / 2], [0, 0, 1]], dtype=torch.float32)
    fwd = np.array([1.0, 0.0, 0.3]); fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w = torch.tensor(np.concatenate([np.stack([right, down, fwd], 1), np.array([[0.3], [1.5], [1.3]])], 1), dtype=torch.float32)
    rays_x, rays_d, dxdu, dydv = real_ldr.to_world(real_ldr.get_direction(K, (H_IMG, W_IMG)), c2w, True, K)
    B = rays_x.shape[0]

    def after_hit(positions, normals, ds, tri, valid, mat, u2, acc):
        """render.py:189-220 through the reference's functions, in the default dtype; returns (keep mask, voxel rows)"""
        albedo_, metallic_, roughness_ = mat["albedo"], mat["metallic"].clone(), mat["roughness"].clone()
        kd_ = albedo_ * (1 - metallic_)
        ks_ = 0.04 * (1 - metallic_) + albedo_ * metallic_
        _, _, g0, g1 = material_net.sample_specular(u2, -ds, normals, roughness_)
        a_prime_ = g0 * ks_ + g1 + kd_
        emission_ = emitter_net.eval_emitter(positions, ds, tri)[0]
        keep = torch.logical_and(valid, emission_.sum(-1) == 0)
        slf_ = emitter_net(positions)
        kd_[~keep] = 1.0; a_prime_[~keep] = 1.0; roughness_[~keep] = 1.0; metallic_[~keep] = 0.0
        for name, x, c in (("kd", kd_, 3), ("a_prime", a_prime_, 3), ("roughness", roughness_, 1), ("metallic", metallic_, 1), ("emission", emission_, 3), ("slf", slf_, 3)):
            acc[name] += x.reshape(-1, SPP, c).mean(1)
        return keep, emitter_net.slf.spatial_idx(positions)

    out = {"verts": verts, "faces": faces, "K": K.numpy(), "c2w": c2w.numpy(), "H": H_IMG, "W": W_IMG, "spp": SPP, "rounds": ROUNDS, "seed": args.seed,
           "slf_mask": mask, "slf_inds": slf.inds.numpy().astype(np.int32), "slf_radiance": slf.radiance.numpy(), "voxel_min": vmin, "voxel_max": vmax,
           "is_emitter": is_emitter.numpy(), "emitter_area": area.numpy(), "emitter_radiance": rad.numpy(), "emitter_vertices": ev.numpy(),
           "rays_o": rays_x.numpy(), "rays_d": rays_d.numpy(), "dx_du": dxdu.numpy(), "dy_dv": dydv.numpy()}
    torch.manual_seed(args.seed)
    acc32 = {k: torch.zeros(B, 1 if k in ("roughness", "metallic") else 3) for k in MAPS}
    rounds = []
    for r in range(ROUNDS):
        # render.py:179-184
        dudv = torch.rand(2, B, SPP, 1)
        du, dv = dudv
        ds = rays_d[:, None] + dxdu[:, None] * du + dydv[:, None] * dv
        ds = NF.normalize(ds, dim=-1).reshape(-1, 3)
        xs = rays_x.repeat_interleave(SPP, dim=0)
        positions, normals, _, tri, valid = rpt.ray_intersect(None, xs, ds)
        mat = material_net(positions)
        u2 = torch.rand(len(positions), 2)
        keep, vox = after_hit(positions, normals, ds, tri, valid, mat, u2, acc32)
        is_em = is_emitter[tri] & valid
        e0 = torch.where(is_em, emitter_net.emitter_idx[tri], torch.full_like(tri, -1)).to(torch.int32)
        rounds.append(dict(positions=positions, normals=normals, ds=ds, tri=tri, valid=valid, mat=mat, u2=u2, keep=keep, vox=vox))
        out.update({f"dudv_{r}": dudv.numpy(), f"u2_{r}": u2.numpy(), f"wi_{r}": ds.numpy(), f"pos_{r}": positions.numpy(), f"nrm_{r}": normals.numpy(),
                    f"wo_{r}": (-ds).numpy(), f"e0_{r}": e0.numpy(), f"valid_next_{r}": (valid & ~is_em).numpy(), f"albedo_{r}": mat["albedo"].numpy(),
                    f"roughness_{r}": mat["roughness"].numpy(), f"metallic_{r}": mat["metallic"].numpy(), f"keep_{r}": keep.numpy(), f"voxel_{r}": vox.numpy().astype(np.int32)})

    # the same lines in float64 on the same per-sample inputs
    torch.set_default_dtype(torch.float64)
    emitter_net.double(); material_net.double()
    acc64 = {k: torch.zeros(B, 1 if k in ("roughness", "metallic") else 3) for k in MAPS}
    try:
        for r, R in enumerate(rounds):
            mat64 = {k: v.double() for k, v in R["mat"].items()}
            keep64, vox64 = after_hit(R["positions"].double(), R["normals"].double(), R["ds"].double(), R["tri"], R["valid"], mat64, R["u2"].double(), acc64)
            assert torch.equal(keep64, R["keep"]) and torch.equal(vox64, R["vox"]), f"round {r}: the float32 and float64 runs classify a sample differently: change --seed"
    finally:
        torch.set_default_dtype(torch.float32)
    for k in MAPS:
        assert acc64[k].dtype == torch.float64
        out[f"map32_{k}"] = acc32[k].numpy()
        out[f"map64_{k}"] = acc64[k].numpy()
        print(f"{k}: max |x| {float(acc64[k].abs().max()):.4g}, d32 {float((acc32[k].double() - acc64[k]).abs().max()):.3g}")

    # shares of the five sample classes
    tri = torch.cat([R["tri"] for R in rounds]); valid = torch.cat([R["valid"] for R in rounds]); keep = torch.cat([R["keep"] for R in rounds]); vox = torch.cat([R["vox"] for R in rounds])
    ordn = torch.where(valid & is_emitter[tri], emitter_net.emitter_idx[tri], torch.full_like(tri, -1))
    shares = {"miss": float((~valid).float().mean()), "kept_surface": float((keep & (ordn < 0)).float().mean()), "real_emitter": float(((ordn >= 0) & ~keep).float().mean()),
              "zero_sum_emitter": float(((ordn >= 2) & keep).float().mean()), "empty_voxel_on_a_hit": float((valid & (vox < 0)).float().mean())}
    print(shares)
    for k, s in shares.items():
        assert s >= 0.01, (k, s)
    assert float(((ordn == 2) & keep).float().mean()) > 0 and float(((ordn == 3) & keep).float().mean()) > 0
    rg, mt = torch.cat([R["mat"]["roughness"] for R in rounds]), torch.cat([R["mat"]["metallic"] for R in rounds])
    assert float(rg.min()) == float(np.float32(0.02)) and float(rg.max()) == 1.0 and float(mt.min()) == 0.0 and float(mt.max()) == 1.0
    path = os.path.join(OUT, "render_intrinsics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
