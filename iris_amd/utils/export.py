"""The texture export stage (reference: utils/export.py, run by scripts/export.sh) on MI355X: the trained material network baked into a UV atlas.

    python -m iris_amd.utils.export --mesh scene.obj --ckpt last_1.ckpt --emitter_path checkpoints/EXP/bake --dir_save outputs/EXP/texture --tex_res 2048

The reference's arguments, and its products: <dir_save>/albedo.png (RGB albedo) and rm.png (roughness in R, metallic in G, 0 in B), 8-bit, row 0 at v ~ 0,
with ft.npy / vt.npy, the atlas they were baked in.  The voxel bounds come from <emitter_path>/vslf.npz, the network from the checkpoint's 'material.' entries
(load_ngpbrdf), the mesh from load_mesh.  The UV triangles are rasterised and the positions interpolated by iris_amd.utils.texture (HIP, an exact contract of
its own: DESIGN.md section 5c-7), the network runs on every texel, the outputs are quantised on the device; the PNGs are written with zlib alone.

Additions: --material pkg.module:factory (as the other command lines); --atlas auto|files|grid|area; --dilate N; --write_obj (mesh.obj + mesh.mtl next to the
images); --verify N; --fit_steps N with --fit_points, --fit_lr, --fit_seed.
    --atlas files  reads <dir_save>/ft.npy and vt.npy, exactly the reference's cache: an atlas unwrapped with xatlas elsewhere drops in that way.
    --atlas grid   builds texture.grid_atlas (two faces per grid cell, shape and area ignored: valid, not good) and saves the two files.
    --atlas area   builds texture.area_atlas on the device from the loaded mesh (one chart per face in a power-of-two cell sized by the face's area, placed in
                   Morton order; exact), saves the two files and prints its report.  --tex_res must be a power of two in [4, 8192].
    --atlas auto   (default) uses the files when both exist and FAILS otherwise: a poor atlas is never produced silently.
    --dilate N     (default 0, at most 4) seam dilation after the bake: every uncovered texel within N texels of a covered one takes the nearest covered
                   texel's bytes, so that a bilinear lookup at a chart's border (model.texture.BakedTextureBRDF, --textures of the render stages) does not
                   read black.  The reference has none.
    --verify N     (default 0: off) after the files are written, the network and the textures read back (BakedTextureBRDF on the arrays still on the device)
                   are evaluated at N surface points -- face i F // N, barycentrics from a CPU generator seeded with 0 -- and one line prints the PSNR of albedo,
                   roughness and metallic: whether --tex_res and --dilate were enough.
    --fit_steps N  (default 0: off, every file as before) after the bake and the dilation, the images become a model.texture.TextureBRDF (float texels, the same
                   bilinear fetch, differentiable) that texture.fit_textures fits to the network: N Adam steps of --fit_lr (default 5e-3, about one 8-bit code
                   per step) on --fit_points (default 262144) area-proportional surface points per step, drawn from --fit_seed (default 0).  albedo.png and
                   rm.png are then its to_images(), ROUNDED to 8 bits; the first and the last loss are printed, and --verify prints its line twice, before and
                   after the fit, at the same points.  

Not built: calling xatlas itself (not a dependency, no ROCm relevance: run it anywhere and drop the .npy files in); charts of several faces and charts that keep
a face's shape (every chart of the two built-in atlases is a right isosceles triangle); a non-square texture for --atlas area; reading vt from an OBJ; fitting
the textures to the photographs (through train_brdf_crf) instead of to the network; mip levels and sRGB for the fitted textures.
"""
import os
import sys

import numpy as np
import torch

from .. import _lib as L
from . import stage, texture as T


def build_parser(area_atlas=False, verify=False, fit=False):
    """The stage's parser.  build_parser() is the stage as it was first built -- the reference's arguments, --material, --atlas auto|files|grid, --write_obj:
    the option table that tests/test_stage_setup_cpu.py pins, option for option.  build_parser(area_atlas=True) is that plus what the built-in area atlas
    brought, the choice --atlas area and the option --dilate (tests/test_atlas_cpu.py pins that table whole).  build_parser(area_atlas=True, verify=True) is
    that plus --verify N, and build_parser(area_atlas=True, verify=True, fit=True) the command line that main() runs: the four options of the fit."""
    import argparse
    parser = argparse.ArgumentParser(description="python -m iris_amd.utils.export: the reference's utils/export.py on MI355X")
    parser.add_argument("--mesh")
    parser.add_argument("--ckpt")
    parser.add_argument("--emitter_path")
    parser.add_argument("--dir_save")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--tex_res", type=int, default=2048)
    parser.add_argument("--chunk_size", type=int, default=160000)
    # additions
    stage.add_common_options(parser, "material")
    parser.add_argument("--atlas", type=str, default="auto", choices=["auto", "files", "grid"] + (["area"] if area_atlas else []),
                        help="files: <dir_save>/ft.npy + vt.npy; grid: the grid stand-in, saved there; auto: the files when both exist, else an error" +
                             ("; area: the area-proportional atlas, built on the device and saved there" if area_atlas else ""))
    if area_atlas:
        parser.add_argument("--dilate", type=int, default=0, help="seam dilation: fill uncovered texels within N texels (0 to 4) of a covered one from the nearest")
    parser.add_argument("--write_obj", action="store_true", help="also write mesh.obj and mesh.mtl (map_Kd albedo.png)")
    if verify:
        parser.add_argument("--verify", type=int, default=0, metavar="N", help="after the files are written: the PSNR of the textures, read back through "
                            "model.texture.BakedTextureBRDF, against the network at N surface points (0, the default: off)")
    if fit:
        parser.add_argument("--fit_steps", type=int, default=0, metavar="N", help="after the bake: N Adam steps that fit the textures, read back bilinearly, to the "
                            "network at surface points; the images are then rounded to 8 bits (0, the default: off)")
        parser.add_argument("--fit_points", type=int, default=262144, metavar="M", help="surface points per step of the fit")
        parser.add_argument("--fit_lr", type=float, default=5e-3, help="the fit's learning rate (about one 8-bit code per step)")
        parser.add_argument("--fit_seed", type=int, default=0, help="the seed of the fit's surface points")
    return parser


def verify_points(v, f, n):
    """The N surface points of --verify, on the host and reproducible -> (face (N,) int64, bary (N, 2) float32, position (N, 3) float32): point i lies on face
    i * F // N, at the barycentrics (b1, b2) = row i of torch.rand(N, 2) from a CPU generator seeded with 0, folded into the triangle (a row with b1 + b2 > 1
    becomes (1 - b1, 1 - b2)); position = ((1 - b1 - b2) p0 + b1 p1) + b2 p2 in float32."""
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f).reshape(-1, 3)
    n, F = int(n), f.shape[0]
    if n < 1 or F < 1:
        raise L.IrisError(f"verify_points: {n} points on {F} faces")
    face = (np.arange(n, dtype=np.int64) * F) // n
    u = torch.rand(n, 2, generator=torch.Generator().manual_seed(0)).numpy()
    u = np.where((u[:, :1] + u[:, 1:]) > 1.0, np.float32(1.0) - u, u).astype(np.float32)
    b1, b2 = u[:, :1], u[:, 1:]
    p0, p1, p2 = (v[f[face, k]] for k in range(3))
    pos = ((np.float32(1.0) - b1 - b2) * p0 + b1 * p1) + b2 * p2
    return face, u, pos.astype(np.float32)


def _psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0.0 else -10.0 * float(np.log10(mse))


@torch.no_grad()
def verify_textures(material_net, v, f, vt, ft, albedo, rm, n, device):
    """--verify N: the network and a BakedTextureBRDF built from the arrays that are still on the device, at verify_points(v, f, N) -> {'albedo', 'roughness',
    'metallic'}: PSNR in dB at a data range of 1 (inf when equal).  What the 8-bit quantisation, the texture resolution, the atlas and the seams cost: the
    number that says whether --tex_res and --dilate were enough."""
    from ..model.texture import BakedTextureBRDF
    from .path_tracing import Scene
    _, _, pos = verify_points(v, f, n)
    pos = torch.from_numpy(pos).to(device)
    baked = BakedTextureBRDF(Scene(v, f, device=device), ft, vt, albedo, rm)
    want, got = material_net(pos), baked(pos)
    return {k: _psnr(want[k].detach().reshape(got[k].shape), got[k]) for k in ("albedo", "roughness", "metallic")}


def build_area_atlas(dir_save, v, f, tex_res, device=None):
    """texture.area_atlas of the mesh on `device`, saved as <dir_save>/ft.npy and vt.npy, its report printed -> (vt, ft, vt_host, ft_host): the device tensors,
    which the bake takes as they are, and the host copies the files were written from"""
    path_ft, path_vt = os.path.join(dir_save, "ft.npy"), os.path.join(dir_save, "vt.npy")
    vt, ft, report = T.area_atlas(v, f, tex_res, device=device)
    vt_np, ft_np = vt.cpu().numpy(), ft.cpu().numpy()
    np.save(path_ft, ft_np)
    np.save(path_vt, vt_np)
    print(f"[INFO] area atlas (one chart per face, cells of 2^k texels by area) saved to {path_ft} and {path_vt}: j = {report['j']}, D_j = {report['D_j']:.6g}, "
          f"used = {report['used']:.4f}, faces per class = {report['histogram']}, clamped at KMIN / KMAX = {report['clamped_min']} / {report['clamped_max']}")
    return vt, ft, vt_np, ft_np


def load_atlas(mode, dir_save, n_faces, tex_res, v=None, f=None, device=None):
    """-> (vt (N, 2) float32, ft (F, 3) int32), host numpy, by the rule of --atlas.  mode 'area' builds the atlas of the mesh (v, f) on `device`
    (build_area_atlas, which also hands out the device tensors)."""
    path_ft, path_vt = os.path.join(dir_save, "ft.npy"), os.path.join(dir_save, "vt.npy")
    have = os.path.exists(path_ft) and os.path.exists(path_vt)
    if mode == "area":
        if v is None or f is None:
            raise L.IrisError("load_atlas: the area atlas is built from the mesh: pass v and f")
        return build_area_atlas(dir_save, v, f, tex_res, device)[2:]
    if mode == "grid":
        vt, ft = T.grid_atlas(n_faces, tex_res)
        np.save(path_ft, ft)
        np.save(path_vt, vt)
        print(f"[INFO] grid atlas (two faces per cell; triangle shape and area ignored) saved to {path_ft} and {path_vt}")
        return vt, ft
    if not have:
        raise L.IrisError(f"no UV atlas: {path_ft} and {path_vt} do not both exist.  Unwrap the mesh with xatlas (not a dependency of this package) and save its "
                          f"ft.npy (F, 3) and vt.npy (N, 2) there, or pass --atlas grid for the built-in stand-in, which is valid but ignores triangle shape and area, "
                          f"or --atlas area for the built-in atlas that gives every face a chart sized by its area")
    print(f"[INFO] found existing UVs, loading from {path_ft} and {path_vt}")
    return np.load(path_vt).astype(np.float32), np.load(path_ft).astype(np.int32)


def main(argv=None):
    from .path_tracing import load_mesh
    args = build_parser(area_atlas=True, verify=True, fit=True).parse_args(argv)
    if args.verify < 0:
        raise L.IrisError(f"export: --verify {args.verify}: a number of points, 0 for none")
    T.check_fit_options(args.fit_steps, args.fit_points, args.fit_lr)
    for name in ("mesh", "emitter_path", "dir_save"):
        if not getattr(args, name):
            raise L.IrisError(f"export: --{name} is required")
    T.check_dilate(args.dilate)
    os.makedirs(args.dir_save, exist_ok=True)
    v_np, f_np = load_mesh(args.mesh)
    if args.atlas == "area":                                               # the one atlas that is built on the device: its host checks come first
        T.check_atlas_inputs(v_np, f_np, args.tex_res)
        device = stage.open_device(args.device, "export")
        vt, ft, vt_np, ft_np = build_area_atlas(args.dir_save, v_np, f_np, args.tex_res, device)          # vt, ft stay on the device for the bake
        T.check_inputs(vt_np, ft_np, v_np, f_np, args.tex_res)
    else:
        vt, ft = vt_np, ft_np = load_atlas(args.atlas, args.dir_save, f_np.shape[0], args.tex_res)
        T.check_inputs(vt_np, ft_np, v_np, f_np, args.tex_res)             # before the device is touched
        device = stage.open_device(args.device, "export")
    material_net = stage.load_material(args.material, os.path.join(args.emitter_path, "vslf.npz"), args.ckpt)
    if isinstance(material_net, torch.nn.Module):
        material_net.to(device)
    print(f"[INFO] mesh v={v_np.shape} f={f_np.shape} vt={vt_np.shape} ft={ft_np.shape}, texture {args.tex_res} x {args.tex_res}")
    albedo, rm = T.bake_textures(material_net, vt, ft, v_np, f_np, args.tex_res, args.chunk_size, device=device, dilate=args.dilate)

    def verify():
        q = verify_textures(material_net, v_np, f_np, vt, ft, albedo, rm, args.verify, device)
        print(f"[INFO] verify: textures against the network at {args.verify} surface points: PSNR albedo {q['albedo']:.2f} dB, roughness {q['roughness']:.2f} dB, "
              f"metallic {q['metallic']:.2f} dB")
    if args.fit_steps:
        from ..model.texture import TextureBRDF
        from .path_tracing import Scene
        if args.verify:
            verify()                                                       # the baked images, before the fit
        fitted = TextureBRDF(Scene(v_np, f_np, device=device), ft, vt, albedo, rm)
        report = T.fit_textures(material_net, fitted, v_np, f_np, args.fit_steps, args.fit_points, args.fit_lr, seed=args.fit_seed)
        albedo, rm = fitted.to_images()
        print(f"[INFO] fit: {args.fit_steps} steps of {args.fit_points} surface points at lr {args.fit_lr:g}: loss {report['first_loss']:.6g} -> {report['last_loss']:.6g}")
    path_albedo, path_rm = os.path.join(args.dir_save, "albedo.png"), os.path.join(args.dir_save, "rm.png")
    T.write_png(path_albedo, albedo)
    T.write_png(path_rm, rm)
    if args.write_obj:
        T.write_textured_obj(args.dir_save, v_np, f_np, vt_np, ft_np)
    print(f"[INFO] saved albedo to {path_albedo}, saved roughness and metallic to {path_rm}")
    if args.verify:
        verify()


if __name__ == "__main__":
    try:
        main()
    except L.IrisError as e:
        sys.exit("export: " + str(e))
