"""The texture export stage (reference: utils/export.py, run by scripts/export.sh) on MI355X: the trained material network baked into a UV atlas.

    python -m iris_amd.utils.export --mesh scene.obj --ckpt last_1.ckpt --emitter_path checkpoints/EXP/bake --dir_save outputs/EXP/texture --tex_res 2048

The reference's arguments, and its products: <dir_save>/albedo.png (RGB albedo) and rm.png (roughness in R, metallic in G, 0 in B), 8-bit, row 0 at v ~ 0,
with ft.npy / vt.npy, the atlas they were baked in.  The voxel bounds come from <emitter_path>/vslf.npz, the network from the checkpoint's 'material.' entries
(load_ngpbrdf), the mesh from load_mesh.  The UV triangles are rasterised and the positions interpolated by iris_amd.utils.texture (HIP, an exact contract of
its own: DESIGN.md section 5c-7), the network runs on every texel, the outputs are quantised on the device; the PNGs are written with zlib alone.

Additions: --material pkg.module:factory (as the other command lines); --atlas auto|files|grid; --write_obj (mesh.obj + mesh.mtl next to the images).
    --atlas files  reads <dir_save>/ft.npy and vt.npy, exactly the reference's cache: an atlas unwrapped with xatlas elsewhere drops in that way.
    --atlas grid   builds texture.grid_atlas (two faces per grid cell, shape and area ignored: valid, not good) and saves the two files.
    --atlas auto   (default) uses the files when both exist and FAILS otherwise: a poor atlas is never produced silently.

Not built: calling xatlas itself (not a dependency, no ROCm relevance: run it anywhere and drop the .npy files in); seam dilation (the reference has none);
reading vt from an OBJ.
"""
import os
import sys

import numpy as np
import torch

from .. import _lib as L
from . import stage, texture as T


def build_parser():
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
    parser.add_argument("--atlas", type=str, default="auto", choices=["auto", "files", "grid"],
                        help="files: <dir_save>/ft.npy + vt.npy; grid: the grid stand-in, saved there; auto: the files when both exist, else an error")
    parser.add_argument("--write_obj", action="store_true", help="also write mesh.obj and mesh.mtl (map_Kd albedo.png)")
    return parser


def load_atlas(mode, dir_save, n_faces, tex_res):
    """-> (vt (N, 2) float32, ft (F, 3) int32), host numpy, by the rule of --atlas"""
    path_ft, path_vt = os.path.join(dir_save, "ft.npy"), os.path.join(dir_save, "vt.npy")
    have = os.path.exists(path_ft) and os.path.exists(path_vt)
    if mode == "grid":
        vt, ft = T.grid_atlas(n_faces, tex_res)
        np.save(path_ft, ft)
        np.save(path_vt, vt)
        print(f"[INFO] grid atlas (two faces per cell; triangle shape and area ignored) saved to {path_ft} and {path_vt}")
        return vt, ft
    if not have:
        raise L.IrisError(f"no UV atlas: {path_ft} and {path_vt} do not both exist.  Unwrap the mesh with xatlas (not a dependency of this package) and save its "
                          f"ft.npy (F, 3) and vt.npy (N, 2) there, or pass --atlas grid for the built-in stand-in, which is valid but ignores triangle shape and area")
    print(f"[INFO] found existing UVs, loading from {path_ft} and {path_vt}")
    return np.load(path_vt).astype(np.float32), np.load(path_ft).astype(np.int32)


def main(argv=None):
    from .path_tracing import load_mesh
    args = build_parser().parse_args(argv)
    for name in ("mesh", "emitter_path", "dir_save"):
        if not getattr(args, name):
            raise L.IrisError(f"export: --{name} is required")
    os.makedirs(args.dir_save, exist_ok=True)
    v_np, f_np = load_mesh(args.mesh)
    vt_np, ft_np = load_atlas(args.atlas, args.dir_save, f_np.shape[0], args.tex_res)
    T.check_inputs(vt_np, ft_np, v_np, f_np, args.tex_res)                 # before the device is touched
    device = stage.open_device(args.device, "export")
    material_net = stage.load_material(args.material, os.path.join(args.emitter_path, "vslf.npz"), args.ckpt)
    if isinstance(material_net, torch.nn.Module):
        material_net.to(device)
    print(f"[INFO] mesh v={v_np.shape} f={f_np.shape} vt={vt_np.shape} ft={ft_np.shape}, texture {args.tex_res} x {args.tex_res}")
    albedo, rm = T.bake_textures(material_net, vt_np, ft_np, v_np, f_np, args.tex_res, args.chunk_size, device=device)
    path_albedo, path_rm = os.path.join(args.dir_save, "albedo.png"), os.path.join(args.dir_save, "rm.png")
    T.write_png(path_albedo, albedo)
    T.write_png(path_rm, rm)
    if args.write_obj:
        T.write_textured_obj(args.dir_save, v_np, f_np, vt_np, ft_np)
    print(f"[INFO] saved albedo to {path_albedo}, saved roughness and metallic to {path_rm}")


if __name__ == "__main__":
    try:
        main()
    except L.IrisError as e:
        sys.exit("export: " + str(e))
