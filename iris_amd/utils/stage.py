"""What the fifteen command-line stages (fuse_segmentation, slf_bake, extract_emitter_ldr, initialize, slf_refine, bake_shading, refine_shading, render, render_video,
render_relight, train_brdf_crf, train_emitter, utils.export, utils.metric_brdf, utils.metric_crf) do before their first kernel launches: find the mesh, list the views and their photographs -- or the frames of the
render trajectory (load_trajectory: render_video, render_relight --mode traj) --, read checkpoints and the material network, build their parsers' shared
options, open the device; for the two stages whose frames become a video, the ffconcat list that stands where the reference's mp4 stands (write_ffconcat);
for the three training stages (initialize, train_brdf_crf, train_emitter; their loop is utils/trainer.py) what their main() refuses before the device
(refuse_unbuilt_training) and the pixel set it trains on (open_training_set); and for the nine stages that end in a `cli` (fuse_segmentation, the three
pre-bake commands, the three trainers and the two metric commands) the exit wrapper (exit_status).
Plain functions; a stage's main() stays a linear script that calls them.  Everything down to exit_status is host code and imports without a GPU; the
last seven functions need one.
"""
import importlib
import os

import numpy as np
import torch

from .. import _lib as L
from . import cameras


# ---- pure host
def mesh_path(dataset, root, scene=None):
    """The mesh file of a scene.  root: for scannetpp the dataset root, for every other dataset the scene's own folder; scene: the scannetpp scene id.
        scannetpp -> <root>/data/<scene>/scans/scene.ply
        else      -> <root>/scene.obj, or <root>/scene.ply when there is no scene.obj
    and IrisError when that file does not exist.  A superset of the rules the stages used to carry: bake and refine did not look for scene.ply under `synthetic`
    and `real`, the training files named scene.obj unseen; the only inputs that behave differently are ones that failed before."""
    if dataset == "scannetpp":
        path = os.path.join(root, "data", scene, "scans", "scene.ply")
    else:
        path = os.path.join(root, "scene.obj")
        if not os.path.exists(path):
            path = os.path.join(root, "scene.ply")
    if not os.path.exists(path):
        raise L.IrisError("mesh not found: " + path)
    return path


def load_views(dataset, root, scene, res_scale, split="train", cameras_json=None, img_hw=None, extras=False):
    """-> (img_hw, views) of a split.  root, scene: as mesh_path takes them.  cameras_json: a generic camera file that replaces the dataset's own (extras: its
    views also carry 'image' and 'exposure', utils.cameras.load_generic); img_hw: the size of a synthetic / real scene that has no Image/000_0001.exr."""
    if cameras_json:
        return cameras.load_generic(cameras_json, res_scale, extras=extras)
    if dataset == "synthetic":
        return cameras.load_synthetic(root, res_scale, img_hw, split=split)
    if dataset == "real":
        return cameras.load_real(root, res_scale, img_hw, split=split)
    if dataset == "scannetpp":                             # Scannetpp(dataset_root, scene, split=split, pixel=False, res_scale=res_scale)
        return cameras.load_scannetpp(root, scene, res_scale, split=split)
    raise L.IrisError("--dataset {!r}: synthetic | real | scannetpp, or --cameras cameras.json".format(dataset))


def load_trajectory(dataset, root, scene, res_scale, img_hw=None, split="val"):
    """-> (img_hw, views) of the scene's render trajectory (utils.cameras.load_trajectory: render_traj.npy through the split's camera).  Host only: the
    IrisError for a missing file comes before a stage opens its device."""
    return cameras.load_trajectory(dataset, root, scene, res_scale, img_hw, split=split)


def ffconcat_text(frames, fps=30):
    """The list `ffmpeg -f concat` reads, standing where the reference's imageio.mimsave(..., fps=30) stands: the frames forward and then reversed
    (imgs += imgs[::-1]: 2 N entries), each shown for 1 / fps seconds.  frames: the files' paths as the list names them (relative to the list's folder)."""
    lines = ["ffconcat version 1.0"]
    for f in list(frames) + list(frames)[::-1]:
        lines += ["file '{}'".format(str(f).replace("'", "'\\''")), "duration {:.9f}".format(1.0 / fps)]
    return "\n".join(lines) + "\n"


def write_ffconcat(path, frames, fps=30):
    """ffconcat_text(frames given as paths, written relative to the list's folder) -> path.  `ffmpeg -f concat -i <path> -vsync vfr -pix_fmt yuv420p out.mp4`
    makes the reference's video on a machine that has ffmpeg; the frames' even sizes are what its encoders need."""
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    with open(path, "w") as fh:
        fh.write(ffconcat_text([os.path.relpath(os.path.abspath(f), folder) for f in frames], fps))


def read_image(path, img_hw):
    """a view's photograph, (H, W, 3) float32: an EXR as stored, anything else through PIL as RGB / 255"""
    if path.lower().endswith(".exr"):
        from .exr import read_exr
        a = read_exr(path)
    else:
        from PIL import Image
        a = np.asarray(Image.open(path).convert("RGB"), np.float32) / 255.0
    if a.shape[:2] != tuple(img_hw):
        raise L.IrisError(f"{path}: {a.shape[:2]} pixels, the view has {tuple(img_hw)}")
    return a


def layout_resizes(dataset, cameras_json=None):
    """whether the stages resize this layout's 8-bit images to the views' size: only the scannetpp layout does (the reference's real and synthetic scripts
    never pass a scale, and InvRealDatasetLDR and InvSyntheticDatasetLDR take none); a --cameras file replaces the layout"""
    return dataset == "scannetpp" and not cameras_json


def check_photograph_size(path, img_hw, resize=False):
    """IrisError when the photograph's size (read from its header: nothing is decoded) is not the view's -- unless it is an 8-bit file of a layout that resizes
    (resize: layout_resizes; the device resizes it, utils/resize.py).  Resizing is built for the scannetpp layout's 8-bit files only, so --res_scale != 1
    against the full-size files of another layout, or against an .exr, ends here; FileNotFoundError when there is no such file"""
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    is_exr = path.lower().endswith(".exr")
    if is_exr:
        from .exr import read_exr_header
        h = read_exr_header(path)
        size = (int(h["height"]), int(h["width"]))
    else:
        from PIL import Image
        with Image.open(path) as im:
            size = (int(im.size[1]), int(im.size[0]))
    if size != tuple(img_hw) and (is_exr or not resize):
        raise L.IrisError(f"{path}: the photograph is {size[0]} x {size[1]}, the view {img_hw[0]} x {img_hw[1]}: resizing photographs is built for the 8-bit "
                          "files of the scannetpp layout only (elsewhere --res_scale 1 only)")


def read_photograph(path, img_hw, resize=False):
    """a view's photograph as the pre-bake stages pool it: a PNG or JPEG through PIL as (H, W, 3) uint8 -- it stays 8-bit on its way to the device, where the
    kernel decodes it as u / 255 --, an .exr through read_image as float32.  IrisError when its size is not the view's; with resize (layout_resizes) an 8-bit
    file comes back at the size it has."""
    check_photograph_size(path, img_hw, resize)
    if path.lower().endswith(".exr"):
        return np.ascontiguousarray(read_image(path, img_hw)[..., :3], dtype=np.float32)
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


def load_photographs(dataset, root, scene, res_scale, ldr_img_dir=None, cameras_json=None, max_views=None):
    """-> (img_hw, views, photographs) of the TRAIN split, for the stages that read the photographs (slf_bake, slf_refine, extract_emitter_ldr).
    photographs[i] = (path, exposure) of views[i]; root, scene: as mesh_path takes them.
        real       <root>/<ldr_img_dir or 'Image'>/%03d_0001.png by CAPTURE id (cameras.real_split_ids), <img_dir>/cam/exposure.npy[ids]
        synthetic  the same under <root>/train, by frame index
        scannetpp  <root>/data/<scene>/psdf/images/<view['name']>, exposure 1.0
        cameras_json   each view's 'image' and 'exposure'
    Without ldr_img_dir the real and synthetic layouts have no exposures (None), as in the reference.  The image size of a real / synthetic scene without
    Image/000_0001.exr is its first photograph's."""
    if cameras_json:
        img_hw, views = load_views(dataset, root, scene, res_scale, cameras_json=cameras_json, extras=True)
        photos = [(v["image"], v["exposure"]) for v in views]
        missing = [i for i, (path, _) in enumerate(photos) if not path]
        if missing:
            raise L.IrisError(f"{cameras_json}: view {missing[0]} names no 'image'")
    elif dataset in ("real", "synthetic"):
        data_root = os.path.join(root, "train") if dataset == "synthetic" else root
        img_dir = os.path.join(data_root, ldr_img_dir or "Image")
        if dataset == "real":
            with open(os.path.join(root, "cam.txt")) as fh:
                n_total = int(fh.readline())
            ids = cameras.real_split_ids(n_total, "train")
        else:
            ids = None
        img_hw = None
        if not os.path.isfile(os.path.join(data_root, "Image", "000_0001.exr")):
            from .dataset.files import _image_size
            h, w = _image_size(data_root, os.path.join(img_dir, "%03d_0001.png" % (ids[0] if ids else 0)))
            img_hw = (int(h * res_scale), int(w * res_scale))
        img_hw, views = load_views(dataset, root, scene, res_scale, img_hw=img_hw)
        ids = list(range(len(views))) if ids is None else ids
        if len(ids) != len(views):
            raise L.IrisError(f"{root}: {len(views)} cameras for {len(ids)} training views")
        exposures = [None] * len(ids)
        if ldr_img_dir:
            table = np.load(os.path.join(img_dir, "cam", "exposure.npy")).astype(np.float32).reshape(-1)
            if table.shape[0] <= max(ids):
                raise L.IrisError(f"{ldr_img_dir}/cam/exposure.npy holds {table.shape[0]} values, the training views reach id {max(ids)}")
            exposures = [float(table[i]) for i in ids]
        photos = [(os.path.join(img_dir, "%03d_0001.png" % i), e) for i, e in zip(ids, exposures)]
    else:
        img_hw, views = load_views(dataset, root, scene, res_scale)
        photos = [(os.path.join(root, "data", scene, "psdf", "images", v["name"]), 1.0) for v in views]
    if max_views is not None:
        views, photos = views[:max_views], photos[:max_views]
    return img_hw, views, photos


def load_pickled(path):
    """torch.load on the CPU.  Recent torch's tensors-only unpickler refuses the plain Python objects a Lightning checkpoint carries (hyper-parameters, callback
    states, optimizer groups); the reference loads its own files with the full unpickler, and so does the second attempt."""
    try:
        return torch.load(path, map_location="cpu")
    except Exception:     # noqa
        return torch.load(path, map_location="cpu", weights_only=False)


def write_checkpoint(path, material_state, crf_state, optimizer_state, *, epoch, global_step, hyper_parameters, emitter_state=None):
    """torch.save of {'state_dict': material.* and model_crf.* entries, 'optimizer_states': [optimizer_state], 'epoch', 'global_step',
    'hyper_parameters'}: the part of a Lightning checkpoint the reference's loaders read (refine_shading.py:84-89, slf_refine.py:74-79,
    train_brdf_crf.py:72-97 all take ['state_dict'] and filter on the two prefixes).  epoch: the number of completed epochs.  emitter_state: the tensors
    of the emitter and initialisation stages' SLFEmitterLearn, written under 'emitter.' -- 'emitter.radiance' is what extract_emitter_ldr --mode update
    reads (extract_emitter_ldr.py:117-122); None (the BRDF-CRF stage, which trains no emitter) writes no such key and the file is what it was before
    the keyword existed.  Written beside the target and renamed: a run that dies mid-write keeps the previous file."""
    state = {"material." + k: v.detach().cpu() for k, v in material_state.items()}
    state.update({"model_crf." + k: v.detach().cpu() for k, v in crf_state.items()})
    if emitter_state is not None:
        state.update({"emitter." + k: v.detach().cpu() for k, v in emitter_state.items()})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = str(path) + ".tmp"
    torch.save({"state_dict": state, "optimizer_states": [optimizer_state], "epoch": int(epoch), "global_step": int(global_step),
                "hyper_parameters": dict(hyper_parameters)}, tmp)
    os.replace(tmp, path)


def read_checkpoint(path):
    """-> the saved dict plus 'material', 'model_crf' and 'emitter': the entries of 'state_dict' under each prefix, the prefix stripped (the
    reference's idiom); 'emitter' is empty for a file without such keys (the BRDF-CRF stage's).  Everything on the CPU.  A Lightning checkpoint of the reference loads too (its other entries are ignored by the callers here)."""
    ck = load_pickled(path)
    out = dict(ck)
    for prefix in ("material", "model_crf", "emitter"):
        out[prefix] = {k.replace(prefix + ".", ""): v for k, v in ck["state_dict"].items() if prefix + "." in k}
    return out


def voxel_range(slf_path):
    """(voxel_min, voxel_max) of a vslf.npz, the pair NGPBRDF is constructed from (refine_shading.py:82-83)"""
    mask = load_pickled(slf_path)
    return float(mask["voxel_min"]), float(mask["voxel_max"])


def load_material(spec, slf_path, ckpt):
    """The material network: by default the reference's own -- NGPBRDF(mask['voxel_min'], mask['voxel_max']) with the checkpoint's 'material.' weights
    (refine_shading.py:82-92) --, or, with --material pkg.module:factory, any callable position -> {'albedo','roughness','metallic'}: the factory is called
    as factory(voxel_min, voxel_max, ckpt) when a checkpoint is given, as factory(voxel_min, voxel_max) otherwise, and as factory() if it takes neither."""
    if not spec:
        from ..model.brdf import load_ngpbrdf
        if not ckpt:
            raise L.IrisError("refine_shading: --ckpt (the checkpoint holding the NGPBRDF weights, refine_shading.py:36,84) or --material pkg.module:factory is required")
        return load_ngpbrdf(*voxel_range(slf_path), ckpt)
    mod, _, attr = spec.partition(":")
    factory = getattr(importlib.import_module(mod), attr or "material")
    vmin, vmax = voxel_range(slf_path)
    try:
        return factory(vmin, vmax, ckpt) if ckpt else factory(vmin, vmax)
    except TypeError:
        return factory()


def refuse_textures_with_material(args):
    """--textures and --material both name the material: IrisError, before the device is touched"""
    if getattr(args, "textures", None) and getattr(args, "material", None):
        raise L.IrisError("--textures and --material both name the material: pass one of them")


def load_texture_material(dir, mesh_path, device):
    """--textures DIR: BakedTextureBRDF.from_export(DIR, <the mesh at mesh_path>) on `device`.  The material builds its own Scene of that mesh (the stage's traced
    scene may hold more: render_relight's has the inserted lights in it).  What from_export refuses, it refuses before the device is touched."""
    from ..model.texture import BakedTextureBRDF
    from .path_tracing import load_mesh
    v, f = load_mesh(mesh_path)
    return BakedTextureBRDF.from_export(dir, v, f, device)


def view_seed_torch(seed, i):
    """seeds torch's CPU and GPU generators for view i of a run seeded with `seed`: the integrators draw with torch.rand.  (The bake's Philox key is
    bake_shading.view_seed, a different thing.)"""
    torch.manual_seed(seed * 1000003 + i)
    torch.cuda.manual_seed(seed * 1000003 + i)


# ---- parser helpers: the option groups more than one stage registers
IGNORED_TRAINER_OPTIONS = (("batch_size", int), ("voxel_path", str), ("num_workers", int), ("dir_val", str), ("val_step", int), ("has_part", int), ("load_crf", int))
COMMON_OPTIONS = {
    "material": dict(type=str, default=None, help="pkg.module:factory returning material_net(position) -> {'albedo','roughness','metallic'} "
                     "(default: the reference's NGPBRDF, loaded from the checkpoint's 'material.' entries)"),
    "cameras": dict(type=str, default=None, help="generic camera JSON instead of the dataset's own camera files"),
    "textures": dict(type=str, default=None, metavar="DIR", help="the folder utils.export wrote (albedo.png, rm.png, ft.npy, vt.npy, made for this stage's mesh): the material "
                     "is those textures, looked up at the closest triangle (model.texture.BakedTextureBRDF), instead of the network; the checkpoint is still read for "
                     "the response model; not together with --material"),
    "emor_path": dict(type=str, default=None, help="the EMoR basis file (default: crf/emor.txt under the working directory, as the reference)"),
    "denoise": dict(type=str, default="atrous", choices=["atrous", "none"]),
    "compression": dict(type=str, default="zip", choices=["none", "zips", "zip"]),
    "seed": dict(type=int, default=0),
    "max_views": dict(type=int, default=None),
    "exr_encoder": dict(type=str, default="host", choices=["host", "device"]),
    "video": dict(type=str, default="none", choices=["none", "mjpeg"], help="mjpeg: the trajectory's frames also as Motion-JPEG .avi files, the JPEG frames encoded "
                  "on the GPU (utils/jpeg.py, utils/avi.py); none (default): the frames and the .ffconcat lists only"),
    "video_quality": dict(type=int, default=90, choices=range(1, 101), metavar="Q", help="JPEG quality of --video mjpeg, 1..100 (the IJG scaling of the standard tables)"),
}


def add_ignored_trainer_options(parser):
    """the options of configs/config.py that the reference's render scripts register and never read"""
    for name, typ in IGNORED_TRAINER_OPTIONS:
        parser.add_argument("--" + name, type=typ, default=None, help="(a trainer option of configs/config.py: accepted, unused)")


def add_common_options(parser, *names, **help_texts):
    """the named options of COMMON_OPTIONS, in the order given; help_texts[name] replaces that option's help text"""
    for name in names:
        parser.add_argument("--" + name, **dict(COMMON_OPTIONS[name], **({"help": help_texts[name]} if name in help_texts else {})))


# ---- what a stage's main() opens and ends with
def refuse_unbuilt_training(args):
    """what every trainer's main() refuses first, before the device is touched: a scannetpp root without its lists, camera file, mesh or first view's files
    (check_scannetpp_files: two JSON files and three image headers, nothing is decoded), what is not built of the real and synthetic layouts (--res_scale
    != 1, no --ldr_img_dir: load_training_files' own messages), then --optimizer Ranger (make_optimizer's), then, with --validate other than none, the
    validation split's files, --val_frame and --val_step (utils.validation.check_validation_args) -> the validation files' dict, or None"""
    from .dataset.files import check_scannetpp_files, load_training_files
    from .trainer import make_optimizer
    from .validation import check_validation_args
    dataset, root = args.dataset
    if dataset == "scannetpp":
        check_scannetpp_files(root, args.scene, args.res_scale)
    elif float(args.res_scale) != 1.0 or not args.ldr_img_dir:
        load_training_files(dataset, root, args.ldr_img_dir, res_scale=args.res_scale)
    if args.optimizer == "Ranger":
        make_optimizer(args.optimizer, [], args.learning_rate, args.weight_decay, networks=())
    return check_validation_args(args)


def exit_status(name, main, argv=None):
    """main(argv) as a process exit status: what is refused, missing or not built is one line on stderr and status 2, not a traceback"""
    import sys
    try:
        return main(argv)
    except (L.IrisError, FileNotFoundError) as err:
        print(f"{name}: {err}", file=sys.stderr)
        return 2


# ---- needs a device
def open_device(index, stage):
    """makes HIP device `index` (an ordinal, or a device name such as 'cuda' or 'cuda:1') the current one and returns it"""
    if not torch.cuda.is_available():
        raise L.IrisError(f"{stage} needs a HIP device; there is no CPU path")
    if not isinstance(index, int):
        index = L.device_index(index)
    torch.cuda.set_device(index)
    return torch.device("cuda", index)


def open_training_set(args, device, ray_diff=True, cache_dir=None):
    """-> (files, scene, pixel set, n): load_training_files' dict, the Scene of its mesh, and the PixelSet of its views restricted to the n pixels that hit
    the mesh.  cache_dir: the baked shadings of the BRDF-CRF stage: attached to the pixel set, which then also keeps the hit positions."""
    from .dataset import PixelSet
    from .dataset.files import load_training_files
    from .path_tracing import load_scene
    dataset, root = args.dataset
    files = load_training_files(dataset, root, args.ldr_img_dir, has_part=args.has_part, res_scale=args.res_scale, cache_dir=cache_dir, device=device,
                                scene=args.scene)
    scene = load_scene(files["mesh_path"], device=device)
    ps = PixelSet(files["views"], files["img_hw"], files["rgb"], segmentation=files["segmentation"], int_albedo=files["int_albedo"], exposure=files["exposure"],
                  synthetic=files["synthetic"], batch_size=args.batch_size, device=device, ray_diff=ray_diff)
    if cache_dir is not None:
        ps.attach_cache(files["cache"])
    n = ps.restrict_to_hits(scene, store_positions=cache_dir is not None)
    if n == 0:
        raise L.IrisError("no training pixel hits the mesh")
    return files, scene, ps, n


def load_crf(crf_state, crf_basis, emor_path, device):
    """EmorCRF with the checkpoint's 'model_crf.' entries (render.py:130-135), on the device.  With no EMoR file at hand (no --emor_path, no crf/emor.txt under the
    working directory) the curves come from the checkpoint: they are buffers of the module, so it carries them."""
    from ..model.crf import EmorCRF
    if emor_path is None and not os.path.isfile(os.path.join(os.getcwd(), "crf", "emor.txt")) and "f0" in crf_state and "basis" in crf_state:
        model_crf = EmorCRF.from_arrays(crf_state["f0"][0], crf_state["basis"])
    else:
        model_crf = EmorCRF(crf_basis, emor_path=emor_path)
    model_crf.load_state_dict(crf_state)
    return model_crf.to(device)


def photograph_batches(views, img_hw, photographs, device, resize=False):
    """the batch dicts iris_amd.slf_bake's functions take, one per view, made as they are asked for: {'camera', 'img_hw', 'image' on the device (8-bit
    stays 8-bit), 'exposure'}.  resize (layout_resizes): an 8-bit photograph of another size is uploaded as it is and resized to img_hw on the device
    (utils.resize.resize_u8, linear: the reference's open_png); the smaller image never exists on the host."""
    from .resize import resize_u8
    for view, (path, exposure) in zip(views, photographs):
        image = torch.from_numpy(read_photograph(path, img_hw, resize)).to(device)
        if resize and image.dtype == torch.uint8:
            image = resize_u8(image, img_hw, "linear")
        yield {"camera": view, "img_hw": tuple(img_hw), "image": image, "exposure": exposure}


def freeze(*modules):
    """requires_grad = False on every parameter; a material network that is a plain callable has none"""
    for m in modules:
        if isinstance(m, torch.nn.Module):
            for p in m.parameters():
                p.requires_grad = False


def make_denoiser(kind, img_hw, device):
    """--denoise: the a-trous filter for (H, W) images, or None"""
    if kind != "atrous":
        return None
    from .denoise import Denoiser
    return Denoiser(img_hw[::-1], device)                  # denoiser = mitsuba.OptixDenoiser(img_hw[::-1])   (bake_shading.py:81)


def stack_maps(out, img_hw):
    """the 13 maps of bake_view / refine_view as the (13, H, W, 3) tensor MapWriter.submit takes: diffuse, then specular0 and specular1 of each roughness level"""
    return torch.stack([out["diffuse"]] + [out[k][r] for r in range(len(out["specular0"])) for k in ("specular0", "specular1")]).reshape(13, *img_hw, 3)
