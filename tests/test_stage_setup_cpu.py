"""The stage-setup module (iris_amd/utils/stage.py) on the CPU: the eight parsers still register exactly the options they registered before the setup
code was shared (the three trainers': before their options moved to iris_amd/utils/trainer.py), and the one mesh rule, view loader, checkpoint reader and material loader return what the stages' own copies returned."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden

# {stage: {dest: (option strings, type, default, choices, required, nargs)}}, read off parser._actions at the commit BEFORE the parsers were rebuilt on
# stage.add_common_options / add_ignored_trainer_options (bake_shading and refine_shading built theirs inside main() then: captured from parse_args);
# train_emitter and initialize: at the commit before the three trainers' parsers were rebuilt on trainer.add_trainer_options
PARSERS = {'bake_shading': {'help': (('-h', '--help'), None, '==SUPPRESS==', None, False, 0),
                  'dataset_root': (('--dataset_root',), str, None, None, False, None),
                  'scene': (('--scene',), str, None, None, True, None),
                  'slf_path': (('--slf_path',), str, None, None, True, None),
                  'emitter_path': (('--emitter_path',), str, None, None, True, None),
                  'output': (('--output',), str, None, None, True, None),
                  'dataset': (('--dataset',), str, None, None, True, None),
                  'ldr_img_dir': (('--ldr_img_dir',), str, None, None, False, None),
                  'res_scale': (('--res_scale',), float, 1.0, None, False, None),
                  'cameras': (('--cameras',), str, None, None, False, None),
                  'img_hw': (('--img_hw',), int, None, None, False, 2),
                  'spp_diffuse': (('--spp_diffuse',), int, 256, None, False, None),
                  'spps_specular': (('--spps_specular',), int, [64, 128, 128, 128, 128, 128], None, False, 6),
                  'seed': (('--seed',), int, 0, None, False, None),
                  'compression': (('--compression',), str, 'zip', ('none', 'zips', 'zip'), False, None),
                  'exr_encoder': (('--exr_encoder',), str, 'host', ('host', 'device'), False, None),
                  'overwrite': (('--overwrite',), None, False, None, False, 0),
                  'denoise': (('--denoise',), str, 'atrous', ('atrous', 'none'), False, None)},
 'refine_shading': {'help': (('-h', '--help'), None, '==SUPPRESS==', None, False, 0),
                    'dataset_root': (('--dataset_root',), str, None, None, False, None),
                    'scene': (('--scene',), str, None, None, True, None),
                    'slf_path': (('--slf_path',), str, None, None, True, None),
                    'emitter_path': (('--emitter_path',), str, None, None, True, None),
                    'output': (('--output',), str, None, None, True, None),
                    'ckpt': (('--ckpt',), str, None, None, False, None),
                    'dataset': (('--dataset',), str, None, None, True, None),
                    'ldr_img_dir': (('--ldr_img_dir',), str, None, None, False, None),
                    'res_scale': (('--res_scale',), float, 1.0, None, False, None),
                    'material': (('--material',), str, None, None, False, None),
                    'cameras': (('--cameras',), str, None, None, False, None),
                    'img_hw': (('--img_hw',), int, None, None, False, 2),
                    'spp_diffuse': (('--spp_diffuse',), int, 128, None, False, None),
                    'spp_specular': (('--spp_specular',), int, 64, None, False, None),
                    'indir_depth': (('--indir_depth',), int, 5, None, False, None),
                    'batch_rays': (('--batch_rays',), int, 20971520, None, False, None),
                    'seed': (('--seed',), int, 0, None, False, None),
                    'compression': (('--compression',), str, 'zip', ('none', 'zips', 'zip'), False, None),
                    'exr_encoder': (('--exr_encoder',), str, 'host', ('host', 'device'), False, None),
                    'overwrite': (('--overwrite',), None, False, None, False, 0),
                    'resume': (('--resume',), None, False, None, False, 0),
                    'denoise': (('--denoise',), str, 'atrous', ('atrous', 'none'), False, None)},
 'render': {'help': (('-h', '--help'), None, '==SUPPRESS==', None, False, 0),
            'experiment_name': (('--experiment_name',), str, None, None, True, None),
            'checkpoint_path': (('--checkpoint_path',), str, './checkpoints', None, False, None),
            'output_path': (('--output_path',), str, 'outputs/kitchen_output', None, False, None),
            'device': (('--device',), int, 0, None, False, None),
            'split': (('--split',), str, 'val', None, False, None),
            'ckpt': (('--ckpt',), str, 'last.ckpt', None, False, None),
            'light_type': (('--light_type',), str, 'slf', ('slf', 'area'), False, None),
            'dataset': (('--dataset',), str, ['synthetic', '../data/indoor_synthetic/kitchen'], None, False, 2),
            'scene': (('--scene',), str, '', None, False, None),
            'emitter_path': (('--emitter_path',), str, None, None, True, None),
            'SPP': (('--SPP',), int, 512, None, False, None),
            'spp': (('--spp',), int, 8, None, False, None),
            'indir_depth': (('--indir_depth',), int, 5, None, False, None),
            'crf_basis': (('--crf_basis',), int, 3, None, False, None),
            'res_scale': (('--res_scale',), float, 1.0, None, False, None),
            'ldr_img_dir': (('--ldr_img_dir',), str, None, None, False, None),
            'log_path': (('--log_path',), str, './logs', None, False, None),
            'batch_size': (('--batch_size',), int, None, None, False, None),
            'voxel_path': (('--voxel_path',), str, None, None, False, None),
            'num_workers': (('--num_workers',), int, None, None, False, None),
            'dir_val': (('--dir_val',), str, None, None, False, None),
            'val_step': (('--val_step',), int, None, None, False, None),
            'has_part': (('--has_part',), int, None, None, False, None),
            'load_crf': (('--load_crf',), int, None, None, False, None),
            'material': (('--material',), str, None, None, False, None),
            'cameras': (('--cameras',), str, None, None, False, None),
            'emor_path': (('--emor_path',), str, None, None, False, None),
            'denoise': (('--denoise',), str, 'atrous', ('atrous', 'none'), False, None),
            'compression': (('--compression',), str, 'zip', ('none', 'zips', 'zip'), False, None),
            'metrics': (('--metrics',), str, 'psnr', ('psnr', 'psnr,ssim'), False, None),
            'seed': (('--seed',), int, 0, None, False, None),
            'max_views': (('--max_views',), int, None, None, False, None)},
 'render_relight': {'help': (('-h', '--help'), None, '==SUPPRESS==', None, False, 0),
                    'experiment_name': (('--experiment_name',), str, None, None, True, None),
                    'mode': (('--mode',), str, 'train_val', ('train_val', 'traj'), False, None),
                    'log_path': (('--log_path',), str, './logs', None, False, None),
                    'checkpoint_path': (('--checkpoint_path',), str, './checkpoints', None, False, None),
                    'output_path': (('--output_path',), str, 'outputs/kitchen_output', None, False, None),
                    'device': (('--device',), int, 0, None, False, None),
                    'split': (('--split',), str, 'val', None, False, None),
                    'ckpt': (('--ckpt',), str, 'last.ckpt', None, False, None),
                    'anti_aliasing': (('--anti_aliasing',), int, 1, None, False, None),
                    'light_cfg': (('--light_cfg',), str, None, None, True, None),
                    'dataset': (('--dataset',), str, ['synthetic', '../data/indoor_synthetic/kitchen'], None, False, 2),
                    'scene': (('--scene',), str, '', None, False, None),
                    'emitter_path': (('--emitter_path',), str, None, None, True, None),
                    'SPP': (('--SPP',), int, 512, None, False, None),
                    'spp': (('--spp',), int, 8, None, False, None),
                    'indir_depth': (('--indir_depth',), int, 5, None, False, None),
                    'crf_basis': (('--crf_basis',), int, 3, None, False, None),
                    'res_scale': (('--res_scale',), float, 1.0, None, False, None),
                    'ldr_img_dir': (('--ldr_img_dir',), str, None, None, False, None),
                    'batch_size': (('--batch_size',), int, None, None, False, None),
                    'voxel_path': (('--voxel_path',), str, None, None, False, None),
                    'num_workers': (('--num_workers',), int, None, None, False, None),
                    'dir_val': (('--dir_val',), str, None, None, False, None),
                    'val_step': (('--val_step',), int, None, None, False, None),
                    'has_part': (('--has_part',), int, None, None, False, None),
                    'load_crf': (('--load_crf',), int, None, None, False, None),
                    'material': (('--material',), str, None, None, False, None),
                    'cameras': (('--cameras',), str, None, None, False, None),
                    'emor_path': (('--emor_path',), str, None, None, False, None),
                    'denoise': (('--denoise',), str, 'atrous', ('atrous', 'none'), False, None),
                    'compression': (('--compression',), str, 'zip', ('none', 'zips', 'zip'), False, None),
                    'seed': (('--seed',), int, 0, None, False, None),
                    'max_views': (('--max_views',), int, None, None, False, None),
                    'keep_lights': (('--keep_lights',), float, 0.0, None, False, None),
                    'sphere_subdiv': (('--sphere_subdiv',), int, 2, None, False, None)},
 'train_brdf_crf': {'help': (('-h', '--help'), None, '==SUPPRESS==', None, False, 0),
                    'batch_size': (('--batch_size',), int, 8192, None, False, None),
                    'dataset': (('--dataset',), str, ['synthetic', '../data/indoor_synthetic/kitchen'], None, False, 2),
                    'scene': (('--scene',), str, '', None, False, None),
                    'voxel_path': (('--voxel_path',), str, 'outputs/kitchen/vslf.npz', None, False, None),
                    'num_workers': (('--num_workers',), int, 12, None, False, None),
                    'dir_val': (('--dir_val',), str, 'val', None, False, None),
                    'val_step': (('--val_step',), int, 250, None, False, None),
                    'has_part': (('--has_part',), int, 1, None, False, None),
                    'res_scale': (('--res_scale',), float, 1.0, None, False, None),
                    'optimizer': (('--optimizer',), str, 'Adam', ('SGD', 'Ranger', 'Adam'), False, None),
                    'learning_rate': (('--learning_rate',), float, 0.001, None, False, None),
                    'weight_decay': (('--weight_decay',), float, 0, None, False, None),
                    'scheduler_rate': (('--scheduler_rate',), float, 0.5, None, False, None),
                    'milestones': (('--milestones',), int, [1000], None, False, '*'),
                    'le': (('--le',), float, 1.0, None, False, None),
                    'ld': (('--ld',), float, 0.0005, None, False, None),
                    'lp': (('--lp',), float, 0.005, None, False, None),
                    'ls': (('--ls',), float, 0.001, None, False, None),
                    'la': (('--la',), float, 0.0, None, False, None),
                    'sigma_albedo': (('--sigma_albedo',), float, 0.016666666666666666, None, False, None),
                    'sigma_pos': (('--sigma_pos',), float, 0.09999999999999999, None, False, None),
                    'ckpt_path': (('--ckpt_path',), str, None, None, False, None),
                    'emitter_path': (('--emitter_path',), str, None, None, False, None),
                    'freeze_emitter': (('--freeze_emitter',), int, 0, None, False, None),
                    'freeze_crf': (('--freeze_crf',), int, 0, None, False, None),
                    'indir_depth': (('--indir_depth',), int, 5, None, False, None),
                    'SPP': (('--SPP',), int, 512, None, False, None),
                    'spp': (('--spp',), int, 8, None, False, None),
                    'ldr_img_dir': (('--ldr_img_dir',), str, None, None, False, None),
                    'crf_basis': (('--crf_basis',), int, 3, None, False, None),
                    'load_crf': (('--load_crf',), int, 0, None, False, None),
                    'l_crf_increasing': (('--l_crf_increasing',), float, 0.1, None, False, None),
                    'l_crf_weight': (('--l_crf_weight',), float, 0.001, None, False, None),
                    'experiment_name': (('--experiment_name',), str, None, None, True, None),
                    'max_epochs': (('--max_epochs',), int, 500, None, False, None),
                    'log_path': (('--log_path',), str, './logs', None, False, None),
                    'ft': (('--ft',), str, None, None, False, None),
                    'checkpoint_path': (('--checkpoint_path',), str, './checkpoints', None, False, None),
                    'resume': (('--resume',), None, False, None, False, 0),
                    'device': (('--device',), int, 0, None, False, None),
                    'val_frame': (('--val_frame',), int, 0, None, False, None),
                    'cache_dir': (('--cache_dir',), str, None, None, False, None),
                    'log_every': (('--log_every',), int, 50, None, False, None)},
 'train_emitter': {'help': (('-h', '--help'), None, '==SUPPRESS==', None, False, 0),
                   'batch_size': (('--batch_size',), int, 8192, None, False, None),
                   'dataset': (('--dataset',), str, ['synthetic', '../data/indoor_synthetic/kitchen'], None, False, 2),
                   'scene': (('--scene',), str, '', None, False, None),
                   'voxel_path': (('--voxel_path',), str, 'outputs/kitchen/vslf.npz', None, False, None),
                   'num_workers': (('--num_workers',), int, 12, None, False, None),
                   'dir_val': (('--dir_val',), str, 'val', None, False, None),
                   'val_step': (('--val_step',), int, 250, None, False, None),
                   'has_part': (('--has_part',), int, 1, None, False, None),
                   'res_scale': (('--res_scale',), float, 1.0, None, False, None),
                   'optimizer': (('--optimizer',), str, 'Adam', ('SGD', 'Ranger', 'Adam'), False, None),
                   'learning_rate': (('--learning_rate',), float, 0.001, None, False, None),
                   'weight_decay': (('--weight_decay',), float, 0, None, False, None),
                   'scheduler_rate': (('--scheduler_rate',), float, 0.5, None, False, None),
                   'milestones': (('--milestones',), int, [1000], None, False, '*'),
                   'le': (('--le',), float, 1.0, None, False, None),
                   'ld': (('--ld',), float, 0.0005, None, False, None),
                   'lp': (('--lp',), float, 0.005, None, False, None),
                   'ls': (('--ls',), float, 0.001, None, False, None),
                   'la': (('--la',), float, 0.0, None, False, None),
                   'sigma_albedo': (('--sigma_albedo',), float, 0.016666666666666666, None, False, None),
                   'sigma_pos': (('--sigma_pos',), float, 0.09999999999999999, None, False, None),
                   'ckpt_path': (('--ckpt_path',), str, None, None, False, None),
                   'emitter_path': (('--emitter_path',), str, None, None, False, None),
                   'freeze_emitter': (('--freeze_emitter',), int, 0, None, False, None),
                   'freeze_crf': (('--freeze_crf',), int, 0, None, False, None),
                   'indir_depth': (('--indir_depth',), int, 5, None, False, None),
                   'SPP': (('--SPP',), int, 512, None, False, None),
                   'spp': (('--spp',), int, 8, None, False, None),
                   'ldr_img_dir': (('--ldr_img_dir',), str, None, None, False, None),
                   'crf_basis': (('--crf_basis',), int, 3, None, False, None),
                   'load_crf': (('--load_crf',), int, 0, None, False, None),
                   'l_crf_increasing': (('--l_crf_increasing',), float, 0.1, None, False, None),
                   'l_crf_weight': (('--l_crf_weight',), float, 0.001, None, False, None),
                   'experiment_name': (('--experiment_name',), str, None, None, True, None),
                   'max_epochs': (('--max_epochs',), int, 500, None, False, None),
                   'log_path': (('--log_path',), str, './logs', None, False, None),
                   'ft': (('--ft',), str, None, None, False, None),
                   'checkpoint_path': (('--checkpoint_path',), str, './checkpoints', None, False, None),
                   'resume': (('--resume',), None, False, None, False, 0),
                   'device': (('--device',), int, 0, None, False, None),
                   'val_frame': (('--val_frame',), int, 0, None, False, None),
                   'emor_path': (('--emor_path',), str, None, None, False, None),
                   'log_every': (('--log_every',), int, 50, None, False, None)},
 'export': {'help': (('-h', '--help'), None, '==SUPPRESS==', None, False, 0),
            'mesh': (('--mesh',), None, None, None, False, None),
            'ckpt': (('--ckpt',), None, None, None, False, None),
            'emitter_path': (('--emitter_path',), None, None, None, False, None),
            'dir_save': (('--dir_save',), None, None, None, False, None),
            'device': (('--device',), None, 'cuda', None, False, None),
            'tex_res': (('--tex_res',), int, 2048, None, False, None),
            'chunk_size': (('--chunk_size',), int, 160000, None, False, None),
            'material': (('--material',), str, None, None, False, None),
            'atlas': (('--atlas',), str, 'auto', ('auto', 'files', 'grid'), False, None),
            'write_obj': (('--write_obj',), None, False, None, False, 0)}}
PARSERS['initialize'] = PARSERS['train_emitter']          # captured apart at the same commit: the two tables were equal option for option


def _table(parser):
    return {a.dest: (tuple(a.option_strings), a.type, a.default, None if a.choices is None else tuple(a.choices), a.required, a.nargs) for a in parser._actions}


def test_the_eight_parsers_register_what_they_registered_before():
    """the six stages of the setup module's first round, and train_emitter and initialize; option order is free, everything else is not"""
    from iris_amd import bake_shading, initialize, refine_shading, render, render_relight, train_brdf_crf, train_emitter
    from iris_amd.utils import export
    built = {"bake_shading": bake_shading.build_parser(), "refine_shading": refine_shading.build_parser(), "render": render.build_parser(),
             "render_relight": render_relight.build_parser(), "train_brdf_crf": train_brdf_crf.parser(), "train_emitter": train_emitter.parser(),
             "initialize": initialize.parser(), "export": export.build_parser()}
    assert set(built) == set(PARSERS)
    for name, parser in built.items():
        assert _table(parser) == PARSERS[name], name
    for name in ("train_brdf_crf", "train_emitter", "initialize"):
        assert built[name].prog == "python -m iris_amd." + name


# ---- mesh_path
def _parent_bake_refine(dataset, dataset_root, scene):
    """the rule bake_shading.main and refine_shading.main carried; None where their assert fired"""
    if dataset in ("synthetic", "real"):
        p = os.path.join(scene, "scene.obj")
    elif dataset == "scannetpp":
        p = os.path.join(dataset_root, "data", scene, "scans", "scene.ply")
    else:
        p = os.path.join(scene, "scene.obj") if os.path.exists(os.path.join(scene, "scene.obj")) else os.path.join(scene, "scene.ply")
    return p if os.path.exists(p) else None


def _parent_render(name, path, scene):
    """the rule render.main and render_relight.main carried"""
    if name == "scannetpp":
        p = os.path.join(path, "data", scene, "scans", "scene.ply")
    else:
        p = os.path.join(path, "scene.obj")
        if not os.path.exists(p) and os.path.exists(os.path.join(path, "scene.ply")):
            p = os.path.join(path, "scene.ply")
    return p if os.path.exists(p) else None


def _parent_training_files(root):
    p = os.path.join(root, "scene.obj")
    return p if os.path.exists(p) else None


LAYOUTS = {"obj": ["scene.obj"], "ply": ["scene.ply"], "both": ["scene.obj", "scene.ply"], "neither": [], "scannetpp": ["data/room/scans/scene.ply"]}


@pytest.mark.parametrize("dataset", ["synthetic", "real", "scannetpp", "generic"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_mesh_path_decision_table(tmp_path, dataset, layout):
    from iris_amd._lib import IrisError
    from iris_amd.utils.stage import mesh_path
    root = str(tmp_path / "root")
    os.makedirs(root)
    for rel in LAYOUTS[layout]:
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        open(os.path.join(root, rel), "w").close()
    if dataset == "scannetpp":
        want = os.path.join(root, "data", "room", "scans", "scene.ply") if layout == "scannetpp" else None
    else:
        want = {"obj": "scene.obj", "ply": "scene.ply", "both": "scene.obj"}.get(layout)
        want = want and os.path.join(root, want)
    if want is None:
        with pytest.raises(IrisError, match="mesh not found: "):
            mesh_path(dataset, root, "room")
    else:
        assert mesh_path(dataset, root, "room") == want
    # whatever a stage accepted before is returned unchanged (bake and refine name the scene's folder --scene, and for scannetpp the root --dataset_root)
    before = [_parent_bake_refine(dataset, root, "room" if dataset == "scannetpp" else root), _parent_render(dataset, root, "room")]
    if dataset in ("synthetic", "real"):
        before.append(_parent_training_files(root))
    for p in before:
        if p is not None:
            assert mesh_path(dataset, root, "room") == p


# ---- load_views
H, W = 4, 6


def _c2w(k):
    a = 0.3 * (k + 1)
    return [[np.cos(a), 0.0, np.sin(a), 0.1 * k], [0.0, 1.0, 0.0, 0.2], [-np.sin(a), 0.0, np.cos(a), 0.3 - k], [0.0, 0.0, 0.0, 1.0]]


def _synthetic_scene(root):
    from iris_amd.utils import exr
    meta = {}
    for split, angle, first in (("train", 1.2, 0), ("val", 0.9, 5)):
        os.makedirs(os.path.join(root, split, "Image"))
        exr.write_exr(os.path.join(root, split, "Image", "000_0001.exr"), np.zeros((H, W, 3), np.float32))
        meta[split] = {"camera_angle_x": angle, "frames": [{"transform_matrix": _c2w(first + k)} for k in range(2)]}
        with open(os.path.join(root, split, "transforms.json"), "w") as fh:
            json.dump(meta[split], fh)
    return meta


def _real_scene(root, n=12):
    from iris_amd.utils import exr
    os.makedirs(os.path.join(root, "Image"))
    exr.write_exr(os.path.join(root, "Image", "000_0001.exr"), np.zeros((H, W, 3), np.float32))
    rows, ks = [str(n)], [str(n)]
    for i in range(n):
        o = np.array([i * 0.1, 0.2, 0.3]); at = np.array([0.0, 1.0, 0.0]); up = np.array([0.0, 0.0, 1.0])
        rows += [" ".join(map(str, o)), " ".join(map(str, o + at)), " ".join(map(str, up))]
        ks += ["%d 0 3" % (5 + i), "0 %d 2" % (5 + i), "0 0 1"]
    with open(os.path.join(root, "cam.txt"), "w") as fh:
        fh.write("\n".join(rows))
    with open(os.path.join(root, "K_list.txt"), "w") as fh:
        fh.write("\n".join(ks))


def _scannetpp_scene(root, scene="sc0"):
    g = golden("scannetpp_cameras.npz")
    d = os.path.join(root, "data", scene, "psdf")
    os.makedirs(d)
    with open(os.path.join(d, "train_test_lists.json"), "w") as fh:
        fh.write(str(g["lists_json"]))
    with open(os.path.join(d, "transforms_all.json"), "w") as fh:
        fh.write(str(g["transforms_json"]))


def _same_views(got, want):
    assert got[0] == want[0] and len(got[1]) == len(want[1]) > 0
    for a, b in zip(got[1], want[1]):
        assert set(a) == set(b)
        for k in a:
            if isinstance(b[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k


@pytest.mark.parametrize("res_scale", [1.0, 0.5])
def test_load_views_equals_the_per_dataset_loaders(tmp_path, res_scale):
    from iris_amd._lib import IrisError
    from iris_amd.utils import cameras
    from iris_amd.utils.stage import load_views
    syn, real, spp = (str(tmp_path / n) for n in ("syn", "real", "spp"))
    meta = _synthetic_scene(syn)
    _real_scene(real)
    _scannetpp_scene(spp)
    hw = (int(H * res_scale), int(W * res_scale))
    for split in ("train", "val"):
        got = load_views("synthetic", syn, "", res_scale, split=split)
        _same_views(got, cameras.load_synthetic(syn, res_scale, split=split))
        # ... and what the reference's dataset computes from this split's transforms.json (synthetic_ldr.py:129-150), written out
        focal = float(0.5 * hw[1] / np.tan(0.5 * meta[split]["camera_angle_x"]))
        assert got[0] == hw and len(got[1]) == 2
        for v, f in zip(got[1], meta[split]["frames"]):
            assert v["kind"] == "synthetic" and v["focal"] == focal
            assert np.array_equal(v["c2w"], np.asarray(f["transform_matrix"], np.float32)[:3, :4])
        got = load_views("real", real, "", res_scale, split=split)
        _same_views(got, cameras.load_real(real, res_scale, split=split))
        assert got[0] == hw and len(got[1]) == (10 if split == "train" else 2)
    assert load_views("synthetic", syn, "", res_scale)[1][0]["focal"] == load_views("synthetic", syn, "", res_scale, split="train")[1][0]["focal"]     # the default split
    _same_views(load_views("synthetic", syn, "", res_scale, img_hw=(8, 10)), cameras.load_synthetic(syn, res_scale, (8, 10)))          # --img_hw: the file is not opened
    _same_views(load_views("real", real, "", res_scale, img_hw=(8, 10)), cameras.load_real(real, res_scale, (8, 10)))
    for split in ("train", "test"):
        _same_views(load_views("scannetpp", spp, "sc0", res_scale, split=split), cameras.load_scannetpp(spp, "sc0", res_scale, split=split))
    assert len(load_views("scannetpp", spp, "sc0", res_scale)[1]) == 5
    with pytest.raises(IrisError, match=r"synthetic \| real \| scannetpp, or --cameras"):
        load_views("generic", syn, "", res_scale)


def test_load_views_generic_json_and_its_extras(tmp_path):
    from iris_amd.utils import cameras
    from iris_amd.utils.stage import load_views
    folder = tmp_path / "cams"
    folder.mkdir()
    K = [[5.0, 0, 3], [0, 5.0, 2], [0, 0, 1]]
    views = [{"K": K, "c2w": _c2w(0)[:3], "image": "photos/a.exr", "exposure": 1.2}, {"K": K, "c2w": _c2w(1)[:3], "image": str(tmp_path / "abs.png")}, {"K": K, "c2w": _c2w(2)[:3]}]
    path = str(folder / "cameras.json")
    with open(path, "w") as fh:
        json.dump({"img_hw": [H, W], "views": views}, fh)
    cwd = os.getcwd()
    os.chdir(tmp_path)                                     # a relative image path is taken from the JSON file's folder, not from the working directory
    try:
        plain = load_views("generic", "unused", "", 0.5, cameras_json=os.path.join("cams", "cameras.json"))
        rich = load_views("synthetic", "unused", "", 0.5, split="val", cameras_json=os.path.join("cams", "cameras.json"), extras=True)
    finally:
        os.chdir(cwd)
    _same_views(plain, cameras.load_generic(path, 0.5))
    assert plain[0] == (2, 3) and all(set(v) == {"kind", "K", "c2w"} for v in plain[1])
    assert rich[0] == plain[0]
    for r, p in zip(rich[1], plain[1]):
        assert np.array_equal(r["K"], p["K"]) and np.array_equal(r["c2w"], p["c2w"]) and r["kind"] == p["kind"]
    assert [v["image"] for v in rich[1]] == [str(folder / "photos/a.exr"), str(tmp_path / "abs.png"), None]
    assert [v["exposure"] for v in rich[1]] == [1.2, 1.0, 1.0]


# ---- checkpoints
def _states():
    g = torch.Generator().manual_seed(5)
    material = {"mlp.params": torch.rand(40, generator=g)}
    crf = {"weight": torch.rand(3, 3, generator=g), "f0": torch.rand(1, 16, generator=g), "basis": torch.rand(3, 16, generator=g)}
    return material, crf


def _reference_idiom(state_dict, prefix):
    """refine_shading.py:84-89"""
    weight = {}
    for k, v in state_dict.items():
        if prefix + "." in k:
            weight[k.replace(prefix + ".", "")] = v
    return weight


def test_checkpoint_round_trip_and_prefix_split(tmp_path):
    from iris_amd import train_brdf_crf
    from iris_amd.utils import stage
    assert train_brdf_crf.read_checkpoint is stage.read_checkpoint and train_brdf_crf.write_checkpoint is stage.write_checkpoint
    material, crf = _states()
    path = str(tmp_path / "exp" / "last.ckpt")
    stage.write_checkpoint(path, material, crf, {"state": {}, "param_groups": [{"lr": 1e-3}]}, epoch=3, global_step=41, hyper_parameters={"learning_rate": 2e-3})
    ck = stage.read_checkpoint(path)
    assert ck["epoch"] == 3 and ck["global_step"] == 41 and ck["hyper_parameters"] == {"learning_rate": 2e-3}
    assert ck["optimizer_states"] == [{"state": {}, "param_groups": [{"lr": 1e-3}]}]
    assert set(ck["state_dict"]) == {"material.mlp.params", "model_crf.weight", "model_crf.f0", "model_crf.basis"}
    for prefix, want in (("material", material), ("model_crf", crf)):
        ref = _reference_idiom(ck["state_dict"], prefix)
        assert set(ck[prefix]) == set(ref) == set(want)
        for k in want:
            assert torch.equal(ck[prefix][k], ref[k]) and torch.equal(ck[prefix][k], want[k])
    assert not os.path.exists(path + ".tmp")


def test_a_checkpoint_with_python_objects_loads_through_the_fallback(tmp_path):
    from iris_amd.utils import stage
    material, crf = _states()
    state = {"material." + k: v for k, v in material.items()}
    state.update({"model_crf." + k: v for k, v in crf.items()})
    path = str(tmp_path / "lightning.ckpt")
    torch.save({"state_dict": state, "hyper_parameters": argparse.Namespace(batch_size=8192, dataset=["real", "dir"])}, path)
    with pytest.raises(Exception):
        torch.load(path, map_location="cpu", weights_only=True)             # the tensors-only unpickler refuses the Namespace: the first attempt fails
    assert stage.load_pickled(path)["hyper_parameters"].batch_size == 8192
    ck = stage.read_checkpoint(path)
    assert ck["hyper_parameters"].dataset == ["real", "dir"]
    assert torch.equal(ck["material"]["mlp.params"], material["mlp.params"]) and set(ck["model_crf"]) == set(crf)
    slf = str(tmp_path / "vslf.npz")
    torch.save({"mask": torch.ones(2, 2, 2, dtype=torch.bool), "voxel_min": -1.5, "voxel_max": torch.tensor(2.5), "note": argparse.Namespace()}, slf)
    assert stage.voxel_range(slf) == (-1.5, 2.5)


# ---- load_material
def factory_three(voxel_min, voxel_max, ckpt):
    return ("three", voxel_min, voxel_max, ckpt)


def factory_two(voxel_min, voxel_max):
    return ("two", voxel_min, voxel_max)


def factory_none():
    return ("none",)


def test_load_material_reaches_each_factory_signature(tmp_path):
    import stub_material
    from iris_amd._lib import IrisError
    from iris_amd.utils.stage import load_material
    slf = str(tmp_path / "vslf.npz")
    torch.save({"voxel_min": -1.5, "voxel_max": 2.5}, slf)
    assert load_material(__name__ + ":factory_three", slf, "last.ckpt") == ("three", -1.5, 2.5, "last.ckpt")
    assert load_material(__name__ + ":factory_two", slf, None) == ("two", -1.5, 2.5)
    assert load_material(__name__ + ":factory_none", slf, "last.ckpt") == ("none",)
    assert load_material(__name__ + ":factory_none", slf, None) == ("none",)
    for ckpt in ("last.ckpt", None):
        assert isinstance(load_material("stub_material:material", slf, ckpt), stub_material.StubMaterial)
    assert isinstance(load_material("stub_material", slf, None), stub_material.StubMaterial)            # no attribute named: 'material'
    with pytest.raises(IrisError) as err:
        load_material(None, slf, None)
    assert str(err.value) == ("refine_shading: --ckpt (the checkpoint holding the NGPBRDF weights, refine_shading.py:36,84) or --material pkg.module:factory "
                              "is required")


# ---- the small blocks
def test_view_seed_torch_seeds_the_generator():
    from iris_amd.utils.stage import view_seed_torch
    before = torch.get_rng_state()
    try:
        for seed, i in ((0, 0), (2, 1), (7, 123)):
            view_seed_torch(seed, i)
            assert torch.initial_seed() == seed * 1000003 + i
    finally:
        torch.set_rng_state(before)


def test_freeze_stack_maps_and_no_denoiser():
    from iris_amd.utils import stage
    net, other = torch.nn.Linear(3, 2), torch.nn.Linear(2, 2)
    stage.freeze(net, lambda x: x, other)                  # a material network may be a plain callable
    assert not any(p.requires_grad for m in (net, other) for p in m.parameters())
    g = torch.Generator().manual_seed(1)
    out = {"diffuse": torch.rand(H * W, 3, generator=g), "specular0": [torch.rand(H * W, 3, generator=g) for _ in range(6)],
           "specular1": [torch.rand(H * W, 3, generator=g) for _ in range(6)]}
    want = torch.stack([out["diffuse"]] + [out[k][r] for r in range(6) for k in ("specular0", "specular1")]).reshape(13, H, W, 3)
    assert torch.equal(stage.stack_maps(out, (H, W)), want)
    assert stage.make_denoiser("none", (H, W), "cpu") is None
