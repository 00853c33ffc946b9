"""Light insertion of the relighting stage, host side (iris_amd/utils/lights.py): the reference's transform chain, the tessellations, the disco ball, the
composition of the box room with inserted lights, the configuration parser and the command line.  No GPU."""
import math

import numpy as np
import pytest

from conftest import golden
from iris_amd._lib import IrisError
from iris_amd.utils import lights as LT

KITCHEN_TO_WORLD = [{"type": "translate", "value": [0.068418, 3.2243, 0.85067]}, {"type": "scale", "value": [0.4, 0.4, 0.4]},
                    {"type": "rotate", "axis": [1, 0, 0], "angle": 90}]

CONFIG_TEXT = """
type: 'scene'
PerspectiveCamera:
  type: 'perspective'
  fov: 45
Integrator:
  type: 'path'
  max_depth: 7
main_scene:
  type: 'ply'
  filename: ''
light_plane:
  type: 'rectangle'
  to_world:
    - type: 'translate'
      value: [0.068418, 3.2243, 0.85067]
    - type: 'scale'
      value: [0.4, 0.4, 0.4]
    - type: 'rotate'
      axis: [1, 0, 0]
      angle: 90
  bsdf:
    type: 'twosided'
    bsdf:
      type: 'diffuse'
      reflectance:
        type: 'rgb'
        value: [0., 0., 0.]
  emitter:
    type: 'area'
    radiance:
      type: 'rgb'
      value: [20, 20, 20]
mirror_ball:
  type: 'sphere'
  to_world:
    - type: 'translate'
      value: [1.0, 1.0, 0.5]
    - type: 'scale'
      value: [0.25, 0.25, 0.25]
  bsdf:
    type: 'conductor'
    material: 'none'
disco_ball:
  position: [0.5, 0.5, 1.5]
  radius: 0.2
  light_intensity: 30
  light_num: 40
  light_radius_rate: 0.1
  spot_intensity: 10
  spot_cutoff_angle: 20.0
  T: 120
"""
CONFIG_DICT = {
    "type": "scene", "PerspectiveCamera": {"type": "perspective", "fov": 45}, "Integrator": {"type": "path", "max_depth": 7}, "main_scene": {"type": "ply", "filename": ""},
    "light_plane": {"type": "rectangle", "to_world": KITCHEN_TO_WORLD,
                    "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0., 0., 0.]}}},
                    "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [20, 20, 20]}}},
    "mirror_ball": {"type": "sphere", "to_world": [{"type": "translate", "value": [1.0, 1.0, 0.5]}, {"type": "scale", "value": [0.25, 0.25, 0.25]}],
                    "bsdf": {"type": "conductor", "material": "none"}},
    "disco_ball": {"position": [0.5, 0.5, 1.5], "radius": 0.2, "light_intensity": 30, "light_num": 40, "light_radius_rate": 0.1, "spot_intensity": 10,
                   "spot_cutoff_angle": 20.0, "T": 120},
}


def test_transform_chain_kitchen_rectangle():
    """configs/fipt/kitchen/relight_1.yaml: translate, scale 0.4, rotate 90 degrees about x, chained as render_relight.py:66-76 does (M = T1 T2 T3)"""
    M = LT.to_world_matrix(KITCHEN_TO_WORLD)
    v, f = LT.rectangle_mesh()
    p = LT.transform_points(M, v)
    np.testing.assert_allclose(p[:, 1], 3.2243, atol=1e-6)
    np.testing.assert_allclose([p[:, 0].min(), p[:, 0].max()], [-0.331582, 0.468418], atol=1e-6)
    np.testing.assert_allclose([p[:, 2].min(), p[:, 2].max()], [0.45067, 1.25067], atol=1e-6)
    corners = {(round(x, 6), round(z, 6)) for x, _, z in p}
    assert corners == {(-0.331582, 0.45067), (0.468418, 0.45067), (0.468418, 1.25067), (-0.331582, 1.25067)}
    for t in f:
        n = np.cross(p[t[1]] - p[t[0]], p[t[2]] - p[t[0]])
        np.testing.assert_allclose(n / np.linalg.norm(n), [0.0, -1.0, 0.0], atol=1e-6)
    with pytest.raises(IrisError, match="shear"):
        LT.to_world_matrix([{"type": "shear"}], "thing.to_world")


@pytest.mark.parametrize("subdiv,nf,nv,ratio", [(0, 20, 12, 0.761918), (1, 80, 42, 0.928345), (2, 320, 162, 0.981178), (3, 1280, 642, 0.995235)])
def test_icosphere(subdiv, nf, nv, ratio):
    V, F = LT.icosphere(subdiv)
    assert V.dtype == np.float64 and V.shape == (nv, 3) and F.shape == (nf, 3)
    np.testing.assert_allclose(np.linalg.norm(V, axis=1), 1.0, atol=1e-12, rtol=0)
    edges = {}
    for a, b, c in F:
        for e in ((a, b), (b, c), (c, a)):
            edges.setdefault((min(e), max(e)), []).append(e)
    assert all(len(v) == 2 and v[0] == v[1][::-1] for v in edges.values())          # closed, consistently oriented
    n = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    assert ((n * V[F].mean(1)).sum(1) > 0).all()                                      # outward
    area = 0.5 * np.linalg.norm(n, axis=1).sum()
    assert abs(area / (4 * math.pi) - ratio) <= 1e-6
    assert abs(LT.ICOSPHERE_AREA_RATIO[subdiv] - ratio) == 0


@pytest.mark.parametrize("timestep", [0, 13])
def test_expand_disco_ball(timestep):
    """against a restatement of utils/disco_ball.py's lattice formula"""
    params = {"position": [0.5, -0.25, 1.5], "radius": 0.2, "light_intensity": 30.0, "light_num": 7, "light_radius_rate": 0.1, "spot_intensity": 10.0,
              "spot_cutoff_angle": 20.0, "T": 120}
    shapes, spots = LT.expand_disco_ball(params, timestep)
    n, radius, pos = 7, 0.2, np.array(params["position"])
    phase = timestep * 2 * math.pi / 120
    phi = (1 + math.sqrt(5)) / 2
    pts = []
    for i in range(n):
        theta = 2 * math.pi * i / phi
        z = 1 - (2 * i + 1) / n
        r = math.sqrt(1 - z * z)
        pts.append([r * math.cos(theta + phase), r * math.sin(theta + phase), z])
    pts = np.array(pts)
    colors = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1]], float)
    lr = radius * 0.1
    assert len(shapes) == n + 1 and len(spots) == n
    centre = shapes[0]
    assert centre["name"] == "disco_ball" and centre["type"] == "sphere" and centre["radiance"] is None
    np.testing.assert_allclose(centre["material"], [0.2, 0.2, 0.2, 1.0, 0.0])
    np.testing.assert_allclose(centre["M"], np.array([[radius, 0, 0, pos[0]], [0, radius, 0, pos[1]], [0, 0, radius, pos[2]], [0, 0, 0, 1]]), atol=1e-15)
    for i in range(n):
        sh, sp = shapes[1 + i], spots[i]
        assert sh["type"] == "sphere" and sh["material"] is None
        np.testing.assert_allclose(sh["M"][:3, 3], pts[i] * (radius - lr * 0.6) + pos, atol=1e-14)
        np.testing.assert_allclose(sh["M"][:3, :3], np.eye(3) * lr, atol=1e-15)
        np.testing.assert_allclose(sh["radiance"], colors[i % 6] * 30.0)
        np.testing.assert_allclose(sp["origin"], pts[i] * (radius + lr) + pos, atol=1e-14)
        np.testing.assert_allclose(sp["axis"], pts[i], atol=1e-12)
        np.testing.assert_allclose(sp["intensity"], colors[i % 6] * 10.0)
        assert sp["cutoff"] == math.radians(20.0) and sp["beam"] == 0.75 * math.radians(20.0)


def _box_lights(scale=0.3):
    return LT.parse_light_config({
        "panel": {"type": "rectangle", "to_world": [{"type": "translate", "value": [2.0, 1.5, 2.0]}, {"type": "scale", "value": [scale, scale, scale]},
                                                    {"type": "rotate", "axis": [1, 0, 0], "angle": 180}],
                  "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [5.0, 6.0, 7.0]}}},
        "ball": {"type": "sphere", "to_world": [{"type": "translate", "value": [1.0, 1.0, 0.5]}, {"type": "scale", "value": [0.3, 0.3, 0.3]}],
                 "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.6, 0.5]}}},
        "lamp": {"type": "spot", "origin": [2.0, 1.5, 2.0], "target": [2.0, 1.5, 0.0], "cutoff_angle": 30.0, "intensity": {"type": "rgb", "value": [3.0, 3.0, 3.0]}},
    })


def _box_state(g):
    import torch
    tri = g["verts"][g["faces"][g["is_emitter"]]]
    return {"is_emitter": torch.from_numpy(g["is_emitter"]), "emitter_vertices": torch.from_numpy(tri.astype(np.float32)),
            "emitter_area": torch.from_numpy(g["emitter_area"]), "emitter_radiance": torch.from_numpy(g["emitter_radiance"])}


def test_compose_box_room():
    g = golden("bake_box.npz")
    s = 0.3
    c = LT.compose(g["verts"], g["faces"], _box_state(g), _box_lights(s))
    nv0, nf0 = g["verts"].shape[0], g["faces"].shape[0]
    assert nf0 == 14 and c["faces"].shape[0] == 14 + 2 + 320 and c["verts"].shape[0] == nv0 + 4 + 162
    np.testing.assert_array_equal(c["verts"][:nv0], g["verts"])
    np.testing.assert_array_equal(c["faces"][:nf0], g["faces"])                   # the room's triangles first, indices unchanged
    assert c["faces"].max() < c["verts"].shape[0] and c["faces"].min() >= 0
    surf = c["surf"]
    assert surf.dtype == np.int32
    np.testing.assert_array_equal(surf[:12], 0)
    np.testing.assert_array_equal(surf[12:14], -1)                               # the ceiling lamp, switched off
    np.testing.assert_array_equal(surf[14:16], 0)                                # the inserted emissive rectangle
    np.testing.assert_array_equal(surf[16:], 1)                                  # the diffuse sphere
    np.testing.assert_allclose(c["cmat"], [[0.7, 0.6, 0.5, 1.0, 0.0]])
    em = c["emitter"]
    ie = em["is_emitter"].numpy()
    assert ie.dtype == bool and ie.sum() == 2 and ie[14:16].all()                # absorbers are not in the table
    np.testing.assert_allclose(em["emitter_area"].numpy(), [2 * s * s, 2 * s * s], rtol=1e-6)
    np.testing.assert_array_equal(em["emitter_radiance"].numpy(), np.array([[5, 6, 7], [5, 6, 7]], np.float32))
    np.testing.assert_array_equal(em["emitter_vertices"].numpy(), c["verts"][c["faces"][14:16]])
    n = np.cross(c["verts"][c["faces"][14, 1]] - c["verts"][c["faces"][14, 0]], c["verts"][c["faces"][14, 2]] - c["verts"][c["faces"][14, 0]])
    assert n[2] < 0 and abs(n[0]) + abs(n[1]) < 1e-6                             # rotated by 180 degrees about x: faces down
    assert c["spots"].shape == (1, LT.SPOT_ROW) and c["spot_intensity"].shape == (1, 3)
    np.testing.assert_allclose(c["spots"][0, :6], [2.0, 1.5, 2.0, 0.0, 0.0, -1.0])
    np.testing.assert_allclose(c["spots"][0, 6:], [math.radians(30), math.radians(22.5), math.cos(math.radians(30)), math.cos(math.radians(22.5))], rtol=1e-6)
    # keep_lights = 0.5: the lamp stays, halved; nothing is an absorber
    k = LT.compose(g["verts"], g["faces"], _box_state(g), _box_lights(s), keep_lights=0.5)
    assert (k["surf"] >= 0).all() and k["emitter"]["is_emitter"].numpy().sum() == 4
    np.testing.assert_array_equal(np.nonzero(k["emitter"]["is_emitter"].numpy())[0], [12, 13, 14, 15])
    np.testing.assert_array_equal(k["emitter"]["emitter_radiance"].numpy()[:2], g["emitter_radiance"][:2] * np.float32(0.5))
    np.testing.assert_array_equal(k["emitter"]["emitter_area"].numpy()[:2], g["emitter_area"])
    # the dict is a file AreaEmitter's loader reads
    assert set(em) == {"is_emitter", "emitter_vertices", "emitter_area", "emitter_radiance"}
    with pytest.raises(IrisError):
        LT.compose(g["verts"], g["faces"][:13], _box_state(g), None)


def _check_parsed(lights):
    assert [s["name"] for s in lights.shapes] == ["light_plane", "mirror_ball"] and not lights.spots
    plane, ball = lights.shapes
    assert plane["type"] == "rectangle" and plane["material"] is None
    np.testing.assert_allclose(plane["radiance"], [20, 20, 20])
    np.testing.assert_allclose(plane["M"], LT.to_world_matrix(KITCHEN_TO_WORLD))
    assert ball["type"] == "sphere" and ball["radiance"] is None
    np.testing.assert_allclose(ball["material"], [1, 1, 1, 0.02, 1])
    assert lights.disco["light_num"] == 40 and lights.disco["T"] == 120
    at3 = lights.at(3)
    assert at3.disco is None and len(at3.shapes) == 2 + 41 and len(at3.spots) == 40


def test_parse_light_config_dict():
    _check_parsed(LT.parse_light_config(CONFIG_DICT))
    with pytest.raises(IrisError, match="teapot"):
        LT.parse_light_config({"teapot": {"type": "obj", "filename": "teapot.obj"}})
    with pytest.raises(IrisError, match="glass_ball.*dielectric"):
        LT.parse_light_config({"glass_ball": {"type": "sphere", "bsdf": {"type": "dielectric"}}})
    with pytest.raises(IrisError, match="gold_ball"):
        LT.parse_light_config({"gold_ball": {"type": "sphere", "bsdf": {"type": "twosided", "bsdf": {"type": "conductor", "material": "Au"}}}})


def test_parse_light_config_yaml():
    yaml = pytest.importorskip("yaml")
    cfg = yaml.safe_load(CONFIG_TEXT)
    _check_parsed(LT.parse_light_config(cfg))


def test_load_light_config_json(tmp_path):
    """a .json file of the same layout is read without PyYAML"""
    import json
    path = tmp_path / "relight.json"
    path.write_text(json.dumps(CONFIG_DICT))
    _check_parsed(LT.load_light_config(str(path)))


def test_cli_parser_takes_the_reference_command_line():
    """scripts/fipt/kitchen/render.sh:40-48"""
    from iris_amd.render_relight import build_parser
    a = build_parser().parse_args(["--experiment_name", "fipt_syn_kitchen", "--device", "0", "--ckpt", "last_1.ckpt", "--mode", "traj", "--dataset", "synthetic",
                                   "/data/indoor_synthetic/kitchen", "--emitter_path", "checkpoints/fipt_syn_kitchen/bake", "--output_path",
                                   "outputs/fipt_syn_kitchen/relight/video_relight_0", "--split", "test", "--ldr_img_dir", "Image", "--light_cfg",
                                   "configs/fipt/kitchen/relight_0.yaml", "--SPP", "256", "--spp", "16", "--crf_basis", "3"])
    assert a.mode == "traj" and a.light_cfg.endswith("relight_0.yaml") and a.SPP == 256 and a.spp == 16 and a.anti_aliasing == 1
    assert a.keep_lights == 0.0 and a.sphere_subdiv == 2 and a.indir_depth == 5
    b = build_parser().parse_args(["--experiment_name", "x", "--emitter_path", "e", "--light_cfg", "l.yaml", "--anti_aliasing", "2", "--scene", "abc", "--res_scale", "0.5",
                                   "--checkpoint_path", "ck", "--keep_lights", "0.25", "--sphere_subdiv", "3", "--batch_size", "4"])
    assert b.anti_aliasing == 2 and b.keep_lights == 0.25 and b.sphere_subdiv == 3
