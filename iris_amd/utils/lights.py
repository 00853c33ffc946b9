"""Light insertion for the relighting stage (reference: render_relight.py:66-114, utils/disco_ball.py, configs/*/*/relight_*.yaml): the reference's light
configuration, parsed from its dict layout, and the composition of the room mesh with the inserted shapes and lights.  Host side, numpy only.

What Mitsuba does with the configuration's shapes happens here explicitly:

* `to_world` is a list of translate / scale / rotate entries that render_relight.py chains on the growing transform (`t = t.translate(..)`, `t = t.scale(..)`):
  M = T1 T2 ..., a point is transformed by the LAST entry first.
* `rectangle` is the two triangles of [-1,1]^2 x {0} (normal +z); `sphere` is an icosphere INSCRIBED in the unit sphere (`sphere_subdiv` subdivisions, default 2:
  320 triangles).  Its area -- and so the power of an emissive sphere of given radiance -- is below the analytic sphere's by the factor ICOSPHERE_AREA_RATIO
  (0.761918, 0.928345, 0.981178, 0.995235 for 0..3 subdivisions).  The radiance is NOT rescaled.
* every triangle of the composed mesh has a surface class (`surf`): 0 network (the room, shaded by the material network; inserted emissive triangles are 0 too and
  end every path as emitters), -1 absorber (the room's own lamps with keep_lights = 0: a lamp switched off is black -- a deviation: FIPTBSDF gives these triangles
  BRDF 0 under eval and weight 1 under sample), g > 0 constant material row g - 1 of `cmat` (albedo rgb, roughness, metallic).
* constant materials: `diffuse` -> albedo = reflectance, roughness 1, metallic 0 (the BRDF of this package keeps its 0.04 specular term there, Mitsuba's is pure
  Lambert); `conductor` with material none -> albedo 1, metallic 1, roughness 0.02; `twosided` is unwrapped; a shape without bsdf is Mitsuba's default diffuse 0.5.
* `spot` entries (an addition: the reference only makes them through its disco ball) carry origin, target, cutoff_angle (degrees), optional beam_width, intensity.
"""
import math

import numpy as np

from .._lib import IrisError

IGNORED_KEYS = ("type", "PerspectiveCamera", "Integrator", "main_scene")
ICOSPHERE_AREA_RATIO = (0.761918, 0.928345, 0.981178, 0.995235)        # area of the inscribed icosphere / 4 pi, 0..3 subdivisions
DISCO_COLORS = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
DISCO_DEFAULTS = {"light_num": 20, "light_radius_rate": 0.1, "spot_intensity": 10, "spot_cutoff_angle": 20.0}      # utils/disco_ball.py:26-35
SPOT_ROW = 10          # origin xyz, axis xyz, cutoff, beam (radians), cos(cutoff), cos(beam): include/iris_hip.h iris_pt_nee_spot


# ------------------------------------------------------------------------------------------------------------------ transforms
def _translate(v):
    m = np.eye(4)
    m[:3, 3] = np.asarray(v, np.float64).reshape(3)
    return m


def _scale(v):
    v = np.asarray(v, np.float64).reshape(-1)
    return np.diag([*(v if v.size == 3 else np.repeat(v, 3)), 1.0])


def _rotate(axis, angle_deg):
    """Rodrigues rotation about `axis` by `angle_deg` degrees"""
    a = np.asarray(axis, np.float64).reshape(3)
    a = a / np.linalg.norm(a)
    t = math.radians(float(angle_deg))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)
    return m


def to_world_matrix(entries, key="to_world"):
    """M = T1 T2 ... in list order (render_relight.py:66-76)"""
    m = np.eye(4)
    for t in entries or ():
        kind = t.get("type")
        if kind == "translate":
            m = m @ _translate(t["value"])
        elif kind == "scale":
            m = m @ _scale(t["value"])
        elif kind == "rotate":
            m = m @ _rotate(t["axis"], t["angle"])
        else:
            raise IrisError(f"{key}: unknown transform {kind!r} (translate, scale, rotate)")
    return m


def transform_points(m, p):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    return p @ m[:3, :3].T + m[:3, 3]


# ------------------------------------------------------------------------------------------------------------------ tessellation
def rectangle_mesh():
    """the two triangles of [-1,1]^2 x {0}, normal +z"""
    return np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def icosphere(subdiv=2):
    """closed, outward-facing icosphere inscribed in the unit sphere: (vertices float64 (V,3), faces int32 (F,3)); F = 20 * 4^subdiv"""
    subdiv = int(subdiv)
    if subdiv < 0 or subdiv > 6:
        raise IrisError(f"icosphere: sphere_subdiv = {subdiv} (0 .. 6)")
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    verts = [np.asarray(p, np.float64) / math.sqrt(1.0 + g * g) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid, out = {}, []

        def midpoint(a, b):
            k = (a, b) if a < b else (b, a)
            if k not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[k] = len(verts) - 1
            return mid[k]
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    V = np.stack(verts)
    V = V / np.linalg.norm(V, axis=1, keepdims=True)
    F = np.asarray(faces, np.int32)
    n = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    flip = (n * V[F].mean(1)).sum(1) < 0
    F[flip] = F[flip][:, ::-1]
    return V, F


# ------------------------------------------------------------------------------------------------------------------ configuration
def _rgb(v, what):
    if isinstance(v, dict):
        if v.get("type", "rgb") != "rgb":
            raise IrisError(f"{what}: only rgb values are supported (got {v.get('type')!r})")
        v = v["value"]
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise IrisError(f"{what}: expected one or three values")
    return a


def material_row(bsdf, key):
    """(albedo r, g, b, roughness, metallic) of a constant material"""
    if bsdf is None:
        return np.array([0.5, 0.5, 0.5, 1.0, 0.0])                          # Mitsuba's default bsdf: diffuse, reflectance 0.5
    kind = bsdf.get("type")
    if kind == "twosided":
        inner = [v for k, v in bsdf.items() if isinstance(v, dict) and "type" in v]
        if len(inner) != 1:
            raise IrisError(f"{key}: twosided bsdf needs exactly one nested bsdf")
        return material_row(inner[0], key)
    if kind == "diffuse":
        return np.array([*_rgb(bsdf.get("reflectance", 0.5), f"{key}.bsdf.reflectance"), 1.0, 0.0])
    if kind == "conductor" and str(bsdf.get("material", "none")).lower() == "none":
        return np.array([1.0, 1.0, 1.0, 0.02, 1.0])
    raise IrisError(f"{key}: unsupported bsdf {kind!r}" + (f" (material {bsdf.get('material')!r})" if kind == "conductor" else "") + " (diffuse, conductor with material none, twosided)")


class Lights:
    """A parsed light configuration: `shapes` [{'name','type' (sphere | rectangle),'M' 4x4,'radiance' (3) or None,'material' (5) or None}],
    `spots` [{'name','origin','axis','cutoff','beam' (radians),'intensity' (3)}], `disco` the disco ball's parameter dict or None."""

    def __init__(self, shapes=(), spots=(), disco=None):
        self.shapes, self.spots, self.disco = list(shapes), list(spots), disco

    def at(self, timestep):
        """the lights of view `timestep`: the disco ball, when there is one, expanded at that time step (render_relight.py:271-272)"""
        if self.disco is None:
            return self
        shapes, spots = expand_disco_ball(self.disco, timestep)
        return Lights(self.shapes + shapes, self.spots + spots, None)


def _spot(name, origin, target, cutoff_deg, intensity, beam_deg=None):
    o, t = np.asarray(origin, np.float64).reshape(3), np.asarray(target, np.float64).reshape(3)
    axis = t - o
    n = np.linalg.norm(axis)
    if not n > 0:
        raise IrisError(f"{name}: spot origin and target coincide")
    cutoff = math.radians(float(cutoff_deg))
    beam = math.radians(float(beam_deg)) if beam_deg is not None else 0.75 * cutoff       # Mitsuba 3 `spot`: beam_width defaults to 3/4 of the cutoff
    if not (0.0 < beam < cutoff < math.pi):
        raise IrisError(f"{name}: spot needs 0 < beam_width < cutoff_angle < 180 degrees")
    return {"name": name, "origin": o, "axis": axis / n, "cutoff": cutoff, "beam": beam, "intensity": _rgb(intensity, f"{name}.intensity")}


def parse_light_config(cfg):
    """cfg: the reference's relight_*.yaml as a dict (yaml.safe_load; the files contain no interpolation) -> Lights"""
    if not isinstance(cfg, dict):
        raise IrisError("parse_light_config: expected a dict (the YAML document)")
    out = Lights()
    for key, item in cfg.items():
        if key in IGNORED_KEYS:
            continue
        if key == "disco_ball":
            missing = [k for k in ("position", "radius", "light_intensity", "T") if k not in item]
            if missing:
                raise IrisError(f"disco_ball: missing {missing}")
            out.disco = {**DISCO_DEFAULTS, **{k: item[k] for k in item}}
            continue
        if not isinstance(item, dict):
            raise IrisError(f"{key}: expected a shape (a dict with a type)")
        kind = item.get("type")
        if kind == "spot":
            out.spots.append(_spot(key, item["origin"], item["target"], item.get("cutoff_angle", 20.0), item.get("intensity", 1.0), item.get("beam_width")))
            continue
        if kind not in ("sphere", "rectangle"):
            raise IrisError(f"{key}: unsupported shape type {kind!r} (sphere, rectangle)")
        radiance = None
        em = item.get("emitter")
        if em is not None:
            if em.get("type") != "area":
                raise IrisError(f"{key}: unsupported emitter {em.get('type')!r} (area)")
            radiance = _rgb(em.get("radiance", 1.0), f"{key}.emitter.radiance")
        material = None if radiance is not None else material_row(item.get("bsdf"), key)     # (an emitter's own bsdf is never sampled: paths end there)
        if radiance is not None and item.get("bsdf") is not None:
            material_row(item["bsdf"], key)                                                  # still checked: an unknown BSDF raises and names the shape
        out.shapes.append({"name": key, "type": kind, "M": to_world_matrix(item.get("to_world"), key + ".to_world"), "radiance": radiance, "material": material})
    return out


def load_light_config(path):
    """the YAML file -> Lights (PyYAML behind a guarded import); a .json file of the same layout is read without it"""
    if str(path).lower().endswith(".json"):
        import json
        with open(path) as fh:
            return parse_light_config(json.load(fh))
    try:
        import yaml
    except ImportError as e:
        raise IrisError("reading a light configuration file needs PyYAML (pass a dict to parse_light_config instead)") from e
    with open(path) as fh:
        return parse_light_config(yaml.safe_load(fh))


def fibonacci_sphere(n, phase=0.0):
    """utils/disco_ball.py:10-24"""
    i = np.arange(int(n), dtype=np.float64)
    phi = (1.0 + np.sqrt(5.0)) / 2.0
    theta = 2.0 * np.pi * i / phi
    z = 1.0 - (2.0 * i + 1.0) / int(n)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(theta + phase), r * np.sin(theta + phase), z], -1)


def expand_disco_ball(params, timestep):
    """make_disco_ball (utils/disco_ball.py:26-108) at phase = timestep * 2 pi / T: (shapes, spots) in Lights' layout -- the grey centre sphere, light_num emissive
    spheres and light_num spots"""
    p = {**DISCO_DEFAULTS, **params}
    n, radius = int(p["light_num"]), float(p["radius"])
    position = np.asarray(p["position"], np.float64).reshape(3)
    phase = float(timestep) * (2.0 * np.pi / float(p["T"]))
    points = fibonacci_sphere(n, phase)
    light_radius = radius * float(p["light_radius_rate"])
    centres = points * (radius - light_radius * 0.6) + position
    shapes = [{"name": "disco_ball", "type": "sphere", "M": _translate(position) @ _scale([radius] * 3), "radiance": None,
               "material": np.array([0.2, 0.2, 0.2, 1.0, 0.0])}]
    spots = []
    for i in range(n):
        colour = DISCO_COLORS[i % len(DISCO_COLORS)]
        shapes.append({"name": f"light_{i}", "type": "sphere", "M": _translate(centres[i]) @ _scale([light_radius] * 3),
                       "radiance": colour * float(p["light_intensity"]), "material": None})
        o = points[i] * (radius + light_radius) + position
        spots.append(_spot(f"spot_{i}", o, o + points[i], p["spot_cutoff_angle"], colour * float(p["spot_intensity"])))
    return shapes, spots


# ------------------------------------------------------------------------------------------------------------------ composition
def _np(a, dtype):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype)


def spot_table(spots):
    """(S, SPOT_ROW) float32 rows and (S,3) float32 intensities"""
    rows = np.zeros((len(spots), SPOT_ROW), np.float32)
    inten = np.zeros((len(spots), 3), np.float32)
    for k, s in enumerate(spots):
        rows[k, 0:3], rows[k, 3:6] = s["origin"], s["axis"]
        rows[k, 6], rows[k, 7] = s["cutoff"], s["beam"]
        rows[k, 8], rows[k, 9] = math.cos(float(rows[k, 6])), math.cos(float(rows[k, 7]))      # of the float32 angles the kernel compares with
        inten[k] = s["intensity"]
    return rows, inten


def compose(verts, faces, emitter_state, lights, keep_lights=0.0, sphere_subdiv=2):
    """The room with the lights put in.  verts (V,3), faces (F,3); emitter_state: the room's emitter file (is_emitter, emitter_vertices, emitter_area,
    emitter_radiance) or None; lights: a Lights (the disco ball already expanded: Lights.at) or None.
    keep_lights = 0: the room's emitter triangles become absorbers and leave the table; s > 0: they stay emitters, their radiance times s.
    Returns a dict: 'verts' (V',3) float32, 'faces' (F',3) int32 (the room's triangles first, unchanged), 'surf' (F') int32, 'cmat' (G,5) float32,
    'emitter' {is_emitter (F') bool, emitter_vertices (K,3,3), emitter_area (K), emitter_radiance (K,3)} as torch tensors -- the reference's emitter file format,
    what AreaEmitter reads --, 'spots' (S,10) float32, 'spot_intensity' (S,3) float32."""
    import torch
    verts, faces = _np(verts, np.float32).reshape(-1, 3), _np(faces, np.int32).reshape(-1, 3)
    F0 = faces.shape[0]
    keep = float(keep_lights)
    if keep < 0:
        raise IrisError(f"compose: keep_lights = {keep} must not be negative")
    lights = lights if lights is not None else Lights()
    if lights.disco is not None:
        raise IrisError("compose: the disco ball is not expanded (Lights.at(timestep))")
    room_em = np.zeros(F0, bool)
    if emitter_state is not None:
        room_em = _np(emitter_state["is_emitter"], bool).reshape(-1).copy()
        if room_em.shape[0] != F0:
            raise IrisError(f"compose: the emitter file is for {room_em.shape[0]} triangles, the mesh has {F0}")
    K0 = int(room_em.sum())
    all_v, all_f, surf, cmat = [verts], [faces], [np.zeros(F0, np.int32)], []
    is_em = [room_em.copy() if keep > 0 else np.zeros(F0, bool)]
    em_v, em_a, em_r = [], [], []
    if keep > 0 and K0:
        tri = verts[faces[room_em]]
        ev = emitter_state.get("emitter_vertices")
        ev = _np(ev, np.float32).reshape(-1, 3, 3) if ev is not None else tri
        if ev.shape[0] != K0:
            ev = tri
        ea = _np(emitter_state["emitter_area"], np.float32).reshape(-1)
        er = _np(emitter_state["emitter_radiance"], np.float32).reshape(-1, 3)[:K0]           # (rows are indexed by emitter ordinal; a file may carry more)
        if ea.shape[0] != K0 or er.shape[0] != K0:
            raise IrisError("compose: emitter_area / emitter_radiance do not match is_emitter")
        em_v.append(ev); em_a.append(ea); em_r.append(er * np.float32(keep))
    elif K0:
        surf[0][room_em] = -1
    nv = verts.shape[0]
    for sh in lights.shapes:
        lv, lf = rectangle_mesh() if sh["type"] == "rectangle" else icosphere(sphere_subdiv)
        wv = transform_points(sh["M"], lv).astype(np.float32)
        if np.linalg.det(sh["M"][:3, :3]) < 0:
            lf = lf[:, ::-1]                                               # a mirroring transform: keep the faces outward
        all_v.append(wv); all_f.append((lf + nv).astype(np.int32)); nv += wv.shape[0]
        n = lf.shape[0]
        if sh["radiance"] is not None:
            tri = wv[lf]
            area = 0.5 * np.linalg.norm(np.cross(tri[:, 1].astype(np.float64) - tri[:, 0], tri[:, 2].astype(np.float64) - tri[:, 0]), axis=1)
            em_v.append(tri); em_a.append(area.astype(np.float32)); em_r.append(np.repeat(np.asarray(sh["radiance"], np.float32)[None], n, 0))
            is_em.append(np.ones(n, bool)); surf.append(np.zeros(n, np.int32))
        else:
            cmat.append(np.asarray(sh["material"], np.float32))
            is_em.append(np.zeros(n, bool)); surf.append(np.full(n, len(cmat), np.int32))
    spots, inten = spot_table(lights.spots)
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)      # noqa: E731
    emitter = {"is_emitter": torch.from_numpy(np.concatenate(is_em)),
               "emitter_vertices": torch.from_numpy(cat(em_v, (0, 3, 3), np.float32)),
               "emitter_area": torch.from_numpy(cat(em_a, (0,), np.float32)),
               "emitter_radiance": torch.from_numpy(cat(em_r, (0, 3), np.float32))}
    return {"verts": np.concatenate(all_v).astype(np.float32), "faces": np.concatenate(all_f).astype(np.int32), "surf": np.concatenate(surf),
            "cmat": np.stack(cmat).astype(np.float32) if cmat else np.zeros((0, 5), np.float32), "emitter": emitter, "spots": spots, "spot_intensity": inten}
