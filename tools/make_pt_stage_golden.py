#!/usr/bin/env python3
"""Generate tests/golden/pt_stage_ref.npz: the reference's own path_tracing_single (spp = 1, so L[b] is one path's total) and trace_indirect (depth 1 and 2) run
UNMODIFIED in float64 on the open scene of tests/pt_stage_ref64.py, with what went in and came out of every stage boundary recorded per path.

Runs only where a checkout of the reference is at hand: `python tools/make_pt_stage_golden.py <reference checkout>` (or IRIS_REFERENCE); the mechanism is tools/make_goldens.py's: stub modules for the absent third-party packages, CWD = the
reference, `StubMaterial` behind the reference's BaseBRDF.  torch's default dtype is float64, so the reference's draws, samplers, formulas and accumulators are all
double.  The one thing the reference cannot do here is intersect rays: utils.path_tracing.ray_intersect is replaced by the exact float64 closest hit of
tests/hit_ref64.py (exact_hits over all triangles).  The recorders wrap the reference's objects from outside; none of its lines is changed or copied.

The file holds data only: the rays, per stage boundary the reference's float64 sampled directions, pdfs, weights, hit positions, normals and triangle ids and the
material rows, the radiance table, and per path L.  tests/test_pt_stage_ref64_cpu.py feeds them to the restatement's float64 stage formulas.
"""
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IRIS_REFERENCE", ""))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    assert os.path.isdir(os.path.join(REF, "utils")), "usage: make_pt_stage_golden.py <checkout of the reference>"
    from make_goldens import _stub_modules
    import hit_ref64 as H
    import pt_stage_ref64 as P
    from stub_material import StubMaterial
    _stub_modules()
    import torch
    sys.path.insert(0, REF)
    os.chdir(REF)
    torch.set_default_dtype(torch.float64)
    import utils.path_tracing as rpt
    from model.brdf import BaseBRDF
    from model.emitter import SLFEmitterLearn
    from model.slf import VoxelSLF

    sc = P.scene("open")
    g, em, s = sc["geom"], sc["em"], sc["slf"]
    rng = np.random.default_rng(11)
    radiance = rng.uniform(0.5, 20.0, (em["K"], 3)).astype(np.float32)
    tmp = tempfile.mkdtemp()
    ep, sp = os.path.join(tmp, "emitter.pth"), os.path.join(tmp, "vslf.npz")
    slf = VoxelSLF(torch.from_numpy(np.array(s["mask"])), s["vmin"], s["vmax"])
    slf.radiance[:] = torch.from_numpy(s["radiance"].astype(np.float64))
    torch.save({"mask": torch.from_numpy(np.array(s["mask"])), "voxel_min": s["vmin"], "voxel_max": s["vmax"], "weight": slf.state_dict()}, sp)
    torch.save({"is_emitter": torch.from_numpy(np.array(sc["is_emitter"])), "emitter_vertices": torch.from_numpy(em["verts"].astype(np.float64)),
                "emitter_area": torch.from_numpy(em["area"].astype(np.float64)), "emitter_normal": torch.zeros(em["K"], 3),
                "emitter_radiance": torch.from_numpy(radiance)}, ep)
    emitter = SLFEmitterLearn(ep, sp)
    emitter.radiance.data = emitter.radiance.data.double()         # (the constructor makes the parameter a FloatTensor; the same values, in the run's dtype)

    events = []

    def rec(kind, **arrays):
        events.append((kind, {k: (v.detach().numpy().copy() if hasattr(v, "detach") else np.asarray(v)) for k, v in arrays.items()}))

    def ray_intersect(scene, xs, ds):
        o, d = xs.detach().numpy(), ds.detach().numpy()
        t, b, _ = H.exact_hits(sc["verts"], sc["faces"], o, d, g)
        with np.errstate(all="ignore"):
            ex = (b.min(0) >= 0) & (t >= 0) & np.isfinite(t)
        te = np.where(ex, t, np.inf)
        k = te.argmin(1)
        ar = np.arange(len(o))
        hit = ex[ar, k]
        bk = b[:, ar, k]
        p = np.where(hit[:, None], (bk.T[:, :, None] * g.Pabs[k]).sum(1), 0.0)
        n = g.N[k] / g.Nlen[k][:, None]
        n = np.where(((n * -d).sum(-1) < 0)[:, None], -n, n)
        n = np.where(hit[:, None], n, 0.0)
        idx = np.where(hit, k, -1)
        rec("hit", position=p, normal=n, idx=idx)
        return torch.from_numpy(p), torch.from_numpy(n), torch.from_numpy(np.where(hit[:, None], bk[1:].T, 0.0)), torch.from_numpy(idx), torch.from_numpy(hit)
    rpt.ray_intersect = ray_intersect

    class RefStub(BaseBRDF):                # the reference's NGPBRDF is a BaseBRDF with a forward(position) (model/brdf.py:213-260)
        def forward(self, x):
            m = {k: v.double() for k, v in StubMaterial()(x).items()}
            rec("material", albedo=m["albedo"], roughness=m["roughness"], metallic=m["metallic"])
            return m

        def sample_brdf(self, *a):
            out = super().sample_brdf(*a)
            rec("sample_brdf", wi=out[0], pdf=out[1], weight=out[2])
            return out
    material = RefStub()
    ref_sample_emitter = emitter.sample_emitter

    def sample_emitter(s1, s2, position):
        out = ref_sample_emitter(s1, s2, position)
        rec("sample_emitter", position=position, wi=out[0], pdf=out[1], tri=out[2])
        return out
    emitter.sample_emitter = sample_emitter

    # rays: from above towards the floor, the occluder and the emitters; and, half of them, from low at the sides to the floor under the occluder, where a sampled
    # direction meets a surface again (elsewhere in this open scene most of them leave it)
    B = 800
    ro = np.stack([rng.uniform(-3.5, 3.5, B), rng.uniform(-3.5, 3.5, B), rng.uniform(1.2, 3.4, B)], -1)
    tg = np.stack([rng.uniform(-3.5, 3.5, B), rng.uniform(-3.5, 3.5, B), np.where(rng.random(B) < 0.8, 0.0, 3.0)], -1)
    a = rng.uniform(0, 2 * np.pi, B // 2)
    ro[::2] = np.stack([-0.5 + 3.0 * np.cos(a), 3.0 * np.sin(a), rng.uniform(0.2, 0.9, B // 2)], -1)
    tg[::2] = np.stack([rng.uniform(-1.4, 0.4, B // 2), rng.uniform(-0.9, 0.9, B // 2), np.zeros(B // 2)], -1)
    rd = tg - ro
    rd /= np.linalg.norm(rd, axis=-1, keepdims=True)
    T = torch.from_numpy
    out = {"rays_o": ro, "rays_d": rd, "radiance": radiance}

    def flush(prefix):
        for i, (kind, arrays) in enumerate(events):
            for k, v in arrays.items():
                out[f"{prefix}/{i:02d}/{kind}/{k}"] = v
        events.clear()

    with torch.no_grad():
        torch.manual_seed(21)
        zero = torch.zeros(B, 3)
        L = rpt.path_tracing_single(None, emitter, material, T(ro), T(rd), zero, zero, 1)
        out["single/L"] = L.numpy()
        flush("single")
        pos, nrm, _, idx, valid = ray_intersect(None, T(ro), T(rd))
        events.clear()
        keep = (valid & ~T(np.array(sc["is_emitter"]))[idx.clamp_min(0)]).numpy()
        start = np.nonzero(keep)[0]
        for depth, rows in ((1, start[: len(start) // 2]), (2, start[len(start) // 2:])):
            torch.manual_seed(30 + depth)
            Li = rpt.trace_indirect(None, emitter, material, pos[rows], -T(rd)[rows], nrm[rows], depth)
            out[f"indirect{depth}/L"] = Li.numpy()
            out[f"indirect{depth}/position"], out[f"indirect{depth}/wo"], out[f"indirect{depth}/normal"] = pos[rows].numpy(), -rd[rows], nrm[rows].numpy()
            flush(f"indirect{depth}")
    path = os.path.join(REPO, "tests", "golden", "pt_stage_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays; single: {B} paths, L mean {float(L.mean()):.4g}; "
          f"indirect: {len(start) // 2} + {len(start) - len(start) // 2} paths")


if __name__ == "__main__":
    main()
