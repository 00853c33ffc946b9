#!/usr/bin/env python3
"""Measurements for the relighting stage on the bench room (1.0 M triangles, its own lamps switched off, one inserted rectangle light; material =
the closed-form GPU stand-in, --material ngp for the reference's NGPBRDF with random parameters): one 1080p view, spp 8, max_depth 7, HIP events, ONE process.
  view    path_tracing_relit for the whole view, median of --repeats, with a stage table from L.StageTimer: summed over the bounces, and per bounce
  shade   iris_relight_shade against the three launches it replaces (iris_pt_apply -> iris_pt_brdf_finish(trace_roughness = +inf) -> iris_pt_apply) on the SAME
          inputs: the arrays of a first bounce of the view; a sample is --batch calls between two events, both are sampled --repeats times, alternating, and the
          spread of each is reported
Writes profiles/relight_bench.json and prints it as one JSON line."""
import argparse, json, math, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def per_bounce(tm):
    """the stage table of a StageTimer cut at the integrator's bounces: [{stage: ms}, ...], entry 0 = before the first bounce; a bounce begins at a mark without a name
    on the stream of the first mark (the side stream's stages are counted with the bounce they are issued in)"""
    torch.cuda.synchronize()
    out, last, main_sid = [{}], {}, tm.events[0][0]
    for k, (sid, name, ev) in enumerate(tm.events):
        if name is None and sid == main_sid and k > 0:
            out.append({})
        if sid in last and name is not None:
            out[-1][name] = round(out[-1].get(name, 0.0) + last[sid].elapsed_time(ev), 3)
        last[sid] = ev
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=8); ap.add_argument("--tris", type=int, default=1_000_000); ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--max_depth", type=int, default=7); ap.add_argument("--height", type=int, default=1080); ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--material", choices=["ngp", "stub"], default="stub")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "relight_bench.json"))
    args = ap.parse_args()
    import numpy as np
    from iris_amd import _lib as L
    from iris_amd.utils import lights as LT
    from iris_amd.utils.dataset import real_ldr
    from iris_amd.utils.relight import RelitScene, path_tracing_relit
    from tools import synth
    from tools.bench_pt_single import GpuStub, ngp_material
    dev = torch.device("cuda:0")
    room = synth.room(1, args.tris)
    emi = synth.emitters_for(room["vertices"], room["faces"], room["is_emitter"])
    state = {k: torch.from_numpy(np.ascontiguousarray(emi[k])) for k in ("is_emitter", "emitter_vertices", "emitter_area", "emitter_radiance")}
    lights = LT.parse_light_config({"panel": {"type": "rectangle", "to_world": [{"type": "translate", "value": [2.0, 1.5, 2.3]}, {"type": "scale", "value": [0.4, 0.4, 0.4]},
                                                                                {"type": "rotate", "axis": [1, 0, 0], "angle": 180}],
                                              "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [20, 20, 20]}}}})
    relit = RelitScene(LT.compose(room["vertices"], room["faces"], state, lights), dev)
    H, W, spp = args.height, args.width, args.spp
    K, c2w = synth.camera(H, W, 0)
    rays = real_ldr.to_world(real_ldr.get_direction(K, (H, W)), c2w, True, K, device=dev)
    net = ngp_material(synth.slf_for(room["vertices"], room["faces"], 256), dev).to(dev) if args.material == "ngp" else GpuStub()
    run = lambda **kw: path_tracing_relit(relit, net, *rays, spp, args.max_depth, **kw)      # noqa: E731
    run(); torch.cuda.synchronize()
    view = sorted(event_ms(run) for _ in range(args.repeats))
    with L.StageTimer() as tm:
        run()
    stages = {k: round(v, 3) for k, v in sorted(tm.ms().items(), key=lambda kv: -kv[1])}
    bounces = per_bounce(tm)
    # the shade stage against the sequence it replaces, on a first bounce's arrays: the view's pixel-centre rays, spp paths each, one bounce of the integrator's calls
    from iris_amd.utils import path_tracing as PT
    lib, eh, rad = L.lib(), relit.emitter.handle(dev), relit.emitter.radiance_on(dev)
    wi0 = torch.nn.functional.normalize(rays[1], dim=-1).repeat_interleave(spp, 0).contiguous()
    pos, nrm, _, tri0, ok = PT.ray_intersect(relit.scene, rays[0].repeat_interleave(spp, 0).contiguous(), wi0)
    ok = ok & (relit.surf[tri0.clamp_min(0)] >= 0)
    pos, nrm, wo = pos[ok].contiguous(), nrm[ok].contiguous(), (-wi0[ok]).contiguous()
    N = pos.shape[0]
    am, rm, mm = PT._mat_tensors(net(pos))
    f3 = lambda: torch.empty(N, 3, device=dev)                    # noqa: E731
    a = {"position": pos, "coef1": f3(), "wi": f3(), "w": f3(), "pos_n": f3(), "nrm_n": f3(), "e1": torch.empty(N, device=dev, dtype=torch.int32), "pdf": torch.empty(N, device=dev),
         "tri_n": torch.empty(N, device=dev, dtype=torch.int64), "rows": torch.arange(N, device=dev, dtype=torch.int32), "L": torch.zeros(N, 3, device=dev),
         "throughput": torch.ones(N, 3, device=dev)}
    hit = torch.empty(N, device=dev, dtype=torch.bool)
    s1, s2, s1b, s2b = PT._bounce_draws(None, True, N, dev)
    L.check(lib.iris_pt_bounce(relit.scene.handle, eh, L.ptr(pos), L.ptr(nrm), L.ptr(wo), L.ptr(am), L.ptr(rm), L.ptr(mm), L.ptr(s1), L.ptr(s2), L.ptr(s1b), L.ptr(s2b), N,
                               L.ptr(a["coef1"]), L.ptr(a["e1"]), 1e-12, 1e-12, 0.0, L.ptr(a["wi"]), L.ptr(a["pdf"]), L.ptr(a["w"]), L.ptr(a["pos_n"]), L.ptr(a["nrm_n"]), L.ptr(a["tri_n"]),
                               L.ptr(hit), L.stream()))
    a["mat_next"] = PT._mat_tensors(net(a["pos_n"]))
    an, rn, mn = (t.clone() for t in a["mat_next"])
    coef2, const2 = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
    e2, vs, vf = torch.empty(N, device=dev, dtype=torch.int32), torch.empty(N, device=dev, dtype=torch.bool), torch.empty(N, device=dev, dtype=torch.bool)
    Ls, ts, Lf, tf = a["L"].clone(), a["throughput"].clone(), a["L"].clone(), a["throughput"].clone()
    P = L.ptr

    def sequence():
        L.check(lib.iris_pt_apply(P(Ls), P(a["rows"]), P(ts), P(rad), P(a["e1"]), P(a["coef1"]), None, None, N, 1, L.stream()))
        L.check(lib.iris_pt_brdf_finish(eh, None, P(a["position"]), P(a["pos_n"]), P(a["nrm_n"]), P(a["wi"]), P(a["tri_n"]), P(rn), P(a["pdf"]), P(a["w"]), N, P(coef2), P(const2), P(e2),
                                        P(vs), math.inf, 1e-12, L.stream()))
        L.check(lib.iris_pt_apply(P(Ls), P(a["rows"]), P(ts), P(rad), P(e2), P(coef2), P(const2), P(a["w"]), N, 1, L.stream()))

    def fused():
        L.check(lib.iris_relight_shade(eh, None, 0, None, 0, P(a["position"]), P(a["pos_n"]), P(a["nrm_n"]), P(a["wi"]), P(a["tri_n"]), P(a["pdf"]), P(a["w"]), P(an), P(rn), P(mn),
                                       P(rad), P(a["e1"]), P(a["coef1"]), None, None, None, P(Lf), P(a["rows"]), P(tf), P(vf), N, 1e-12, L.stream()))
    sequence(); fused(); torch.cuda.synchronize()
    same = bool(torch.equal(Ls, Lf) and torch.equal(ts, tf) and torch.equal(vs, vf))         # (after one application each, from the same state)
    # a sample is --batch calls back to back between two events (L and throughput keep changing: the kernels do not look at the values), divided by the batch
    many = lambda fn: (lambda: [fn() for _ in range(args.batch)])          # noqa: E731
    seq_ms, fus_ms = [], []
    for _ in range(args.repeats):
        seq_ms.append(event_ms(many(sequence)) / args.batch); fus_ms.append(event_ms(many(fused)) / args.batch)
    seq_ms.sort(); fus_ms.sort()
    med = lambda v: v[len(v) // 2]           # noqa: E731
    row = {"case": f"one {W} x {H} view of the bench room ({args.tris} triangles, lamps off) with one rectangle light, spp {spp}, max_depth {args.max_depth}: {H * W * spp} primary paths; "
                   f"material {args.material}",
           "view": {"ms": round(med(view), 2), "all_ms": [round(x, 2) for x in view], "Mpaths_per_s": round(H * W * spp / med(view) / 1e3, 1), "stages_ms_summed_over_bounces": stages,
                    "stages_ms_per_bounce": bounces},
           "shade_stage_first_bounce": {"paths": N, "calls_per_sample": args.batch, "fused_ms": round(med(fus_ms), 3), "fused_all_ms": [round(x, 3) for x in fus_ms], "sequence_ms": round(med(seq_ms), 3),
                                        "sequence_all_ms": [round(x, 3) for x in seq_ms], "sequence_over_fused": round(med(seq_ms) / med(fus_ms), 3),
                                        "spread_ms": round(max(fus_ms[-1] - fus_ms[0], seq_ms[-1] - seq_ms[0]), 3), "same_bits": same}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(row, fh, indent=1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
