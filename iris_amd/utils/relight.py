"""The relighting integrator (reference: render_relight.py, which hands the job to Mitsuba's `path` integrator with model/fipt_bsdf.py called per bounce).

The scene is the room composed with inserted lights (utils/lights.py); the surface light field is stale under new lighting, so no path ends in it: a path runs
all max_depth - 1 bounces unless it hits an emitter, an absorber or leaves the scene.  A bounce is shaped like trace_indirect's (utils/path_tracing.py):
draws -> iris_pt_bounce (emitter sampling + visibility ray + BRDF sampling + closest hit) [-> iris_pt_nee_spot on a side stream when there are spot lights]
-> the material network at the hits -> iris_relight_shade (everything after the network, one launch) -> compact_rows.

Differences from Mitsuba's integrator, all documented in DESIGN.md 5c-6: no Russian roulette (Mitsuba's rr_depth defaults to 5), the room's own lamps are
absorbers when switched off, the emitter pick is uniform over table rows, the spot falloff is Mitsuba 3's documented formula (unpinned).
"""
import torch

from .. import _lib as L
from ..model.emitter import AreaEmitter
from .path_tracing import Scene, _Pool, _bounce_draws, _mat_tensors, _side_stream, compact_rows, ray_intersect


class RelitScene:
    """What the relit integrator traces and shades against: the composed mesh's Scene, its AreaEmitter, the per-triangle surface classes, the constant
    materials and the spot tables, on `device`.  composed: the dict utils.lights.compose returns.  The native objects are the Scene's and the AreaEmitter's
    (L.Native each); the tables are plain tensors."""

    def __init__(self, composed, device=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.scene = Scene(composed["verts"], composed["faces"], device=self.device)
        self.emitter = AreaEmitter(composed["emitter"]).to(self.device)
        surf = torch.as_tensor(composed["surf"], dtype=torch.int32).reshape(-1)
        if surf.shape[0] != self.scene.n_triangles or len(self.emitter.is_emitter) != self.scene.n_triangles:
            raise L.IrisError("RelitScene: surf / is_emitter do not have one entry per triangle of the composed mesh")
        cmat = torch.as_tensor(composed["cmat"], dtype=torch.float32).reshape(-1, 5)
        if int(surf.max()) > cmat.shape[0] or int(surf.min()) < -1:
            raise L.IrisError("RelitScene: surf names a constant-material row that cmat does not have")
        self.has_classes = bool((surf != 0).any())                  # (none: the kernels skip the lookup)
        self.surf = surf.to(self.device).contiguous()
        self.cmat = cmat.to(self.device).contiguous()
        self.spots = torch.as_tensor(composed["spots"], dtype=torch.float32).reshape(-1, 10).to(self.device).contiguous()
        self.spot_intensity = torch.as_tensor(composed["spot_intensity"], dtype=torch.float32).reshape(-1, 3).to(self.device).contiguous()
        if self.spots.shape[0] != self.spot_intensity.shape[0]:
            raise L.IrisError("RelitScene: spots and spot_intensity differ in length")

    @property
    def n_spots(self):
        return int(self.spots.shape[0])

    @property
    def n_emitters(self):
        return self.emitter.n_emitters

    def surf_args(self):
        """(surf, n_surf, cmat, n_cmat) as the entry points take them"""
        if not self.has_classes:
            return None, 0, None, 0
        return L.ptr(self.surf), self.surf.shape[0], L.ptr(self.cmat) if self.cmat.shape[0] else None, self.cmat.shape[0]


@torch.no_grad()
def path_tracing_relit(relit, material_net, rays_o, rays_d, dx_du, dy_dv, spp, max_depth, uniforms=None, return_paths=False):
    """Path trace the relit scene: emitter sampling + BRDF sampling with power-2 MIS, next-event estimation for the spot lights, max_depth as Mitsuba counts it
    (1: emitters only, 2: direct light, ...; render_relight.py passes indir_depth + 2), no Russian roulette.

    rays_o, rays_d, dx_du, dy_dv: (B,3) float32 on the GPU; the pixel jitter is path_tracing_single's (offset 0.5: Mitsuba's box filter).
    uniforms: optional list of recorded draws in order: rand(2,B,spp), then per bounce rand(N), rand(N,2), rand(N), rand(N,2) (trace_indirect's four) and, only when
    the scene has spot lights, rand(N) for the spot pick; N = the paths alive at that bounce.
    Returns L (B,3): per pixel the path radiances added in the order s = 0, 1, ... in float32, times 1.0f / spp (the render stage's summation contract);
    return_paths: the (B*spp,3) path radiances instead.
    Runs without gradient: relighting trains nothing."""
    spp, max_depth = int(spp), int(max_depth)
    if spp < 1 or max_depth < 1:
        raise L.IrisError(f"path_tracing_relit: spp ({spp}) and max_depth ({max_depth}) must be at least 1")
    rays_o = L.require_gpu(rays_o, torch.float32, "rays_o").reshape(-1, 3)
    rays_d = L.require_gpu(rays_d, torch.float32, "rays_d").reshape(-1, 3)
    dx_du = L.require_gpu(dx_du, torch.float32, "dx_du").reshape(-1, 3)
    dy_dv = L.require_gpu(dy_dv, torch.float32, "dy_dv").reshape(-1, 3)
    B, dev = rays_o.shape[0], rays_o.device
    N0 = B * spp
    if N0 >= 1 << 31:
        raise L.IrisError(f"path_tracing_relit: B * spp = {N0} paths in one call, the limit is 2^31 - 1")
    own = uniforms is None
    u = None if own else list(uniforms)
    nxt = (lambda *shape: torch.rand(*shape, device=dev)) if own else (lambda *shape: L.require_gpu(u.pop(0), torch.float32, "uniforms").reshape(*shape))
    lib, scene, em = L.lib(), relit.scene, relit.emitter
    K, S = relit.n_emitters, relit.n_spots
    surf, n_surf, cmat, n_cmat = relit.surf_args()
    with torch.cuda.device(dev):
        L.mark()
        eh = em.handle(dev)
        radiance = em.radiance_on(dev)
        dudv = nxt(2, B, spp).contiguous()
        wi0 = torch.empty(N0, 3, device=dev)
        L.check(lib.iris_pt_jitter(L.ptr(rays_d), L.ptr(dx_du), L.ptr(dy_dv), L.ptr(dudv), B, spp, L.ptr(wi0), L.stream()))
        position, normal, _, tri0, _ = ray_intersect(scene, rays_o.repeat_interleave(spp, 0), wi0)
        e0 = torch.empty(N0, device=dev, dtype=torch.int32); valid = torch.empty(N0, device=dev, dtype=torch.bool)
        L.check(lib.iris_pt_primary_emit(eh, L.ptr(tri0), N0, L.ptr(e0), L.ptr(valid), L.stream()))
        if n_surf:                                                        # an absorber ends the path at once (class alone: no material rows yet)
            L.check(lib.iris_relight_surface(surf, n_surf, cmat, n_cmat, L.ptr(tri0), N0, None, None, None, L.ptr(valid), L.stream()))
        # the path radiance starts at radiance[e0] for a visible light; absorbers and misses start at 0
        ext = torch.cat([radiance, radiance.new_zeros(1, 3)])
        Lacc = ext[torch.where(e0 >= 0, e0.long(), torch.full_like(e0, K).long())].contiguous()
        L.mark("relit: jitter + primary hit")
        if max_depth > 1:
            iota = torch.arange(N0, device=dev, dtype=torch.int32)
            _, (position, normal, wo), _, (rows, tri_k) = compact_rows(valid, rows3=(position, normal), neg3=(wi0,), rowsi=(iota, tri0.to(torch.int32)))
            N = position.shape[0]
            throughput = torch.ones(N, 3, device=dev)
            mat = None
            if N:
                mat = _mat_tensors(material_net(position))
                if n_cmat:
                    mat = tuple(t.clone() for t in mat)                   # (written in place below: never the network's own tensors)
                    tri_k = tri_k.long()
                    L.check(lib.iris_relight_surface(surf, n_surf, cmat, n_cmat, L.ptr(tri_k), N, L.ptr(mat[0]), L.ptr(mat[1]), L.ptr(mat[2]), None, L.stream()))
                L.mark("relit: material network")
            for depth in range(max_depth - 1):
                N = position.shape[0]
                if N == 0:
                    break
                L.mark()
                a, r, m = mat
                s1, s2, s1b, s2b = _bounce_draws(nxt, own, N, dev)
                pick = nxt(N).contiguous() if S else None
                L.mark("relit: draws")
                pool = _Pool(34 * N + 320, dev)
                coef1 = pool.f(N, 3); e1 = pool.i32(N)
                wi = pool.f(N, 3); pdf = pool.f(N); w = pool.f(N, 3)
                pos_n = pool.f(N, 3); nrm_n = pool.f(N, 3)
                tri_n = pool.i64(N); hit = pool.u8(N)
                valid_next = pool.u8(N)
                coef_s = e_s = join = None
                if S:
                    # the spot stage is independent of the bounce's own two rays: on the side stream, as _path_tracing runs its emitter-sampling stage
                    coef_s = pool.f(N, 3); e_s = pool.i32(N)
                    main, side = torch.cuda.current_stream(dev), _side_stream(dev)
                    fork = torch.cuda.Event(); fork.record(main)
                    with torch.cuda.stream(side):
                        side.wait_event(fork)
                        L.mark()
                        L.check(lib.iris_pt_nee_spot(scene.handle, L.ptr(position), L.ptr(normal), L.ptr(wo), L.ptr(a), L.ptr(r), L.ptr(m), L.ptr(pick), L.ptr(relit.spots), S, N,
                                                     L.ptr(coef_s), L.ptr(e_s), L.stream()))
                        L.mark("relit: spot next-event estimation (side stream)")
                        join = torch.cuda.Event(); join.record(side)
                    for t_side in (position, normal, wo, a, r, m, pick, pool.buf):
                        t_side.record_stream(side)
                if K:
                    L.check(lib.iris_pt_bounce(scene.handle, eh, L.ptr(position), L.ptr(normal), L.ptr(wo), L.ptr(a), L.ptr(r), L.ptr(m), L.ptr(s1), L.ptr(s2), L.ptr(s1b), L.ptr(s2b), N,
                                               L.ptr(coef1), L.ptr(e1), 1e-12, 1e-12, 0.0, L.ptr(wi), L.ptr(pdf), L.ptr(w), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(tri_n), L.ptr(hit), L.stream()))
                else:                                                     # no area light at all: nothing to sample, the BRDF stage alone
                    L.check(lib.iris_pt_brdf_trace(scene.handle, L.ptr(position), L.ptr(normal), L.ptr(wo), L.ptr(a), L.ptr(r), L.ptr(m), L.ptr(s1b), L.ptr(s2b), N,
                                                   L.ptr(wi), L.ptr(pdf), L.ptr(w), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(tri_n), L.ptr(hit), 0, 0.0, L.stream()))
                L.mark("relit: emitter sample + visibility ray, BRDF sample + closest hit")
                mat_next = _mat_tensors(material_net(pos_n))
                if n_cmat:
                    mat_next = tuple(t.clone() for t in mat_next)
                L.mark("relit: material network")
                if join is not None:
                    torch.cuda.current_stream(dev).wait_event(join)
                L.check(lib.iris_relight_shade(eh, surf, n_surf, cmat, n_cmat, L.ptr(position), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(wi), L.ptr(tri_n), L.ptr(pdf), L.ptr(w),
                                               L.ptr(mat_next[0]), L.ptr(mat_next[1]), L.ptr(mat_next[2]), L.ptr(radiance) if K else None, L.ptr(e1) if K else None,
                                               L.ptr(coef1) if K else None, L.ptr(relit.spot_intensity) if S else None, L.ptr(e_s), L.ptr(coef_s), L.ptr(Lacc), L.ptr(rows),
                                               L.ptr(throughput), L.ptr(valid_next), N, 1e-12, L.stream()))
                L.mark("relit: shade (one launch)")
                if depth + 2 == max_depth:
                    break
                _, (position, normal, throughput, alb, wo), (rgh, mtl), (rows,) = compact_rows(valid_next, rows3=(pos_n, nrm_n, throughput, mat_next[0]), neg3=(wi,),
                                                                                              rows1=(mat_next[1], mat_next[2]), rowsi=(rows,))
                mat = (alb, rgh, mtl)
                L.mark("relit: survivors to the front (+ the count's read-back)")
        if return_paths:
            return Lacc
        # the mean over the samples of a pixel, sequential in s, times 1.0f / spp: iris_pt_accumulate_fwd's sum with the path radiances as its table
        iota = torch.arange(N0, device=dev, dtype=torch.int32)
        none = torch.full((N0,), -1, device=dev, dtype=torch.int32)
        Lout = torch.empty(B, 3, device=dev)
        L.check(lib.iris_pt_accumulate_fwd(L.ptr(Lacc), L.ptr(iota), L.ptr(none), None, None, None, None, None, B, spp, L.ptr(Lout), L.stream()))
        L.mark("relit: mean over the samples")
    return Lout
