// Closest point on the mesh: the BVH the rays traverse, walked by a DISTANCE query.  One point per lane.
//
//   triangle    Ericson, "Real-Time Collision Detection" 5.1.5: the six dot products d1..d6 classify the point into a vertex, an edge or the interior region.
//               The edge vectors and the point's offsets from the three vertices are float32 differences, and so are the weights, the distance vector and
//               dist2.  The dot products, their three differences of products and the one division are FLOAT64: in float32 the differences of products lose a
//               sliver's weights -- on a triangle 100 long and 1 high the distance was off by 390 x 2^-24 x the scene's largest coordinate, against the 64 the
//               tests allow; with float64 products (exact for float32 factors) the same points are off by 0.06.  (b1, b2) are the weights of vertices 1 and
//               2 as in iris_intersect, clamped so that b1, b2 >= 0 and b1 + b2 <= 1 hold as real numbers.
//   distance    d = (p0 - x) + b1 (p1 - p0) + b2 (p2 - p0), dist2 = (dx dx + dy dy) + dz dz.
//   winner      the lexicographic minimum of (dist2 as computed, original face index): a face met through several presplit references is evaluated from the same
//               record bits every time and gives one answer.  A triangle whose float32 cross product (p1 - p0) x (p2 - p0) is exactly zero is skipped (no ray
//               can hit it either), and one whose dist2 is not finite (overflow, NaN vertices) never wins.
//   nodes       octant 0 of the Q8 node table: its "near" bytes are the lower planes and its "far" bytes the upper ones; the order of the children there is
//               irrelevant, the four squared box distances are sorted here.
//   prune       an entry is dropped when its box distance exceeds best * kClosestSlack.  CHOSEN: the best distance scaled UP (by 16 ulps), not a bound rounded
//               down.  What it has to absorb is the float32 rounding of the three squares and two sums of either side (a few ulps, relative).  The absolute
//               part -- a plane decoded with one rounding, half an ulp of the coordinate -- is absorbed by the builder, which pads every box by 2e-5 of the
//               scene's largest coordinate or extent (330 ulps) before the planes are rounded outward to 8 bits.  A NaN bound is never pruned.
//   stack       two per-lane stacks of iris_trace.h side by side, node / leaf references and their box distances, moved together.  A visit replaces the current
//               reference by at most three pushed ones, so along a path of `depth` nodes at most 3 * depth entries wait; iris_scene_create refuses every tree with
//               3 * depth + 4 > kStackCapacity: every scene that exists fits, and the capacity is the rays' (no second constant).  2 x 24 entries x 256 lanes
//               = 48 KiB of LDS per workgroup (three workgroups per compute unit); the first descent starts with best = inf and pushes every sibling, so trees
//               deeper than eight levels reach the spill part (scratch, 2 x 72 words per lane) on most queries.
#pragma once
#include "iris_trace.h"

namespace iris {

constexpr float kClosestSlack = 1.0f + 16.0f * 1.1920929e-07f;      // 1 + 16 * 2^-23

struct Closest {
    float d2, b1, b2;
    int slot;       // index into SceneDev::tris, -1 = none
    int id;         // original face index
};
typedef Stack<kStackLds> ClosestStack;

__device__ __forceinline__ void closest_tri_eval(const iris_f4v X, const iris_f4v Y, const iris_f4v Z, int slot, f3 p, Closest& c) {
    const int id = __float_as_int(Z.w);
    const f3 a = mk3(X.x, Y.x, Z.x), ab = sub3(mk3(X.y, Y.y, Z.y), a), ac = sub3(mk3(X.z, Y.z, Z.z), a);
    const f3 n = t_cross(ab, ac);
    const bool has_area = !(n.x == 0.f && n.y == 0.f && n.z == 0.f);
    const f3 ap = sub3(p, a), bp = sub3(p, mk3(X.y, Y.y, Z.y)), cp = sub3(p, mk3(X.z, Y.z, Z.z));
    // (float64 from here to the two weights: see the header)
#define IRIS_DOT64(A, B) fma((double)(A).z, (double)(B).z, fma((double)(A).y, (double)(B).y, (double)(A).x * (double)(B).x))
    const double d1 = IRIS_DOT64(ab, ap), d2 = IRIS_DOT64(ac, ap), d3 = IRIS_DOT64(ab, bp), d4 = IRIS_DOT64(ac, bp), d5 = IRIS_DOT64(ab, cp), d6 = IRIS_DOT64(ac, cp);
#undef IRIS_DOT64
    const double va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
    const double e = d4 - d3, g = d5 - d6;
    // the regions as selects, the one Ericson tests LAST first: a later line overrides an earlier one.  Every region's weights are one or two numerators over
    // ONE denominator, so the numerators and the denominator are selected and there is a single division.
    double nv = vb, nw = vc, den = (va + vb) + vc;                                               // interior: v = vb / den, w = vc / den
    int kind = 0;                                                                                // 0: (nv, nw) / den;  1: w = nw / den, v = 1 - w;  2: constants
    if (va <= 0.0 && e >= 0.0 && g >= 0.0) { nw = e; den = e + g; kind = 1; }                    // edge p1 p2
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { nv = 0.0; nw = d2; den = d2 - d6; kind = 0; }     // edge p0 p2
    if (d6 >= 0.0 && d5 <= d6) { nv = 0.0; nw = 1.0; den = 1.0; kind = 2; }                      // vertex p2
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { nv = d1; nw = 0.0; den = d1 - d3; kind = 0; }     // edge p0 p1
    if (d3 >= 0.0 && d4 <= d3) { nv = 1.0; nw = 0.0; den = 1.0; kind = 2; }                      // vertex p1
    if (d1 <= 0.0 && d2 <= 0.0) { nv = 0.0; nw = 0.0; den = 1.0; kind = 2; }                     // vertex p0
    const double rden = 1.0 / den;
    const double w64 = nw * rden, v64 = kind == 1 ? 1.0 - w64 : nv * rden;
    float v = (float)v64, w = (float)w64;
    // whatever the rounding of a sliver did to (v, w): a point OF the triangle (fmaxf drops a NaN), so dist2 is a distance that exists
    v = fminf(fmaxf(v, 0.f), 1.f);
    w = fminf(fmaxf(w, 0.f), 1.0f - v);
    if ((double)v + (double)w > 1.0) w = __uint_as_float(__float_as_uint(w) - 1u);               // (1 - v was rounded up: w > 0 here, one ulp less is below 1 - v)
    const float dx = fmaf(w, ac.x, fmaf(v, ab.x, -ap.x)), dy = fmaf(w, ac.y, fmaf(v, ab.y, -ap.y)), dz = fmaf(w, ac.z, fmaf(v, ab.z, -ap.z));
    const float dd = (dx * dx + dy * dy) + dz * dz;
    // (+inf can only tie with the initial c.d2, whose c.id = INT_MIN no index is smaller than; a NaN fails both comparisons)
    const bool closer = (int)(dd < c.d2) | ((int)(dd == c.d2) & (int)(id < c.id));
    if ((int)has_area & (int)closer) { c.d2 = dd; c.b1 = v; c.b2 = w; c.slot = slot; c.id = id; }
}

// the next waiting reference whose box can still hold a closer triangle, kEmptyRef when none is left
__device__ __forceinline__ uint32_t closest_pop(ClosestStack& refs, ClosestStack& bounds, float best_d2) {
    const float limit = best_d2 * kClosestSlack;
    while (refs.sp > 0) {
        const uint32_t r = refs.pop();
        const float b = __uint_as_float(bounds.pop());
        if (!(b > limit)) return r;
    }
    return kEmptyRef;
}

// One node visit: the four children's squared box distances, the nearest next, the others pushed farthest first.
__device__ __forceinline__ uint32_t closest_node(const SceneDev& sc, f3 p, uint32_t cur, ClosestStack& refs, ClosestStack& bounds, float best_d2) {
    glb_u4v* n = (glb_u4v*)(reinterpret_cast<const char*>(sc.nodes) + (size_t)node_offset(cur));          // octant 0: near = lower planes, far = upper planes
    const iris_u4v hd = n[0], q1 = n[1], q2 = n[2], rf = n[3];
    const float ox = __uint_as_float(hd.x), oy = __uint_as_float(hd.y), oz = __uint_as_float(hd.z);
    // the node stores 2^(e + 24) per axis (node_step feeds the bytes in as q * 2^-24); plane = origin + q * 2^e, one rounding
    const float sx = __uint_as_float(hd.w) * 0x1p-24f, sy = __uint_as_float(q1.x) * 0x1p-24f, sz = __uint_as_float(q1.y) * 0x1p-24f;
    const uint32_t lxq = q1.z, lyq = q1.w, lzq = q2.x, hxq = q2.y, hyq = q2.z, hzq = q2.w;
    float k0, k1, k2, k3;
#define IRIS_QB(W, C) ((float)(((W) >> (8 * (C))) & 0xffu))
#define IRIS_BOXD2(K, C)                                                                                           \
    {                                                                                                              \
        const float ex = fmaxf(fmaxf(fmaf(IRIS_QB(lxq, C), sx, ox) - p.x, p.x - fmaf(IRIS_QB(hxq, C), sx, ox)), 0.f); \
        const float ey = fmaxf(fmaxf(fmaf(IRIS_QB(lyq, C), sy, oy) - p.y, p.y - fmaf(IRIS_QB(hyq, C), sy, oy)), 0.f); \
        const float ez = fmaxf(fmaxf(fmaf(IRIS_QB(lzq, C), sz, oz) - p.z, p.z - fmaf(IRIS_QB(hzq, C), sz, oz)), 0.f); \
        K = (ex * ex + ey * ey) + ez * ez;                                                                         \
    }
    IRIS_BOXD2(k0, 0) IRIS_BOXD2(k1, 1) IRIS_BOXD2(k2, 2) IRIS_BOXD2(k3, 3)
#undef IRIS_BOXD2
#undef IRIS_QB
    uint32_t r0 = rf.x, r1 = rf.y, r2 = rf.z, r3 = rf.w;      // (an unused slot: the inverted box, some positive distance, and the degenerate record no query accepts)
    IRIS_CE(k0, r0, k1, r1) IRIS_CE(k2, r2, k3, r3) IRIS_CE(k0, r0, k2, r2) IRIS_CE(k1, r1, k3, r3) IRIS_CE(k1, r1, k2, r2)
    const float limit = best_d2 * kClosestSlack;
    if (k0 > limit) return closest_pop(refs, bounds, best_d2);
    if (!(k3 > limit)) { refs.push(r3); bounds.push(__float_as_uint(k3)); }
    if (!(k2 > limit)) { refs.push(r2); bounds.push(__float_as_uint(k2)); }
    if (!(k1 > limit)) { refs.push(r1); bounds.push(__float_as_uint(k1)); }
    return r0;
}

// s_refs, s_bounds: &array[threadIdx.x] of two kStackLds * kBlock word arrays in LDS
__device__ __forceinline__ Closest closest_query(const SceneDev& sc, f3 p, uint32_t* s_refs, uint32_t* s_bounds) {
    Closest c;
    c.d2 = INFINITY; c.b1 = 0.f; c.b2 = 0.f; c.slot = -1; c.id = (int)0x80000000;
    ClosestStack refs, bounds;
    refs.lds = (lds_u32*)s_refs; refs.ovf = nullptr; refs.sp = 0; refs.tid = threadIdx.x;
    bounds.lds = (lds_u32*)s_bounds; bounds.ovf = nullptr; bounds.sp = 0; bounds.tid = threadIdx.x;
    const bool finite = fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY;      // (a NaN fails)
    uint32_t cur = finite && sc.n_nodes > 0 ? 0u : kEmptyRef;
    for (;;) {
        const bool at_node = cur != kEmptyRef && !(cur & kLeafBit);
        const bool at_leaf = cur != kEmptyRef && (cur & kLeafBit);
        if (__ballot(at_node || at_leaf) == 0) break;
        if (at_node) cur = closest_node(sc, p, cur, refs, bounds, c.d2);
        if (at_leaf) {                                   // one triangle of the leaf; the reference is consumed in place as leaf_step does
            const int slot = (int)((cur & 0x7fffffffu) >> 3);
            glb_f4v* r = (glb_f4v*)(reinterpret_cast<const char*>(sc.tris) + ((size_t)(uint32_t)slot << 6));
            closest_tri_eval(r[0], r[1], r[2], slot, p, c);
            cur += 7u;
            if ((cur & 7u) == 0u) cur = closest_pop(refs, bounds, c.d2);
        }
    }
    return c;
}

// pos as iris_intersect interpolates it (hit_position), from the record the winner was evaluated on
__device__ __forceinline__ f3 closest_position(const SceneDev& sc, const Closest& c) {
    Hit h; h.t = 0.f; h.u = c.b1; h.v = c.b2; h.slot = c.slot; h.id = c.id;
    f3 p0, p1, p2;
    hit_vertices(sc, h, p0, p1, p2);
    return hit_position(h, p0, p1, p2);
}

__global__ __launch_bounds__(kBlock) void closest_point_kernel(SceneDev sc, const float* __restrict__ xs, int64_t B, int64_t* __restrict__ tri, float* __restrict__ bary,
                                                               float* __restrict__ pos, float* __restrict__ dist2) {
    __shared__ uint32_t s_refs[kStackLds * kBlock];
    __shared__ uint32_t s_bounds[kStackLds * kBlock];
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < B; i += (int64_t)gridDim.x * kBlock) {
        const Closest c = closest_query(sc, ld3(xs + i * 3), s_refs + threadIdx.x, s_bounds + threadIdx.x);
        const bool found = c.slot >= 0;
        if (tri) tri[i] = found ? (int64_t)c.id : (int64_t)-1;
        if (bary) { bary[i * 2] = c.b1; bary[i * 2 + 1] = c.b2; }
        if (pos) st3(pos + i * 3, found ? closest_position(sc, c) : mk3(0.f, 0.f, 0.f));
        if (dist2) dist2[i] = c.d2;
    }
}

}  // namespace iris
