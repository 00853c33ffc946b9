// How deep does the traversal stack of iris_trace.h get?  Builds the 4-wide tree of a mesh with the library's own builder (bvh_build.cpp) and replays, per ray, the
// PUSH RULE of the kernels on the host -- no GPU: tests/test_deep_stack_cpu.py asserts on its output the preconditions tests/test_deep_stack.py relies on.
//   Q8 rule   (node_step<kLayoutQ8>, node_step_shared, node_eval_q8): the children in the ray octant's front-to-back order (WideNode::order), tested against the node's
//             8-bit planes; the first child hit is visited next, the other hit children are pushed, the farthest first.
//   F32 rule  (node_step<kLayoutF32>): the f32 boxes, the children sorted by entry distance with the kernel's five compare-exchanges.
// Both cull against the closest hit so far, test a leaf's triangles with the watertight test's arithmetic and pop when a leaf is done or no child is hit.
// The slab arithmetic is the kernels' in float (1 / d where the device takes v_rcp_f32: a ray that grazes a box within an ulp may differ).
//
//   stack_replay SCENE RAYS [max_leaf = 4] [presplit = 8.0]      -> one JSON object on stdout
//   SCENE: int32 nv, int32 nf, float verts[nv][3], int32 faces[nf][3]       RAYS: int32 n, float o[n][3], float d[n][3]        (little endian, as numpy writes them)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "bvh_build.h"

using namespace iris;

namespace {

constexpr float kInf = std::numeric_limits<float>::infinity();

template <class T> bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

float safe_rcp_dir(float d) { return std::fabs(d) < 1e-20f ? std::copysign(1e20f, d) : 1.0f / d; }

struct Ray {
    float o[3], d[3];
    float i[3], n[3];      // 1 / d, -(o / d)
    int oct;
    // the watertight test's transform (iris_trace.h ray_xform)
    int kx, ky, kz;
    float sx, sy, sz;
    float t; int id;       // closest hit so far: lexicographic minimum of (t, index)
};

void ray_begin(Ray& r, const float* o, const float* d) {
    for (int k = 0; k < 3; ++k) { r.o[k] = o[k]; r.d[k] = d[k]; r.i[k] = safe_rcp_dir(d[k]); r.n[k] = -(o[k] * r.i[k]); }
    r.oct = (r.i[0] >= 0.f ? 0 : 1) | (r.i[1] >= 0.f ? 0 : 2) | (r.i[2] >= 0.f ? 0 : 4);
    const float ax = std::fabs(d[0]), ay = std::fabs(d[1]), az = std::fabs(d[2]);
    r.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    r.kx = r.kz == 2 ? 0 : r.kz + 1; r.ky = r.kx == 2 ? 0 : r.kx + 1;
    r.sz = 1.0f / d[r.kz]; r.sx = d[r.kx] * r.sz; r.sy = d[r.ky] * r.sz;
    r.t = kInf; r.id = std::numeric_limits<int>::min();
}

void tri_test(Ray& r, const float* verts, const int32_t* faces, int32_t f) {
    const float* p[3];
    for (int v = 0; v < 3; ++v) p[v] = verts + (int64_t)faces[(int64_t)f * 3 + v] * 3;
    const float ox = r.o[r.kx], oy = r.o[r.ky], oz = r.o[r.kz];
    const float Atz = p[0][r.kz] - oz, Btz = p[1][r.kz] - oz, Ctz = p[2][r.kz] - oz;
    const float Ax = std::fmaf(-r.sx, Atz, p[0][r.kx] - ox), Ay = std::fmaf(-r.sy, Atz, p[0][r.ky] - oy);
    const float Bx = std::fmaf(-r.sx, Btz, p[1][r.kx] - ox), By = std::fmaf(-r.sy, Btz, p[1][r.ky] - oy);
    const float Cx = std::fmaf(-r.sx, Ctz, p[2][r.kx] - ox), Cy = std::fmaf(-r.sy, Ctz, p[2][r.ky] - oy);
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (std::fmin(std::fmin(std::fabs(U), std::fabs(V)), std::fabs(W)) == 0.f) {
        U = (float)((double)Cx * By - (double)Cy * Bx);
        V = (float)((double)Ax * Cy - (double)Ay * Cx);
        W = (float)((double)Bx * Ay - (double)By * Ax);
    }
    const float det = (U + V) + W;
    const float inv_det = 1.0f / det;
    const float t = (std::fmaf(U, Atz, std::fmaf(V, Btz, W * Ctz)) * r.sz) * inv_det;
    const bool mixed = std::fmin(std::fmin(U, V), W) < 0.f && std::fmax(std::fmax(U, V), W) > 0.f;
    if (!mixed && t >= 0.f && (t < r.t || (t == r.t && f < r.id))) { r.t = t; r.id = f; }
}

struct Tree {
    WideBvh bvh;
    std::vector<QuantNode> q;
};

// the references a node visit leaves: next (or "none"), and the pushes in push order
struct Step { uint32_t next; bool any; uint32_t push[3]; int n_push; };

uint32_t ref_of(const Tree& t, const WideNode& w, int s) { return s < w.n ? child_ref(w, s) : leaf_ref((uint32_t)t.bvh.tri_order.size(), 1u); }

Step step_q8(const Tree& t, const Ray& r, uint32_t cur) {
    const WideNode& w = t.bvh.nodes[cur];
    const QuantNode& q = t.q[cur];
    float a[3], b[3];
    for (int k = 0; k < 3; ++k) { a[k] = std::ldexp(1.0f, q.exp[k]) * r.i[k]; b[k] = std::fmaf(q.origin[k], r.i[k], r.n[k]); }
    bool hit[4]; uint32_t ref[4];
    for (int j = 0; j < 4; ++j) {
        const int sl = j < w.n ? (int)w.order[r.oct][j] : j;
        float tn = 0.f, tf = r.t;
        for (int k = 0; k < 3; ++k) {
            const bool neg = (r.oct >> k) & 1;
            const uint8_t lo = sl < w.n ? q.lo[k][sl] : 255, hi = sl < w.n ? q.hi[k][sl] : 0;
            tn = std::fmax(tn, std::fmaf((float)(neg ? hi : lo), a[k], b[k]));
            tf = std::fmin(tf, std::fmaf((float)(neg ? lo : hi), a[k], b[k]));
        }
        hit[j] = !std::signbit(tf - tn);
        ref[j] = ref_of(t, w, sl);
    }
    Step s{}; s.any = hit[0] || hit[1] || hit[2] || hit[3];
    if (!s.any) return s;
    int first = 0; while (!hit[first]) ++first;
    s.next = ref[first];
    for (int j = 3; j > first; --j) if (hit[j]) s.push[s.n_push++] = ref[j];
    return s;
}

Step step_f32(const Tree& t, const Ray& r, uint32_t cur) {
    const WideNode& w = t.bvh.nodes[cur];
    float key[4]; uint32_t ref[4];
    for (int s = 0; s < 4; ++s) {
        float tn = 0.f, tf = r.t;
        for (int k = 0; k < 3; ++k) {
            const bool pos = r.i[k] >= 0.f;
            tn = std::fmax(tn, std::fmaf(pos ? w.lo[s][k] : w.hi[s][k], r.i[k], r.n[k]));
            tf = std::fmin(tf, std::fmaf(pos ? w.hi[s][k] : w.lo[s][k], r.i[k], r.n[k]));
        }
        key[s] = tn <= tf ? tn : kInf;
        ref[s] = ref_of(t, w, s);
    }
    auto ce = [&](int x, int y) { if (key[y] < key[x]) { std::swap(key[x], key[y]); std::swap(ref[x], ref[y]); } };
    ce(0, 1); ce(2, 3); ce(0, 2); ce(1, 3); ce(1, 2);
    Step s{}; s.any = key[0] < kInf;
    if (!s.any) return s;
    s.next = ref[0];
    for (int j = 3; j >= 1; --j) if (key[j] < kInf) s.push[s.n_push++] = ref[j];
    return s;
}

// the largest number of entries the ray's stack holds at any time
int replay(const Tree& t, const float* verts, const int32_t* faces, const float* o, const float* d, bool q8, int* hit_id) {
    Ray r; ray_begin(r, o, d);
    std::vector<uint32_t> stack;
    size_t max_sp = 0;
    const uint32_t none = 0xFFFFFFFFu;
    const size_t n_rec = t.bvh.tri_order.size();
    uint32_t cur = 0;
    while (cur != none) {
        if (cur & kLeafBit) {
            const uint32_t start = leaf_ref_start(cur), count = leaf_ref_count(cur);
            for (uint32_t i = start; i < start + count; ++i)
                if (i < n_rec) tri_test(r, verts, faces, t.bvh.tri_order[i]);        // (record n_rec: the degenerate one unused slots refer to, never accepted)
            if (stack.empty()) cur = none; else { cur = stack.back(); stack.pop_back(); }
            continue;
        }
        const Step s = q8 ? step_q8(t, r, cur) : step_f32(t, r, cur);
        if (!s.any) {
            if (stack.empty()) cur = none; else { cur = stack.back(); stack.pop_back(); }
            continue;
        }
        cur = s.next;
        for (int j = 0; j < s.n_push; ++j) stack.push_back(s.push[j]);
        max_sp = std::max(max_sp, stack.size());
    }
    *hit_id = r.t < kInf ? r.id : -1;
    return (int)max_sp;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: stack_replay SCENE RAYS [max_leaf] [presplit]\n"); return 2; }
    const int max_leaf = argc > 3 ? std::atoi(argv[3]) : 4;
    const float presplit = argc > 4 ? (float)std::atof(argv[4]) : 8.f;
    std::vector<float> verts, o, d; std::vector<int32_t> faces;
    int32_t nv = 0, nf = 0, nr = 0;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(&nv, 4, 1, f) != 1 || std::fread(&nf, 4, 1, f) != 1 || nv < 0 || nf < 0 || !read_vec(f, verts, (size_t)nv * 3) || !read_vec(f, faces, (size_t)nf * 3)) {
        std::fprintf(stderr, "stack_replay: cannot read the scene %s\n", argv[1]); return 2;
    }
    std::fclose(f);
    for (int32_t i : faces) if (i < 0 || i >= nv) { std::fprintf(stderr, "stack_replay: face index out of range\n"); return 2; }
    f = std::fopen(argv[2], "rb");
    if (!f || std::fread(&nr, 4, 1, f) != 1 || nr < 0 || !read_vec(f, o, (size_t)nr * 3) || !read_vec(f, d, (size_t)nr * 3)) {
        std::fprintf(stderr, "stack_replay: cannot read the rays %s\n", argv[2]); return 2;
    }
    std::fclose(f);

    if (!buildable_extent(verts.data(), faces.data(), nf)) {          // what iris_scene_create refuses with IRIS_ERR_ARG
        const WideBvh none = build_wide_bvh(verts.data(), nv, faces.data(), nf, 4, max_leaf, 2e-5f, 0.7f, presplit);     // (must come back, empty)
        std::printf("{\"buildable\": false, \"n_nodes\": %zu}\n", none.nodes.size());
        return 0;
    }
    Tree t;
    t.bvh = build_wide_bvh(verts.data(), nv, faces.data(), nf, 4, max_leaf, 2e-5f, 0.7f, presplit);
    t.q.resize(t.bvh.nodes.size());
    bool quantised = true;
    for (size_t i = 0; i < t.bvh.nodes.size(); ++i) quantised = quantise_node(t.bvh.nodes[i], 4, t.q[i]) && quantised;
    std::printf("{\"buildable\": true, \"depth\": %d, \"n_nodes\": %zu, \"n_leaf_records\": %zu, \"quantised\": %s, \"rays\": %d", t.bvh.depth, t.bvh.nodes.size(),
                t.bvh.tri_order.size(), quantised ? "true" : "false", nr);
    for (int pass = 0; pass < 2; ++pass) {
        const bool q8 = pass == 0;
        if (q8 && !quantised) { std::printf(", \"max_q8\": [], \"hit_q8\": []"); continue; }
        std::vector<int> mx((size_t)nr), hit((size_t)nr);
        for (int32_t i = 0; i < nr; ++i) mx[(size_t)i] = replay(t, verts.data(), faces.data(), &o[(size_t)i * 3], &d[(size_t)i * 3], q8, &hit[(size_t)i]);
        std::printf(", \"max_%s\": [", q8 ? "q8" : "f32");
        for (int32_t i = 0; i < nr; ++i) std::printf("%s%d", i ? "," : "", mx[(size_t)i]);
        std::printf("], \"hit_%s\": [", q8 ? "q8" : "f32");
        for (int32_t i = 0; i < nr; ++i) std::printf("%s%d", i ? "," : "", hit[(size_t)i]);
        std::printf("]");
    }
    std::printf("}\n");
    return 0;
}
