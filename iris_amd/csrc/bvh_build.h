// Host-side BVH construction for libiris_hip.so: binned-SAH binary build, collapse to a W-wide tree, and the encoding of that tree into the
// node / leaf-record tables the kernels read (host-only C++: the library, tools/bvh_eval and tests/native use the same encoder).
// (The reference has no counterpart: it calls mitsuba.load_dict -> OptiX GAS build, bake_shading.py:55-61.)
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace iris {

constexpr int kMaxWidth = 8;

struct WideNode {
    int n = 0;                       // children in use (slots [0,n))
    float lo[kMaxWidth][3];          // child boxes (already padded)
    float hi[kMaxWidth][3];
    int32_t child[kMaxWidth];        // >=0: index of an internal wide node; -1: leaf
    int32_t leaf_start[kMaxWidth];   // leaf: first triangle in tri_order
    int32_t leaf_count[kMaxWidth];   // leaf: number of triangles
    uint8_t order[8][kMaxWidth];     // per ray octant (bit 0: d.x < 0, bit 1: d.y < 0, bit 2: d.z < 0): the slots in front-to-back order as the binary splits the
                                     // node was collapsed from give it (at every split the side the ray enters first; the left child holds the lower centroids)
};

struct WideBvh {
    int width = 0;
    std::vector<WideNode> nodes;     // nodes[0] is the root; the internal children of a node are consecutive
    std::vector<int32_t> tri_order;  // leaf order -> original triangle index; a node's leaf triangles are consecutive.  Longer than the mesh
                                     // when long triangles were split into several references (presplit): those appear once per reference
    float root_lo[3], root_hi[3];
    int depth = 0;
    float sah_cost = 0.f;
    float pad = 0.f;
};

// verts: (nv,3) f32, faces: (nf,3) i32.  leaf_tris: max triangles per leaf (1..7).  tri_cost: cost of one triangle test relative to
// one wide-node visit in the SAH the collapse minimises (measured on the traversal kernels: ~70 against ~110 instructions).
// Boxes are padded by `pad_rel * max(|coordinate|, extent)` so that the f32 slab test is conservative with respect to the
// Moeller-Trumbore test (see DESIGN.md "closest-hit semantics").  presplit: early split clipping of triangles whose box is longer than
// presplit x the median triangle's (0 = off), see bvh_build.cpp.
// A mesh whose bounding-box AREA is not finite in float32 (coordinates beyond ~1e19 apart) cannot be built: every SAH cost is inf or NaN.  build_wide_bvh
// returns a tree without nodes (depth 0) for it; callers refuse such a mesh up front with buildable_extent().
WideBvh build_wide_bvh(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, int width, int leaf_tris,
                       float pad_rel = 2e-5f, float tri_cost = 0.7f, float presplit = 8.f);
// true when the area of the mesh's bounding box, as the builder computes it, is finite (an empty mesh is)
bool buildable_extent(const float* verts, const int32_t* faces, int64_t nf);

// ------------------------------------------------------------------------------------------------------
// The tree as the kernels read it (iris_trace.h): what this encoder and the traversal share.
// ------------------------------------------------------------------------------------------------------
// Node layouts (iris_hip.h): BVH4_F32 = 128-B node with f32 planes (7 dwordx4 per visit); BVH4_Q8 = 64-B node
// {origin.xyz, scale.x | scale.y, scale.z, qlo_x, qlo_y | qlo_z, qhi_x, qhi_y, qhi_z | ref[4]} with 8-bit planes relative to the node's
// own box (4 dwordx4 per visit): plane = origin + q * 2^e per axis (the node stores 2^(e+24) as a float, see node_step), lo rounded down /
// hi rounded up, so the decoded box contains the f32 box.
constexpr int kLayoutF32 = 1, kLayoutQ8 = 3;
// Q8 node record: 64 B, 8-bit planes four to a word (a visit isolates near / far byte pairs with 12 v_perm_b32).
constexpr uint32_t kNodeBytes = 64u;
constexpr uint32_t kNodeBytesF32 = 128u;
constexpr uint32_t kLeafRecordBytes = 64u;   // one leaf triangle per 64-B line
// A child reference is the index of an internal node, or a leaf: kLeafBit | first record << 3 | number of records (1..7).
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t leaf_ref(uint32_t start, uint32_t count) { return kLeafBit | (start << 3) | count; }
constexpr uint32_t leaf_ref_start(uint32_t ref) { return (ref & ~kLeafBit) >> 3; }
constexpr uint32_t leaf_ref_count(uint32_t ref) { return ref & 7u; }
inline uint32_t child_ref(const WideNode& w, int s) {   // slot s < w.n
    return w.child[s] >= 0 ? (uint32_t)w.child[s] : leaf_ref((uint32_t)w.leaf_start[s], (uint32_t)w.leaf_count[s]);
}

// The 8-bit planes of one node: per axis k the plane q stands for origin[k] + q * 2^exp[k].  Slots [n, width) carry the inverted box (lo 255, hi 0).
struct QuantNode {
    int n;                           // children in use, as WideNode::n
    float origin[3];
    int exp[3];
    uint8_t lo[3][kMaxWidth], hi[3][kMaxWidth];
};
struct NodeBoxes { float lo[kMaxWidth][3], hi[kMaxWidth][3]; };
// Conservative: every decoded child box contains the builder's f32 box.  false when 255 steps of the axis' scale cannot reach a child's upper plane.
bool quantise_node(const WideNode& w, int width, QuantNode& q);
inline float decode_plane(float origin, int exp, uint8_t q) { return (float)((double)origin + (double)q * std::ldexp(1.0, exp)); }
// The boxes those bytes stand for; unused slots come back as the empty box (+inf, -inf).
void decode_node(const QuantNode& q, NodeBoxes& out);

// The node table of a 4-wide tree in `layout`, as floats (references bit-copied).  F32: one 128-B record per node, lox[4] hix[4] loy[4] hiy[4] loz[4]
// hiz[4] ref[4] pad[4].  Q8: EIGHT tables of 64-B records, one per ray octant, one behind the other (see bvh_build.cpp).  Unused child slots refer to the
// degenerate leaf record encode_leaf_records appends.  Empty when a node cannot be quantised (or the tree is not 4-wide).
std::vector<float> encode_nodes(const WideBvh& bvh, int layout);
// The leaf records (64 B each, in tri_order) + the degenerate record: tri_order.size() + 1 records.
std::vector<float> encode_leaf_records(const WideBvh& bvh, const float* verts, const int32_t* faces);

}  // namespace iris
