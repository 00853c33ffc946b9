#!/usr/bin/env python3
"""The segmentation fusion's three passes over one view (iris_amd/utils/segmentation.py, iris_amd/csrc/iris_labels.h) on one MI355X
-> profiles/fuse_segmentation_1080p.json.

Scene: the bench scene (tools/synth.room, --tris 1 000 000) and ONE 1080p view (tools/synth.camera); the view's label map is the hit triangle's index
modulo 40, plus 1 (0 where the ray hits nothing), so rows are 41 wide and the histogram is tris x 41 x 4 bytes.  In the same process, the arms taking turns
call by call (per-call HIP event times; --warmup calls, then the median and the half distance between the 16th and 84th percentile of --steps calls):

  trace_only           pool_view with no sink: ray generation and closest hit alone, the floor of the two view passes
  vote_fused           vote_view, a wave's equal (triangle, id) keys combined before the atomic (the default)
  vote_fused_per_lane  the same launch with one atomic per hit (iris_debug_set("pool_combine", 0)): the arm that decides which form is the default
  vote_composed        what it replaces, the reference's composition: cameras.view_rays + ray_intersect + boolean mask + scatter_add_ of int64 ones into a
                       flat int64 vector
  argmax_fused         triangle_labels against argmax_torch, hist[:, 1:].max(-1) plus the reference's +1 and zeroing
  view_fused           label_view against view_composed, cameras.view_rays + ray_intersect + gather + masked fill
Before anything is timed every fused pass, in both forms of the vote, is compared with its composition (integers: exact).  There is no earlier measurement
of either side: no time here is an acceptance threshold."""
import argparse, json, os, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--img_hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--ids", type=int, default=40, help="distinct ids in the label map")
    ap.add_argument("--steps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fuse_segmentation_1080p.json"))
    args = ap.parse_args()
    import torch
    from iris_amd import _lib as L
    from iris_amd.utils import cameras
    from iris_amd.utils.gbuffer import pool_view
    from iris_amd.utils.path_tracing import Scene, ray_intersect
    from iris_amd.utils.segmentation import label_view, triangle_labels, vote_view
    from tools import synth
    from tools.bench_prebake import half_spread, interleaved_ms, med
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse_segmentation needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    hw = tuple(args.img_hw)
    n = hw[0] * hw[1]
    room = synth.room(0, args.tris)
    scene = Scene(room["vertices"], room["faces"], device=dev)
    n_tri, n_labels = len(room["faces"]), args.ids + 1
    K, c2w = synth.camera(hw[0], hw[1], 0)
    view = {"kind": "real", "K": K, "c2w": c2w}
    cam = {"camera": view, "img_hw": hw}

    def hits():
        xs, ds = cameras.view_rays(view, hw, dev)
        _, _, _, idx, valid = ray_intersect(scene, xs, ds)
        return idx, valid

    idx, valid = hits()
    labels = torch.where(valid, idx % args.ids + 1, torch.zeros_like(idx)).float()
    hit_pixels, seen_triangles = int(valid.sum()), int(torch.unique(idx[valid]).numel())

    def per_lane(fn):
        def call():
            L.debug_set("pool_combine", 0)
            try:
                fn()
            finally:
                L.debug_set("pool_combine", -1)
        return call

    def new_hist():
        return torch.zeros(n_tri, n_labels, dtype=torch.int32, device=dev)

    def vote_composed(flat):                              # fuse_segmentation.py:72-81
        idx, valid = hits()
        inds = idx[valid] * n_labels + labels.long()[valid]
        flat.scatter_add_(0, inds, torch.ones_like(inds))

    def argmax_torch(hist):                               # fuse_segmentation.py:84-87
        count, label = hist[:, 1:].max(-1)
        label = label + 1
        label[count == 0] = 0
        return label

    def view_composed(table):                             # fuse_segmentation.py:98-100
        idx, valid = hits()
        out = table[idx.clamp_min(0)]
        out[~valid] = 0
        return out.float()

    # same results first
    a, b, flat = new_hist(), new_hist(), torch.zeros(n_tri * n_labels, dtype=torch.int64, device=dev)
    vote_view(scene, a, labels, **cam)
    per_lane(lambda: vote_view(scene, b, labels, **cam))()
    vote_composed(flat)
    table = triangle_labels(a)
    same = {"vote": bool(torch.equal(a.long(), flat.reshape(n_tri, n_labels))), "vote_per_lane": bool(torch.equal(b, a)),
            "argmax": bool(torch.equal(table.long(), argmax_torch(a).long())),
            "view": bool(torch.equal(label_view(scene, table, **cam), view_composed(table)))}
    assert all(same.values()), same
    assert int(a.sum()) == hit_pixels

    voted = a.clone()                                     # (the timed votes go on adding to a and b; the argmax arms read this copy)
    arms = {"trace_only": lambda: pool_view(scene, **cam),
            "vote_fused": lambda: vote_view(scene, a, labels, **cam),
            "vote_fused_per_lane": per_lane(lambda: vote_view(scene, b, labels, **cam)),
            "vote_composed": lambda: vote_composed(flat),
            "argmax_fused": lambda: triangle_labels(voted),
            "argmax_torch": lambda: argmax_torch(voted),
            "view_fused": lambda: label_view(scene, table, **cam),
            "view_composed": lambda: view_composed(table)}
    ms = interleaved_ms(arms, args.steps, args.warmup)
    rows = {k: {"ms": med(v), "half_spread_ms": half_spread(v)} for k, v in ms.items()}
    ratio = lambda x, y: round(rows[x]["ms"] / rows[y]["ms"], 3)
    rows["vote_fused"].update(composed_over_fused=ratio("vote_composed", "vote_fused"), per_lane_over_combined=ratio("vote_fused_per_lane", "vote_fused"),
                              trace_share=round(rows["trace_only"]["ms"] / rows["vote_fused"]["ms"], 4))
    rows["argmax_fused"].update(torch_over_fused=ratio("argmax_torch", "argmax_fused"))
    rows["view_fused"].update(composed_over_fused=ratio("view_composed", "view_fused"), trace_share=round(rows["trace_only"]["ms"] / rows["view_fused"]["ms"], 4))
    res = {"what": "one 1080p view of the bench scene through the segmentation fusion's passes: vote_view, triangle_labels and label_view (one launch each) against "
                   "the compositions they replace, interleaved; per-call HIP event medians (ms)",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "tris": n_tri, "img_hw": list(hw), "pixels": n, "hit_pixels": hit_pixels,
           "seen_triangles": seen_triangles, "n_labels": n_labels, "hist_bytes": n_tri * n_labels * 4, "steps": args.steps, "warmup": args.warmup,
           "same_results": same, "rows": rows,
           "wave_combining": "vote_fused combines a wave's equal (triangle, id) keys before the atomic; vote_fused_per_lane issues one atomic per hit "
                             "(iris_debug_set pool_combine 0), as the composition's scatter_add_ does",
           "not_measured": "more than one view per histogram; label maps with other id statistics (this one gives neighbouring pixels of a triangle the same id); "
                           "the uint8 forms; the command line end to end (EXR decode and encode); kernel times by profiler"}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
