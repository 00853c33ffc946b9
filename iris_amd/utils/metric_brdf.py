"""python -m iris_amd.utils.metric_brdf --gt DIR --method DIR: the reference's utils/metric_brdf.py -- the material table of a synthetic scene -- with its
hard-coded paths made arguments and without cv2 and pandas.

--gt is the split folder of a synthetic scene (Image/, Emit/, albedo/, DiffCol/, Roughness/), --method is <output_path>/<split> of python -m iris_amd.render.
The view count is the number of Image/*.exr files under --gt, as in the reference.  The files of --batch views are decoded on the utils.exr.chunk_pool()
threads, uploaded once and scored by one launch of the fused kernel (utils/material_metrics.py); the run is bound by decoding the files on the host.
Prints the reference's five lines; --json FILE also writes them with the per-view values and the raw integer sums.

Not here: the real and scannetpp layouts (they have no ground truth) and the reference's commented-out gamma variant of the emission error.
"""
import json
import os

from .. import _lib as L
from . import material_metrics as M
from .stage import exit_status

NAME = "metric_brdf"


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="python -m iris_amd.utils.metric_brdf: the reference's utils/metric_brdf.py on MI355X")
    parser.add_argument("--gt", type=str, required=True, metavar="DIR", help="the split folder of a synthetic scene: Image/, Emit/, albedo/, DiffCol/, Roughness/")
    parser.add_argument("--method", type=str, required=True, metavar="DIR", help="<output_path>/<split> of python -m iris_amd.render: emission/, a_prime/, diffuse/, roughness/")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--max_views", type=int, default=None)
    parser.add_argument("--batch", type=int, default=8, help="views per kernel launch")
    parser.add_argument("--json", type=str, default=None, metavar="FILE", help="also write the five numbers, the per-view values and the raw sums here")
    return parser


def write_json(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main(argv=None):
    from .exr import chunk_pool
    from .stage import open_device
    args = build_parser().parse_args(argv)
    if args.batch < 1:
        raise L.IrisError("--batch must be at least 1")
    n_views = M.count_views(args.gt)
    if args.max_views is not None:
        n_views = min(n_views, max(args.max_views, 0))
    if n_views == 0:
        raise L.IrisError(f"{os.path.join(args.gt, 'Image')}: no .exr file, so no view to score")
    if not os.path.isdir(args.method):
        raise L.IrisError(f"{args.method}: no such folder (--method is <output_path>/<split> of the render stage)")
    img_hw = M.load_gt_view(args.gt, 0)["emit"].shape[:2]

    def load(i):
        g, e = M.load_gt_view(args.gt, i), M.load_method_view(args.method, i)
        for what, maps in (("ground truth", g), ("method", e)):
            if maps["emit"].shape[:2] != img_hw:
                raise L.IrisError(f"view {i}: the {what} maps are {maps['emit'].shape[0]} x {maps['emit'].shape[1]}, view 0's ground truth {img_hw[0]} x {img_hw[1]}")
        return g, e
    first = load(0)                       # (a missing or mis-sized first view ends the run before the device is opened)
    device = open_device(args.device, NAME)
    pool, table = chunk_pool(), M.Table(img_hw)
    for start in range(0, n_views, args.batch):
        loaded = ([first] if start == 0 else []) + list(pool.map(load, range(max(start, 1), min(start + args.batch, n_views))))
        table.add(M.material_metrics(M.upload([g for g, _ in loaded], device), M.upload([e for _, e in loaded], device)))
    summary, doc = table.finish()
    print(M.format_summary(summary))
    if args.json:
        write_json(args.json, dict(doc, gt=args.gt, method=args.method))
    return 0


def cli(argv=None):
    return exit_status(NAME, main, argv)


if __name__ == "__main__":
    raise SystemExit(cli())
