"""The material table of the reference's utils/metric_brdf.py on the device: PSNR of kd, a_prime (albedo) and roughness, emission IoU and emission log-MSE of
a method's maps against a synthetic scene's ground-truth EXR maps.

The reference compares x / 255 values in float32; 51 / 255 and 255 / 255 round to float32 0.2 and 1, so its clamps and its `== 1` test are tests of the 8-bit
code value and three of its five metrics are sums of squared integer differences, the IoU three counts.  One fused HIP kernel
(iris_amd/csrc/iris_matmetrics.h, where the per-pixel contract is stated) returns those integers exactly and the emission log-MSE's sum in float64, for a
stack of views per launch, from either the PNGs' code values or the float32 maps the render stage holds (quantised in the kernel as render.save_png does):
the numbers are the same bits on every call and the same for the files and for the tensors they were written from.
"""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib as L

GT_KEYS = ("emit", "albedo", "kd", "rough")
SUM_NAMES = ("S_albedo", "S_kd", "S_rough", "n_gt", "n_est", "n_and", "n_or", "S_emit")
SUMMARY_KEYS = ("kd", "albedo", "roughness", "emit_iou", "emit_log_mse")            # the order metric_brdf.py:88-92 prints them in


def _stack(d, who, key, channels, dtypes):
    t = d[key]
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.IrisError(f"material_metrics: {who}['{key}']: expected a tensor on a HIP device (got {getattr(t, 'device', type(t))}); iris_amd has no CPU path")
    if t.dtype not in dtypes:
        raise L.IrisError(f"material_metrics: {who}['{key}'] has dtype {t.dtype}; expected {' or '.join(str(x) for x in dtypes)}")
    want = 3 + (channels == 3)
    if t.dim() == want - 1:
        t = t[None]
    if t.dim() != want or (channels == 3 and t.shape[-1] != 3):
        raise L.IrisError(f"material_metrics: {who}['{key}'] has shape {tuple(d[key].shape)}; expected " + ("(H,W,3) or (N,H,W,3)" if channels == 3 else "(H,W) or (N,H,W)"))
    return t.detach().contiguous()


def material_metrics(gt, est):
    """gt: {'emit', 'albedo', 'kd': (N,H,W,3) or (H,W,3), 'rough': (N,H,W) or (H,W)} GPU float32, the ground-truth maps as the EXR files hold them;
    est: the same keys, 'emit' float32, 'albedo', 'kd', 'rough' each uint8 code values (a PNG as read) or float32 (quantised as save_png does).
    -> device tensors, nothing synchronises with the host:
        'sums' (N,8) int64: S_albedo, S_kd, S_rough, n_gt, n_est, n_and, n_or and, in [:,7], the BITS of the double S_emit ('s_emit' (N,) float64 views it);
        'mse_albedo', 'mse_kd' = S / (255^2 3 H W), 'mse_roughness' = S_rough / (255^2 H W), 'emit_iou' = n_and / n_or, 'emit_log_mse' = S_emit / (3 H W),
        (N,) float64; the two emission metrics are NaN for a view without a ground-truth emitter (n_gt == 0), which the reference leaves out of its means."""
    for who, d in (("gt", gt), ("est", est)):
        if not isinstance(d, dict):
            raise L.IrisError(f"material_metrics: {who} must be a dict with the keys {', '.join(GT_KEYS)}")
        for k in GT_KEYS:
            if k not in d:
                raise L.IrisError(f"material_metrics: {who} has no '{k}' (keys: {', '.join(GT_KEYS)})")
    f32, either = (torch.float32,), (torch.uint8, torch.float32)
    g = {k: _stack(gt, "gt", k, 1 if k == "rough" else 3, f32) for k in GT_KEYS}
    e = {k: _stack(est, "est", k, 1 if k == "rough" else 3, f32 if k == "emit" else either) for k in GT_KEYS}
    N, H, W = (int(s) for s in g["rough"].shape)
    dev = g["rough"].device
    for who, d in (("gt", g), ("est", e)):
        for k, t in d.items():
            if tuple(t.shape[:3]) != (N, H, W):
                raise L.IrisError(f"material_metrics: {who}['{k}'] is {tuple(t.shape)}, gt['rough'] {(N, H, W)}")
            if t.device != dev:
                raise L.IrisError(f"material_metrics: {who}['{k}'] is on {t.device}, gt['rough'] on {dev}")
    L.no_autograd("material_metrics", *gt.values(), *est.values())
    lib = L.lib()
    need = int(lib.iris_material_metrics_workspace_bytes(N, H, W))
    if need == 0:
        raise L.IrisError(f"material_metrics: size (N, H, W) = {(N, H, W)} is not supported: N, H, W >= 1, H W <= 2^30, N ceil(H W / 512) < 2^31")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    sums = torch.empty(N, 8, dtype=torch.int64, device=dev)
    a = L.MaterialMetricsArgs(emit_gt=L.ptr(g["emit"]), albedo_gt=L.ptr(g["albedo"]), kd_gt=L.ptr(g["kd"]), rough_gt=L.ptr(g["rough"]), emit=L.ptr(e["emit"]),
                              albedo=L.ptr(e["albedo"]), kd=L.ptr(e["kd"]), rough=L.ptr(e["rough"]), sums=L.ptr(sums), workspace=L.ptr(ws), workspace_bytes=need,
                              albedo_is_u8=int(e["albedo"].dtype == torch.uint8), kd_is_u8=int(e["kd"].dtype == torch.uint8),
                              rough_is_u8=int(e["rough"].dtype == torch.uint8), N=N, H=H, W=W)
    with torch.cuda.device(dev):
        L.check(lib.iris_material_metrics(C.byref(a), L.stream()))
    s_emit = sums[:, 7:8].view(torch.float64)[:, 0]
    s = sums.to(torch.float64)
    # (tensor / tensor: a correctly rounded float64 division; torch divides a device tensor by a Python scalar as a product with the reciprocal)
    den = lambda v: torch.full_like(s_emit, float(v))
    nan = den(float("nan"))
    has = sums[:, 3] > 0
    return {"sums": sums, "s_emit": s_emit,
            "mse_albedo": s[:, 0] / den(65025 * 3 * H * W), "mse_kd": s[:, 1] / den(65025 * 3 * H * W), "mse_roughness": s[:, 2] / den(65025 * H * W),
            "emit_iou": torch.where(has, s[:, 5] / s[:, 6], nan), "emit_log_mse": torch.where(has, s_emit / den(3 * H * W), nan)}


def per_view_from_sums(sums, s_emit, H, W):
    """the per-view values of material_metrics from host copies of its sums -- (V,8) integers and (V,) float64 -- in numpy float64, the same expressions"""
    sums = np.asarray(sums, np.int64).reshape(-1, 8)
    s_emit = np.asarray(s_emit, np.float64).reshape(-1)
    s, hw = sums.astype(np.float64), float(H * W)
    has = sums[:, 3] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"mse_albedo": s[:, 0] / (65025.0 * 3.0 * hw), "mse_kd": s[:, 1] / (65025.0 * 3.0 * hw), "mse_roughness": s[:, 2] / (65025.0 * hw),
                "emit_iou": np.where(has, s[:, 5] / s[:, 6], np.nan), "emit_log_mse": np.where(has, s_emit / (3.0 * hw), np.nan)}


def summarize(per_view):
    """metric_brdf.py:88-92 -> {'kd', 'albedo', 'roughness', 'emit_iou', 'emit_log_mse'}, Python floats.  per_view: the per-view values of material_metrics
    (device tensors, arrays or lists; only mse_kd, mse_albedo, mse_roughness, emit_iou, emit_log_mse are read): the three PSNRs are the mean over the views of
    -10 log10(max(mse, 1e-10)); the emission metrics the mean over the views that have an emitter (not NaN), NaN when none has.  float64 throughout."""
    def host(key):
        v = per_view[key]
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        return v.astype(np.float64).reshape(-1)

    def psnr(key):
        mse = host(key)
        return float(np.mean(-10.0 * np.log10(np.maximum(mse, 1e-10)))) if mse.size else float("nan")

    def emitter_mean(key):
        v = host(key)
        v = v[~np.isnan(v)]
        return float(np.mean(v)) if v.size else float("nan")
    return {"kd": psnr("mse_kd"), "albedo": psnr("mse_albedo"), "roughness": psnr("mse_roughness"), "emit_iou": emitter_mean("emit_iou"),
            "emit_log_mse": emitter_mean("emit_log_mse")}


def format_summary(summary):
    """the reference's five lines (metric_brdf.py:88-92), same order, same labels"""
    labels = {"kd": "kd:          ", "albedo": "albedo:      ", "roughness": "roughness:   ", "emit_iou": "emit_iou:    ", "emit_log_mse": "emit_log_mse:"}
    return "\n".join("{} {}".format(labels[k], summary[k]) for k in SUMMARY_KEYS)


# ---- the files
def _read_exr(path):
    """utils.exr.read_exr of a file that must exist and be one it decodes (NONE, ZIPS, ZIP; half or float samples)"""
    from .exr import _LINES, read_exr, read_exr_header
    if not os.path.isfile(path):
        raise L.IrisError(f"{path}: no such file")
    comp = read_exr_header(path)["compression"]
    if comp not in _LINES:
        raise L.IrisError(f"{path}: EXR compression {comp} is not read here (NONE, ZIPS and ZIP only): re-save the file with one of them")
    return read_exr(path)


def _blue(a):
    """what cv2.imread(path, -1)[..., 0] is: the B channel of a colour image, the only channel of a single-channel one"""
    return np.ascontiguousarray(a[..., 2] if a.shape[-1] >= 3 else a[..., 0])


def _rgb3(a, path):
    if a.ndim != 3 or a.shape[-1] < 3:
        raise L.IrisError(f"{path}: three colour channels expected, the file has {a.shape[-1] if a.ndim == 3 else 1}")
    return np.ascontiguousarray(a[..., :3])


def load_gt_view(dir, i):
    """View i of a synthetic scene's split folder (metric_brdf.py:32-43): Emit/{i:03d}_0001.exr, albedo/{i:03d}.exr, DiffCol/{i:03d}_0001.exr,
    Roughness/{i:03d}_0001.exr -> {'emit', 'albedo', 'kd' (H,W,3), 'rough' (H,W)} float32 arrays, raw as stored; roughness is the file's B channel."""
    paths = {"emit": os.path.join(dir, "Emit", "{:03d}_0001.exr".format(i)), "albedo": os.path.join(dir, "albedo", "{:03d}.exr".format(i)),
             "kd": os.path.join(dir, "DiffCol", "{:03d}_0001.exr".format(i)), "rough": os.path.join(dir, "Roughness", "{:03d}_0001.exr".format(i))}
    out = {k: _read_exr(p) for k, p in paths.items()}
    out = {k: (_blue(a) if k == "rough" else _rgb3(a, paths[k])).astype(np.float32, copy=False) for k, a in out.items()}
    return _same_size(out, paths)


def _read_png(path):
    from PIL import Image
    if not os.path.isfile(path):
        raise L.IrisError(f"{path}: no such file")
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA", "L", "P"):
            raise L.IrisError(f"{path}: an 8-bit PNG is expected, the file's mode is {im.mode}")
        return np.array(im.convert("RGB"), dtype=np.uint8)


def load_method_view(dir, i):
    """View i of <output_path>/<split> of the render stage (metric_brdf.py:51-64): emission/{i:05d}_emission.exr (float32), a_prime/{i:05d}_a_prime.png,
    diffuse/{i:05d}_kd.png, roughness/{i:05d}_roughness.png -> {'emit' (H,W,3) float32, 'albedo', 'kd' (H,W,3) uint8, 'rough' (H,W) uint8}: the PNGs stay
    code values; roughness is the file's B channel (the three are equal in the files render writes)."""
    paths = {"emit": os.path.join(dir, "emission", "{:05d}_emission.exr".format(i)), "albedo": os.path.join(dir, "a_prime", "{:05d}_a_prime.png".format(i)),
             "kd": os.path.join(dir, "diffuse", "{:05d}_kd.png".format(i)), "rough": os.path.join(dir, "roughness", "{:05d}_roughness.png".format(i))}
    out = {"emit": _rgb3(_read_exr(paths["emit"]), paths["emit"]).astype(np.float32, copy=False), "albedo": _read_png(paths["albedo"]),
           "kd": _read_png(paths["kd"]), "rough": _blue(_read_png(paths["rough"]))}
    return _same_size(out, paths)


def _same_size(maps, paths):
    hw = maps["emit"].shape[:2]
    for k, a in maps.items():
        if a.shape[:2] != hw:
            raise L.IrisError(f"{paths[k]}: {a.shape[0]} x {a.shape[1]} pixels, {paths['emit']} has {hw[0]} x {hw[1]}")
    return maps


def count_views(gt_dir):
    """the reference's view count (metric_brdf.py:25): the .exr files of <gt>/Image that are not hidden"""
    folder = os.path.join(gt_dir, "Image")
    if not os.path.isdir(folder):
        raise L.IrisError(f"{folder}: no such folder (--gt is the split folder of a synthetic scene: Image/, Emit/, albedo/, DiffCol/, Roughness/)")
    return len([f for f in os.listdir(folder) if f[0] != "." and f[-4:] == ".exr"])


def upload(views, device):
    """a list of load_*_view dicts -> the stacked device tensors material_metrics takes (one host stack and one copy per map)"""
    return {k: torch.from_numpy(np.stack([v[k] for v in views])).to(device) for k in GT_KEYS}


class Table:
    """Collects batches of material_metrics results on the device and turns them into the table once: no host synchronisation per batch."""

    def __init__(self, img_hw):
        self.img_hw, self.sums = (int(img_hw[0]), int(img_hw[1])), []

    def add(self, result):
        self.sums.append(result["sums"])

    def finish(self):
        """-> (summary, document): summarize()'s five numbers, and the JSON document {'summary', 'img_hw', 'views', 'sum_names', 'sums' (per view: seven
        integers and S_emit), 'per_view' (the five per-view values; NaN written as null)}"""
        sums = torch.cat(self.sums).cpu().numpy() if self.sums else np.zeros((0, 8), np.int64)
        s_emit = np.ascontiguousarray(sums[:, 7]).view(np.float64)
        per_view = per_view_from_sums(sums, s_emit, *self.img_hw)
        summary = summarize(per_view)
        clean = lambda v: None if v != v else float(v)
        doc = {"summary": {k: clean(summary[k]) for k in SUMMARY_KEYS}, "img_hw": list(self.img_hw), "views": int(sums.shape[0]), "sum_names": list(SUM_NAMES),
               "sums": [[int(x) for x in row[:7]] + [clean(e)] for row, e in zip(sums, s_emit)],
               "per_view": {k: [clean(x) for x in v] for k, v in per_view.items()}}
        return summary, doc
