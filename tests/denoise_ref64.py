"""The denoiser of iris_amd/csrc/iris_denoise.h written from the definition in that header's comment, in NumPy float64: what
tests/test_denoise_reference.py holds both the HIP kernels and the oracle's float32 restatement to.  Shares no code with oracle/.

    guides    n = normal (absent: (0,0,1)), x = position (absent: 0); the guides stored at an invalid pixel are ignored
    w_g(p,q)  = w_n * w_p, 0 for an invalid or out-of-image q
                w_n = (n_p.n_q)^sigma_n for n_p.n_q > 0, else 0;   w_p = exp(-|n_p.(x_q-x_p)| / (sigma_p*|x_q-x_p| + 1e-12))
    variance  7x7 window, w = w_g (centre: 1):  mean = sum w l / sum w,  var = sum w (l - mean)^2 / sum w      (two passes: no cancellation)
    a-trous   pass i, 5x5 B3-spline taps at stride 2^i:  w = h/h(0,0) * w_g * exp(-|l_p-l_q| / (sigma_l*sqrt(gauss3x3(var)_p) + 1e-6)), centre 1
              colour' = sum w c / sum w,  var' = sum w^2 var / (sum w)^2;  gauss3x3 = [1 2 1]x[1 2 1] over the valid in-image pixels, renormalised
    invalid pixels output 0, weigh 0 as taps and are left out of the 3x3 gaussian.

The inputs are the float32 arrays converted exactly; sigmas, the two epsilons and the luminance coefficients enter as the float64 values of their float32
roundings (they are float32 in the kernel: the reference answers "what does this formula give for these numbers", not "for nearby numbers").
Vectorised over tap offsets with shifted arrays."""
import numpy as np

_F = lambda v: np.float64(np.float32(v))
LUM = np.array([_F(0.2126), _F(0.7152), _F(0.0722)])
EPS_P = _F(1e-12)
EPS_L = _F(1e-6)
H1 = np.array([3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0])


def _shift(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx] where that lies in the image (else 0), and the in-image mask"""
    H, W = a.shape[:2]
    b = np.zeros_like(a)
    inb = np.zeros((H, W), bool)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inb[y0:y1, x0:x1] = True
    return b, inb


def _guides(H, W, normal, position, valid):
    v = np.ones((H, W), bool) if valid is None else np.asarray(valid).reshape(H, W) != 0
    n = np.zeros((H, W, 3)); n[..., 2] = 1.0
    x = np.zeros((H, W, 3))
    if normal is not None:
        n[v] = np.asarray(normal, np.float32).reshape(H, W, 3).astype(np.float64)[v]
    if position is not None:
        x[v] = np.asarray(position, np.float32).reshape(H, W, 3).astype(np.float64)[v]
    return n, x, v


def _geo(n, x, v, dy, dx, sigma_n, sigma_p):
    """w_g(p, p + (dy, dx)) for every p (H,W); the value at an invalid p is not used by the callers"""
    nq, inb = _shift(n, dy, dx)
    xq, _ = _shift(x, dy, dx)
    vq, _ = _shift(v, dy, dx)
    nn = np.sum(n * nq, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        wn = np.where(nn > 0, np.power(np.where(nn > 0, nn, 1.0), sigma_n), 0.0)
    d = xq - x
    dist = np.sqrt(np.sum(d * d, -1))
    plane = np.abs(np.sum(n * d, -1))
    wp = np.exp(-plane / (sigma_p * dist + EPS_P))
    return np.where(inb & vq, wn * wp, 0.0)


def geometric_weights(H, W, normal=None, position=None, valid=None, sigma_n=128.0, sigma_p=0.05, radius=3):
    """All w_g(p, q) with p, q valid, q in the image and in the (2*radius+1)^2 window of p, q != p: a flat float64 array (what the scene conditions of
    the tests are asserted on)."""
    n, x, v = _guides(H, W, normal, position, valid)
    out = []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0:
                continue
            vq, inb = _shift(v, dy, dx)
            out.append(_geo(n, x, v, dy, dx, _F(sigma_n), _F(sigma_p))[v & vq & inb])
    return np.concatenate(out)


def denoise(img, normal=None, position=None, valid=None, iterations=5, sigma_l=16.0, sigma_n=128.0, sigma_p=0.05, intermediates=False):
    """img (H,W,3) float32 -> (H,W,3) float64.  With intermediates=True also a dict: "variance" (H,W) as the variance pass leaves it, "colour" and
    "var" lists with the state after every a-trous pass."""
    img = np.asarray(img, np.float32)
    H, W, _ = img.shape
    sigma_l, sigma_n, sigma_p = _F(sigma_l), _F(sigma_n), _F(sigma_p)
    n, x, v = _guides(H, W, normal, position, valid)
    c = np.where(v[..., None], img.astype(np.float64), 0.0)          # what an invalid pixel stores is never read
    lum = lambda a: a @ LUM

    # variance: two passes over the 7x7 window
    l = lum(c)
    offs = [(dy, dx) for dy in range(-3, 4) for dx in range(-3, 4)]
    wgt = {o: (v.astype(np.float64) if o == (0, 0) else _geo(n, x, v, o[0], o[1], sigma_n, sigma_p)) for o in offs}
    ws = sum(wgt.values())
    ws1 = np.where(v, ws, 1.0)
    mean = sum(wgt[o] * _shift(l, *o)[0] for o in offs) / ws1
    var = sum(wgt[o] * (_shift(l, *o)[0] - mean) ** 2 for o in offs) / ws1
    var = np.where(v, var, 0.0)
    inter = {"variance": var.copy(), "colour": [], "var": []}

    vf = v.astype(np.float64)
    for it in range(int(iterations)):
        step = 1 << it
        gw = np.zeros((H, W)); gv = np.zeros((H, W))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = (2.0 if dx == 0 else 1.0) * (2.0 if dy == 0 else 1.0)
                gw += k * _shift(vf, dy, dx)[0]
                gv += k * _shift(var * vf, dy, dx)[0]
        inv_sl = 1.0 / (sigma_l * np.sqrt(gv / np.where(v, gw, 1.0)) + EPS_L)
        lp = lum(c)
        sc = c.copy(); sv = var.copy(); sw = np.ones((H, W))                # centre tap: weight 1
        for j in range(-2, 3):
            for i in range(-2, 3):
                if i == 0 and j == 0:
                    continue
                dy, dx = j * step, i * step
                if abs(dy) >= H or abs(dx) >= W:
                    continue                                               # the tap lies outside the image for every pixel
                h = H1[abs(i)] * H1[abs(j)] / (H1[0] * H1[0])
                cq = _shift(c, dy, dx)[0]
                w = h * _geo(n, x, v, dy, dx, sigma_n, sigma_p) * np.exp(-np.abs(lp - lum(cq)) * inv_sl)
                sc += w[..., None] * cq; sv += w * w * _shift(var, dy, dx)[0]; sw += w
        c = np.where(v[..., None], sc / sw[..., None], 0.0)
        var = np.where(v, sv / (sw * sw), 0.0)
        inter["colour"].append(c.copy()); inter["var"].append(var.copy())
    return (c, inter) if intermediates else c
