"""Feature extraction (sfm_extract_features) restated in plain numpy, stage by
stage as include/sfmcore.h defines it and not as the kernels compute it:
restate_pyramid, restate_candidates, restate_refine, restate_orient,
restate_describe and restate (all of them chained), each in fp64 or fp32.
Checked here against things known independently (blobs, edges, constant and
low-contrast images, a rotated patch), against tests/golden/extract_features.npz
(generator: tests/golden/make_golden_extract_features.py; nothing comes from
the reference, which has no extractor) and through the C ABI's argument checks.
tests/test_extract_features_gpu.py compares the device call with it, each
stage from the device's own output of the stage before.  No GPU needed.
"""
import math
import os
import re

import numpy as np

from conftest import GOLDEN, REPO

S = 3                # layers per octave
NBINS = 36           # orientation histogram
BORDER = 5
MAX_MOVES = 5
MAX_RADIUS = 25      # of a blur: sigma above 3.2 is refused
F32, F64 = np.float32, np.float64
TWO_PI = 2.0 * math.pi


# ------------------------------------------------------------------ the pyramid
def max_octaves(H, W):
    n = 0
    while min(H, W) >= 16:
        n, H, W = n + 1, (H + 1) // 2, (W + 1) // 2
    return n


def blur_sigmas(sigma, first_octave):
    """sigma_inc of the S + 3 layers of an octave; entry 0 is None where the layer is a down-sample"""
    sig = [sigma * 2.0 ** (l / float(S)) for l in range(S + 3)]
    inc = [math.sqrt(sigma * sigma - 0.25) if first_octave else None]
    return inc + [math.sqrt(sig[l] * sig[l] - sig[l - 1] * sig[l - 1]) for l in range(1, S + 3)]


def taps(s):
    """the 2 R + 1 fp32 weights of a blur of standard deviation s, R = ceil(4 s)"""
    R = int(math.ceil(4.0 * s))
    i = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * s * s))
    return (g / g.sum()).astype(np.float32)


def reflect101(i, n):
    p = 2 * (n - 1)
    m = np.abs(i) % p
    return np.where(m >= n, p - m, m)


def blur(a, w, dtype):
    """rows, then columns; every sum in ``dtype`` over ascending tap index"""
    R, (H, W) = (len(w) - 1) // 2, a.shape
    wd, a = w.astype(dtype), a.astype(dtype)
    ap = a[:, reflect101(np.arange(-R, W + R), W)]
    t = np.zeros((H, W), dtype)
    for k in range(2 * R + 1):
        t += wd[k] * ap[:, k:k + W]
    tp = t[reflect101(np.arange(-R, H + R), H), :]
    o = np.zeros((H, W), dtype)
    for k in range(2 * R + 1):
        o += wd[k] * tp[k:k + H, :]
    return o


def restate_pyramid(image, n_octaves=None, sigma=1.6, dtype=F64):
    """pyr[o][l]: the S + 3 Gaussian layers of every octave of one uint8 image"""
    H, W = image.shape
    n_octaves = max_octaves(H, W) if not n_octaves else n_octaves
    base = (image.astype(np.float32) / np.float32(255.0)).astype(dtype)
    pyr = []
    for o in range(n_octaves):
        inc = blur_sigmas(sigma, o == 0)
        layers = [blur(base, taps(inc[0]), dtype) if o == 0 else pyr[-1][S][::2, ::2].copy()]
        for l in range(1, S + 3):
            layers.append(blur(layers[-1], taps(inc[l]), dtype))
        pyr.append(layers)
    return pyr


def pyramid_error_bounds(H, W, n_octaves=None, sigma=1.6):
    """bound[o][l] on |device fp32 layer - exact layer|: each pass of a blur adds (taps + 1) 2^-24 -- its weights are
    non-negative and sum to 1 up to their own rounding (the + 1), the pixels are in [0, 1], and each of the `taps` fused
    multiply-adds rounds a partial sum below 2 -- and carries the error of its input on unchanged; a down-sample adds
    nothing.  The fp64 restatement's own error is orders below."""
    n_octaves = max_octaves(H, W) if not n_octaves else n_octaves
    eps, out, carry = 2.0 ** -24, [], 0.0
    for o in range(n_octaves):
        inc = blur_sigmas(sigma, o == 0)
        row = []
        for l in range(S + 3):
            if inc[l] is None:
                e = out[-1][S]
            else:
                e = (row[-1] if l else carry) + 2 * (len(taps(inc[l])) + 1) * eps
            row.append(e)
        out.append(row)
    return out


def flatten_pyramid(pyr):
    return np.concatenate([l.reshape(-1) for layers in pyr for l in layers])


def unflatten_pyramid(flat, H, W, n_octaves=None):
    n_octaves = max_octaves(H, W) if not n_octaves else n_octaves
    pyr, at = [], 0
    for _ in range(n_octaves):
        pyr.append([flat[at + l * H * W:at + (l + 1) * H * W].reshape(H, W) for l in range(S + 3)])
        at += (S + 3) * H * W
        H, W = (H + 1) // 2, (W + 1) // 2
    return pyr


def dog(layers):
    """one subtraction of neighbouring layers, in the layers' own dtype"""
    return [b - a for a, b in zip(layers, layers[1:])]


# ------------------------------------------------------------------ candidates
def restate_candidates(pyr, contrast_threshold=0.04):
    """(n, 4) int32 (octave, layer, row, col), sorted: comparisons only"""
    out = []
    for o, layers in enumerate(pyr):
        D = np.stack(dog(layers))
        thr = D.dtype.type(np.float32(0.5 * contrast_threshold / S))
        H, W = D.shape[1:]
        if H <= 2 * BORDER or W <= 2 * BORDER:
            continue
        for l in range(1, S + 1):
            c = D[l, BORDER:H - BORDER, BORDER:W - BORDER]
            gt, lt = np.ones(c.shape, bool), np.ones(c.shape, bool)
            for dl in (-1, 0, 1):
                for dr in (-1, 0, 1):
                    for dc in (-1, 0, 1):
                        if dl == dr == dc == 0:
                            continue
                        n = D[l + dl, BORDER + dr:H - BORDER + dr, BORDER + dc:W - BORDER + dc]
                        gt &= c > n
                        lt &= c < n
            rr, cc = np.nonzero((np.abs(c) > thr) & (gt | lt))
            out += [(o, l, r + BORDER, q + BORDER) for r, q in zip(rr, cc)]
    return np.array(sorted(out), dtype=np.int32).reshape(-1, 4)


# ------------------------------------------------------------------ refinement
def solve3(dxx, dyy, dss, dxy, dxs, dys, gx, gy, gs, T):
    """X with H X = -g by the adjugate, in this order of operations; None when the determinant is 0 or not finite"""
    c00, c01, c02 = dyy * dss - dys * dys, dxs * dys - dxy * dss, dxy * dys - dxs * dyy
    c11, c12, c22 = dxx * dss - dxs * dxs, dxy * dxs - dxx * dys, dxx * dyy - dxy * dxy
    det = dxx * c00 + dxy * c01 + dxs * c02
    if not np.isfinite(det) or det == 0:
        return None
    inv = T(-1.0) / det
    return ((c00 * gx + c01 * gy + c02 * gs) * inv, (c01 * gx + c11 * gy + c12 * gs) * inv,
            (c02 * gx + c12 * gy + c22 * gs) * inv)


def restate_refine(pyr, cands, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, dtype=F64):
    """per candidate: ok, site (final layer, row, col), off (xc, xr, xs), resp, x, y, scale and the margins of its
    decisions (fp distance to the thresholds: move = min | |offset| - 0.5 |, contrast = | |D^| S - threshold |,
    edge = | tr^2 r - (r + 1)^2 det | / ((r + 1)^2 |det|), det = |det| / tr^2); inf where a decision was not reached"""
    T = dtype
    n = len(cands)
    out = dict(ok=np.zeros(n, bool), site=np.zeros((n, 3), np.int32), off=np.zeros((n, 3), T), resp=np.zeros(n, T),
               x=np.zeros(n, np.float64), y=np.zeros(n, np.float64), scale=np.zeros(n, T),
               m_move=np.full(n, np.inf), m_contrast=np.full(n, np.inf), m_edge=np.full(n, np.inf))
    dogs = [np.stack(dog(layers)).astype(T) for layers in pyr]
    half, quarter, two = T(0.5), T(0.25), T(2.0)
    ct, er = T(contrast_threshold), T(edge_threshold)
    for k, (o, l, r, c) in enumerate(np.asarray(cands).reshape(-1, 4)):
        D = dogs[o]
        H, W = D.shape[1:]
        l, r, c = int(l), int(r), int(c)
        done = False
        for move in range(MAX_MOVES + 1):
            v = D[l, r, c]
            gx, gy, gs = (D[l, r, c + 1] - D[l, r, c - 1]) * half, (D[l, r + 1, c] - D[l, r - 1, c]) * half, \
                (D[l + 1, r, c] - D[l - 1, r, c]) * half
            v2 = v * two
            dxx, dyy, dss = D[l, r, c + 1] + D[l, r, c - 1] - v2, D[l, r + 1, c] + D[l, r - 1, c] - v2, \
                D[l + 1, r, c] + D[l - 1, r, c] - v2
            dxy = (D[l, r + 1, c + 1] - D[l, r + 1, c - 1] - D[l, r - 1, c + 1] + D[l, r - 1, c - 1]) * quarter
            dxs = (D[l + 1, r, c + 1] - D[l + 1, r, c - 1] - D[l - 1, r, c + 1] + D[l - 1, r, c - 1]) * quarter
            dys = (D[l + 1, r + 1, c] - D[l + 1, r - 1, c] - D[l - 1, r + 1, c] + D[l - 1, r - 1, c]) * quarter
            X = solve3(dxx, dyy, dss, dxy, dxs, dys, gx, gy, gs, T)
            if X is None or not all(abs(float(t)) < 1000.0 for t in X):
                break
            out["m_move"][k] = min(out["m_move"][k], min(abs(abs(float(t)) - 0.5) for t in X))
            if all(abs(t) <= half for t in X):
                done = True
                break
            if move == MAX_MOVES:
                break
            c, r, l = c + int(np.floor(X[0] + half)), r + int(np.floor(X[1] + half)), l + int(np.floor(X[2] + half))
            if l < 1 or l > S or c < BORDER or c >= W - BORDER or r < BORDER or r >= H - BORDER:
                break
        if not done:
            continue
        xc, xr, xs = X
        dhat = v + half * (gx * xc + gy * xr + gs * xs)
        resp = abs(dhat)
        out["m_contrast"][k] = abs(float(resp) * S - contrast_threshold)
        if resp * T(S) < ct:
            continue
        tr, det = dxx + dyy, dxx * dyy - dxy * dxy
        lhs, rhs = tr * tr * er, (er + T(1.0)) * (er + T(1.0)) * det
        if float(tr) != 0.0:
            out["m_edge"][k] = abs(float(det)) / float(tr * tr)
        if det <= 0:
            continue
        out["m_edge"][k] = min(out["m_edge"][k], abs(float(lhs) - float(rhs)) / float(rhs))
        if lhs >= rhs:
            continue
        step = float(2 ** int(o))
        out["ok"][k], out["site"][k], out["off"][k], out["resp"][k] = True, (l, r, c), (xc, xr, xs), resp
        out["x"][k], out["y"][k] = (float(c) + float(xc)) * step, (float(r) + float(xr)) * step
        out["scale"][k] = T(sigma) * T(step) * T(np.exp2(T((T(l) + xs) / T(S))))
    return out


# ------------------------------------------------------------------ orientation
def smooth_circular(h, T):
    a, b, c = T(1.0 / 16.0), T(4.0 / 16.0), T(6.0 / 16.0)
    return (np.roll(h, 2) + np.roll(h, -2)) * a + (np.roll(h, 1) + np.roll(h, -1)) * b + h * c


def restate_orient(pyr, octave, site, off, sigma=1.6, dtype=F64):
    """per refined keypoint (octave (n,), site (n, 3), off (n, 3)): a list of (bin, angle) for every local peak of
    the smoothed histogram at or above 0.8 of its maximum, and the peak margin: the smallest
    |h - 0.8 max| / max and |h - neighbour| / max over the bins whose decision it could change"""
    T = dtype
    peaks, margin = [], []
    for o, (l, r, c), (_, _, xs) in zip(octave, site, off):
        G = pyr[o][l]
        H, W = G.shape
        s_oct = T(sigma) * T(np.exp2(T((T(l) + T(xs)) / T(S))))
        rad = int(np.floor(T(4.5) * s_oct + T(0.5)))
        sw = T(1.5) * s_oct
        ii, jj = np.meshgrid(np.arange(-rad, rad + 1), np.arange(-rad, rad + 1), indexing="ij")
        y, x = r + ii, c + jj
        keep = (y > 0) & (y < H - 1) & (x > 0) & (x < W - 1)
        y, x, ii, jj = y[keep], x[keep], ii[keep].astype(T), jj[keep].astype(T)
        dx, dy = (G[y, x + 1] - G[y, x - 1]).astype(T), (G[y + 1, x] - G[y - 1, x]).astype(T)
        mag = np.sqrt(dx * dx + dy * dy)
        ang = np.arctan2(dy, dx)
        ang = np.where(ang < 0, ang + T(TWO_PI), ang)
        w = np.exp(-(ii * ii + jj * jj) / (T(2.0) * sw * sw))
        b = np.floor(ang * T(NBINS / TWO_PI) + T(0.5)).astype(np.int64) % NBINS
        h = np.zeros(NBINS, T)
        np.add.at(h, b, (w * mag).astype(T))
        h = smooth_circular(smooth_circular(h, T), T)
        top = h.max()
        found, m = [], np.inf
        for i in range(NBINS):
            lo, hi = h[(i - 1) % NBINS], h[(i + 1) % NBINS]
            if top > 0:
                near = h[i] >= T(0.8) * top or (h[i] > lo and h[i] > hi)
                if near and h[i] > min(lo, hi):  # a bin that is or could become a peak at the ratio
                    if h[i] > lo and h[i] > hi:
                        m = min(m, abs(float(h[i]) - 0.8 * float(top)) / float(top))
                    if h[i] >= T(0.8) * top:
                        m = min(m, abs(float(h[i] - lo)) / float(top), abs(float(h[i] - hi)) / float(top))
            if top > 0 and h[i] > lo and h[i] > hi and h[i] >= T(0.8) * top:
                bi = T(i) + T(0.5) * (lo - hi) / (lo - T(2.0) * h[i] + hi)
                bi = bi + T(NBINS) if bi < 0 else (bi - T(NBINS) if bi >= T(NBINS) else bi)
                found.append((i, T(bi * T(TWO_PI / NBINS))))
        peaks.append(found)
        margin.append(m)
    return peaks, np.array(margin, dtype=np.float64)


# ------------------------------------------------------------------ descriptors
def describe_raw(pyr, octave, layer, x, y, scale, angle, dtype=F64):
    """(n, 128) 512 v before the rounding to bytes"""
    T = dtype
    out = np.zeros((len(x), 128), T)
    for k in range(len(x)):
        o, G = int(octave[k]), pyr[int(octave[k])][int(layer[k])]
        H, W = G.shape
        step = float(2 ** o)
        xo, yo, s_oct = T(x[k] / step), T(y[k] / step), T(T(scale[k]) / T(step))
        hw = T(3.0) * s_oct
        rad = int(np.floor(hw * T(3.5355339) + T(0.5))) + 1
        cx, cy = int(np.floor(xo + T(0.5))), int(np.floor(yo + T(0.5)))
        ca, sa = T(np.cos(T(angle[k]))), T(np.sin(T(angle[k])))
        py, px = np.meshgrid(np.arange(max(cy - rad, 1), min(cy + rad, H - 2) + 1),
                             np.arange(max(cx - rad, 1), min(cx + rad, W - 2) + 1), indexing="ij")
        py, px = py.reshape(-1), px.reshape(-1)
        dx, dy = px.astype(T) - xo, py.astype(T) - yo
        rx, ry = (ca * dx + sa * dy) / hw, (ca * dy - sa * dx) / hw
        cb, rb = rx + T(1.5), ry + T(1.5)
        keep = (rb > -1) & (rb < 4) & (cb > -1) & (cb < 4)
        py, px, rx, ry, cb, rb = py[keep], px[keep], rx[keep], ry[keep], cb[keep], rb[keep]
        gx, gy = (G[py, px + 1] - G[py, px - 1]).astype(T), (G[py + 1, px] - G[py - 1, px]).astype(T)
        mag = np.sqrt(gx * gx + gy * gy) * np.exp(-(rx * rx + ry * ry) * T(0.125))
        ori = np.arctan2(gy, gx) - T(angle[k])
        ob = ori * T(8.0 / TWO_PI)
        ob = ob - T(8.0) * np.floor(ob * T(0.125))
        ob = np.where(ob >= T(8.0), ob - T(8.0), ob)
        r0, c0, o0 = np.floor(rb), np.floor(cb), np.floor(ob)
        fr, fc, fo = rb - r0, cb - c0, ob - o0
        r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
        h = np.zeros(128, T)
        for dr, wr in ((0, T(1.0) - fr), (1, fr)):
            for dc, wc in ((0, T(1.0) - fc), (1, fc)):
                for do, wo in ((0, T(1.0) - fo), (1, fo)):
                    rr, cc, oo = r0 + dr, c0 + dc, (o0 + do) % 8
                    ok = (rr >= 0) & (rr < 4) & (cc >= 0) & (cc < 4)
                    np.add.at(h, ((rr * 4 + cc) * 8 + oo)[ok], (mag * wr * wc * wo).astype(T)[ok])
        nrm = np.sqrt((h * h).sum())
        h = np.minimum(h / max(nrm, T(1e-12)), T(0.2))
        nrm = np.sqrt((h * h).sum())
        out[k] = T(512.0) * (h / max(nrm, T(1e-12)))
    return out


def to_bytes(raw):
    return np.minimum(255, np.floor(raw + raw.dtype.type(0.5))).astype(np.uint8)


def restate_describe(pyr, octave, layer, x, y, scale, angle, dtype=F64):
    return to_bytes(describe_raw(pyr, octave, layer, x, y, scale, angle, dtype))


# ------------------------------------------------------------------ the chain
def restate(image, n_octaves=None, max_keypoints=0, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6,
            dtype=F64):
    """every stage chained on one image; a dict with the outputs in key order and the intermediate stages"""
    pyr = restate_pyramid(image, n_octaves, sigma, dtype)
    cands = restate_candidates(pyr, contrast_threshold)
    ref = restate_refine(pyr, cands, contrast_threshold, edge_threshold, sigma, dtype)
    idx = np.nonzero(ref["ok"])[0]
    peaks, m_peak = restate_orient(pyr, cands[idx, 0], ref["site"][idx], ref["off"][idx], sigma, dtype)
    src = np.array([i for i, p in zip(idx, peaks) for _ in p], dtype=np.int64)
    bins = np.array([b for p in peaks for b, _ in p], dtype=np.int32)
    angle = np.array([a for p in peaks for _, a in p], dtype=dtype)
    keep = np.arange(len(src))
    if max_keypoints > 0 and len(src) > max_keypoints:
        order = np.lexsort((keep, -ref["resp"][src].astype(np.float64)))  # response descending, then the key
        keep = np.sort(order[:max_keypoints])
    src, bins, angle = src[keep], bins[keep], angle[keep]
    out = dict(pyr=pyr, cands=cands, refined=ref, peaks=peaks, m_peak=m_peak, src=src, bin=bins, angle=angle,
               octave=cands[src, 0], layer=ref["site"][src, 0], xy=np.stack([ref["x"][src], ref["y"][src]], axis=1),
               scale=ref["scale"][src], response=ref["resp"][src])
    out["desc"] = restate_describe(pyr, out["octave"], out["layer"], out["xy"][:, 0], out["xy"][:, 1], out["scale"],
                                   angle, dtype)
    return out


# ------------------------------------------------------------------ images
def texture(H, W, seed, n_blobs=None):
    """a smooth random texture: a sum of random Gaussian blobs of several scales, as uint8"""
    rng = np.random.default_rng(seed)
    n_blobs = (H * W) // 10 if n_blobs is None else n_blobs
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W))
    for _ in range(n_blobs):
        s = rng.choice([1.5, 2.5, 4.0, 6.5, 10.0])
        cy, cx, a = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(-1, 1)
        r = int(4 * s) + 1
        y0, y1, x0, x1 = max(int(cy) - r, 0), min(int(cy) + r + 1, H), max(int(cx) - r, 0), min(int(cx) + r + 1, W)
        img[y0:y1, x0:x1] += a * np.exp(-((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2) / (2 * s * s))
    img = (img - img.min()) / (img.max() - img.min())
    return np.floor(img * 255.0 + 0.5).astype(np.uint8)


def blob(H, W, cy, cx, s, amplitude=0.8):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.floor(255.0 * (0.1 + amplitude * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))) + 0.5
                    ).astype(np.uint8)


FIXTURE_SHAPES = [(97, 130), (130, 97), (64, 80)]  # H, W
FIXTURE_SEEDS = [101, 102, 103]
CHAIN_SEED, CHAIN_SHAPE, CHAIN_SHIFT = 7, (160, 200), (16, 8)  # the larger texture; the crops are 128 rows x 160 columns


def fixture_images():
    return [texture(H, W, s) for (H, W), s in zip(FIXTURE_SHAPES, FIXTURE_SEEDS)]


def chain_crops():
    """two 160 x 128 (W x H) crops of one texture; the second shows the first's content displaced by (-16, -8)"""
    big = texture(CHAIN_SHAPE[0], CHAIN_SHAPE[1], CHAIN_SEED)
    dx, dy = CHAIN_SHIFT
    return np.ascontiguousarray(big[dy:dy + 128, dx:dx + 160]), np.ascontiguousarray(big[0:128, 0:160])


def fixture():
    return np.load(os.path.join(GOLDEN, "extract_features.npz"))


def budget(images):
    """the ambiguity budget of the fp32 against the fp64 restatement: the largest value differences over keypoints
    accepted by both and, per decision, the largest fp64 margin at which the two runs disagree"""
    val = dict(x=0.0, y=0.0, scale=0.0, response=0.0, angle=0.0)
    dec = dict(move=0.0, contrast=0.0, edge=0.0, peak=0.0)
    for img in images:
        a, b = restate(img, dtype=F64), restate(img, dtype=F32)
        common = {tuple(c): k for k, c in enumerate(a["cands"])}
        for kb, c in enumerate(b["cands"]):
            ka = common.get(tuple(c))
            if ka is None:
                continue
            ra, rb = a["refined"], b["refined"]
            same_site = np.array_equal(ra["site"][ka], rb["site"][kb])
            if ra["ok"][ka] != rb["ok"][kb] or (ra["ok"][ka] and not same_site):
                for name in ("move", "contrast", "edge"):
                    m = ra["m_" + name][ka]
                    if np.isfinite(m) and m == min(ra["m_move"][ka], ra["m_contrast"][ka], ra["m_edge"][ka]):
                        dec[name] = max(dec[name], float(m))
            elif ra["ok"][ka]:
                val["x"] = max(val["x"], abs(ra["x"][ka] - rb["x"][kb]))
                val["y"] = max(val["y"], abs(ra["y"][ka] - rb["y"][kb]))
                val["scale"] = max(val["scale"], abs(float(ra["scale"][ka]) - float(rb["scale"][kb])))
                val["response"] = max(val["response"], abs(float(ra["resp"][ka]) - float(rb["resp"][kb])))
        ia, ib = np.nonzero(a["refined"]["ok"])[0], np.nonzero(b["refined"]["ok"])[0]
        pa = {tuple(a["cands"][i]): (p, m) for i, p, m in zip(ia, a["peaks"], a["m_peak"])}
        for i, p in zip(ib, b["peaks"]):
            if tuple(b["cands"][i]) not in pa:
                continue
            q, m = pa[tuple(b["cands"][i])]
            if [t[0] for t in p] != [t[0] for t in q]:
                dec["peak"] = max(dec["peak"], float(m))
            else:
                for (_, u), (_, v) in zip(p, q):
                    d = abs(float(u) - float(v))
                    val["angle"] = max(val["angle"], min(d, TWO_PI - d))
    return val, dec


def budget_one_pyramid(images):
    """the same budget with both precisions run stage by stage on one fp32 pyramid, its candidates and (for the
    orientations) the fp32 refined list -- what the device tests compare, where no pyramid difference enters"""
    val = dict(x=0.0, y=0.0, scale=0.0, response=0.0, angle=0.0)
    dec = dict(move=0.0, contrast=0.0, edge=0.0, peak=0.0)
    for img in images:
        pyr = restate_pyramid(img, dtype=F32)
        cands = restate_candidates(pyr)
        a, b = restate_refine(pyr, cands, dtype=F64), restate_refine(pyr, cands, dtype=F32)
        same = a["ok"] & b["ok"] & (a["site"] == b["site"]).all(axis=1)
        for k in np.nonzero((a["ok"] != b["ok"]) | (a["ok"] & b["ok"] & ~same))[0]:
            m = {n: a["m_" + n][k] for n in ("move", "contrast", "edge")}
            n = min(m, key=m.get)
            dec[n] = max(dec[n], float(m[n]))
        for n, f in (("x", "x"), ("y", "y"), ("scale", "scale"), ("response", "resp")):
            if same.any():
                val[n] = max(val[n], float(np.abs(a[f].astype(np.float64) - b[f].astype(np.float64))[same].max()))
        idx = np.nonzero(b["ok"])[0]
        pa, ma = restate_orient(pyr, cands[idx, 0], b["site"][idx], b["off"][idx], dtype=F64)
        pb, _ = restate_orient(pyr, cands[idx, 0], b["site"][idx], b["off"][idx], dtype=F32)
        for p, q, m in zip(pa, pb, ma):
            if [t[0] for t in p] != [t[0] for t in q]:
                dec["peak"] = max(dec["peak"], float(m))
                continue
            for (_, u), (_, v) in zip(p, q):
                d = abs(float(u) - float(v))
                val["angle"] = max(val["angle"], min(d, TWO_PI - d))
    return val, dec


def ambiguous(ref, m_peak_by_candidate, dec_tol):
    """per candidate: True when its smallest fp64 margin is below the decision tolerance of that decision"""
    amb = (ref["m_move"] <= dec_tol["move"]) | (ref["m_contrast"] <= dec_tol["contrast"]) | \
          (ref["m_edge"] <= dec_tol["edge"])
    return amb | (m_peak_by_candidate <= dec_tol["peak"])


# ------------------------------------------------------------------ the restatement against known things
def test_constant_and_low_contrast_images_give_nothing():
    for v in (0, 77, 255):
        r = restate(np.full((40, 56), v, np.uint8))
        assert len(r["cands"]) == 0 and len(r["xy"]) == 0 and r["desc"].shape == (0, 128)
    rng = np.random.default_rng(5)
    # noise of +-1 grey level: |D| <= 2 / 255 * (a difference of two averages) stays under 0.5 * 0.04 / 3 = 0.0067
    noise = (128 + rng.integers(-1, 2, (48, 64))).astype(np.uint8)
    r = restate(noise)
    assert len(r["xy"]) == 0
    assert all(np.abs(np.stack(dog(layers))).max() < 0.0067 for layers in r["pyr"])


def test_a_blob_gives_one_keypoint_at_its_centre_and_scale():
    for s in (2.5, 4.0, 6.5):
        r = restate(blob(80, 96, 40, 48, s))
        assert len(r["refined"]["ok"]) >= 1 and r["refined"]["ok"].sum() == 1, s
        k = int(np.nonzero(r["refined"]["ok"])[0][0])
        assert abs(r["refined"]["x"][k] - 48.0) <= 1e-6 and abs(r["refined"]["y"][k] - 40.0) <= 1e-6, s
        assert s * 2.0 ** (-1.0 / 3.0) <= r["refined"]["scale"][k] <= s * 2.0 ** (1.0 / 3.0), (s, r["refined"]["scale"][k])


def test_a_step_edge_gives_no_keypoint():
    img = np.full((64, 64), 40, np.uint8)
    img[:, 29:] = 200
    assert len(restate(img)["xy"]) == 0
    yy, xx = np.mgrid[0:64, 0:64]
    slanted = np.where(2 * xx + yy > 90, 210, 30).astype(np.uint8)  # a straight edge across the pixel grid
    assert len(restate(slanted)["xy"]) == 0


def test_a_rotated_patch_gives_the_same_descriptor():
    img = texture(65, 65, 9)
    pyr = restate_pyramid(img, 1)
    rot = np.rot90(img).copy()  # rot[i, j] = img[j, 64 - i]: the point (x, y) goes to (y, 64 - x)
    pyr_r = restate_pyramid(rot, 1)
    x, y, scale, ang = np.array([32.0, 30.0]), np.array([32.0, 35.0]), np.array([2.0, 2.5], F64), np.array([0.3, 4.0])
    d0 = describe_raw(pyr, [0, 0], [1, 2], x, y, scale, ang)
    # a direction (dx, dy) goes to (dy, -dx): the angle turns by -pi/2
    d1 = describe_raw(pyr_r, [0, 0], [1, 2], y, 64.0 - x, scale, ang - math.pi / 2)
    assert np.abs(to_bytes(d0).astype(int) - to_bytes(d1).astype(int)).max() <= 1
    assert to_bytes(d0).max() > 50
    # With the angle held the cells and bins permute.  A displacement (dx, dy) from the keypoint becomes (dy, -dx),
    # so the rotated sample has rx' = (ca dy - sa dx) / hw = ry and ry' = (-ca dx - sa dy) / hw = -rx: column
    # coordinate rx' + 1.5 is the old row coordinate and row coordinate ry' + 1.5 is 3 minus the old column
    # coordinate.  Cell (r, c) goes to (3 - c, r); the gradient direction turns by -pi/2: bin o goes to o - 2.
    # Entry ((row 4) + column) 8 + bin: the last axis is the bin, the middle one the column.
    orig = to_bytes(d0).reshape(2, 4, 4, 8).astype(int)
    held = to_bytes(describe_raw(pyr_r, [0, 0], [1, 2], y, 64.0 - x, scale, ang)).reshape(2, 4, 4, 8).astype(int)
    want = np.zeros_like(orig)
    for r in range(4):
        for c in range(4):
            for o in range(8):
                want[:, 3 - c, r, (o - 2) % 8] = orig[:, r, c, o]
    assert np.abs(held - want).max() <= 1
    # the permutation is pinned: rows and columns exchanged, the bins the other way round, the other turn of the
    # cells or no permutation at all are far off
    wrong = [want.transpose(0, 2, 1, 3), want[..., ::-1], np.roll(want, 4, axis=3), want[:, ::-1, ::-1, :], orig]
    assert all(np.abs(held - w).max() > 50 for w in wrong)


def test_pyramid_layout_and_bounds():
    assert [max_octaves(*s) for s in ((16, 16), (15, 40), (31, 31), (32, 32), (97, 130), (1200, 1600))] == \
        [1, 0, 2, 2, 3, 7]
    img = texture(33, 47, 3)
    p64, p32 = restate_pyramid(img), restate_pyramid(img, dtype=F32)
    assert [l.shape for l in p64[1]] == [(17, 24)] * 6 and len(p64) == 2
    assert np.array_equal(p64[1][0], p64[0][S][::2, ::2])
    bounds = pyramid_error_bounds(33, 47)
    for o in range(2):
        for l in range(S + 3):
            assert np.abs(p64[o][l] - p32[o][l]).max() <= bounds[o][l]
            assert 0.0 <= p64[o][l].min() and p64[o][l].max() <= 1.0 + 1e-6
    flat = flatten_pyramid(p32)
    back = unflatten_pyramid(flat, 33, 47)
    assert all(np.array_equal(a, b) for la, lb in zip(back, p32) for a, b in zip(la, lb))
    assert len(taps(blur_sigmas(1.6, True)[0])) == 15 and len(taps(blur_sigmas(1.6, True)[5])) == 27
    assert abs(float(taps(1.2262).astype(np.float64).sum()) - 1.0) < 1e-6


# ------------------------------------------------------------------ the fixture and the budget
def test_restatement_matches_the_fixture():
    fx = fixture()
    for k, img in enumerate(fixture_images()):
        assert np.array_equal(fx[f"img{k}"], img)
        r = restate(img)
        assert np.array_equal(fx[f"img{k}_cands"], r["cands"])
        assert np.array_equal(fx[f"img{k}_desc"], r["desc"])
        for n in ("xy", "scale", "response", "angle"):
            assert np.allclose(fx[f"img{k}_{n}"], r[n], rtol=0, atol=1e-9), n
        assert len(r["xy"]) >= 10
    assert os.path.getsize(os.path.join(GOLDEN, "extract_features.npz")) < 200_000


def test_ambiguity_budget_is_the_fixtures_and_few_candidates_are_ambiguous():
    fx = fixture()
    images = fixture_images()
    val, dec = budget(images)
    for n, v in val.items():
        assert fx["budget_" + n] == v, n
    for n, v in dec.items():
        assert fx["budget_dec_" + n] == v, n
    val1, dec1 = budget_one_pyramid(images)
    for n, v in val1.items():
        assert fx["budget1_" + n] == v and v <= val[n], n  # never looser than the chained budget the issue names
    for n, v in dec1.items():
        assert fx["budget1_dec_" + n] == v and v <= dec[n], n
    tol = {n: 4.0 * v for n, v in dec.items()}
    for img in images:
        r = restate(img)
        m_peak = np.full(len(r["cands"]), np.inf)
        m_peak[np.nonzero(r["refined"]["ok"])[0]] = r["m_peak"]
        amb = ambiguous(r["refined"], m_peak, tol)
        assert amb.sum() <= 0.1 * len(r["cands"]), (amb.sum(), len(r["cands"]))


def test_chain_crops_match_in_the_restatement():
    """the fp64 restatement on the two crops: nearest neighbours at ratio 0.8 with the cross-check all lie within a
    pixel of the displacement, and there are at least 30 (the count the GPU test halves)"""
    import test_match_descriptors as md
    a, b = chain_crops()
    ra, rb = restate(a), restate(b)
    desc, st = md.pack([ra["desc"], rb["desc"]])
    m = md.restate(desc, st, [(0, 1)])
    d = rb["xy"][m["b"]] - ra["xy"][m["a"]]
    assert np.abs(d - np.array(CHAIN_SHIFT, dtype=np.float64)).max() <= 1.0
    assert len(m["a"]) == int(fixture()["chain_matches"]) >= 30


# ------------------------------------------------------------------ header, bindings, arguments
ARGS = ["const uint8_t *images", "int32_t n_images", "int32_t H", "int32_t W", "int32_t n_octaves",
        "int32_t max_keypoints", "double contrast_threshold", "double edge_threshold", "double sigma",
        "int64_t capacity", "int64_t *kp_start", "double *xy", "float *scale", "float *angle", "float *response",
        "uint8_t *desc", "int32_t *kp_site", "float *pyramid", "int64_t cand_capacity", "int64_t *cand_start",
        "int32_t *cand", "uint8_t *ref_ok", "int32_t *ref_site", "float *ref_val", "int device"]


def test_header_declares_the_entry_point():
    txt = open(os.path.join(REPO, "include", "sfmcore.h")).read()
    m = re.search(r"\bint\s+sfm_extract_features\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/sfmcore.h does not declare sfm_extract_features"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ARGS
    assert "from which every output follows" in txt[txt.index("Feature extraction"):m.start()]
    import _sfmcore
    assert hasattr(_sfmcore._lib, "sfm_extract_features")
    assert len(dict((n, a) for n, _, a in _sfmcore.SIGNATURES)["sfm_extract_features"]) == len(ARGS)
    import sfm_io
    import sfm_multiview
    assert sfm_multiview.extract_features is sfm_io.extract_features


def raw_call(core, images, H=None, W=None, n_octaves=0, max_keypoints=0, ct=0.04, et=10.0, sigma=1.6, capacity=32,
             null=()):
    """the C entry point with sentinel-filled outputs; returns (rc, outputs)"""
    images = np.ascontiguousarray(images, dtype=np.uint8)
    n = len(images)
    rows = max(n, 1) * max(capacity, 1)
    outs = dict(kp_start=np.full(n + 1, -7, np.int64), xy=np.full((rows, 2), -7.0),
                scale=np.full(rows, -7, np.float32), angle=np.full(rows, -7, np.float32),
                response=np.full(rows, -7, np.float32), desc=np.full((rows, 128), 249, np.uint8))
    P = core._p
    types = dict(kp_start=core._i64, xy=core._d, scale=core._f32, angle=core._f32, response=core._f32, desc=core._u8)
    ptr = {k: (None if k in null else P(v, types[k])) for k, v in outs.items()}
    rc = core._lib.sfm_extract_features(None if "images" in null else P(images, core._u8), n,
                                        images.shape[1] if H is None else H, images.shape[2] if W is None else W,
                                        n_octaves, max_keypoints, ct, et, sigma, capacity, ptr["kp_start"], ptr["xy"],
                                        ptr["scale"], ptr["angle"], ptr["response"], ptr["desc"], None, None, 0, None,
                                        None, None, None, None, 0)
    return rc, outs


def untouched(outs):
    return all((v == (249 if k == "desc" else -7)).all() for k, v in outs.items())


def test_arguments_are_refused_before_a_device_is_looked_for():
    """each SFM_ERR_ARG case through the C ABI: -1 and no output touched (no GPU: the checks come first)"""
    import _sfmcore as core
    imgs = np.zeros((2, 32, 48), np.uint8)
    nan, inf = float("nan"), float("inf")
    cases = {"null_images": dict(null=("images",)), "null_kp_start": dict(null=("kp_start",)),
             "null_xy": dict(null=("xy",)), "null_scale": dict(null=("scale",)), "null_angle": dict(null=("angle",)),
             "null_response": dict(null=("response",)), "null_desc": dict(null=("desc",)),
             "H_15": dict(H=15), "W_15": dict(W=15), "H_0": dict(H=0), "W_negative": dict(W=-3),
             "octaves_negative": dict(n_octaves=-1), "octaves_above": dict(n_octaves=3),  # 32 x 48 allows 2
             "contrast_0": dict(ct=0.0), "contrast_negative": dict(ct=-0.04), "contrast_nan": dict(ct=nan),
             "contrast_inf": dict(ct=inf), "edge_0": dict(et=0.0), "edge_nan": dict(et=nan), "edge_inf": dict(et=inf),
             "sigma_0": dict(sigma=0.0), "sigma_negative": dict(sigma=-1.6), "sigma_nan": dict(sigma=nan),
             "sigma_inf": dict(sigma=inf), "sigma_below_input_blur": dict(sigma=0.5), "sigma_large": dict(sigma=3.3),
             "max_keypoints_negative": dict(max_keypoints=-1), "capacity_negative": dict(capacity=-1),
             "capacity_below_cap": dict(max_keypoints=33, capacity=32)}
    for name, change in cases.items():
        rc, outs = raw_call(core, imgs, **change)
        assert rc == -1, name
        assert untouched(outs), name
        assert core._lib.sfm_last_error().startswith(b"argument:"), name
    # what the arguments allow goes on to look for a device
    for change in (dict(n_octaves=2), dict(max_keypoints=32, capacity=32), dict(sigma=3.2)):
        rc, _ = raw_call(core, imgs, **change)
        assert rc == 0 or not core._lib.sfm_last_error().startswith(b"argument:")
    with np.testing.assert_raises(core.SfmCoreError):
        core.extract_features(imgs, sigma=-1.0)


def test_no_images_need_no_device():
    import _sfmcore as core
    rc, outs = raw_call(core, np.zeros((0, 32, 48), np.uint8), null=("images", "xy", "scale", "angle", "response", "desc"))
    assert rc == 0 and outs["kp_start"].tolist() == [0]
    out = core.extract_features(np.zeros((0, 32, 48), np.uint8), want_diagnostics=True)
    assert out["kp_start"].tolist() == [0] and out["xy"].shape == (0, 2) and out["desc"].shape == (0, 128)
    from sfm_io import extract_features
    kps, descs, scale, angle, response = extract_features([])
    assert kps == [] and descs == [] and scale == [] and angle == [] and response == []


def test_python_layer_refuses_bad_inputs():
    from sfm_io import extract_features
    a = np.zeros((32, 48), np.uint8)
    bad = [dict(images=[a, np.zeros((32, 40), np.uint8)]), dict(images=[a.astype(np.float32)]),
           dict(images=[np.zeros((32, 48, 3), np.uint8)]), dict(images=[np.zeros((15, 48), np.uint8)]),
           dict(images=[a], n_octaves=3), dict(images=[a], n_octaves=0), dict(images=[a], max_keypoints=-1),
           dict(images=[a], contrast_threshold=0.0), dict(images=[a], edge_threshold=float("nan")),
           dict(images=[a], sigma=0.4), dict(images=[a], capacity=0), dict(images=[a], max_keypoints=9, capacity=8), dict(images=np.zeros((2, 3, 32, 48), np.uint8))]
    for kw in bad:
        with np.testing.assert_raises(ValueError) as e:
            extract_features(**kw)
        assert "extract_features" in str(e.exception)
