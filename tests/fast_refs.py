"""Vectorised restatements of descriptor matching, guided matching, vocabulary
training and tf-idf retrieval, and the large scenes they exist for: more pairs
than one grid holds (the kernels' pair stride), more descriptor rows than one
pseudo-image (2^20) and more images than 64 KB of LDS accumulators.  The plain
restatements of tests/test_match_descriptors.py, tests/test_match_guided.py and
tests/test_retrieval.py remain the definition; what is here is trusted only
because tests/test_fast_refs.py finds it equal to them, element for element, on
the committed fixture scenes and on samples cut out of the large scenes.  The
GPU tests compare the device with these at the sizes the plain ones cannot
reach in seconds.  No GPU needed; nothing here is collected as a test.
"""
import functools
import math

import numpy as np

INT32_MAX = 2 ** 31 - 1
BIG = np.iinfo(np.int64).max
EXACT = 2 ** 53  # integers below it are exact in fp64, and so are their sums and products below it


# ------------------------------------------------------------------ matching
def gate_batch(F, xa, xb, gate):
    """test_match_guided.gate_matrix for g pairs at once: F (g, 9), xa (g, n, 2), xb (g, m, 2) -> (g, n, m) bool;
    the same fp64 operations in the same order, one numpy operation each"""
    f = [F[:, k][:, None, None] for k in range(9)]
    x, y = xa[:, :, 0][:, :, None], xa[:, :, 1][:, :, None]
    u, v = xb[:, :, 0][:, None, :], xb[:, :, 1][:, None, :]
    with np.errstate(all="ignore"):
        l0 = (f[0] * x + f[1] * y) + f[2]
        l1 = (f[3] * x + f[4] * y) + f[5]
        l2 = (f[6] * x + f[7] * y) + f[8]
        m0 = (f[0] * u + f[3] * v) + f[6]
        m1 = (f[1] * u + f[4] * v) + f[7]
        e = (u * l0 + v * l1) + l2
        den = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1)
        thr2 = np.float64(gate) * np.float64(gate)
        return (den > 0.0) & (e * e < thr2 * den)


def first_two_batch(D, G=None):
    """(nn, d1, d2), each (g, n) int32, of the (dsq, index) order of the columns of every row of the int64
    distances D (g, n, m), over the columns that G admits: the order as the one integer dsq * m + index"""
    g, n, m = D.shape
    nn = np.full((g, n), -1, np.int32)
    d1, d2 = np.full((g, n), INT32_MAX, np.int32), np.full((g, n), INT32_MAX, np.int32)
    if g == 0 or n == 0 or m == 0:
        return nn, d1, d2
    key = D * m + np.arange(m, dtype=np.int64)  # dsq < 2^25 and m <= 2^20: far below BIG
    if G is not None:
        key = np.where(G, key, BIG)
    k1 = key.argmin(axis=2)[..., None]
    v1 = np.take_along_axis(key, k1, 2)[..., 0]
    has = v1 != BIG
    nn[has], d1[has] = k1[..., 0][has], (v1 // m)[has]
    if m >= 2:
        np.put_along_axis(key, k1, BIG, 2)
        v2 = key.min(axis=2)
        has = v2 != BIG
        d2[has] = (v2 // m)[has]
    return nn, d1, d2


def match_neighbours(desc, img_start, pairs, xy=None, F=None, gate=None, max_cells=1 << 22):
    """What precedes the tests: nn, d1, d2 (and n_cand with a gate) per row and nn_rev per column, pair-major,
    with the pairs batched by equal (N_i, N_j) and the distances in int64.  xy, F and gate are the guided call's."""
    desc = np.asarray(desc).astype(np.int64)
    st = np.asarray(img_start, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    gated = gate is not None
    if gated:
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        F = np.asarray(F, dtype=np.float64).reshape(-1, 9)
    n = np.diff(st)
    ni, nj = n[pairs[:, 0]], n[pairs[:, 1]]
    row_off = np.concatenate([[0], np.cumsum(ni)]).astype(np.int64)
    col_off = np.concatenate([[0], np.cumsum(nj)]).astype(np.int64)
    out = dict(nn=np.full(row_off[-1], -1, np.int32), d1=np.full(row_off[-1], INT32_MAX, np.int32),
               d2=np.full(row_off[-1], INT32_MAX, np.int32), nn_rev=np.full(col_off[-1], -1, np.int32))
    if gated:
        out["n_cand"] = np.zeros(row_off[-1], np.int32)
    shapes, group = np.unique(np.stack([ni, nj], axis=1), axis=0, return_inverse=True) if len(pairs) else ([], [])
    group = np.asarray(group).reshape(-1)
    for s, (a, b) in enumerate(shapes):
        members = np.flatnonzero(group == s)
        step = max(1, max_cells // max(int(a) * int(b), 1))
        for lo in range(0, len(members), step):
            idx = members[lo:lo + step]
            rows = st[pairs[idx, 0]][:, None] + np.arange(a)
            cols = st[pairs[idx, 1]][:, None] + np.arange(b)
            A, B = desc[rows], desc[cols]
            D = (A * A).sum(axis=2)[:, :, None] + (B * B).sum(axis=2)[:, None, :] - 2 * np.matmul(A, B.transpose(0, 2, 1))
            G = gate_batch(F[idx], xy[rows], xy[cols], gate) if gated else None
            fwd = first_two_batch(D, G)
            rev = first_two_batch(D.transpose(0, 2, 1), None if G is None else G.transpose(0, 2, 1))[0]
            at = (row_off[idx][:, None] + np.arange(a)).reshape(-1)
            for k, v in zip(("nn", "d1", "d2"), fwd):
                out[k][at] = v.reshape(-1)
            out["nn_rev"][(col_off[idx][:, None] + np.arange(b)).reshape(-1)] = rev.reshape(-1)
            if gated:
                out["n_cand"][at] = G.sum(axis=2).reshape(-1)
    out.update(row_off=row_off, col_off=col_off)
    return out


def match_accept(nb, ratio=0.8, max_dsq=INT32_MAX, cross_check=True):
    """the tests of include/sfmcore.h on match_neighbours' result: the outputs of sfm_match_descriptors (of the
    guided call when nb holds n_cand) as a dict of numpy arrays"""
    row_off, col_off = nb["row_off"], nb["col_off"]
    P = len(row_off) - 1
    nn, d1, d2 = nb["nn"], nb["d1"], nb["d2"]
    pair = np.repeat(np.arange(P), np.diff(row_off))
    a = np.arange(len(nn)) - row_off[pair]
    r2 = np.float64(ratio) * np.float64(ratio)
    ok = (nn >= 0) & (d1 <= max_dsq)
    ok &= (d2 == INT32_MAX) | (d1.astype(np.float64) < r2 * d2.astype(np.float64))
    if cross_check and len(nb["nn_rev"]):
        back = nb["nn_rev"][np.minimum(col_off[pair] + np.maximum(nn, 0), len(nb["nn_rev"]) - 1)]
        ok &= back == a  # where nn is -1 the row is refused already
    sel = np.flatnonzero(ok)
    res = {k: nb[k] for k in ("nn", "d1", "d2", "nn_rev", "n_cand") if k in nb}
    res.update(a=a[sel].astype(np.int32), b=nn[sel], dsq=d1[sel])
    res["match_start"] = np.concatenate([[0], np.cumsum(np.bincount(pair[sel], minlength=P))]).astype(np.int64)
    return res


def match(desc, img_start, pairs, ratio=0.8, max_dsq=INT32_MAX, cross_check=True):
    """test_match_descriptors.restate, vectorised"""
    return match_accept(match_neighbours(desc, img_start, pairs), ratio, max_dsq, cross_check)


def match_guided(desc, xy, img_start, pairs, F, gate, ratio=0.8, max_dsq=INT32_MAX, cross_check=True):
    """test_match_guided.restate_guided, vectorised"""
    return match_accept(match_neighbours(desc, img_start, pairs, xy, F, gate), ratio, max_dsq, cross_check)


# ------------------------------------------------------------------ assignment and training
def assign(desc, centres, chunk=1 << 16):
    """(word, count, inertia) of the descriptors against the centres in row chunks: the distances as an fp64 BLAS
    product of integer-valued arrays, exact because every value stays below 2^53; the first minimum wins a tie"""
    dim = desc.shape[1]
    assert 4 * dim * 255 * 255 < EXACT  # |a|^2 + |c|^2 + 2 a.c, whichever way it is summed
    c = np.asarray(centres).astype(np.float64)
    nc = (c * c).sum(axis=1)
    word = np.zeros(len(desc), dtype=np.int64)
    total = 0
    for r0 in range(0, len(desc), chunk):
        a = desc[r0:r0 + chunk].astype(np.float64)
        D = (a * a).sum(axis=1)[:, None] + nc[None, :] - 2.0 * (a @ c.T)
        w = np.argmin(D, axis=1)
        word[r0:r0 + chunk] = w
        total += int(D[np.arange(len(a)), w].astype(np.int64).sum())
    return word, np.bincount(word, minlength=len(c)).astype(np.int64), total


def train(desc, centres0, max_iterations, chunk=1 << 16):
    """test_retrieval.restate_train with assign() and the members' byte sums as an fp64 product per row chunk;
    the same integer centre update and the same early stop"""
    desc = np.asarray(desc, dtype=np.uint8)
    centres = np.array(centres0, dtype=np.uint8)
    n_words, dim = centres.shape
    assert 255 * len(desc) < EXACT  # a byte sum over every row
    word, count, total = assign(desc, centres, chunk)
    inertia, T = [total], 0
    while T < max_iterations:
        sums = np.zeros((n_words, dim), dtype=np.float64)
        for r0 in range(0, len(desc), chunk):
            w = word[r0:r0 + chunk]
            member = np.zeros((len(w), n_words), dtype=np.float64)
            member[np.arange(len(w)), w] = 1.0
            sums += member.T @ desc[r0:r0 + chunk].astype(np.float64)
        s, new = sums.astype(np.int64), centres.copy()
        full = np.nonzero(count)[0]
        new[full] = (2 * s[full] + count[full, None]) // (2 * count[full, None])
        T += 1
        changed = not np.array_equal(new, centres)
        centres = new
        word, count, total = assign(desc, centres, chunk)
        inertia.append(total)
        if not changed:
            break
    return dict(centres=centres, word=word.astype(np.int32), count=count, inertia=np.array(inertia, dtype=np.int64),
                iterations=np.int32(T))


# ------------------------------------------------------------------ retrieval
def select(word, img_start, n_words, top_k, block=512):
    """test_retrieval.restate_select with dots in row blocks by fp64 BLAS (exact below 2^53), the score by the same
    five IEEE operations (two roots, their product, the conversion of dot and the division) and top_k rounds of
    the first maximum: score descending, then index ascending"""
    word, st = np.asarray(word, dtype=np.int64), np.asarray(img_start, dtype=np.int64)
    n = len(st) - 1
    image = np.repeat(np.arange(n), np.diff(st))
    h = np.bincount(image * n_words + word, minlength=n * n_words).reshape(n, n_words).astype(np.int64)
    df = (h > 0).sum(axis=0)
    q = np.array([0] + [math.floor(256.0 * math.log(n / d) + 0.5) for d in range(1, n + 1)], dtype=np.int64)
    v = h * q[df][None, :]
    norm2 = (v * v).sum(axis=1)
    assert int(np.abs(v).max(initial=0)) ** 2 * n_words < EXACT  # a dot product, whichever way it is summed
    vf, root = v.astype(np.float64), np.sqrt(norm2.astype(np.float64))
    neighbour = np.full((n, top_k), -1, dtype=np.int32)
    score = np.zeros((n, top_k), dtype=np.float64)
    dot = np.zeros((n, top_k), dtype=np.int64)
    for r0 in range(0, n, block):
        d = vf[r0:r0 + block] @ vf.T
        r = np.arange(len(d))
        d[r, r0 + r] = 0.0  # an image is no neighbour of itself
        with np.errstate(all="ignore"):
            s = d / (root[r0:r0 + block, None] * root[None, :])
        s[~(d > 0.0)] = -np.inf
        for k in range(min(top_k, n)):
            j = np.argmax(s, axis=1)  # the first maximum: the smaller index on a tie
            best = s[r, j]
            ok = best > -np.inf
            neighbour[r0:r0 + block, k][ok] = j[ok]
            score[r0:r0 + block, k][ok] = best[ok]
            dot[r0:r0 + block, k][ok] = d[r, j][ok].astype(np.int64)
            s[r, j] = -np.inf
    return dict(neighbour=neighbour, score=score, dot=dot, norm2=norm2.astype(np.int64), df=df.astype(np.int32))


# ------------------------------------------------------------------ the scene of 65,535 + 600 pairs
T, BM = 64, 128                      # the matchers' column tile and row block at dim 64 and 128
WRAP, PLACED = 65535, 600            # gridDim.y's cap; pairs 0 .. 599 and 65,535 .. 66,134 are placed by hand
SHAPES = (0, 1, 17, 65, 130, 2 * BM + 9)  # keypoints of a placed image: up to three column tiles and row blocks
COPIES, FILLERS, BASES = 3, 300, 400
TRANSITIONS = [(a, b) for a in range(len(SHAPES)) for b in range(len(SHAPES))]
GUIDED_GATE = 120.0                  # pixels: two fifths of the scene's (row, column) pairs are admitted


@functools.lru_cache(maxsize=None)
def wrap_scene(dim=64, seed=41):
    """COPIES images of every size in SHAPES and FILLERS images of 1 to 3 keypoints, every descriptor one of BASES
    uniform random base descriptors plus integer noise in [-2, 2], so that images share scene points; 66,135 pairs.
    Pair t < 600 and pair t + 65,535 -- the two pairs of one workgroup -- take their (N_i, N_j) from TRANSITIONS:
    t runs through every ordered pair of sizes on the row side while the column side runs through them at an
    offset that changes every 36 pairs.  The pairs between are random pairs of fillers.  The 130-keypoint image
    of copy 0 holds its descriptor 3 again at 3 + T and 129, the 17-keypoint image of copy 0 holds it in row 5,
    and wrapped pair TIE_PAIR is that pair.  Keypoints are uniform in a 640 x 480 frame and every pair has an F
    of its own (random, rank 2, unit norm; one wrapped pair's holds a NaN).
    Returns dict(desc, xy, img_start, pairs, F, shape (P, 2), tie_pair, nan_pair)."""
    rng = np.random.default_rng(seed + dim)
    base = rng.integers(0, 256, (BASES, dim))
    sizes = [s for s in SHAPES for _ in range(COPIES)] + rng.integers(1, 4, FILLERS).tolist()
    descs = [np.clip(base[rng.permutation(BASES)[:n]] + rng.integers(-2, 3, (n, dim)), 0, 255).astype(np.uint8)
             for n in sizes]
    wide, narrow = descs[COPIES * SHAPES.index(130)], descs[COPIES * SHAPES.index(17)]
    wide[3 + T] = wide[129] = narrow[5] = wide[3]
    P = WRAP + PLACED
    first_filler = COPIES * len(SHAPES)
    i = first_filler + rng.integers(0, FILLERS, P)
    j = first_filler + (i - first_filler + 1 + rng.integers(0, FILLERS - 1, P)) % FILLERS
    pairs = np.stack([i, j], axis=1).astype(np.int32)
    tie_pair = None
    for t in range(PLACED):
        rows, cols = TRANSITIONS[t % 36], TRANSITIONS[(t + 5 * (t // 36)) % 36]
        for p, side, ca, cb in ((t, 0, t % 3, (t // 3) % 3), (t + WRAP, 1, (t // 9) % 3, (t // 27) % 3)):
            a, b = rows[side], cols[side]
            if SHAPES[a] == 17 and SHAPES[b] == 130 and side == 1 and tie_pair is None:
                ca, cb, tie_pair = 0, 0, p
            if a == b and ca == cb:
                cb = (cb + 1) % COPIES
            pairs[p] = (COPIES * a + ca, COPIES * b + cb)
    img_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    xy = rng.random((img_start[-1], 2)) * np.array([640.0, 480.0])
    U, s, Vt = np.linalg.svd(rng.standard_normal((P, 3, 3)))
    s[:, 2] = 0.0
    F = (U * s[:, None, :]) @ Vt
    F /= np.sqrt((F * F).sum(axis=(1, 2)))[:, None, None]
    nan_pair = WRAP + 11
    F[nan_pair, 1, 2] = np.nan
    n = np.diff(img_start)
    return dict(desc=np.concatenate(descs), xy=xy, img_start=img_start, pairs=pairs, F=F, shape=n[pairs],
                tie_pair=tie_pair, nan_pair=nan_pair)


def wrap_limit(dim):
    """max_dsq of the scene: true matches are within 16 dim, two unrelated descriptors are at 10,922 dim on average
    with a deviation of about 9,800 sqrt(dim): the limit refuses most unrelated nearest neighbours, not all"""
    return 9400 * dim


def wrap_sample(scene, seed=3, n_fill=110):
    """indices of about three hundred pairs for the plain restatements: every seventh placed pair with its wrapped
    partner, the tie and the NaN pair, and a seeded choice of the filler pairs between"""
    t = np.arange(0, PLACED, 7)
    fill = np.random.default_rng(seed).choice(np.arange(PLACED, WRAP), n_fill, replace=False)
    return np.unique(np.concatenate([t, t + WRAP, [scene["tie_pair"], scene["nan_pair"]], fill]))


# ------------------------------------------------------------------ the scene of 2^20 + 300 descriptors
TRAIN_ROWS, TRAIN_WORDS, TRAIN_TAIL = 2 ** 20 + 300, 65, 300


@functools.lru_cache(maxsize=None)
def train_scene(seed=47, dim=64):
    """(desc, centres): 2^20 + 300 uniform random descriptors, one block of 2^20 rows and a second of 300, and 65
    uniform random centres, two column tiles"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (TRAIN_ROWS, dim), dtype=np.uint8),
            rng.integers(0, 256, (TRAIN_WORDS, dim), dtype=np.uint8))


def train_sample(desc, head=200):
    """the first 200 rows and the second block's 300"""
    return np.concatenate([desc[:head], desc[-TRAIN_TAIL:]])


# ------------------------------------------------------------------ the retrieval scenes
SP_THREADS = 512
SELECT_SIZES = (513, 6145, 8193, 16384)  # one past SP_THREADS, above 48 KiB of LDS, above 64 KiB, the limit
SELECT_WORDS, SELECT_TOP_K, SELECT_TWIN = 256, 3, 7


@functools.lru_cache(maxsize=None)
def select_scene(n_images, seed=53):
    """(word, img_start): four uniform random words of 256 per image; image n_images // 2 is empty, and the last
    image holds the words of image SELECT_TWIN, so that an index past SP_THREADS is somebody's best neighbour"""
    rng = np.random.default_rng(seed + n_images)
    words = rng.integers(0, SELECT_WORDS, (n_images, 4))
    words[-1] = words[SELECT_TWIN]
    count = np.full(n_images, 4)
    count[n_images // 2] = 0
    keep = np.repeat(count > 0, 4)
    return (words.reshape(-1)[keep].astype(np.int32), np.concatenate([[0], np.cumsum(count)]).astype(np.int64))


def select_sample(word, img_start, head=300):
    """the scene of the first 300 images, the empty one and the last"""
    n = len(img_start) - 1
    images = list(range(head)) + [n // 2, n - 1]
    per = [word[img_start[k]:img_start[k + 1]] for k in images]
    return (np.concatenate(per).astype(np.int32), np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64))
