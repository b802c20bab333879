"""Generate tests/golden/two_view.npz: the reference's two-view initialisation
(Wrapper_dev.py:156-179) on its own data and on synthetic pairs.

Runs only where make_golden.py runs: it imports the reference from the place
make_golden.py names (make_golden.REF).  Every expected output comes from calling
the reference's own functions (EssentialMatrixFromFundamentalMatrix,
ExtractCameraPose, LinearTriangulation, DisambiguateCameraPose); nothing of
its source is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_two_view.py

Cases (key prefix):
  p3      P3Data pair 1_2, seed 0: F from ransac_p3data.npz, the 14 inliers
          from triangulation.npz.  The counts tie 7/7 between candidates 2
          and 3; the reference's strict '>' selects 2.
  syn0    sfm_synthetic.two_view(seed=0) with its 40 % outliers, F from the
  syn1    reference's EstimateFundamentalMatrix on the first 300 clean pairs
          (seed 1 likewise).  Stored once at N = 1025; the smaller sizes in
          `sizes` are prefixes (the reference triangulates point by point,
          asserted below), each with its own counts / selection / line.  The
          inputs are not stored: the test regenerates them from the seed.
  exact   F = K^-T [t]x R K^-1 exactly for two_view(seed=2)'s camera (E's two
          singular values equal), its first 100 clean pairs.
Per case: F, E, Cset, Rset, X (4, N, 3) -- the four LinearTriangulation
results --, counts (each from DisambiguateCameraPose on that candidate alone),
sel / C / R (DisambiguateCameraPose on all four; X_sel = X[sel]), line (what it
printed), and margin: the smallest |z1|, |z2| over max(1, |X|_inf) of the case.
Every depth is asserted to be at least 1e-6 of that scale from zero, so no
cheirality bit is within rounding of flipping and the tests compare counts
with no point excluded.
"""
import contextlib
import io
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

syn = mg.syn
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)


def disambiguate(ref_d, Cset, Rset, Xset):
    """The reference's DisambiguateCameraPose and the line it prints."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        C, R, X = ref_d.DisambiguateCameraPose(Cset, Rset, Xset)
    return C, R, X, buf.getvalue().rstrip("\n")


def margin(Cset, Rset, X):
    """Smallest distance of a depth from zero, relative to max(1, |X|_inf)."""
    m = np.inf
    for i in range(len(Cset)):
        z1 = X[i][:, 2]
        z2 = ((X[i] - Cset[i]) @ Rset[i].T)[:, 2]
        m = min(m, np.abs(z1).min(), np.abs(z2).min())
    return m / max(1.0, np.abs(X).max())


def select(ref_d, Cset, Rset, X):
    """counts (one reference call per candidate), sel, C, R, line."""
    counts = np.zeros(len(Cset), dtype=np.int64)
    for i in range(len(Cset)):
        line = disambiguate(ref_d, Cset[i:i + 1], Rset[i:i + 1], [X[i]])[3]
        counts[i] = int(re.fullmatch(r"Selected camera pose configuration 0 with (\d+) points in front of both "
                                     r"cameras", line).group(1))
    C, R, Xs, line = disambiguate(ref_d, Cset, Rset, [X[i] for i in range(len(Cset))])
    sel = int(re.match(r"Selected camera pose configuration (\d+) ", line).group(1))
    assert np.array_equal(Xs, X[sel]) and np.array_equal(C, Cset[sel]) and np.array_equal(R, Rset[sel])
    assert counts[sel] == counts.max() and sel == int(np.argmax(counts))
    return counts, sel, C, R, line


def candidates(ref, F, x1, x2):
    K = syn.K_REF
    E = ref.e.EssentialMatrixFromFundamentalMatrix(F, K)
    Cset, Rset = ref.p.ExtractCameraPose(E)
    X = np.stack([ref.t.LinearTriangulation(K, np.zeros(3), np.eye(3), Cset[i], Rset[i], x1, x2) for i in range(4)])
    return E, Cset, Rset, X


def main():
    ref = mg._import_reference()
    import DisambiguateCameraPose as ref_d
    assert os.path.dirname(os.path.abspath(ref_d.__file__)) == mg.REF
    K = syn.K_REF
    out = {"sizes": np.array(SIZES)}
    margins = {}

    def single(name, F, x1, x2, store_x):
        E, Cset, Rset, X = candidates(ref, F, x1, x2)
        counts, sel, C, R, line = select(ref_d, Cset, Rset, X)
        margins[name] = margin(Cset, Rset, X)
        out.update({f"{name}_F": F, f"{name}_E": E, f"{name}_Cset": Cset, f"{name}_Rset": Rset, f"{name}_X": X,
                    f"{name}_counts": counts, f"{name}_sel": np.array(sel), f"{name}_C": C, f"{name}_R": R,
                    f"{name}_line": np.array(line), f"{name}_margin": np.array(margins[name])})
        if store_x:
            out[f"{name}_x1"], out[f"{name}_x2"] = x1, x2
        print(name, len(x1), counts, sel, f"margin {margins[name]:.3g}")

    p3 = np.load(os.path.join(HERE, "ransac_p3data.npz"))
    tri = np.load(os.path.join(HERE, "triangulation.npz"))
    single("p3", p3["s0_1_2_F"], tri["p3_x1"], tri["p3_x2"], True)
    assert list(out["p3_counts"]) == [0, 0, 7, 7] and int(out["p3_sel"]) == 2

    for seed in (0, 1):
        name = f"syn{seed}"
        x1, x2, _, meta = syn.two_view(seed=seed)
        F = ref.f.EstimateFundamentalMatrix(meta["clean1"][:300], meta["clean2"][:300])
        n = max(SIZES)
        E, Cset, Rset, X = candidates(ref, F, x1[:n], x2[:n])
        # the smaller sizes are prefixes: the reference triangulates point by point
        X63 = np.stack([ref.t.LinearTriangulation(K, np.zeros(3), np.eye(3), Cset[i], Rset[i], x1[:63], x2[:63])
                        for i in range(4)])
        assert np.array_equal(X63, X[:, :63])
        rows = [select(ref_d, Cset, Rset, X[:, :s]) for s in SIZES]
        margins[name] = margin(Cset, Rset, X)
        out.update({f"{name}_F": F, f"{name}_E": E, f"{name}_Cset": Cset, f"{name}_Rset": Rset, f"{name}_X": X,
                    f"{name}_counts": np.stack([r[0] for r in rows]), f"{name}_sel": np.array([r[1] for r in rows]),
                    f"{name}_line": np.array([r[4] for r in rows]), f"{name}_margin": np.array(margins[name])})
        for s, r in zip(SIZES, rows):
            print(name, s, r[0], r[1])
        print(name, f"margin {margins[name]:.3g}")

    _, _, _, meta = syn.two_view(seed=2)
    R2, C2 = meta["R2"], meta["C2"]
    t = -R2 @ C2
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    single("exact", Ki.T @ tx @ R2 @ Ki, meta["clean1"][:100], meta["clean2"][:100], True)
    s = np.linalg.svd(out["exact_E"], compute_uv=False)
    assert abs(s[0] - s[1]) <= 1e-12 * s[0] and s[2] <= 1e-12 * s[0], s

    for name, m in margins.items():
        assert m >= 1e-6, (name, m)
    path = os.path.join(HERE, "two_view.npz")
    np.savez_compressed(path, **out)
    print("two_view.npz", os.path.getsize(path), "bytes; smallest margin", min(margins.values()))


if __name__ == "__main__":
    main()
