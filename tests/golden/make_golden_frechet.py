"""Records tests/golden/frechet/<case>.npz by running the REFERENCE's calculate_frechet_distance (eval/fid_score.py:203-257:
scipy.linalg.sqrtm of sigma1 . sigma2) on np.mean / np.cov of the seeded features of tests/frechet_reference.py (build
container only; the tests read the files, never the reference).

    python tests/golden/make_golden_frechet.py

Per case: mu1, mu2, the upper triangles of sigma1 and sigma2 (row-major, np.triu_indices), distance, tr_covmean (recovered
from the distance's other terms, which the reference does not return), and, for the small cases, X1 and X2 (float32).  Case
f stores scalars only -- its features are regenerated from the seed -- plus what the float64 restatement's own Jacobi route
gives for it (restated_distance, restated_tr_covmean, restated_sweeps: half a minute of numpy at F = 512), which the host
and the GPU tests read and do not recompute; for case f the tests' Jacobi leg is therefore this script's run of
frechet_reference.distance_jacobi, while its eigh and nuclear-norm routes are computed in the tests.  Each file stays at or
below the 369 060 bytes the t-SNE fixtures are held to.
"""
import importlib.machinery
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import frechet_reference as R      # noqa: E402
import ref_harness                 # noqa: E402

OUT = os.path.join(HERE, "frechet")
LIMIT = 369060


def load_reference():
    ref_harness.install()
    try:
        import PIL  # noqa: F401
    except Exception:      # fid_score.py imports PIL.Image for its file loader, which nothing here calls
        for name in ("PIL", "PIL.Image"):
            m = types.ModuleType(name)
            m.__path__ = []
            m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
            sys.modules[name] = m
        sys.modules["PIL"].Image = sys.modules["PIL.Image"]
    from eval import fid_score
    return fid_score.calculate_frechet_distance


def record(name, calculate):
    X1, X2 = R.features(name)
    (mu1, s1), (mu2, s2) = R.moments(X1), R.moments(X2)
    d2 = float(calculate(mu1, s1, mu2, s2))
    diff = mu1 - mu2
    tr = 0.5 * (diff.dot(diff) + np.trace(s1) + np.trace(s2) - d2)
    iu = np.triu_indices(s1.shape[0])
    out = {"mu1": mu1, "mu2": mu2, "sigma1_triu": s1[iu], "sigma2_triu": s2[iu], "distance": np.float64(d2),
           "tr_covmean": np.float64(tr)}
    if name in R.SMALL:
        out["X1"], out["X2"] = X1, X2
    else:
        out = {k: v for k, v in out.items() if k in ("distance", "tr_covmean")}
        dj, trj, sweeps = R.distance_jacobi(mu1, s1, mu2, s2)
        out.update(restated_distance=np.float64(dj), restated_tr_covmean=np.float64(trj),
                   restated_sweeps=np.array(sweeps, np.int64))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= LIMIT, (name, size)
    print(f"{name}: d^2 = {d2:.12g}, tr covmean = {tr:.12g}, {size} bytes")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    calc = load_reference()
    for case in R.CASES:
        record(case, calc)
