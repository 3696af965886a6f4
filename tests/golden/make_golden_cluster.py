"""Records tests/golden/cluster/*.npz from scikit-learn (1.7.2 when these were made) on float64 copies of the seeded inputs of
tests/cluster_reference.py.  The GPU machine needs neither this script nor scikit-learn.

    python tests/golden/make_golden_cluster.py

Per shape case i (case<i>.npz), restart by restart with KMeans(init=<the start centres>, n_init=1, tol=0,
algorithm="lloyd", max_iter=m), m in (300, 3): labels (int16), centres (those of m = 3 only where they differ), inertia,
n_iter_; of the best restart at m = 300: silhouette_samples, calinski_harabasz_score, davies_bouldin_score, and against the generating labels i mod C:
adjusted_rand_score, normalized_mutual_info_score, homogeneity_completeness_v_measure.  crafted.npz: the same scores of the
crafted partition (against the labeling i mod 3), and silhouette_samples once more from a matrix of distances taken by
direct differences (metric="precomputed"): scikit-learn's own Euclidean distances go through the Gram product, which
puts the two equal rows of that case sqrt(rounding) apart instead of 0."""
import os
import sys

import numpy as np
from sklearn import metrics as M
from sklearn.cluster import KMeans

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cluster_reference as R  # noqa: E402

OUT = os.path.join(HERE, "cluster")


def scores(X64, labels, classes):
    h, c, _ = M.homogeneity_completeness_v_measure(classes, labels)
    return {"silhouette": M.silhouette_samples(X64, labels), "ch": M.calinski_harabasz_score(X64, labels),
            "db": M.davies_bouldin_score(X64, labels), "ari": M.adjusted_rand_score(classes, labels),
            "nmi": M.normalized_mutual_info_score(classes, labels), "homogeneity": h, "completeness": c}


def main():
    os.makedirs(OUT, exist_ok=True)
    for i, (N, F, C) in enumerate(R.SHAPES):
        X, init = R.case(i)
        X64 = X.astype(np.float64)
        rec = {}
        for m in (300, 3):
            fits = [KMeans(n_clusters=C, init=X64[init[r]], n_init=1, tol=0, algorithm="lloyd", max_iter=m).fit(X64)
                    for r in range(len(init))]
            rec[f"labels_{m}"] = np.stack([f.labels_ for f in fits]).astype(np.int16)
            rec[f"centres_{m}"] = np.stack([f.cluster_centers_ for f in fits])
            rec[f"inertia_{m}"] = np.array([f.inertia_ for f in fits])
            rec[f"n_iter_{m}"] = np.array([f.n_iter_ for f in fits], dtype=np.int16)
        if np.array_equal(rec["centres_3"], rec["centres_300"]):      # (every restart converged within three iterations)
            del rec["centres_3"]
        best = int(np.argmin(rec["inertia_300"]))
        rec["best"] = np.int16(best)
        rec.update(scores(X64, rec["labels_300"][best].astype(np.int64), np.arange(N) % C))
        np.savez_compressed(os.path.join(OUT, f"case{i}.npz"), **rec)
    X, labels, other, _ = R.crafted()
    rec = scores(X.astype(np.float64), labels, other)
    rec["silhouette_direct"] = M.silhouette_samples(R.distances(X), labels, metric="precomputed")
    np.savez_compressed(os.path.join(OUT, "crafted.npz"), **rec)


if __name__ == "__main__":
    main()
