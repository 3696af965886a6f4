"""Records tests/golden/tsne/{a,b}.npz from scikit-learn's exact t-SNE (sklearn.manifold._t_sne, 1.7.2 when these were
written): the joint probabilities, the objective and its gradient at the initial embedding and, for case B, the final
objective and trustworthiness of a full run.  scikit-learn is needed by this script alone: the tests read the files.

    python tests/golden/make_golden_tsne.py
"""
import os
import sys

import numpy as np
from scipy.spatial.distance import squareform
from sklearn.manifold import TSNE, _t_sne, trustworthiness
from sklearn.metrics import pairwise_distances

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tsne_reference as R      # noqa: E402

# name -> (seed of the inputs, N, D, clusters, perplexity)
CASES = {"a": (11, 67, 8, 3, 10.0), "b": (12, 257, 20, 10, 30.0)}
ROWS_B = (0, 1, 37, 100, 128, 200, 255, 256)


def record(name):
    seed, N, D, C, perplexity = CASES[name]
    X, labels = R.clustered(seed, N, D, C)
    Y0 = R.default_init(N, 123)
    dist = pairwise_distances(X, metric="euclidean", squared=True)      # as TSNE._fit does for method="exact"
    P = _t_sne._joint_probabilities(dist, perplexity, 0)
    full = squareform(P)
    out = {"X": X, "labels": labels, "Y0": Y0, "perplexity": np.float64(perplexity), "P_rowsum": full.sum(1)}
    if name == "a":
        out["P_condensed"], out["P_full"] = P, full
    else:
        out["P_rows_index"], out["P_rows"] = np.array(ROWS_B), full[list(ROWS_B)]
    for ex in (1, 12):
        kl, grad = _t_sne._kl_divergence(Y0.astype(np.float64).ravel(), P * float(ex), 1.0, N, 2)
        out[f"kl_ex{ex}"], out[f"grad_ex{ex}"] = np.float64(kl), grad.reshape(N, 2)
    if name == "b":
        ts = TSNE(n_components=2, method="exact", init=Y0, perplexity=perplexity, max_iter=1000, learning_rate="auto",
                  n_iter_without_progress=10 ** 6, min_grad_norm=0, random_state=123)
        Y = ts.fit_transform(X)
        out["final_kl"] = np.float64(ts.kl_divergence_)
        out["final_trustworthiness"] = np.float64(trustworthiness(X, Y, n_neighbors=5))
        out["final_n_iter"] = np.int64(ts.n_iter_)
    os.makedirs(os.path.join(HERE, "tsne"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "tsne", name + ".npz"), **out)
    return out


if __name__ == "__main__":
    for case in CASES:
        got = record(case)
        print(case, {k: (v.shape if v.ndim else v.item()) for k, v in got.items()})
