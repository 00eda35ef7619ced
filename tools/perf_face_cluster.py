"""Times the face-clustering sweeps on one GPU: the core-distance sweep and the Boruvka rounds of fe_mreach_mst at d = 512.

    python tools/perf_face_cluster.py [--sizes 10000,50000,100000] [--sklearn 10000]

Per size: core-distance call, whole MST call, rounds, time per Boruvka round (the MST call minus the core call, over the rounds),
the sweep rate in TFLOP/s (2 n^2 d per sweep) beside the 157 TFLOP/s fp32 matrix peak, and the host time of hdbscan_labels.
--sklearn N also times sklearn.cluster.HDBSCAN (NOT the `hdbscan` package or cuML) on the CPU threads of this host, for scale.
Data: planted identities of 20 faces (centre + 0.035 N(0,1)), shuffled, like tests/test_face_cluster_gpu.py."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK = 157.0


def make(n, d=512, per=20, seed=1):
    rng = np.random.default_rng(seed)
    k = (n + per - 1) // per
    centres = rng.standard_normal((k, d)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = np.repeat(centres, per, axis=0)[:n] + np.float32(0.035) * rng.standard_normal((n, d), dtype=np.float32)
    x *= rng.uniform(5.0, 30.0, (n, 1)).astype(np.float32)
    return np.ascontiguousarray(x[rng.permutation(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000,100000")
    ap.add_argument("--sklearn", type=int, default=0)
    ap.add_argument("--k", type=int, default=2)
    a = ap.parse_args()
    from facet_amd import Engine
    from facet_amd.face_cluster import hdbscan_labels
    eng = Engine(0, arena_bytes=1 << 30)
    eng.core_distances(make(2000), a.k)                      # warm-up: module load, LDS attribute
    print(f"{'n':>8} {'core ms':>10} {'core TF/s':>10} {'mst ms':>10} {'rounds':>6} {'ms/round':>10} {'round TF/s':>10} {'of peak':>8} {'labels s':>9} {'clusters':>8}")
    for n in (int(v) for v in a.sizes.split(",")):
        x = make(n)
        import torch
        t = torch.from_numpy(x).cuda()
        dev = (t.data_ptr(), n, 512)
        flop = 2.0 * n * n * 512
        t0 = time.perf_counter(); eng.core_distances(dev, a.k); t1 = time.perf_counter()
        eu, ev, ew, core, rounds = eng.mreach_mst(dev, a.k); t2 = time.perf_counter()
        labels = hdbscan_labels(n, eu, ev, ew, 2, float(np.sqrt(0.3))); t3 = time.perf_counter()
        core_ms, mst_ms = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        per_round = (mst_ms - core_ms) / rounds
        print(f"{n:8d} {core_ms:10.1f} {flop / (core_ms * 1e-3) / 1e12:10.1f} {mst_ms:10.1f} {rounds:6d} {per_round:10.1f} "
              f"{flop / (per_round * 1e-3) / 1e12:10.1f} {flop / (per_round * 1e-3) / 1e12 / PEAK:8.2f} {t3 - t2:9.2f} {labels.max() + 1:8d}", flush=True)
        del t
    if a.sklearn:
        from sklearn.cluster import HDBSCAN
        x = make(a.sklearn)
        xn = x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-10)
        t0 = time.perf_counter()
        lab = HDBSCAN(min_cluster_size=2, min_samples=a.k, metric="euclidean", cluster_selection_epsilon=float(np.sqrt(0.3)), n_jobs=16).fit(xn).labels_
        print(f"sklearn.cluster.HDBSCAN (not the hdbscan package, not cuML), n = {a.sklearn}, 16 CPU threads: {time.perf_counter() - t0:.1f} s, "
              f"{lab.max() + 1} clusters", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
