#!/usr/bin/env python3
"""Developer tool: the graph index (anorag_hip.GraphIndex) against the exact FlatIndex and IVF-Flat on one synthetic
corpus, in one process (not part of bench.py): build time split into kNN / prune / image, then per batch size and ef the
ms per batch, queries per second, recall@10 and recall@100 against the exact top-k and rows scored per query; the exact
scan at the same batches and IVFIndex at nprobe 8 and 32 next to it.  --clustered: the corpus of tools/ivf_perf.py
(1024 Gaussian centres, sigma 0.3)."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ano-rag_amd"))
import numpy as np
import torch
from anorag_hip import FlatIndex, GraphIndex, IVFIndex, METRIC_IP

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--clustered", action="store_true")
ap.add_argument("--R", type=int, default=64)
ap.add_argument("--build-degree", type=int, default=128)
ap.add_argument("--ef", default="64,100,200")
ap.add_argument("--batches", default="1,64,256")
ap.add_argument("--nlist", type=int, default=1024)
ap.add_argument("--nprobe", default="8,32")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--skip-ivf", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)


def corpus():
    g.manual_seed(1)
    cent = torch.randn((1024, a.dim), generator=g, device=dev) if a.clustered else None
    done = 0
    while done < a.rows:
        m = min(1 << 20, a.rows - done)
        x = torch.randn((m, a.dim), generator=g, device=dev)
        if cent is not None:
            x = cent[torch.randint(0, 1024, (m,), generator=g, device=dev)] + 0.3 * x
        yield x
        done += m
    corpus.cent = cent


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps * 1e3, out


def recall(I, Ix, k):
    return float(np.mean([len(set(I[i, :k]) & set(Ix[i, :k])) / k for i in range(len(I))]))


print(f"graph_perf: {a.rows} x {a.dim}, {'clustered' if a.clustered else 'gaussian'} corpus, R {a.R}, "
      f"build_degree {a.build_degree}", flush=True)
gi = GraphIndex(a.dim, METRIC_IP, normalize=True, R=a.R, build_degree=a.build_degree)
gi.reserve(a.rows)
for x in corpus():
    torch.cuda.synchronize()
    gi.add_device(x.data_ptr(), len(x))
    torch.cuda.synchronize()
nb_max = max(int(v) for v in a.batches.split(","))
Q = torch.randn((nb_max, a.dim), generator=g, device=dev)
if corpus.cent is not None:
    Q = corpus.cent[torch.randint(0, 1024, (nb_max,), generator=g, device=dev)] + 0.3 * Q
Q = Q.cpu().numpy()
t0 = time.perf_counter()
gi.build_graph()
t_build = time.perf_counter() - t0
st = gi.graph_stats()
print(f"build: {t_build:.2f} s (kNN {st['knn_ms'] / 1e3:.2f} s, prune {st['prune_ms'] / 1e3:.2f} s, image "
      f"{st['image_ms'] / 1e3:.2f} s); graph {st['graph_bytes'] / 1e6:.1f} MB, image {st['image_bytes'] / 1e6:.1f} MB",
      flush=True)
_, (Dx, Ix) = timed(lambda: gi.exact_search(Q, 100), 1)
for nb in [int(v) for v in a.batches.split(",")]:
    ms, _ = timed(lambda: gi.exact_search(Q[:nb], 10), a.reps)
    print(f"exact FlatIndex batch {nb}: {ms:.3f} ms per batch, {nb / ms * 1e3:.0f} q/s (k 10)", flush=True)
for ef in [int(v) for v in a.ef.split(",")]:
    _, (D, I) = timed(lambda: gi.search(Q, 100, ef=max(ef, 100)), 1)
    r100 = recall(I, Ix, 100)
    _, (D, I) = timed(lambda: gi.search(Q, 10, ef=ef), 1)
    st = gi.graph_stats()
    r10 = recall(I, Ix, 10)
    for nb in [int(v) for v in a.batches.split(",")]:
        ms, _ = timed(lambda: gi.search(Q[:nb], 10, ef=ef), a.reps)
        st = gi.graph_stats()
        print(f"graph ef {ef} batch {nb}: {ms:.3f} ms per batch, {nb / ms * 1e3:.0f} q/s; recall@10 {r10:.4f}, "
              f"recall@100 (ef {max(ef, 100)}) {r100:.4f}; rows scored per query {st['last_rows_scored'] / nb:.0f}, "
              f"iterations per query {st['last_iterations'] / nb:.1f}, capped {st['last_capped']}", flush=True)
gi.close()
if not a.skip_ivf:
    ivf = IVFIndex(a.dim, a.nlist, METRIC_IP, normalize=True, spherical=True)
    trained = False
    t0 = time.perf_counter()
    for x in corpus():
        torch.cuda.synchronize()
        if not trained:
            ivf.train(x[: min(256 * a.nlist, len(x))].cpu().numpy(), niter=10, seed=1234)
            trained = True
        ivf.add_device(x.data_ptr(), len(x))
        torch.cuda.synchronize()
    ivf.list_sizes()
    print(f"ivf-flat nlist {a.nlist}: train + add {time.perf_counter() - t0:.2f} s", flush=True)
    for nprobe in [int(v) for v in a.nprobe.split(",")]:
        _, (D, I) = timed(lambda: ivf.search(Q, 100, nprobe=nprobe), 1)
        r100 = recall(I, Ix, 100)
        _, (D, I) = timed(lambda: ivf.search(Q, 10, nprobe=nprobe), 1)
        r10 = recall(I, Ix, 10)
        for nb in [int(v) for v in a.batches.split(",")]:
            ms, _ = timed(lambda: ivf.search(Q[:nb], 10, nprobe=nprobe), a.reps)
            print(f"ivf nprobe {nprobe} batch {nb}: {ms:.3f} ms per batch, {nb / ms * 1e3:.0f} q/s; recall@10 {r10:.4f}, "
                  f"recall@100 {r100:.4f}", flush=True)
    ivf.close()
