#!/usr/bin/env python3
"""Developer tool: IVF-Flat (anorag_hip.IVFIndex) against the exact FlatIndex on one synthetic corpus, in one process —
train and add time, search ms per batch at several nprobe, recall@k against the exact top-k (not part of bench.py).
--pq-m 8,32,96: the same for IVF-PQ handles (IVFIndex(..., pq_m=m)) on the same corpus, one after the other, with the
device / host bytes of each index (memory()) and the code bytes the ADC scan looks up per batch."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ano-rag_amd"))
import numpy as np
import torch
from anorag_hip import FlatIndex, IVFIndex, METRIC_IP

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--train-rows", type=int, default=1_000_000)
ap.add_argument("--niter", type=int, default=25)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--nprobe", default="1,8,32,128")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--clustered", action="store_true", help="1024 Gaussian centres, sigma 0.3 (as tools/scan_perf.py)")
ap.add_argument("--pq-m", default="", help="comma-separated sub-space counts: also measure IVF-PQ handles")
ap.add_argument("--skip-ivf-flat", action="store_true", help="measure only the IVF-PQ handles (with --pq-m)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
chunk = 1 << 20


def rows(m, cent):
    x = torch.randn((m, a.dim), generator=g, device=dev)
    if cent is not None:
        x = cent[torch.randint(0, 1024, (m,), generator=g, device=dev)] + 0.3 * x
    return x


def corpus():
    """the corpus in chunks of 2^20 rows; every pass yields the same rows, and leaves the generator where the queries
    start"""
    g.manual_seed(1)
    cent = torch.randn((1024, a.dim), generator=g, device=dev) if a.clustered else None
    done = 0
    while done < a.rows:
        m = min(chunk, a.rows - done)
        yield rows(m, cent)
        done += m
    corpus.cent = cent


def build(idx, flat=None):
    """train on the first train-rows rows, add every row (add_device); returns (train s, add s)"""
    t_train = t_add = 0.0
    trained = False
    for x in corpus():
        torch.cuda.synchronize()
        if not trained:
            xtrain = x[: min(a.train_rows, len(x))].cpu().numpy()
            t0 = time.perf_counter()
            idx.train(xtrain, niter=a.niter, seed=1234)
            t_train = time.perf_counter() - t0
            trained = True
        t0 = time.perf_counter()
        idx.add_device(x.data_ptr(), len(x))
        t_add += time.perf_counter() - t0
        if flat is not None:
            flat.add_device(x.data_ptr(), len(x))
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    sizes = idx.list_sizes()  # the list-ordered copy is built here, once, after the last add
    t_add += time.perf_counter() - t0
    return t_train, t_add, sizes


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps * 1e3, out


def report(name, idx, Q, Ix, extra=None):
    for nprobe in [int(v) for v in a.nprobe.split(",")]:
        line = []
        for nb in (1, 64):
            ms, (D, I) = timed(lambda: idx.search(Q[:nb], a.k, nprobe=nprobe), a.reps)
            line.append(f"batch {nb} {ms:.3f} ms")
        _, (D, I) = timed(lambda: idx.search(Q, a.k, nprobe=nprobe), 1)
        recall = np.mean([len(set(I[i]) & set(Ix[i])) / a.k for i in range(len(Q))])
        tail = f"; {extra(nprobe)}" if extra else ""
        print(f"{name} nprobe {nprobe}: {', '.join(line)}; recall@{a.k} vs exact {recall:.4f}{tail}", flush=True)


print(f"ivf_perf: {a.rows} x {a.dim}, nlist {a.nlist}, {'clustered' if a.clustered else 'gaussian'} corpus, k {a.k}", flush=True)
flat = FlatIndex(a.dim, METRIC_IP, normalize=True)
flat.reserve(a.rows)
ivf = None if a.skip_ivf_flat else IVFIndex(a.dim, a.nlist, METRIC_IP, normalize=True)
if ivf is not None:
    t_train, t_add, sizes = build(ivf, flat)
    print(f"train: {min(a.train_rows, chunk, a.rows)} rows, {a.niter} iterations: {t_train:.3f} s", flush=True)
    print(f"add: {a.rows} rows in {t_add:.3f} s ({a.rows / t_add / 1e6:.2f} M rows/s); list sizes min {sizes.min()} "
          f"median {int(np.median(sizes))} max {sizes.max()}", flush=True)
else:
    for x in corpus():
        torch.cuda.synchronize()
        flat.add_device(x.data_ptr(), len(x))
        torch.cuda.synchronize()  # before the chunk's memory can be reused
Q = rows(64, corpus.cent).cpu().numpy()
for nb in (1, 64):
    ms, _ = timed(lambda: flat.search(Q[:nb], a.k), a.reps)
    print(f"exact FlatIndex batch {nb}: {ms:.3f} ms per batch", flush=True)
_, (Dx, Ix) = timed(lambda: flat.search(Q, a.k), 1)
flat.close()
if ivf is not None:
    mem = ivf.memory()
    print(f"ivf-flat memory: device {mem['device_bytes'] / 1e9:.3f} GB, host {mem['host_bytes'] / 1e9:.3f} GB", flush=True)
    report("ivf", ivf, Q, Ix)
    ivf.close()
for m in [int(v) for v in a.pq_m.split(",") if v]:
    pq = IVFIndex(a.dim, a.nlist, METRIC_IP, normalize=True, pq_m=m)
    t_train, t_add, sizes = build(pq)
    mem = pq.memory()
    print(f"ivf-pq m {m}: train {t_train:.3f} s, add {a.rows} rows {t_add:.3f} s; memory device "
          f"{mem['device_bytes'] / 1e9:.3f} GB, host {mem['host_bytes'] / 1e9:.3f} GB", flush=True)
    # rows whose codes a batch of 64 looks up: the probed lists' 64-row tiles (the lists nearest to each normalised query)
    qn = Q / np.linalg.norm(Q, axis=1, keepdims=True)
    cs = qn.astype(np.float64) @ pq.centroids.T.astype(np.float64)
    padded = (sizes + 63) // 64 * 64

    def lookups(nprobe):
        top = np.argsort(-cs, axis=1, kind="stable")[:, :nprobe]
        rows = int(padded[top].sum())
        return f"batch 64 scans {rows} code rows ({rows * 4 * ((m + 3) // 4) / 1e6:.1f} M LUT lookups)"

    report(f"ivf-pq m {m}", pq, Q, Ix, lookups)
    pq.close()
