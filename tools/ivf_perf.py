#!/usr/bin/env python3
"""Developer tool: IVF-Flat (anorag_hip.IVFIndex) against the exact FlatIndex on one synthetic corpus, in one process —
train and add time, search ms per batch at several nprobe, recall@k against the exact top-k (not part of bench.py)."""
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
a = ap.parse_args()
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(1)
chunk = 1 << 20
cent = torch.randn((1024, a.dim), generator=g, device=dev) if a.clustered else None


def rows(m):
    x = torch.randn((m, a.dim), generator=g, device=dev)
    if cent is not None:
        x = cent[torch.randint(0, 1024, (m,), generator=g, device=dev)] + 0.3 * x
    return x


print(f"ivf_perf: {a.rows} x {a.dim}, nlist {a.nlist}, {'clustered' if a.clustered else 'gaussian'} corpus, k {a.k}", flush=True)
ivf = IVFIndex(a.dim, a.nlist, METRIC_IP, normalize=True)
flat = FlatIndex(a.dim, METRIC_IP, normalize=True)
flat.reserve(a.rows)
xtrain = None
t_add = 0.0
done = 0
while done < a.rows:
    m = min(chunk, a.rows - done)
    x = rows(m)
    torch.cuda.synchronize()
    if xtrain is None:
        xtrain = x[: min(a.train_rows, m)].cpu().numpy()
        t0 = time.perf_counter()
        ivf.train(xtrain, niter=a.niter, seed=1234)
        t_train = time.perf_counter() - t0
        print(f"train: {len(xtrain)} rows, {a.niter} iterations: {t_train:.3f} s", flush=True)
    t0 = time.perf_counter()
    ivf.add_device(x.data_ptr(), m)
    t_add += time.perf_counter() - t0
    flat.add_device(x.data_ptr(), m)
    torch.cuda.synchronize()
    done += m
t0 = time.perf_counter()
sizes = ivf.list_sizes()  # the list-ordered copy is built here, once, after the last add
t_add += time.perf_counter() - t0
print(f"add: {a.rows} rows in {t_add:.3f} s ({a.rows / t_add / 1e6:.2f} M rows/s); list sizes min {sizes.min()} "
      f"median {int(np.median(sizes))} max {sizes.max()}", flush=True)

Q = rows(64).cpu().numpy()


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps * 1e3, out


for nb in (1, 64):
    ms, _ = timed(lambda: flat.search(Q[:nb], a.k), a.reps)
    print(f"exact FlatIndex batch {nb}: {ms:.3f} ms per batch", flush=True)
_, (Dx, Ix) = timed(lambda: flat.search(Q, a.k), 1)
for nprobe in [int(v) for v in a.nprobe.split(",")]:
    line = []
    for nb in (1, 64):
        ms, (D, I) = timed(lambda: ivf.search(Q[:nb], a.k, nprobe=nprobe), a.reps)
        line.append(f"batch {nb} {ms:.3f} ms")
    _, (D, I) = timed(lambda: ivf.search(Q, a.k, nprobe=nprobe), 1)
    recall = np.mean([len(set(I[i]) & set(Ix[i])) / a.k for i in range(len(Q))])
    print(f"ivf nprobe {nprobe}: {', '.join(line)}; recall@{a.k} vs exact {recall:.4f}", flush=True)
ivf.close()
flat.close()
