#!/usr/bin/env python3
"""bench.py — headline benchmark of the dense-retrieval hot path (BASELINE.json `metric`).

Workload: exact top-100 of batch-64 queries over a 10M x 768 synthetic corpus (unit-norm Gaussian rows,
cosine == inner product), the configuration BASELINE.json's metric is quoted on.  One "step" is one
batch of 64 queries answered end to end (query prep, scan, select, exact re-score, merge).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run builds the corpus, warms up, times the K steps and prints the headline line (`value`, `ms_per_step`, `dtype`,
the timed region's own search statistics).  --dump-outputs DIR then also writes the last timed step's results, as a
caller of the search receives them, to DIR/topk_scores.npy (float32 [batch, k]) and DIR/topk_ids.npy (the int64 global
row ids as float64, exact below 2^53); the corpus and the queries come from fixed seeds, so two builds run with the same
arguments can be compared output for output.  Everything else below (`roofline`, `recall_at_k`,
`same_results_from_the_f16_image`, `facade`, `legs`, `cpu_baseline`) is measured only with --full.

N = 1: the whole corpus sits on one MI355X (fp32 rows + blocked f16 image + its 12-bit image = 57.6 GB).
N > 1 (launched by torch.distributed.run, one rank per GPU): the corpus is row-sharded, every rank
scans its shard for the same batch, the [64,100] partial top-k (score f32 + global id i64) of two consecutive
batches are all-gathered over RCCL in one collective and merged — each batch only after anr_index_wait() has made it
final on its shard (certificate recovery included); strong scaling (total corpus fixed).

Rank 0 prints ONE JSON line.  `value` = queries/s of the whole job with the corpus resident in HBM.
`roofline` is for the dominant kernel (k_scan): algorithmic bytes = rows x 768 x 1.5 B (the image actually streamed:
every stored f16 rounded to its top 12 bits, ANR_OPT_SCAN_BITS — 2 B with --scan-bits 16; the figure is the library's own
`scan_bytes` statistic) per launch / that kernel's duration.  The duration is taken with HIP events around the
launch on its own stream in a leg of SERIALISED batches right after the timed region (one batch in flight,
so the events bracket the kernel and nothing else): inside the timed region three batches are in flight on
three streams and the same events also span the wait for the previous batch's scan to leave the CUs (that
figure is kept as `ms_per_launch_overlapped`; in round 2 it was reported as the kernel time and exceeded
ms_per_step).  `cpu_baseline` is the oracle (numpy sgemm + argpartition restatement of the reference's
faiss-flat path) timed on this box's host cores on a bounded row sample and scaled linearly to the full corpus.
The interpreter's cyclic garbage collector is switched off once the corpus is built (as `timeit` does).
`legs` (N = 1 only, untimed extras, never `value`): the other BASELINE.json configurations measured in the same
driver-run process, before any CPU leg — the 1.25 M-row shard and the 1 M-row C2 pipeline (every segment of their timed
loops, with the library's batch log naming the largest host and device gap of each), the shard size on SURVEY.md 8d's
clustered corpus and on a tight mixture whose certificates fail, C1 (one query at a time), the C4 encoder forward (MFMA
roofline), the C5 N-array fusion (HBM roofline).
"""
from __future__ import annotations

import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "ano-rag_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
SCAN_BITS = 0  # ANR_OPT_SCAN_BITS of every index this file builds (--scan-bits; 0 = the library's default: 12 bits from 262 144 rows on)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's top-k scores and ids to DIR/topk_scores.npy and DIR/topk_ids.npy")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: the scan kernel's own time and "
                         "roofline, the f16-image cross-check, the facade leg, the other configurations' legs, recall@k "
                         "against the oracle and the CPU baseline (the --no-* options below switch parts of it off)")
    ap.add_argument("--rows", type=int, default=10_000_000, help="total corpus rows (all ranks)")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--cpu-rows", type=int, default=1_000_000, help="rows of the CPU-baseline sample (SURVEY.md 8d: 1 M)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--recall-queries", type=int, default=-1,
                    help="queries of the last batch checked against the oracle (-1 = the whole batch, 0 = skip)")
    ap.add_argument("--no-legs", action="store_true", help="skip the C2 / shard-size / C4 / C5 legs (N = 1 only)")
    ap.add_argument("--serial-launches", type=int, default=20,
                    help="serialised batches after the timed region from which the kernel-only scan time is taken")
    ap.add_argument("--no-facade", action="store_true", help="skip the VectorIndex.search (host in, dicts out) leg")
    ap.add_argument("--scan-bits", type=int, default=SCAN_BITS, choices=(0, 12, 16),
                    help="ANR_OPT_SCAN_BITS: the image the streaming pass reads (12: every f16 rounded to its top 12 bits, 25 %% "
                         "fewer bytes per row; the certificate accounts for it, results stay exact)")
    ap.add_argument("--in-flight", type=int, default=3,
                    help="batches left in flight (default 3).  1: every batch is retired before the next is enqueued — the form "
                         "the rocprofv3 kernel statistics are taken on: with batches in flight the NEXT scan's workgroups "
                         "take over CU by CU while the previous scan retires, so a profiler's per-kernel span (first "
                         "workgroup start to last workgroup end) includes that wait and is not the kernel's time")
    ap.add_argument("--exchange-group", type=int, default=2,
                    help="N > 1: batches whose partial top-k lists travel in one all-gather")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for rehearsal)")
    ap.add_argument("--one-device", action="store_true", help="rehearsal: every rank uses cuda:0")
    ap.add_argument("--force-dist", action="store_true",
                    help="rehearsal on one GPU: run the N > 1 pipeline (process group, all-gather, merge) with world size 1")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def gen_shard(rows, dim, shard, device, chunk=262_144, centroids=0, sigma=0.0):
    """unit-norm-able Gaussian rows, generated on the device chunk by chunk (torch Philox, seed 1234000 + shard:
    a 30 GB host array from numpy's default_rng([1234, s]) would take minutes; same distribution, other stream).
    centroids > 0: the clustered variant of SURVEY.md 8d — every row is one of `centroids` Gaussian centres + sigma x noise."""
    g = torch.Generator(device=device)
    g.manual_seed(1234 * 1000 + shard)
    cent = torch.randn((centroids, dim), generator=g, device=device, dtype=torch.float32) if centroids else None
    done = 0
    while done < rows:
        m = min(chunk, rows - done)
        x = torch.randn((m, dim), generator=g, device=device, dtype=torch.float32)
        if cent is not None:
            x = cent[torch.randint(0, centroids, (m,), generator=g, device=device)] + sigma * x
        yield x
        done += m


def cpu_baseline(args, world):
    """oracle timed on host cores: bounded sample (1 M rows), scaled linearly in rows; batch 64 (the
    metric's batch) and batch 1 (the reference's own per-query regime)."""
    from oracle import flat_index as orc
    try:
        from threadpoolctl import threadpool_info
        thr = max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
    except Exception:
        thr = os.cpu_count() or 1
    n = min(args.cpu_rows, args.rows)
    # the SAME synthetic stream as the GPU run: the first rows of shard 0 (torch Philox, seed 1234000) and the first
    # query batch (seed 4321), generated on the device and copied to the host
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    xs, got = [], 0
    for xb in gen_shard(max(n, min(args.rows, 262_144)), args.dim, 0, dev):  # the corpus's own chunking: same numbers
        xs.append(xb[: n - got].cpu().numpy())
        got += xs[-1].shape[0]
        if got >= n:
            break
    x = orc.preprocess_vectors(np.concatenate(xs, axis=0))
    del xs
    gq = torch.Generator(device=dev)
    gq.manual_seed(4321)
    q = orc.preprocess_vectors(torch.randn((args.batch, args.dim), generator=gq, device=dev, dtype=torch.float32).cpu().numpy())

    def one(qq):
        s = qq @ x.T
        part = np.argpartition(-s, args.k - 1, axis=1)[:, :args.k]
        ps = np.take_along_axis(s, part, axis=1)
        order = np.argsort(-ps, axis=1, kind="stable")
        return np.take_along_axis(part, order, axis=1)

    def timed(qq, budget_s, max_it):
        one(qq)
        t0 = time.perf_counter()
        it = 0
        while True:
            one(qq)
            it += 1
            dt = time.perf_counter() - t0
            if dt > budget_s or it >= max_it:
                break
        return dt / it, it

    t_batch, it = timed(q, 10.0, 50)
    t_one, it1 = timed(q[:1], 5.0, 200)
    qps_sample = args.batch / t_batch
    qps_full = qps_sample * n / args.rows
    return {
        "value": qps_full,
        "unit": "queries/s",
        "cores": int(thr),
        "kind": "port",
        "batch1_value": (1.0 / t_one) * n / args.rows,
        "sample": (f"numpy fp32 sgemm + argpartition top-{args.k}, the first {n} x {args.dim} rows of the bench corpus (same "
                   f"device-generated stream) and its first query batch: batch {args.batch} {qps_sample:.1f} q/s over {it} batches, "
                   f"batch 1 {1.0 / t_one:.1f} q/s over {it1} calls (`batch1_value`), both scaled x{n / args.rows:.4g} to "
                   f"{args.rows} rows; BLAS threads {int(thr)}, os.cpu_count()={os.cpu_count()}"),
    }


def oracle_partial_topk(args, shards_host_iter, q_host, row0):
    """float64-arbitrated top-k of the given queries over this rank's rows (global ids): (scores [nq,k], ids [nq,k])"""
    from oracle import flat_index as orc
    top = orc.BlockedTopK(orc.preprocess_vectors(q_host), args.k, "ip")
    base = row0
    for xb in shards_host_iter():
        top.push(orc.preprocess_vectors(xb), base)
        base += xb.shape[0]
    return top.result()


def recall_from_partials(parts, I_gpu, k):
    s = np.concatenate([p[0] for p in parts], axis=1)
    i = np.concatenate([p[1] for p in parts], axis=1)
    o = np.argsort(-s, axis=1, kind="stable")[:, :k]
    ref = np.take_along_axis(i, o, axis=1)
    hits = sum(len(set(ref[r].tolist()) & set(I_gpu[r].tolist())) for r in range(ref.shape[0]))
    return hits / float(ref.shape[0] * k)


def pmc_traffic(rows_per_gpu, dim, notes, bytes_per_value=None):
    """HBM bytes per k_scan launch from the committed PMC passes (profiles/*_pmc_traffic_k_scan.json: FETCH_SIZE
    doubled as MI355X_MICROARCH.md prescribes for gfx950, + WRITE_SIZE, separate --pmc runs), scaled by rows when the
    shard differs.  The file records the sha256 of the k_scan region of csrc/index_kernels.hpp it was measured on
    (tools/scan_source_hash.py): when the kernel source has changed since, the figure is stale and is NOT reported (traffic = null, the reason goes to `traffic_note` and
    stderr) — re-run tools/refresh_profiles.sh."""
    import glob
    import hashlib
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic_k_scan.json")))
    if not files:
        notes.append("no profiles/*_pmc_traffic_k_scan.json")
        return None
    with open(files[-1]) as f:
        p = json.load(f)
    src = open(os.path.join(ROOT, "ano-rag_amd", "csrc", "index_kernels.hpp"), "rb").read()
    if p.get("kernel_source_region") == "k_scan":   # (round 4: the scan kernel's own text, not the whole header)
        a = src.index(b"// scan: the dominant kernel.")
        src = src[a:src.index(b"// sample (shadow form of k_scan<DENSE>", a)]
    sha = hashlib.sha256(src).hexdigest()
    if p.get("kernel_source_sha256") != sha:
        msg = (f"{os.path.basename(files[-1])} was measured on another version of index_kernels.hpp "
               f"(recorded {str(p.get('kernel_source_sha256'))[:12]}, current {sha[:12]}): traffic not reported")
        print("bench.py: " + msg, file=sys.stderr)
        notes.append(msg)
        return None
    if p["dim"] != dim:
        notes.append("PMC profile taken at another dim")
        return None
    if bytes_per_value is not None and abs(p.get("bytes_per_stored_value", 2.0) - bytes_per_value) > 0.1:
        notes.append(f"PMC profile taken on the {p.get('bytes_per_stored_value', 2.0)}-byte image, this run scanned the "
                     f"{bytes_per_value:.2f}-byte one: traffic not reported")
        return None
    notes.append(f"STORED measurement, not read in this run: {os.path.basename(files[-1])} (rocprofv3 --pmc passes on the same "
                 f"kernel source, sha256 checked), scaled by rows")
    return p["traffic_bytes_per_launch"] * rows_per_gpu / p["rows"]


MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense f16 / bf16 MFMA peak


def serial_kernel_time(idx, Q, first, count, batch, k, d_ptr, i_ptr, stream):
    """k_scan's own duration: `count` batches issued ONE AT A TIME (sync after each), so the HIP events the library
    records around the launch (OPT_TIMING) bracket the kernel alone — with several batches in flight they also span
    the wait for the previous batch's scan to free the CUs.  Returns (ms per launch, bytes per launch)."""
    from anorag_hip._lib import OPT_TIMING
    idx.sync()
    idx.set_option(OPT_TIMING, 1)  # (only here: the two timing events per batch are markers in the batch's queue — the
    idx.reset_stats()              # pipelined loops run without them)
    for j in range(count):
        idx.search_device_async(Q[first + j].data_ptr(), batch, k, d_ptr, i_ptr, stream)
        idx.sync()
    st = idx.last_stats()
    idx.set_option(OPT_TIMING, 0)
    idx.reset_stats()
    return st["scan_ms"] / max(1, count), st["scan_bytes"] / max(1, count)


def pipeline_leg(rows, dim, batch, k, dev, seed, steps=60, warmup=10, serial=20, centroids=0, sigma=0.0, overfetch=0):
    """the search pipeline at another corpus size (the 8-GPU shard, C2) or distribution (clustered): 3-deep asynchronous
    batches for the per-batch time, then serialised batches for the scan kernel's own time.  EVERY segment of the timed
    loop is reported (a one-off ~78 ms stall sat in the first segment of this leg in the round-3 driver record, hidden
    by a median), and the library's batch log (anr_index_batch_log: host enqueue times + device clock stamps of every
    batch) says where a slow batch lost its time: the largest host gap between two enqueues and the largest
    scan-start-to-scan-start period on the device, per segment."""
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip._lib import OPT_OVERFETCH, OPT_SCAN_BITS
    idx = FlatIndex(dim, METRIC_IP, normalize=True, device=dev.index)
    idx.set_option(OPT_SCAN_BITS, SCAN_BITS)
    idx.reserve(rows)
    for xb in gen_shard(rows, dim, seed, dev, centroids=centroids, sigma=sigma):
        torch.cuda.synchronize()
        idx.add_device(xb.data_ptr(), xb.shape[0])
    del xb
    if overfetch:
        idx.set_option(OPT_OVERFETCH, overfetch)
    g = torch.Generator(device=dev)
    g.manual_seed(4321 + seed)
    nb = warmup + steps
    Q = torch.randn((nb + serial, batch, dim), generator=g, device=dev, dtype=torch.float32)
    if centroids:  # queries from the same mixture (the centres are the first draw of the corpus generator)
        gc_ = torch.Generator(device=dev)
        gc_.manual_seed(1234 * 1000 + seed)
        cent = torch.randn((centroids, dim), generator=gc_, device=dev, dtype=torch.float32)
        Q = cent[torch.randint(0, centroids, (nb + serial, batch), generator=g, device=dev)] + sigma * Q
        del cent
    NS = 3
    S = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    D = [torch.empty((batch, k), device=dev, dtype=torch.float32) for _ in range(NS)]
    I = [torch.empty((batch, k), device=dev, dtype=torch.int64) for _ in range(NS)]

    def run(a, b):
        for i in range(a, b):
            idx.search_device_async(Q[i].data_ptr(), batch, k, D[i % NS].data_ptr(), I[i % NS].data_ptr(), S[i % NS].cuda_stream)
        idx.sync()
        torch.cuda.synchronize()

    run(0, warmup)
    idx.reset_stats()
    seg = max(1, steps // 3)
    segs, diag = [], []
    t_all = 0.0
    for a in range(warmup, nb, seg):
        b = min(a + seg, nb)
        t0 = time.perf_counter()
        run(a, b)
        dt = time.perf_counter() - t0
        t_all += dt
        segs.append(dt / (b - a))
        rec, _ = idx.batch_log(b - a, correlate=False)
        if rec.shape[0] >= 2:
            host = np.diff(np.sort(rec[:, 1])) / 1e3                      # enqueue -> next enqueue, us
            first = np.sort(rec[:, 7])                                    # first workgroup of each main scan, device clock
            per = np.diff(first) / 1e3
            diag.append({"max_host_enqueue_gap_us": float(host.max()), "max_device_scan_to_scan_us": float(per.max()),
                         "median_device_scan_to_scan_us": float(np.median(per)),
                         "host_recovery_ms_per_batch": float(rec[:, 13].mean()) / 1e6})
    st = idx.last_stats()
    ms_k, bytes_k = serial_kernel_time(idx, Q, nb, serial, batch, k, D[0].data_ptr(), I[0].data_ptr(), S[0].cuda_stream)
    idx.close()
    dt = t_all / steps
    gbps = bytes_k / 1e9 / (ms_k / 1e3) if ms_k > 0 else None
    return {"rows": rows, "dim": dim, "batch": batch, "k": k, "ms_per_batch": dt * 1e3,
            "ms_per_batch_note": "mean over all timed batches (every segment below counts)",
            "ms_per_batch_segments": [x * 1e3 for x in segs], "ms_per_batch_median_segment": float(np.median(segs)) * 1e3,
            "ms_per_batch_worst_segment": float(np.max(segs)) * 1e3, "segment_diagnostics": diag, "value": batch / dt,
            "unit": "queries/s", "batches": steps, "exact_fallback_queries": st["n_fallback"],
            "n_from_lists": st["n_from_lists"], "n_dense_exact": st["n_dense_exact"], "overfetch": st["overfetch"],
            "candidates_per_query": st["n_candidates"] / max(1, steps * batch),
            "scan_ms_per_launch": ms_k, "scan_bytes_per_launch": bytes_k, "scan_GBps": gbps,
            "scan_frac_hbm": gbps / HBM_PEAK_GBPS if gbps else None,
            "batch_GBps": bytes_k / 1e9 / dt, "batch_frac_hbm": bytes_k / 1e9 / dt / HBM_PEAK_GBPS}


def encoder_leg(dev):
    """C4's encoder half: bge-base-en SHAPE (12 layers, H 768, 12 heads, I 3072, vocab 30522, CLS pooling + L2
    normalisation) with seeded random weights — no checkpoint exists offline — token ids in, embeddings left on the
    device.  flops per SURVEY.md 8d: sum over layers of 2 T (4 H^2 + 2 H I) + 4 B L^2 H with T = B x padded L."""
    from anorag_hip.encoder import DeviceEncoder
    LAYERS, H, HEADS, I, V, P = 12, 768, 12, 3072, 30522, 512
    rng = np.random.default_rng(7)

    def w(*shape, std=0.03):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std))

    t = {"emb.word": w(V, H), "emb.pos": w(P, H), "emb.type": w(2, H), "emb.ln.g": np.ones(H, np.float32),
         "emb.ln.b": np.zeros(H, np.float32)}
    for li in range(LAYERS):
        for nm, shp in (("q", (H, H)), ("k", (H, H)), ("v", (H, H)), ("o", (H, H)), ("ffn1", (I, H)), ("ffn2", (H, I))):
            t[f"L{li}.{nm}.w"] = w(*shp)
            t[f"L{li}.{nm}.b"] = w(shp[0], std=0.01)
        for ln in ("ln1", "ln2"):
            t[f"L{li}.{ln}.g"] = np.ones(H, np.float32)
            t[f"L{li}.{ln}.b"] = np.zeros(H, np.float32)
    hf = {"num_hidden_layers": LAYERS, "hidden_size": H, "num_attention_heads": HEADS, "intermediate_size": I,
          "vocab_size": V, "max_position_embeddings": P, "type_vocab_size": 2, "layer_norm_eps": 1e-12}
    enc = DeviceEncoder(hf, t, pooling="cls", pos_offset=0, device=dev.index)
    del t
    out = {"model_shape": "bge-base-en: 12 layers, H 768, 12 heads, I 3072, vocab 30522, CLS + L2 normalise; seeded random weights",
           "dtype": "f16 MFMA operands and activations, f32 accumulate / LayerNorm", "peak_TFLOPs": MFMA_PEAK_TFLOPS}
    E = torch.empty((256, H), device=dev, dtype=torch.float32)
    for name, B, L, ragged in (("b256_l64", 256, 64, False), ("c4_b256_l51_ragged", 256, 51, True)):
        ids = rng.integers(5, 30000, size=(B, L)).astype(np.int32)
        lens = (rng.integers(27, L + 1, size=B) if ragged else np.full(B, L)).astype(np.int32)
        if ragged:
            lens[0] = L
        types = np.zeros_like(ids)
        for _ in range(3):
            enc.forward_device(ids, lens, types, True, E.data_ptr())
        ts = []
        for _ in range(15):  # synchronous forwards timed one by one: the median is not moved by a host hiccup
            t0 = time.perf_counter()
            enc.forward_device(ids, lens, types, True, E.data_ptr())
            ts.append(time.perf_counter() - t0)
        dt, dt_mean = float(np.median(ts)), float(np.mean(ts))
        Lp = (L + 31) // 32 * 32
        T = B * Lp
        flops = LAYERS * (2 * T * (4 * H * H + 2 * H * I) + 4 * B * Lp * Lp * H)
        out[name] = {"sequences": B, "max_len": L, "padded_tokens": T, "ms_per_forward": dt * 1e3,
                     "ms_per_forward_mean": dt_mean * 1e3, "forwards_timed": len(ts),
                     "TFLOPs": flops / dt / 1e12, "frac_mfma_peak": flops / dt / 1e12 / MFMA_PEAK_TFLOPS,
                     "sequences_per_s": B / dt,
                     "note": "host ids in (H2D of ids included), embeddings left on the device, synchronous"}
    return out, enc, E


def c4_leg(dev, rows=1_000_000, dim=768, k=100):
    """C4: encode 256 queries (bge-base-en shape) and search them over 1 M x 768 notes — token ids in, ids/scores out"""
    from anorag_hip import FlatIndex, METRIC_IP
    out, enc, E = encoder_leg(dev)
    idx = FlatIndex(dim, METRIC_IP, normalize=True, device=dev.index)
    idx.reserve(rows)
    for xb in gen_shard(rows, dim, 77, dev):
        torch.cuda.synchronize()
        idx.add_device(xb.data_ptr(), xb.shape[0])
    del xb
    rng = np.random.default_rng(8)
    B, L = 256, 51
    ids = rng.integers(5, 30000, size=(B, L)).astype(np.int32)
    lens = rng.integers(27, L + 1, size=B).astype(np.int32)
    types = np.zeros_like(ids)

    def once():
        enc.forward_device(ids, lens, types, True, E.data_ptr())
        return idx.search_device_queries(E.data_ptr(), B, k)

    for _ in range(2):
        once()
    n = 5
    t0 = time.perf_counter()
    for _ in range(n):
        D, I = once()
    dt = (time.perf_counter() - t0) / n
    out["encode_plus_search_1m"] = {"queries": B, "rows": rows, "k": k, "ms_per_256_queries": dt * 1e3, "value": B / dt,
                                    "unit": "queries/s", "note": "token ids in (tokeniser not included), top-k ids and scores "
                                    "out in host memory; the encoder's output never leaves the device"}
    idx.close()
    enc.close()
    return out


def c1_leg(dev, rows=10_000, dim=384, k=10):
    """C1, the reference's own regime: one query at a time over a small corpus, host buffers in and out, synchronous
    (FlatIndex.search -> the single-launch path); numpy on the host beside it"""
    from anorag_hip import FlatIndex, METRIC_IP
    x = np.random.default_rng(1234).standard_normal((rows, dim), dtype=np.float32)
    q = np.random.default_rng(4321).standard_normal((512, dim), dtype=np.float32)
    idx = FlatIndex(dim, METRIC_IP, normalize=True, device=dev.index)
    idx.add(x)
    for i in range(300):
        idx.search(q[i:i + 1], k)
    ts = []
    for i in range(1000):
        t0 = time.perf_counter()
        D, I = idx.search(q[i % 512:i % 512 + 1], k)
        ts.append(time.perf_counter() - t0)
    idx.close()
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    tc = []
    for i in range(200):
        t0 = time.perf_counter()
        qq = q[i:i + 1] / np.linalg.norm(q[i:i + 1])
        s = qq @ xn.T
        part = np.argpartition(-s, k - 1, axis=1)[:, :k]
        np.argsort(-np.take_along_axis(s, part, 1), axis=1)
        tc.append(time.perf_counter() - t0)
    return {"rows": rows, "dim": dim, "k": k, "us_per_query_median": float(np.median(ts)) * 1e6,
            "us_per_query_p99": float(np.percentile(ts, 99)) * 1e6, "queries_timed": len(ts),
            "numpy_host_us_per_query_median": float(np.median(tc)) * 1e6,
            "note": "FlatIndex.search(np.float32[1, dim], k): host buffers in and out, one kernel launch, results polled from pinned memory"}


def c5_leg(dev, nq=200, nn=1_000_000, pool=80):
    """C5's fusion half: HybridSearcher.fuse's arithmetic with bm25 = the FULL N-note score vector per query (what
    bm25_scores() returns: one float64 per note, ~0.1 % non-zero, divided by its maximum) resident on the device and
    dense = a top-100 list per query; algorithmic bytes = N x 8 (float64) or N x 4 (float32 arrays) per query."""
    from anorag_hip.fusion import DeviceArray, fuse_dense
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    bm = torch.zeros((nq, nn), device=dev, dtype=torch.float64)
    pos = torch.randint(0, nn, (nq, nn // 1000), generator=g, device=dev)
    val = torch.randn((nq, nn // 1000), generator=g, device=dev, dtype=torch.float64).abs()
    bm.scatter_(1, pos, val)
    mx = bm.max(dim=1, keepdim=True).values.contiguous()
    bm /= mx
    one = torch.ones_like(mx)
    bm32 = bm.to(torch.float32)
    torch.cuda.synchronize()
    rng = np.random.default_rng(99)
    dense = [(rng.choice(nn, 100, replace=False).astype(np.int64), np.sort(rng.random(100))[::-1].copy()) for _ in range(nq)]
    w = {"dense": 1.0, "bm25": 0.5, "graph": 0.5, "path": 0.1}
    res = {"queries": nq, "notes": nn, "pool": pool, "nonzero_per_query": nn // 1000}
    for label, method, arr_t, with_max in (("linear_f64_max_known", "linear", bm, True), ("linear_f64", "linear", bm, False),
                                           ("rrf_f64", "rrf", bm, False), ("linear_f32_max_known", "linear", bm32, True),
                                           ("rrf_f32", "rrf", bm32, False)):
        dt_np = np.float64 if arr_t.dtype == torch.float64 else np.float32
        rm = DeviceArray.wrap(one.data_ptr(), nq, 1, np.float64, dev.index) if with_max else None
        arr = DeviceArray.wrap(arr_t.data_ptr(), nq, nn, dt_np, dev.index, row_max=rm)
        fuse_dense(method, w, 60.0, pool, nq, {"dense": dense, "bm25": arr}, device=dev.index)
        best = None
        for _ in range(4):
            t0 = time.perf_counter()
            o = fuse_dense(method, w, 60.0, pool, nq, {"dense": dense, "bm25": arr}, device=dev.index, want_stats=True)
            dt = time.perf_counter() - t0
            if best is None or o[4]["scan_ms"] < best[0]["scan_ms"]:
                best = (o[4], dt)
        st, dt = best
        gbps = st["scan_bytes"] / 1e9 / (st["scan_ms"] / 1e3)
        res[label] = {"streaming_kernels_ms": st["scan_ms"], "algorithmic_GB": st["scan_bytes"] / 1e9, "GBps": gbps,
                      "frac_hbm": gbps / HBM_PEAK_GBPS, "call_ms": dt * 1e3, "candidates_per_query": st["n_candidates"] / nq}
    # the same rows in SPARSE form (what anr_bm25_sparse_dev leaves on the device): (id, value) entries instead of N scores
    from anorag_hip.fusion import SparseRows
    cap = nn // 1000
    nzm = bm != 0
    cnt = nzm.sum(dim=1).to(torch.int32).contiguous()
    order = torch.argsort(nzm.to(torch.uint8), dim=1, descending=True, stable=True)[:, :cap].contiguous()  # non-zero ids first
    sp_val = torch.gather(bm, 1, order).contiguous()
    sp_ids = order.to(torch.int32).contiguous()  # (ids < 2^31: the bit pattern of the uint32 the kernel reads)
    del nzm, order
    torch.cuda.synchronize()
    sp = SparseRows.wrap(sp_ids.data_ptr(), sp_val.data_ptr(), cnt.data_ptr(), nq, nn, cap, dev.index)
    full = DeviceArray.wrap(bm.data_ptr(), nq, nn, np.float64, dev.index)
    for label, method in (("linear_sparse_rows", "linear"), ("rrf_sparse_rows", "rrf")):
        ref = fuse_dense(method, w, 60.0, pool, nq, {"dense": dense, "bm25": full}, device=dev.index)
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            o = fuse_dense(method, w, 60.0, pool, nq, {"dense": dense, "bm25": sp}, device=dev.index, want_stats=True)
            dt = time.perf_counter() - t0
            if best is None or o[4]["scan_ms"] < best[0]["scan_ms"]:
                best = (o[4], dt)
        same = bool(np.array_equal(ref[0], o[0]) and ref[1].tobytes() == o[1].tobytes() and np.array_equal(ref[3], o[3]))
        res[label] = {"staging_kernels_ms": best[0]["scan_ms"], "call_ms": best[1] * 1e3, "entries_per_query": float(cnt.float().mean()),
                      "identical_to_the_dense_array_result": same,
                      "note": "sort + prep + stage kernels over the rows' entries; no pass over the N scores"}
    del bm, bm32, sp_val, sp_ids
    torch.cuda.empty_cache()
    return res



def facade_leg(idx, args, q_host):
    """The reference-facing call: VectorIndex.search(np.ndarray[B, D], top_k) -> list of per-query lists of dicts
    (reference vector_store/vector_index.py:206-263), timed end to end on the same resident corpus."""
    from vector_store.vector_index import VectorIndex
    vi = VectorIndex(embedding_dim=args.dim)
    vi.index_type, vi.similarity_metric = "Flat", "cosine"
    vi.index, vi.is_trained, vi.total_vectors = idx, True, idx.ntotal  # the corpus already on the device
    for _ in range(3):
        res = vi.search(q_host, top_k=args.k)
    n = 20
    t0 = time.perf_counter()
    for _ in range(n):
        res = vi.search(q_host, top_k=args.k)
    dt = (time.perf_counter() - t0) / n
    ok = len(res) == args.batch and all(len(r) == args.k for r in res) and set(res[0][0]) == {"index", "score", "rank", "similarity"}
    vi.index = None  # the bench owns the handle
    return {"call": f"VectorIndex.search(np.float32[{args.batch},{args.dim}], top_k={args.k}) -> list[list[dict]]",
            "ms_per_call": dt * 1e3, "value": args.batch / dt, "unit": "queries/s", "calls": n, "shape_ok": bool(ok),
            "note": "host numpy in, Python dicts out, synchronous, one batch at a time (not `value`)"}


def main():
    global SCAN_BITS
    args = parse()
    SCAN_BITS = args.scan_bits
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N")
    dist = None
    dist_on = world > 1 or args.force_dist
    if dist_on:
        import torch.distributed as dist  # noqa: F811
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.one_device:
            local_rank = 0
        torch.cuda.set_device(local_rank)
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    from anorag_hip import FlatIndex, METRIC_IP, _lib
    from anorag_hip._lib import OPT_TIMING

    rows_total = args.rows
    per = (rows_total + world - 1) // world
    row0 = min(rank * per, rows_total)
    my_rows = max(0, min(per, rows_total - row0))

    idx = FlatIndex(args.dim, METRIC_IP, normalize=True, device=local_rank)
    from anorag_hip._lib import OPT_SCAN_BITS
    idx.set_option(OPT_SCAN_BITS, SCAN_BITS)
    idx.reserve(my_rows)
    for xb in gen_shard(my_rows, args.dim, rank, dev):
        torch.cuda.synchronize()
        idx.add_device(xb.data_ptr(), xb.shape[0])
    del xb
    torch.cuda.empty_cache()
    # Python's cyclic collector stays off from here on, as `timeit` runs its statements: a generation-2 pass over the heap
    # torch and numpy leave behind takes 40-70 ms — one landed inside a 60-batch leg and turned 0.35 ms per batch into 1.57
    # (reference counting still frees everything the loops allocate)
    gc.collect()
    gc.disable()

    nb = args.steps + args.warmup
    # (Q keeps room for the serialised batches in a plain run too: the same shape draws the same queries)
    n_q_serial = max(0, args.serial_launches)
    n_serial = n_q_serial if args.full else 0
    gq = torch.Generator(device=dev)
    gq.manual_seed(4321)
    Q = torch.randn((nb + n_q_serial, args.batch, args.dim), generator=gq, device=dev, dtype=torch.float32)
    # steps are issued asynchronously and overlap (the small kernels of neighbouring batches run beside the scan).
    # N = 1: three rotating sets of output buffers and streams.
    # N > 1: anorag_hip.sharded.ShardedStream — the shard's search of a batch is launched and left in flight; the partial
    # lists of G consecutive batches travel in ONE all-gather (fewer, larger collectives: at shard size a per-batch
    # exchange added a serial ~44 us to a 345-us batch — measured with the world-size-1 rehearsal), only once they are
    # FINAL on this shard (anr_index_wait: certificate recovery done) and LAG batches behind the search front, so the
    # device never idles on the host; the merge runs out of the receive buffer on the device.
    LAG = 2
    G = max(1, args.exchange_group) if dist_on else 1
    NSLOT = 3
    streams = [torch.cuda.Stream(device=dev) for _ in range(NSLOT)]
    Dl = [torch.empty((args.batch, args.k), device=dev, dtype=torch.float32) for _ in range(NSLOT)]
    Il = [torch.empty((args.batch, args.k), device=dev, dtype=torch.int64) for _ in range(NSLOT)]
    stream = None
    if dist_on:
        from anorag_hip.sharded import ShardedSearcher
        # (the searcher makes the shard return global ids: ANR_OPT_ID_OFFSET = row0; every shard holds >= k rows)
        searcher = ShardedSearcher(idx, row0, force_device=(world == 1 and args.backend == "nccl"))
        stream = searcher.stream(args.batch, args.k, lag=LAG, group=G, order_caller=False)  # (finish() waits on the host)
    torch.cuda.synchronize()

    issued = [0]   # N = 1: batches issued since the last finish()
    merged = {}

    def step(i):
        if stream is None:
            s = issued[0] % NSLOT
            issued[0] += 1
            idx.search_device_async(Q[i].data_ptr(), args.batch, args.k, Dl[s].data_ptr(), Il[s].data_ptr(),
                                    streams[s].cuda_stream)
            if args.in_flight < NSLOT:
                idx.wait(max(0, args.in_flight - 1))
            merged["last"] = (Dl[s], Il[s])
            return
        done = stream.submit(Q[i], tag=i)
        if done:
            merged["last"] = done[-1][1:]

    def finish():
        idx.sync()              # retires every batch; runs the exact path where a certificate failed
        if stream is not None:
            done = stream.flush()
            if done:
                merged["last"] = done[-1][1:]
            stream.wait()
        torch.cuda.synchronize()
        issued[0] = 0

    # clocks and first touches settle over the first few dozen batches of a process (the driver's 5-step warm-up left the
    # scan ~4 % slower than steady state in round 2): a fixed untimed pre-warm-up before the W warm-up steps
    for rep in range(2):
        for i in range(min(nb, 16)):
            step(i)
        finish()
    for i in range(args.warmup):
        step(i)
    finish()
    idx.reset_stats()
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, nb):
        step(i)
    finish()
    Dres, Ires = merged["last"]
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st_all = idx.last_stats()
    scan_bytes = st_all["scan_bytes"]
    n_fallback, n_cand = st_all["n_fallback"], st_all["n_candidates"]
    if dist_on:
        t = torch.tensor([dt], device=dev if args.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, Dres, Ires)
    if args.full:
        full_run(args, idx, dev, Q, Dl, Il, streams, Dres, Ires, dt, scan_bytes, n_fallback, n_cand, nb, n_serial, per,
                 rows_total, my_rows, row0, world, rank, dist, dist_on, G)
    elif rank == 0:
        print(json.dumps(headline(args, dt, scan_bytes / max(1, args.steps), n_fallback, n_cand, per, rows_total, world,
                                  dist_on, G)), flush=True)
    idx.close()
    if dist_on:
        dist.destroy_process_group()


def dump_outputs(out_dir, Dres, Ires):
    """the last timed step's top-k as a caller receives it: scores float32 [batch, k], global row ids (int64, -1 = none)
    as float64 — exact for every id below 2^53"""
    os.makedirs(out_dir, exist_ok=True)
    D = torch.as_tensor(Dres).cpu().numpy().astype(np.float32, copy=False)
    ids = torch.as_tensor(Ires).cpu().numpy()
    np.save(os.path.join(out_dir, "topk_scores.npy"), D)
    np.save(os.path.join(out_dir, "topk_ids.npy"), ids.astype(np.float64))


def headline(args, dt, bytes_per_step, n_fallback, n_cand, per, rows_total, world, dist_on, G):
    """the fields of the result line that a plain run measures (the timed region and the library's statistics of it)"""
    bytes_per_value = bytes_per_step / max(1.0, float(-(-per // 32) * 32) * args.dim)
    twelve = bytes_per_value < 1.75
    return {
        "metric": "queries/sec + recall@k vs CPU ref, 10M×768 corpus, batch-64 top-100",
        "value": args.batch * args.steps / dt,
        "unit": "queries/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": ("f16 scan (MFMA f16 x f16, f32 accumulate; the scanned image keeps the top 12 bits of every stored f16 — "
                  "ANR_OPT_SCAN_BITS) + f32 rows re-scored in f64" if twelve else
                  "f16 scan (MFMA, f32 accumulate) + f32 rows re-scored in f64"),
        "data": "synthetic",
        "config": {
            "workload": f"{rows_total} x {args.dim} unit-norm Gaussian corpus, batch-{args.batch} top-{args.k} "
                        f"exact cosine search",
            "rows_total": rows_total,
            "rows_per_gpu": per,
            "dim": args.dim,
            "batch": args.batch,
            "k": args.k,
            "parallelism": (f"row-shard x{world}, partial top-k of {G} batches per RCCL all-gather" if dist_on
                            else "single GPU"),
        },
        "exact_fallback_queries": n_fallback,
        "candidates_per_query": n_cand / max(1, args.steps * args.batch),
    }


def full_run(args, idx, dev, Q, Dl, Il, streams, Dres, Ires, dt, scan_bytes, n_fallback, n_cand, nb, n_serial, per,
             rows_total, my_rows, row0, world, rank, dist, dist_on, G):
    """--full: everything after the timed region that the headline figure does not need; prints the full result line"""
    # what the device did inside the timed region, from the library's batch log (device clock stamps left by the kernels
    # themselves; no timing events sit in the batches' queues): the main scans' own spans and the scan-to-scan period
    rec, _ = idx.batch_log(min(args.steps, 512), correlate=False)
    pipe = None
    if rec.shape[0] >= 2:
        first = np.sort(rec[:, 7])
        span = (rec[:, 9] - rec[:, 7]) / 1e6
        pipe = {"scan_span_ms_median": float(np.median(span)), "scan_to_scan_ms_median": float(np.median(np.diff(first))) / 1e6,
                "scan_to_scan_ms_max": float(np.max(np.diff(first))) / 1e6, "batches_logged": int(rec.shape[0]),
                "note": "first workgroup start -> last workgroup end of each main scan (spans of neighbouring scans overlap: "
                        "the next scan's workgroups take over CU by CU), and start-to-start periods, device clock"}
    # the scan kernel's own duration (rank 0's shard): serialised batches, outside the timed region
    Dk, Ik = Dl[0].clone(), Il[0].clone()  # scratch outputs: the last timed batch's results stay untouched
    ker_ms, ker_bytes = (serial_kernel_time(idx, Q, nb, n_serial, args.batch, args.k, Dk.data_ptr(), Ik.data_ptr(),
                                            streams[0].cuda_stream) if n_serial else (None, None))

    # the 12-bit image nominates, the float32 rows decide: the last timed batch again from the f16 image — ids and scores
    # must be the same bits (both are the exact top-k of the float32 rows; `recall_at_k` below checks them against the CPU)
    same_as_f16 = None
    if world == 1 and not dist_on:
        _bpv = (ker_bytes if ker_ms else scan_bytes / max(1, args.steps)) / max(1.0, float(-(-per // 32) * 32) * args.dim)
        if _bpv < 1.75:
            from anorag_hip._lib import OPT_SCAN_BITS
            idx.sync()
            idx.set_option(OPT_SCAN_BITS, 16)
            D16, I16 = torch.empty_like(Dl[0]), torch.empty_like(Il[0])
            idx.search_device(Q[nb - 1].data_ptr(), args.batch, args.k, D16.data_ptr(), I16.data_ptr())
            torch.cuda.synchronize()
            same_as_f16 = bool(torch.equal(I16, torch.as_tensor(Ires).to(I16.device)) and
                               torch.equal(D16, torch.as_tensor(Dres).to(D16.device)))
            idx.set_option(OPT_SCAN_BITS, SCAN_BITS)
            del D16, I16

    # the reference-facing call is timed BEFORE the CPU legs: after the oracle's 10 M-row BLAS passes (recall) the same
    # loop ran 2.3x slower on two boxes (6.4 vs 2.8 ms per call) — host threads left spinning, nothing on the device
    facade = None
    if rank == 0 and world == 1 and not args.no_facade:
        facade = facade_leg(idx, args, Q[nb - 1].cpu().numpy())

    # the other BASELINE.json configurations, in the same driver-run process and BEFORE any CPU leg: in the round-3 driver
    # record the first pipeline leg after the oracle's 10 M-row BLAS passes (the recall check) carried a ~78 ms stall in its
    # first segment — the same host-side after-effect the facade leg had shown (128 BLAS threads left spinning) — and the
    # legs had been left behind the recall pass.  Order now: timed region, kernel-only launches, facade, legs, recall, CPU.
    legs = None
    if rank == 0 and world == 1 and not args.no_legs:
        legs = {}
        shard_rows = 1_250_000
        for name, fn in (("shard_1250k", lambda: pipeline_leg(shard_rows, args.dim, args.batch, args.k, dev, 11)),
                         ("c2_1m", lambda: pipeline_leg(1_000_000, args.dim, args.batch, args.k, dev, 12)),
                         # SURVEY.md 8d's clustered variant (1024 centroids, sigma 0.3) at the shard size, and a TIGHT mixture
                         # (sigma 0.02: hundreds of rows within the f16 error bound of the k-th score) whose certificates
                         # fail, so that the recovery passes' cost is in the record
                         ("shard_1250k_clustered", lambda: pipeline_leg(shard_rows, args.dim, args.batch, args.k, dev, 13,
                                                                        centroids=1024, sigma=0.3)),
                         ("shard_1250k_tight_clusters", lambda: pipeline_leg(shard_rows, args.dim, args.batch, args.k, dev, 14,
                                                                             steps=30, warmup=14, serial=6, centroids=1024, sigma=0.02)),
                         ("c1_10k", lambda: c1_leg(dev)), ("c4", lambda: c4_leg(dev)), ("c5", lambda: c5_leg(dev))):
            try:
                legs[name] = fn()
            except Exception as e:  # a failing extra leg must not cost the headline line
                legs[name] = {"error": f"{type(e).__name__}: {e}"}
                print(f"bench.py: leg {name} failed: {e}", file=sys.stderr)
            torch.cuda.empty_cache()

    # recall@k of the last batch's first few queries vs the oracle: every rank ranks its own rows on the CPU
    # (float64), rank 0 merges the partial lists and compares with the ids the GPU path returned
    recall = None
    if args.recall_queries != 0:
        nrq = args.batch if args.recall_queries < 0 else min(args.recall_queries, args.batch)
        I_gpu = torch.as_tensor(Ires)[:nrq].cpu().numpy()  # (numpy already in the gloo rehearsal)
        qh = Q[nb - 1, :nrq].cpu().numpy()

        def shards():
            for xb in gen_shard(my_rows, args.dim, rank, dev, chunk=524_288):
                yield xb.cpu().numpy()

        part = oracle_partial_topk(args, shards, qh, row0)
        if dist_on:
            parts = [None] * world
            dist.all_gather_object(parts, part)
        else:
            parts = [part]
        if rank == 0:
            recall = recall_from_partials(parts, I_gpu, args.k)

    if rank == 0:
        tnotes = []
        _bpl = ker_bytes if ker_ms else scan_bytes / max(1, args.steps)
        traffic = pmc_traffic(per, args.dim, tnotes, _bpl / max(1.0, float(-(-per // 32) * 32) * args.dim))
        ms_step = dt / args.steps * 1e3
        if ker_ms:
            achieved = (ker_bytes / 1e9) / (ker_ms / 1e3)
            ms_launch = ker_ms
        else:  # --serial-launches 0: the scans' spans in the pipeline (an upper bound of the kernel time)
            ms_launch = pipe["scan_span_ms_median"] if pipe else None
            achieved = (scan_bytes / max(1, args.steps) / 1e9) / (ms_launch / 1e3) if ms_launch else None
        consistent = bool(ms_launch is not None and ms_launch <= ms_step * 1.005)
        if not consistent:
            print(f"bench.py: kernel time per launch {ms_launch:.4f} ms exceeds the step time {ms_step:.4f} ms", file=sys.stderr)
        bpl = ker_bytes if ker_ms else scan_bytes / max(1, args.steps)
        bytes_per_value = bpl / max(1.0, float(-(-per // 32) * 32) * args.dim)
        out = headline(args, dt, bpl, n_fallback, n_cand, per, rows_total, world, dist_on, G)
        out.update({
            "recall_at_k": recall,
            "recall_queries": (args.batch if args.recall_queries < 0 else args.recall_queries),
            "same_results_from_the_f16_image": same_as_f16,
            "roofline": {
                "bound": "hbm",
                "kernel": "k_scan",
                "achieved": achieved,
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": (achieved / HBM_PEAK_GBPS) if achieved else None,
                "traffic": traffic,
                "traffic_note": "; ".join(tnotes),
                "bytes_per_launch": bpl,
                "bytes_per_stored_value": round(bytes_per_value, 3),
                "ms_per_launch": ms_launch,
                "launches_timed": n_serial if ker_ms else args.steps,
                "timing": ("HIP events around the launch on its stream, serialised batches after the timed region"
                           if ker_ms else "device clock stamps of the scans inside the timed region (spans include placement)"),
                "in_timed_region": pipe,
                "launch_le_step": consistent,
                "frac_end_to_end": (scan_bytes / max(1, args.steps) / 1e9) / (ms_step / 1e3) / HBM_PEAK_GBPS,
            },
        })
        if legs is not None:
            out["legs"] = legs
        if facade is not None:
            out["facade"] = facade
        if not args.no_cpu and world == 1:
            out["cpu_baseline"] = cpu_baseline(args, world)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
