#!/usr/bin/env python3
"""Developer tool: the 8-bit scan with either cache policy of its scale words, alternated in one process.  Needs a library
built with `make EXTRA=-DANR_SCAN8_AB` (load it with ANORAG_LIB): while the environment variable ANR_SCAN8_AB is 1 the library
launches k_scan8_ab, the scan with the policy that is not the shipped one.  Prints ms per scan of synchronous batches."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ano-rag_amd"))
import torch
from anorag_hip import FlatIndex, METRIC_IP
from anorag_hip._lib import OPT_TIMING

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=2)
a = ap.parse_args()
dev = torch.device("cuda", 0)
idx = FlatIndex(a.dim, METRIC_IP, normalize=True)
idx.reserve(a.rows)
g = torch.Generator(device=dev); g.manual_seed(1)
done = 0
while done < a.rows:
    m = min(262144, a.rows - done)
    x = torch.randn((m, a.dim), generator=g, device=dev)
    torch.cuda.synchronize()
    idx.add_device(x.data_ptr(), m)
    done += m
idx.set_option(OPT_TIMING, 1)
Q = torch.randn((a.steps + 2, 64, a.dim), generator=g, device=dev)
D = torch.empty((64, 100), device=dev); I = torch.empty((64, 100), device=dev, dtype=torch.int64)
ref = None
for rnd in range(a.rounds):
    for form in ("0", "1"):
        os.environ["ANR_SCAN8_AB"] = form
        tot = 0.0
        for i in range(a.steps + 2):
            idx.search_device(Q[i].data_ptr(), 64, 100, D.data_ptr(), I.data_ptr())
            if i >= 2:
                tot += idx.last_stats()["scan_ms"]
        torch.cuda.synchronize()
        if ref is None:
            ref = (D.clone(), I.clone())
        assert torch.equal(ref[0], D) and torch.equal(ref[1], I)
        st = idx.last_stats()
        print(f"round {rnd + 1} {'k_scan8_ab (other policy)' if form == '1' else 'k_scan8 (shipped policy) '} "
              f"scan={tot / a.steps:.3f} ms  GB/s={st['scan_bytes'] / 1e9 / (tot / a.steps / 1e3):.0f}", flush=True)
idx.close()
