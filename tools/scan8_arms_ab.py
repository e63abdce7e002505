#!/usr/bin/env python3
"""Developer tool: the 8-bit scan with each set of pipelining arms of ScanChunk8 (csrc/index_kernels.hpp), alternated in one
process.  Needs a library built with `make EXTRA=-DANR_SCAN8_AB` (load it with ANORAG_LIB): the environment variable
ANR_SCAN8_AB picks the form the library launches (launch_scan's table in csrc/index.hip), 0 is the shipped k_scan8.  Prints
ms per scan of synchronous batches and checks that every form returns the same ids and scores."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ano-rag_amd"))
import torch
from anorag_hip import FlatIndex, METRIC_IP
from anorag_hip._lib import OPT_TIMING

FORMS = {
    "0": "shipped k_scan8: (a) splat folded + (c) decode ahead + priority",
    "2": "no arm (the unpipelined loop)",
    "3": "(a) splat folded",
    "4": "(a) + (c) decode one operand ahead",
    "5": "(a) + priority",
    "6": "priority alone",
}
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--forms", default="2,0,3,4,5,6")
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
    for form in a.forms.split(","):
        os.environ["ANR_SCAN8_AB"] = form
        tot = 0.0
        for i in range(a.steps + 2):
            idx.search_device(Q[i].data_ptr(), 64, 100, D.data_ptr(), I.data_ptr())
            if i >= 2:
                tot += idx.last_stats()["scan_ms"]
        torch.cuda.synchronize()
        if ref is None:
            ref = (D.clone(), I.clone())
        else:
            assert torch.equal(ref[0], D) and torch.equal(ref[1], I), f"form {form} changed the result"
        st = idx.last_stats()
        print(f"round {rnd + 1} form {form} {FORMS[form]:58s} scan={tot / a.steps:.3f} ms  "
              f"GB/s={st['scan_bytes'] / 1e9 / (tot / a.steps / 1e3):.0f}", flush=True)
idx.close()
