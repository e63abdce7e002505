"""Loader of tests/golden/notegraph_cases.npz (written by tests/golden/make_notegraph_golden.py from the reference's own
GraphIndex / GraphRetriever) and the PageRank error bound both note-graph test files hold their results to."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "notegraph_cases.npz")
CASES = ("A", "B")


def load_case(name):
    z = np.load(GOLD)
    c = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    c["n"], c["iters"], c["khop"] = int(c["n"]), int(c["iters"]), float(c["khop"])
    c["seed_lists"] = [c["seeds"][a:b] for a, b in zip(c["seed_offs"][:-1], c["seed_offs"][1:])]
    c["results"] = [(c["res_ids"][a:b], c["res_dist"][a:b], c["res_score"][a:b])
                    for a, b in zip(c["res_offs"][:-1], c["res_offs"][1:])]
    c["ties"] = [c["tie_groups"][a:b] for a, b in zip(c["tie_offs"][:-1], c["tie_offs"][1:])]
    return c


def relations_case():
    return json.loads(str(np.load(GOLD)["relations_case"]))


def pagerank_bound(n, src, dst, iters):
    """Componentwise relative distance allowed between two float64 evaluations of the same PageRank iteration
    (networkx's and the restatement's / the device's), derived from the operation count — u = 2**-53, every quantity is
    positive, so a relative error of the addends bounds that of a sum:

      entry of A:   S_i by d_i - 1 additions, a reciprocal, a product             <= (d_max + 1) u
      x_i * A_ij:   one product                                                     <= u
      row j:        d_j positive terms added one at a time from 0.0                 <= d_max u
      dangling:     n_d positive terms in any order (networkx adds them one at a time: n_d - 1; the device's tree is at
                    most 24 deep up to 1.3 M nodes), times p — one addend of the row       <= (max(n_d, 24) + 1) u
      the rest:     acc + dangling, alpha *, (1 - alpha), * p, the final addition   <= 5 u

    so one step is eps = (2 d_max + max(n_d, 24) + 8) u away from the exact map F at its input, componentwise.  F is
    monotone and linear in x with non-negative coefficients, so an input within c (relative, componentwise) gives an
    output within c: after T steps from the common start 1/n an evaluation is within T eps of the exact iterate, and
    two evaluations within 2 T eps of each other (the damping by alpha holds for the L1 norm, not per component, and is
    not claimed).  Second-order terms are ~1e-28 and are covered by the factor 1.01."""
    deg = np.bincount(np.concatenate([src, dst]), minlength=n)
    n_d = int((deg == 0).sum())
    eps = (2 * int(deg.max()) + max(n_d, 24) + 8) * 2.0 ** -53
    return 1.01 * 2 * iters * eps


def max_rel_diff(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))
