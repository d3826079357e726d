"""Dispatch models of C2's launch beyond index order.

    python tools/slice_model.py

Iteration counts of the C2 batch from the oracle (equal to the GPU's); per-iteration
time 1.69 us alone on a CU / 2.03 us with a co-resident instance (tools/iterbench.py,
r07_iterbench.txt; round 5's model ran at 1.823 / 2.19); 256 CUs x 2 slots; a per-instance
setup of 16 iteration-equivalents.  Policies:
index order (the hardware), a clairvoyant longest-first order, and time slicing (an
instance is suspended after Q iterations and requeued at the tail, resuming from its
checkpointed iterate after R iteration-equivalents of recomputation).  1-us steps.

Round 8 adds slice-then-resume (slice_then_resume): a first launch runs every instance to
Q iterations at most, a second one resumes the survivors, the longest first -- ordered by
their true remaining count (clairvoyant) or by the extrapolation the engine's resume key
uses (the residual's geometric decay between Q / 2 and Q, tools/resume_predictors.py's
restatement of it), with that predictor's Spearman correlation with the final count.
"""
import collections
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mpc-tsid_amd")]

ALONE, CO, SETUP, CUS = 1.69, 2.03, 16.0, 256


def run(iters, order, Q=None, R=0.0):
    q = collections.deque((int(i), float(iters[i]) + SETUP) for i in order)
    slot = [[None, None] for _ in range(CUS)]

    def pull():
        if not q:
            return None
        i, rem = q.popleft()
        return [i, rem, Q if Q is not None else float("inf")]
    for s in range(2):
        for c in range(CUS):
            slot[c][s] = pull()
    t = 0.0
    while any(e is not None for row in slot for e in row):
        t += 1.0
        for c in range(CUS):
            rate = 1.0 / (CO if slot[c][0] is not None and slot[c][1] is not None else ALONE)
            for s in range(2):
                e = slot[c][s]
                if e is None:
                    continue
                e[1] -= rate
                e[2] -= rate
                if e[1] <= 0:
                    slot[c][s] = pull()
                elif e[2] <= 0:
                    if q:  # suspend and requeue; run to completion once nothing waits
                        q.append((e[0], e[1] + R))
                        slot[c][s] = pull()
                    else:
                        e[2] = float("inf")
    return t


def slice_then_resume(iters, Q, key, R=41.0):
    """Two launches: every instance in index order for min(iters, Q) iterations, then the survivors
    (iters > Q) for their remaining iterations + R, in descending order of key (indexed like iters)."""
    it = np.asarray(iters)
    first = run(np.minimum(it, Q), np.arange(len(it)))
    sel = np.where(it > Q)[0]
    if len(sel) == 0:
        return first
    rem = np.zeros(len(it))
    rem[sel] = it[sel] - Q + R - SETUP  # (run() adds the setup; the resume cost R stands in for it)
    order = sel[np.argsort(-np.asarray(key, dtype=np.float64)[sel], kind="stable")]
    return first + run(rem, order)


def extrapolated_left(O, b, sel, Q):
    """The iterations left after Q as the engine's resume key extrapolates them (restated on the
    unscaled relative residuals, as tools/resume_predictors.py): the residual's geometric decay
    between Q / 2 and Q, primal and dual, the larger."""
    import scipy.sparse as sp
    N = b["xref"].shape[2] - 1
    indptr, indices = O.pattern(N)
    n, m, _ = O.dims(N)
    p0 = O.default_params()
    Pd = np.concatenate([np.tile(np.array(p0.state_weights), N), np.full(12 * N, p0.force_weight)])
    eps = p0.eps_rel
    out = np.zeros(len(sel))
    for j, i in enumerate(sel):
        Ax, l, u = O.formulate(b["xref"][i], b["fsteps"][i])
        A = sp.csc_matrix((Ax, indices, indptr), shape=(m, n))
        r = []
        for K in (Q // 2, Q):
            s = O.qp_solve(N, Ax, l, u, params=O.default_params(max_iter=K))
            ax, aty = A @ s["x"], A.T @ s["y"]
            rp = np.max(np.maximum(0.0, np.maximum(l - ax, ax - u))) / max(np.max(np.abs(ax)), 1e-300)
            rd = np.max(np.abs(Pd * s["x"] + aty)) / max(np.max(np.abs(Pd * s["x"])), np.max(np.abs(aty)), 1e-300)
            r.append((rp / eps, rd / eps))

        def left(r1, r2):
            if not r2 > 1.0:
                return 0.0
            if not r1 > r2:
                return 1e30
            return np.log(r2) / np.log(r1 / r2) * (Q - Q // 2)
        out[j] = max(left(r[0][0], r[1][0]), left(r[0][1], r[1][1]))
    return out


def main():
    import mpcq
    from oracle import oracle as O
    O.build()
    b = mpcq.synth.make_batch(1024, 16, gaits=("trot",), seed=2)
    it = O.solve_batch(b["xref"], b["fsteps"], 0, nthreads=os.cpu_count() or 1)["iters"]
    idx = np.arange(len(it))
    base = run(it, idx)
    print(f"index order: {base / 1e3:.2f} ms")
    lpt = run(it, np.argsort(-it, kind="stable"))
    print(f"longest first (clairvoyant): {lpt / 1e3:.2f} ms ({lpt / base:.2f}x)")
    for Q in (100, 200, 400, 800):
        for R in (41.0, 5.0):
            v = run(it, idx, Q, R)
            print(f"time slicing Q = {Q} iterations, resume {R:.0f}: {v / 1e3:.2f} ms ({v / base:.2f}x)")
    from scipy.stats import spearmanr
    for Q in (400, 500, 600):
        sel = np.where(it > Q)[0]
        true = slice_then_resume(it, Q, it)
        key = np.zeros(len(it))
        key[sel] = extrapolated_left(O, b, sel, Q)
        pred = slice_then_resume(it, Q, key)
        print(f"slice at Q = {Q}, resume {len(sel)} survivors longest first: by the true count {true / 1e3:.2f} ms "
              f"({true / base:.2f}x), by the extrapolated count {pred / 1e3:.2f} ms ({pred / base:.2f}x; Spearman "
              f"with the final count {spearmanr(key[sel], it[sel])[0]:+.2f})")


if __name__ == "__main__":
    main()
