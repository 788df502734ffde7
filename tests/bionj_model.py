"""NumPy restatement of BIONJ's arithmetic contract (andi_hip_tree with ANDI_TREE_BIONJ, include/andi_hip.h): what
tests/test_bionj_*.py hold the device to.  Built the way nj_model.nj is -- blockwise selection, sequential row sums by
R += C[k], no copy of the active block per step -- with the second matrix V beside D."""
import numpy as np

from nj_model import NJ_JOIN


def _chain(row):
    """the sequential sum of row's entries, in order, from +0.0 (np.add.accumulate adds one after the other)"""
    return np.add.accumulate(np.concatenate(([0.0], row)))[-1]


def bionj(D, steps=None, lambdas=False):
    """The records andi_hip_tree(..., ANDI_TREE_BIONJ) writes for D (only the upper triangle is read), bit for bit; with
    steps=k only the first k records.  lambdas=True: (records, lam) with lam[s] the weight step s used (one per pair join
    the call went through, so min(steps, n - 3) of them) and why: lam is a structured array of `value` and `halved`
    (vab == 0 or a NaN quotient made it 1/2)."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    nrec = 1 if n == 2 else n - 2
    steps = nrec if steps is None else min(steps, nrec)
    iu = np.triu_indices(n, 1)
    C = np.zeros((n, n))  # diagonal +0.0
    C[iu] = D[iu]
    C.T[iu] = D[iu]
    V = C.copy()
    out = np.zeros(steps, NJ_JOIN)
    lam_out = np.zeros(max(0, min(steps, n - 3)), np.dtype([("value", "<f8"), ("halved", "?")]))
    if steps and n == 2:
        h = C[0, 1] * 0.5
        out[0] = (0, 1, -1, 0, h, h, 0.0)
    if steps == 0 or n == 2:
        return (out, lam_out) if lambdas else out
    ids = np.arange(n)  # ids[p]: the id of the node at position p
    live = np.ones(n, bool)
    with np.errstate(all="ignore"):  # (overflow of finite input: inf and NaN are part of the contract)
        for s in range(min(steps, n - 3)):
            r = n - s
            if len(live) - r > len(live) // 4:
                keep = np.ix_(live, live)
                C, V, ids, live = C[keep], V[keep], ids[live], live[live]
            R = np.zeros(len(live))
            for k in np.flatnonzero(live):
                R += C[k]

            def q_rows(p0):
                rows = slice(p0, p0 + 64)
                Q = (np.float64(r - 2) * C[rows] - R[rows, None]) - R[None, :]
                pair = live[rows, None] & live[None, :] & (ids[rows, None] < ids[None, :])
                return Q, pair

            least = {}  # row block -> its least non-NaN Q
            for p0 in range(0, len(live), 64):
                Q, pair = q_rows(p0)
                num = pair & ~np.isnan(Q)
                if num.any():
                    least[p0] = Q.min(where=num, initial=np.inf)
            if least:
                m = min(least.values())
                px, py = [], []
                for p0 in (p0 for p0, q in least.items() if q == m):
                    Q, pair = q_rows(p0)
                    x, y = np.nonzero(pair & (Q == m))
                    px.append(x + p0)
                    py.append(y)
                px, py = np.concatenate(px), np.concatenate(py)
                k = np.lexsort((ids[py], ids[px]))[0]  # ties: the smaller id(x), then the smaller id(y)
                pa, pb = px[k], py[k]
            else:  # every Q is NaN: the id order alone, so the two smallest ids
                pa, pb = sorted(np.flatnonzero(live), key=lambda p: ids[p])[:2]
            d = C[pa, pb]
            la = d * 0.5 + (R[pa] - R[pb]) / np.float64(2 * (r - 2))
            lb = d - la
            out[s] = (ids[pa], ids[pb], -1, 0, la, lb, 0.0)
            # lambda, from the sums of rows a and b of V over the active slots in ascending order
            rva, rvb = _chain(V[pa][live]), _chain(V[pb][live])
            vab = V[pa, pb]
            lam = np.float64(0.5) + (rvb - rva) / (np.float64(2 * (r - 2)) * vab)
            halved = bool(vab == 0.0 or np.isnan(lam))
            if halved:
                lam = np.float64(0.5)
            if lam < 0.0:
                lam = np.float64(0.0)
            if lam > 1.0:
                lam = np.float64(1.0)
            mu = np.float64(1.0) - lam
            lam_out[s] = (lam, halved)
            pu, po = min(pa, pb), max(pa, pb)  # the new node takes the lower slot, the other retires
            dv = lam * (C[pa] - la) + mu * (C[pb] - lb)
            vv = (lam * V[pa] + mu * V[pb]) - (lam * mu) * vab
            dv[pu] = 0.0
            vv[pu] = 0.0
            C[pu], C[:, pu] = dv, dv
            V[pu], V[:, pu] = vv, vv
            ids[pu] = n + s
            live[po] = False
        if steps == n - 2:
            act = np.flatnonzero(live)
            x, y, z = act[np.argsort(ids[act])]  # (r = 3)
            xy, xz, yz = C[x, y], C[x, z], C[y, z]
            out[n - 3] = (ids[x], ids[y], ids[z], 0, ((xy + xz) - yz) * 0.5, ((xy + yz) - xz) * 0.5,
                          ((xz + yz) - xy) * 0.5)
    return (out, lam_out) if lambdas else out
