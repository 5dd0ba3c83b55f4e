"""The fp64 route for long patterns (sed_fit_index_search_long_f64) as references and a model, shared
by tests/test_fit_long_f64_host.py and tests/test_gpu_fit_long_f64.py.  No device is needed here.

last_rows: the fp64 last row of any P from the oracle's cell order (left + insert, up + delete, diag + cost, one add
each, the lexicographic minimum of (D, -start)), the pairs side by side in numpy.  It takes P x n Python steps, so it is
for P <= ~130 and n <= ~200; fit_f64_cases.run_lanes is fixed at 32 rows, and the running minimum of
test_fit_hits_host.hits_rows is not valid under rounding.
run_waves: sed_fit_long_f64.hip's wave, step by step: the skew, the hand-over and its one-step delay, lanes not yet
started, front rows, the border column, nsteps + 63 steps, the owned columns, the per-wave record."""
import numpy as np

from fit_f64_cases import MAXK, reduce_lanes  # noqa: F401  (reduce_lanes: the runtime's reduction, by record)

LANES = 64


def last_rows(plan, pats, texts):
    """[(E float64[n + 1], S int64[n + 1])] per pair (pats[k], texts[k]): the last row of the oracle's DP."""
    ins, dele = np.float64(plan.ins) + 0.0, np.float64(plan.dele) + 0.0
    sub = np.asarray(plan.sub, np.float64) + 0.0
    out = [None] * len(pats)
    for P in sorted({len(p) for p in pats}):
        idx = [k for k, p in enumerate(pats) if len(p) == P]
        nmax = max(len(texts[k]) for k in idx)
        T = np.zeros((len(idx), nmax), np.int64)
        for r, k in enumerate(idx):
            T[r, :len(texts[k])] = texts[k]
        A = np.array([np.asarray(pats[k], np.int64) for k in idx]).reshape(len(idx), P)
        D = np.zeros((len(idx), nmax + 1, P + 1))
        S = np.zeros((len(idx), nmax + 1, P + 1), np.int64)
        D[:, 0, :] = np.arange(P + 1, dtype=np.float64) * dele
        S[:, :, 0] = np.arange(nmax + 1)[None, :]
        for j in range(1, nmax + 1):
            t = T[:, j - 1]
            for i in range(1, P + 1):
                vD, vS = D[:, j - 1, i] + ins, S[:, j - 1, i]
                for cD, cS in ((D[:, j, i - 1] + dele, S[:, j, i - 1]), (D[:, j - 1, i - 1] + sub[A[:, i - 1], t], S[:, j - 1, i - 1])):
                    less = (cD < vD) | ((cD == vD) & (cS > vS))
                    vD, vS = np.where(less, cD, vD), np.where(less, cS, vS)
                D[:, j, i], S[:, j, i] = vD, vS
        for r, k in enumerate(idx):
            n = len(texts[k])
            out[k] = (D[r, :n + 1, P].copy(), S[r, :n + 1, P].copy())
    return out


def hits_reference(plan, pats, texts, max_dist):
    """Sorted [(pair, start, end, dist)] with dist <= max_dist, from last_rows."""
    out = []
    for k, (E, S) in enumerate(last_rows(plan, pats, texts)):
        out += [(k, int(S[e]), int(e), float(E[e])) for e in np.nonzero(E <= max_dist)[0].tolist()]
    return out


def best_of_row(E, S):
    """The first strict minimum of a last row: (dist, start, end)."""
    e = int(np.argmin(E))  # (argmin returns the first of equal minima)
    return float(E[e]), int(S[e]), e


def cross(queries, texts):
    """The cross product's pairs, query-major: (pats, texts) by pair = q * len(texts) + d."""
    return [q for q in queries for _ in texts], [t for _ in queries for t in texts]


def run_waves(plan, lanes, R, queries, texts, max_dist=None):
    """Every record of `lanes` (fit_index_long_f64_lanes: query-major, pair = q * len(texts) + d) as one wave of R rows
    a lane, all waves side by side.  Returns (best, hits) as fit_f64_cases.run_lanes does: best = (D, start, end) by
    record; hits (max_dist not None) = [(pair, end, start, D)]."""
    Wn = len(lanes["pair"])
    pair, plen = np.asarray(lanes["pair"]), np.asarray(lanes["plen"])
    lead, cnt, c0, nsteps = (np.asarray(lanes[k]) for k in ("lead", "cnt", "c0", "nsteps"))
    ins, dele = np.float64(plan.ins) + 0.0, np.float64(plan.dele) + 0.0
    tab = np.zeros((MAXK, MAXK))
    tab[:plan.K, :plan.K] = np.asarray(plan.sub, np.float64) + 0.0
    G = LANES * R
    assert (plen <= G).all()
    npad = G - plen                       # G[1 .. npad] are front rows
    jb = c0 - lead
    total = np.where(nsteps > 0, (nsteps + 63 + 3) & ~3, 0)
    steps = int(total.max()) if Wn else 0
    sym = np.zeros((Wn, steps + 1), np.int64)   # lane 0's symbol at step s: the words up to the chunk's last, then zeros
    pcode = np.full((Wn, G), 8, np.int64)
    for w in range(Wn):
        q, d = divmod(int(pair[w]), len(texts))
        words = (int(nsteps[w]) + 3) & ~3
        t = np.asarray(texts[d], np.int64)[jb[w]:jb[w] + words]
        sym[w, :len(t)] = t
        pcode[w, G - plen[w]:] = queries[q]
    pcode = pcode.reshape(Wn, LANES, R)
    lane = np.arange(LANES)[None, :]
    g = (lane * R)[:, :, None] + np.arange(1, R + 1)[None, None, :]           # the register's index in G
    i = g - npad[:, None, None]                                                # its pattern row
    D = np.where(i > 0, i.astype(np.float64) * dele, 0.0)
    S = np.broadcast_to(jb[:, None, None], (Wn, LANES, R)).copy()
    nf = npad[:, None] - lane * R                                              # the lane's registers r < nf are front rows
    g0 = lane * R - npad[:, None]
    tpD = np.where(g0 > 0, g0.astype(np.float64) * dele, 0.0)
    tpS = np.broadcast_to(jb[:, None], (Wn, LANES)).copy()
    tsym = np.zeros((Wn, LANES), np.int64)
    jj = np.broadcast_to(-lane, (Wn, LANES)).copy()
    bD = np.where(lead == 0, D[:, 63, R - 1], np.inf)
    bS, bE = jb.copy(), c0.copy()
    hits = []
    if max_dist is not None:
        for w in np.nonzero((lead == 0) & (D[:, 63, R - 1] <= max_dist))[0]:
            hits.append((int(pair[w]), int(c0[w]), int(jb[w]), float(D[w, 63, R - 1])))
    for s in range(steps):
        jj = jj + 1
        act = jj >= 1
        j = jb[:, None] + jj
        # the hand-over: what lane l - 1 held before this step; lane 0 keeps row 0 and the text's symbol
        upD = np.concatenate([np.zeros((Wn, 1)), D[:, :-1, R - 1]], axis=1)
        upS = np.concatenate([j[:, :1], S[:, :-1, R - 1]], axis=1)
        tsym = np.concatenate([sym[:, s:s + 1], tsym[:, :-1]], axis=1)
        dgD, dgS, abD, abS = tpD, tpS, upD, upS
        for r in range(R):
            cost = tab[pcode[:, :, r], tsym]
            oldD, oldS = D[:, :, r].copy(), S[:, :, r].copy()
            vD, vS = oldD + ins, oldS
            for cD, cS in ((abD + dele, abS), (dgD + cost, dgS)):
                less = (cD < vD) | ((cD == vD) & (cS > vS))
                vD, vS = np.where(less, cD, vD), np.where(less, cS, vS)
            front = r < nf
            nD, nS = np.where(front, 0.0, vD), np.where(front, j, vS)
            D[:, :, r], S[:, :, r] = np.where(act, nD, oldD), np.where(act, nS, oldS)  # (a lane not started keeps the border)
            abD, abS = D[:, :, r], S[:, :, r]
            dgD, dgS = oldD, oldS
        tpD, tpS = upD, upS
        u = jj[:, 63] - lead
        owned = act[:, 63] & (u >= 0) & (u < cnt) & (s < total)
        sD, sS, sE = D[:, 63, R - 1], S[:, 63, R - 1], j[:, 63]
        take = owned & (sD < bD)
        bD, bS, bE = np.where(take, sD, bD), np.where(take, sS, bS), np.where(take, sE, bE)
        if max_dist is not None:
            for w in np.nonzero(owned & (sD <= max_dist))[0]:
                hits.append((int(pair[w]), int(sE[w]), int(sS[w]), float(sD[w])))
    return (bD, bS, bE), hits


def run_waves_grouped(plan, lanes, rows, queries, texts, max_dist=None):
    """run_waves over records whose queries run with different R (rows[q]): best by record, hits concatenated."""
    Wn = len(lanes["pair"])
    q_of = np.asarray(lanes["pair"]) // max(len(texts), 1)
    bD, bS, bE = np.full(Wn, np.inf), np.zeros(Wn, np.int64), np.zeros(Wn, np.int64)
    hits = []
    for R in sorted(set(int(r) for r in rows)):
        sel = np.nonzero(np.asarray(rows)[q_of] == R)[0]
        sub = {k: np.asarray(v)[sel] for k, v in lanes.items()}
        (d, s, e), h = run_waves(plan, sub, R, queries, texts, max_dist)
        bD[sel], bS[sel], bE[sel] = d, s, e
        hits += h
    return (bD, bS, bE), hits
