"""The fp64 route of fit search (sed_fit_search_f64) as cost tables, texts and references, shared by
the CPU tests (tests/test_fit_f64_host.py) and the GPU tests (tests/test_gpu_fit_f64.py).  No device is needed here.

Tables: the two golden tables over all 15 IUPAC symbols, unit costs over 9 and 16 symbols, a table whose fp64 sums
depend on their order, tables that break each limit of the integer planner in turn, and the zero-cost corners.
References: oracle.fit for best hits (fit_envelope.oracle_fit); for hits, run_lanes below over one lane per text,
which keeps the whole last row; the host tests pin it against oracle.fit and against the pure-Python row of
tests/test_fit_hits_host.py.  run_lanes is also the word-for-word model of the kernel's lane."""
import numpy as np

from conftest import load_golden
import sedcost
from fit_envelope import Plan, oracle_fit  # noqa: F401  (oracle_fit: the best-hit reference)

IUPAC = "AGCUYRWSKMDVHBN"
MAXK = 16  # SED_FIT_F64_MAXK
ROWS = 32


def golden15(name):
    p = sedcost.build_plan(load_golden(name), [IUPAC], [IUPAC])
    return Plan(p.sub, p.ins, p.dele)


def golden_dyadic(name, alphabet):
    p = sedcost.build_plan(load_golden(name), [alphabet], [alphabet])
    return Plan(p.sub, p.ins, p.dele)


def unit(K, ins=1.0, dele=1.0):
    return Plan(np.where(np.eye(K) > 0, 0.0, 1.0), ins, dele)


def rounding_table(K=5, seed=11):
    """insert 0.1, delete 0.2, substitutions from {0.1, 0.3, 0.7} off a zero diagonal: 0.1 + 0.2 != 0.3 and
    (0.1 + 0.7) + 0.3 != 0.1 + (0.7 + 0.3) in fp64, so a kernel that reassociates, rebases or fuses shows."""
    rng = np.random.default_rng(seed)
    sub = rng.choice([0.1, 0.3, 0.7], size=(K, K))
    np.fill_diagonal(sub, 0.0)
    return Plan(sub, 0.1, 0.2)


def seeded(seed, K, ins, dele, values):
    rng = np.random.default_rng(seed)
    sub = rng.choice(np.asarray(values, np.float64), size=(K, K))
    np.fill_diagonal(sub, 0.0)
    return Plan(sub, ins, dele)


def integer_limit_tables():
    """(name, Plan, the words of the integer planner's refusal for a 32-symbol pattern): one limit each."""
    third = seeded(3, 4, 1.0, 1.0, [1.0, 2.0])
    third.sub[0, 1] = 1.0 / 3.0
    return [("delete_S_256", seeded(1, 4, 1.0, 256.0, [1.0, 2.0, 7.0]), "delete * S"),
            ("ins_del_256", seeded(2, 4, 128.0, 128.0, [1.0, 100.0, 255.0]), "(insert + delete) * S"),
            ("P_delete_S", seeded(4, 4, 0.5, 10.0, [1.0 / 256, 0.75, 0.5]), "P * delete * S"),
            ("one_third", third, "not all multiples")]


def zero_tables():
    return [("insert_0", seeded(5, 5, 0.0, 1.0, [0.5, 1.0, 2.0])),
            ("delete_0", seeded(6, 5, 1.0, 0.0, [0.5, 1.0, 2.0])),
            ("sub_0", Plan(np.zeros((4, 4)), 0.3, 0.7))]


def f64_only_tables():
    """(name, Plan) of every table above that the integer planner refuses."""
    return ([("costs15", golden15("costs.json")), ("user15", golden15("user_costs.json")), ("unit9", unit(9)),
             ("unit16", unit(16)), ("rounding", rounding_table())]
            + [(n, p) for n, p, _ in integer_limit_tables()] + [("sub_0", zero_tables()[2][1])])


def all_tables():
    """(name, Plan): what the GPU tests run, the integer-served zero corners included."""
    return f64_only_tables() + zero_tables()[:2]


def seam_columns(lanes):
    """End columns that sit on the lanes' seams: every lane's first and last owned column."""
    c0, cnt = np.asarray(lanes["c0"]), np.asarray(lanes["cnt"])
    return sorted(set(c0.tolist()) | set((c0 + cnt - 1).tolist()))


def plant(rng, K, p, n, ends):
    """n random symbols with an exact copy of p ending on each column of `ends` where it fits (column e = after e
    symbols), later ones over earlier ones."""
    t = rng.integers(0, K, size=n).astype(np.uint8)
    for e in ends:
        if len(p) <= e <= n:
            t[e - len(p):e] = p
    return t


def single_lanes(len_p, len_t):
    """One lane per pair from column 0, by hand: the definition itself, no window."""
    n = np.asarray(len_t, np.int64)
    z = np.zeros(len(n), np.int64)
    return {"tw": z, "pair": np.arange(len(n), dtype=np.int64), "pat": z, "plen": np.asarray(len_p, np.int64), "nsteps": n,
            "lead": z, "cnt": n + 1, "c0": z}


def run_lanes(plan, lanes, pats, texts, max_dist=None):
    """sed_fit_f64.hip's lane (fit_f64_dp), word for word, every lane side by side in numpy: the border column
    (double)i * delete with the lane's first column as start, 33 values and 33 starts per lane with the pattern
    right-aligned, front rows overwritten with row 0's (0.0, j), one fp64 add per candidate, the lexicographic minimum
    of (D, -start), nsteps rounded up to 4 with the spare columns unowned, and per lane the first strict minimum over
    the columns it owns.  pats / texts = each pair's codes.  Returns (best, hits): best = (D, start, end) arrays by
    lane; hits (max_dist not None) = [(pair, end, start, D)] of every owned column with D <= max_dist, unsorted."""
    L = len(lanes["pair"])
    pair, plen = np.asarray(lanes["pair"]), np.asarray(lanes["plen"])
    lead, cnt, c0, nsteps = (np.asarray(lanes[k]) for k in ("lead", "cnt", "c0", "nsteps"))
    ins, dele = np.float64(plan.ins) + 0.0, np.float64(plan.dele) + 0.0
    tab = np.zeros((MAXK, MAXK))
    tab[:plan.K, :plan.K] = plan.sub + 0.0
    npad = ROWS - plen
    jb = c0 - lead
    steps = int(((nsteps.max() if L else 0) + 3) & ~3)
    sym = np.zeros((L, steps + 1), np.int64)  # the text symbol a lane reads at step s (zeros past the text)
    pcode = np.full((L, ROWS), 8, np.int64)
    for l in range(L):
        t = np.asarray(texts[pair[l]], np.int64)[jb[l]:jb[l] + steps]
        sym[l, :len(t)] = t
        pcode[l, ROWS - plen[l]:] = pats[pair[l]]
    r = np.arange(ROWS + 1)[None, :]
    D = np.where(r > npad[:, None], (r - npad[:, None]).astype(np.float64) * dele, 0.0)
    S = np.broadcast_to(jb[:, None], (L, ROWS + 1)).copy()
    bD = np.where(lead == 0, D[:, ROWS], np.inf)
    bS, bE = jb.copy(), c0.copy()
    hits = []
    if max_dist is not None:
        for l in np.nonzero((lead == 0) & (D[:, ROWS] <= max_dist))[0]:
            hits.append((int(pair[l]), int(c0[l]), int(jb[l]), float(D[l, ROWS])))
    j = jb.copy()
    u = -lead.copy()
    for s in range(steps):
        t = sym[:, s]
        j = j + 1
        dgD, dgS = D[:, 0].copy(), S[:, 0].copy()
        D[:, 0], S[:, 0] = 0.0, j
        for row in range(1, ROWS + 1):
            cost = tab[pcode[:, row - 1], t]
            oldD, oldS = D[:, row].copy(), S[:, row].copy()
            vD, vS = oldD + ins, oldS
            for cD, cS in ((D[:, row - 1] + dele, S[:, row - 1]), (dgD + cost, dgS)):
                less = (cD < vD) | ((cD == vD) & (cS > vS))
                vD, vS = np.where(less, cD, vD), np.where(less, cS, vS)
            front = row <= npad
            D[:, row], S[:, row] = np.where(front, 0.0, vD), np.where(front, j, vS)
            dgD, dgS = oldD, oldS
        u = u + 1
        owned = (u >= 0) & (u < cnt) & (s < ((nsteps + 3) & ~3))
        take = owned & (D[:, ROWS] < bD)
        bD, bS, bE = np.where(take, D[:, ROWS], bD), np.where(take, S[:, ROWS], bS), np.where(take, j, bE)
        if max_dist is not None:
            for l in np.nonzero(owned & (D[:, ROWS] <= max_dist))[0]:
                hits.append((int(pair[l]), int(j[l]), int(S[l, ROWS]), float(D[l, ROWS])))
    return (bD, bS, bE), hits


def reduce_lanes(best, lanes, npairs):
    """The runtime's reduction: per pair the first strict minimum over its lanes in chunk order: [(D, start, end)]."""
    bD, bS, bE = best
    out = [None] * npairs
    for l, p in enumerate(np.asarray(lanes["pair"]).tolist()):
        if out[p] is None or bD[l] < out[p][0]:
            out[p] = (float(bD[l]), int(bS[l]), int(bE[l]))
    return out


def rows_reference(plan, pats, texts, max_dist):
    """The hits of every (pattern, text) pair from the definition, the whole last row kept: sorted
    [(pair, start, end, dist)] with dist <= max_dist."""
    lanes = single_lanes([len(p) for p in pats], [len(t) for t in texts])
    _, hits = run_lanes(plan, lanes, pats, texts, max_dist)
    return sorted((p, s, e, d) for p, e, s, d in hits)
