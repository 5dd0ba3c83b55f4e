"""The numeric envelope of fit search (sed_fit_search) as cost models and texts, shared by the CPU
model of the lane kernel (tests/test_fit_model.py) and the GPU tests (tests/test_gpu_fit.py).  The planner admits any
table whose costs are integers 0..255 on some scale S = 2^k, k <= 8, with (insert + delete) S <= 255 and K <= 8; the
tables here sit on those limits."""
import numpy as np

import oracle
import sedgpu


class Plan:
    """A cost model over codes 0..K-1, as Context.set_costs and oracle.Costs.from_plan read it."""

    def __init__(self, sub, ins, dele):
        self.sub = np.ascontiguousarray(sub, np.float64)
        self.K = len(self.sub)
        self.sub_int = np.zeros((self.K, self.K), np.uint8)
        self.ins, self.ins_int, self.dele, self.del_int = float(ins), 0, float(dele), 0

    def key(self):
        return (self.K, self.sub.tobytes(), self.ins, self.dele)

    def costs(self):
        """The sed_set_costs arguments (sedgpu.fit_plan, sedgpu.fit_lanes)."""
        return (self.K, self.sub, self.sub_int, self.ins, 0, self.dele, 0)


def seeded_table(seed, K, ins_s, del_s, scale, sub_hi=255):
    """Scaled costs insert = ins_s, delete = del_s, substitutions uniform in 0..sub_hi, all divided by `scale`: a
    nonzero diagonal, asymmetric entries, and (where sub_hi allows) 0, sub_hi, insert + delete and one above it forced
    in, so that the clamp min(cost, insert + delete) and both ends of the addend byte occur."""
    rng = np.random.default_rng(seed)
    sub = rng.integers(0, sub_hi + 1, size=(K, K))
    forced = [0, sub_hi, min(ins_s + del_s, sub_hi), min(ins_s + del_s + 1, sub_hi), 1]
    cells = rng.permutation(K * K)[:len(forced)]
    for c, v in zip(cells, forced):
        sub[c // K, c % K] = v
    sub[0, 0], sub[1, 1] = 0, 3  # one free match, one nonzero diagonal entry for certain
    if scale > 1:
        sub[K - 1, 0] |= 1  # an odd numerator: no smaller scale serves the table
    assert (sub != sub.T).any() and np.diag(sub).any()
    return Plan(sub / float(scale), ins_s / float(scale), del_s / float(scale))


def cost_limit_tables():
    """(name, Plan): the four (insert, delete) S splits of 255, an S = 256 table in steps of 1/256, and an S = 4 table
    whose substitutions reach far above insert + delete."""
    return [("i127_d128", seeded_table(1, 4, 127, 128, 1)),
            ("i1_d254", seeded_table(2, 4, 1, 254, 1)),
            ("i254_d1", seeded_table(3, 5, 254, 1, 1)),
            ("i255_d0", seeded_table(4, 4, 255, 0, 1)),
            ("s256", seeded_table(5, 6, 100, 155, 256)),
            ("s4_clamp", seeded_table(6, 4, 41, 26, 4))]


def eight_symbol_table(K):
    """Rows that differ in every column, and columns that differ in every row: cost(a -> b) = (37 a + 11 b + 5) mod 64
    + (a != b), all below insert + delete = 150, so every byte of the addend words is distinct within its row."""
    a, b = np.indices((K, K))
    sub = (37 * a + 11 * b + 5) % 64 + (a != b)
    for r in range(K):
        assert len(set(sub[r].tolist())) == K and len(set(sub[:, r].tolist())) == K
    return Plan(sub.astype(np.float64), 70, 80)


def mutate(rng, p, K, edits):
    s = p.tolist()
    for _ in range(edits):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(s) + 1))
        if kind == 0 and len(s) > 1:
            del s[min(at, len(s) - 1)]
        elif kind == 1:
            s.insert(at, int(rng.integers(0, K)))
        else:
            s[min(at, len(s) - 1)] = int(rng.integers(0, K))
    return np.array(s, np.uint8)


def planted_text(rng, K, p, n, copies=3):
    """n random symbols with `copies` mutated copies of p (0..3 edits each) written over them."""
    t = rng.integers(0, K, size=n).astype(np.uint8)
    for _ in range(copies):
        m = mutate(rng, p, K, int(rng.integers(0, 4)))[:n]
        at = int(rng.integers(0, n - len(m) + 1))
        t[at:at + len(m)] = m
    return t


def oracle_fit(plan, pats, texts, nthreads=4):
    """[(dist, start, end)] of the pairs from the compiled definition (oracle.fit)."""
    pk = sedgpu.PackedPairs(pats, texts)
    d, s, e = oracle.fit(oracle.Costs.from_plan(plan), pk.codes_a, pk.off_a, pk.len_a, pk.codes_b, pk.off_b, pk.len_b,
                         pk.npairs, nthreads)
    return list(zip(d.tolist(), s.tolist(), e.tolist()))
