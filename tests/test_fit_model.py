"""CPU: the lane kernel of fit search (sed_fit.hip: sed_fit_kernel) restated word op by word op in numpy, vectorised over
lanes, and driven by the planner's own lane records and parameter words (sedgpu.fit_lanes).  Every value is carried
twice: as the 32-bit word the kernel holds, and as the pair of unbounded fields (D field, start field) that word is
meant to pack, updated field by field with no carry between them.  At every column a lane owns or warms up on the model
asserts that
  - every one of the 33 registers, row 0's key inj and every update candidate equals its fields packed, each field
    within 0..65535: no wrap, and no borrow out of or into either half;
  - the sink row's start field is at least inj's (V[32] - inj has no borrow), and u and cnt fit 16 bits;
and at the end that the 64-bit join of the lanes decodes to oracle.fit's hit, exactly.  The unbounded side takes its
update addends from the cost table itself, not from the planner's bytes.  The 32 chained v_min3_u32 of a column are a
running unsigned minimum down the registers, which is how both sides compute them."""
import numpy as np
import pytest

import sedgpu
from fit_envelope import Plan, cost_limit_tables, eight_symbol_table, oracle_fit, planted_text

M32 = 0xFFFFFFFF
ROWS = 32       # FIT_ROWS
REBASE = 128    # FIT_REBASE


def perm(s0, s1, sel):
    """v_perm_b32 D = perm(S0, S1, selector), as __builtin_amdgcn_perm(s0, s1, sel): selector byte 0..3 picks that byte
    of s1, 4..7 a byte of s0, 0x0C gives 0x00 and 0x0D.. 0xFF (8..11, the sign replications, do not occur here)."""
    s0, s1, sel = np.broadcast_arrays(np.asarray(s0, np.int64), np.asarray(s1, np.int64), np.asarray(sel, np.int64))
    src = (s0 << 32) | s1
    out = np.zeros(src.shape, np.int64)
    for b in range(4):
        k = (sel >> (8 * b)) & 0xFF
        assert not ((k >= 8) & (k < 12)).any()
        byte = (src >> (8 * (k & 7))) & 0xFF
        byte = np.where(k >= 0x0D, 0xFF, np.where(k == 0x0C, 0, byte))
        out |= byte << (8 * b)
    return out


def s32(x):
    """The int32 reading of a 32-bit word."""
    return np.where(x & 0x80000000, x - (1 << 32), x)


class Job:
    """One search: a cost model, options, patterns and texts.  filler = (count, P, n): that many more pairs of these
    lengths go to the planner after the real ones (a batch large enough to change the chunk rule); the model leaves
    their lanes out."""

    def __init__(self, name, plan, options, pats, texts, filler=(0, 1, 0)):
        self.name, self.plan, self.options, self.pats, self.texts = name, plan, options, pats, texts
        self.len_p = [len(p) for p in pats] + [filler[1]] * filler[0]
        self.len_t = [len(t) for t in texts] + [filler[2]] * filler[0]


def run_model(jobs):
    """Runs every lane of every job side by side and returns, per job, the joined hits [(dist, start, end)]."""
    rec = {k: [] for k in sedgpu.FIT_LANE_FIELDS}
    lane_job, clo, chi, kx, ins32, del32, insx, delx, text_of = [], [], [], [], [], [], [], [], []
    pair_base, scale = [], []
    npairs = 0
    for jn, jb in enumerate(jobs):
        lanes, par = sedgpu.fit_lanes(jb.plan.costs(), jb.options, jb.len_p, jb.len_t)
        real = lanes["pair"] < len(jb.pats)
        lanes = {k: v[real] for k, v in lanes.items()}
        S = sedgpu.fit_plan(jb.plan.costs(), jb.options, jb.len_p, jb.len_t)["scale"]
        scale.append(S)
        pair_base.append(npairs)
        K = jb.plan.K
        sub = jb.plan.sub * S
        I, D = jb.plan.ins * S, jb.plan.dele * S
        assert I == int(I) and D == int(D) and (sub == np.floor(sub)).all()
        assert (par["ins"], par["del"]) == (int(I), int(D))
        # tab[9] of the kernel: the addend words of pattern symbol a, row 8 (front rows) zeros
        tab = np.zeros((9, 2), np.int64)
        tab[:8] = par["row"]
        # the unbounded side's addends kappa(a -> b) = insert + delete - min(cost, insert + delete), from the table
        kap = np.zeros((9, 8), np.int64)
        kap[:K, :K] = I + D - np.minimum(sub, I + D)
        for q, p in enumerate(jb.pats):  # the pattern record: 32 byte codes, right-aligned, code 8 in front
            code = np.full(ROWS, 8, np.int64)
            code[ROWS - len(p):] = p
            sel = lanes["pair"] == q
            n = int(sel.sum())
            clo += [tab[code, 0]] * n
            chi += [tab[code, 1]] * n
            kx += [kap[code]] * n
            text_of += [np.asarray(jb.texts[q], np.int64)] * n
        assert (np.diff(lanes["pair"]) >= 0).all()  # (lanes come pair by pair, so the lists above are in lane order)
        nl = len(lanes["pair"])
        for k in sedgpu.FIT_LANE_FIELDS:
            rec[k].append(lanes[k] + (npairs if k == "pair" else 0))
        lane_job += [jn] * nl
        ins32 += [par["ins"]] * nl
        del32 += [par["del"]] * nl
        insx += [int(I)] * nl
        delx += [int(D)] * nl
        npairs += len(jb.pats)
    rec = {k: np.concatenate(v) for k, v in rec.items()}
    L = len(lane_job)
    lane_job = np.array(lane_job)
    clo, chi, kx = np.array(clo), np.array(chi), np.array(kx)          # [L, 32], [L, 32], [L, 32, 8]
    ins32, del32, insx, delx = (np.array(v, np.int64) for v in (ins32, del32, insx, delx))
    nsteps, lead, cnt, c0, plen = rec["nsteps"], rec["lead"], rec["cnt"], rec["c0"], rec["plen"]
    assert (cnt >= 1).all() and (cnt <= 0xFFFF).all(), "cnt fits 16 bits"
    ncols = int(((nsteps.max() + 3) // 4) * 4)
    T = np.zeros((L, ncols + 4), np.int64)  # the text from each lane's border column on, zeros past its end
    for i in range(L):
        seg = text_of[i][4 * int(rec["tw"][i]):4 * int(rec["tw"][i]) + ncols]
        T[i, :len(seg)] = seg
    # perm(chi, clo, sel) for sel of every (k, symbol): the selector is built from the text word as the kernel does,
    # with the word's other bytes all ones to show they do not matter
    KW = np.zeros((4, 8, L, ROWS), np.int64)
    for k in range(4):
        for sym in range(8):
            w = (M32 ^ (0xFF << (8 * k))) | (sym << (8 * k))
            sel = perm(w, 0x0C0C0C0C, (4 + k) << 16)
            KW[k, sym] = perm(chi, clo, sel)
    KW = np.ascontiguousarray(KW.transpose(0, 2, 3, 1))  # [k, L, 32, sym]
    ar = np.arange(L)

    # the kernel's words
    pdel = (plen * del32) & M32
    rebase = ((REBASE * ins32) << 16) & M32
    step = ((ins32 << 16) + 1) & M32
    inj = (((pdel << 16) + rebase) & M32) | 0xFFFF
    V = np.repeat(inj[:, None], ROWS + 1, axis=1)
    u = -lead.copy()
    bestc = np.where(lead == 0, 0, 0x7FFFFFFF).astype(np.int64)
    bestt = np.zeros(L, np.int64)
    # the fields: X = D field * 2^32 + start field (ordered as (D field, start field) while |start field| < 2^31)
    F = 1 << 32
    pdx = plen * delx
    injx = (pdx + REBASE * insx) * F + 0xFFFF
    VX = np.repeat(injx[:, None], ROWS + 1, axis=1)
    bhi = np.where(lead == 0, 0, 1 << 40).astype(np.int64)  # best D - P delete, its owned column, its end - start
    bu = np.zeros(L, np.int64)
    blen = np.zeros(L, np.int64)

    def fields(X):
        hi = (X + (1 << 31)) >> 32
        return hi, X - hi * F

    def check(W32, X, valid, what, col):
        hi, lo = fields(X)
        bad = ((hi < 0) | (hi > 0xFFFF) | (lo < 0) | (lo > 0xFFFF) | (W32 != ((hi << 16) | lo)))
        bad = bad & (valid if bad.ndim == 1 else valid[:, None])
        if bad.any():
            i = int(np.argwhere(bad)[0][0])
            raise AssertionError("%s: job %s lane %d (P %d, c0 %d, lead %d, cnt %d) column %d: word %s, fields %s"
                                 % (what, jobs[lane_job[i]].name, i, plen[i], c0[i], lead[i], cnt[i], col,
                                    np.atleast_1d(W32[i])[:].tolist(), list(zip(*[np.atleast_1d(f[i]).tolist() for f in (hi, lo)]))))

    for s in range(0, ncols, 4):
        active = s < nsteps  # the lane is still in its loop
        for k in range(4):
            col = s + k + 1                 # columns after the border column
            valid = col <= nsteps           # a column of the lane's own text: warm-up or owned
            sym = T[:, s + k]
            kw = KW[k, ar, :, sym]          # [L, 32]: perm(chi[r], clo[r], sel)
            kex = kx[ar, :, sym] * F
            inj = (inj - step) & M32
            injx = injx - (insx * F + 1)
            dg = (V[:, :ROWS] - kw) & M32   # register r + 1's update candidate: old V[r] - kappa << 16
            dgx = VX[:, :ROWS] - kex
            check(dg, dgx, valid, "update candidate", col)
            m = np.minimum(V[:, 1:], dg)
            V = np.minimum.accumulate(np.concatenate([inj[:, None], m], axis=1), axis=1)
            VX = np.minimum.accumulate(np.concatenate([injx[:, None], np.minimum(VX[:, 1:], dgx)], axis=1), axis=1)
            check(V, VX, valid, "register", col)
            check(inj, injx, valid, "inj", col)
            u = u + 1
            tt = (V[:, ROWS] - inj) & M32
            c = s32((tt & 0xFFFF0000) | (u & 0xFFFF))
            take = active & (u >= 0) & (u < cnt) & (c < s32(bestc & 0xFFFF0000))
            bestc = np.where(take, c & M32, bestc)
            bestt = np.where(take, tt, bestt)
            shi, slo = fields(VX[:, ROWS])
            ihi, ilo = fields(injx)
            thi, tlo = shi - ihi, slo - ilo
            owned = valid & (u >= 0) & (u < cnt)
            assert (tlo >= 0)[valid].all(), ("the sink row's start field is below inj's", col)
            assert (u <= 0xFFFF)[owned].all(), ("u fits 16 bits", col)
            assert ((s32(tt) >> 16 == thi) & ((tt & 0xFFFF) == tlo))[valid].all(), ("V[32] - inj", col)
            takex = owned & (thi < bhi)
            assert (take == takex).all(), ("the take rule", col, np.argwhere(take != takex)[:3].tolist())
            bhi, bu, blen = np.where(takex, thi, bhi), np.where(takex, u, bu), np.where(takex, tlo, blen)
        if (s & (REBASE - 1)) == REBASE - 4:
            inj = (inj + rebase) & M32
            V = (V + rebase[:, None]) & M32
            injx = injx + REBASE * insx * F
            VX = VX + (REBASE * insx * F)[:, None]
    # the join: atomicMin of D << 48 | end << 16 | (end - start) over a pair's lanes
    D32 = ((s32(bestt) >> 16) + pdel) & M32
    len32 = bestt & 0xFFFF
    end32 = (c0 + (bestc & 0xFFFF)) & M32
    Dx, endx = bhi + pdx, c0 + bu
    assert ((Dx >= 0) & (Dx <= 0xFFFF) & (blen >= 0) & (blen <= 0xFFFF) & (blen <= endx)).all()
    assert ((D32 == Dx) & (len32 == blen) & (end32 == endx)).all()
    keys = [(1 << 64) - 1] * npairs
    for i in range(L):
        key = ((int(D32[i]) << 48) | (int(end32[i]) << 16) | int(len32[i])) & ((1 << 64) - 1)
        keys[rec["pair"][i]] = min(keys[rec["pair"][i]], key)
    out = []
    for jn, jb in enumerate(jobs):  # decoded as sed_fit_search decodes them
        hits = []
        for q in range(len(jb.pats)):
            key = keys[pair_base[jn] + q]
            end, ln = (key >> 16) & M32, key & 0xFFFF
            hits.append(((key >> 48) / scale[jn], end - ln, end))
        out.append(hits)
    return out


def run_and_compare(jobs):
    for jb, got in zip(jobs, run_model(jobs)):
        want = oracle_fit(jb.plan, jb.pats, jb.texts)
        bad = [(q, g, w) for q, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (jb.name, bad[:3])


def _patterns(rng, K):
    return [rng.integers(0, K, size=P).astype(np.uint8) for P in (1, 31, 32)]


def test_perm_model():
    assert perm(0x07060504, 0x03020100, 0x0C000704) == 0x00000704
    assert perm(0xAABBCCDD, 0x11223344, 0x0D0C0304) == 0xFF0011DD


def test_cost_limit_tables_under_every_chunking():
    """The cost-limit tables, P in {1, 31, 32}, texts of 2100 symbols (16 rebases) with planted mutated copies, under
    chunk overrides W, W + 1, 255, 1024 and the automatic rule: no wrap anywhere, and the definition's hits."""
    jobs = []
    for name, plan in cost_limit_tables():
        rng = np.random.default_rng(len(name))
        pats = _patterns(rng, plan.K)
        texts = [planted_text(rng, plan.K, p, 2100) for p in pats]
        W = sedgpu.fit_plan(plan.costs(), {}, [32], [2100])["W"]
        for chunk in (W, W + 1, 255, 1024, 0):
            jobs.append(Job("%s/chunk %d" % (name, chunk), plan, {sedgpu.SED_OPT_FIT_CHUNK: chunk}, pats, texts))
    run_and_compare(jobs)


def test_zero_insert_zero_delete_and_eight_symbols():
    jobs = []
    rng = np.random.default_rng(88)
    for K in (6, 7, 8):
        plan = eight_symbol_table(K)
        pats = _patterns(rng, K)
        for p in pats:
            p[:K] = rng.permutation(K)[:len(p)]
        jobs.append(Job("K=%d" % K, plan, {}, pats, [planted_text(rng, K, p, 700) for p in pats]))
    unit = np.where(np.eye(4) > 0, 0.0, 1.5)
    for name, ins, dele in (("insert 0", 0, 2.5), ("delete 0", 1.25, 0), ("both 0", 0, 0)):
        plan = Plan(unit, ins, dele)
        pats = _patterns(rng, 4)
        for n in (0, 1, 127, 128, 129, 700):
            jobs.append(Job("%s n=%d" % (name, n), plan, {sedgpu.SED_OPT_FIT_CHUNK: 64},
                            pats, [planted_text(rng, 4, p[:n], n) if n else np.zeros(0, np.uint8) for p in pats]))
    run_and_compare(jobs)


def _largest_unsplit_text(plan):
    """The longest text the planner runs as one lane under insert = 0."""
    n = 65000
    while True:
        try:
            got = sedgpu.fit_plan(plan.costs(), {}, [32], [n + 1])
        except sedgpu.SedError:
            return n
        assert got["lanes"] == 1 and n < 70000
        n += 1


def test_longest_lanes():
    """The longest lanes the planner makes: the largest one-lane text under insert = 0, whatever the planner says it is,
    and the forced split of longer texts under the automatic rule (lanes of chunk + lead columns).  The start field
    reaches its last values here; a planner that admitted a few more columns would borrow out of it."""
    rng = np.random.default_rng(65535)
    sub = np.where(np.eye(4) > 0, 0.0, 2.0)
    zero = Plan(sub, 0, 1)
    n0 = _largest_unsplit_text(zero)
    p = rng.integers(0, 4, size=32).astype(np.uint8)
    t0 = rng.integers(0, 4, size=n0).astype(np.uint8)
    t0[n0 - 32:] = p  # an exact copy ends at the last column
    jobs = [Job("insert 0, n=%d" % n0, zero, {}, [p], [t0])]
    split = Plan(sub, 1, 4)
    texts = []
    for n in (65535, 65536, 70001):
        t = rng.integers(0, 4, size=n).astype(np.uint8)
        t[n - 32:] = p
        texts.append(t)
    # 2 waves on every SIMD keep one lane per text (the automatic rule), so only the span limit splits these
    job = Job("forced split", split, {}, [p] * 3, texts, filler=(1 << 17, 1, 0))
    got = sedgpu.fit_plan(split.costs(), {}, job.len_p, job.len_t)
    assert got["lanes"] == 6 + (1 << 17) and got["chunk"] > 60000
    jobs.append(job)
    run_and_compare(jobs)
    # what include/sed.h documents: a text of up to 65534 symbols as one chunk, chunks of at most 65535 - W columns
    assert n0 == 65534 and got["chunk"] + got["W"] + 3 == 65535
