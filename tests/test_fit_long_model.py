"""CPU: the wave kernel of long fit search (sed_fit_long.hip) restated word op by word op in numpy: 64 lanes of R
registers, the skew (lane l computes column t - l at step t), both hand-overs through wave_shr:1 (the boundary key and
the perm selector), the top row's diagonal from the word received the step before, and the per-lane rebase after the
lane's own columns 128, 256, ...  It runs on the planner's own wave records and parameter words
(sedgpu.FitIndex.long_lanes / long_plan).  As tests/test_fit_model.py does, every value is carried twice: as the 32-bit
word the kernel holds and as two unbounded fields (D field, start field) updated with no carry between them, the
unbounded side taking its update addends from the cost table and its text symbol from a hand-over of its own.  At every
step, for every lane that computes a column of its text, the model asserts that each register, the received boundary key,
each update candidate and row 0's key equal their fields packed, each field within 0..65535; that lane 63's
V[R - 1] - inj has no borrow and decodes to the unbounded D and end - start; and at the end that the 64-bit join of the
waves is oracle.fit's hit, exactly."""
import numpy as np
import pytest

import sedgpu
from fit_envelope import Plan, cost_limit_tables, eight_symbol_table, oracle_fit, planted_text
from test_fit_model import M32, perm, s32

REBASE = 128    # FIT_REBASE
F = 1 << 32


class Job:
    """Queries x texts under a cost model and options.  filler = that many more empty texts go to the planner after the
    real ones (enough pairs to change the chunk rule); the model leaves their waves out."""

    def __init__(self, name, plan, options, pats, texts, filler=0):
        self.name, self.plan, self.options, self.pats, self.texts = name, plan, options, pats, texts
        self.len_p, self.len_t = [len(p) for p in pats], [len(t) for t in texts] + [0] * filler


def fields(X):
    hi = (X + (1 << 31)) >> 32
    return hi, X - hi * F


def run_waves(R, waves):
    """waves: dicts (rec: the wave's record, par, S, plan, pat, text).  Returns each wave's (pair key, 64-bit key)."""
    Wn = len(waves)
    ROWS = 64 * R
    g = lambda k: np.array([w["rec"][k] for w in waves], np.int64)
    nsteps, lead, cnt, c0, plen, tw = g("nsteps"), g("lead"), g("cnt"), g("c0"), g("plen"), g("tw")
    assert (cnt >= 1).all() and (cnt <= 0xFFFF).all()
    ins32 = np.array([w["par"]["ins"] for w in waves], np.int64)
    del32 = np.array([w["par"]["del"] for w in waves], np.int64)
    clo = np.zeros((Wn, 64, R), np.int64)
    chi = np.zeros((Wn, 64, R), np.int64)
    kap = np.zeros((Wn, 64, R, 9), np.int64)   # the unbounded side's addends (symbol 8: no column yet, kappa 0)
    insx, delx = np.zeros(Wn, np.int64), np.zeros(Wn, np.int64)
    ncols = int(((nsteps.max() + 63 + 3) // 4) * 4)
    T = np.zeros((Wn, ncols + 4), np.int64)
    for i, w in enumerate(waves):
        S, pl = w["S"], w["plan"]
        sub, I, D = pl.sub * S, pl.ins * S, pl.dele * S
        assert I == int(I) and D == int(D) and (sub == np.floor(sub)).all()
        assert (w["par"]["ins"], w["par"]["del"]) == (int(I), int(D))
        insx[i], delx[i] = int(I), int(D)
        tab = np.zeros((9, 2), np.int64)
        tab[:8] = w["par"]["row"]
        kp = np.zeros((9, 8), np.int64)
        kp[:pl.K, :pl.K] = I + D - np.minimum(sub, I + D)
        code = np.full(ROWS, 8, np.int64)       # the pattern record: 64 R codes, right-aligned, code 8 in front
        code[ROWS - len(w["pat"]):] = w["pat"]
        code = code.reshape(64, R)              # lane l reads bytes l R .. l R + R - 1
        clo[i], chi[i], kap[i, :, :, :8] = tab[code, 0], tab[code, 1], kp[code]
        # the wave reads whole words while s < nsteps, zeros after (the kernel loads no word past the chunk's last)
        nw = (int(nsteps[i]) + 3) // 4 * 4
        seg = np.asarray(w["text"], np.int64)[4 * int(tw[i]):4 * int(tw[i]) + nw]
        T[i, :len(seg)] = seg
    lane = np.arange(64)[None, :]
    pdel = (plen * del32) & M32
    rebase = ((REBASE * ins32) << 16) & M32
    step = ((ins32 << 16) + 1) & M32
    inj0 = (((pdel << 16) + rebase) & M32) | 0xFFFF
    pdx = plen * delx
    injx0 = (pdx + REBASE * insx) * F + 0xFFFF
    rbx = REBASE * insx * F
    col = lambda a: np.repeat(a[:, None], 64, axis=1)
    inj, injx = col(inj0), col(injx0)
    V = np.repeat(inj[:, :, None], R, axis=2)
    VX = np.repeat(injx[:, :, None], R, axis=2)
    top_prev, top_prevx, bottom, bottomx = inj.copy(), injx.copy(), inj.copy(), injx.copy()
    selv = np.full((Wn, 64), 0x0C0C0C0C, np.int64)
    sym = np.full((Wn, 64), -1, np.int64)       # the unbounded side's symbol of the lane's column; -1: kappa 0
    j = np.repeat(-lane, Wn, axis=0).astype(np.int64)
    bestd = np.where(lead == 0, pdel, 0x10000).astype(np.int64)
    bestu, bestt = np.zeros(Wn, np.int64), np.zeros(Wn, np.int64)
    bdx = np.where(lead == 0, pdx, 1 << 40).astype(np.int64)
    bux, blx = np.zeros(Wn, np.int64), np.zeros(Wn, np.int64)
    # A column's selector as lane 0 builds it from the text word, the word's other bytes all ones to show they do not
    # matter, and perm(chi, clo, selector) for each of the eight symbols and for the initial selector (index 8)
    SEL = np.array([[int(perm((M32 ^ (0xFF << (8 * k))) | (b << (8 * k)), 0x0C0C0C0C, (4 + k) << 16)) for b in range(8)]
                    + [0x0C0C0C0C] for k in range(4)], np.int64)
    assert (SEL[:, :8] == SEL[0, :8]).all()
    KW = np.stack([perm(chi, clo, int(SEL[0, b])) for b in range(9)], axis=3)
    total = nsteps + 63

    def check(W32, X, valid, what, t):
        hi, lo = fields(X)
        bad = (hi < 0) | (hi > 0xFFFF) | (lo < 0) | (lo > 0xFFFF) | (W32 != ((hi << 16) | lo))
        bad = bad & (valid if bad.ndim == 2 else valid[:, :, None])
        if bad.any():
            at = np.argwhere(bad)[0].tolist()
            i = at[0]
            raise AssertionError("%s: R %d wave %s (P %d c0 %d lead %d cnt %d nsteps %d) step %d at %s: word %#x fields %s"
                                 % (what, R, waves[i]["name"], plen[i], c0[i], lead[i], cnt[i], nsteps[i], t, at,
                                    int(W32[tuple(at)]), (int(hi[tuple(at)]), int(lo[tuple(at)]))))

    for s in range(0, ncols, 4):
        running = (s < total) & (nsteps > 0)     # the wave is still in its loop
        if not running.any():
            break
        live = s < nsteps                        # its text word of these four columns is loaded
        for k in range(4):
            t = s + k + 1
            tsym = np.where(live, T[:, s + k], 0)
            sel0 = SEL[k, tsym]
            j = j + 1
            act = j >= 1
            valid = act & (j <= nsteps[:, None]) & running[:, None]
            inj = np.where(act, (inj - step[:, None]) & M32, inj)
            injx = np.where(act, injx - (insx * F + 1)[:, None], injx)
            up = np.concatenate([inj[:, :1], bottom[:, :-1]], axis=1)
            upx = np.concatenate([injx[:, :1], bottomx[:, :-1]], axis=1)
            selv = np.concatenate([sel0[:, None], selv[:, :-1]], axis=1)
            sym = np.concatenate([tsym[:, None], sym[:, :-1]], axis=1)
            si = np.where(sym < 0, 8, sym)
            assert (selv == SEL[0, si]).all(), ("the handed selector", t)
            kw = np.take_along_axis(KW, si[:, :, None, None], axis=3)[..., 0]   # perm(chi[r], clo[r], selv)
            kx = np.take_along_axis(kap, si[:, :, None, None], axis=3)[..., 0]
            above_old = np.concatenate([top_prev[:, :, None], V[:, :, :-1]], axis=2)
            above_oldx = np.concatenate([top_prevx[:, :, None], VX[:, :, :-1]], axis=2)
            dg = (above_old - kw) & M32
            dgx = above_oldx - kx * F
            check(up, upx, valid, "received boundary key", t)
            check(dg, dgx, valid, "update candidate", t)
            V = np.minimum.accumulate(np.concatenate([up[:, :, None], np.minimum(V, dg)], axis=2), axis=2)[:, :, 1:]
            VX = np.minimum.accumulate(np.concatenate([upx[:, :, None], np.minimum(VX, dgx)], axis=2), axis=2)[:, :, 1:]
            check(V, VX, valid, "register", t)
            check(inj, injx, valid, "inj", t)
            top_prev, top_prevx = up, upx
            bottom, bottomx = V[:, :, R - 1], VX[:, :, R - 1]
            # lane 63 reports
            tt = (V[:, 63, R - 1] - inj[:, 63]) & M32
            u = j[:, 63] - lead
            d = ((tt >> 16) + pdel) & 0xFFFF
            own = running & act[:, 63] & (u >= 0) & (u < cnt)
            take = own & (d < bestd)
            bestd, bestu, bestt = np.where(take, d, bestd), np.where(take, u, bestu), np.where(take, tt, bestt)
            shi, slo = fields(VX[:, 63, R - 1])
            ihi, ilo = fields(injx[:, 63])
            dx, lx = shi - ihi + pdx, slo - ilo
            v63 = valid[:, 63]
            assert (lx >= 0)[v63].all(), ("the sink row's start field is below inj's", t)
            assert ((dx >= 0) & (dx <= 0xFFFF))[v63].all(), ("D outside 16 bits", t)
            assert ((d == dx) & ((tt & 0xFFFF) == lx))[v63].all(), ("V[R - 1] - inj", t)
            assert (own <= v63).all() and (u <= 0xFFFF)[own].all()
            takex = own & (dx < bdx)
            assert (take == takex).all(), ("the take rule", t)
            bdx, bux, blx = np.where(takex, dx, bdx), np.where(takex, u, bux), np.where(takex, lx, blx)
            rb = act & ((j & (REBASE - 1)) == 0)
            inj = np.where(rb, (inj + rebase[:, None]) & M32, inj)
            top_prev = np.where(rb, (top_prev + rebase[:, None]) & M32, top_prev)
            V = np.where(rb[:, :, None], (V + rebase[:, None, None]) & M32, V)
            injx = np.where(rb, injx + rbx[:, None], injx)
            top_prevx = np.where(rb, top_prevx + rbx[:, None], top_prevx)
            VX = np.where(rb[:, :, None], VX + rbx[:, None, None], VX)
    assert ((bestd == bdx) & (bestu == bux) & ((bestt & 0xFFFF) == blx) & (bestd <= 0xFFFF) & (blx <= c0 + bux)).all()
    return [(int(bestd[i]) << 48) | (int(c0[i] + bestu[i]) << 16) | int(bestt[i] & 0xFFFF) for i in range(Wn)]


def run_and_compare(jobs):
    by_rows = {}
    for jn, jb in enumerate(jobs):
        costs = jb.plan.costs()
        plan = sedgpu.FitIndex.long_plan(costs, jb.options, jb.len_p, jb.len_t)
        lanes, par = sedgpu.FitIndex.long_lanes(costs, jb.options, jb.len_p, jb.len_t)
        D = len(jb.len_t)
        for i in range(len(lanes["pair"])):
            q, d = divmod(int(lanes["pair"][i]), D)
            if d >= len(jb.texts):
                continue
            by_rows.setdefault(int(plan["rows"][q]), []).append(
                {"rec": {k: int(v[i]) for k, v in lanes.items()}, "par": par, "S": plan["scale"], "plan": jb.plan,
                 "pat": jb.pats[q], "text": jb.texts[d], "job": jn, "name": "%s q%d d%d" % (jb.name, q, d)})
    keys = [dict() for _ in jobs]
    for R, waves in sorted(by_rows.items()):
        for w, key in zip(waves, run_waves(R, waves)):
            kd = keys[w["job"]]
            kd[w["rec"]["pair"]] = min(kd.get(w["rec"]["pair"], (1 << 64) - 1), key)
    for jn, jb in enumerate(jobs):
        D = len(jb.len_t)
        S = sedgpu.FitIndex.long_plan(jb.plan.costs(), jb.options, jb.len_p, jb.len_t)["scale"]
        want = oracle_fit(jb.plan, [p for p in jb.pats for _ in jb.texts], [t for _ in jb.pats for t in jb.texts])
        for n, w in enumerate(want):
            pair = n // len(jb.texts) * D + n % len(jb.texts)
            key = keys[jn][pair]
            end, ln = (key >> 16) & M32, key & 0xFFFF
            assert ((key >> 48) / S, end - ln, end) == w, (jb.name, divmod(pair, D), key, w)
    return by_rows


def _pat(rng, K, P):
    return rng.integers(0, K, size=P).astype(np.uint8)


def test_every_rows_per_lane_and_chunking():
    """Every R, automatic and forced, P on both sides of each 64 R, chunks 8, 72 and automatic; texts around the
    63-step skew and past two rebases, with planted mutated copies."""
    rng = np.random.default_rng(2048)
    sub = np.where(np.eye(4) > 0, 0.0, 1.5)
    plan = Plan(sub, 1.0, 1.25)
    jobs = []
    pats = [_pat(rng, 4, P) for P in (1, 33, 128, 129, 257)]
    texts = [planted_text(rng, 4, pats[3], 300), planted_text(rng, 4, pats[1], 64), np.zeros(0, np.uint8),
             planted_text(rng, 4, pats[0], 1)]
    for chunk in (8, 72, 0):
        jobs.append(Job("chunk %d" % chunk, plan, {sedgpu.SED_OPT_FIT_CHUNK: chunk}, pats, texts))
    for R in (2, 4, 8, 16, 32):
        jobs.append(Job("forced R %d" % R, plan, {sedgpu.SED_OPT_FIT_ROWS: R, sedgpu.SED_OPT_FIT_CHUNK: 200},
                        [p for p in pats if len(p) <= 64 * R][:3], texts[:2]))
    big = [_pat(rng, 4, P) for P in (1025, 2048)]
    jobs.append(Job("R 32", plan, {}, big, [planted_text(rng, 4, big[0][:300], 400, copies=1)]))
    rows = run_and_compare(jobs)
    assert sorted(rows) == [2, 4, 8, 16, 32]


def test_tables_on_each_limit():
    """The cost-limit tables of the short envelope, the eight-symbol table, zero insert and zero delete, and tables on
    the D-field limit P delete S + 128 insert S = 65535 (with insert = 0: D itself reaches 65535)."""
    jobs = []
    for name, plan in cost_limit_tables():
        rng = np.random.default_rng(len(name))
        P = 100
        if 128 * plan.ins + P * plan.dele > 65535:   # (scale 1 tables; i1_d254: 25400 + 128)
            P = int((65535 - 128 * plan.ins) // plan.dele)
        pats = [_pat(rng, plan.K, P), _pat(rng, plan.K, 31)]
        jobs.append(Job(name, plan, {sedgpu.SED_OPT_FIT_CHUNK: 72}, pats, [planted_text(rng, plan.K, pats[0], 400)]))
    rng = np.random.default_rng(7)
    p8 = _pat(rng, 8, 70)
    p8[:8] = rng.permutation(8)
    jobs.append(Job("K=8", eight_symbol_table(8), {}, [p8], [planted_text(rng, 8, p8, 500)]))
    unit = np.where(np.eye(4) > 0, 0.0, 1.5)
    for name, ins, dele in (("insert 0", 0, 2.5), ("delete 0", 1.25, 0), ("both 0", 0, 0)):
        p = _pat(rng, 4, 90)
        jobs.append(Job(name, Plan(unit, ins, dele), {sedgpu.SED_OPT_FIT_CHUNK: 64}, [p],
                        [planted_text(rng, 4, p, n) for n in (127, 128, 129, 300)]))
    sub = np.where(np.eye(4) > 0, 0.0, 255.0)
    # 257 * 255 = 65535 with insert = 0; (65535 - 128 * 3) // 255 = 255 rows of delete 255 beside insert 3
    for name, ins, dele, P in (("D = 65535", 0, 255, 257), ("P del + 128 ins", 3, 252, 258)):
        assert P * dele + 128 * ins <= 65535 < (P + 1) * dele + 128 * ins
        p = _pat(rng, 4, P)
        t = planted_text(rng, 4, p, 400, copies=1)
        jobs.append(Job(name, Plan(sub, ins, dele), {}, [p], [t, (3 - t[:20]).astype(np.uint8)]))
    run_and_compare(jobs)


def test_longest_waves():
    """The longest waves the planner makes: the largest one-chunk text under insert = 0, and the forced split of a longer
    text under the automatic rule (chunk + W + 3 = 65535).  The start field reaches its last values here."""
    rng = np.random.default_rng(65535)
    sub = np.where(np.eye(4) > 0, 0.0, 2.0)
    p = _pat(rng, 4, 33)
    zero = Plan(sub, 0, 1)
    with pytest.raises(sedgpu.SedError):
        sedgpu.FitIndex.long_plan(zero.costs(), {}, [33], [65535])
    t0 = rng.integers(0, 4, size=65534).astype(np.uint8)
    t0[-33:] = p
    split = Plan(sub, 1, 4)
    t1 = rng.integers(0, 4, size=70001).astype(np.uint8)
    t1[-33:] = p
    # 2048 pairs keep one chunk per text (the automatic rule), so only the span limit splits the long one
    got = sedgpu.FitIndex.long_plan(split.costs(), {}, [33], [70001] + [0] * 2047)
    assert got["chunk"] + got["W"] + 3 == 65535 and got["lanes"] == 2 + 2047
    run_and_compare([Job("insert 0, n=65534", zero, {}, [p], [t0]), Job("forced split", split, {}, [p], [t1], filler=2047)])
