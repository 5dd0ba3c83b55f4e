"""Canonical paths built to cross the seams of the tracebacks, shared by the CPU tests (tests/test_path_cases.py) and the
GPU tests (tests/test_gpu_path_envelope.py).  Random and mutated pairs give paths that hug the diagonal and turn every
few cells; a traceback breaks where a path does one thing for a long time or at an exact place.  Each family here builds
its pairs from segments, so that the canonical path is known before any DP runs:

  M(k)  a matched block: the same random text of k symbols on both sides, over the matched symbols only;
  I(k)  an inserted run: k times the insert symbol on str2 only (the matched symbols lack it);
  D(k)  a deleted run: k times the delete symbol on str1 only.

A pair with runs of one kind has exactly one optimal alignment under every table whose mismatches cost more than 0 (any
alignment needs that many indels, and str2 less its insert symbols is str1), so its claim holds whatever the table.
Where insert and delete runs alternate (staircase) the optimal alignment may instead pay mismatches across a block: the
(family, table) combinations where it does are in DROPPED, by name.

A family is (rng, R, SW, sym) -> [(a, b, claim)], a and b strings.  R: rows per lane; SW: the layout's lanes (64, or 16
for the fp64 segments), so a stripe is SW R rows, a chunk SW columns, a tile min(64, SW) rows, a band R rows.  `claim`
says in data what the canonical path must do: {"family", "what", "runs": [{"op", "run", "start": (i, j), "end": (i, j)}],
"through": [(i, j)], "avoid": [(i, j)], "script": the whole script or None}; (i, j) = (symbols of str1, of str2)
consumed.  tests/test_path_cases.py asserts every claim on the oracle's script.  Everything is seeded and device-free."""
import json
import os

import numpy as np

from band_cases import GOLDEN, TABLES as BAND_TABLES

IUPAC = "AGCUYRWSKMDVHBN"
with open(os.path.join(GOLDEN, "g8_cost_tables.json")) as _f:
    _G8 = json.load(_f)["tables"]

# ---- tables: the integer ones from band_cases.TABLES (not retyped), the fp64 ones from the golden files ----
INT_TABLES = {name: BAND_TABLES[name] for name in ("costs.json", "user_costs.json", "sum", "gui_int")}
with open(os.path.join(GOLDEN, "costs.json")) as _f:
    F64_TABLES = {"costs.json": json.load(_f), "frac_indel": _G8["frac_indel"], "int_literals": _G8["int_literals"]}
FACTORS = ("costs.json", "user_costs.json")  # dot keys (band_cases.FACTORABLE); `sum` and `gui_int` run distance keys

# (matched symbols, insert symbol, delete symbol) per table.  The staircase needs mismatches against the run symbols
# that cost more than half of insert + delete: gui_int A, G against U cost 4 and 2, C against A, G 3 and 4, of 4;
# frac_indel A, C against U cost 1 and G against A, C 2, of 1.49.
SYM = {"int": ("AC", "U", "G"), "gui_int": ("AG", "U", "C"), "f64": ("ACYRWSKM", "U", "G"), "frac_indel": ("AC", "U", "G")}


def symbols(table, f64=False):
    return SYM.get(table, SYM["f64" if f64 else "int"])


# (family, table): the claim does not hold, so the combination runs nowhere.  Reasons, from the costs: a staircase step
# I(p) M(p) D(p) costs p (insert + delete) as indels and at most 2 p mismatches as updates, which is no dearer, and
# shorter, when a mismatch costs at most (insert + delete) / 2: costs.json 1 of 2, user_costs.json <= 2 of 5,
# int_literals <= 2 of 5.  `ell` is defined by the `sum` table (every mismatch = insert + delete) alone.
DROPPED = (("staircase", "costs.json"), ("staircase", "user_costs.json"), ("staircase", "int_literals"))


# ---- segments -> a pair and the runs of its path ----
def M(k):
    return ("M", k)


def I(k):  # noqa: E743
    return ("I", k)


def D(k):
    return ("D", k)


def assemble(rng, segs, sym, family, what, through=(), avoid=()):
    """(a, b, claim) of a segment list.  Neighbouring matched blocks never meet a run symbol, so every I / D segment is
    one maximal run of the script."""
    matched, x, y = sym
    a, b, runs, i, j = [], [], [], 0, 0
    for kind, k in segs:
        if k <= 0:
            continue
        if kind == "M":
            t = "".join(rng.choice(list(matched), size=k))
            a.append(t)
            b.append(t)
            i, j = i + k, j + k
        elif kind == "I":
            b.append(x * k)
            runs.append({"op": "insert", "run": k, "start": (i, j), "end": (i, j + k)})
            j += k
        else:
            a.append(y * k)
            runs.append({"op": "delete", "run": k, "start": (i, j), "end": (i + k, j)})
            i += k
    claim = {"family": family, "what": what, "runs": runs, "through": list(through), "avoid": list(avoid), "script": None}
    return "".join(a), "".join(b), claim


class Geo:
    def __init__(self, R, SW):
        self.R, self.SW, self.rows, self.chunk, self.tile, self.G = R, SW, SW * R, SW, min(64, SW), 64 // R


# ---- the families ----
def long_insert(rng, R, SW, sym=SYM["int"]):
    """One insert run of 3 chunks + 5 columns (the checkpoint walk leaves its tile through the left edge visit after
    visit; the per-cell walk crosses chunks and groups moving left only), on the first and the last row of a stripe, the
    first and the last row of a tile inside a stripe, and the middle of a band."""
    g = Geo(R, SW)
    run = 3 * g.chunk + 5
    rows = {"first row of stripe 1": g.rows + 1, "last row of stripe 0": g.rows, "last row of stripe 1": 2 * g.rows,
            "first row of a tile": g.rows + g.tile + 1, "last row of a tile": g.rows + g.tile,
            "middle of a band": g.rows + 2 * R + R // 2 + 1}
    if g.tile == g.rows:  # (a stripe of one tile: the tile rows are the stripe rows)
        rows = {k: v for k, v in rows.items() if "tile" not in k}
    return [assemble(rng, [M(i), I(run), M(70)], sym, "long_insert", "%s: row %d" % (what, i))
            for what, i in rows.items()]


def long_delete(rng, R, SW, sym=SYM["int"], deep=0):
    """One delete run of a stripe + a tile + 3 rows in one column (band, tile and stripe borders, the hand-off rows and
    planes, the composed band maps): columns 1, 63, 64, 65, the last one, and 257, past the fp64 ring of 256.  deep: that
    many stripes more in the run, so that it crosses 1 + deep stripe borders."""
    g = Geo(R, SW)
    run = (1 + deep) * g.rows + g.tile + 3
    out = [assemble(rng, [M(c), D(run), M(2 if c == 257 else 70)], sym, "long_delete", "column %d" % c)
           for c in (1, 63, 64, 65, 257)]
    out.append(assemble(rng, [M(100), D(run)], sym, "long_delete", "the last column, 100"))
    return out


def long_delete_m(rng, R, SW, m, sym=SYM["int"]):
    """long_delete's run in the last column of a pair with m columns (the fp64 SPLIT ring at m = 255, 256, 257)."""
    g = Geo(R, SW)
    return assemble(rng, [M(m), D(g.rows + g.tile + 3)], sym, "long_delete", "the last column, %d" % m)


def corner(rng, R, SW, sym=SYM["int"], deep=0):
    """A matched block ends, and a run of 2 starts, exactly on a tile corner inside a stripe and on a stripe
    corner (i % 64 == 0 and j % 64 == 0), and one row or one column to either side of it.  The block starts from a
    border run that sets its diagonal.  deep: the first two corners that many stripes further down and right."""
    g = Geo(R, SW)
    t, r1 = g.tile, (1 + deep) * g.rows
    corners = {"tile corner": (r1 + t, r1 + 2 * t) if g.tile < g.rows else None, "stripe corner": (r1, max(r1 - t, t)),
               "stripe corner on the diagonal": (2 * g.rows, 2 * g.rows)}
    out = []
    for what, ij in corners.items():
        if ij is None:
            continue
        for di, dj in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            i, j = ij[0] + di, ij[1] + dj
            lead = [I(j - i)] if j > i else [D(i - j)]
            # (the turn: two rows down, or beside a row miss two columns right, which keeps clear of the corner)
            turn = [I(2), M(40), D(2)] if di else [D(2), M(40), I(2)]
            segs = lead + [M(min(i, j))] + turn + [M(30)]
            miss = (di, dj) != (0, 0)
            out.append(assemble(rng, segs, sym, "corner", "%s (%d, %d) %+d row %+d column" % (what, ij[0], ij[1], di, dj),
                                through=[(i, j)], avoid=[ij] if miss else []))
    return out


def border_finish(rng, R, SW, sym=SYM["int"]):
    """The path leaves column 1 at a row past the second stripe, or row 1 at a column past the third chunk: from there to
    the origin the script is one run (the c == 0 walk, then the trailing emit loops for hundreds of ops)."""
    g = Geo(R, SW)
    return [assemble(rng, [D(2 * g.rows + 5), M(60)], sym, "border_finish", "column 1 at row %d" % (2 * g.rows + 6)),
            assemble(rng, [I(3 * g.chunk + 7), M(g.rows + 9)], sym, "border_finish",
                     "row 1 at column %d" % (3 * g.chunk + 8)),
            assemble(rng, [D(g.rows + 1), M(1)], sym, "border_finish", "column 1 at the last row"),
            assemble(rng, [I(g.chunk + 1), M(1)], sym, "border_finish", "row 1 at the last column")]


def staircase(rng, R, SW, sym=SYM["int"], deep=0):
    """Insert, delete, insert runs of p symbols with matched blocks of p between (six turns), p = 63, 64, 65: the turn
    drifts across every phase of a chunk.  The stairs straddle the first stripe border (deep: the one that many
    further down)."""
    g = Geo(R, SW)
    return [assemble(rng, [M(max(p, (1 + deep) * g.rows - 2 * p)), I(p), M(p), D(p), M(p), I(p), M(p)], sym, "staircase",
                     "p = %d" % p) for p in (63, 64, 65)]


def ell(rng, R, SW, sym=SYM["int"]):
    """One homopolymer against another: under `sum` every cell is a three-way tie in cost, so the fewest-ops rule and the
    insert < delete < update order alone decide the path: min(n, m) updates from the origin, then one run to the sink.
    n < m, n > m and n == m on both sides of a stripe border."""
    g = Geo(R, SW)
    x, y = sym[0][0], sym[0][1]
    out = []
    for n, m in ((g.rows - 1, g.rows + 40), (g.rows + 1, g.rows + 40), (g.rows + 40, g.rows - 1), (g.rows + 40, g.rows + 1),
                 (g.rows, g.rows), (g.rows + 1, g.rows + 1), (g.rows + 1, 20), (20, g.rows + 1), (17, 30), (30, 17)):
        k = min(n, m)
        run = {"op": "insert" if m > n else "delete", "run": abs(n - m), "start": (k, k), "end": (n, m)}
        out.append((x * n, y * m, {"family": "ell", "what": "%d x %d" % (n, m), "runs": [run] if n != m else [],
                                   "through": [(k, k)], "avoid": [],
                                   "script": "u" * k + ("i" if m > n else "d") * abs(n - m)}))
    return out


def thin(rng, R, SW, sym=SYM["int"]):
    """m = 1, 2, G - 1, G against a str1 of a stripe + a tile + 3 rows, and n = 1, R, R + 1 against a str2 of 3 chunks + 5
    columns: the matched block sits a third of the way along the long side."""
    g = Geo(R, SW)
    long_n, long_m = g.rows + g.tile + 3, 3 * g.chunk + 5
    out = []
    for m in sorted({1, 2, g.G - 1, g.G} - {0}):
        k = (long_n - m) // 3
        out.append(assemble(rng, [D(k), M(m), D(long_n - m - k)], sym, "thin", "m = %d" % m))
    for n in sorted({1, R, R + 1}):
        k = (long_m - n) // 3
        out.append(assemble(rng, [I(k), M(n), I(long_m - n - k)], sym, "thin", "n = %d" % n))
    return out


FAMILIES = {"long_insert": long_insert, "long_delete": long_delete, "corner": corner, "border_finish": border_finish,
            "staircase": staircase, "ell": ell, "thin": thin}


def seed(*parts):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("/".join(map(str, parts))))


def members(family, table, R, SW=64, f64=False, **kw):
    """[(a, b, claim)] of one family under one table; nothing for a dropped combination.  kw: the family's own (deep)."""
    if (family, table) in DROPPED or (family == "ell" and (f64 or table != "sum")):
        return []
    rng = np.random.default_rng(seed(family, table, R, SW, *sorted(kw.items())))
    return FAMILIES[family](rng, R, SW, symbols(table, f64), **kw)


def batch(table, R, SW=64, f64=False, families=tuple(FAMILIES), keep=None):
    """Every family's members under a table, as one list; keep(a, b, claim) filters."""
    out = [x for fam in families for x in members(fam, table, R, SW, f64)]
    return [x for x in out if keep is None or keep(*x)]


def combinations():
    """Every (family, table, f64) the GPU file could run, dropped ones included (the cap of one in eight)."""
    out = [(fam, t, False) for fam in FAMILIES for t in INT_TABLES if fam != "ell" or t == "sum"]
    return out + [(fam, t, True) for fam in FAMILIES for t in F64_TABLES if fam != "ell"]


# ---- a script against its claim ----
def path_cells(script):
    """The cells (i, j) of a script "idu...", origin first."""
    cells, i, j = [(0, 0)], 0, 0
    for op in script:
        i, j = i + (op != "i"), j + (op != "d")
        cells.append((i, j))
    return cells


def claim_errors(script, claim):
    """What of a claim the script does not do (empty: it holds).  A run must be maximal: exactly `run` ops of its kind
    from `start` to `end`, with another op before and after."""
    cells = path_cells(script)
    at = {c: k for k, c in enumerate(cells)}
    bad = []
    if claim["script"] is not None and script != claim["script"]:
        bad.append("script")
    for r in claim["runs"]:
        ch = r["op"][0]
        k0, k1 = at.get(tuple(r["start"])), at.get(tuple(r["end"]))
        if k0 is None or k1 is None or k1 - k0 != r["run"] or script[k0:k1] != ch * r["run"]:
            bad.append(("run", r))
        elif (k0 > 0 and script[k0 - 1] == ch) or (k1 < len(script) and script[k1] == ch):
            bad.append(("run not maximal", r))
    bad += [("through", c) for c in claim["through"] if tuple(c) not in at]
    bad += [("avoid", c) for c in claim["avoid"] if tuple(c) in at]
    return bad


def longest_run(script):
    best = cur = 0
    for k, op in enumerate(script):
        cur = cur + 1 if k and op == script[k - 1] and op != "u" else (op != "u")
        best = max(best, cur)
    return best


# ---- the batches of tests/test_gpu_path_envelope.py, device-free so that tests/test_path_cases.py can place them ----
def pad_pairs(n, tag, alphabet="ACGU", lo=33, hi=60):
    """n short random pairs (str2 past the lane kernels' 32 columns) that fill a batch up to a pair count."""
    rng = np.random.default_rng(seed("pad", tag))
    return [("".join(rng.choice(list(alphabet), size=int(rng.integers(lo, hi)))),
             "".join(rng.choice(list(alphabet), size=int(rng.integers(lo, hi))))) for _ in range(n)]


def pairs_of(items):
    return [(a, b) for a, b, _ in items]


def one_stripe(R, SW=64):
    return lambda a, b, claim: 1 <= len(a) <= SW * R and len(b) >= 1


def chain_batch(table, R):
    """CHAIN runs pairs of one stripe: the members of at most 64 R rows of every family built at R, and of every family
    built with the 64-row tile in the stripe's place (R = 1: rows 64, 65 and 128, tile borders inside the stripe)."""
    return batch(table, 1, keep=one_stripe(R)) + batch(table, R, keep=one_stripe(R))


def split_batch(table, R=4):
    """Integer SPLIT: long_delete at columns 64 and 65, the staircase and the corners, each one stripe deeper (deep = 1)
    so that every pair has three stripes or more: the band map and compose kernels leave shorter pairs to the emit
    kernel's single segment.  The delete runs (2 stripes + a tile + 3 rows from row 64 or 65) cross both stripe borders,
    the stairs straddle the second, and the corners lie on it and on the first tile border below it."""
    out = [x for fam in ("long_delete", "staircase", "corner") for x in members(fam, table, R, deep=1)]
    return [x for x in out if x[2]["family"] != "long_delete" or x[2]["what"] in ("column 64", "column 65")]


def lane_batch(table, R=4):
    """The thin and ell members the lane kernels take (n <= 512, m <= 32), built at a stripe of 16 R rows: a batch of
    few pairs with a str1 past 256 symbols would go SPLIT."""
    return batch(table, R, SW=16, families=("thin", "ell"), keep=lambda a, b, c: len(a) <= 256 and 1 <= len(b) <= 32)


def window_batch(table, R=4):
    """One member of each family, padded with short random pairs to 70 pairs (the window traceback's 65..256)."""
    items = [members(fam, table, R)[:1] for fam in FAMILIES]
    pairs = pairs_of([x for it in items for x in it])
    return pairs + pad_pairs(70 - len(pairs), "window " + table)


def f64_split_batch(table, R):
    """fp64 SPLIT: every family at a stripe of 64 R rows, and long_delete in the last column of m = 255, 256, 257."""
    items = batch(table, R, f64=True)
    rng = np.random.default_rng(seed("ring", table, R))
    return items + [long_delete_m(rng, R, 64, m, symbols(table, True)) for m in (255, 256, 257)]
