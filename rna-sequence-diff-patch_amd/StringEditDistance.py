"""StringEditDistance — drop-in replacement for the reference module of the
same name (plsakr/rna-sequence-diff-patch, StringEditDistance.py), backed by
the MI355X engine (libsed.so, HIP kernels for gfx950).

Same names, same argument meaning, same globals and the same exceptions, so
gui.py, IRMethods.py, timing.py and performance.py run unchanged with this
directory on sys.path (or as the CWD):

    default_costs, user_costs, reload_user_costs()       StringEditDistance.py:6-27
    Edge, Node                                            :31-71
    cost(char1, char2, userCosts=False)                   :76-89
    min_cost(dp, i, j, str1, str2, userCosts=False)       :92-128
    wagnerFisher(str1, str2, userCosts=False) -> dp       :133-224
    create_paths(dp) -> paths                             :228-271
    generate_es(path, str1, str2) -> edit script          :274-334
    generate_rev_es(es), generate_sequence_from_es(es)    :338-377
    patching(es, str1) -> (error_code, str)               :380-457

What runs where.  wagnerFisher checks the cost table (raising the reference's
KeyError) and asks the GPU for dp[n][m]; the returned dp is a lazy matrix:
len(dp), len(dp[0]) and dp[n][m].value need nothing more, any other cell
materialises the whole matrix (values, int/float typing and the co-optimal
edges) with one fp64 kernel.  create_paths(dp)[0] — the path the GUI and
every edit-script consumer takes first — comes from the device traceback;
later paths are enumerated on the host in the reference's order (length, then
sink-lexicographic) over the materialised edges by copaths.iter_paths, and
count_paths(dp) gives their number without enumerating them.  Deliberate differences: no import-time demo print
(:463-471), and create_paths never blocks (the reference's bounded Queue
deadlocks once live paths exceed (n+1)(m+1), :237,265).

There is no CPU fallback for the DP: without libsed.so or a HIP device the
functions raise sedgpu.SedError.
"""
import json
import math
import sys
from collections import deque

import numpy as np

import _sedhost  # host C: edit-script dicts, reversal, patching, JSON (csrc/sedhost.c)
import copaths
import sedcost
import sedgpu

# Step 1 (reference :6-18): cost tables from the current working directory, at import.
with open('costs.json', 'r') as f:
    default_costs = json.load(f)

try:
    with open('user_costs.json', 'r') as f:
        user_costs = json.load(f)
except (OSError, IOError):
    user_costs = default_costs
    print('Could not find user costs file')


def reload_user_costs():
    """Re-read user_costs.json into the module global (reference :24-27)."""
    global user_costs
    with open('user_costs.json', 'r') as f:
        user_costs = json.load(f)


def _table(userCosts):
    return user_costs if userCosts else default_costs


class Edge:
    """source -> destination via operation ('insert' | 'delete' | 'update')."""

    def __init__(self, source, destination, operation):
        self.source = source
        self.destination = destination
        self.operation = operation


class Node:
    """A DP cell: i/j are string indices (row-1, col-1), value the cell cost."""

    def __init__(self, i, j, value=0):
        self.i = i
        self.j = j
        self.value = value
        self.edges = []
        self.incoming_edges = []
        self.visited = False

    def add_neighbor(self, dest, operation):
        e = Edge(self, dest, operation)
        self.edges.append(e)
        dest.incoming_edges.append(e)

    def __repr__(self):
        return str(self.value)


def cost(char1, char2, userCosts=False):
    """int 0 for a case-insensitive match, else the table's update cost (reference :76-89)."""
    if char1.lower() == char2.lower():
        return 0
    return _table(userCosts)['update'][char1][char2]


def min_cost(dp, i, j, str1, str2, userCosts=False):
    """(value, [insert, delete, update] op tuples or None) for cell (i, j) (reference :92-128)."""
    table = _table(userCosts)
    cands = [dp[i][j - 1].value + table['insert'],
             dp[i - 1][j].value + table['delete'],
             dp[i - 1][j - 1].value + cost(str1[i - 1], str2[j - 1], userCosts)]
    val = min(cands)
    ops = [None, None, None]
    if cands[0] == val:
        ops[0] = (i, j - 1, 'insert')
    if cands[1] == val:
        ops[1] = (i - 1, j, 'delete')
    if cands[2] == val:
        ops[2] = (i - 1, j - 1, 'update')
    return val, ops


# ---------------------------------------------------------------------------
# the lazy dp matrix
# ---------------------------------------------------------------------------
_OPNAME = ('insert', 'delete', 'update')
_MASKBIT = {'insert': 1, 'delete': 2, 'update': 4}


class Cell(Node):
    """Node view of cell (row, col) of a DPMatrix; identical surface to Node."""

    __slots__ = ('_dp', 'row', 'col', 'visited', '_in', '_out')

    def __init__(self, dp, row, col):  # noqa: D401 — Node.__init__ deliberately not called
        self._dp = dp
        self.row = row
        self.col = col
        self.visited = False
        self._in = None
        self._out = None

    @property
    def i(self):
        return self.row - 1

    @property
    def j(self):
        return self.col - 1

    @property
    def value(self):
        return self._dp._value(self.row, self.col)

    @property
    def incoming_edges(self):
        if self._in is None:
            self._in = self._dp._incoming(self.row, self.col)
        return self._in

    @property
    def edges(self):
        if self._out is None:
            self._out = self._dp._outgoing(self.row, self.col)
        return self._out

    def add_neighbor(self, dest, operation):
        e = Edge(self, dest, operation)
        self.edges.append(e)
        dest.incoming_edges.append(e)

    def __repr__(self):
        return str(self.value)


class _Row:
    __slots__ = ('_dp', '_r')

    def __init__(self, dp, r):
        self._dp = dp
        self._r = r

    def __len__(self):
        return self._dp.m + 1

    def __getitem__(self, j):
        w = self._dp.m + 1
        if isinstance(j, slice):
            return [self._dp.cell(self._r, k) for k in range(*j.indices(w))]
        if j < 0:
            j += w
        if not 0 <= j < w:
            raise IndexError('list index out of range')
        return self._dp.cell(self._r, j)

    def __iter__(self):
        for j in range(self._dp.m + 1):
            yield self._dp.cell(self._r, j)

    def __repr__(self):
        return '[' + ', '.join(repr(c) for c in self) + ']'


class DPMatrix:
    """(n+1) x (m+1) matrix of Cell views; what wagnerFisher returns."""

    def __init__(self, str1, str2, plan):
        self.str1, self.str2 = str1, str2
        self.n, self.m = len(str1), len(str2)
        self._plan = plan
        self._bcodes = (plan.encode_bytes(str1), plan.encode_bytes(str2))
        self._ncodes = None
        self._final = None
        self._full = None
        self._script = None
        self._skel = None  # generate_es records built during the script run, for its canonical path (_run)
        self._cells = {}
        self._edges = {}
        self._rows = {}

    @property
    def _codes(self):
        if self._ncodes is None:
            self._ncodes = tuple(np.frombuffer(b, np.uint8) for b in self._bcodes)
        return self._ncodes

    # -- engine calls --
    def _run(self, want_script):
        ctx = sedgpu.context()
        ctx.set_costs(self._plan)
        a, b = self._bcodes
        if want_script and self.n + self.m >= _SKEL_MIN and hasattr(ctx, "submit_pair"):
            # the GUI's call (wagnerFisher -> create_paths -> generate_es, gui.py:360,385-391): the edit script's
            # records (at least max(n, m) of them) are built while the device computes the script, and generate_es
            # of this matrix's canonical path only fills in their values (tools/es_build_bench.py: ~1/4 of the build)
            ctx.submit_pair(a, b, True)
            try:
                self._skel = _skeleton(max(self.n, self.m), self.n + self.m)
            finally:
                d, is_int, ln, ops = ctx.wait_pair()
        else:
            d, is_int, ln, ops = ctx.run_pair(a, b, want_script, no_len=not want_script)
        self._final = int(d) if is_int else d
        if want_script:
            self._script = sedgpu.unpack_ops(ops, (0,), 0, int(ln))

    def _materialise(self):
        if self._full is None:
            ctx = sedgpu.context()
            ctx.set_costs(self._plan)
            D, M = ctx.full_matrix(self._codes[0], self._codes[1])
            self._full = (D, M)
        return self._full

    def script(self):
        """Canonical op codes (0 insert, 1 delete, 2 update), origin -> sink."""
        global _script_hint
        _script_hint = True
        if self._script is None:
            self._run(True)
        return self._script

    # -- cell access --
    def _value(self, r, c):
        if r == self.n and c == self.m and self._final is not None:
            return self._final
        D, M = self._materialise()
        v = float(D[r, c])
        return int(v) if M[r, c] & 8 else v

    def _edge(self, r, c, op):
        key = (r, c, op)
        e = self._edges.get(key)
        if e is None:
            pr, pc = (r, c - 1) if op == 'insert' else ((r - 1, c) if op == 'delete' else (r - 1, c - 1))
            e = Edge(self.cell(pr, pc), self.cell(r, c), op)
            self._edges[key] = e
        return e

    def _incoming(self, r, c):
        M = self._materialise()[1]
        mask = int(M[r, c]) & 7
        return [self._edge(r, c, op) for op in _OPNAME if mask & _MASKBIT[op]]

    def _outgoing(self, r, c):
        M = self._materialise()[1]
        out = []
        # reference creation order: row 0 first, then column 0, then the interior row-major
        cand = [('insert', r, c + 1), ('delete', r + 1, c), ('update', r + 1, c + 1)]
        if c == 0 and r > 0:
            cand = [cand[1], cand[0], cand[2]]
        for op, rr, cc in cand:
            if rr <= self.n and cc <= self.m and int(M[rr, cc]) & _MASKBIT[op]:
                out.append(self._edge(rr, cc, op))
        return out

    def cell(self, r, c):
        k = (r, c)
        x = self._cells.get(k)
        if x is None:
            x = Cell(self, r, c)
            self._cells[k] = x
        return x

    # -- list protocol --
    def __len__(self):
        return self.n + 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(self.n + 1))]
        if i < 0:
            i += self.n + 1
        if not 0 <= i <= self.n:
            raise IndexError('list index out of range')
        row = self._rows.get(i)
        if row is None:
            row = self._rows[i] = _Row(self, i)
        return row

    def __iter__(self):
        for i in range(self.n + 1):
            yield self[i]

    def __repr__(self):
        return '[' + ', '.join(repr(r) for r in self) + ']'


# script calls of at least this many symbols (n + m) build their generate_es records during the device run (_run)
_SKEL_MIN = 512

# generate_es lists of those calls, kept (a reference each) until no one else holds them: the next script call's
# device window then reuses one as its records (es_recycle: its values are overwritten) or releases it, instead of
# the caller paying for ~13 000 dict deallocations when it drops a 4096^2 script (gui.py:386-388 clears the previous
# call's scripts; a loop rebinds its variable).  A list the caller still holds is kept and looked at again.
_retired = deque()
_RETIRE_MAX = 3
_RETIRE_RECORDS = 1 << 16  # (longer scripts are not kept: at most ~3 x 20 MB of dicts held past their use)


def _skeleton(count, most):
    """Records for the next script's generate_es (at least `count`): a retired list no one else holds and with at most
    `most` records (no surplus to drop after the run), reused, else new ones (es_skeleton).  The other retired lists
    no one holds any more are released here, while the device computes."""
    skel = None
    for _ in range(len(_retired)):
        lst = _retired.popleft()
        if sys.getrefcount(lst) > 2:  # (this name and getrefcount's argument: anything more is the caller's)
            _retired.append(lst)
        elif skel is None and len(lst) <= most:
            skel = _sedhost.es_recycle(lst, count)
        del lst
    return skel if skel is not None else _sedhost.es_skeleton(count)

# One-deep predictor of the caller's pattern: True when the matrix of the previous wagnerFisher call
# was asked for its script (the GUI: wagnerFisher -> create_paths -> generate_es).  The next call then
# runs DP + traceback in one engine call instead of a distance run followed by a script run; callers
# that only read distances (IRMethods.wf_score) keep the cheaper distance-only run.  Either way the
# matrix is computed eagerly, as in the reference, and the results are the same.
_script_hint = False


def wagnerFisher(str1, str2, userCosts=False):
    """Weighted Wagner–Fischer matrix of str1 (rows) -> str2 (columns) (reference :133-224)."""
    global _script_hint
    table = _table(userCosts)
    if type(str1) is str and type(str2) is str and str1 and str2:
        plan = sedcost.pair_plan(table, str1, str2)  # check_pair + build_plan, cached by the resolved costs
    else:
        sedcost.check_pair(table, str1, str2)
        plan = sedcost.build_plan(table, [str1], [str2])
    dp = DPMatrix(str1, str2, plan)
    want, _script_hint = _script_hint, False
    dp._run(want)
    return dp


# ---------------------------------------------------------------------------
# paths
# ---------------------------------------------------------------------------
class Path(list):
    """A co-optimal path (list of Cell, origin -> sink) with its op codes.

    The cells are built on first use: generate_es and the batch helpers only need
    the op codes, and building 8k cell views of a 4096 x 4096 path costs ~4 ms."""

    def __init__(self, dp, ops):
        super().__init__()
        self.ops = ops
        self._dp = dp
        self._filled = False

    def _fill(self):
        if not self._filled:
            self._filled = True
            r = c = 0
            cells = [self._dp.cell(0, 0)]
            for op in self.ops:
                if op != 1:
                    c += 1
                if op != 0:
                    r += 1
                cells.append(self._dp.cell(r, c))
            list.extend(self, cells)
        return self

    def __len__(self):
        return len(self.ops) + 1

    def __bool__(self):
        return True

    def __getitem__(self, k):
        return list.__getitem__(self._fill(), k)

    def __iter__(self):
        return list.__iter__(self._fill())

    def __reversed__(self):
        return list.__reversed__(self._fill())

    def __contains__(self, x):
        return list.__contains__(self._fill(), x)

    def __eq__(self, other):
        return list.__eq__(self._fill(), other)

    __hash__ = None

    def __repr__(self):
        return list.__repr__(self._fill())

    def index(self, *a):
        return list.index(self._fill(), *a)

    def count(self, x):
        return list.count(self._fill(), x)

    def copy(self):
        return list(self._fill())

    def __add__(self, other):
        return list(self._fill()) + list(other)

    def __reduce__(self):
        return (list, (list(self._fill()),))


def _cells_of_script(dp, ops):
    return Path(dp, ops)


class PathList:
    """Lazy result of create_paths(dp): element 0 is the device's canonical
    path; the rest are enumerated on demand, in the reference's order, by
    copaths.iter_paths over the materialised edge mask (no BFS frontier)."""

    def __init__(self, dp):
        self._dp = dp
        self._done = []
        self._gen = None
        self._exhausted = False

    def _next(self):
        if not self._done:
            self._done.append(_cells_of_script(self._dp, self._dp.script()))
            return True
        if self._exhausted:
            return False
        if self._gen is None:
            self._gen = copaths.iter_paths(self._dp._materialise()[1])
            next(self._gen)  # the first path in reference order is the canonical one already returned
        try:
            ops = next(self._gen)
        except StopIteration:
            self._exhausted = True
            return False
        self._done.append(_cells_of_script(self._dp, ops))
        return True

    def __getitem__(self, k):
        if isinstance(k, slice):
            return list(self)[k]
        if k < 0:
            return list(self)[k]
        while len(self._done) <= k:
            if not self._next():
                raise IndexError('list index out of range')
        return self._done[k]

    def __iter__(self):
        k = 0
        while True:
            if k >= len(self._done) and not self._next():
                return
            yield self._done[k]
            k += 1

    def __len__(self):
        while self._next():
            pass
        return len(self._done)

    def __bool__(self):
        return True  # a dp always has at least one co-optimal path


def create_paths(dp):
    """All co-optimal paths, shortest first (reference :228-271)."""
    if isinstance(dp, DPMatrix):
        dp[dp.n][dp.m].visited = True
        return PathList(dp)
    return _create_paths_graph(dp)


def count_paths(dp):
    """Number of co-optimal paths, i.e. len(create_paths(dp)), as an exact int without
    enumerating them (extension)."""
    if isinstance(dp, DPMatrix):
        return copaths.count_paths(dp._materialise()[1])
    n, m = len(dp) - 1, len(dp[0]) - 1
    M = np.zeros((n + 1, m + 1), np.uint8)
    bit = {"insert": 1, "delete": 2, "update": 4}
    for r in range(n + 1):
        for c in range(m + 1):
            for e in dp[r][c].incoming_edges:
                M[r, c] |= bit[e.operation]
    return copaths.count_paths(M)


def _create_paths_graph(dp):
    """The same enumeration over a caller-built Node graph (list of lists)."""
    goal = dp[0][0]
    src = dp[len(dp) - 1][len(dp[0]) - 1]
    src.visited = True
    q = deque([[src]])
    out = []
    while q:
        p = q.popleft()
        if p[-1] is goal:
            out.append(p)
        for e in p[-1].incoming_edges:
            if not any(x is e.source for x in p):
                q.append(p + [e.source])
    return [p[::-1] for p in out]


# ---------------------------------------------------------------------------
# edit scripts
# ---------------------------------------------------------------------------
def _op_record(op, str1, str2, ni, nj):
    return {"operation": op,
            "source": {"character": str1[ni], "index": ni},
            "destination": {"character": str2[nj], "index": nj}}


def generate_es(path, str1, str2):
    """One dict per edge of the path, origin -> sink (reference :274-334).
    source/destination describe the edge's destination cell (i, j); index -1
    (row 0 / column 0) reads str[-1], the last character, as the reference does."""
    if len(path) < 2:
        path[1]  # IndexError, as the reference's `next = path[1]`
    ops = getattr(path, 'ops', None)
    es = []
    if ops is not None and len(ops) == len(path) - 1:
        if type(str1) is str and type(str2) is str:
            codes = np.asarray(ops, np.uint8).tobytes()
            dp = getattr(path, '_dp', None)
            skel = dp._skel if isinstance(dp, DPMatrix) else None
            if skel is not None and ops is dp._script and str1 == dp.str1 and str2 == dp.str2:
                dp._skel = None  # (each call returns new records: the next one builds its own)
                es = _sedhost.es_fill(skel[0], skel[1], codes, str1, str2)
                if len(es) <= _RETIRE_RECORDS:
                    _retired.append(es)
                    while len(_retired) > _RETIRE_MAX:
                        _retired.popleft()
                return es
            return _sedhost.es_from_ops(codes, str1, str2)
        for op, nxt in zip(ops, path[1:]):
            es.append(_op_record(_OPNAME[op], str1, str2, nxt.i, nxt.j))
        return es
    for cur, nxt in zip(path, path[1:]):
        edge = [e for e in cur.edges if e.source is cur and e.destination is nxt]
        if not edge:
            edge = [e for e in cur.edges if e.source == cur and e.destination == nxt]
        es.append(_op_record(edge[0].operation, str1, str2, nxt.i, nxt.j))  # IndexError if not an edge
    return es


def generate_rev_es(es):
    """The script that turns str2 back into str1 (reference :338-369)."""
    fast = _sedhost.rev_es(es)
    if fast is not NotImplemented:
        return fast
    out = []
    for e in es:
        op = e['operation']
        if op == 'insert':
            new = {'operation': 'delete', 'source': e['destination'], 'destination': e['source']}
        elif op == 'delete':
            new = {'operation': 'insert',
                   'source': {'index': e['destination']['index'] - 1, 'character': e['destination']['character']},
                   'destination': e['source']}
        elif op == 'update':
            new = {'operation': 'update', 'source': e['destination'], 'destination': e['source']}
        else:  # the reference reuses the previous iteration's bindings (or raises NameError on the first)
            new = {'operation': out[-1]['operation'], 'source': out[-1]['source'],
                   'destination': out[-1]['destination']} if out else None
            if new is None:
                raise UnboundLocalError("local variable 'new_operation' referenced before assignment")
        out.append(new)
    return out


def generate_sequence_from_es(es):
    """The source string a script was generated from (reference :371-377)."""
    fast = _sedhost.seq_from_es(es)
    if fast is not NotImplemented:
        return fast
    return ''.join(op['source']['character'] for op in es if op['operation'] != 'insert')


def patching(es, str1):
    """Apply an edit script to str1 -> (error_code, patched) (reference :380-457).
    error_code: 0 str1 is the script's source, 1 str1 is at least as long (warn),
    -1 str1 is shorter (returns (-1, ''))."""
    fast = _sedhost.patching(es, str1)
    if fast is not NotImplemented:
        return fast
    original = generate_sequence_from_es(es)
    if str1 == original:
        error_code = 0
    elif len(str1) >= len(original):
        error_code = 1
    else:
        return (-1, '')
    out = str1
    removed = inserted = 0
    for rec in es:
        op = rec['operation']
        at, dst_at = rec['source']['index'], rec['destination']['index']  # both read, as the reference does
        if op != 'insert':
            at = at + removed + inserted
        else:
            at = dst_at
        if op == 'update':
            out = out[:at] + rec['destination']['character'] + out[at + 1:]
        elif op == 'delete':
            out = out[:at] + out[at + 1:]
            removed -= 1
        elif op == 'insert':
            out = out[:at] + rec['destination']['character'] + out[at:]
            inserted += 1
    return (error_code, out)


def es_to_json(es, indent=4):
    """json.dumps({'edit_script': es}, indent=indent) — the GUI's export format (gui.py:629-638)."""
    fast = _sedhost.es_json(es, indent)
    if fast is not NotImplemented:
        return fast
    return json.dumps({'edit_script': es}, indent=indent)


def save_es(path, es, indent=4):
    """Write an edit script the way the GUI's export does (gui.py:629-638)."""
    with open(path, 'w') as f:
        f.write(es_to_json(es, indent))


def load_es(path):
    """Read an edit script the way the GUI's patch-tab import does (gui.py:650-657)."""
    with open(path, 'r') as f:
        return json.load(f)['edit_script']


# ---------------------------------------------------------------------------
# batch extensions (not in the reference): one launch for many pairs
# ---------------------------------------------------------------------------
def batch_plan(strs1, strs2, userCosts=False):
    """The reference's KeyError for the first offending pair, if any (sedcost.check_batch), then the batch's plan."""
    table = _table(userCosts)
    u = None  # the batch's symbols, once for both steps
    if sedcost._all_str(strs1) and sedcost._all_str(strs2):
        u = (sedcost.distinct_many(strs1), sedcost.distinct_many(strs2))
    sedcost.check_batch(table, strs1, strs2, u)
    return sedcost.build_plan(table, strs1, strs2, u)


def _packed(plan, strs1, strs2):
    ca, la = plan.encode_many(strs1)
    cb, lb = plan.encode_many(strs2)
    return sedgpu.PackedPairs.from_concat(ca, la, cb, lb)


def distance_batch(strs1, strs2, userCosts=False, plan=None, max_dist=None):
    """[dp[n][m].value for each (str1, str2)] — one GPU launch; same typing and KeyErrors.  plan: batch_plan()'s
    result for the same arguments (wfsearch builds it once for its cache key).  max_dist (a batch extension, not in
    the reference): pairs whose value exceeds it come back as math.inf, and the integer kernels skip the cells no
    path within it can reach."""
    strs1, strs2 = list(strs1), list(strs2)
    if plan is None:
        plan = batch_plan(strs1, strs2, userCosts)
    if not strs1:
        return []
    ctx = sedgpu.context()
    ctx.set_costs(plan)
    if max_dist is None:
        dist, is_int, _, _ = ctx.run(_packed(plan, strs1, strs2), False, no_len=True)
    else:
        dist, is_int, _, _ = ctx.run_cutoff(_packed(plan, strs1, strs2), max_dist, True)
    return [int(d) if t else float(d) for d, t in zip(dist.tolist(), is_int.tolist())]


def distance_deepen(strs1, strs2, k, first, last, userCosts=False, plan=None):
    """distance_batch under the smallest cutoff of first, 2 first, 4 first, ... (at most last) that at least k pairs
    are within, on one resident batch: (values, cutoffs tried).  wfsearch.nearest's engine call."""
    strs1, strs2 = list(strs1), list(strs2)
    if plan is None:
        plan = batch_plan(strs1, strs2, userCosts)
    if not strs1:
        return [], []
    ctx = sedgpu.context()
    ctx.set_costs(plan)
    dist, is_int, _, _, cuts = ctx.deepen(_packed(plan, strs1, strs2), k, first, last, True)
    return [int(d) if t else float(d) for d, t in zip(dist.tolist(), is_int.tolist())], cuts


FIT_F64_SYMBOLS = 16  # the fp64 route's table bound (include/sed.h: sed_fit_search_f64)


def fit_batch(patterns, texts, userCosts=False, f64=False):
    """[(dist, start, end)] for each (pattern, text): the smallest wagnerFisher(pattern, text[start:end]) value over
    all substrings of the text (the empty one included), for the occurrence that ends earliest and, among those, starts
    latest — one GPU launch (sedgpu.Context.fit).  Patterns have 1..32 symbols; the integer kernels serve dyadic cost
    tables over at most 8 symbols and raise SedError otherwise (include/sed.h: sed_fit_search).  f64=True runs the fp64
    kernels instead (sedgpu.Context.fit_f64): any table of costs >= 0 over at most 16 symbols, the full IUPAC alphabet
    of costs.json among them; sedgpu.fit_route says which a batch needs.  dist is a float (no int
    typing: run the window through wagnerFisher for the reference's typed value).  Same KeyErrors as the reference
    would raise for (pattern, text)."""
    patterns, texts = list(patterns), list(texts)
    plan = batch_plan(patterns, texts, userCosts)
    if not patterns:
        return []
    ctx = sedgpu.context()
    ctx.set_costs(plan)
    dist, start, end = (ctx.fit_f64 if f64 else ctx.fit)(_packed(plan, patterns, texts))
    return list(zip(dist.tolist(), start.tolist(), end.tolist()))


class _EngineIndex:
    """The device half of a FitIndex: the texts' codes resident on the process's engine (sedgpu.FitIndex)."""

    def __init__(self, codes, off, lens):
        self.ctx = sedgpu.context()
        self.ix = self.ctx.fit_index(codes, off, lens)

    def search(self, plan, packed):
        self.ctx.set_costs(plan)
        return self.ix.search(packed)

    def hits(self, plan, packed, max_dist):
        self.ctx.set_costs(plan)
        return self.ix.hits(packed, max_dist)

    def search_long(self, plan, packed):
        self.ctx.set_costs(plan)
        return self.ix.search_long(packed)

    def hits_long(self, plan, packed, max_dist):
        self.ctx.set_costs(plan)
        return self.ix.hits_long(packed, max_dist)

    def search_f64(self, plan, packed):
        self.ctx.set_costs(plan)
        return self.ix.search_f64(packed)

    def hits_f64(self, plan, packed, max_dist):
        self.ctx.set_costs(plan)
        return self.ix.hits_f64(packed, max_dist)

    def search_long_f64(self, plan, packed):
        self.ctx.set_costs(plan)
        return self.ix.search_long_f64(packed)

    def hits_long_f64(self, plan, packed, max_dist):
        self.ctx.set_costs(plan)
        return self.ix.hits_long_f64(packed, max_dist)

    def close(self):
        self.ix.close()


class FitIndex:
    """fit_batch over texts that stay on the device: fit_index(texts) encodes and uploads them once, and
    search(patterns) sends only the patterns and runs all of them against every text in one launch.

    The texts' symbols get their codes when the index is built (first-occurrence order over the texts, as batch_plan
    resolves them; or `alphabet` first, for a collection that may grow into symbols it does not hold yet).  A search
    whose patterns bring symbols the texts do not have appends them for that search only; more than 8 symbols in all
    raise SedError (the integer kernels serve at most 8).  f64=True builds the index for the fp64 route instead: the
    bound is 16 symbols, and search_f64 / hits_f64 (and search_long_f64 / hits_long_f64 for patterns of up to 2048
    symbols) serve any table of costs >= 0 (search / hits still run the integer
    kernels and refuse what those refuse).  The cost table is read at every search, so edits to it take effect,
    and the KeyErrors are the reference's for the first offending (pattern, text) in pattern-major order."""

    def __init__(self, texts, userCosts=False, alphabet=None, engine=None, f64=False):
        self.texts = list(texts)
        self.userCosts = userCosts
        self.f64 = bool(f64)
        self.max_symbols = FIT_F64_SYMBOLS if self.f64 else 8
        used = sedcost.distinct_many(self.texts) if sedcost._all_str(self.texts) else \
            list(dict.fromkeys(c for t in self.texts for c in t))
        self._used = used  # the symbols the texts hold: the str2 side of every cost lookup
        self.symbols = list(dict.fromkeys(list(alphabet or ()) + used))
        if len(self.symbols) > self.max_symbols:
            raise sedgpu.SedError("fit index: the texts have %d symbols (fit search serves at most %d%s)"
                                  % (len(self.symbols), self.max_symbols, "" if self.f64 else "; f64=True serves 16"))
        code = {c: k for k, c in enumerate(self.symbols)}
        lens = np.fromiter(map(len, self.texts), dtype=np.int32, count=len(self.texts))
        codes = np.fromiter((code[c] for t in self.texts for c in t), dtype=np.uint8, count=int(lens.sum()))
        off = np.zeros(len(lens), np.int64)
        if len(lens):
            off[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        self._dev = (engine or _EngineIndex)(codes, off, lens)

    def plan(self, patterns):
        """The reference's KeyError for the first offending (pattern, text), if any, then the search's CostPlan: the
        index's symbols in their order, then the patterns' new ones."""
        table = _table(self.userCosts)
        rep = "".join(self._used) if sedcost._all_str(self.texts) and all(len(c) == 1 for c in self._used) else None
        u1 = sedcost.distinct_many(patterns) if sedcost._all_str(patterns) else \
            list(dict.fromkeys(c for p in patterns for c in p))
        # one pair per pattern against a text of every symbol the index holds resolves exactly when every pair does
        if rep is None or not sedcost._batch_resolves(table, patterns, [rep] * len(patterns), (u1, self._used)):
            for p in patterns:
                for t in self.texts:
                    sedcost.check_pair(table, p, t)
        alphabet = self.symbols + [c for c in u1 if c not in self.symbols]
        if len(alphabet) > self.max_symbols:
            raise sedgpu.SedError("fit index: the texts and these patterns have %d symbols (fit search serves at most %d%s)"
                                  % (len(alphabet), self.max_symbols, "" if self.f64 else "; f64=True serves 16"))
        return sedcost.plan_over(table, alphabet, set(u1), set(self._used))

    def search(self, patterns, _dev="search"):
        """[[(dist, start, end) for each text] for each pattern], every hit as fit_batch defines it."""
        patterns = list(patterns)
        plan = self.plan(patterns)
        if not patterns:
            return []
        ca, la = plan.encode_many(patterns)
        packed = sedgpu.PackedPairs.from_concat(ca, la, np.zeros(0, np.uint8), np.zeros(len(la), np.int32))
        dist, start, end = getattr(self._dev, _dev)(plan, packed)
        return [list(zip(d, s, e)) for d, s, e in zip(dist.tolist(), start.tolist(), end.tolist())]

    def search_long(self, patterns):
        """search() for patterns of 1..2048 symbols (include/sed.h: sed_fit_index_search_long); the same alphabet growth
        and errors."""
        return self.search(patterns, "search_long")

    def hits_long(self, patterns, max_dist):
        """hits() for patterns of 1..2048 symbols (include/sed.h: sed_fit_index_hits_long)."""
        return self.hits(patterns, max_dist, "hits_long")

    def search_f64(self, patterns):
        """search() through the fp64 kernels (include/sed.h: sed_fit_index_search_f64): any table of costs >= 0; with
        an index built f64=True, up to 16 symbols."""
        return self.search(patterns, "search_f64")

    def hits_f64(self, patterns, max_dist):
        """hits() through the fp64 kernels (include/sed.h: sed_fit_index_hits_f64)."""
        return self.hits(patterns, max_dist, "hits_f64")

    def search_long_f64(self, patterns):
        """search_f64() for patterns of 1..2048 symbols (include/sed.h: sed_fit_index_search_long_f64): what search_long
        refuses, e.g. a 76-nt query over IUPAC documents under costs.json, on an index built f64=True."""
        return self.search(patterns, "search_long_f64")

    def hits_long_f64(self, patterns, max_dist):
        """hits_f64() for patterns of 1..2048 symbols (include/sed.h: sed_fit_index_hits_long_f64)."""
        return self.hits(patterns, max_dist, "hits_long_f64")

    def hits(self, patterns, max_dist, _dev="hits"):
        """[(pattern index, text index, start, end, dist)] sorted by (pattern, text, end): for every end column e of a
        text (0 <= e <= its length) the smallest wagnerFisher(pattern, text[s:e]) value over s, with the largest such s
        as start, kept when that value is <= max_dist (include/sed.h: sed_fit_index_hits; math.inf keeps every
        column).  The same alphabet growth, KeyErrors and SedErrors as search()."""
        patterns = list(patterns)
        plan = self.plan(patterns)
        if not patterns:
            return []
        ca, la = plan.encode_many(patterns)
        packed = sedgpu.PackedPairs.from_concat(ca, la, np.zeros(0, np.uint8), np.zeros(len(la), np.int32))
        h = getattr(self._dev, _dev)(plan, packed, max_dist)
        return list(zip(h["query"].tolist(), h["text"].tolist(), h["start"].tolist(), h["end"].tolist(), h["dist"].tolist()))

    def close(self):
        self._dev.close()


def fit_index(texts, userCosts=False, alphabet=None, engine=None, f64=False):
    """A FitIndex over texts: fit_batch for callers who search one collection query after query.  engine(codes, off,
    lens) -> an object with search(plan, packed), hits(plan, packed, max_dist), their search_long / hits_long,
    search_f64 / hits_f64, search_long_f64 / hits_long_f64 and close() replaces the device (CPU tests)."""
    return FitIndex(texts, userCosts, alphabet, engine, f64)


JOIN_MAX_LEN = 32  # the join's longest sequence (include/sed.h: sed_join_index_create)
JOIN_LONG_MAX_LEN = 128  # the long join's (include/sed.h: sed_join_long_index_create)
JOIN_F64_SYMBOLS = 16  # the fp64 route's table bound (include/sed.h: sed_join_self_f64)
JOIN_KNN_MAX_K = 64  # the k-nearest calls' largest k (include/sed.h: sed_join_knn_self)


class _EngineJoin:
    """The device half of a JoinIndex: the sequences' codes resident on the process's engine (sedgpu.JoinIndex)."""

    def __init__(self, codes, off, lens, long_seqs=False):
        self.ctx = sedgpu.context()
        self.ix = (self.ctx.join_long_index if long_seqs else self.ctx.join_index)(codes, off, lens)

    def self_join(self, plan, max_dist, rows):
        self.ctx.set_costs(plan)
        return self.ix.self_join(max_dist, rows)

    def search(self, plan, packed, max_dist):
        self.ctx.set_costs(plan)
        return self.ix.search(packed, max_dist)

    def self_join_f64(self, plan, max_dist, rows):
        self.ctx.set_costs(plan)
        return self.ix.self_join_f64(max_dist, rows)

    def self_knn(self, plan, k, max_dist, rows):
        self.ctx.set_costs(plan)
        return self.ix.self_knn(k, max_dist, rows)

    def search_knn(self, plan, packed, k, max_dist):
        self.ctx.set_costs(plan)
        return self.ix.search_knn(packed, k, max_dist)

    def search_f64(self, plan, packed, max_dist):
        self.ctx.set_costs(plan)
        return self.ix.search_f64(packed, max_dist)

    def self_knn_f64(self, plan, k, max_dist, rows):
        self.ctx.set_costs(plan)
        return self.ix.self_knn_f64(k, max_dist, rows)

    def search_knn_f64(self, plan, packed, k, max_dist):
        self.ctx.set_costs(plan)
        return self.ix.search_knn_f64(packed, k, max_dist)

    def close(self):
        self.ix.close()


class JoinIndex:
    """Every pair of short sequences within a distance, over sequences that stay on the device: join_index(seqs) encodes
    and uploads them once (0..32 symbols each); self_join(max_dist) returns [(i, j, dist)] for every i != j with
    wagnerFisher(seqs[i], seqs[j]).value <= max_dist, search(queries, max_dist) returns [(q, j, dist)] for every query
    against every sequence, both sorted by (row, column); rows are str1, columns str2 (include/sed.h: sed_join_self,
    sed_join_search).  dist is a float (no int typing).  Symbols get their codes as in FitIndex; the engine serves dyadic
    cost tables over at most 8 symbols and raises SedError otherwise.  f64=True builds the index for the fp64 route
    instead: the bound is 16 symbols (the refusal names the bound in force; the default's text is unchanged), and
    self_join_f64 / search_f64 serve any table of costs >= 0 (self_join / search still run the integer kernels and
    refuse what those refuse).  long_seqs=True builds the index for sequences and queries of 0..128 symbols
    (include/sed.h: sed_join_long_self, sed_join_long_search): the integer route only, so with f64=True it is a
    ValueError; the engine is then called with long_seqs=True as a further, keyword argument.  The cost table is read at
    every call, and the KeyErrors are the reference's for the first offending (row, column) in row-major order.
    self_nearest(k) and search_nearest(queries, k) return, for every row, its k nearest sequences instead (include/sed.h:
    sed_join_knn_self, sed_join_knn_search): [(row, j, dist)] sorted by (row, dist, j), nearest first, ties going to the
    lower j, at most k a row, k = 1..64; max_dist (None: no cap) leaves out what lies farther.  They run the integer
    kernels, with long_seqs=True too, and on an index built f64=True refuse what those refuse; self_nearest_f64 and
    search_nearest_f64 are the same calls through the fp64 kernel (include/sed.h: sed_join_knn_self_f64,
    sed_join_knn_search_f64), as self_join_f64 / search_f64 are to self_join / search."""

    def __init__(self, seqs, userCosts=False, alphabet=None, engine=None, f64=False, long_seqs=False):
        self.seqs = list(seqs)
        self.userCosts = userCosts
        self.f64 = bool(f64)
        self.long_seqs = bool(long_seqs)
        if self.f64 and self.long_seqs:
            raise ValueError("the long join has no fp64 route yet: long_seqs=True takes f64=False")
        self.max_len = JOIN_LONG_MAX_LEN if self.long_seqs else JOIN_MAX_LEN
        self.max_symbols = JOIN_F64_SYMBOLS if self.f64 else 8
        for i, s in enumerate(self.seqs):
            if len(s) > self.max_len:
                raise sedgpu.SedError("join index: sequence %d has %d symbols (the join serves at most %d)"
                                      % (i, len(s), self.max_len))
        used = sedcost.distinct_many(self.seqs) if sedcost._all_str(self.seqs) else \
            list(dict.fromkeys(c for t in self.seqs for c in t))
        self._used = used
        self.symbols = list(dict.fromkeys(list(alphabet or ()) + used))
        if len(self.symbols) > self.max_symbols:
            raise sedgpu.SedError("join index: the sequences have %d symbols (the join serves at most %d)"
                                  % (len(self.symbols), self.max_symbols))
        code = {c: k for k, c in enumerate(self.symbols)}
        lens = np.fromiter(map(len, self.seqs), dtype=np.int32, count=len(self.seqs))
        codes = np.fromiter((code[c] for t in self.seqs for c in t), dtype=np.uint8, count=int(lens.sum()))
        off = np.zeros(len(lens), np.int64)
        if len(lens):
            off[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        self._dev = (engine or _EngineJoin)(codes, off, lens, long_seqs=True) if self.long_seqs else \
            (engine or _EngineJoin)(codes, off, lens)

    def plan(self, rows):
        """The reference's KeyError for the first offending (row, sequence), if any, then the call's CostPlan: the
        index's symbols in their order, then the rows' new ones."""
        table = _table(self.userCosts)
        rep = "".join(self._used) if sedcost._all_str(self.seqs) and all(len(c) == 1 for c in self._used) else None
        u1 = sedcost.distinct_many(rows) if sedcost._all_str(rows) else list(dict.fromkeys(c for p in rows for c in p))
        # one pair per row against a sequence of every symbol the index holds resolves exactly when every pair does
        if rep is None or not sedcost._batch_resolves(table, rows, [rep] * len(rows), (u1, self._used)):
            for p in rows:
                for t in self.seqs:
                    sedcost.check_pair(table, p, t)
        alphabet = self.symbols + [c for c in u1 if c not in self.symbols]
        if len(alphabet) > self.max_symbols:
            raise sedgpu.SedError("join index: the sequences and these rows have %d symbols (the join serves at most %d)"
                                  % (len(alphabet), self.max_symbols))
        return sedcost.plan_over(table, alphabet, set(u1), set(self._used))

    def self_join(self, max_dist, rows=None, _dev="self_join"):
        lo, hi = (0, len(self.seqs)) if rows is None else rows
        if not 0 <= lo <= hi <= len(self.seqs):
            raise ValueError("rows=(%r, %r) is no range of the index's %d sequences" % (lo, hi, len(self.seqs)))
        plan = self.plan(self.seqs[lo:hi])
        if lo == hi:
            return []
        h = getattr(self._dev, _dev)(plan, max_dist, (lo, hi))
        return list(zip(h["row"].tolist(), h["col"].tolist(), h["dist"].tolist()))

    @staticmethod
    def check_k(k):
        """k of the k-nearest calls, refused here as the engine refuses it, so that a call the engine is not reached for
        (no rows, no queries, no sequences) refuses it too."""
        if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= JOIN_KNN_MAX_K:
            raise sedgpu.SedError("join: k = %r neighbours a row (1..%d)" % (k, JOIN_KNN_MAX_K))

    def self_nearest(self, k, max_dist=None, rows=None, _dev="self_knn"):
        self.check_k(k)
        lo, hi = (0, len(self.seqs)) if rows is None else rows
        if not 0 <= lo <= hi <= len(self.seqs):
            raise ValueError("rows=(%r, %r) is no range of the index's %d sequences" % (lo, hi, len(self.seqs)))
        plan = self.plan(self.seqs[lo:hi])
        if lo == hi:
            return []
        h = getattr(self._dev, _dev)(plan, k, math.inf if max_dist is None else max_dist, (lo, hi))
        return list(zip(h["row"].tolist(), h["col"].tolist(), h["dist"].tolist()))

    def search_nearest(self, queries, k, max_dist=None, _dev="search_knn"):
        self.check_k(k)
        queries = list(queries)
        for q, s in enumerate(queries):
            if len(s) > self.max_len:
                raise sedgpu.SedError("join: query %d has %d symbols (the join serves at most %d)" % (q, len(s), self.max_len))
        plan = self.plan(queries)
        if not queries or not self.seqs:
            return []
        ca, la = plan.encode_many(queries)
        packed = sedgpu.PackedPairs.from_concat(ca, la, np.zeros(0, np.uint8), np.zeros(len(la), np.int32))
        h = getattr(self._dev, _dev)(plan, packed, k, math.inf if max_dist is None else max_dist)
        return list(zip(h["row"].tolist(), h["col"].tolist(), h["dist"].tolist()))

    def self_nearest_f64(self, k, max_dist=None, rows=None):
        """self_nearest() through the fp64 kernel (include/sed.h: sed_join_knn_self_f64): any table of costs >= 0; with
        an index built f64=True, up to 16 symbols."""
        return self.self_nearest(k, max_dist, rows, "self_knn_f64")

    def search_nearest_f64(self, queries, k, max_dist=None):
        """search_nearest() through the fp64 kernel (include/sed.h: sed_join_knn_search_f64)."""
        return self.search_nearest(queries, k, max_dist, "search_knn_f64")

    def self_join_f64(self, max_dist, rows=None):
        """self_join() through the fp64 kernel (include/sed.h: sed_join_self_f64): any table of costs >= 0; with an
        index built f64=True, up to 16 symbols."""
        return self.self_join(max_dist, rows, "self_join_f64")

    def search_f64(self, queries, max_dist):
        """search() through the fp64 kernel (include/sed.h: sed_join_search_f64)."""
        return self.search(queries, max_dist, "search_f64")

    def search(self, queries, max_dist, _dev="search"):
        queries = list(queries)
        for q, s in enumerate(queries):
            if len(s) > self.max_len:
                raise sedgpu.SedError("join: query %d has %d symbols (the join serves at most %d)" % (q, len(s), self.max_len))
        plan = self.plan(queries)
        if not queries or not self.seqs:
            return []
        ca, la = plan.encode_many(queries)
        packed = sedgpu.PackedPairs.from_concat(ca, la, np.zeros(0, np.uint8), np.zeros(len(la), np.int32))
        h = getattr(self._dev, _dev)(plan, packed, max_dist)
        return list(zip(h["row"].tolist(), h["col"].tolist(), h["dist"].tolist()))

    def close(self):
        self._dev.close()


def join_index(seqs, userCosts=False, alphabet=None, engine=None, f64=False, long_seqs=False):
    """A JoinIndex over seqs (0..32 symbols each; long_seqs=True: 0..128, the integer route only): every pair within a
    distance, for clustering, de-duplication, neighbour graphs, or many queries against one collection.  engine(codes,
    off, lens) -> an object with self_join(plan, max_dist, (lo, hi)), search(plan, packed, max_dist), their
    self_join_f64 / search_f64, self_knn(plan, k, max_dist, (lo, hi)) and search_knn(plan, packed, k, max_dist), their
    self_knn_f64 / search_knn_f64, all returning sedgpu.JOIN_HIT_DTYPE records, and close() replaces the device (CPU tests); under long_seqs=True it is
    called with that keyword."""
    return JoinIndex(seqs, userCosts, alphabet, engine, f64, long_seqs)


def join_route(rows, seqs, max_dist, userCosts=False):
    """"int" or "f64": the join kernels that serve rows (str1) against seqs (str2) within max_dist.  The integer kernels
    whenever sedgpu.join_route says they serve the cost table over the symbols of both sides; the fp64 kernel when only
    it does.  A join neither serves, one with bad arguments, or one whose symbols the cost table does not resolve goes to
    the integer call, which raises what it always raised."""
    rows, seqs = list(rows), list(seqs)
    if not rows or not seqs:
        return "int"
    n = max(len(rows), len(seqs))  # every row and every sequence once: the plan's alphabet is the join's
    try:
        plan = batch_plan([rows[i % len(rows)] for i in range(n)], [seqs[i % len(seqs)] for i in range(n)], userCosts)
        costs = (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)
        route, _ = sedgpu.join_route(costs, {}, [len(r) for r in rows], [len(t) for t in seqs], False,
                                     sedgpu.codes_seen(plan.encode_many(rows)[0]),
                                     sedgpu.codes_seen(plan.encode_many(seqs)[0]), max_dist)
    except (KeyError, sedgpu.SedError):
        return "int"
    return "f64" if route == "f64" else "int"


def edit_script_batch(strs1, strs2, userCosts=False):
    """[(value, generate_es(create_paths(dp)[0], s1, s2))] for each pair — one GPU launch."""
    strs1, strs2 = list(strs1), list(strs2)
    plan = batch_plan(strs1, strs2, userCosts)
    if not strs1:
        return []
    ctx = sedgpu.context()
    ctx.set_costs(plan)
    packed = _packed(plan, strs1, strs2)
    dist, is_int, ln, ops = ctx.run(packed, True)
    out = []
    for p, (a, b) in enumerate(zip(strs1, strs2)):
        codes = sedgpu.unpack_ops(ops, packed.ops_off, p, int(ln[p]))
        es = _sedhost.es_from_ops(codes.tobytes(), a, b)
        v = float(dist[p])
        out.append((int(v) if is_int[p] else v, es))
    return out


# ---------------------------------------------------------------------------
# the reference's import-time demo globals (StringEditDistance.py:459-466), on first access
# ---------------------------------------------------------------------------
_DEMO_NAMES = ("dp", "all_paths", "path", "es")
str1 = 'AGRGA'
str2 = 'AGGGAA'


def __getattr__(name):
    """PEP 562: the reference builds dp / all_paths / path / es for ('AGRGA', 'AGGGAA', user costs) and prints
    them when it is imported.  Here importing stays free of GPU work and output; the first access to any of
    these names computes them the same way (with the user costs loaded at that moment)."""
    if name in _DEMO_NAMES:
        g = globals()
        d = wagnerFisher('AGRGA', 'AGGGAA', True)
        paths = create_paths(d)
        last = None
        for last in paths:  # the reference's loop leaves path / es at the last path
            pass
        g["dp"], g["all_paths"], g["path"] = d, paths, last
        g["es"] = generate_es(last, 'AGRGA', 'AGGGAA')
        return g[name]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
