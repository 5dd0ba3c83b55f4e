"""Batched one-vs-many Wagner-Fischer search.

The reference scores a query against every document of the collection with one full
`wagnerFisher` per pair (`IRMethods.search_collection`, IRMethods.py:443-477, method
`wf_score`, :435-440), and `create_search_threads` runs that search twice per query
(:487-491 and :511-515).  Here the whole collection is one engine launch (short piRNA
documents go to the lane-per-pair kernel), and repeated searches with the same query,
documents and cost table are answered from a small cache.

    search_collection(query, vector_type, collection, wf_score, return_dict=None, callback=None)

has the reference's signature and output: a list of (doc['sequence'], score) in
`collection.find({})` order, delivered through callback / return_dict['wf_score'] /
the return value exactly like the reference.  Other scoring methods (tf/idf vectors, set
similarities) are not on the engine's path and raise NotImplementedError.
"""
import math
from collections import OrderedDict

import StringEditDistance as SED
import sedgpu

_CACHE = OrderedDict()
_CACHE_SIZE = 8


def wf_score(seq1, seq2, user_cost=False):
    """IRMethods.wf_score (IRMethods.py:435-440): 1 / (1 + dp[n][m].value)."""
    dp = SED.wagnerFisher(seq1, seq2, user_cost)
    cost = dp[len(dp) - 1][len(dp[0]) - 1].value
    return 1 / (1 + cost)


def wf_scores(query, seqs, user_cost=False):
    """[wf_score(query, s, user_cost) for s in seqs] with one engine launch (cached)."""
    seqs = list(seqs)
    if not seqs:
        return []
    queries = [query] * len(seqs)
    plan = SED.batch_plan(queries, seqs, user_cost)  # the reference raises on the first offending document, in order
    key = (query, tuple(seqs), plan.key())
    hit = _CACHE.get(key)
    if hit is not None:
        _CACHE.move_to_end(key)
        return list(hit)
    vals = SED.distance_batch(queries, seqs, user_cost, plan=plan)
    scores = [1 / (1 + v) for v in vals]
    _CACHE[key] = tuple(scores)
    while len(_CACHE) > _CACHE_SIZE:
        _CACHE.popitem(last=False)
    return scores


def clear_cache():
    _CACHE.clear()


def _sequences(seqs_or_collection):
    """A list of sequences, or a collection's doc['sequence'] in find({}) order."""
    if hasattr(seqs_or_collection, 'find'):
        return [doc['sequence'] for doc in seqs_or_collection.find({})]
    return list(seqs_or_collection)


def search_within(query, seqs_or_collection, max_dist, user_cost=False):
    """[(sequence, 1 / (1 + d))] for the documents whose distance d from query is <= max_dist, in collection order,
    with one engine launch that skips the cells no path within max_dist can reach.  A batch extension (the
    reference scores every document); not cached."""
    seqs = _sequences(seqs_or_collection)
    if not seqs:
        return []
    vals = SED.distance_batch([query] * len(seqs), seqs, user_cost, max_dist=max_dist)
    return [(s, 1 / (1 + v)) for s, v in zip(seqs, vals) if v != math.inf]


def nearest(query, seqs, k, user_cost=False, distance_fn=None):
    """The k documents of smallest distance from query as [(sequence, 1 / (1 + d))], nearest first, ties in
    collection order.  One resident batch runs under a cutoff that starts at the k-th smallest length-difference
    lower bound (at least insert + delete) and doubles until k documents are within it or it has reached the largest
    n delete + m insert; the far documents are never computed in full.  Those k are the true top k: every document
    outside the last cutoff T has d > T, and T is >= each of theirs.
    distance_fn(queries, seqs, max_dist) -> [d or math.inf] replaces the engine (CPU tests).  Not cached."""
    seqs = _sequences(seqs)
    k = min(int(k), len(seqs))
    if k <= 0:
        return []
    queries = [query] * len(seqs)
    plan = SED.batch_plan(queries, seqs, user_cost)
    ins, dele, n = plan.ins, plan.dele, len(query)
    bounds = sorted(ins * max(len(s) - n, 0) + dele * max(n - len(s), 0) for s in seqs)
    last = max(max(n * dele + len(s) * ins for s in seqs), 0)
    first = max(bounds[k - 1], ins + dele)
    first = min(first if first > 0 else 1, last)
    if distance_fn is None:
        vals, _ = SED.distance_deepen(queries, seqs, k, first, last, user_cost, plan=plan)
    else:
        cut = first
        while True:
            vals = list(distance_fn(queries, seqs, cut))
            if sum(v != math.inf for v in vals) >= k or cut >= last:
                break
            cut = min(2 * cut, last)
    order = sorted((v, i) for i, v in enumerate(vals) if v != math.inf)[:k]
    return [(seqs[i], 1 / (1 + v)) for v, i in order]


ROUTES = ("int", "f64", "auto")


def fit_route(queries, seqs, user_cost=False):
    """"int" or "f64": the fit kernels that serve these queries against these documents (route="auto").  The integer
    kernels whenever sedgpu.fit_route says they serve the cost table over the symbols of queries and documents, the
    longest query and the longest document; the fp64 kernels when only they do.  A search neither serves, or one whose
    symbols the cost table does not resolve, goes to the integer call, which raises what it always raised."""
    queries, seqs = list(queries), list(seqs)
    if not queries or not seqs:
        return "int"
    n = max(len(queries), len(seqs))  # every query and every document once: the plan's alphabet is the search's
    try:
        plan = SED.batch_plan([queries[i % len(queries)] for i in range(n)], [seqs[i % len(seqs)] for i in range(n)],
                              user_cost)
    except KeyError:
        return "int"
    costs = (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)
    longest = max(map(len, seqs))
    route, _ = sedgpu.fit_route(costs, {}, [len(q) for q in queries], [longest] * len(queries))
    return "f64" if route == "f64" else "int"


def fit_long_route(queries, seqs, user_cost=False):
    """fit_route for the long calls of an index (queries of up to 2048 symbols): "int" whenever
    sedgpu.fit_long_route says the integer long calls serve these queries against these documents, "f64" when only
    the fp64 long calls do; a search neither serves goes to the integer call, as in fit_route."""
    queries, seqs = list(queries), list(seqs)
    if not queries or not seqs:
        return "int"
    n = max(len(queries), len(seqs))
    try:
        plan = SED.batch_plan([queries[i % len(queries)] for i in range(n)], [seqs[i % len(seqs)] for i in range(n)],
                              user_cost)
    except KeyError:
        return "int"
    costs = (plan.K, plan.sub, plan.sub_int, plan.ins, plan.ins_int, plan.dele, plan.del_int)
    route, _ = sedgpu.fit_long_route(costs, {}, [len(q) for q in queries], [len(s) for s in seqs])
    return "f64" if route == "f64" else "int"


def _resolve_route(route, queries, seqs, user_cost):
    if route not in ROUTES:
        raise ValueError("route must be one of %s, not %r" % (", ".join(ROUTES), route))
    return fit_route(queries, seqs, user_cost) if route == "auto" else route


def fit_search(query, seqs_or_collection, user_cost=False, max_dist=None, scripts=False, fit_fn=None, route="int"):
    """Where in each document does query occur, approximately: [(sequence, 1 / (1 + dist), start, end)] in collection
    order, dist = the smallest distance from query to any substring sequence[start:end] (the one ending earliest, then
    the shortest; StringEditDistance.fit_batch), one engine launch for the collection.  max_dist keeps only the hits
    with dist <= max_dist.  scripts=True appends the edit script of (query, sequence[start:end]) to each kept hit, from
    one edit_script_batch call; patching(es, query) then gives the matched substring.
    route: "int" (the default) runs the integer kernels, which serve dyadic cost tables over at most 8 symbols and raise
    SedError otherwise; "f64" runs the fp64 kernels, which serve any table of costs >= 0 over at most 16 symbols (IUPAC
    documents under costs.json); "auto" takes the integer kernels whenever they serve the search (fit_route).  The
    scripts need no route: the batch engine has its own fp64 path.
    fit_fn(patterns, texts, user_cost) -> [(dist, start, end)] replaces the engine (CPU tests); the fp64 route calls it
    with f64=True as a fourth, keyword argument.  Not cached."""
    seqs = _sequences(seqs_or_collection)
    if not seqs:
        return []
    engine = fit_fn or SED.fit_batch
    if _resolve_route(route, [query], seqs, user_cost) == "f64":
        hits = engine([query] * len(seqs), seqs, user_cost, f64=True)
    else:
        hits = engine([query] * len(seqs), seqs, user_cost)
    kept = [(s, d, a, b) for s, (d, a, b) in zip(seqs, hits) if max_dist is None or d <= max_dist]
    out = [(s, 1 / (1 + d), a, b) for s, d, a, b in kept]
    if scripts and kept:
        es = SED.edit_script_batch([query] * len(kept), [s[a:b] for s, _, a, b in kept], user_cost)
        out = [hit + (e,) for hit, (_, e) in zip(out, es)]
    return out


class FitIndex:
    """fit_search for a collection that is searched query after query: the documents are encoded and uploaded once
    (StringEditDistance.fit_index), and each search sends only its queries.

        ix = FitIndex(collection, user_cost=True)
        ix.search(query, max_dist=3)          # == fit_search(query, collection, True, max_dist=3)
        ix.search_many(queries)               # one such list per query, from one engine launch
        ix.occurrences(query, max_dist=3)     # every site within 3 of every document, not only the best one

    index_fn(sequences, user_cost) -> an object with search(patterns) -> [[(dist, start, end)] per sequence] per
    pattern, hits(patterns, max_dist) -> [(pattern index, sequence index, start, end, dist)] sorted, and close(),
    replaces the engine (CPU tests).  Not cached.

    long_patterns=True (search, search_many, occurrences, occurrences_many) serves queries of up to 2048 symbols: those
    of at most 32 go through the calls above, the longer ones through the index's search_long / hits_long, and the
    results merge in query order.  The default refuses a query over 32 as before.

    route (the constructor's, and per call on search, search_many, occurrences, occurrences_many; None = the
    constructor's): "int", "f64" or "auto" as fit_search takes it.  It holds for the short and, apart, for the long
    queries of a call: under "f64" the long ones run the index's search_long_f64 / hits_long_f64, under "auto" they
    take the integer long calls whenever fit_long_route says those serve them and the fp64 long calls otherwise, so
    only a refusal turns into a result.  An index whose constructor route is "f64" or "auto" is built with f64=True (up to 16
    symbols; index_fn is called with that keyword), and serves integer searches too; one built under the default keeps
    the 8-symbol bound, whatever route a later call names.  The fp64 route calls the index's search_f64 / hits_f64."""

    SHORT = 32  # the longest query search() / hits() serve

    def __init__(self, seqs_or_collection, user_cost=False, index_fn=None, route="int"):
        if route not in ROUTES:
            raise ValueError("route must be one of %s, not %r" % (", ".join(ROUTES), route))
        self.seqs = _sequences(seqs_or_collection)
        self.user_cost = user_cost
        self.route = route
        make = index_fn or SED.fit_index
        self._ix = (make(self.seqs, user_cost) if route == "int" else make(self.seqs, user_cost, f64=True)) \
            if self.seqs else None

    def _calls(self, route, queries, short):
        """(the search call, the hits call) that serve the short queries under route"""
        r = _resolve_route(self.route if route is None else route, [queries[i] for i in short], self.seqs,
                           self.user_cost) if short else "int"
        return (self._ix.search_f64, self._ix.hits_f64) if r == "f64" else (self._ix.search, self._ix.hits)

    def _long_calls(self, route, queries, lng):
        """(the search call, the hits call) that serve the long queries under route"""
        route = self.route if route is None else route
        if route not in ROUTES:
            raise ValueError("route must be one of %s, not %r" % (", ".join(ROUTES), route))
        r = "int" if not lng or route == "int" else \
            fit_long_route([queries[i] for i in lng], self.seqs, self.user_cost) if route == "auto" else route
        return (self._ix.search_long_f64, self._ix.hits_long_f64) if r == "f64" else \
            (getattr(self._ix, "search_long", None), getattr(self._ix, "hits_long", None))

    def _split(self, queries, long_patterns):
        """(indices the short calls serve, indices the long calls serve)"""
        if not long_patterns:
            return list(range(len(queries))), []
        return ([i for i, q in enumerate(queries) if len(q) <= self.SHORT],
                [i for i, q in enumerate(queries) if len(q) > self.SHORT])

    def search_many(self, queries, max_dist=None, scripts=False, long_patterns=False, route=None):
        queries = list(queries)
        if not self.seqs:
            return [[] for _ in queries]
        if not queries:
            return []
        short, lng = self._split(queries, long_patterns)
        rows = [None] * len(queries)
        for idx, call in ((short, self._calls(route, queries, short)[0]), (lng, self._long_calls(route, queries, lng)[0])):
            if idx:
                for i, r in zip(idx, call([queries[i] for i in idx])):
                    rows[i] = r
        kept = [[(s, d, a, b) for s, (d, a, b) in zip(self.seqs, hits) if max_dist is None or d <= max_dist]
                for hits in rows]
        out = [[(s, 1 / (1 + d), a, b) for s, d, a, b in k] for k in kept]
        if scripts and any(kept):  # the scripts of every kept hit of every query: one edit_script_batch call
            flat = [(q, s[a:b]) for q, k in zip(queries, kept) for s, _, a, b in k]
            es = iter(SED.edit_script_batch([q for q, _ in flat], [w for _, w in flat], self.user_cost))
            out = [[hit + (next(es)[1],) for hit in o] for o in out]
        return out

    def search(self, query, max_dist=None, scripts=False, long_patterns=False, route=None):
        return self.search_many([query], max_dist, scripts, long_patterns, route)[0]

    def occurrences_many(self, queries, max_dist, all_ends=False, scripts=False, long_patterns=False, route=None):
        """For each query, [(sequence, 1 / (1 + d), start, end)] for every occurrence within max_dist, in collection
        order, then by end: one engine launch for all the queries (StringEditDistance.FitIndex.hits).  A hit is an end
        column e of a document whose best distance E(e) = min over s of d(query, sequence[s:e]) is <= max_dist, with
        the largest such s as start; the occurrences are the hits that are local minima of E (local_minima): the
        earliest end of every valley or plateau, search()'s best hit among them.  all_ends=True returns every hit
        unfiltered.  scripts=True appends each returned tuple's edit script of (query, sequence[start:end]), all from
        one edit_script_batch call; patching(es, query) then gives sequence[start:end]."""
        queries = list(queries)
        if not self.seqs:
            return [[] for _ in queries]
        if not queries:
            return []
        short, lng = self._split(queries, long_patterns)
        hits = []
        for idx, call in ((short, self._calls(route, queries, short)[1]), (lng, self._long_calls(route, queries, lng)[1])):
            if idx:
                hits += [(idx[q], t, a, b, d) for q, t, a, b, d in call([queries[i] for i in idx], max_dist)]
        hits.sort(key=lambda h: (h[0], h[1], h[3]))  # (each call's list is sorted; the merge is by query)
        kept = hits if all_ends else local_minima(hits)
        out = [[] for _ in queries]
        for q, t, a, b, d in kept:
            out[q].append((self.seqs[t], 1 / (1 + d), a, b))
        if scripts and kept:
            es = iter(SED.edit_script_batch([queries[q] for q, _, _, _, _ in kept],
                                            [self.seqs[t][a:b] for _, t, a, b, _ in kept], self.user_cost))
            out = [[hit + (next(es)[1],) for hit in o] for o in out]
        return out

    def occurrences(self, query, max_dist, all_ends=False, scripts=False, long_patterns=False, route=None):
        return self.occurrences_many([query], max_dist, all_ends, scripts, long_patterns, route)[0]

    def close(self):
        if self._ix is not None:
            self._ix.close()
        self._ix = None


def local_minima(hits):
    """The occurrences among hits = [(query, text, start, end, dist)] sorted by (query, text, end): a hit at end e is
    kept iff E(e) < E(e - 1) and E(e) <= E(e + 1), where E of a column that is no hit (or lies outside the text)
    counts as +inf - it exceeds the cutoff, and every hit is within it.  So the rule needs the hit list alone."""
    out = []
    for i, h in enumerate(hits):
        q, t, _, e, d = h
        prev = hits[i - 1] if i > 0 else None
        nxt = hits[i + 1] if i + 1 < len(hits) else None
        before = prev[4] if prev is not None and prev[:2] == (q, t) and prev[3] == e - 1 else math.inf
        after = nxt[4] if nxt is not None and nxt[:2] == (q, t) and nxt[3] == e + 1 else math.inf
        if d < before and d <= after:
            out.append(h)
    return out


def fit_occurrences(query, seqs_or_collection, max_dist, user_cost=False, all_ends=False, scripts=False, index_fn=None,
                    long_patterns=False, route="int"):
    """FitIndex.occurrences in one shot: builds an index over the documents, searches it and closes it."""
    ix = FitIndex(seqs_or_collection, user_cost, index_fn=index_fn, route=route)
    try:
        return ix.occurrences(query, max_dist, all_ends, scripts, long_patterns)
    finally:
        ix.close()


class JoinIndex:
    """Every pair of short sequences (0..32 symbols) within a distance, for a collection that stays on the device
    (StringEditDistance.join_index): clustering, de-duplication, neighbour graphs, many queries against one collection.

        ix = JoinIndex(collection, user_cost=True)
        ix.neighbors(2)                      # [(i, j, 1 / (1 + d))] for every i != j with d(seq i -> seq j) <= 2
        ix.search_many(queries, 2)           # per query, == search_within(query, collection, 2, True)
        ix.search(query, 2)
        ix.nearest(8)                        # per sequence i, its 8 nearest [(j, 1 / (1 + d))], nearest first
        ix.nearest_many(queries, 8)          # per query, its 8 nearest [(sequence, score)]

    Rows (i, the queries) are str1 and columns (j, the documents) str2, the direction of wf_score(query, doc).
    index_fn(sequences, user_cost) -> an object with self_join(max_dist, rows) -> [(i, j, d)] and
    search(queries, max_dist) -> [(q, j, d)], both sorted, self_nearest(k, max_dist, rows) and search_nearest(queries, k,
    max_dist) -> the same records sorted by (row, d, j), and close(), replaces the engine (CPU tests).  Not cached.

    route (the constructor's, and per call on neighbors, search_many, search, nearest, nearest_many; None = the
    constructor's): "int" (the
    default) runs the integer kernels, which serve dyadic cost tables over at most 8 symbols and raise SedError
    otherwise; "f64" runs the fp64 kernel, which serves any table of costs >= 0 over at most 16 symbols (IUPAC
    collections under costs.json); "auto" takes the integer call whenever it serves the join
    (StringEditDistance.join_route), so only a refusal turns into a result.  An index whose constructor route is "f64"
    or "auto" is built with f64=True (up to 16 symbols; index_fn is called with that keyword) and serves integer calls
    too; one built under the default keeps the 8-symbol bound, whatever route a later call names.  The fp64 route calls
    the index's self_join_f64 / search_f64, and self_nearest_f64 / search_nearest_f64 for nearest / nearest_many
    (max_dist None counts as +inf when "auto" asks which route serves); where the integer route serves a table both
    routes return identical lists.

    long_sequences=True serves sequences and queries of 0..128 symbols (tRNA, pre-miRNA hairpins, 5S rRNA) through the
    integer route's long kernel (StringEditDistance.join_index(..., long_seqs=True); index_fn is called with
    long_seqs=True).  It has no fp64 route yet: "f64" and "auto" raise ValueError, at the constructor and per call."""

    def __init__(self, seqs_or_collection, user_cost=False, index_fn=None, route="int", long_sequences=False):
        if route not in ROUTES:
            raise ValueError("route must be one of %s, not %r" % (", ".join(ROUTES), route))
        self.long_sequences = bool(long_sequences)
        self._no_f64(route)
        self.seqs = _sequences(seqs_or_collection)
        self.user_cost = user_cost
        self.route = route
        make = index_fn or SED.join_index
        if self.long_sequences:
            self._ix = make(self.seqs, user_cost, long_seqs=True) if self.seqs else None
            return
        self._ix = (make(self.seqs, user_cost) if route == "int" else make(self.seqs, user_cost, f64=True)) \
            if self.seqs else None

    def _no_f64(self, route):
        if self.long_sequences and route != "int":
            raise ValueError("the long join has no fp64 route yet: long_sequences=True takes route=\"int\", not %r" % (route,))

    def _f64(self, route, rows, max_dist):
        """whether the fp64 calls serve these rows under route"""
        route = self.route if route is None else route
        if route not in ROUTES:
            raise ValueError("route must be one of %s, not %r" % (", ".join(ROUTES), route))
        self._no_f64(route)
        return (SED.join_route(rows, self.seqs, max_dist, self.user_cost) if route == "auto" else route) == "f64"

    def neighbors(self, max_dist, rows=None, route=None):
        """[(i, j, 1 / (1 + d))] sorted by (i, j): every ordered pair i != j, i in rows = (lo, hi) (default: all), whose
        distance d from sequence i to sequence j is <= max_dist."""
        if self._ix is None:
            return []
        lo, hi = (0, len(self.seqs)) if rows is None else rows
        call = self._ix.self_join_f64 if self._f64(route, self.seqs[lo:hi], max_dist) else self._ix.self_join
        return [(i, j, 1 / (1 + d)) for i, j, d in call(max_dist, rows)]

    def search_many(self, queries, max_dist, route=None):
        """Per query, [(sequence, 1 / (1 + d))] for the documents within max_dist, in collection order: what
        search_within(query, seqs, max_dist, user_cost) returns, for all the queries from one engine call."""
        queries = list(queries)
        out = [[] for _ in queries]
        if self._ix is None or not queries:
            return out
        call = self._ix.search_f64 if self._f64(route, queries, max_dist) else self._ix.search
        for q, j, d in call(queries, max_dist):
            out[q].append((self.seqs[j], 1 / (1 + d)))
        return out

    def search(self, query, max_dist, route=None):
        return self.search_many([query], max_dist, route)[0]

    def nearest(self, k, max_dist=None, rows=None, route=None):
        """Per sequence i of rows = (lo, hi) (default: all), [(j, 1 / (1 + d))] for its k nearest sequences j != i by the
        distance d from sequence i to sequence j, nearest first, ties going to the lower j; max_dist (None: no cap)
        leaves out what lies farther, so a list may be shorter than k.  k = 1..64; exact."""
        lo, hi = (0, len(self.seqs)) if rows is None else rows
        if self._ix is None:  # (an empty collection: what the index would refuse is refused here)
            SED.JoinIndex.check_k(k)
            if (lo, hi) != (0, 0):
                raise ValueError("rows=(%r, %r) is no range of the index's 0 sequences" % (lo, hi))
            return []
        out = [[] for _ in range(lo, hi)]
        f64 = self._f64(route, self.seqs[lo:hi], math.inf if max_dist is None else max_dist)
        for i, j, d in (self._ix.self_nearest_f64 if f64 else self._ix.self_nearest)(k, max_dist, rows):
            out[i - lo].append((j, 1 / (1 + d)))
        return out

    def nearest_many(self, queries, k, max_dist=None, route=None):
        """Per query, [(sequence, 1 / (1 + d))] for its k nearest documents, nearest first: nearest(query, seqs, k) for
        all the queries from one engine call (ties go to the document that comes first in the collection)."""
        queries = list(queries)
        out = [[] for _ in queries]
        if self._ix is None:
            SED.JoinIndex.check_k(k)
            return out
        f64 = self._f64(route, queries, math.inf if max_dist is None else max_dist)
        for q, j, d in (self._ix.search_nearest_f64 if f64 else self._ix.search_nearest)(queries, k, max_dist):
            out[q].append((self.seqs[j], 1 / (1 + d)))
        return out

    def close(self):
        if self._ix is not None:
            self._ix.close()
        self._ix = None


def neighbors(seqs_or_collection, max_dist, user_cost=False, index_fn=None, route="int", long_sequences=False):
    """JoinIndex.neighbors in one shot: builds an index over the sequences, joins it with itself and closes it."""
    ix = JoinIndex(seqs_or_collection, user_cost, index_fn=index_fn, route=route, long_sequences=long_sequences)
    try:
        return ix.neighbors(max_dist)
    finally:
        ix.close()


def nearest_neighbors(seqs_or_collection, k, max_dist=None, user_cost=False, index_fn=None, long_sequences=False,
                      route="int"):
    """JoinIndex.nearest in one shot: builds an index over the sequences, takes every sequence's k nearest and closes it."""
    ix = JoinIndex(seqs_or_collection, user_cost, index_fn=index_fn, route=route, long_sequences=long_sequences)
    try:
        return ix.nearest(k, max_dist)
    finally:
        ix.close()


def search_collection(query, vector_type, collection, method, return_dict=None, callback=None):
    """IRMethods.search_collection for method == wf_score (IRMethods.py:443-477)."""
    if getattr(method, '__name__', None) != 'wf_score':
        raise NotImplementedError("only the wf_score method runs on the edit-distance engine")
    seqs = [doc['sequence'] for doc in collection.find({})]
    scores = list(zip(seqs, wf_scores(query, seqs)))
    if callback is not None:
        callback(scores)
    elif return_dict is not None:
        return_dict[method.__name__] = scores
    else:
        return scores
