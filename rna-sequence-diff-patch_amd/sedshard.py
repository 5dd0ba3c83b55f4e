"""Multi-GPU sharding for batches of independent pairs.

One process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI on
MI355X).  Pairs are independent, so the data path has no collective: rank r
takes a contiguous block of pair (or query-row) indices, generates or loads its
own inputs, runs the engine, and only the fixed-size per-pair results travel,
once, to rank 0 (gather_to_rank0).  The same code runs over gloo on CPU tensors
for the tests.
"""
import math

import numpy as np


def shard_range(total, world, rank):
    """[start, stop) of a contiguous, near-equal block of `total` items for `rank`."""
    base, extra = divmod(total, world)
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


def gather_to_rank0(tensors, world, rank):
    """Gather 1-D tensors of per-rank length to rank 0 (pad to the max length,
    gather, trim).  Returns, on rank 0, one concatenated tensor per input; None elsewhere."""
    import torch
    import torch.distributed as dist
    n_local = torch.tensor([t.numel() for t in tensors], dtype=torch.int64, device=tensors[0].device)
    sizes = [torch.zeros_like(n_local) for _ in range(world)]
    dist.all_gather(sizes, n_local)
    sizes = torch.stack(sizes).cpu()
    out = []
    for k, t in enumerate(tensors):
        width = int(sizes[:, k].max())
        buf = torch.zeros(width, dtype=t.dtype, device=t.device)
        buf[:t.numel()] = t
        parts = [torch.empty_like(buf) for _ in range(world)] if rank == 0 else None
        dist.gather(buf, parts, dst=0)
        if rank == 0:
            out.append(torch.cat([p[:int(sizes[r, k])] for r, p in enumerate(parts)]))
    return out if rank == 0 else None


def all_vs_all(seqs, userCosts=False, world=1, rank=0, device=None, distance_fn=None):
    """Row block of the len(seqs) x len(seqs) matrix of dp[n][m].value
    (query = row = str1, document = column = str2, as IRMethods.search_collection
    orders them) computed on this rank's GPU, gathered to rank 0 as a float64
    numpy matrix (None on other ranks).  One engine launch per rank.
    distance_fn(strs1, strs2, userCosts) -> values replaces StringEditDistance.distance_batch
    (the CPU tests inject the oracle to check the sharding and reassembly)."""
    import torch
    if distance_fn is None:
        import StringEditDistance as SED
        distance_fn = SED.distance_batch
    lo, hi = shard_range(len(seqs), world, rank)
    q = [a for a in seqs[lo:hi] for _ in seqs]
    d = [b for _ in seqs[lo:hi] for b in seqs]
    vals = np.array(distance_fn(q, d, userCosts), dtype=np.float64) if q else np.zeros(0)
    if world == 1:
        return vals.reshape(hi - lo, len(seqs))
    t = torch.from_numpy(vals).to(device if device is not None else "cpu")
    got = gather_to_rank0([t], world, rank)
    if rank != 0:
        return None
    return got[0].cpu().numpy().reshape(len(seqs), len(seqs))


def neighbors(seqs, max_dist, userCosts=False, world=1, rank=0, device=None, join_fn=None, route="int",
              long_sequences=False):
    """Every ordered pair (i, j), i != j, of the short sequences seqs (0..32 symbols) whose distance from seqs[i] to
    seqs[j] is <= max_dist, as a numpy record array (row, col, dist) sorted by (row, col), on rank 0 (None on other
    ranks).  Rank r joins its block of rows, shard_range(len(seqs), world, r), against every sequence on its own GPU
    (StringEditDistance.join_index; every rank holds the whole collection, which is small: 32 bytes a sequence), and
    only its hits travel, once, to rank 0; the blocks are contiguous, so their concatenation is sorted.
    route: "int" (the default) runs the integer kernels, "f64" the fp64 kernel (any table of costs >= 0 over at most 16
    symbols: IUPAC collections under costs.json), "auto" the integer call whenever it serves this rank's rows
    (StringEditDistance.join_route), as wfsearch.JoinIndex takes it.
    join_fn(seqs, lo, hi, max_dist, userCosts) -> [(i, j, dist)] sorted replaces the engine (the CPU tests inject the
    oracle to check the sharding and reassembly); the fp64 route calls it with f64=True as a further, keyword argument.
    long_sequences=True serves sequences of 0..128 symbols through the integer route's long kernel
    (StringEditDistance.join_index(..., long_seqs=True); 128 bytes a sequence on every rank); join_fn is then called with
    long_seqs=True as a further, keyword argument.  It has no fp64 route yet: "f64" and "auto" raise ValueError."""
    import torch
    if route not in ("int", "f64", "auto"):
        raise ValueError("route must be one of int, f64, auto, not %r" % (route,))
    if long_sequences and route != "int":
        raise ValueError("the long join has no fp64 route yet: long_sequences=True takes route=\"int\", not %r" % (route,))
    if join_fn is None or route == "auto":
        import StringEditDistance as SED
    if join_fn is None:
        def join_fn(seqs, lo, hi, max_dist, userCosts, f64=False, long_seqs=False):
            ix = SED.join_index(seqs, userCosts, f64=route != "int", long_seqs=long_seqs)
            try:
                return (ix.self_join_f64 if f64 else ix.self_join)(max_dist, (lo, hi))
            finally:
                ix.close()
    lo, hi = shard_range(len(seqs), world, rank)
    if hi <= lo:
        hits = []
    elif long_sequences:
        hits = list(join_fn(seqs, lo, hi, max_dist, userCosts, long_seqs=True))
    elif (SED.join_route(seqs[lo:hi], seqs, max_dist, userCosts) if route == "auto" else route) == "f64":
        hits = list(join_fn(seqs, lo, hi, max_dist, userCosts, f64=True))
    else:
        hits = list(join_fn(seqs, lo, hi, max_dist, userCosts))
    return _hits_to_rank0(hits, world, rank, device, torch)


def _hits_to_rank0(hits, world, rank, device, torch):
    """This rank's (row, col, dist) tuples, in the ranks' order, as one record array on rank 0 (None elsewhere)."""
    dtype = np.dtype([("row", np.int32), ("col", np.int32), ("dist", np.float64)])
    rows = np.array([h[0] for h in hits], np.int32)
    cols = np.array([h[1] for h in hits], np.int32)
    dist = np.array([h[2] for h in hits], np.float64)
    if world > 1:
        dev = device if device is not None else "cpu"
        got = gather_to_rank0([torch.from_numpy(x).to(dev) for x in (rows, cols, dist)], world, rank)
        if rank != 0:
            return None
        rows, cols, dist = (g.cpu().numpy() for g in got)
    out = np.zeros(len(rows), dtype)
    out["row"], out["col"], out["dist"] = rows, cols, dist
    return out


def nearest_neighbors(seqs, k, max_dist=None, userCosts=False, world=1, rank=0, device=None, join_fn=None,
                      long_sequences=False, route="int"):
    """For every sequence i of seqs, its k nearest sequences j != i by the distance from seqs[i] to seqs[j] (k = 1..64;
    max_dist, None for no cap, leaves out what lies farther), as a numpy record array (row, col, dist) sorted by (row,
    dist, col), on rank 0 (None on other ranks).  Rows are independent: rank r takes its block of rows,
    shard_range(len(seqs), world, r), against every sequence on its own GPU (StringEditDistance.JoinIndex.self_nearest
    or, under route "f64" / "auto", self_nearest_f64), and the blocks are contiguous, so their concatenation is sorted by
    row.  route: as neighbors takes it ("auto" asks with max_dist None as +inf); the fp64 route calls join_fn with
    f64=True as a further, keyword argument, and with long_sequences=True "f64" and "auto" raise ValueError.
    join_fn(seqs, lo, hi, k, max_dist, userCosts) -> [(i, j, dist)] sorted replaces the engine (CPU tests), as for
    neighbors; long_sequences=True serves sequences of 0..128 symbols, and join_fn is then called with long_seqs=True as
    a further, keyword argument."""
    import torch
    if route not in ("int", "f64", "auto"):
        raise ValueError("route must be one of int, f64, auto, not %r" % (route,))
    if long_sequences and route != "int":
        raise ValueError("the long join has no fp64 route yet: long_sequences=True takes route=\"int\", not %r" % (route,))
    if join_fn is None or route == "auto":
        import StringEditDistance as SED
    if join_fn is None:
        def join_fn(seqs, lo, hi, k, max_dist, userCosts, f64=False, long_seqs=False):
            ix = SED.join_index(seqs, userCosts, f64=route != "int", long_seqs=long_seqs)
            try:
                return (ix.self_nearest_f64 if f64 else ix.self_nearest)(k, max_dist, (lo, hi))
            finally:
                ix.close()
    lo, hi = shard_range(len(seqs), world, rank)
    if hi <= lo:
        hits = []
    elif long_sequences:
        hits = list(join_fn(seqs, lo, hi, k, max_dist, userCosts, long_seqs=True))
    elif (SED.join_route(seqs[lo:hi], seqs, math.inf if max_dist is None else max_dist, userCosts)
          if route == "auto" else route) == "f64":
        hits = list(join_fn(seqs, lo, hi, k, max_dist, userCosts, f64=True))
    else:
        hits = list(join_fn(seqs, lo, hi, k, max_dist, userCosts))
    return _hits_to_rank0(hits, world, rank, device, torch)
