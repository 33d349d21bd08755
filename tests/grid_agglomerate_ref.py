"""numpy restatement of conv3p_grid_agglomerate_segments (include/conv3p_graph.h, rules H1-H10), twice.

agglomerate_ref works on the adjacency alone, as the kernels do, but vectorised: the combined edges by np.unique over
root(src) * S + root(dst), the proposals by np.maximum.at of H4's key, the result by merge_ref on the log, the contracted
graph by np.unique again -- no hash table, no radix sort, no atomics.

agglomerate_slow never contracts anything: every round it runs adjacency_ref on the CURRENT segmentation -- the walk over
all voxels the device call avoids -- chooses by H4 with plain loops over the rows of that graph, and applies merge_ref;
the contracted graph is adjacency_ref of the result.  That the two agree is H8's claim that contacts and offsets are
additive under a merge.
"""
import numpy as np

from tests.grid_adjacency_ref import adjacency_ref, merge_ref

TOP = 0x7fffffff
GRAPH_KEYS = ("start", "src", "dst", "contacts", "offset", "twin")
LOG_KEYS = ("log_a", "log_b", "log_round", "log_contacts")
SEG_KEYS = ("seg_map", "segment", "root", "size", "rows", "label", "stats", "merge_stats")
ALL_KEYS = SEG_KEYS + ("voxel_label",) + LOG_KEYS + GRAPH_KEYS + ("agg_stats",)


def _roots_after(S, pairs):
    """root[s] for s < S after the pairs are joined transitively: the lowest number of the class."""
    parent = list(range(S))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(s) for s in range(S)], dtype=np.int64)


def _finish(seg, log, unusable, rounds, small, cand, graph):
    """The outputs from the log rows [(a, b, round, contacts)], the census and the contracted graph."""
    M = np.asarray(seg["segment"]).size
    out = {k: np.full(M, -1 if k != "log_contacts" else 0, dtype=np.int32) for k in LOG_KEYS}
    for i, row in enumerate(log):
        for k, v in zip(LOG_KEYS, row):
            out[k][i] = v
    m = merge_ref(seg, out["log_a"], out["log_b"])                             # H7
    out.update({k: m[k] for k in SEG_KEYS})
    inside = m["segment"] >= 0
    out["voxel_label"] = np.where(inside, m["label"][np.maximum(m["segment"], 0)], -1).astype(np.int32)
    out.update(graph)
    E = int((graph["src"] >= 0).sum())
    out["agg_stats"] = np.array([m["stats"][0], m["merge_stats"][1], rounds, len(log), small, cand, int(unusable), E], dtype=np.int64)
    return out


def _empty_graph(M, max_edges):
    g = dict(start=np.zeros(M + 1, np.int32), offset=np.zeros((max_edges, 3), np.int32), contacts=np.zeros(max_edges, np.int32))
    for k in ("src", "dst", "twin"):
        g[k] = np.full(max_edges, -1, dtype=np.int32)
    return g


def _group_label(seg, S, grp):
    """H2: per root segment, the seg_label of the member with the largest seg_size, the lowest number on a tie."""
    key = (np.maximum(np.asarray(seg["size"], dtype=np.int64)[:S], 0) << 32) | (TOP - np.arange(S, dtype=np.int64))
    best = np.zeros(S, dtype=np.int64)
    np.maximum.at(best, grp, key)
    return np.asarray(seg["label"], dtype=np.int64)[(TOP - (best & TOP)) % max(S, 1)]


def agglomerate_ref(seg, adj, min_size, weight=0, same_label=0, min_contacts=1, max_rounds=8):
    """seg: the dict of segments_ref or merge_ref; adj: the dict of adjacency_ref made from it -> dict of ALL_KEYS."""
    segment = np.asarray(seg["segment"])
    M = segment.size
    S = min(max(int(seg["stats"][0]), 0), M)
    E, max_edges = int(adj["stats"][0]), int(np.asarray(adj["src"]).shape[0])
    weights = np.asarray(seg["rows"] if weight else seg["size"], dtype=np.int64)[:S]
    if E < 0 or E > max_edges:                                                  # H1
        return _finish(seg, [], True, 0, int((weights < min_size).sum()), 0, _empty_graph(M, max_edges))
    src, dst = np.asarray(adj["src"], dtype=np.int64)[:E], np.asarray(adj["dst"], dtype=np.int64)[:E]
    ok = (src >= 0) & (src < S) & (dst >= 0) & (dst < S)
    src, dst = src[ok], dst[ok]
    con, off = np.asarray(adj["contacts"], dtype=np.int64)[:E][ok], np.asarray(adj["offset"], dtype=np.int64)[:E][ok]

    def contract(of, n):
        """The combined edges under the map `of` onto [0, n) -> (a, b, contacts, offset), in ascending (a, b)."""
        g, h = of[src], of[dst]
        cross = g != h
        uniq, inv = np.unique(g[cross] * max(n, 1) + h[cross], return_inverse=True)
        inv = inv.reshape(-1)
        c, o = np.zeros(uniq.size, np.int64), np.zeros((uniq.size, 3), np.int64)
        np.add.at(c, inv, con[cross])
        np.add.at(o, inv, off[cross])
        return uniq // max(n, 1), uniq % max(n, 1), c, o

    def choose(grp):
        """H3, H4 -> best int64 (S): the key of every root's proposal, 0 for none; W per root."""
        W = np.zeros(S, np.int64)
        np.add.at(W, grp, weights)
        a, b, c, _ = contract(grp, S)
        cand = (W[a] < min_size) & (c >= min_contacts)
        if same_label:
            lab = _group_label(seg, S, grp)
            cand &= lab[a] == lab[b]
        key = ((W[b] >= min_size).astype(np.int64) << 62) | (c << 31) | (TOP - b)
        best = np.zeros(S, np.int64)
        np.maximum.at(best, a[cand], key[cand])
        return best, W

    grp = np.arange(S, dtype=np.int64)
    log, rounds = [], 0
    for k in range(max_rounds):                                                 # H5
        best, _ = choose(grp)
        g = np.nonzero(best)[0]
        if g.size == 0:
            break
        h = TOP - (best[g] & TOP)
        mutual = (best[h] != 0) & (TOP - (best[h] & TOP) == g)
        logged = ~mutual | (g < h)                                              # H6: g ascends
        log += [(int(x), int(y), k, int(z)) for x, y, z in zip(g[logged], h[logged], (best[g] >> 31)[logged] & TOP)]
        grp = _roots_after(S, zip(g.tolist(), h.tolist()))[grp]
        rounds += 1
    best, W = choose(grp)
    small = (grp == np.arange(S)) & (W < min_size)
    out = _finish(seg, log, False, rounds, int(small.sum()), int((best != 0).sum()), _empty_graph(M, max_edges))
    G = int(out["stats"][0])
    a, b, c, o = contract(np.asarray(out["seg_map"], dtype=np.int64), G)        # H8
    n = a.size
    for k, v in (("src", a), ("dst", b), ("contacts", c), ("offset", o), ("twin", np.searchsorted(a * max(G, 1) + b, b * max(G, 1) + a))):
        out[k][:n] = v
    out["start"] = np.searchsorted(a, np.arange(M + 1)).astype(np.int32)
    out["agg_stats"][7] = n
    return out


def agglomerate_slow(neigh, seg, ne, connectivity, max_edges, min_size, weight=0, same_label=0, min_contacts=1, max_rounds=8):
    """The same from the voxels, round by round (see the module's docstring) -> dict of ALL_KEYS.  The input adjacency
    is the one adjacency_ref gives at `connectivity`; an overflow (H1) is the caller's to test."""
    M = np.asarray(seg["segment"]).size
    S = min(max(int(seg["stats"][0]), 0), M)
    cur, total = seg, np.arange(S)                                              # total: original segment -> current group
    size0, label0 = np.asarray(seg["size"]), np.asarray(seg["label"])
    log, rounds, left = [], 0, (0, 0)
    for k in range(max_rounds + 1):
        G = int(cur["stats"][0])
        adj = adjacency_ref(neigh, cur["segment"], G, ne, connectivity, 26 * M)
        members = [[] for _ in range(G)]
        for s in range(S):
            members[total[s]].append(s)
        W = [int(cur["rows" if weight else "size"][g]) for g in range(G)]
        lab = [int(label0[max(m, key=lambda s: (size0[s], -s))]) for m in members]
        prop = {}
        for g in range(G):
            if W[g] >= min_size:
                continue
            best = None
            for e in range(adj["start"][g], adj["start"][g + 1]):
                h, c = int(adj["dst"][e]), int(adj["contacts"][e])
                if c < min_contacts or (same_label and lab[g] != lab[h]):
                    continue
                key = (W[h] >= min_size, c, -h)
                if best is None or key > best[0]:
                    best = (key, h, c)
            if best is not None:
                prop[g] = best[1:]
        left = (sum(w < min_size for w in W), len(prop))
        if k == max_rounds or not prop:
            break
        rows = [(g, h, c) for g, (h, c) in sorted(prop.items()) if not (h in prop and prop[h][0] == g and h < g)]
        log += [(members[g][0], members[h][0], k, c) for g, h, c in rows]
        cur = merge_ref(cur, [g for g, _, _ in rows], [h for _, h, _ in rows])
        total = cur["seg_map"][total]
        rounds += 1
    result = _finish(seg, log, False, rounds, left[0], left[1], _empty_graph(M, max_edges))
    for key in ("segment", "root", "size", "rows"):                            # the iterated merges are the merge on the log
        assert np.array_equal(result[key], cur[key]), key
    g = adjacency_ref(neigh, result["segment"], int(result["stats"][0]), ne, connectivity, max_edges)
    result.update({key: g[key] for key in GRAPH_KEYS})
    result["agg_stats"][7] = max(int(g["stats"][0]), 0)
    return result


# ------------------------------------------------------------------------------------- the fields the tests share
def random_classes(cells, seed=5, classes=13):
    """A label per voxel drawn from `classes`: nearly every voxel its own segment at 6."""
    return np.random.default_rng(seed).integers(0, classes, cells.shape[0]).astype(np.int32)


def redrawn_slabs(cells, seed=11, thick=2, classes=13, share=0.05):
    """Slabs `thick` cells high, the label the slab's number, with `share` of the voxels redrawn from `classes`: a few large
    segments strewn with specks, some of which touch each other."""
    rng = np.random.default_rng(seed)
    lab = (cells[:, 2] // thick).astype(np.int32)
    redraw = rng.random(cells.shape[0]) < share
    lab[redraw] = rng.integers(0, classes, int(redraw.sum()))
    return lab
