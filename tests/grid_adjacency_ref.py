"""numpy restatement of conv3p_grid_segment_adjacency and conv3p_grid_merge_segments (include/conv3p.h, rules E1-E7 and
U1-U5).

The adjacency is vectorised: the (voxel, tap) pairs of E2 as a mask over (M, taps), keys a * S + b, np.unique -- no loop
over voxels, no hash table, no sort of its own, so the kernels' table, runs and radix passes are checked against none of
themselves.  The merge is a plain union-find over the active pairs.
"""
import numpy as np

from tests.grid_segments_ref import taps

FILLER = dict(src=-1, dst=-1, contacts=0, voxels=0, offset=0, twin=-1)


def tap_offsets(connectivity):
    """(taps, 3) int64: (dx, dy, dz) of every tap of the connectivity, in ascending t."""
    return np.array([(t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1) for t in taps(connectivity)], dtype=np.int64)


def adjacency_ref(neigh, segment, S, ne, connectivity, max_edges):
    """-> dict(start int32 (M + 1); src, dst, contacts, voxels, twin int32 (max_edges); offset int32 (max_edges, 3); border
    int32 (M, 4); stats int64 (8))."""
    neigh = np.asarray(neigh)
    M = neigh.shape[0]
    ne = min(max(int(ne), 0), M)
    S = min(max(int(S), 0), M)
    seg = np.asarray(segment, dtype=np.int64)
    member = (np.arange(M) < ne) & (seg >= 0) & (seg < S)                      # E1
    a_of = np.where(member, seg, -1)
    tp = np.array(taps(connectivity))
    nb = neigh[:, tp].astype(np.int64)
    has = (nb >= 0) & (nb < ne)
    b = np.where(has, a_of[np.clip(nb, 0, max(M - 1, 0))], -2)                 # -2: no neighbour, -1: a member of nothing
    contact = member[:, None] & (b >= 0) & (b != a_of[:, None])                # E2
    kinds = np.stack([contact.sum(1), (member[:, None] & (b == -1)).sum(1), (member[:, None] & (b == -2)).sum(1)], axis=1)
    kinds = np.concatenate([kinds, (kinds.sum(1) > 0)[:, None]], axis=1)
    border = np.zeros((M, 4), dtype=np.int64)                                  # E6
    np.add.at(border, a_of[member], kinds[member])

    v_idx, t_idx = np.nonzero(contact)
    key = a_of[v_idx] * max(S, 1) + b[v_idx, t_idx]
    uniq, inv, contacts = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    E = uniq.size
    src, dst = uniq // max(S, 1), uniq % max(S, 1)
    offset = np.zeros((E, 3), dtype=np.int64)
    np.add.at(offset, inv, tap_offsets(connectivity)[t_idx])
    pairs = np.unique(key * M + v_idx)                                         # (edge, voxel) once each
    voxels = np.bincount(np.searchsorted(uniq, pairs // M), minlength=E)
    B = pairs.size
    twin = np.searchsorted(uniq, dst * max(S, 1) + src)
    start = np.searchsorted(src, np.arange(M + 1))                             # E5: E past S, since src < S

    out = dict(start=np.zeros(M + 1, np.int32), border=border.astype(np.int32))
    rows = int(max_edges)
    for k, fill in FILLER.items():
        out[k] = np.full((rows, 3) if k == "offset" else (rows,), fill, dtype=np.int32)
    total = int(contact.sum())
    if E <= rows:                                                              # E7
        out["start"] = start.astype(np.int32)
        for k, val in (("src", src), ("dst", dst), ("contacts", contacts), ("voxels", voxels), ("offset", offset), ("twin", twin)):
            out[k][:E] = val
        degree = np.diff(start)
        out["stats"] = np.array([E, B, S, total, degree.max(initial=0), contacts.max(initial=0), 0, 0], dtype=np.int64)
    else:
        out["stats"] = np.array([-1, B, S, total, 0, 0, 1, 0], dtype=np.int64)
    return out


def adjacency_loops(neigh, segment, S, ne, connectivity):
    """The same by loops over voxels and taps, for the hand cases: dict (a, b) -> [contacts, set of voxels, offset], and
    border as a list of rows."""
    M = len(neigh)
    edges, border = {}, [[0, 0, 0, 0] for _ in range(M)]

    def member(v):
        return segment[v] if v < ne and 0 <= segment[v] < S else -1

    for v in range(M):
        a = member(v)
        if a < 0:
            continue
        surface = False
        for t in taps(connectivity):
            w = int(neigh[v][t])
            if w < 0 or w >= ne:
                border[a][2] += 1
            elif member(w) < 0:
                border[a][1] += 1
            elif member(w) != a:
                border[a][0] += 1
                e = edges.setdefault((int(a), int(member(w))), [0, set(), [0, 0, 0]])
                e[0] += 1
                e[1].add(v)
                for k, d in enumerate((t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1)):
                    e[2][k] += d
            else:
                continue
            surface = True
        border[a][3] += surface
    return edges, border


def merge_ref(seg, pair_a, pair_b, select=None):
    """seg: the dict of grid_segments_ref.segments_ref (or of merge_ref) -> dict(seg_map, segment, root, size, rows, label:
    int32 (M); stats: int32 (8); merge_stats: int32 (4))."""
    segment = np.asarray(seg["segment"], dtype=np.int64)
    M = segment.size
    S = min(max(int(seg["stats"][0]), 0), M)
    pa, pb = np.asarray(pair_a, dtype=np.int64).reshape(-1), np.asarray(pair_b, dtype=np.int64).reshape(-1)
    active = np.ones(pa.size, bool) if select is None else np.asarray(select).reshape(-1) != 0
    active &= (pa >= 0) & (pa < S) & (pb >= 0) & (pb < S) & (pa != pb)         # U1
    parent = list(range(S))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b in zip(pa[active].tolist(), pb[active].tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    root_of = np.array([find(s) for s in range(S)], dtype=np.int64)
    roots = np.nonzero(root_of == np.arange(S))[0]                             # U2: ascending root segment
    G = roots.size
    rank = np.full(max(S, 1), -1, dtype=np.int64)
    rank[roots] = np.arange(G)
    seg_map = np.full(M, -1, dtype=np.int32)
    seg_map[:S] = rank[root_of]
    out = dict(seg_map=seg_map)
    inside = (segment >= 0) & (segment < S)
    out["segment"] = np.where(inside, seg_map[np.clip(segment, 0, max(M - 1, 0))], -1).astype(np.int32)
    root = np.full(M, -1, dtype=np.int32)
    size = np.zeros(M, dtype=np.int32)
    rows = np.zeros(M, dtype=np.int32)
    label = np.full(M, -1, dtype=np.int32)
    root[:G] = np.asarray(seg["root"])[roots]
    np.add.at(size, seg_map[:S], np.asarray(seg["size"])[:S])
    np.add.at(rows, seg_map[:S], np.asarray(seg["rows"])[:S])
    # the member with the largest size, the lowest number on a tie: a stable sort by (group, -size)
    order = np.lexsort((np.arange(S), -np.asarray(seg["size"], dtype=np.int64)[:S], seg_map[:S]))
    firsts = order[np.concatenate([[True], seg_map[:S][order][1:] != seg_map[:S][order][:-1]])] if S else order
    label[:G] = np.asarray(seg["label"])[firsts]
    stats = np.array(seg["stats"], dtype=np.int32).copy()
    stats[0], stats[4], stats[5], stats[6], stats[7] = G, size.max(initial=0), rows.max(initial=0), 0, 0
    out.update(root=root, size=size, rows=rows, label=label, stats=stats)
    out["merge_stats"] = np.array([G, S, int(active.sum()), int((np.bincount(seg_map[:S], minlength=1) > 1).sum())], dtype=np.int32)
    return out
