"""numpy restatement of conv3p_grid_segments and conv3p_grid_absorb_segments (include/conv3p.h, rules S1-S4 and A1-A4).

A plain union-find over the directed relation of S2 as it is written -- every tap of every labelled voxel, not the half
the kernels use -- so a kernel that leans on the table's symmetry is checked against a reference that does not.
"""
import numpy as np


def taps(connectivity):
    """The taps t != 13 of a connectivity, t = (dx+1)*9 + (dy+1)*3 + (dz+1)."""
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for t in range(27):
        d = abs(t // 9 - 1) + abs(t // 3 % 3 - 1) + abs(t % 3 - 1)
        if 1 <= d <= reach:
            out.append(t)
    return out


def voxel_labelling(labels, L, ne, num_class, M):
    """S1 -> int64 (M): the label of every labelled voxel, -1 for the others."""
    lab = np.full(M, -1, dtype=np.int64)
    if labels is None:
        lab[:ne] = 0
        return lab
    n = min(int(L), ne)
    src = np.asarray(labels[:n], dtype=np.int64)
    lab[:n] = np.where((src >= 0) & (src < num_class), src, -1)
    return lab


def segments_ref(neigh, labels, L, voxel_count, ne, num_class, connectivity):
    """-> dict(segment, root, size, rows, label: int32 (M); stats: int32 (8))."""
    neigh = np.asarray(neigh)
    M = neigh.shape[0]
    ne = min(max(int(ne), 0), M)
    lab = voxel_labelling(labels, L, ne, 1 if labels is None else num_class, M)
    parent = list(range(M))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for t in taps(connectivity):
        col = neigh[:, t].astype(np.int64)
        ok = (lab >= 0) & (col >= 0) & (col < ne)
        ok[ok] = lab[col[ok]] == lab[ok]
        for v in np.nonzero(ok)[0]:
            a, b = find(int(v)), find(int(col[v]))
            if a != b:
                parent[max(a, b)] = min(a, b)
    root_of = np.array([find(v) if lab[v] >= 0 else -1 for v in range(M)], dtype=np.int64)
    roots = np.nonzero((root_of == np.arange(M)) & (lab >= 0))[0]
    S = roots.size
    rank = np.full(M, -1, dtype=np.int64)
    rank[roots] = np.arange(S)
    segment = np.where(lab >= 0, rank[np.maximum(root_of, 0)], -1).astype(np.int32)
    root = np.full(M, -1, dtype=np.int32)
    size = np.zeros(M, dtype=np.int32)
    rows = np.zeros(M, dtype=np.int32)
    label = np.full(M, -1, dtype=np.int32)
    root[:S] = roots
    label[:S] = lab[roots]
    inside = segment >= 0
    size[:S] = np.bincount(segment[inside], minlength=S)[:S]
    rows[:S] = np.bincount(segment[inside], weights=np.asarray(voxel_count)[inside].astype(np.float64), minlength=S)[:S]
    stats = np.array([S, inside.sum(), ne - inside.sum(), M - ne, size.max(initial=0), rows.max(initial=0), 0, 0],
                     dtype=np.int32)
    return dict(segment=segment, root=root, size=size, rows=rows, label=label, stats=stats)


def absorb_ref(neigh, labels, L, seg, ne, num_class, connectivity, min_size, drop_orphans):
    """seg: the dict of segments_ref -> dict(labels: int32 (M), seg_label: int32 (M), stats: int64 (4))."""
    neigh = np.asarray(neigh)
    M = neigh.shape[0]
    ne = min(max(int(ne), 0), M)
    segment, size, label = seg["segment"], seg["size"], seg["label"]
    S = int(seg["stats"][0])
    if labels is None:
        num_class = 1
    small = np.zeros(M, dtype=bool)
    small[:S] = size[:S] < min_size
    votes = np.zeros((S, num_class), dtype=np.int64)
    for t in taps(connectivity):
        col = neigh[:, t].astype(np.int64)
        s_u = segment.astype(np.int64)
        ok = (s_u >= 0) & (col >= 0) & (col < ne)
        ok[ok] = small[s_u[ok]]
        s_w = np.full(M, -1, dtype=np.int64)
        s_w[ok] = segment[col[ok]]
        ok &= (s_w >= 0) & (s_w != s_u)
        ok[ok] = ~small[s_w[ok]]
        np.add.at(votes, (s_u[ok], label[s_w[ok]].astype(np.int64)), 1)
    seg_label = np.full(M, -1, dtype=np.int32)
    seg_label[:S] = label[:S]
    absorbed = orphans = changed = 0
    for s in np.nonzero(small)[0]:
        if votes[s].max(initial=0) > 0:
            seg_label[s] = int(np.argmax(votes[s]))           # the first of equal maxima: the lowest class
            absorbed += 1
        else:
            orphans += 1
            if drop_orphans:
                seg_label[s] = -1
        if seg_label[s] != label[s]:
            changed += int(size[s])
    out = np.full(M, -1, dtype=np.int32)
    if labels is not None:
        n = min(int(L), ne)
        out[:n] = np.asarray(labels[:n], dtype=np.int32)
    inside = segment >= 0
    out[inside] = seg_label[segment[inside]]
    stats = np.array([int(small.sum()), absorbed, orphans, changed], dtype=np.int64)
    return dict(labels=out, seg_label=seg_label, stats=stats)


def lattice_table(occ):
    """A dense lattice's occupancy (nx, ny, nz) bool -> (neigh int32 (M, 27), cells (M, 3)): the voxels in ascending (i, j, l)
    as conv3p_grid_subsample numbers them, the table as rule N2 of include/conv3p.h defines it."""
    occ = np.asarray(occ, dtype=bool)
    cells = np.argwhere(occ)                                   # C order: ascending (i, j, l)
    M = cells.shape[0]
    number = np.full(tuple(s + 2 for s in occ.shape), -1, dtype=np.int32)
    number[1:-1, 1:-1, 1:-1][occ] = np.arange(M, dtype=np.int32)
    neigh = np.full((M, 27), -1, dtype=np.int32)
    for t in range(27):
        dx, dy, dz = t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1
        neigh[:, t] = number[cells[:, 0] + 1 + dx, cells[:, 1] + 1 + dy, cells[:, 2] + 1 + dz]
    return neigh, cells
