"""From a scan to a class per raw row through smooth patches (-m gpu): a synthetic room of a floor, a wall and a box, xyz +
rgb, 3000 rows -> grid_subsample (mean) -> GridSubsample.normals -> segments(normals=nrm, max_angle=15, max_curvature=0.05)
-> GridSegments.adjacency -> a policy written as a torch expression (every patch below 8 voxels joins the LARGE patch it
shares the most contacts with, the lowest edge on a tie: one edge a patch, so no two large patches are bridged) ->
SegmentAdjacency.merge -> GridSegments.pool of noisy per-voxel class scores (a SceneScores) -> GridSubsample.project of the
patches' classes.  Every stage equals its numpy reference to the bit, the references fed the device's own normals; the
interior of each plane ends up as one segment, the two differ, and every raw row of a plane's interior takes the plane's
class although a fifth of its voxels voted for another."""
import numpy as np
import pytest

from tests import grid_adjacency_ref as ga
from tests import grid_ref as gr
from tests import grid_smooth_ref as sm

F = np.float32
VOXEL, MAX_ANGLE, MAX_CURVATURE, MIN_SIZE, NCLS = 0.1, 15, 0.05, 8, 3
ADJ = ("start", "src", "dst", "contacts", "voxels", "offset", "twin", "border", "stats")
SEG = ("segment", "root", "size", "rows", "label", "stats")


def room(n=3000, seed=8101):
    """A floor z = 0 of 2.4 x 2.4, a wall x = 0 of 2.4 x 2.0 and the top and sides of a box of 0.6 standing on the floor,
    sampled exactly on their planes -> float32 (n, 6), xyz + rgb."""
    rng = np.random.default_rng(seed)
    k = n // 10
    parts = [np.c_[rng.random((4 * k, 2)) * 2.4, np.zeros(4 * k)],
             np.c_[np.zeros(4 * k), rng.random(4 * k) * 2.4, rng.random(4 * k) * 2.0]]
    per = (n - 8 * k) // 5
    for face in range(5):
        u, v, c = rng.random(per) * 0.6, rng.random(per) * 0.6, np.ones(per)
        parts.append([np.c_[1.2 + u, 0.9 + v, 0.6 * c], np.c_[1.2 * c, 0.9 + u, v], np.c_[1.8 * c, 0.9 + u, v],
                      np.c_[1.2 + u, 0.9 * c, v], np.c_[1.2 + u, 1.5 * c, v]][face])
    xyz = np.concatenate(parts)
    return np.c_[xyz, rng.random((xyz.shape[0], 3))].astype(F)


@pytest.mark.gpu
def test_a_room_s_planes_become_patches_that_vote_for_their_class():
    import torch
    from pointwise_amd import _lib, grid, scene
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data = room()
    N = data.shape[0]
    want = gr.grid_subsample_ref(data, None, voxel=VOXEL, mode="mean")
    V = int(want["stats"][0])
    g = grid.grid_subsample(torch.from_numpy(data).to(dev), None, voxel=VOXEL).trim()
    assert g.num_voxels() == V
    nrm = g.normals()
    seg = g.segments(normals=nrm, max_angle=MAX_ANGLE, max_curvature=MAX_CURVATURE)
    adj = seg.adjacency()
    if adj.overflowed():
        adj = seg.adjacency(max_edges=adj.edges_bound())  # always fits
    assert not adj.overflowed()
    rows_e, E = adj.shape[1], adj.num_edges()
    # the policy, on the device: one edge per small patch, into a large one
    src, dst, contacts = adj.src[:E].long(), adj.dst[:E].long(), adj.contacts[:E].long()
    ok = (seg.size[src] < MIN_SIZE) & (seg.size[dst] >= MIN_SIZE)
    key = torch.where(ok, contacts * rows_e + (rows_e - 1 - torch.arange(E, device=dev)), torch.full_like(contacts, -1))
    best = torch.full((V,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, src, key, "amax")
    select = torch.zeros(rows_e, dtype=torch.bool, device=dev)
    select[:E] = ok & (key == best[src])
    merged = adj.merge(select)
    # the votes: the class of a voxel's plane, a fifth of the voxels drawn at random, three votes a voxel
    xyz = g.data[:, :3].cpu().numpy()
    truth = np.where(xyz[:, 2] == 0, 0, np.where(xyz[:, 0] == 0, 1, 2)).astype(np.int64)
    rng = np.random.default_rng(8102)
    noisy = np.where(rng.random(V) < 0.2, rng.integers(0, NCLS, V), truth)
    logits = rng.standard_normal((3, V, NCLS)).astype(F)
    logits[:, np.arange(V), noisy] += 4.0
    scores = scene.SceneScores(V, NCLS, dev)
    index = torch.arange(V, dtype=torch.int32, device=dev)
    for k in range(3):
        scores.add(torch.from_numpy(logits[k]).to(dev), index)
    pool = merged.pool(scores.scores)
    rows_out = g.project(pool.voxel_label).cpu().numpy()

    # every stage against its reference, fed the device's own normals
    neigh, count = g.neighbors().cpu().numpy(), g.voxel_count.cpu().numpy()
    n, f, c = nrm.normals.cpu().numpy(), nrm.flags.cpu().numpy(), nrm.curvature.cpu().numpy()
    ref = sm.smooth_segments_ref(neigh, None, 0, count, V, None, 26, normals=n, flags=f, curvature=c,
                                 min_cos=sm.min_cos_of(MAX_ANGLE), max_curvature=MAX_CURVATURE)
    for k in SEG + ("smooth_stats",):
        assert np.array_equal(getattr(seg, k).cpu().numpy(), ref[k]), k
    S = int(ref["stats"][0])
    ref_adj = ga.adjacency_ref(neigh, ref["segment"], S, V, 26, rows_e)
    for k in ADJ:
        assert np.array_equal(getattr(adj, k).cpu().numpy(), ref_adj[k]), k
    rs, rd, rc = ref_adj["src"][:E], ref_adj["dst"][:E], ref_adj["contacts"][:E].astype(np.int64)
    rok = (ref["size"][rs] < MIN_SIZE) & (ref["size"][rd] >= MIN_SIZE)
    rkey = np.where(rok, rc * rows_e + (rows_e - 1 - np.arange(E)), -1)
    top = np.full(V, -1, np.int64)
    np.maximum.at(top, rs, rkey)
    sel = np.zeros(rows_e, bool)
    sel[:E] = rok & (rkey == top[rs])
    assert np.array_equal(select.cpu().numpy(), sel)
    ref_m = ga.merge_ref(ref, ref_adj["src"], ref_adj["dst"], sel)
    for k in SEG + ("seg_map", "merge_stats"):
        assert np.array_equal(getattr(merged, k).cpu().numpy(), ref_m[k]), k
    S2 = int(ref_m["stats"][0])
    ref_p = sm.pool_ref(scores.scores.cpu().numpy(), ref_m["segment"], S2, count, V, 0)
    for k in ("sums", "weights", "label", "voxel_label", "stats"):
        assert np.array_equal(getattr(pool, k).cpu().numpy(), ref_p[k]), k
    assert np.array_equal(pool.mean.cpu().numpy().view(np.int64), ref_p["mean"].view(np.int64))
    assert np.array_equal(rows_out, gr.project_ref(ref_p["voxel_label"], want["inverse"]))

    # what it is for: the interior of each plane is one patch, and the patch's class repairs its voxels' votes
    inside = lambda a, lo, hi: (a > lo + 0.25) & (a < hi - 0.25)
    box = (xyz[:, 0] > 0.95) & (xyz[:, 0] < 2.05) & (xyz[:, 1] > 0.65) & (xyz[:, 1] < 1.75)
    floor = (xyz[:, 2] == 0) & inside(xyz[:, 0], 0.0, 2.4) & inside(xyz[:, 1], 0.0, 2.4) & ~box
    wall = (xyz[:, 0] == 0) & inside(xyz[:, 1], 0.0, 2.4) & inside(xyz[:, 2], 0.0, 2.0)
    ms = ref_m["segment"]
    print("%d rows, %d voxels, %d patches -> %d after the merge; smooth_stats %s; floor interior %d voxels, wall %d"
          % (N, V, S, S2, ref["smooth_stats"].tolist(), floor.sum(), wall.sum()))
    assert floor.sum() > 150 and wall.sum() > 150 and S2 < S
    assert len(set(ms[floor])) == 1 and len(set(ms[wall])) == 1 and ms[floor][0] != ms[wall][0]
    voted = scores.labels().cpu().numpy()
    assert (voted[floor] != 0).any() and (voted[wall] != 1).any()              # the votes alone are noisy ...
    assert (ref_p["voxel_label"][floor] == 0).all() and (ref_p["voxel_label"][wall] == 1).all()     # ... the patches are not
    inv = want["inverse"]
    assert (rows_out[floor[inv]] == 0).all() and (rows_out[wall[inv]] == 1).all()
