"""GPU tests (-m gpu) of the k-nearest-voxel search, GridSubsample.knn on conv3p_grid_knn_f32, and of its consumers
GridKnn.interpolate and GridKnn.normals: every output bit for bit against tests/grid_knn_ref.py on the cases of
tests/grid_knn_cases.py -- exact ties, a full lattice, a sparse one, two slabs, the corner cell, two rooms that overlap in
space, rows with NaN / inf and rows of cut voxels -- over k, rings, exclude_self, valid_labels and both kinds of query, into
outputs prefilled with garbage; representatives displaced out of their cells and a wrong lattice step; the identities with
the plain and the ring interpolation; reproducibility and out=; the normals of every case and of a checkerboard sheet whose
voxels are alone in their 27 cells."""
import functools

import numpy as np
import pytest

from tests import grid_interp_ref as gi
from tests import grid_knn_cases as kc
from tests import grid_knn_ref as kr
from tests import grid_normals_ref as gn

pytestmark = pytest.mark.gpu
F = np.float32
OUTPUTS = ("index", "d2", "count", "ring", "scanned", "certified", "stats")


def _dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(name, trimmed):
    """A case subsampled on the device, once -> (the case, its data on the device, the subsampling, what the reference
    reads of it)."""
    import torch
    from pointwise_amd import grid
    c = kc.build(name)
    d = torch.from_numpy(np.ascontiguousarray(c["data"])).to(_dev())
    kw = dict(voxel=c["voxel"], mode=c["mode"], max_voxels=c["max_voxels"])
    if c["room_start"] is None:
        g = grid.grid_subsample(d, None, **kw)
    else:
        g = grid.grid_subsample_rooms(d, torch.from_numpy(c["room_start"]).to(d.device), None, **kw)
    g = g.trim() if trimmed else g
    return c, d, g, host(g)


def host(g):
    h = dict(inverse=g.inverse.cpu().numpy(), data=g.data.cpu().numpy(), cell=g.voxel_cell.cpu().numpy(), nv=int(g.stats[0]),
             room=None, start=None)
    if getattr(g, "voxel_room", None) is not None:
        h.update(room=g.voxel_room.cpu().numpy(), start=g.voxel_start.cpu().numpy())
    return h


def garbage(dev, Q, k):
    """A GridKnn whose every word is set to something the call never writes."""
    from pointwise_amd import grid
    out = grid.GridKnn(Q, k, dev)
    out.index.fill_(0x5a5a5a5a)
    out.d2.fill_(-7.0)
    for t in (out.count, out.ring, out.scanned, out.certified):
        t.fill_(-77)
    out.stats.fill_(-(1 << 40))
    return out


def same(got, ref, what):
    for name in OUTPUTS:
        gi.assert_same(getattr(got, name).cpu().numpy(), ref[name], "%s: %s" % (what, name))


def search_of(c, d, h, voxel_queries, exclude_self, valid, voxel=None, voxel_data=None):
    q, qv = (h["data"] if voxel_data is None else voxel_data, None) if voxel_queries else (c["data"], h["inverse"])
    return kr.Search(q, qv, h["data"] if voxel_data is None else voxel_data, h["cell"], h["nv"], c["voxel"] if voxel is None else voxel,
                     exclude_self, valid, h["room"], h["start"])


# ------------------------------------------------------------------------------------------------ 1. the cases, swept
@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("voxel_queries", [True, False])
@pytest.mark.parametrize("name", kc.NAMES)
def test_every_case_over_k_rings_and_valid_labels(name, voxel_queries, exclude_self):
    import torch
    c, d, g, h = case(name, trimmed=exclude_self)
    M = g.data.shape[0]
    Q = M if voxel_queries else d.shape[0]
    for valid in (None, c["valid"](h["cell"], h["nv"], M)):
        s = search_of(c, d, h, voxel_queries, exclude_self, valid)
        vt = None if valid is None else torch.from_numpy(valid).to(d.device)
        for k in kc.KS:
            for rings in kc.RINGS:
                ref = kr.knn_ref(None, None, None, None, None, None, k, rings, search=s)
                got = g.knn(c["voxel"], None if voxel_queries else d, k=k, rings=rings, valid_labels=vt, exclude_self=exclude_self,
                            out=garbage(d.device, Q, k))
                same(got, ref, "%s, %s, k = %d, rings = %d, exclude_self = %s, valid %s" % (
                    name, "voxels" if voxel_queries else "rows", k, rings, exclude_self, valid is not None))
                assert got.num_certified() == int(ref["certified"].sum())


def test_exact_ties_come_in_ascending_voxel_number():
    c, d, g, h = case("centres", False)
    got = g.knn(c["voxel"], k=8, rings=2)
    index, d2 = got.index.cpu().numpy()[:h["nv"]], got.d2.cpu().numpy()[:h["nv"]]
    interior = ((h["cell"][:h["nv"]] >= 1) & (h["cell"][:h["nv"]] <= 4)).all(axis=1)
    assert interior.sum() == 64 and (d2[interior, 1:7] == F(0.0625)).all() and (np.diff(index[interior, 1:7], axis=1) > 0).all()
    assert (index[:, 0] == np.arange(h["nv"])).all() and (d2[:, 0] == 0).all()


def test_a_raw_row_table_with_any_query_voxel_and_an_empty_call():
    """query_voxel given: rows handed to other voxels than their own, to none (-1) and to numbers past the voxels."""
    import torch
    from pointwise_amd import grid
    c, d, g, h = case("lattice", True)
    rng = np.random.default_rng(5)
    qv = h["inverse"].copy()
    qv[::7] = -1
    qv[3::11] = h["nv"] + 5
    qv[5::13] = rng.integers(0, h["nv"], size=qv[5::13].size)
    s = kr.Search(c["data"], qv, h["data"], h["cell"], h["nv"], c["voxel"])
    got = g.knn(c["voxel"], d, query_voxel=torch.from_numpy(qv).to(d.device), k=5, rings=4, out=garbage(d.device, d.shape[0], 5))
    same(got, kr.knn_ref(None, None, None, None, None, None, 5, 4, search=s), "any query_voxel")
    e = grid.grid_subsample(torch.zeros((0, 4), device=d.device), None, voxel=0.1)
    t = e.knn(0.1, out=garbage(d.device, 0, 8))
    assert t.stats.cpu().tolist() == [0] * 16 and t.index.shape == (0, 8)


# --------------------------------------------------------------------------- 2. what a stop rule must not assume
@pytest.mark.parametrize("voxel_queries", [True, False])
@pytest.mark.parametrize("what", ["displaced", "voxel / 3", "voxel * 3"])
def test_displaced_representatives_and_a_wrong_step_keep_the_neighbours(what, voxel_queries):
    """voxel_data with xyz displaced by up to 1.5 voxels, the cells unchanged, and a step three times too small or too
    large: the neighbours still equal K3 / K4.  A stop rule that took the representatives to lie in their cells fails here."""
    import torch
    c, d, g0, h = case("lattice", True)
    g = g0.trim()                                        # views of its own to overwrite: the cached object stays as it is
    vd = kc.displaced(h["data"], c["voxel"], 7) if what == "displaced" else h["data"]
    g.data = torch.from_numpy(vd).to(d.device)
    voxel = float(F(c["voxel"] * {"displaced": 1.0, "voxel / 3": 1 / 3, "voxel * 3": 3.0}[what]))
    plain = search_of(c, d, h, voxel_queries, False, None, voxel_data=vd)
    s = search_of(c, d, h, voxel_queries, False, None, voxel=voxel, voxel_data=vd)
    for k in (3, 8):
        for rings in (2, 8):
            ref = kr.knn_ref(None, None, None, None, None, None, k, rings, search=s)
            got = g.knn(voxel, None if voxel_queries else d, k=k, rings=rings, out=garbage(d.device, s.Q, k))
            same(got, ref, "%s, k = %d, rings = %d" % (what, k, rings))
            index, d2, count, ring = plain.kept(k, rings)                # K3 / K4 know nothing of the step
            gi.assert_same(got.index.cpu().numpy(), index, what + ": index against K4")
            gi.assert_same(got.d2.cpu().numpy(), d2, what + ": d2 against K4")
            kr.check_theorem(ref, k, rings)


# ----------------------------------------------------------------------------------------------------- 3. identities
def scores_for(M, C, seed, entry, dev, voted=None):
    """float32 (M, C) scores as a tensor, or a SceneScores with votes on the voxels `voted`."""
    import torch
    from pointwise_amd import scene
    rng = np.random.default_rng(seed)
    if entry == "f32":
        return torch.from_numpy(rng.standard_normal((M, C)).astype(F)).to(dev)
    s = scene.SceneScores(M, C, dev)
    rows = np.nonzero(voted >= 0)[0].astype(np.int32)
    s.add(torch.from_numpy((rng.standard_normal((rows.size, C)) * 4).astype(F)).to(dev), torch.from_numpy(rows).to(dev))
    return s


@pytest.mark.parametrize("entry", ["f32", "i64"])
@pytest.mark.parametrize("name", ["lattice", "sparse", "rooms", "nonfinite"])
def test_a_table_of_one_ring_interpolates_as_the_plain_call_does(name, entry):
    import torch
    c, d, g, h = case(name, True)
    M = g.data.shape[0]
    valid = c["valid"](h["cell"], h["nv"], M)
    s = scores_for(M, 13, 9, entry, d.device, valid)
    v = torch.from_numpy(valid).to(d.device) if entry == "f32" else None
    want = g.interpolate(d, s, k=3, valid_labels=v, return_scores=True)
    got = g.knn(c["voxel"], d, k=3, rings=1, valid_labels=v if entry == "f32" else s).interpolate(s, return_scores=True)
    gi.assert_same(got[0].cpu().numpy(), want[0].cpu().numpy(), "labels")
    gi.assert_same(got[1].cpu().numpy(), want[1].cpu().numpy(), "scores")
    assert (want[0] >= 0).any()


@pytest.mark.parametrize("name", ["slabs", "sparse", "corner"])
def test_a_table_of_r_rings_labels_the_rows_the_ring_call_labels(name):
    import torch
    c, d, g, h = case(name, True)
    M = g.data.shape[0]
    valid = c["valid"](h["cell"], h["nv"], M)
    s, v = scores_for(M, 13, 10, "f32", d.device), torch.from_numpy(valid).to(d.device)
    seen = set()
    for rings in range(1, 9):
        want = g.interpolate(d, s, valid_labels=v, rings=rings) >= 0
        got = g.knn(c["voxel"], d, k=3, rings=rings, valid_labels=v).interpolate(s) >= 0
        assert torch.equal(got, want), rings
        seen.add(int(want.sum()))
    assert len(seen) > 1                                 # more rings label more rows


def test_two_calls_and_out_reuse_give_the_same_bits():
    c, d, g, h = case("sparse", False)
    a = g.knn(c["voxel"], d, k=8, rings=8)
    keep = {name: getattr(a, name).cpu().numpy().copy() for name in OUTPUTS}
    b = g.knn(c["voxel"], d, k=8, rings=8)
    same(b, keep, "a second call")
    g.knn(c["voxel"], d, k=8, rings=1, out=a)            # other contents first
    assert not np.array_equal(a.scanned.cpu().numpy(), keep["scanned"])
    assert g.knn(c["voxel"], d, k=8, rings=8, out=a) is a
    same(a, keep, "out=")
    s = scores_for(g.data.shape[0], 5, 11, "f32", d.device)
    x = a.interpolate(s, return_scores=True)
    lab, sc = x[0].clone(), x[1].clone()
    x[0].fill_(99), x[1].fill_(99.0)
    y = a.interpolate(s, return_scores=True, out=x)
    assert y[0] is x[0] and y[1] is x[1]
    gi.assert_same(y[0].cpu().numpy(), lab.cpu().numpy(), "out= labels")
    gi.assert_same(y[1].cpu().numpy(), sc.cpu().numpy(), "out= scores")


# ------------------------------------------------------------------------------------------- 4. the interpolation
@pytest.mark.parametrize("entry", ["f32", "i64"])
@pytest.mark.parametrize("name", ["centres", "sparse", "rooms", "nonfinite"])
def test_the_interpolation_of_a_table_is_rule_five_on_its_entries(name, entry):
    import torch
    c, d, g, h = case(name, True)
    M = g.data.shape[0]
    valid = c["valid"](h["cell"], h["nv"], M)
    t = g.knn(c["voxel"], d, k=16, rings=4, valid_labels=torch.from_numpy(valid).to(d.device))
    index, count = t.index.cpu().numpy(), t.count.cpu().numpy()
    for C in (1, 13, 128):
        s = scores_for(M, C, 12 + C, entry, d.device, valid)
        sc = s.cpu().numpy() if entry == "f32" else s.scores.cpu().numpy()
        for k_use in (1, 3, 8, 16):
            lab = torch.full((d.shape[0],), 99, dtype=torch.int32, device=d.device)
            out = torch.full((d.shape[0], C), 99.0, device=d.device)
            t.interpolate(s, k=k_use, return_scores=True, out=(lab, out))
            want = kr.interpolate_knn_ref(c["data"], h["data"], index, count, sc, k_use)
            for nm, a, b in (("labels", lab, want[0]), ("scores", out, want[1]), ("stats", t.interp_stats, want[2])):
                gi.assert_same(a.cpu().numpy(), b, "%s %s, C = %d, k = %d: %s" % (name, entry, C, k_use, nm))
    # scores of fewer voxels than the table names: a row with such an entry among its first k has no neighbour
    few = max(1, M // 2)
    s = scores_for(few, 7, 13, "f32", d.device)
    lab, out = t.interpolate(s, k=3, return_scores=True)
    n = np.minimum(count, 3)
    bad = ((index[:, :3] >= few) & (np.arange(3)[None, :] < n[:, None])).any(axis=1)
    assert bad.any() and (~bad & (n > 0)).any()
    want = kr.interpolate_knn_ref(c["data"], h["data"], index, np.where(bad, 0, count), s.cpu().numpy(), 3)
    gi.assert_same(lab.cpu().numpy(), want[0], "short scores: labels")
    gi.assert_same(out.cpu().numpy(), want[1], "short scores: scores")
    gi.assert_same(t.interp_stats.cpu().numpy(), want[2], "short scores: stats")


# ------------------------------------------------------------------------------------------------------ 5. normals
def check_normals(g, h, t, min_neighbors, viewpoint=None, what=""):
    nrm = t.normals(viewpoint=viewpoint, min_neighbors=min_neighbors, return_moments=True)
    samples, flags, moments, stats = kr.normals_knn_ref(h["data"], t.index.cpu().numpy(), t.count.cpu().numpy(), h["nv"], min_neighbors)
    for name, a, b in (("samples", nrm.samples, samples), ("flags", nrm.flags, flags), ("moments", nrm.moments, moments),
                       ("stats", nrm.stats, stats)):
        gi.assert_same(a.cpu().numpy(), b, "%s: %s" % (what, name))
    vp = None if viewpoint is None else (viewpoint.cpu().numpy() if hasattr(viewpoint, "cpu") else np.asarray(viewpoint, F))
    compared = gn.compare_r5(nrm.normals.cpu().numpy(), nrm.curvature.cpu().numpy(), flags, moments, h["data"], viewpoint=vp,
                             voxel_room=h["room"])
    return nrm, flags, samples, compared


@pytest.mark.parametrize("name", kc.NAMES)
def test_the_normals_of_every_case(name):
    import torch
    c, d, g, h = case(name, name in ("sparse", "rooms"))
    seen = 0
    for k, rings, min_neighbors, exclude_self in ((9, 2, 6, False), (16, 4, 3, False), (16, 8, 16, False), (8, 2, 4, True), (3, 1, 3, False)):
        t = g.knn(c["voxel"], k=k, rings=rings, exclude_self=exclude_self)
        vp = None
        if k == 16 and rings == 4:
            vp = (0.3, -2.0, 5.0) if h["room"] is None else torch.tensor([[0.3, -2.0, 5.0], [9.0, 0.1, -4.0]], device=d.device)
        _, flags, samples, compared = check_normals(g, h, t, min_neighbors, vp, "%s, k = %d, rings = %d" % (name, k, rings))
        assert (samples[:h["nv"]] <= k).all()
        seen += int((flags == 0).sum())
    assert seen > 0 or name == "corner"                  # three voxels in a plane of their own: never 3 samples off a line


def test_a_checkerboard_sheet_has_no_normal_in_27_cells_and_one_from_its_nearest_nine():
    """One row in every cell (2a, 2b, 0), a, b < 8, z identical in all rows: each voxel's 27 cells hold itself alone.
    Within two rings a voxel has itself and its 8 neighbours of the sheet: 9 samples at the 36 interior voxels, 6 at the 24
    on an edge, 4 at the 4 corners."""
    import torch
    from pointwise_amd import grid
    data = kc.checkerboard(8, 0.25)
    d = torch.from_numpy(data).to(_dev())
    g = grid.grid_subsample(d, None, voxel=0.25, mode="center").trim()
    h = host(g)
    assert h["nv"] == 64 and (h["cell"][:, 2] == 0).all() and (h["cell"][:, :2] % 2 == 0).all()
    plain = g.normals()
    assert (plain.flags == 1).all() and (plain.samples == 1).all()
    t = g.knn(0.25, k=9, rings=2)
    nrm, flags, samples, compared = check_normals(g, h, t, 6, None, "checkerboard")
    assert np.bincount(samples, minlength=10).tolist() == [0, 0, 0, 0, 4, 0, 24, 0, 0, 36]
    assert np.array_equal(flags == 0, samples >= 6) and (flags[samples < 6] == 1).all()
    assert nrm.stats.cpu().tolist() == [60, 4, 0, 0] and compared[:2] == (60, 60)
    n, cv = nrm.normals.cpu().numpy()[flags == 0], nrm.curvature.cpu().numpy()[flags == 0]
    assert np.abs(n - np.array([0, 0, 1], F)).max() <= 1e-6 and (cv == 0).all()
