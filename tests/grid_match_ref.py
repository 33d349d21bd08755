"""The rules M1-M10 of include/conv3p_match.h (c3p_grid_match_segments) restated in numpy by brute force: np.unique over
the (p, t) pairs of the units and plain loops over the rows.  What the device writes equals this bit for bit."""
import numpy as np

I32, I64 = np.int32, np.int64
ONE = 1 << 30
OUTPUTS = ("pred_size", "pred_void", "truth_size", "truth_missed", "pair_pred", "pair_truth", "pair_inter", "start", "t_start",
           "t_pair", "best_truth", "best_truth_inter", "best_truth_union", "best_pred", "best_pred_inter", "best_pred_union",
           "pred_match", "truth_match", "pred_iou_q30", "class_stats", "stats")


def units_of(segment, S, inverse, emitted, truth, weight):
    """M1: (p, t) per unit, p already -1 outside [0, S)."""
    M = segment.shape[0]
    if weight == "rows":
        inv = np.asarray(inverse, I64)
        inside = (inv >= 0) & (inv < M)
        p = np.where(inside, segment[np.where(inside, inv, 0)], -1).astype(I64) if M else np.full(inv.shape, -1, I64)
        t = np.asarray(truth, I64)
    else:
        p = np.asarray(segment[:emitted], I64)
        t = np.asarray(truth[:emitted], I64)
    return np.where((p >= 0) & (p < S), p, -1), t


def better(ci, cu, cid, bi, bu, bid):
    """M7: a larger IoU by cross-multiplication in Python ints, the lower id on a tie."""
    if bid < 0:
        return True
    l, r = int(ci) * int(bu), int(bi) * int(cu)
    return l > r or (l == r and cid < bid)


def match_ref(segment, seg_stats0, inverse, emitted, truth, T, weight="rows", pred_class=None, truth_class=None, num_class=1,
              iou=(1, 2), max_pairs=None):
    segment = np.asarray(segment, I32)
    M = segment.shape[0]
    S = min(max(int(seg_stats0), 0), M)
    emitted = min(max(int(emitted), 0), M)
    if max_pairs is None:
        max_pairs = M
    num, den = iou
    p, t = units_of(segment, S, inverse, emitted, truth, weight)
    invalid = (t < -1) | (t >= T)
    known = (t >= 0) & (t < T)
    if truth_class is not None:
        c = np.asarray(truth_class, I64)[np.where(known, t, 0)]
        known &= (c >= 0) & (c < num_class)
    t = np.where(known, t, -1)                                                  # M2
    o = {}
    o["pred_size"] = np.bincount(p[(p >= 0) & (t >= 0)], minlength=M).astype(I32)          # M3
    o["pred_void"] = np.bincount(p[(p >= 0) & (t < 0)], minlength=M).astype(I32)
    o["truth_size"] = np.bincount(t[t >= 0], minlength=T).astype(I32)
    o["truth_missed"] = np.bincount(t[(t >= 0) & (p < 0)], minlength=T).astype(I32)
    both = (p >= 0) & (t >= 0)
    keys, inter = np.unique(p[both] * (1 << 32) + t[both], return_counts=True)            # M4: ascending (p, t)
    P, B = keys.shape[0], int(both.sum())
    over = P > max_pairs                                                        # M5
    n = 0 if over else P
    pp, pt = (keys >> 32).astype(I32)[:n], (keys & 0xffffffff).astype(I32)[:n]
    pi = inter.astype(I32)[:n]
    for name, fill, vals in (("pair_pred", -1, pp), ("pair_truth", -1, pt), ("pair_inter", 0, pi)):
        o[name] = np.full(max_pairs, fill, I32)
        o[name][:n] = vals
    o["start"] = np.zeros(M + 1, I32)
    o["t_start"] = np.zeros(T + 1, I32)
    o["t_pair"] = np.full(max_pairs, -1, I32)
    if not over:
        o["start"][:] = np.searchsorted(pp, np.minimum(np.arange(M + 1), S))
        o["start"][S:] = n
        order = np.lexsort((pp, pt))                                            # ascending (t, p)
        o["t_pair"][:n] = order
        o["t_start"][:] = np.searchsorted(pt[order], np.arange(T + 1))
    for side, count in (("truth", M), ("pred", T)):
        o["best_" + side] = np.full(count, -1, I32)
        o["best_%s_inter" % side] = np.zeros(count, I32)
        o["best_%s_union" % side] = np.zeros(count, I32)
    o["pred_match"] = np.full(M, -1, I32)
    o["truth_match"] = np.full(T, -1, I32)
    o["pred_iou_q30"] = np.zeros(M, I32)
    cs = np.zeros((num_class, 6), I64)
    pc = (lambda s: int(pred_class[s])) if pred_class is not None else (lambda s: 0)
    tc = (lambda k: int(truth_class[k])) if truth_class is not None else (lambda k: 0)
    passes = lambda s, k, i, u: pc(s) == tc(k) and 0 <= pc(s) < num_class and int(i) * den > num * int(u)      # M8
    cover = wcover = 0
    if not over:
        for r in range(n):                                                      # M6, M7: every row against both bests
            s, k, i = int(pp[r]), int(pt[r]), int(pi[r])
            u = int(o["pred_size"][s]) + int(o["truth_size"][k]) - i
            if better(i, u, k, o["best_truth_inter"][s], o["best_truth_union"][s], o["best_truth"][s]):
                o["best_truth"][s], o["best_truth_inter"][s], o["best_truth_union"][s] = k, i, u
            if better(i, u, s, o["best_pred_inter"][k], o["best_pred_union"][k], o["best_pred"][k]):
                o["best_pred"][k], o["best_pred_inter"][k], o["best_pred_union"][k] = s, i, u
        for s in range(S):                                                      # M8, M9
            k = int(o["best_truth"][s])
            if k >= 0 and passes(s, k, o["best_truth_inter"][s], o["best_truth_union"][s]):
                o["pred_match"][s] = k
                o["pred_iou_q30"][s] = (int(o["best_truth_inter"][s]) << 30) // int(o["best_truth_union"][s])
            if 0 <= pc(s) < num_class:
                cs[pc(s), 5] += 1
                if o["pred_match"][s] >= 0:
                    cs[pc(s), 0] += 1
                    cs[pc(s), 3] += int(o["pred_iou_q30"][s])
                elif not o["pred_void"][s] > o["pred_size"][s]:
                    cs[pc(s), 1] += 1
        for k in range(T):
            s = int(o["best_pred"][k])
            if s >= 0 and passes(s, k, o["best_pred_inter"][k], o["best_pred_union"][k]):
                o["truth_match"][k] = s
            if o["truth_size"][k] > 0:
                if s >= 0:
                    q = (int(o["best_pred_inter"][k]) << 30) // int(o["best_pred_union"][k])
                    cover += q
                    wcover += q * int(o["truth_size"][k])
                if 0 <= tc(k) < num_class:
                    cs[tc(k), 4] += 1
                    cs[tc(k), 2] += o["truth_match"][k] < 0
    o["class_stats"] = cs
    st = np.zeros(16, I64)                                                      # M10
    st[:8] = (-1 if over else P, B, S, int((o["truth_size"] > 0).sum()), int((t < 0).sum()), int(invalid.sum()),
              int(((p < 0) & (t >= 0)).sum()), int(over))
    st[8:11] = (cover, wcover, int(o["truth_size"].sum(dtype=I64)))
    o["stats"] = st
    return o


def check_theorem(o):
    """M8: a match is unique on both sides, mutual, and the best partner of both -> the number of matches."""
    pm, tm = o["pred_match"], o["truth_match"]
    matched = np.flatnonzero(pm >= 0)
    assert len(set(pm[matched].tolist())) == matched.size                      # no instance taken twice
    for s in matched:
        k = pm[s]
        assert tm[k] == s and o["best_truth"][s] == k and o["best_pred"][k] == s
        assert 2 * int(o["best_truth_inter"][s]) > int(o["best_truth_union"][s])
    assert int((tm >= 0).sum()) == matched.size
    assert int(o["class_stats"][:, 0].sum()) == matched.size or o["stats"][0] < 0
    return matched.size


def summary_ref(o):
    """SegmentMatch.summary()'s formulas, written out once more."""
    one = float(ONE)
    res = {k: [] for k in ("pq", "sq", "rq", "precision", "recall", "tp", "fp", "fn")}
    for tp, fp, fn, siou, _a, _b in o["class_stats"].tolist():
        res["tp"].append(tp)
        res["fp"].append(fp)
        res["fn"].append(fn)
        d = 2 * tp + fp + fn
        res["sq"].append((siou / one) / tp if tp else None)
        res["rq"].append(2 * tp / d if d else None)
        res["pq"].append(2 * (siou / one) / d if d else None)
        res["precision"].append(tp / (tp + fp) if tp + fp else None)
        res["recall"].append(tp / (tp + fn) if tp + fn else None)
    for k in ("pq", "sq", "rq", "precision", "recall"):
        have = [x for x in res[k] if x is not None]
        res["mean_" + k] = sum(have) / len(have) if have else None
    st = o["stats"].tolist()
    res["mcov"] = (st[8] / one) / st[3] if st[3] else None
    res["mwcov"] = (st[9] / one) / st[10] if st[10] else None
    return res
