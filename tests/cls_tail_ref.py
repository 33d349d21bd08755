"""float64 numpy restatement of the classification model's fused tail (the CPU side of test_cls_tail*.py;
pointwise_amd.head.classification_tail is the device side): oracle/head_numpy.py's layers, plus what that file does
not have -- the batch counters of train_modelnet40_acsd.py:136-146 in the layout of conv3p_seg_head_*, the ignored-row
rule (a label outside [0, C): loss 0, gradient row 0, counted under `invalid`) and the Philox4x32-10 dropout draw."""
import numpy as np

from oracle import head_numpy

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) uint32 -> (..., 4) uint32 (Salmon et al., SC'11)."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def keep_mask(seed, step, M, H, rate, rows=None):
    """The device's draw: element e = m H + h takes word e & 3 of the block with counter (e >> 2, 0, step low, step
    high) under key (seed low, seed high); u = (word >> 8) 2^-24; keep = floor(float32(1 - rate) + u) in float32.
    rows: the row indices m (default 0 .. M - 1) -> uint8 (len(rows), H)."""
    rows = np.arange(M) if rows is None else np.asarray(rows)
    e = (rows[:, None].astype(np.int64) * H + np.arange(H)[None, :]).reshape(-1)
    ctr = np.zeros((e.size, 4), dtype=np.uint32)
    ctr[:, 0] = e >> 2
    ctr[:, 2] = step & 0xFFFFFFFF
    ctr[:, 3] = step >> 32
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), (e.size, 2))
    word = philox4x32_10(ctr, key)[np.arange(e.size), e & 3]
    u = (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.floor(np.float32(1.0 - rate) + u).astype(np.uint8).reshape(len(rows), H)


def counters(pred, labels, C):
    """{correct, invalid, seen[C], correct_class[C], predicted[C]} as int64[2 + 3 C]."""
    pred, lab = np.asarray(pred).astype(np.int64), np.asarray(labels).astype(np.int64)
    valid = (lab >= 0) & (lab < C)
    lv, pv = lab[valid], pred[valid]
    return np.concatenate([[int((pv == lv).sum()), int((~valid).sum())], np.bincount(lv, minlength=C),
                           np.bincount(lv[pv == lv], minlength=C), np.bincount(pv, minlength=C)]).astype(np.int64)


def cls_tail_ref(fc1, W2, b2, labels, rate, keep, grad_scale=None):
    """fc1 (M, H), W2 (H, C), b2 (C), labels (M), keep (M, H) 0 / 1 or None (no dropout) -> dict of float64 arrays:
    drop, logits, pred, row_loss, loss_sum, counts, dz, dfc1, dW2, db2.  grad_scale: default 1 / M."""
    fc1, W2, b2 = (np.asarray(a, dtype=np.float64) for a in (fc1, W2, b2))
    lab = np.asarray(labels).astype(np.int64)
    M, C = fc1.shape[0], W2.shape[1]
    scale = 1.0 / M if grad_scale is None else float(grad_scale)
    if keep is None:
        drop, back = fc1, np.ones_like(fc1)
    else:
        keep = np.asarray(keep, dtype=np.float64)
        drop, a = head_numpy.dropout_selu(fc1, rate, keep)
        back = a * keep
    logits = head_numpy.fully_connected(drop, W2, b2)
    valid = (lab >= 0) & (lab < C)
    safe = np.where(valid, lab, 0)
    mx = logits.max(axis=1)
    e = np.exp(logits - mx[:, None])
    s = e.sum(axis=1)
    row_loss = np.where(valid, np.log(s) + mx - logits[np.arange(M), safe], 0.0)
    onehot = np.zeros_like(logits)
    onehot[np.arange(M), safe] = 1.0
    dlogits = np.where(valid[:, None], (e / s[:, None] - onehot) * scale, 0.0)
    dz = dlogits * head_numpy.selu_slope_from_output(logits)
    pred = np.argmax(logits, axis=1)
    return {"drop": drop, "logits": logits, "pred": pred, "row_loss": row_loss, "loss_sum": float(row_loss.sum()),
            "counts": counters(pred, lab, C), "dz": dz, "dfc1": (dz @ W2.T) * back, "dW2": drop.T @ dz,
            "db2": dz.sum(axis=0)}
