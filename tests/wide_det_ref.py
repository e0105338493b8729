"""NumPy mirrors of the summation orders that include/fastegnn_hip.h documents for the ordered wide operators (test infrastructure:
no GPU, no library).  tests/test_gpu_wide_det.py compares the kernels against these bit for bit."""
import numpy as np


def rows_per_slot(M, W):
    """segment_sum_ordered: rps = 16, doubled while rps < 256 and ceil(M / rps) * W > 2^21"""
    rps = 16
    while rps < 256 and -(-M // rps) * W > (1 << 21):
        rps *= 2
    return rps


def segment_sum_ws_bytes(M, W):
    return 0 if M <= 0 else -(-M // rows_per_slot(M, W)) * 2 * W * 4


def segment_sum_ordered(idx_sorted, terms, R, table=None):
    """table[t] = the documented fp32 sum of terms[m] over idx_sorted[m] == t; `terms` [M, W] float32 are the rows in SORTED order
    (already read through the permutation, already activated).  Rows of `table` that no index names are left as passed."""
    idx = np.asarray(idx_sorted)
    terms = np.asarray(terms, dtype=np.float32)
    M, W = terms.shape
    out = np.zeros((R, W), np.float32) if table is None else np.array(table, dtype=np.float32)
    if M == 0:
        return out
    rps = rows_per_slot(M, W)
    pieces = {}   # target -> the run's sums within each slot, ascending slot
    for lo in range(0, M, rps):
        hi = min(lo + rps, M)
        cur, acc = idx[lo], np.zeros(W, np.float32)
        for m in range(lo, hi):
            if idx[m] != cur:
                pieces.setdefault(int(cur), []).append(acc)
                cur, acc = idx[m], np.zeros(W, np.float32)
            acc = acc + terms[m]
        pieces.setdefault(int(cur), []).append(acc)
    for t, ps in pieces.items():
        tot = ps[0]
        for q in ps[1:]:
            tot = tot + q
        out[t] = tot
    return out


def dw_splits(M, O, K):
    """linear_dw_ordered / head_dw_ordered: (rows per range, number of ranges, workspace floats), a function of (M, O, K) alone"""
    if M <= 0:
        return 0, 0, 0
    if O <= 8 or K <= 8:
        ns = max(1, min(-(-M // 512), 512, (4 << 20) // (4 * (O * K + O))))
        rows = -(-M // ns)
        nz = -(-M // rows)
        return rows, nz, nz * (O * K + O)
    blocks = -(-O // 128) * -(-K // 128)
    per = O * K + 2 * O
    ns = max(1, min(-(-512 // blocks), -(-M // 256), (16 << 20) // (4 * per)))
    rows = -(-(-(-M // ns)) // 32) * 32
    nz = -(-M // rows)
    return rows, nz, nz * per
