"""numpy restatement of kemr_list_fuse (include/kemr.h) for the tests of the knowledge-fused rerank: np.float32 multiply, np.float32
adds in list order, the project's order rule by np.lexsort.  Not a test module; no GPU, no library."""
import numpy as np


def list_order(scores, ids):
    """Slots of one list in the project's order: id >= 0 only, score descending (-0.0 ties +0.0, NaN behind -inf), then lower id."""
    ok = np.flatnonzero(ids >= 0)
    s = np.asarray(scores, np.float32)[ok]
    nan = np.isnan(s)
    key = np.where(nan, 0.0, -np.where(s == 0, np.float32(0), s).astype(np.float64))
    return ok[np.lexsort((ids[ok], key, nan))]


def sorted_rows(scores, ids, k):
    """kemr_select_topk on explicit ids: the first k of every row's order, padded with -inf / -1."""
    out_s = np.full((ids.shape[0], k), -np.inf, np.float32)
    out_i = np.full((ids.shape[0], k), -1, np.int32)
    for r in range(ids.shape[0]):
        o = list_order(scores[r], ids[r])[:k]
        out_s[r, :len(o)], out_i[r, :len(o)] = scores[r][o], ids[r][o]
    return out_s, out_i


def list_fuse(scores, ids, depth=None, scale=1.0, bonus=None, gt=None, out=None):
    """-> (fused fp32 [nq, ld], ahead int32 [nq] | None, found int32 [nq] | None, gt_score fp32 [nq] | None).  Columns >= depth are
    those of ``out`` (default: -inf)."""
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids, np.int32)
    nq, ld = scores.shape
    depth = ld if depth is None else depth
    fused = np.full((nq, ld), -np.inf, np.float32) if out is None else np.array(out, np.float32)
    scale = np.float32(scale)
    for q in range(nq):
        row = {}
        if bonus is not None:
            ptr, col, val = bonus
            for e in range(int(ptr[q]), int(ptr[q + 1])):
                row.setdefault(int(col[e]), []).append(np.float32(val[e]))
        for j in range(depth):
            c = int(ids[q, j])
            if c < 0:
                fused[q, j] = -np.inf
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                f = np.float32(scale * scores[q, j])
                for v in row.get(c, ()):
                    f = np.float32(f + v)
            fused[q, j] = f
    if gt is None:
        return fused, None, None, None
    ahead, found, gt_score = np.zeros(nq, np.int32), np.zeros(nq, np.int32), np.full(nq, -np.inf, np.float32)
    for q in range(nq):
        order = list_order(fused[q, :depth], ids[q, :depth])
        at = np.flatnonzero(ids[q, :depth][order] == gt[q]) if gt[q] >= 0 else np.zeros(0, np.int64)
        if len(at):
            ahead[q], found[q], gt_score[q] = at[0], 1, fused[q, order[at[0]]]
        else:
            ahead[q] = len(order)
    return fused, ahead, found, gt_score


def dense_bonus(bonus, nq, m):
    """The CSR as the fp32 adds it stands for, per (query, candidate) in list order: a list of value lists."""
    ptr, col, val = bonus
    rows = [dict() for _ in range(nq)]
    for q in range(nq):
        for e in range(int(ptr[q]), int(ptr[q + 1])):
            if 0 <= int(col[e]) < m:
                rows[q].setdefault(int(col[e]), []).append(np.float32(val[e]))
    return rows


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)
