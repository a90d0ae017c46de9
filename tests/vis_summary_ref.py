"""fp64 NumPy restatement of `tbn_clip_summary`, the error bounds derived from fp32 rounding, and the list of cases the
operator test and scripts/vis_info_profile.py both run (the script records the largest observed error / bound ratios).

Probabilities, per row, relative error at most (2 (max - min) + 32) 2^-24: the subtraction v - max rounds by
|v - max| 2^-24 in the exponent (numerator and, weighted, normaliser); expf within 3 ulp twice and the division within
1 ulp (the OpenCL bounds); the ordered sum a dozen additions in sequence.
Entropy, absolute error at most 2^-20 (1 + S), S = the rows' mean of sum_t |w log(w + 1e-6)|: logf within 3 ulp, the
rounding of w + 1e-6f, the product, the ordered sum."""
import numpy as np

EPS32 = np.float64(np.float32(1e-6))
B_SIZES = (1, 3, 4, 5, 9)
CLASSES = (1, 5, 63, 64, 65, 125, 352, 1000)
K_SIZES = (1, 5, 8)
SEGMENTS = (1, 2, 3, 25)
T_SIZES = (1, 8, 13, 25, 64, 65, 130)


def ref_topk(scores, k):
    """(B, C) fp32 -> idx (B, k) int32 with -1 padding, prob (B, k) fp64, bound (B,) relative"""
    B, C = scores.shape
    idx = -np.ones((B, k), dtype=np.int32)
    prob = np.full((B, k), np.nan)
    bound = np.zeros(B)
    for b in range(B):
        v = scores[b].astype(np.float64)
        ok = np.flatnonzero(~np.isnan(v))
        order = ok[np.lexsort((ok, -v[ok]))][:k]          # score descending, class index ascending
        idx[b, :len(order)] = order
        finite = v[np.isfinite(v)]
        if np.isnan(v).any() or np.isposinf(v).any() or finite.size == 0:
            continue                                       # NaN throughout, as torch.softmax
        with np.errstate(under="ignore"):
            e = np.exp(v - finite.max())                   # exp(-inf) = 0
        prob[b, :len(order)] = e[order] / e.sum()
        bound[b] = (2.0 * (finite.max() - finite.min()) + 32.0) * 2.0 ** -24
    return idx, prob, bound


def ref_entropy(weights, segments):
    """(B * segments, T) fp32 -> entropy (B,) fp64, bound (B,) absolute"""
    w = weights.astype(np.float64)
    terms = w * np.log(w + EPS32)
    ent = (-terms.sum(1)).reshape(-1, segments).mean(1)
    S = np.abs(terms).sum(1).reshape(-1, segments).mean(1)
    return ent, 2.0 ** -20 * (1.0 + S)


def pitched(a, extra):
    """(rows, cols) -> the same values as a view of a (rows, cols + extra) array filled with NaN beyond the columns"""
    buf = np.full((a.shape[0], a.shape[1] + extra), np.nan, dtype=np.float32)
    buf[:, :a.shape[1]] = a
    return buf


def score_rows(rng, B, C, special=True):
    """seeded randn * 4 rows; with `special`, rows of the batch in turn carry exact ties, all-equal scores, NaN entries
    (one row with a single rankable class), -inf entries, a +inf entry"""
    s = (rng.randn(B, C) * 4).astype(np.float32)
    if not special:
        return s
    for b in range(B):
        kind = b % 6
        if kind == 1:
            s[b] = rng.randint(0, 3, C).astype(np.float32)             # exact ties: the lower index first
        elif kind == 2:
            s[b] = np.float32(1.25)                                     # all equal
        elif kind == 3 and C > 1:
            s[b, rng.rand(C) < 0.4] = np.nan
            s[b, C // 2] = np.nan
            s[b, 0] = np.float32(0.25)                                  # at least one class ranks
        elif kind == 4 and C > 1:
            s[b, rng.rand(C) < 0.3] = -np.inf
            s[b, 0] = -np.inf
        elif kind == 5 and C > 1:
            s[b, C - 1] = np.inf
    if B >= 9 and C > 1:
        s[8] = np.nan
        s[8, C - 1] = 0.5                                               # one rankable class: -1 from the second slot on
    return s


def weight_rows(rng, R, T):
    """softmax rows; in turn a one-hot row (Gumbel `hard`), a row with exact zeros, a uniform row"""
    z = rng.randn(R, T) * 2
    w = np.exp(z - z.max(1, keepdims=True))
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    for r in range(R):
        kind = r % 4
        if kind == 1:
            w[r] = 0
            w[r, rng.randint(T)] = 1
        elif kind == 2:
            w[r, rng.rand(T) < 0.5] = 0
        elif kind == 3:
            w[r] = np.float32(1.0 / T)
    return w


def cases():
    """dicts of: heads (list of (C, extra pitch)), B, k, and segments / T / weight pitch or None"""
    out, n = [], 0
    for C in CLASSES:                                   # one head, every width, k in {1, 5, 8} and k == classes
        ks = sorted({min(k, C) for k in K_SIZES} | ({C} if C <= 8 else set()))
        for k in ks:
            out.append(dict(heads=[(C, 3 * (n % 2))], B=B_SIZES[n % 5], k=k, weights=None))
            n += 1
    out.append(dict(heads=[(125, 0), (352, 4)], B=9, k=5, weights=(3, 8, 0)))          # the model's two heads
    out.append(dict(heads=[(125, 0), (352, 0)], B=4, k=1, weights=(2, 8, 0)))
    out.append(dict(heads=[(8, 0), (64, 1), (65, 0), (1000, 24)], B=5, k=8, weights=None))     # four heads, k == classes
    out.append(dict(heads=[(5, 2), (63, 0), (125, 0), (352, 0)], B=3, k=5, weights=(1, 25, 7)))
    for segments in SEGMENTS:
        for T in T_SIZES:
            out.append(dict(heads=[(5, 0)], B=B_SIZES[n % 5], k=1, weights=(segments, T, 5 * (n % 2))))
            n += 1
    return out


def make_case(case, seed):
    """-> (list of pitched score buffers, pitched weight buffer or None), NumPy fp32"""
    rng = np.random.RandomState(seed)
    scores = [pitched(score_rows(rng, case["B"], C), extra) for C, extra in case["heads"]]
    weights = None
    if case["weights"] is not None:
        segments, T, extra = case["weights"]
        weights = pitched(weight_rows(rng, case["B"] * segments, T), extra)
    return scores, weights


def run_case(case, seed, device):
    """runs the operator on the case -> (idx, prob, ent as NumPy; the score views and weight view as NumPy)"""
    import torch
    from attention_based_tbn_amd import ops
    scores, weights = make_case(case, seed)
    views = {}
    for h, ((C, _), buf) in enumerate(zip(case["heads"], scores)):
        views["h%d" % h] = torch.from_numpy(buf).to(device)[:, :C]
    w, segments = None, 1
    if weights is not None:
        segments, T, _ = case["weights"]
        w = torch.from_numpy(weights).to(device)[:, :T]
    idx, prob, ent = ops.clip_summary(views, case["k"], w, segments)
    return (idx.cpu().numpy(), prob.cpu().numpy(), None if ent is None else ent.cpu().numpy(),
            [buf[:, :C] for (C, _), buf in zip(case["heads"], scores)],
            None if weights is None else weights[:, :case["weights"][1]])


def check_case(case, got):
    """asserts the exact parts, -> (largest probability error / bound, largest entropy error / bound) of the case"""
    idx, prob, ent, scores, weights = got
    p_ratio, e_ratio = 0.0, 0.0
    for h, s in enumerate(scores):
        want_idx, want_prob, bound = ref_topk(s, case["k"])
        assert np.array_equal(idx[:, h], want_idx), (case, h, idx[:, h], want_idx)
        nan = np.isnan(want_prob)
        assert np.array_equal(np.isnan(prob[:, h]), nan), (case, h, prob[:, h], want_prob)
        zero = (want_prob == 0) & ~nan
        assert np.all(prob[:, h][zero] == 0), (case, h)
        live = ~nan & ~zero
        if live.any():
            rel = np.abs(prob[:, h].astype(np.float64) - want_prob) / np.where(live, want_prob, 1.0)
            ratio = rel / np.maximum(bound, 1e-300)[:, None]
            p_ratio = max(p_ratio, float(ratio[live].max()))
    if weights is not None:
        want, bound = ref_entropy(weights, case["weights"][0])
        e_ratio = float((np.abs(ent.astype(np.float64) - want) / bound).max())
    else:
        assert ent is None
    return p_ratio, e_ratio
