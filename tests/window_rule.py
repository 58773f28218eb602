"""(not collected by pytest) The window rule of `amd:step = minibatch`, restated: into how many windows a pass is cut (svdf_wseq_rule.h; DESIGN.md
sections 6, 6k, 6m, 6r).  The only Python statement of it -- tests/test_window_rule.py holds it equal to the engine's own functions on the CPU,
through the probes svdf_window_rule / svdf_window_rule_as_cut / svdf_window_block_cuts, and the GPU tests compare `num_batches` with it.

Counts are per pass: c_i = how often the pass updates row i.  The sums run in the order and the arithmetic of the C++ (plain doubles, one id
after the other), so that the two agree to the last window and not only away from a knife edge."""
import math

import numpy as np

PER, PER_MAX, PER_FB, PER_SHARED, PER_CHILD = 24, 128, 16, 12, 3   # window_per_target, _max, _fb, _shared, _child (include/svdfeature_amd.h)
SLACK, ROUNDS = 1.5, 40                                            # svdf_wseq_rule.h: kWseqSlack, kWseqRounds
NO_LANE = (0, 0)                                                   # a lane of ordered sub-steps is (sub, cap); sub 0: the side has none
TAG_START, TAG_MIDDLE = 1, 3


def _counts(c):
    return [int(x) for x in np.asarray(c).ravel()]


def met(counts, per_over_per_max=PER / PER_MAX):
    """mean_updates_met: the updates of its own row an entry meets per pass, sum c^2 / sum c, and -- on the mean's scale -- the most updates
    of one row"""
    s1 = s2 = 0.0
    mx = 0
    for c in _counts(counts):
        s1 += float(c)
        s2 += float(c) * float(c)
        mx = max(mx, c)
    return max(s2 / s1 if s1 > 0.0 else 0.0, float(mx) * per_over_per_max)


def class_term(counts, per, per_target=PER, per_target_max=PER_MAX):
    """wseq_class_term: a class of rows with a per-target mean of its own under the common cap, on the item term's scale"""
    counts = _counts(counts)
    return met(counts, per / per_target_max) * per_target / per if counts else 0.0


def windows(n, terms, per_target=PER, per_target_fb=PER_FB, window=0):
    """wseq_windows: the common term -- terms = (item rows, global biases[, feedback mass[, ...]]); amd:window overrides"""
    if n <= 0:
        return 1
    if window > 0:
        return max(1, (n + window - 1) // window)
    worst = 0.0
    for j, t in enumerate(terms):
        worst = max(worst, t / float(per_target_fb if j == 2 else per_target))
    return max(1, int(math.ceil(worst)))


def search(n, plain, child, sub, cap, per_plain, per_child):
    """wseq_windows_shared: the fewest windows W >= ceil(max c / cap) at which, per class, the mean over entries of min(c / W, sub) stays at the
    class value -- lower bound, doubling, bisection, as the C++ searches"""
    if n <= 0:
        return 1
    plain, child = _counts(plain), _counts(child)

    def mean(cnt, W):
        s = s1 = 0.0
        for c in cnt:
            s += min(float(c) / float(W), float(sub)) * float(c)
            s1 += float(c)
        return s / s1 if s1 > 0.0 else 0.0

    def ok(W):
        return mean(plain, W) <= per_plain and mean(child, W) <= per_child
    lo = max(1, (max(plain + child + [0]) + cap - 1) // cap)
    if ok(lo):
        return lo
    hi = lo
    while not ok(hi) and hi < n:
        hi *= 2
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        if ok(mid):
            hi = mid
        else:
            lo = mid
    return hi


def columns(n, item_count, lane=NO_LANE, per_target=PER, per_target_max=PER_MAX, window=0):
    """wseq_rule_columns: ratings and rank pairs (both items of a pair counted); lane = (window_hot_sub, window_hot_max) or the pair knobs"""
    if lane[0] > 0 and n > 0 and window == 0:
        return search(n, item_count, [], lane[0], lane[1], per_target, 0)
    return windows(n, [met(item_count, per_target / per_target_max)], per_target, window=window)


def csr(n, item_count, global_count, shared_count=(), item_child=None, shared_child=None, shared_lane=NO_LANE, item_lane=NO_LANE, per_target=PER,
        per_target_max=PER_MAX, per_target_shared=PER_SHARED, per_target_child=PER_CHILD, window=0):
    """wseq_rule_csr: rows with item, global and shared user entries; *_child mark the rows that are a side-table child somewhere -- a class of
    its own with all its updates.  Without a lane the children of both sides are one class; with one they follow their side."""
    ci, cg, cs = _counts(item_count), _counts(global_count), _counts(shared_count)
    cc, ccu = [], []
    for i, m in enumerate(_counts(item_child) if item_child is not None else []):
        if m:
            cc.append(ci[i])
            ci[i] = 0
    for j, m in enumerate(_counts(shared_child) if shared_child is not None else []):
        if m:
            cc.append(cs[j])
            ccu.append(cs[j])
            cs[j] = 0
    ratio = per_target / per_target_max
    term = lambda cnt, per: class_term(cnt, per, per_target, per_target_max)   # noqa: E731
    shared_met, child_met = term(cs, per_target_shared), term(cc, per_target_child)
    if shared_lane[0] == 0 and item_lane[0] == 0:
        return windows(n, [max(met(ci, ratio), shared_met, child_met), met(cg, ratio)], per_target, window=window)
    cc = cc[:len(cc) - len(ccu)]
    item_term = 0.0 if item_lane[0] > 0 else max(met(ci, ratio), term(cc, per_target_child))
    user_term = 0.0 if shared_lane[0] > 0 else max(shared_met, child_met if ccu else 0.0)
    W = windows(n, [max(item_term, user_term), met(cg, ratio)], per_target, window=window)
    if window == 0 and shared_lane[0] > 0:
        W = max(W, search(n, cs, ccu, shared_lane[0], shared_lane[1], per_target_shared, per_target_child))
    if window == 0 and item_lane[0] > 0:
        W = max(W, search(n, ci, cc, item_lane[0], item_lane[1], per_target, per_target_child))
    return W


def blocks(n, num_block, item_count, global_count=(), shared_count=(), fb_mass=(), shared_lane=NO_LANE, item_lane=NO_LANE, per_target=PER,
           per_target_max=PER_MAX, per_target_fb=PER_FB, per_target_shared=PER_SHARED, window=0):
    """wseq_rule_blocks: user-group blocks; fb_mass = per feedback row, the instance-sized updates a pass pushes into it; capped by the blocks"""
    ratio = per_target / per_target_max
    m1 = m2 = 0.0
    for m in np.asarray(fb_mass, np.float64).ravel().tolist():
        m1 += m
        m2 += m * m
    terms = [0.0 if item_lane[0] > 0 else met(item_count, ratio), met(global_count, ratio), m2 / m1 if m1 > 0.0 else 0.0,
             0.0 if shared_lane[0] > 0 else class_term(shared_count, per_target_shared, per_target, per_target_max)]
    W = windows(n, terms, per_target, per_target_fb, window)
    if shared_lane[0] > 0 and window == 0:
        W = max(W, search(n, shared_count, [], shared_lane[0], shared_lane[1], per_target_shared, 0))
    if item_lane[0] > 0 and window == 0:
        W = max(W, search(n, item_count, [], item_lane[0], item_lane[1], per_target, 0))
    return min(max(num_block, 1), W)


def block_cuts(extend_tag, W):
    """wseq_block_cuts: even block positions, each moved forward to the next position where no START .. END span is open"""
    nb = len(extend_tag)
    cut = [0]
    for w in range(1, W):
        pos = max(nb * w // W, cut[-1])
        while 0 < pos < nb and int(extend_tag[pos - 1]) in (TAG_START, TAG_MIDDLE):
            pos += 1
        cut.append(pos)
    return cut + [nb]


# ---- the rule on the windows as cut

def window_cuts(n, W):
    """the windows of a sequence: equal positions [n w / W, n (w + 1) / W)"""
    return [(n * w // W, n * (w + 1) // W) for w in range(W)]


def window_counts(ids, num_id, W):
    """(worst count of one id in one window, for every entry the count of its id in its window) -- ids: one array, or several columns of one
    class (rank pairs: both items) with one entry per row each"""
    cols = [np.asarray(c, np.int64) for c in (ids if isinstance(ids, (list, tuple)) else [ids])]
    n = len(cols[0])
    worst, per_entry = 0, []
    for b0, b1 in window_cuts(n, W):
        c = np.bincount(np.concatenate([col[b0:b1] for col in cols]), minlength=num_id)
        worst = max(worst, int(c.max()) if b1 > b0 else 0)
        for col in cols:
            per_entry.append(c[col[b0:b1]])
    return worst, np.concatenate(per_entry) if per_entry else np.zeros(0, np.int64)


def mean_met(per_entry, sub):
    """the mean over entries of min(count of the entry's row in its window, sub); sub = 0: of the count"""
    c = np.asarray(per_entry, np.float64)
    return float((np.minimum(c, sub) if sub > 0 else c).mean()) if c.size else 0.0


def as_cut(W, cols, num_id, sub=0, cap=PER_MAX, per=PER, slack=SLACK, rounds=ROUNDS):
    """wseq_windows_actual for one class over id columns: more windows at equal positions until the mean over entries of min(count of the
    entry's row in its window, sub) is within per * slack and the worst count within cap * slack"""
    n = len(cols[0])
    if n <= 0:
        return W
    for _ in range(rounds):
        worst, per_entry = window_counts(list(cols), num_id, W)
        num, den = max([(mean_met(per_entry, sub), per * slack), (float(worst), cap * slack)], key=lambda f: f[0] / f[1])
        if num <= den:
            return W
        W = max(W + 1, int(math.ceil(W * num / den)))
        if W >= n:
            return n
    return n
