"""Checker of the window step with feature_user / feature_item side tables (svdf_wunit.cpp / svdf_k_wunit.hip), built on
tests/shared_user_sim.py and the pinned C port of the reference, one window at a time.  The port loads the same table files
(set_param("feature_user" / "feature_item", path)) and runs the reference's update_inner on every row, children included:

  * snapshot of the shared state: W_item, i_bias, g_bias and the rows >= B of W_user / u_bias;
  * every row of the window, in file order: the shared parts are set back to the snapshot (private user rows keep their current values),
    the row is the port's update_csr, and new - snapshot of every target the row touches -- its global and item entries, its shared user
    entries, and the children the table files give its user and item entries -- is added, in fp32 and in file order, to that target's
    accumulator (acc = +0 + c_1 + c_2 ...);
  * at the window's end every touched target becomes snapshot + acc.

With tables that give no children this is shared_user_sim.window_step, which tests/test_side_table_checker.py pins bit for bit."""
import numpy as np

from shared_user_sim import SHARED, make_oracle, window_cuts   # noqa: F401  (make_oracle: the port the checker drives)
from svdfeature_amd import CSRData


def read_table(path):
    """a feature_user / feature_item text table (apex-utils/apex_utils.h:172-195, ``n idx:val ...`` per id) -> per id a list of
    (child id, value)"""
    with open(path) as f:
        tok = f.read().split()
    rows, p = [], 0
    while p < len(tok):
        n = int(tok[p])
        rows.append([(int(t.split(":")[0]), float(np.float32(t.split(":")[1]))) for t in tok[p + 1:p + 1 + n]])
        p += 1 + n
    return rows


def write_table(path, rows):
    with open(path, "w") as f:
        for row in rows:
            f.write(("%d %s" % (len(row), " ".join("%d:%.9g" % (c, v) for c, v in row))).strip() + "\n")
    return path


def random_table(rng, num_rows, lo, hi, max_children=2, p_none=0.2, vals=(1.0, 0.5, 0.25, 2.0, 0.75), hot=(), hot_p=0.0):
    """per id 0 .. max_children distinct children drawn from [lo, hi) (a feature_user table for amd:shared_user_from = B: lo = B); `hot`
    children are drawn with probability hot_p per id (many slots per window), the rest uniformly (rare ones: applied in place)"""
    rows = []
    for _ in range(num_rows):
        n = 0 if rng.random() < p_none else int(rng.integers(1, max_children + 1))
        n = min(n, hi - lo)
        ch = []
        if n and hot and rng.random() < hot_p:
            ch.append(int(rng.choice(hot)))
        while len(ch) < n:
            x = int(rng.integers(lo, hi))
            if x not in ch:
                ch.append(x)
        rows.append([(c, float(rng.choice(vals))) for c in ch])
    return rows


def children(table, ids):
    out = []
    for x in ids:
        if x < len(table):
            out += [c for c, _ in table[x]]
    return out


def row_targets(idx, ng, nu, B, fu, fi):
    """(shared user rows, item rows) one row touches: its shared user entries and item entries, then the children the tables give"""
    uids = [int(x) for x in idx[ng:ng + nu]]
    iids = [int(x) for x in idx[ng + nu:]]
    return [u for u in uids if u >= B] + children(fu, uids), iids + children(fi, iids)


def reaches_twice(d, r, B, fu, fi):
    _, ng, nu, _, idx, _ = d.row(r)
    us, its = row_targets(idx, ng, nu, B, fu, fi)
    return len(set(us)) != len(us) or len(set(its)) != len(its)


def drop_rows_reaching_twice(d, B, fu, fi):
    """the window step refuses a row that touches one target twice after expansion: keep the others"""
    keep = np.array([not reaches_twice(d, r, B, fu, fi) for r in range(d.num_row)], bool)
    return d.select_rows(keep)


def _views(o):
    return {name: o.view(name).copy() for name in SHARED}


def window_step(o, d, B, fu=(), fi=(), user_bias=True):
    """one window (CSRData d, rows in file order) on oracle trainer o, which has loaded the tables fu / fi (read_table of its files);
    user ids >= B are shared rows"""
    snap = _views(o)
    acc = {name: np.zeros_like(v) for name, v in snap.items()}
    touched = {name: set() for name in SHARED}
    cur = {name: v.copy() for name, v in snap.items()}
    for r in range(d.num_row):
        label, ng, nu, ni, idx, val = d.row(r)
        gids = [int(x) for x in idx[:ng]]
        users, items = row_targets(idx, ng, nu, B, fu, fi)
        cur["W_item"][...] = snap["W_item"]
        cur["i_bias"][...] = snap["i_bias"]
        cur["g_bias"][...] = snap["g_bias"]
        cur["W_user"][B:] = snap["W_user"][B:]
        cur["u_bias"][B:] = snap["u_bias"][B:]
        for name in SHARED:
            o.set_view(name, cur[name])
        o.update_csr(label, ng, nu, ni, idx, val)
        new = _views(o)
        for name, ids in (("g_bias", gids), ("W_item", items), ("i_bias", items), ("W_user", users), ("u_bias", users if user_bias else [])):
            for j in ids:
                c = (new[name][j] - snap[name][j]).astype(np.float32)
                acc[name][j] = (acc[name][j] + c).astype(np.float32)
                touched[name].add(j)
        cur = new
    out = cur
    for name in SHARED:
        lo = B if name in ("W_user", "u_bias") else 0
        out[name][lo:] = snap[name][lo:]
        for j in touched[name]:
            out[name][j] = (snap[name][j] + acc[name][j]).astype(np.float32)
        o.set_view(name, out[name])


def simulate(o, d, B, W, passes, fu=(), fi=(), user_bias=True):
    for _ in range(passes):
        for b0, b1 in window_cuts(d.num_row, W):
            window_step(o, d.slice_rows(b0, b1), B, fu, fi, user_bias)
    return o


def table_rows(rng, n, num_private, num_shared, num_item, num_global=0, max_g=0, max_shared=2, max_items=1, uvals=False, ivals=False,
               positions=("first", "middle", "last"), hot_items=(), hot_p=0.0):
    """rows of (globals, [private user + 0 .. max_shared shared ids num_private + j], 1 .. max_items distinct items); the private entry
    sits first, in the middle or last of the user section, by `positions`.  ivals: item values other than 1 (the item-side forms of the
    children differ from plain entries only then)"""
    rows = []
    for _ in range(n):
        g = sorted(int(x) for x in rng.choice(num_global, size=int(rng.integers(0, max_g + 1)), replace=False)) if num_global and max_g else []
        ns = min(int(rng.integers(0, max_shared + 1)), num_shared)
        sh = [num_private + int(x) for x in rng.choice(num_shared, size=ns, replace=False)] if ns else []
        sh = [(s, float(rng.choice([1.0, 0.5, 2.0])) if uvals else 1.0) for s in sh]
        priv = (int(rng.integers(0, num_private)), float(rng.choice([1.0, 0.5, 1.5])) if uvals else 1.0)
        pos = str(rng.choice(list(positions)))
        at = 0 if pos == "first" else len(sh) if pos == "last" else (len(sh) + 1) // 2
        users = sh[:at] + [priv] + sh[at:]
        nitem = min(int(rng.integers(1, max_items + 1)), num_item)
        if hot_items and rng.random() < hot_p:
            it = [int(rng.choice(hot_items))]
        else:
            it = [int(rng.integers(0, num_item))]
        while len(it) < nitem:
            x = int(rng.integers(0, num_item))
            if x not in it:
                it.append(x)
        items = [(x, float(rng.choice([1.0, 0.5, -0.75, 1.25])) if ivals else 1.0) for x in it]
        rows.append((float(rng.integers(1, 6)), [(x, float(rng.uniform(0.1, 1.0))) for x in g], users, items))
    return CSRData.from_rows(rows)
