"""Regenerates tests/golden/rank_eval.npz: the sums of the reference's own EvaluatorMAP (apex-utils/apex_evaluator.h) over position lists.

A small driver of this project's text is written to a temporary directory, compiled against the reference header where it lies, fed the
position lists of every case below and its output recorded: the line print_result writes (the %f text) and the raw sums as hex floats.
Nothing of the reference and nothing compiled is kept.  The driver is built a second time against a temporary copy of the header whose
`std::vector<float> sum_ar` is a vector of double; generation fails unless that changes at least one recorded sum -- otherwise the float
rounding of the running sum that MAP@k reads (:138-150) would not be tested.

    python tests/golden/make_rank_eval_golden.py [reference root, default /root/reference]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rank_eval.npz")

DRIVER = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>
#define private public   /* the raw sums are private members */
#include "apex_evaluator.h"
#undef private
int main(int argc, char **argv) {
    FILE *fi = fopen(argv[1], "r");
    if (!fi) return 2;
    int nat, S;
    if (fscanf(fi, "%d", &nat) != 1) return 3;
    apex_utils::EvaluatorMAP ev;
    for (int i = 0; i < nat; i++) {
        int k;
        if (fscanf(fi, "%d", &k) != 1) return 3;
        ev.add_map_at(k); ev.add_precision_at(k); ev.add_recall_at(k);
    }
    ev.init();
    if (fscanf(fi, "%d", &S) != 1) return 3;
    for (int s = 0; s < S; s++) {
        int n;
        if (fscanf(fi, "%d", &n) != 1) return 3;
        std::vector<int> pos((size_t)n);
        for (int j = 0; j < n; j++) if (fscanf(fi, "%d", &pos[(size_t)j]) != 1) return 3;
        ev.add_eval(pos, false);
    }
    fclose(fi);
    ev.print_result(stdout, true);
    printf("%ld %a", ev.num_instance(), ev.sum_mapall);
    for (size_t i = 0; i < ev.sum_map.size(); i++) printf(" %a", ev.sum_map[i]);
    for (size_t i = 0; i < ev.sum_pre.size(); i++) printf(" %a", ev.sum_pre[i]);
    for (size_t i = 0; i < ev.sum_rec.size(); i++) printf(" %a", ev.sum_rec[i]);
    printf("\n");
    return 0;
}
"""


def cases():
    """name -> (cut-offs as given, list of position lists, ranked per list).  Positions inside a list are distinct (they are rank positions of
    distinct items) and NOT sorted; position 0 and position ranked - 1 occur; list lengths 1, 2, 17 and 300."""
    rng = np.random.default_rng(24)
    ranked = 517
    lists = [[0], [ranked - 1], [0, ranked - 1], [ranked - 1, 0], [3, 1], list(range(17)), list(range(ranked - 17, ranked))]
    for n, count in ((1, 90), (2, 90), (17, 90), (300, 24)):
        for c in range(count):
            # half of them crowd the head of the list, where the cut-offs bite
            hi = ranked if c % 2 == 0 else min(ranked, max(n, 12 * n))
            lists.append([int(x) for x in rng.permutation(hi)[:n]])
    lists.append(list(range(300)))            # npos == a prefix of the ranking
    lists.append([int(x) for x in rng.permutation(300)])   # every position below 300, ranked == npos for the AUC skip
    rk = [ranked] * len(lists)
    rk[-1] = 300
    out = {"all": ((10, 1, 100, 5), lists, rk)}
    # a running sum that float cannot hold: 300 terms (i + 1) / (pos_i + 1) of different magnitudes
    long_list = [int(x) for x in np.sort(rng.permutation(5000)[:300])]
    out["long"] = ((1, 5, 10, 100, 1000, 4000), [long_list], [5000])
    pairs = [[int(a), int(b)] for a, b in rng.integers(0, 6, size=(40, 2)) if a != b]
    out["pairs"] = ((1, 2, 3), pairs, [6] * len(pairs))
    return out


def run(exe, tmp, at, lists):
    path = os.path.join(tmp, "in.txt")
    with open(path, "w") as f:
        f.write("%d %s\n%d\n" % (len(at), " ".join(str(k) for k in at), len(lists)))
        for p in lists:
            f.write("%d %s\n" % (len(p), " ".join(str(x) for x in p)))
    text, raw = subprocess.check_output([exe, path]).decode().splitlines()
    raw = raw.split()
    return text, int(raw[0]), np.array([float.fromhex(x) for x in raw[1:]], np.float64)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    hdr_dir = os.path.join(ref, "apex-utils")
    assert os.path.exists(os.path.join(hdr_dir, "apex_evaluator.h")), "reference header not found under %s" % ref
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "driver.cpp")
        with open(src, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["g++", "-O1", "-w", "-I", hdr_dir, src, "-o", exe])
        # the same driver against a copy of the header with a double running sum: only to prove the fixture sees the float
        dbl_dir = os.path.join(tmp, "dbl")
        os.makedirs(os.path.join(dbl_dir, "apex-utils"))
        text = open(os.path.join(hdr_dir, "apex_evaluator.h")).read()
        assert "std::vector<float> sum_ar;" in text
        text = text.replace("std::vector<float> sum_ar;", "std::vector<double> sum_ar;").replace('"../apex-tensor/', '"%s/apex-tensor/' % ref)
        text = text.replace('"apex_utils.h"', '"%s/apex_utils.h"' % hdr_dir)
        with open(os.path.join(dbl_dir, "apex-utils", "apex_evaluator.h"), "w") as f:
            f.write(text)
        exe2 = os.path.join(tmp, "driver_dbl")
        subprocess.check_call(["g++", "-O1", "-w", "-I", os.path.join(dbl_dir, "apex-utils"), src, "-o", exe2])
        store, changed = {}, []
        for name, (at, lists, ranked) in cases().items():
            text, ninst, sums = run(exe, tmp, at, lists)
            _, _, sums2 = run(exe2, tmp, at, lists)
            if not np.array_equal(sums, sums2):
                changed.append(name)
            assert ninst == len(lists)
            store[name + "_at"] = np.array(at, np.int32)
            store[name + "_sec_ptr"] = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
            store[name + "_position"] = np.array([x for p in lists for x in p], np.int32)
            store[name + "_ranked"] = np.array(ranked, np.int32)
            store[name + "_text"] = np.array(text)
            store[name + "_ninst"] = np.array(ninst, np.int64)
            store[name + "_sums"] = sums   # sum_mapall | sum_map[at ascending] | sum_pre[..] | sum_rec[..]
            print("%-6s %4d sections  %s" % (name, len(lists), text))
        assert changed, "no case changes when sum_ar is a vector of double: the float rounding is not tested"
        print("cases whose sums change with a double sum_ar:", ", ".join(changed))
        store["cases"] = np.array(sorted(cases()))
        np.savez_compressed(OUT, **store)
        print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
