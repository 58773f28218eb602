"""`amd:step = minibatch` through the reference's OWN binary: the unmodified trainer CLI (svd_feature.cpp, its config parser, buffer iterators,
loader thread and pairwise-rank generator) linked against integration/apex_svd_amd.cpp + libsvdfeature_amd.so (oracle/_ref/svd_feature_amd), with
the key passed as an extra command-line argument.  The binary drives ISVDTrainer::update() one virtual call at a time; the handle trains every
chunk of staged rows as the window sequence the resident route would build from it (svdf_staged.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from svdfeature_amd import data as D
from test_gpu_dropin_cli import AMD_CLI, _build_bulk, _write_conf

pytestmark = pytest.mark.gpu

need_cli = pytest.mark.skipif(not os.path.exists(AMD_CLI), reason="oracle/_ref CLIs are built in the build container only")
STEP = "amd:step=minibatch"


def _run(cli, d, conf, make_buffer, rounds, extra=()):
    """one CLI run in directory d -> (model bytes of every round, (window chunks, exact chunks) the handle reports when it goes)"""
    d.mkdir()
    make_buffer(str(d / "train.buffer"))
    _write_conf(str(d / "run.conf"), list(conf) + [("buffer_feature", "train.buffer"), ("model_out_folder", "./")])
    p = subprocess.run([cli, "run.conf", "num_round=%d" % rounds, "silent=1"] + list(extra), cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600, env=dict(os.environ, SVDF_VERBOSE="1"))
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text
    m = re.search(r"staged route: (\d+) chunks trained by the window step, (\d+) kept exact", text)
    return [open(str(d / ("%04d.model" % r)), "rb").read() for r in range(rounds + 1)], (int(m.group(1)), int(m.group(2))) if m else (0, 0)


def _rmse(path, fmt, test, blocks=None):
    t = sa.Trainer(fmt, 0)
    t.load_model(path)
    t.init_trainer()
    if fmt == 0:
        return cases.rmse(t.predict_batch(test), test.row_label)
    fb = {int(b.data.feat_index[0]): b for b in blocks}
    tu = test.feat_index[0::2]
    pred = np.concatenate([t.predict_block(D.PlusBlock(fb[int(tu[r])].index_ufeedback, fb[int(tu[r])].value_ufeedback, test.slice_rows(r, r + 1), 0))
                           for r in range(0, test.num_row, 11)])
    return cases.rmse(pred, test.row_label[0::11])


@need_cli
def test_ml100k_basicmf_a_round_is_one_chunk(tmp_path):
    """Test A.  90 570 ratings are fewer than stage_window: a round is one chunk, cut at finish_round -- the NNNN.model files are byte-identical to
    those of the plain-C bulk loop (integration/svdf_train_bulk.c: one resident data set, svdf_train_dataset per round) under the same key, and the
    test RMSE stays within the project's contract (1e-4) of the exact run of the same rounds"""
    base, test = cases.ml100k()
    rounds, make = 5, (lambda p: D.write_csr_buffer(p, base))
    exact, (w0, _) = _run(AMD_CLI, tmp_path / "exact", cases.BASICMF_CONF, make, rounds)
    win, (w1, e1) = _run(AMD_CLI, tmp_path / "win", cases.BASICMF_CONF, make, rounds, [STEP])
    bulk, _ = _run(_build_bulk(tmp_path), tmp_path / "bulk", cases.BASICMF_CONF + [("amd:step", "minibatch")], make, rounds)
    assert (w0, w1, e1) == (0, rounds, 0)
    assert exact[0] == win[0] and all(exact[r] != win[r] for r in range(1, rounds + 1))
    for r in range(rounds + 1):
        assert win[r] == bulk[r], "round %d: the staged chunk and the resident data set trained differently" % r
    rm = [_rmse(str(tmp_path / x / ("%04d.model" % rounds)), 0, test) for x in ("exact", "win")]
    print("ML-100K basicMF, %d rounds: test RMSE exact %.6f, amd:step = minibatch %.6f, dRMSE %+.2e" % (rounds, rm[0], rm[1], rm[1] - rm[0]))
    assert abs(rm[1] - rm[0]) <= 1e-4, rm


def _ml100k_user_blocks(base, feedback, binary=False):
    """one block per ML-100K user in user order: its ratings (binary: liked = rating >= 4) and, with `feedback`, its rated items as the
    implicit-feedback list with value n^-1/2 (demo/implicitFeedback/mkimplicitfeedbackfeature.py)"""
    order = np.argsort(base.feat_index[0::2], kind="stable")
    users, items, labels = base.feat_index[0::2][order], base.feat_index[1::2][order], base.row_label[order]
    if binary:
        labels = (labels >= 4).astype(np.float32)
    cut = np.flatnonzero(np.diff(users)) + 1
    blocks = []
    for us, it, lb in zip(np.split(users, cut), np.split(items, cut), np.split(labels, cut)):
        fb = np.unique(it).astype(np.uint32) if feedback else np.zeros(0, np.uint32)
        blocks.append(D.PlusBlock(fb, np.full(len(fb), 1.0 / np.sqrt(max(len(fb), 1)), np.float32), sa.CSRData.from_triples(us, it, lb), 0))
    return blocks


DEMO_ROUNDS = 40   # demo/pairwiseRank/run.sh, demo/implicitFeedback/run.sh: num_round=40


@need_cli
def test_pairwise_rank_generator_order_takes_the_window_step(tmp_path):
    """Test B.  demo/pairwiseRank in its own configuration (pairwiseRank.conf: k = 64, learning rate 0.005, 40 rounds, input_type = 2) on ML-100K with
    liked = rating >= 4: the generator hands over one block of pairs per user, in its own order; the closed units go through wseq_from_blocks.
    Held-out pair accuracy (ua.test: every liked item of a user against every other test item of the user) within 3e-3 of the exact run of the
    same rounds (benchlib/orders.py's contract)"""
    base, test = cases.ml100k()
    blocks = _ml100k_user_blocks(base, feedback=False, binary=True)
    conf = [(k, v) for k, v in cases.conf_with(cases.BASICMF_CONF, format_type=1, num_ufeedback=1682, wd_ufeedback=0.004, active_type=3, no_user_bias=1,
                                               input_type=2) if k != "base_score"]
    rounds, make = DEMO_ROUNDS, (lambda p: D.write_ugroup_buffer(p, blocks))
    exact, (w0, _) = _run(AMD_CLI, tmp_path / "exact", conf, make, rounds)
    win, (w1, e1) = _run(AMD_CLI, tmp_path / "win", conf, make, rounds, [STEP])
    assert w0 == 0 and w1 == rounds and e1 == 0          # counter evidence: every round's chunk was trained by the window step
    assert exact[0] == win[0] and exact[rounds] != win[rounds]
    tu, ti, liked = test.feat_index[0::2], test.feat_index[1::2], test.row_label >= 4
    hu, hp, hn = [], [], []
    for u in np.unique(tu):
        m = tu == u
        for x in ti[m & liked]:
            for y in ti[m & ~liked]:
                hu.append(u); hp.append(x); hn.append(y)
    hu, hp, hn = (np.array(x, np.uint32) for x in (hu, hp, hn))
    acc = []
    for x in ("exact", "win"):
        t = sa.Trainer(1, 3)
        t.load_model(str(tmp_path / x / ("%04d.model" % rounds)))
        t.init_trainer()
        e = np.zeros(0, np.uint32), np.zeros(0, np.float32)   # scored as blocks without a feedback list, like the training blocks
        sp = t.predict_block(D.PlusBlock(e[0], e[1], sa.CSRData.from_triples(hu, hp, np.ones(len(hu), np.float32)), 0))
        sn = t.predict_block(D.PlusBlock(e[0], e[1], sa.CSRData.from_triples(hu, hn, np.ones(len(hu), np.float32)), 0))
        acc.append(cases.pair_accuracy(sp.astype(np.float64) - sn))
    print("pairwise rank, %d held-out pairs, %d rounds: accuracy exact %.5f, amd:step = minibatch %.5f" % (len(hu), rounds, acc[0], acc[1]))
    assert len(hu) > 5000
    assert abs(acc[1] - acc[0]) <= 3e-3, acc


@need_cli
@pytest.mark.parametrize("shape", ["implicit", "feature_user"])
def test_implicit_feedback_blocks_and_a_feature_user_config(shape, tmp_path):
    """Test C.  ML-100K as implicit-feedback blocks in demo/implicitFeedback's own configuration (implicitFeedback.conf: k = 64, 40 rounds; one block
    per user: its ratings, its rated items as the feedback list) and as plain ratings with a feature_user table (every user a child among 8
    bucket rows, amd:shared_user_from; k = 16, 3 rounds): they run, differ from the exact models, |dRMSE| <= 1e-4 on ua.test.  Measured: implicit
    +5.9e-5, feature_user -2.2e-6.  (Early in training -- k = 16, 3 rounds -- the data-driven window rule is NOT inside 1e-4 on the blocks of this
    943-user file: +9.2e-4 here, +7.7e-4 on the resident route, profiles/r04_wstep_demo_shape_calibration.txt; such a file wants amd:window.)"""
    base, test = cases.ml100k()
    rounds, blocks = 3, None
    if shape == "implicit":   # the demo's own configuration: on this 943-user file the step is calibrated there (profiles/r04_wstep_demo_shape_calibration.txt)
        blocks = _ml100k_user_blocks(base, feedback=True)
        conf = cases.conf_with(cases.BASICMF_CONF, format_type=1, num_ufeedback=1682, wd_ufeedback=0.004)
        make, fmt, extra, rounds = (lambda p: D.write_ugroup_buffer(p, blocks)), 1, [STEP], DEMO_ROUNDS
    else:
        with open(str(tmp_path / "fu.txt"), "w") as f:
            for u in range(943):
                f.write("1 %d:0.5\n" % (943 + u % 8))
        conf = cases.conf_with(cases.BASICMF_CONF, num_user=943 + 8, num_factor=16) + [("feature_user", str(tmp_path / "fu.txt"))]
        make, fmt, extra = (lambda p: D.write_csr_buffer(p, base)), 0, [STEP, "amd:shared_user_from=943"]
    exact, (w0, _) = _run(AMD_CLI, tmp_path / "exact", conf, make, rounds)
    win, (w1, e1) = _run(AMD_CLI, tmp_path / "win", conf, make, rounds, extra)
    assert w0 == 0 and w1 == rounds and e1 == 0
    assert exact[0] == win[0] and exact[rounds] != win[rounds]
    rm = []
    for x in ("exact", "win"):
        if fmt == 0:   # the model is scored by a handle that has the table loaded
            t = sa.Trainer(0, 0)
            t.set_param("feature_user", str(tmp_path / "fu.txt"))
            t.load_model(str(tmp_path / x / ("%04d.model" % rounds)))
            t.init_trainer()
            rm.append(cases.rmse(t.predict_batch(test), test.row_label))
        else:
            rm.append(_rmse(str(tmp_path / x / ("%04d.model" % rounds)), 1, test, blocks))
    print("%s, %d rounds: test RMSE exact %.6f, amd:step = minibatch %.6f, dRMSE %+.2e" % (shape, rounds, rm[0], rm[1], rm[1] - rm[0]))
    assert abs(rm[1] - rm[0]) <= 1e-4, rm
