"""svdfeature_amd -- MI355X-native engine for the apex_svd SGD hot path of Gnnng/SVDFeature.

The product is ``libsvdfeature_amd.so`` (hand-written gfx950 HIP kernels + C++ host engine behind
the C ABI of ``include/svdfeature_amd.h``).  This module is only the ctypes binding the tests and
bench.py use; ``Trainer`` mirrors the reference's ``ISVDTrainer`` surface (apex_svd.h:33-107)
method for method.  There is no CPU fallback: if the shared library is missing or no GPU is
visible, construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

from .data import BlockArrays, CSRData, PlusBlock, pairs_as_csr  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsvdfeature_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "svdfeature_amd.h")

VIEW = {"u_bias": 0, "W_user": 1, "i_bias": 2, "W_item": 3, "g_bias": 4, "ufeedback_bias": 5, "W_ufeedback": 6}

_u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")

_lib = None
_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]


class SvdfError(RuntimeError):
    pass


class RankMetrics(C.Structure):
    """struct svdf_rank_metrics (include/svdfeature_amd.h)"""
    _fields_ = [("ninst", C.c_int64), ("skipped", C.c_int64), ("nan_sections", C.c_int64), ("nauc", C.c_int64), ("num_at", C.c_int), ("at", C.c_int * 8),
                ("sum_map", C.c_double), ("sum_map_at", C.c_double * 8), ("sum_pre_at", C.c_double * 8), ("sum_rec_at", C.c_double * 8), ("sum_auc", C.c_double)]

    def as_dict(self):
        """the raw sums and counts, and the figures EvaluatorMAP::print_result divides out of them (sum / ninst)"""
        n, at = self.ninst, list(self.at[:self.num_at])
        d = {"ninst": n, "skipped": self.skipped, "nan_sections": self.nan_sections, "nauc": self.nauc, "at": at, "sum_map": self.sum_map,
             "sum_map_at": list(self.sum_map_at[:self.num_at]), "sum_pre_at": list(self.sum_pre_at[:self.num_at]),
             "sum_rec_at": list(self.sum_rec_at[:self.num_at]), "sum_auc": self.sum_auc}
        if n:
            d["MAP"] = self.sum_map / n
            for j, k in enumerate(at):
                d["MAP@%d" % k], d["Pre@%d" % k], d["Rec@%d" % k] = self.sum_map_at[j] / n, self.sum_pre_at[j] / n, self.sum_rec_at[j] / n
        if self.nauc:
            d["AUC"] = self.sum_auc / self.nauc   # not in the reference
        return d


def _opt_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class WindowRuleIn(C.Structure):
    """struct svdf_window_rule_in (include/svdfeature_amd.h)"""
    _fields_ = [("per_target", C.c_int), ("per_target_max", C.c_int), ("per_target_fb", C.c_int), ("per_target_shared", C.c_int),
                ("per_target_child", C.c_int), ("window", C.c_long), ("shared_sub", C.c_int), ("shared_cap", C.c_int), ("item_sub", C.c_int),
                ("item_cap", C.c_int), ("n", C.c_long), ("num_block", C.c_long), ("num_item", C.c_long), ("num_global", C.c_long),
                ("num_shared", C.c_long), ("item_count", C.c_void_p), ("global_count", C.c_void_p), ("shared_count", C.c_void_p),
                ("item_child", C.c_void_p), ("shared_child", C.c_void_p), ("num_fb", C.c_long), ("fb_mass", C.c_void_p)]


WINDOW_ROUTES = {"columns": 0, "csr": 1, "blocks": 2}


def window_rule(route, n, item_count, global_count=(), shared_count=(), item_child=None, shared_child=None, fb_mass=(), num_block=0,
                shared_lane=(0, 0), item_lane=(0, 0), per_target=24, per_target_max=128, per_target_fb=16, per_target_shared=12,
                per_target_child=3, window=0):
    """svdf_window_rule: the window count of `amd:step = minibatch` for one route ("columns", "csr", "blocks") from per-pass counts, the
    lanes (sub, cap) and the knob values.  A host function: no GPU, no handle; the data-set builders call the same code."""
    lib = load_library()
    keep = [np.ascontiguousarray(a, np.int64) for a in (item_count, global_count, shared_count)]
    marks = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in (item_child, shared_child)]
    mass = np.ascontiguousarray(fb_mass, np.float64)
    a = WindowRuleIn(per_target, per_target_max, per_target_fb, per_target_shared, per_target_child, int(window), int(shared_lane[0]),
                     int(shared_lane[1]), int(item_lane[0]), int(item_lane[1]), int(n), int(num_block), len(keep[0]), len(keep[1]), len(keep[2]),
                     _opt_ptr(keep[0]), _opt_ptr(keep[1]), _opt_ptr(keep[2]), _opt_ptr(marks[0]), _opt_ptr(marks[1]), len(mass), _opt_ptr(mass))
    W = lib.svdf_window_rule(WINDOW_ROUTES[route], C.byref(a))
    if W < 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return W


def window_rule_as_cut(W, cols, num_id, target, cap, sub=0, slack=1.5, rounds=40):
    """svdf_window_rule_as_cut: W raised until one class of rows (ids < num_id, the id columns `cols` of the file's rows) keeps the rule on
    the windows as cut.  A host function."""
    lib = load_library()
    cols = [np.ascontiguousarray(c, np.uint32) for c in cols]
    ptrs = (C.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    out = lib.svdf_window_rule_as_cut(int(W), len(cols[0]), len(cols), ptrs, int(num_id), float(target), int(cap), int(sub), float(slack), int(rounds))
    if out < 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return out


def window_block_cuts(extend_tag, W):
    """svdf_window_block_cuts: the W + 1 block positions at which a pass of user-group blocks is cut into W windows.  A host function."""
    lib = load_library()
    tag = np.ascontiguousarray(extend_tag, np.int32)
    cut = np.zeros(int(W) + 1, np.int64)
    if lib.svdf_window_block_cuts(len(tag), _pad(tag, np.int32), int(W), cut.ctypes.data_as(C.c_void_p)) != 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return cut


def rank_metrics(sec_ptr, position, ranked=None, nan=None, at=(1, 5, 10, 100)):
    """svdf_rank_eval_metrics: the reference's MAP / MAP@k / Pre@k / Rec@k sums (EvaluatorMAP) over sections of rank positions, plus a
    per-section AUC when `ranked` is given.  A host function: no GPU, no handle.  Returns RankMetrics.as_dict()."""
    lib = load_library()
    sec_ptr = _pad(sec_ptr, np.int64)
    ranked = None if ranked is None else _pad(ranked, np.int32)
    nan = None if nan is None else _pad(nan, np.int32)
    m = RankMetrics()
    if lib.svdf_rank_eval_metrics(len(sec_ptr) - 1, sec_ptr, _pad(position, np.int32), _opt_ptr(ranked), _opt_ptr(nan), len(at), _pad(list(at), np.int32),
                                  C.byref(m)) != 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return m.as_dict()


def rank_negatives(num_item, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, seed):
    """svdf_rank_negatives: the negatives Trainer.rank_positions(..., sampled=(num_neg, seed)) ranks each section's positives against, by the
    published rule (include/svdfeature_amd.h): [S, num_neg] int32 in draw order, a row of -1 for a section without positives.
    A host function: no GPU, no handle.  ban_ptr = None: no bans."""
    lib = load_library()
    S = len(_pad(pos_ptr, np.int64)) - 1
    pos_ptr, pos_item, ban_ptr, ban_item = _sampled_lists(S, pos_ptr, pos_item, ban_ptr, ban_item)
    n = max(int(num_neg), 1)
    neg = np.full((max(S, 1), n), -1, np.int32)
    if lib.svdf_rank_negatives(S, pos_ptr, pos_item, _opt_ptr(ban_ptr), _opt_ptr(ban_item), int(num_item), int(num_neg),
                               int(seed) & 0xFFFFFFFFFFFFFFFF, neg.reshape(-1)) != 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return neg[:S]


def _pair_rows(user, pos_item):
    """the rows of a pair source as the two arrays the library reads n entries of"""
    user, pos_item = np.atleast_1d(user), np.atleast_1d(pos_item)
    if len(user) != len(pos_item):
        raise SvdfError("pair_source: user and pos_item must have one entry per row")
    return len(user), _pad(user, np.uint32), _pad(pos_item, np.uint32)


def _pass_size(n, num_neg):
    """entries of a pass's negative column (the library refuses what is out of range before it writes)"""
    return n * int(num_neg) if 1 <= int(num_neg) <= 256 and n * int(num_neg) < (1 << 31) - 16 else 0


def _item_weights(item_weight, num_item):
    """the weights of a weighted pair source as the uint32 array the library reads num_item entries of (num_item None: not known here)"""
    w = np.atleast_1d(np.asarray(item_weight))
    if w.ndim != 1 or (num_item is not None and len(w) != int(num_item)):
        raise SvdfError("pair_source: item_weight must have one entry per item")
    if w.dtype.kind not in "iu" or (w.size and (int(w.min()) < 0 or int(w.max()) > 0xFFFFFFFF)):
        raise SvdfError("pair_source: item_weight must hold integers in 0 .. 2^32 - 1")
    return _pad(w, np.uint32)


def pair_negatives(num_user, num_item, user, pos_item, num_neg, seed, item_weight=None):
    """svdf_pair_negatives: the negatives Trainer.dataset_from_pair_source(src, num_neg, seed) trains a source of these rows against, by the
    published rule (include/svdfeature_amd.h): uint32[n * num_neg], pair r * num_neg + j belongs to row r.  A host function:
    no GPU, no handle.  item_weight (uint32 per item): the negatives of a source created with these weights (svdf_pair_negatives_weighted,
    DESIGN.md 6ae).  The negatives of a SHUFFLED pass (shuffle=s) are this call on the rows user[sigma], pos_item[sigma] with
    sigma = pair_order(n, s)."""
    lib = load_library()
    n, user, pos_item = _pair_rows(user, pos_item)
    neg = np.zeros(max(_pass_size(n, num_neg), 1), np.uint32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if item_weight is None:
        rc = lib.svdf_pair_negatives(int(num_user), int(num_item), n, user, pos_item, int(num_neg), seed, neg)
    else:
        rc = lib.svdf_pair_negatives_weighted(int(num_user), int(num_item), n, user, pos_item, _item_weights(item_weight, num_item), int(num_neg), seed, neg)
    if rc != 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return neg[:n * int(num_neg)]


def pair_order(n, order_seed):
    """svdf_pair_order: the order of a shuffled pass (Trainer.dataset_from_pair_source(..., shuffle=order_seed)) -- uint32[n],
    position p of the pass holds source row sigma[p]; a permutation of 0 .. n-1 by the published rule (include/svdfeature_amd.h).  A host
    function: no GPU, no handle."""
    lib = load_library()
    n = int(n)
    sigma = np.zeros(n if 1 <= n < (1 << 31) - 16 else 1, np.uint32)
    if lib.svdf_pair_order(n, int(order_seed) & 0xFFFFFFFFFFFFFFFF, sigma) != 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return sigma


def pair_weight_lookup(item_weight, x, form=1, trainer=None):
    """svdf_pair_weight_lookup: the item ids the weighted rule maps the 64-bit words x onto under item_weight, in form 1 (binary
    search of the running sums) or 2 (guide table); on the host, or with trainer= by the same function on that trainer's GPU."""
    lib = load_library()
    w = _item_weights(item_weight, None)
    x = np.ascontiguousarray(x, np.uint64).reshape(-1)
    ids = np.zeros(max(len(x), 1), np.uint32)
    if lib.svdf_pair_weight_lookup(None if trainer is None else trainer.h, len(np.atleast_1d(item_weight)), w, int(form), len(x), _pad(x, np.uint64), ids) != 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return ids[:len(x)]


def pair_popularity_weights(pos_item, num_item, power=0.75, unseen=1):
    """A convenience, NOT part of the pinned rule: uint32 item weights rint(1024 * count^power) for the items among pos_item and `unseen` for
    the rest, computed in numpy float64 (so the last unit of a weight may differ between numpy versions -- keep the array if a run is to be
    repeated).  Raises if the sum reaches 2^32."""
    count = np.bincount(np.asarray(pos_item, np.int64).reshape(-1), minlength=int(num_item)).astype(np.float64)
    if len(count) != int(num_item):
        raise SvdfError("item feature index exceed bound")
    w = np.where(count > 0, np.rint(1024.0 * np.power(count, float(power))), float(int(unseen)))
    if w.min() < 0 or float(w.sum()) >= 4294967296.0:
        raise SvdfError("pair_source: the item weights sum to %d: the sum must stay below 2^32" % int(w.sum()))
    return w.astype(np.uint32)


def _hard_size(n, num_neg, num_cand):
    """entries of a hard pass's negative column (as _pass_size: the library refuses what is out of range before it writes)"""
    ok = 1 <= int(num_cand) <= 256 and 1 <= int(num_neg) <= 256 and int(num_neg) * int(num_cand) <= 256
    return n * int(num_neg) if ok and n * int(num_neg) * int(num_cand) < (1 << 31) - 16 else 0


def _shuffled_cand(hard):
    """num_cand of the _shuffled entry points for hard=C: there 0 selects the plain pass, so a hard=0 is passed on as what the hard pass refuses"""
    return int(hard) if int(hard) != 0 else -1


def pair_hard_negatives(num_user, num_item, user, pos_item, num_neg, num_cand, seed, W_user, W_item, i_bias, return_scores=False, item_weight=None):
    """svdf_pair_hard_negatives: the negatives Trainer.dataset_from_pair_source(src, num_neg, seed, hard=num_cand) trains against on the model
    (W_user [num_user, k], W_item [num_item, k], i_bias [num_item]) -- per pair the best-scoring of num_cand candidates of the plain rule
    (include/svdfeature_amd.h): uint32[n * num_neg], with return_scores also the chosen scores.  A host function: no GPU, no
    handle.  item_weight: the candidates are those of a source created with these weights (svdf_pair_hard_negatives_weighted).
    The negatives of a SHUFFLED hard pass (shuffle=s) are this call on the rows user[sigma], pos_item[sigma] with
    sigma = pair_order(n, s)."""
    lib = load_library()
    n, user, pos_item = _pair_rows(user, pos_item)
    W_user, W_item = np.ascontiguousarray(W_user, np.float32), np.ascontiguousarray(W_item, np.float32)
    i_bias = np.ascontiguousarray(i_bias, np.float32).reshape(-1)
    if W_user.ndim != 2 or W_item.ndim != 2 or W_user.shape != (int(num_user), W_item.shape[1]) or W_item.shape[0] != int(num_item) or len(i_bias) != int(num_item):
        raise SvdfError("pair_source: W_user, W_item and i_bias must be [num_user, k], [num_item, k] and [num_item]")
    size = max(_hard_size(n, num_neg, num_cand), 1)
    neg, score = np.zeros(size, np.uint32), np.zeros(size, np.float32)
    model = (W_item.shape[1], _pad(W_user, np.float32), _pad(W_item, np.float32), _pad(i_bias, np.float32), neg, _opt_ptr(score if return_scores else None))
    if item_weight is None:
        rc = lib.svdf_pair_hard_negatives(int(num_user), int(num_item), n, user, pos_item, int(num_neg), int(num_cand), int(seed) & 0xFFFFFFFFFFFFFFFF, *model)
    else:
        rc = lib.svdf_pair_hard_negatives_weighted(int(num_user), int(num_item), n, user, pos_item, _item_weights(item_weight, num_item), int(num_neg),
                                                   int(num_cand), int(seed) & 0xFFFFFFFFFFFFFFFF, *model)
    if rc != 0:
        raise SvdfError(lib.svdf_last_error().decode())
    N = n * int(num_neg)
    return (neg[:N], score[:N]) if return_scores else neg[:N]


def item_unit_rows(W):
    """svdf_item_unit_rows: the unit rows of the cosine metric of Trainer.similar_items (include/svdfeature_amd.h) for the
    rows W [n, k] -- W[i] / sqrt(<W[i], W[i]>) element by element, the sum of squares in the pinned float32 order, +0 rows where it is 0.
    A host function: no GPU, no handle."""
    lib = load_library()
    W = np.ascontiguousarray(W, np.float32)
    if W.ndim != 2 or W.shape[1] < 1:
        raise SvdfError("item_unit_rows: W must be [n, k] with k >= 1")
    out = np.zeros(max(W.size, 1), np.float32)
    if lib.svdf_item_unit_rows(W.shape[0], W.shape[1], _pad(W, np.float32), out) != 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return out[:W.size].reshape(W.shape)


ITEM_METRICS = {"dot": 0, "cosine": 1}


def _sampled_lists(S, pos_ptr, pos_item, ban_ptr, ban_item):
    """the positives and bans of S sections as the arrays the sampled calls take (ban_ptr = None: two None); the library reads as many ids
    as the pointers say, so arrays shorter than that are refused here"""
    pos_ptr, given = _pad(pos_ptr, np.int64), len(np.atleast_1d(pos_item))
    if len(pos_ptr) != S + 1:
        raise SvdfError("rank_eval: pos_ptr must have one entry more than users")
    if S and int(pos_ptr.max()) > given:
        raise SvdfError("rank_eval: pos_item is shorter than pos_ptr says")
    if ban_ptr is None:
        return pos_ptr, _pad(pos_item, np.uint32), None, None
    ban_ptr, given = _pad(ban_ptr, np.int64), len(np.atleast_1d(ban_item)) if ban_item is not None else 0
    if len(ban_ptr) != S + 1:
        raise SvdfError("rank_eval: ban_ptr must have one entry more than users")
    if S and int(ban_ptr.max()) > given:
        raise SvdfError("rank_eval: ban_item is shorter than ban_ptr says")
    return pos_ptr, _pad(pos_item, np.uint32), ban_ptr, _pad(ban_item if ban_item is not None else [], np.uint32)


def load_library():
    """dlopen libsvdfeature_amd.so and declare every prototype of include/svdfeature_amd.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SvdfError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    # PyTorch-ROCm bundles its own libamdhip64; a process must hold ONE HIP runtime, so when torch is
    # installed it is imported first and libsvdfeature_amd.so binds to the runtime torch loaded
    # (otherwise torch.cuda reports "no GPUs" after /opt/rocm's copy has been initialised).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    P = C.c_void_p
    lib.svdf_version.restype = C.c_char_p
    lib.svdf_last_error.restype = C.c_char_p
    lib.svdf_set_error_mode.argtypes = [C.c_int]
    lib.svdf_device_count.restype = C.c_int
    lib.svdf_create.restype = P
    lib.svdf_create.argtypes = [C.c_uint8] * 4 + [C.c_int]
    lib.svdf_destroy.argtypes = [P]
    lib.svdf_set_param.argtypes = [P, C.c_char_p, C.c_char_p]
    lib.svdf_seed.argtypes = [C.c_uint]
    for f in ("svdf_init_model", "svdf_init_trainer", "svdf_finish_round", "svdf_synchronize",
              "svdf_item_delta_begin", "svdf_item_delta_apply"):
        getattr(lib, f).argtypes = [P]
    lib.svdf_set_round.argtypes = [P, C.c_int]
    lib.svdf_load_model.argtypes = [P, C.c_void_p]
    lib.svdf_save_model.argtypes = [P, C.c_void_p]
    lib.svdf_save_model_begin.argtypes = [P, C.c_void_p]
    lib.svdf_save_model_end.argtypes = [P]
    lib.svdf_update_csr.argtypes = [P, C.c_float, C.c_int, C.c_int, C.c_int, _u32p, _f32p]
    lib.svdf_predict_csr.argtypes = lib.svdf_update_csr.argtypes
    lib.svdf_predict_csr.restype = C.c_float
    lib.svdf_update_csr_batch.argtypes = [P, C.c_int, _f32p, _i32p, _u32p, _f32p]
    lib.svdf_predict_csr_batch.argtypes = [P, C.c_int, _f32p, _i32p, _u32p, _f32p, _f32p]
    lib.svdf_update_block.argtypes = [P, C.c_int, C.c_int, _u32p, _f32p, C.c_int, _f32p, _i32p, _u32p, _f32p]
    lib.svdf_predict_block.argtypes = lib.svdf_update_block.argtypes + [_f32p]
    lib.svdf_dataset_from_csr.restype = P
    lib.svdf_dataset_from_csr.argtypes = [P, C.c_long, _f32p, _i64p, _u32p, _f32p]
    lib.svdf_dataset_from_triples.restype = P
    lib.svdf_dataset_from_triples.argtypes = [P, C.c_long, _u32p, _u32p, _f32p]
    lib.svdf_dataset_from_pairs.restype = P
    lib.svdf_dataset_from_pairs.argtypes = [P, C.c_long, _u32p, _u32p, _u32p]
    lib.svdf_dataset_window_from_triples.restype = P
    lib.svdf_dataset_window_from_triples.argtypes = [P, C.c_long, _u32p, _u32p, _f32p]
    lib.svdf_dataset_window_from_pairs.restype = P
    lib.svdf_dataset_window_from_pairs.argtypes = [P, C.c_long, _u32p, _u32p, _u32p]
    lib.svdf_dataset_window_from_csr.restype = P
    lib.svdf_dataset_window_from_csr.argtypes = [P, C.c_long, _f32p, _i64p, _u32p, _f32p]
    lib.svdf_dataset_window_from_blocks.restype = P
    lib.svdf_dataset_window_from_blocks.argtypes = [P, C.c_long, _i32p, _i64p, _u32p, _f32p, _i64p, _f32p, _i64p, _u32p, _f32p]
    lib.svdf_ipc_setup.argtypes = [P, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_char_p]
    lib.svdf_ipc_connect.argtypes = [P, C.c_char_p]
    lib.svdf_ipc_window_pack.argtypes = [P, P, C.c_int]
    lib.svdf_ipc_window_reduce.argtypes = [P, C.c_int]
    lib.svdf_ipc_window_apply.argtypes = [P, C.c_int]
    lib.svdf_ipc_block_send.argtypes = [P, C.c_int, C.c_int]
    lib.svdf_ipc_block_recv.argtypes = [P, C.c_int, C.c_int, C.c_uint]
    lib.svdf_ipc_status.argtypes = [P]
    lib.svdf_ipc_close.argtypes = [P]
    lib.svdf_stratum_step.argtypes = [P, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, P]
    lib.svdf_item_block_set_at.argtypes = [P, C.c_int, C.c_int, P]
    lib.svdf_rccl_unique_id.argtypes = [C.c_char_p]
    lib.svdf_rccl_init.argtypes = [P, C.c_char_p, C.c_int, C.c_int]
    lib.svdf_rccl_window_allreduce.argtypes = [P, P, C.c_int]
    lib.svdf_rccl_block_handoff.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.svdf_rccl_block_arrive.argtypes = [P, C.c_int]
    lib.svdf_rccl_counter.restype = C.c_int64
    lib.svdf_rccl_counter.argtypes = [P, C.c_int]
    lib.svdf_rccl_close.argtypes = [P]
    lib.svdf_window_delta_pack.argtypes = [P, P, P, C.c_int, C.POINTER(C.c_int64)]
    lib.svdf_window_delta_apply.argtypes = [P, P, C.c_int]
    lib.svdf_window_delta_apply_local.argtypes = [P, P]
    lib.svdf_item_block_get.argtypes = [P, P, C.POINTER(C.c_int64)]
    lib.svdf_item_block_set.argtypes = [P, P]
    lib.svdf_set_view.restype = C.c_int64
    lib.svdf_set_view.argtypes = [P, C.c_int, _f32p, C.c_int64]
    lib.svdf_dataset_from_buffer_file.restype = P
    lib.svdf_dataset_from_buffer_file.argtypes = [P, C.c_char_p, C.c_int]
    lib.svdf_dataset_from_rank_buffer_file.restype = P
    lib.svdf_dataset_from_rank_buffer_file.argtypes = [P, C.c_char_p]
    lib.svdf_rank_prefetch_buffer_file.restype = C.c_int
    lib.svdf_rank_prefetch_buffer_file.argtypes = [P, C.c_char_p]
    lib.svdf_rank_sample_buffer_file.restype = C.c_int64
    lib.svdf_rank_sample_buffer_file.argtypes = [P, C.c_char_p, C.c_char_p]
    lib.svdf_dataset_from_blocks.restype = P
    lib.svdf_dataset_from_blocks.argtypes = [P, C.c_long, _i32p, _i64p, _u32p, _f32p, _i64p, _f32p, _i64p, _u32p, _f32p]
    lib.svdf_dataset_destroy.argtypes = [P]
    lib.svdf_train_dataset.argtypes = [P, P]
    lib.svdf_predict_dataset.argtypes = [P, P, _f32p]
    lib.svdf_dataset_info.restype = C.c_int64
    lib.svdf_dataset_info.argtypes = [P, C.c_int]
    lib.svdf_item_delta_buffer.restype = P
    lib.svdf_item_delta_buffer.argtypes = [P, C.POINTER(C.c_int64)]
    lib.svdf_item_delta_export.argtypes = [P, P]
    lib.svdf_item_delta_import.argtypes = [P, P]
    lib.svdf_item_delta_into.argtypes = [P, P, C.POINTER(C.c_int64)]
    lib.svdf_item_delta_apply_from.argtypes = [P, P]
    lib.svdf_item_delta_pack.argtypes = [P, P, C.c_int, C.POINTER(C.c_int64)]
    lib.svdf_item_delta_unpack.argtypes = [P, P, C.c_int, C.c_int]
    lib.svdf_set_stream.argtypes = [P, P]
    lib.svdf_item_delta_select.argtypes = [P, C.c_int, C.c_int]
    lib.svdf_get_view.restype = C.c_int64
    lib.svdf_get_view.argtypes = [P, C.c_int, _f32p, C.c_int64]
    lib.svdf_view_shape.argtypes = [P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.svdf_stream.restype = P
    lib.svdf_stream.argtypes = [P]
    lib.svdf_counter.restype = C.c_int64
    lib.svdf_counter.argtypes = [P, C.c_int]
    lib.svdf_set_knob.argtypes = [P, C.c_char_p, C.c_long]
    lib.svdf_schedule_resources.argtypes = [C.c_long, _i64p, _u32p, C.c_long, _i32p, _i64p, C.c_long]
    lib.svdf_eval_dataset.argtypes = [P, P, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.svdf_rank_eval_positions.argtypes = [P, C.c_long, _u32p, _i64p, _u32p, C.c_void_p, C.c_void_p, _i32p, _i32p, _i32p, _i32p]
    lib.svdf_rank_eval_metrics.argtypes = [C.c_long, _i64p, _i32p, C.c_void_p, C.c_void_p, C.c_int, _i32p, C.POINTER(RankMetrics)]
    lib.svdf_rank_eval.argtypes = [P, C.c_long, _u32p, _i64p, _u32p, C.c_void_p, C.c_void_p, C.c_int, _i32p, C.POINTER(RankMetrics)]
    lib.svdf_rank_topn.argtypes = [P, C.c_long, _u32p, C.c_void_p, C.c_void_p, C.c_int, _i32p, C.c_void_p, _i32p, _i32p]
    lib.svdf_item_topn.argtypes = [P, C.c_long, _u32p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, _i32p, C.c_void_p, _i32p, _i32p]
    lib.svdf_item_unit_rows.argtypes = [C.c_long, C.c_int, _f32p, _f32p]
    _fb = [C.c_void_p, C.c_void_p, C.c_void_p]   # fb_ptr, fb_index, fb_value behind `user`
    lib.svdf_rank_eval_positions_fb.argtypes = [P, C.c_long, _u32p] + _fb + [_i64p, _u32p, C.c_void_p, C.c_void_p, _i32p, _i32p, _i32p, _i32p]
    lib.svdf_rank_eval_fb.argtypes = [P, C.c_long, _u32p] + _fb + [_i64p, _u32p, C.c_void_p, C.c_void_p, C.c_int, _i32p, C.POINTER(RankMetrics)]
    lib.svdf_rank_topn_fb.argtypes = [P, C.c_long, _u32p] + _fb + [C.c_void_p, C.c_void_p, C.c_int, _i32p, C.c_void_p, _i32p, _i32p]
    _ul = [C.c_void_p, C.c_void_p, C.c_void_p]   # ul_ptr, ul_index, ul_value in place of `user`
    lib.svdf_rank_eval_positions_lines.argtypes = [P, C.c_long] + _ul + _fb + [_i64p, _u32p, C.c_void_p, C.c_void_p, _i32p, _i32p, _i32p, _i32p]
    lib.svdf_rank_eval_lines.argtypes = [P, C.c_long] + _ul + _fb + [_i64p, _u32p, C.c_void_p, C.c_void_p, C.c_int, _i32p, C.POINTER(RankMetrics)]
    lib.svdf_rank_topn_lines.argtypes = [P, C.c_long] + _ul + _fb + [C.c_void_p, C.c_void_p, C.c_int, _i32p, C.c_void_p, _i32p, _i32p]
    _cand = [C.c_void_p] + _ul + _fb   # user or ul_ptr, ul_index, ul_value; fb_ptr, fb_index, fb_value
    lib.svdf_rank_eval_positions_cand.argtypes = [P, C.c_long] + _cand + [_i64p, _u32p, C.c_void_p, C.c_void_p, _i32p, _i32p, _i32p, _i32p]
    lib.svdf_rank_eval_cand.argtypes = [P, C.c_long] + _cand + [_i64p, _u32p, C.c_void_p, C.c_void_p, C.c_int, _i32p, C.POINTER(RankMetrics)]
    lib.svdf_rank_topn_cand.argtypes = [P, C.c_long] + _cand + [C.c_void_p, C.c_void_p, C.c_int, _i32p, C.c_void_p, _i32p, _i32p]
    _lists = [_i64p, _u32p, C.c_void_p, C.c_void_p]   # pos_ptr, pos_item, ban_ptr, ban_item
    lib.svdf_rank_negatives.argtypes = [C.c_long] + _lists + [C.c_long, C.c_int, C.c_uint64, _i32p]
    lib.svdf_rank_eval_positions_sampled.argtypes = [P, C.c_long] + _cand + _lists + [C.c_int, C.c_uint64, _i32p, _i32p, _i32p, _i32p, C.c_void_p]
    lib.svdf_rank_eval_sampled.argtypes = [P, C.c_long] + _cand + _lists + [C.c_int, C.c_uint64, C.c_int, _i32p, C.POINTER(RankMetrics)]
    lib.svdf_pair_source_create.restype = P
    lib.svdf_pair_source_create.argtypes = [P, C.c_long, _u32p, _u32p]
    lib.svdf_pair_source_destroy.argtypes = [P]
    lib.svdf_dataset_from_pair_source.restype = P
    lib.svdf_dataset_from_pair_source.argtypes = [P, P, C.c_int, C.c_uint64]
    lib.svdf_pair_source_draw.argtypes = [P, P, C.c_int, C.c_uint64, _u32p]
    lib.svdf_pair_negatives.argtypes = [C.c_long, C.c_long, C.c_long, _u32p, _u32p, C.c_int, C.c_uint64, _u32p]
    lib.svdf_dataset_from_pair_source_hard.restype = P
    lib.svdf_dataset_from_pair_source_hard.argtypes = [P, P, C.c_int, C.c_int, C.c_uint64]
    lib.svdf_pair_source_draw_hard.argtypes = [P, P, C.c_int, C.c_int, C.c_uint64, _u32p, C.c_void_p]
    lib.svdf_pair_hard_negatives.argtypes = [C.c_long, C.c_long, C.c_long, _u32p, _u32p, C.c_int, C.c_int, C.c_uint64, C.c_int, _f32p, _f32p, _f32p, _u32p,
                                             C.c_void_p]
    lib.svdf_dataset_from_pair_source_shuffled.restype = P
    lib.svdf_dataset_from_pair_source_shuffled.argtypes = [P, P, C.c_int, C.c_int, C.c_uint64, C.c_uint64]
    lib.svdf_pair_source_draw_shuffled.argtypes = [P, P, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _u32p, _u32p, _u32p, C.c_void_p]
    lib.svdf_pair_order.argtypes = [C.c_long, C.c_uint64, _u32p]
    lib.svdf_pair_source_create_weighted.restype = P
    lib.svdf_pair_source_create_weighted.argtypes = [P, C.c_long, _u32p, _u32p, _u32p]
    lib.svdf_pair_negatives_weighted.argtypes = [C.c_long, C.c_long, C.c_long, _u32p, _u32p, _u32p, C.c_int, C.c_uint64, _u32p]
    lib.svdf_pair_hard_negatives_weighted.argtypes = [C.c_long, C.c_long, C.c_long, _u32p, _u32p, _u32p, C.c_int, C.c_int, C.c_uint64, C.c_int, _f32p, _f32p,
                                                      _f32p, _u32p, C.c_void_p]
    lib.svdf_pair_weight_lookup.argtypes = [P, C.c_long, _u32p, C.c_int, C.c_long, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"), _u32p]
    lib.svdf_ranker_create.restype = P
    lib.svdf_ranker_create.argtypes = [C.c_uint8] * 4 + [C.c_int]
    lib.svdf_ranker_destroy.argtypes = [P]
    lib.svdf_ranker_set_param.argtypes = [P, C.c_char_p, C.c_char_p]
    lib.svdf_ranker_load_model.argtypes = [P, C.c_void_p]
    lib.svdf_ranker_init.argtypes = [P, C.c_int]
    lib.svdf_ranker_process_csr.restype = C.c_int64
    lib.svdf_ranker_process_csr.argtypes = [P, C.c_float, C.c_int, C.c_int, C.c_int, _u32p, _f32p, _i32p, C.c_int64]
    lib.svdf_ranker_process_rows.restype = C.c_int64
    lib.svdf_ranker_process_rows.argtypes = [P, C.c_int, _f32p, _i32p, _u32p, _f32p, _i32p, C.c_int64]
    lib.svdf_ranker_process_block.restype = C.c_int64
    lib.svdf_ranker_process_block.argtypes = [P, C.c_int, C.c_int, _u32p, _f32p, C.c_int, _f32p, _i32p, _u32p, _f32p, _i32p, C.c_int64]
    lib.svdf_ranker_counter.restype = C.c_int64
    lib.svdf_ranker_counter.argtypes = [P, C.c_int]
    lib.svdf_rand_peek.argtypes = [C.c_long, _i32p]
    lib.svdf_rand_skip.argtypes = [C.c_long]
    lib.svdf_rank_geometry.argtypes = [P, C.c_int, C.c_long, C.c_int, C.c_void_p, C.POINTER(C.c_long)]
    lib.svdf_level_geometry.argtypes = [P, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_long)]
    lib.svdf_device_expf.argtypes = [C.c_void_p, C.c_uint, C.c_uint, _f32p, C.c_long]
    lib.svdf_window_rule.restype = C.c_long
    lib.svdf_window_rule.argtypes = [C.c_int, C.POINTER(WindowRuleIn)]
    lib.svdf_window_rule_as_cut.restype = C.c_long
    lib.svdf_window_rule_as_cut.argtypes = [C.c_long, C.c_long, C.c_int, C.POINTER(C.c_void_p), C.c_long, C.c_double, C.c_long, C.c_int, C.c_double, C.c_int]
    lib.svdf_window_block_cuts.argtypes = [C.c_long, _i32p, C.c_long, C.c_void_p]
    lib.svdf_debug_sort_labels.argtypes = [C.c_long, _f32p, _i32p, _i32p]
    lib.svdf_debug_sort_scores.argtypes = [C.c_long, _f32p, C.c_int, _i32p, _i32p]
    lib.svdf_set_error_mode(1)   # python callers get exceptions instead of exit(-1)
    _lib = lib
    return lib


def device_count():
    return load_library().svdf_device_count()


def rccl_unique_id():
    """ncclGetUniqueId (rank 0): 128 bytes for svdf_rccl_init on every rank"""
    buf = C.create_string_buffer(128)
    if load_library().svdf_rccl_unique_id(buf) != 0:
        raise SvdfError(load_library().svdf_last_error().decode())
    return buf.raw


def rand_peek(n):
    """the next n libc rand() results, without consuming them (svdf_rand_peek)"""
    out = np.zeros(max(int(n), 1), np.int32)
    if load_library().svdf_rand_peek(int(n), out) != 0:
        raise SvdfError(load_library().svdf_last_error().decode())
    return out[:n]


def rand_skip(n):
    """advance libc rand() by n draws (svdf_rand_skip)"""
    if load_library().svdf_rand_skip(int(n)) != 0:
        raise SvdfError(load_library().svdf_last_error().decode())


def debug_sort_labels(label):
    """(ids sorted by label with the restated libstdc++ std::sort of svdf_stdsort.h, the same with the C++ library's std::sort)"""
    label = np.ascontiguousarray(label, np.float32)
    a, b = np.zeros(max(len(label), 1), np.int32), np.zeros(max(len(label), 1), np.int32)
    if load_library().svdf_debug_sort_labels(len(label), _pad(label, np.float32), a, b) != 0:
        raise SvdfError(load_library().svdf_last_error().decode())
    return a[:len(label)], b[:len(label)]


def debug_sort_scores(score, threads=8):
    """(ids by descending score with the ranker's threaded restatement of std::sort, the same with the library's std::sort over the
    reference's Entry struct)"""
    score = np.ascontiguousarray(score, np.float32)
    a, b = np.zeros(max(len(score), 1), np.int32), np.zeros(max(len(score), 1), np.int32)
    if load_library().svdf_debug_sort_scores(len(score), _pad(score, np.float32), int(threads), a, b) != 0:
        raise SvdfError(load_library().svdf_last_error().decode())
    return a[:len(score)], b[:len(score)]


def device_expf(x=None, first=0, step=1, n=None):
    """The expf the sigmoid links use ON THE GPU (svdf_device.h: glibc_expf), over an array or over the floats with bit
    patterns first + j*step; tests compare it with the host libm bit for bit."""
    lib = load_library()
    if x is not None:
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty(len(x), np.float32)
        rc = lib.svdf_device_expf(x.ctypes.data_as(C.c_void_p), 0, 0, out, len(x))
    else:
        out = np.empty(n, np.float32)
        rc = lib.svdf_device_expf(None, first, step, out, n)
    if rc != 0:
        raise SvdfError("svdf_device_expf failed")
    return out


def _pad(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a if a.size else np.zeros(1, dtype=dtype)


def schedule_resources(res_ptr, res, num_res):
    """Host scheduler (no GPU needed): returns (order, level_ptr)."""
    lib = load_library()
    n = len(res_ptr) - 1
    order = np.zeros(max(n, 1), np.int32)
    level_ptr = np.zeros(n + 2, np.int64)
    nl = lib.svdf_schedule_resources(n, _pad(res_ptr, np.int64), _pad(res, np.uint32), int(num_res), order, level_ptr, n + 2)
    if nl < 0:
        raise SvdfError(lib.svdf_last_error().decode())
    return order[:n], level_ptr[:nl + 1]


class Dataset:
    """A scheduled, HBM-resident training set (svdf_dataset)."""

    def __init__(self, trainer, handle):
        self.trainer, self.h = trainer, handle

    def info(self, what):
        return int(self.trainer.lib.svdf_dataset_info(self.h, what))

    num_row = property(lambda s: s.info(0))
    num_batches = property(lambda s: s.info(1))
    max_batch = property(lambda s: s.info(2))
    kind = property(lambda s: s.info(3))
    algorithmic_bytes = property(lambda s: s.info(4))
    num_units = property(lambda s: s.info(5))
    num_simple_units = property(lambda s: s.info(6))

    def close(self):
        if self.h:
            self.trainer.lib.svdf_dataset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PairSource:
    """Positives (user, item) resident in HBM, the source of rank-pair passes whose negatives the device draws (svdf_pair_source)."""

    def __init__(self, trainer, handle, num_row):
        self.trainer, self.lib, self.h, self.num_row = trainer, trainer.lib, handle, num_row

    def close(self):
        """safe after the trainer's close; data sets built from the source stay valid"""
        if self.h:
            self.lib.svdf_pair_source_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Trainer:
    """ISVDTrainer over the HIP engine.  device=-1: current GPU (required); device=-2: host-only
    handle for config / model-file / staging logic (compute calls raise)."""

    def __init__(self, format_type=0, active_type=0, extend_type=0, variant_type=0, params=None, device=-1):
        self.lib = load_library()
        self.h = self.lib.svdf_create(format_type, active_type, extend_type, variant_type, device)
        if not self.h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        self.mtype = bytes([format_type, active_type, extend_type, variant_type])
        for k, v in (params or {}).items():
            self.set_param(k, v)

    # -- plumbing
    def _ok(self, rc):
        if rc != 0:
            raise SvdfError(self.lib.svdf_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "_async_fo", None) is not None:   # an asynchronous save still open: join the writer and close its file (buffered bytes!)
                try:
                    self.save_model_end()
                except Exception:
                    pass
            self.lib.svdf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ISVDTrainer
    def set_param(self, name, val):
        self._ok(self.lib.svdf_set_param(self.h, str(name).encode(), str(val).encode()))

    def seed(self, s):
        self.lib.svdf_seed(int(s))

    def init_model(self):
        self._ok(self.lib.svdf_init_model(self.h))

    def init_trainer(self):
        self._ok(self.lib.svdf_init_trainer(self.h))

    def set_round(self, r):
        self._ok(self.lib.svdf_set_round(self.h, int(r)))

    def finish_round(self):
        self._ok(self.lib.svdf_finish_round(self.h))

    def save_model_begin(self, path, with_type_header=True):
        """svdf_save_model_begin: the model as of NOW goes to `path` on a writer thread while training continues; save_model_end() joins it and closes the file."""
        assert getattr(self, "_async_fo", None) is None, "one asynchronous save at a time"
        fo = _libc.fopen(str(path).encode(), b"wb")
        if not fo:
            raise SvdfError("can not open file \"%s\"" % path)
        if with_type_header:
            hdr = (C.c_char * 4).from_buffer_copy(self.mtype)
            _libc.fwrite(hdr, 1, 4, C.c_void_p(fo))
        self._async_fo = fo
        try:
            self._ok(self.lib.svdf_save_model_begin(self.h, fo))
        except Exception:
            _libc.fclose(fo)
            self._async_fo = None
            raise

    def save_model_end(self):
        fo = getattr(self, "_async_fo", None)
        if fo is None:
            return
        try:
            self._ok(self.lib.svdf_save_model_end(self.h))
        finally:
            _libc.fclose(fo)
            self._async_fo = None

    def save_model(self, path, with_type_header=True):
        """Caller-side protocol of svd_feature.cpp:184-191: fopen, 4-byte SVDTypeParam, save_model(fo)."""
        fo = _libc.fopen(str(path).encode(), b"wb")
        if not fo:
            raise SvdfError("can not open file \"%s\"" % path)
        try:
            if with_type_header:
                hdr = (C.c_char * 4).from_buffer_copy(self.mtype)
                _libc.fwrite(hdr, 1, 4, C.c_void_p(fo))
            self._ok(self.lib.svdf_save_model(self.h, fo))
        finally:
            _libc.fclose(fo)

    def load_model(self, path, with_type_header=True):
        fi = _libc.fopen(str(path).encode(), b"rb")
        if not fi:
            raise SvdfError("can not open file \"%s\"" % path)
        try:
            if with_type_header:
                buf = (C.c_char * 4)()
                _libc.fread(buf, 1, 4, C.c_void_p(fi))
            self._ok(self.lib.svdf_load_model(self.h, fi))
        finally:
            _libc.fclose(fi)

    def update_csr(self, label, ng, nu, ni, index, value):
        self._ok(self.lib.svdf_update_csr(self.h, float(label), ng, nu, ni, _pad(index, np.uint32), _pad(value, np.float32)))

    def predict_csr(self, label, ng, nu, ni, index, value):
        self.lib.svdf_last_error()
        return self.lib.svdf_predict_csr(self.h, float(label), ng, nu, ni, _pad(index, np.uint32), _pad(value, np.float32))

    def update_batch(self, d):
        self._ok(self.lib.svdf_update_csr_batch(self.h, d.num_row, _pad(d.row_label, np.float32), _pad(d.row_ptr, np.int32),
                                                _pad(d.feat_index, np.uint32), _pad(d.feat_value, np.float32)))

    def predict_batch(self, d):
        out = np.zeros(max(d.num_row, 1), dtype=np.float32)
        self._ok(self.lib.svdf_predict_csr_batch(self.h, d.num_row, _pad(d.row_label, np.float32), _pad(d.row_ptr, np.int32),
                                                 _pad(d.feat_index, np.uint32), _pad(d.feat_value, np.float32), out))
        return out[:d.num_row]

    def update_block(self, b):
        d = b.data
        self._ok(self.lib.svdf_update_block(self.h, b.num_ufeedback, b.extend_tag, _pad(b.index_ufeedback, np.uint32),
                                            _pad(b.value_ufeedback, np.float32), d.num_row, _pad(d.row_label, np.float32),
                                            _pad(d.row_ptr, np.int32), _pad(d.feat_index, np.uint32), _pad(d.feat_value, np.float32)))

    def predict_block(self, b):
        d = b.data
        out = np.zeros(max(d.num_row, 1), dtype=np.float32)
        self._ok(self.lib.svdf_predict_block(self.h, b.num_ufeedback, b.extend_tag, _pad(b.index_ufeedback, np.uint32),
                                             _pad(b.value_ufeedback, np.float32), d.num_row, _pad(d.row_label, np.float32),
                                             _pad(d.row_ptr, np.int32), _pad(d.feat_index, np.uint32), _pad(d.feat_value, np.float32), out))
        return out[:d.num_row]

    # -- resident datasets
    def dataset_from_csr(self, d):
        h = self.lib.svdf_dataset_from_csr(self.h, d.num_row, _pad(d.row_label, np.float32), _pad(d.row_ptr, np.int64),
                                           _pad(d.feat_index, np.uint32), _pad(d.feat_value, np.float32))
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    def dataset_from_triples(self, user, item, label):
        n = len(label)
        h = self.lib.svdf_dataset_from_triples(self.h, n, _pad(user, np.uint32), _pad(item, np.uint32), _pad(label, np.float32))
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    def dataset_window_from_triples(self, user, item, label):
        """One exchange window of a rank's shard for the window-minibatch step (svdf_dataset_window_from_triples)."""
        h = self.lib.svdf_dataset_window_from_triples(self.h, len(label), _pad(user, np.uint32), _pad(item, np.uint32), _pad(label, np.float32))
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    def dataset_window_from_pairs(self, user, pos, neg):
        """One exchange window of a rank's rank pairs for the window-minibatch step (svdf_dataset_window_from_pairs)."""
        h = self.lib.svdf_dataset_window_from_pairs(self.h, len(user), _pad(user, np.uint32), _pad(pos, np.uint32), _pad(neg, np.uint32))
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    def dataset_window_from_csr(self, d):
        """One exchange window of rows with global features / several item entries (svdf_dataset_window_from_csr)."""
        h = self.lib.svdf_dataset_window_from_csr(self.h, d.num_row, _pad(d.row_label, np.float32), _pad(d.row_ptr, np.int64),
                                                  _pad(d.feat_index, np.uint32), _pad(d.feat_value, np.float32))
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    def dataset_window_from_blocks(self, ba):
        """One exchange window of user-group (SVD++) blocks, a data.BlockArrays (svdf_dataset_window_from_blocks)."""
        h = self.lib.svdf_dataset_window_from_blocks(self.h, ba.num_block, _pad(ba.extend_tag, np.int32), _pad(ba.fb_ptr, np.int64),
                                                     _pad(ba.fb_index, np.uint32), _pad(ba.fb_value, np.float32), _pad(ba.block_row_ptr, np.int64),
                                                     _pad(ba.row_label, np.float32), _pad(ba.row_ptr, np.int64), _pad(ba.feat_index, np.uint32),
                                                     _pad(ba.feat_value, np.float32))
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    # -- cross-process direct exchange through IPC-mapped buffers (svdf_ipc.cpp)
    def ipc_setup(self, rank, world, wire_bytes, block_floats=0):
        """allocates + exports this rank's wire buffer / flag page; returns the 128 handle bytes to all-gather"""
        buf = C.create_string_buffer(128)
        self._ok(self.lib.svdf_ipc_setup(self.h, rank, world, int(wire_bytes), int(block_floats), buf))
        return buf.raw

    def ipc_connect(self, all_handles):
        self._ok(self.lib.svdf_ipc_connect(self.h, bytes(all_handles)))

    def ipc_window_pack(self, ds, half=False):
        self._ok(self.lib.svdf_ipc_window_pack(self.h, ds.h, 1 if half else 0))

    def ipc_window_reduce(self, half=False):
        self._ok(self.lib.svdf_ipc_window_reduce(self.h, 1 if half else 0))

    def ipc_window_apply(self, half=False):
        self._ok(self.lib.svdf_ipc_window_apply(self.h, 1 if half else 0))

    def ipc_block_send(self, dst, slot):
        self._ok(self.lib.svdf_ipc_block_send(self.h, dst, slot))

    def ipc_block_recv(self, src, slot, seq):
        self._ok(self.lib.svdf_ipc_block_recv(self.h, src, slot, seq))

    def ipc_status(self):
        return int(self.lib.svdf_ipc_status(self.h))

    def ipc_close(self):
        self._ok(self.lib.svdf_ipc_close(self.h))

    # -- the exchanges issued from C++ straight into RCCL (svdf_rccl.cpp): the rank's own communicator
    def rccl_init(self, unique_id, rank, world):
        self._ok(self.lib.svdf_rccl_init(self.h, bytes(unique_id), rank, world))

    def rccl_window_allreduce(self, ds, half=False):
        self._ok(self.lib.svdf_rccl_window_allreduce(self.h, ds.h, 1 if half else 0))

    def rccl_block_handoff(self, dst, src, slot, in_block, nblocks):
        self._ok(self.lib.svdf_rccl_block_handoff(self.h, dst, src, slot, in_block, nblocks))

    def rccl_block_arrive(self, slot):
        self._ok(self.lib.svdf_rccl_block_arrive(self.h, slot))

    def rccl_counter(self, what):
        return int(self.lib.svdf_rccl_counter(self.h, what))

    def rccl_close(self):
        self._ok(self.lib.svdf_rccl_close(self.h))

    def window_delta_pack(self, ds, device_ptr, half=False):
        """Sum of the trained window's item-side contributions into the wire buffer at device_ptr; returns its element count."""
        n = C.c_int64()
        self._ok(self.lib.svdf_window_delta_pack(self.h, ds.h, C.c_void_p(device_ptr), 1 if half else 0, C.byref(n)))
        return n.value

    def window_delta_apply(self, device_ptr, half=False):
        """replicated ranges += the (all-reduced) wire buffer"""
        self._ok(self.lib.svdf_window_delta_apply(self.h, C.c_void_p(device_ptr), 1 if half else 0))

    def window_delta_apply_local(self, ds):
        """stratified schedule: the active item block (item_delta_select) += the trained window's per-item sums, in place"""
        self._ok(self.lib.svdf_window_delta_apply_local(self.h, ds.h))

    def item_block_count(self):
        n = C.c_int64()
        self._ok(self.lib.svdf_item_block_get(self.h, None, C.byref(n)))
        return n.value

    def item_block_get(self, device_ptr):
        n = C.c_int64()
        self._ok(self.lib.svdf_item_block_get(self.h, C.c_void_p(device_ptr), C.byref(n)))
        return n.value

    def item_block_set(self, device_ptr):
        self._ok(self.lib.svdf_item_block_set(self.h, C.c_void_p(device_ptr)))

    def stratum_step(self, handles, n, block, nblocks, out_ptr):
        """handles: a ctypes array of the window data sets' handles (svdf_stratum_step)"""
        self._ok(self.lib.svdf_stratum_step(self.h, handles, n, block, nblocks, C.c_void_p(out_ptr) if out_ptr else None))

    def item_block_set_at(self, block, nblocks, device_ptr):
        self._ok(self.lib.svdf_item_block_set_at(self.h, block, nblocks, C.c_void_p(device_ptr)))

    def dataset_from_pairs(self, user, pos, neg):
        """Rank pairs (user, positive item, negative item), see svdf_dataset_from_pairs."""
        h = self.lib.svdf_dataset_from_pairs(self.h, len(user), _pad(user, np.uint32), _pad(pos, np.uint32), _pad(neg, np.uint32))
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    # -- passes of rank pairs from positives only (svdf_pair_source_*)
    def pair_source(self, user, pos_item, item_weight=None):
        """The positives (user, item) of pairwise training, uploaded once: see svdf_pair_source_create.  item_weight (uint32 per item): every
        pass of the source draws its negatives with probability proportional to these weights (svdf_pair_source_create_weighted)."""
        n, user, pos_item = _pair_rows(user, pos_item)
        if item_weight is None:
            h = self.lib.svdf_pair_source_create(self.h, n, user, pos_item)
        else:
            rows, cols = C.c_int(-1), C.c_int()
            known = self.lib.svdf_view_shape(self.h, VIEW["W_item"], C.byref(rows), C.byref(cols)) == 0 and rows.value > 0
            h = self.lib.svdf_pair_source_create_weighted(self.h, n, user, pos_item, _item_weights(item_weight, rows.value if known else None))
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return PairSource(self, h, n)

    def dataset_from_pair_source(self, src, num_neg=1, seed=0, hard=None, shuffle=None):
        """One pass over the source's rows with num_neg negatives each, drawn on the device from (seed, pair index): the data set
        dataset_from_pairs builds from pair_negatives(...)'s column, without that column crossing PCIe where a route allows.
        hard=C: every negative is the best-scoring of C drawn candidates on the live model (pair_hard_negatives' column).
        shuffle=order_seed: the rows in the order pair_order(n, order_seed), permuted on the device -- the pass of a source created from
        user[sigma], pos_item[sigma]; None: the source's own order."""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if shuffle is not None:
            h = self.lib.svdf_dataset_from_pair_source_shuffled(self.h, src.h, int(num_neg), 0 if hard is None else _shuffled_cand(hard), seed,
                                                                int(shuffle) & 0xFFFFFFFFFFFFFFFF)
        elif hard is None:
            h = self.lib.svdf_dataset_from_pair_source(self.h, src.h, int(num_neg), seed)
        else:
            h = self.lib.svdf_dataset_from_pair_source_hard(self.h, src.h, int(num_neg), int(hard), seed)
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    def pair_source_draw(self, src, num_neg, seed, hard=None, return_scores=False, shuffle=None):
        """the negative column the device draws for such a pass: uint32[n * num_neg]; with hard=C the best of C candidates per pair and,
        with return_scores, (negatives, float32 scores of the chosen candidates).  shuffle=order_seed: the three columns (user, pos, neg) of
        the shuffled pass and, with return_scores, the scores as a fourth."""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if hard is None and return_scores:
            raise SvdfError("pair_source: return_scores needs hard=")
        if shuffle is not None:
            size = max(_pass_size(src.num_row, num_neg) if hard is None else _hard_size(src.num_row, num_neg, hard), 1)
            user, pos, neg, score = np.zeros(size, np.uint32), np.zeros(size, np.uint32), np.zeros(size, np.uint32), np.zeros(size, np.float32)
            self._ok(self.lib.svdf_pair_source_draw_shuffled(self.h, src.h, int(num_neg), 0 if hard is None else _shuffled_cand(hard), seed,
                                                             int(shuffle) & 0xFFFFFFFFFFFFFFFF, user, pos, neg, _opt_ptr(score if return_scores else None)))
            N = src.num_row * int(num_neg)
            return (user[:N], pos[:N], neg[:N], score[:N]) if return_scores else (user[:N], pos[:N], neg[:N])
        if hard is None:
            neg = np.zeros(max(_pass_size(src.num_row, num_neg), 1), np.uint32)
            self._ok(self.lib.svdf_pair_source_draw(self.h, src.h, int(num_neg), seed, neg))
            return neg[:src.num_row * int(num_neg)]
        size = max(_hard_size(src.num_row, num_neg, hard), 1)
        neg, score = np.zeros(size, np.uint32), np.zeros(size, np.float32)
        self._ok(self.lib.svdf_pair_source_draw_hard(self.h, src.h, int(num_neg), int(hard), seed, neg, _opt_ptr(score if return_scores else None)))
        N = src.num_row * int(num_neg)
        return (neg[:N], score[:N]) if return_scores else neg[:N]

    def dataset_from_blocks(self, blocks):
        """blocks: list of PlusBlock in file order (one pass of a user-group buffer), or a flat BlockArrays."""
        ba = blocks if isinstance(blocks, BlockArrays) else BlockArrays.from_blocks(blocks)
        h = self.lib.svdf_dataset_from_blocks(self.h, ba.num_block, _pad(ba.extend_tag, np.int32), ba.fb_ptr, _pad(ba.fb_index, np.uint32),
                                              _pad(ba.fb_value, np.float32), ba.block_row_ptr, _pad(ba.row_label, np.float32),
                                              _pad(ba.row_ptr, np.int64), _pad(ba.feat_index, np.uint32), _pad(ba.feat_value, np.float32))
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    def dataset_from_buffer_file(self, path, user_group=False):
        """Resident dataset straight from a reference buffer file (make_feature_buffer / make_ugroup_buffer output)."""
        h = self.lib.svdf_dataset_from_buffer_file(self.h, str(path).encode(), 1 if user_group else 0)
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    def dataset_from_rank_buffer_file(self, path):
        """One pass of the reference's input_type = 2 (user-group buffer file through the rank-pair sampler)."""
        h = self.lib.svdf_dataset_from_rank_buffer_file(self.h, str(path).encode())
        if not h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return Dataset(self, h)

    def rank_prefetch_buffer_file(self, path):
        """Draw the next rank-pair pass on a background thread; the next dataset_from_rank_buffer_file takes it."""
        self._ok(self.lib.svdf_rank_prefetch_buffer_file(self.h, str(path).encode()))

    def rank_sample_buffer_file(self, in_path, out_path):
        """The same pass written as a user-group buffer file (host only); returns the number of generated rows."""
        n = self.lib.svdf_rank_sample_buffer_file(self.h, str(in_path).encode(), str(out_path).encode())
        if n < 0:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return int(n)

    def train_dataset(self, ds):
        self._ok(self.lib.svdf_train_dataset(self.h, ds.h))

    def eval_dataset(self, ds, scale_score=1.0):
        """RMSEEvaluator over a resident data set (svd_feature_infer.cpp:38-56, 243-277): (sum of squared errors, count)."""
        ss, cnt = C.c_double(), C.c_int64()
        self._ok(self.lib.svdf_eval_dataset(self.h, ds.h, float(scale_score), C.byref(ss), C.byref(cnt)))
        return ss.value, cnt.value

    def predict_dataset(self, ds):
        out = np.zeros(max(ds.num_row, 1), dtype=np.float32)
        self._ok(self.lib.svdf_predict_dataset(self.h, ds.h, out))
        return out[:ds.num_row]

    # -- batch ranking evaluation on the live model (svdf_rank_eval_*)
    @staticmethod
    def _rank_lists(users, pos_ptr, pos_item, ban_ptr, ban_item):
        users, pos_ptr = np.ascontiguousarray(users, np.uint32), _pad(pos_ptr, np.int64)
        if len(pos_ptr) != len(users) + 1:
            raise SvdfError("rank_eval: pos_ptr must have one entry more than users")
        if ban_ptr is not None:
            ban_ptr, ban_item = _pad(ban_ptr, np.int64), _pad(ban_item if ban_item is not None else [], np.uint32)
            if len(ban_ptr) != len(users) + 1:
                raise SvdfError("rank_eval: ban_ptr must have one entry more than users")
        return users, pos_ptr, _pad(pos_item, np.uint32), ban_ptr, (ban_item if ban_ptr is not None else None)

    @staticmethod
    def _feedback_lists(who, feedback, S):
        """feedback = (fb_ptr, fb_index, fb_value), section s carrying the entries [fb_ptr[s], fb_ptr[s + 1]) -> the three pointer arguments of the
        svdf_rank_*_fb calls (the arrays are kept alive by the returned tuple); fb_ptr = None passes NULL pointers"""
        fb_ptr, fb_index, fb_value = feedback
        if fb_ptr is None:
            return (None, None, None), ()
        keep = (_pad(fb_ptr, np.int64), _pad(fb_index if fb_index is not None else [], np.uint32), _pad(fb_value if fb_value is not None else [], np.float32))
        if len(keep[0]) != S + 1:
            raise SvdfError(who + ": fb_ptr must have one entry more than users")
        n = int(keep[0][-1]) if S else 0
        if n > 0 and (len(keep[1]) < n or len(keep[2]) < n):
            raise SvdfError(who + ": fb_index / fb_value are shorter than fb_ptr says")
        return tuple(_opt_ptr(a) for a in keep), keep

    @staticmethod
    def _user_lines(who, users, lines):
        """lines = (ul_ptr, ul_index, ul_value), section s bringing the USER line entries [ul_ptr[s], ul_ptr[s + 1]) in place of a user ->
        (S, the three pointer arguments of the svdf_rank_*_lines calls, the arrays they point into); the section count is ul_ptr's"""
        if users is not None:
            raise SvdfError(who + ": with lines= the sections bring USER lines: users must be None")
        ul_ptr, ul_index, ul_value = lines
        if ul_ptr is None:
            raise SvdfError(who + ": ul_ptr is missing")
        keep = (_pad(ul_ptr, np.int64), _pad(ul_index if ul_index is not None else [], np.uint32), _pad(ul_value if ul_value is not None else [], np.float32))
        S = len(ul_ptr) - 1
        if S < 0:
            raise SvdfError(who + ": ul_ptr must have one entry more than there are sections")
        n = int(keep[0][S]) if S else 0
        if n > 0 and (len(keep[1]) < n or len(keep[2]) < n):
            raise SvdfError(who + ": ul_index / ul_value are shorter than ul_ptr says")
        return S, tuple(_opt_ptr(a) for a in keep), keep

    def _cand_call(self, who, users, feedback, lines, candidates, ban_ptr):
        """candidates = (cand_ptr, cand_item), section s ranking over the ids cand_item[cand_ptr[s] .. cand_ptr[s + 1]) -> (S, the seven
        pointer arguments of the svdf_rank_*_cand calls that name the sections -- user, ul_*, fb_* --, the two of the lists, the arrays they point into)"""
        if ban_ptr is not None:
            raise SvdfError(who + ": bans and candidates exclude each other")
        if lines is not None:
            S, ul, keep_ul = self._user_lines(who, users, lines)
            who_ptr = [None] + list(ul)
        else:
            keep_ul = _pad(np.ascontiguousarray(users, np.uint32), np.uint32)
            S = len(np.ascontiguousarray(users, np.uint32))
            who_ptr = [_opt_ptr(keep_ul), None, None, None]
        fb, keep_fb = self._feedback_lists(who, feedback or (None, None, None), S)
        cand_ptr, cand_item = candidates
        keep = (_pad(cand_ptr, np.int64) if cand_ptr is not None else None, _pad(cand_item if cand_item is not None else [], np.uint32))
        if keep[0] is not None:
            if len(keep[0]) != S + 1:
                raise SvdfError(who + ": cand_ptr must have one entry more than there are sections")
            if S and cand_item is not None and int(keep[0][S]) > len(keep[1]):
                raise SvdfError(who + ": cand_item is shorter than cand_ptr says")
        cand = [_opt_ptr(keep[0]), _opt_ptr(keep[1]) if cand_item is not None else None]
        return S, who_ptr + list(fb), cand, (keep_ul, keep_fb, keep)

    def _sampled_call(self, users, feedback, lines, candidates, sampled, pos_ptr, pos_item, ban_ptr, ban_item):
        """sampled = (num_neg, seed) -> (S, the arguments of the svdf_rank_eval*_sampled calls from `user` to `seed`, the arrays they point into)"""
        who = "rank_eval"
        if candidates is not None:
            raise SvdfError(who + ": candidates and sampled exclude each other")
        num_neg, seed = sampled
        if lines is not None:
            S, ul, keep_ul = self._user_lines(who, users, lines)
            who_ptr = [None] + list(ul)
        else:
            keep_ul = _pad(np.ascontiguousarray(users, np.uint32), np.uint32)
            S = len(np.ascontiguousarray(users, np.uint32))
            who_ptr = [_opt_ptr(keep_ul), None, None, None]
        fb, keep_fb = self._feedback_lists(who, feedback or (None, None, None), S)
        pos_ptr, pos_item, ban_ptr, ban_item = _sampled_lists(S, pos_ptr, pos_item, ban_ptr, ban_item)
        args = who_ptr + list(fb) + [pos_ptr, pos_item, _opt_ptr(ban_ptr), _opt_ptr(ban_item), int(num_neg), int(seed) & 0xFFFFFFFFFFFFFFFF]
        return S, args, (keep_ul, keep_fb, pos_ptr, pos_item, ban_ptr, ban_item)

    def rank_positions(self, users, pos_ptr, pos_item, ban_ptr=None, ban_item=None, feedback=None, lines=None, candidates=None, sampled=None,
                       return_negatives=False):
        """svdf_rank_eval_positions: (position, tied) per positive, (ranked, nan) per section.  feedback = (fb_ptr, fb_index, fb_value): the
        sections' feedback lists, for user-group trainers (svdf_rank_eval_positions_fb).  lines = (ul_ptr, ul_index, ul_value):
        the sections bring USER lines of several (id, value) entries and the trainer may have side tables (svdf_rank_eval_positions_lines,
        DESIGN.md 6z); users is None then, and feedback= combines with it.  candidates = (cand_ptr, cand_item): section s ranks over its own
        item list and its positives instead of the catalogue minus bans (svdf_rank_eval_positions_cand); it combines with
        feedback= and lines=, and ban_ptr must be None.  sampled = (num_neg, seed): section s ranks its positives against num_neg negatives
        the device draws by the published rule from (seed, s, the section's bans and positives) (svdf_rank_eval_positions_sampled, DESIGN.md
        6ab); it combines with feedback= and lines=, never with candidates=; return_negatives=True returns the drawn ids as a fifth array,
        [S, num_neg] int32 in draw order (-1 for a section without positives)."""
        if sampled is not None:
            S, args, keep_s = self._sampled_call(users, feedback, lines, candidates, sampled, pos_ptr, pos_item, ban_ptr, ban_item)
            n = int(keep_s[2][-1]) if S else 0
            position, tied = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
            ranked, nan = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.int32)
            neg = np.full((max(S, 1), max(args[-2], 1)), -1, np.int32) if return_negatives else None
            self._ok(self.lib.svdf_rank_eval_positions_sampled(self.h, S, *args, position, tied, ranked, nan, _opt_ptr(neg)))
            out = (position[:n], tied[:n], ranked[:S], nan[:S])
            return out + (neg[:S],) if return_negatives else out
        if return_negatives:
            raise SvdfError("rank_eval: return_negatives needs sampled=(num_neg, seed)")
        if candidates is not None:
            S, who_ptr, cand, keep_c = self._cand_call("rank_eval", users, feedback, lines, candidates, ban_ptr)
            pos_ptr, pos_item = _pad(pos_ptr, np.int64), _pad(pos_item, np.uint32)
            if len(pos_ptr) != S + 1:
                raise SvdfError("rank_eval: pos_ptr must have one entry more than users")
            n = int(pos_ptr[-1]) if S else 0
            position, tied = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
            ranked, nan = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.int32)
            self._ok(self.lib.svdf_rank_eval_positions_cand(self.h, S, *who_ptr, pos_ptr, pos_item, cand[0], cand[1], position, tied, ranked, nan))
            return position[:n], tied[:n], ranked[:S], nan[:S]
        if lines is not None:
            S, ul, keep_ul = self._user_lines("rank_eval", users, lines)
            users = np.zeros(S, np.uint32)
        users, pos_ptr, pos_item, ban_ptr, ban_item = self._rank_lists(users, pos_ptr, pos_item, ban_ptr, ban_item)
        S, n = len(users), int(pos_ptr[-1]) if len(users) else 0
        position, tied = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        ranked, nan = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.int32)
        if lines is not None:
            fb, keep = self._feedback_lists("rank_eval", feedback or (None, None, None), S)
            self._ok(self.lib.svdf_rank_eval_positions_lines(self.h, S, ul[0], ul[1], ul[2], fb[0], fb[1], fb[2], pos_ptr, pos_item, _opt_ptr(ban_ptr),
                                                             _opt_ptr(ban_item), position, tied, ranked, nan))
        elif feedback is None:
            self._ok(self.lib.svdf_rank_eval_positions(self.h, S, _pad(users, np.uint32), pos_ptr, pos_item, _opt_ptr(ban_ptr), _opt_ptr(ban_item),
                                                       position, tied, ranked, nan))
        else:
            fb, keep = self._feedback_lists("rank_eval", feedback, S)
            self._ok(self.lib.svdf_rank_eval_positions_fb(self.h, S, _pad(users, np.uint32), fb[0], fb[1], fb[2], pos_ptr, pos_item, _opt_ptr(ban_ptr),
                                                          _opt_ptr(ban_item), position, tied, ranked, nan))
        return position[:n], tied[:n], ranked[:S], nan[:S]

    def rank_eval(self, users, pos_ptr, pos_item, ban_ptr=None, ban_item=None, at=(1, 5, 10, 100), feedback=None, lines=None, candidates=None,
                  sampled=None):
        """svdf_rank_eval: positions on the GPU, then the reference's metrics of them on the host; a dict (see RankMetrics.as_dict).
        feedback, lines, candidates, sampled: as in rank_positions (svdf_rank_eval_fb, svdf_rank_eval_lines, svdf_rank_eval_cand,
        svdf_rank_eval_sampled)."""
        if sampled is not None:
            S, args, keep_s = self._sampled_call(users, feedback, lines, candidates, sampled, pos_ptr, pos_item, ban_ptr, ban_item)
            m = RankMetrics()
            self._ok(self.lib.svdf_rank_eval_sampled(self.h, S, *args, len(at), _pad(list(at), np.int32), C.byref(m)))
            return m.as_dict()
        if candidates is not None:
            S, who_ptr, cand, keep_c = self._cand_call("rank_eval", users, feedback, lines, candidates, ban_ptr)
            pos_ptr, pos_item = _pad(pos_ptr, np.int64), _pad(pos_item, np.uint32)
            if len(pos_ptr) != S + 1:
                raise SvdfError("rank_eval: pos_ptr must have one entry more than users")
            m = RankMetrics()
            self._ok(self.lib.svdf_rank_eval_cand(self.h, S, *who_ptr, pos_ptr, pos_item, cand[0], cand[1], len(at), _pad(list(at), np.int32), C.byref(m)))
            return m.as_dict()
        if lines is not None:
            S, ul, keep_ul = self._user_lines("rank_eval", users, lines)
            users = np.zeros(S, np.uint32)
        users, pos_ptr, pos_item, ban_ptr, ban_item = self._rank_lists(users, pos_ptr, pos_item, ban_ptr, ban_item)
        m = RankMetrics()
        if lines is not None:
            fb, keep = self._feedback_lists("rank_eval", feedback or (None, None, None), len(users))
            self._ok(self.lib.svdf_rank_eval_lines(self.h, len(users), ul[0], ul[1], ul[2], fb[0], fb[1], fb[2], pos_ptr, pos_item, _opt_ptr(ban_ptr),
                                                   _opt_ptr(ban_item), len(at), _pad(list(at), np.int32), C.byref(m)))
        elif feedback is None:
            self._ok(self.lib.svdf_rank_eval(self.h, len(users), _pad(users, np.uint32), pos_ptr, pos_item, _opt_ptr(ban_ptr), _opt_ptr(ban_item),
                                             len(at), _pad(list(at), np.int32), C.byref(m)))
        else:
            fb, keep = self._feedback_lists("rank_eval", feedback, len(users))
            self._ok(self.lib.svdf_rank_eval_fb(self.h, len(users), _pad(users, np.uint32), fb[0], fb[1], fb[2], pos_ptr, pos_item, _opt_ptr(ban_ptr),
                                                _opt_ptr(ban_item), len(at), _pad(list(at), np.int32), C.byref(m)))
        return m.as_dict()

    def rank_topn(self, users, top_n, ban_ptr=None, ban_item=None, feedback=None, lines=None, candidates=None):
        """svdf_rank_topn: the top_n best items per section among all items that are not banned, higher score first and equal
        scores by ascending id; (items [S, top_n] int32, -1 beyond count; scores [S, top_n] float32; count [S]; nan [S]).  feedback = (fb_ptr,
        fb_index, fb_value): the sections' feedback lists, for user-group trainers (svdf_rank_topn_fb).  lines = (ul_ptr, ul_index,
        ul_value): the sections bring USER lines and the trainer may have side tables (svdf_rank_topn_lines); users is None then.
        candidates = (cand_ptr, cand_item): the top_n best of each section's own item list (svdf_rank_topn_cand); ban_ptr must
        be None."""
        if candidates is not None:
            S, who_ptr, cand, keep_c = self._cand_call("rank_topn", users, feedback, lines, candidates, ban_ptr)
            top_n = int(top_n)
            n = max(top_n, 1)
            items, scores = np.full((max(S, 1), n), -1, np.int32), np.zeros((max(S, 1), n), np.float32)
            count, nan = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.int32)
            self._ok(self.lib.svdf_rank_topn_cand(self.h, S, *who_ptr, cand[0], cand[1], top_n, items.reshape(-1), scores.ctypes.data_as(C.c_void_p),
                                                  count, nan))
            return items[:S], scores[:S], count[:S], nan[:S]
        if lines is not None:
            S, ul, keep_ul = self._user_lines("rank_topn", users, lines)
            users = np.zeros(S, np.uint32)
        users, top_n = np.ascontiguousarray(users, np.uint32), int(top_n)
        S = len(users)
        if ban_ptr is not None:
            ban_ptr, ban_item = _pad(ban_ptr, np.int64), _pad(ban_item if ban_item is not None else [], np.uint32)
            if len(ban_ptr) != S + 1:
                raise SvdfError("rank_topn: ban_ptr must have one entry more than users")
        else:
            ban_item = None
        n = max(top_n, 1)
        items, scores = np.full((max(S, 1), n), -1, np.int32), np.zeros((max(S, 1), n), np.float32)
        count, nan = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.int32)
        if lines is not None:
            fb, keep = self._feedback_lists("rank_topn", feedback or (None, None, None), S)
            self._ok(self.lib.svdf_rank_topn_lines(self.h, S, ul[0], ul[1], ul[2], fb[0], fb[1], fb[2], _opt_ptr(ban_ptr), _opt_ptr(ban_item), top_n,
                                                   items.reshape(-1), scores.ctypes.data_as(C.c_void_p), count, nan))
        elif feedback is None:
            self._ok(self.lib.svdf_rank_topn(self.h, S, _pad(users, np.uint32), _opt_ptr(ban_ptr), _opt_ptr(ban_item), top_n, items.reshape(-1),
                                             scores.ctypes.data_as(C.c_void_p), count, nan))
        else:
            fb, keep = self._feedback_lists("rank_topn", feedback, S)
            self._ok(self.lib.svdf_rank_topn_fb(self.h, S, _pad(users, np.uint32), fb[0], fb[1], fb[2], _opt_ptr(ban_ptr), _opt_ptr(ban_item), top_n,
                                                items.reshape(-1), scores.ctypes.data_as(C.c_void_p), count, nan))
        return items[:S], scores[:S], count[:S], nan[:S]

    def similar_items(self, items, top_n, metric="cosine", ban_ptr=None, ban_item=None):
        """svdf_item_topn: per query item the top_n items most like it on the live model, by the dot product or the cosine of
        the W_item rows in the pinned float32 order; the query itself and the section's banned items are excluded.  items = None: every item
        in id order.  metric: "dot", "cosine" or the integers 0 / 1.  Returns (items [S, top_n] int32, -1 beyond count; scores [S, top_n]
        float32; count [S]; nan [S]) as rank_topn does."""
        if items is None:
            shape = (C.c_int(), C.c_int())
            self._ok(self.lib.svdf_view_shape(self.h, VIEW["W_item"], C.byref(shape[0]), C.byref(shape[1])))
            items = np.arange(max(shape[0].value, 0), dtype=np.uint32)
        items, top_n = np.ascontiguousarray(items, np.uint32).reshape(-1), int(top_n)
        if isinstance(metric, str):
            if metric not in ITEM_METRICS:
                raise SvdfError("item_topn: metric must be \"dot\", \"cosine\", 0 or 1")
            metric = ITEM_METRICS[metric]
        S = len(items)
        if ban_ptr is not None:
            ban_ptr, ban_item = _pad(ban_ptr, np.int64), _pad(ban_item if ban_item is not None else [], np.uint32)
            if len(ban_ptr) != S + 1:
                raise SvdfError("item_topn: ban_ptr must have one entry more than items")
        else:
            ban_item = None
        n = max(top_n, 1)
        out, scores = np.full((max(S, 1), n), -1, np.int32), np.zeros((max(S, 1), n), np.float32)
        count, nan = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.int32)
        self._ok(self.lib.svdf_item_topn(self.h, S, _pad(items, np.uint32), int(metric), _opt_ptr(ban_ptr), _opt_ptr(ban_item), top_n, out.reshape(-1),
                                         scores.ctypes.data_as(C.c_void_p), count, nan))
        return out[:S], scores[:S], count[:S], nan[:S]

    # -- multi-GPU item-side delta
    def item_delta_begin(self):
        self._ok(self.lib.svdf_item_delta_begin(self.h))

    def item_delta_buffer(self):
        """(device pointer, float count) of the packed item-side delta."""
        n = C.c_int64()
        p = self.lib.svdf_item_delta_buffer(self.h, C.byref(n))
        if not p:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return p, n.value

    def item_delta_apply(self):
        self._ok(self.lib.svdf_item_delta_apply(self.h))

    def item_delta_export(self, device_ptr):
        self._ok(self.lib.svdf_item_delta_export(self.h, C.c_void_p(device_ptr)))

    def item_delta_count(self):
        """number of elements of the packed item-side delta"""
        n = C.c_int64()
        self._ok(self.lib.svdf_item_delta_pack(self.h, None, 0, C.byref(n)))
        return n.value

    def item_delta_select(self, part, nparts):
        self._ok(self.lib.svdf_item_delta_select(self.h, int(part), int(nparts)))

    def item_delta_pack(self, device_ptr, half=False):
        n = C.c_int64()
        self._ok(self.lib.svdf_item_delta_pack(self.h, C.c_void_p(device_ptr), 1 if half else 0, C.byref(n)))
        return n.value

    def item_delta_unpack(self, device_ptr, half=False, refresh_snapshot=True):
        self._ok(self.lib.svdf_item_delta_unpack(self.h, C.c_void_p(device_ptr), 1 if half else 0, 1 if refresh_snapshot else 0))

    def item_delta_into(self, device_ptr):
        n = C.c_int64()
        self._ok(self.lib.svdf_item_delta_into(self.h, C.c_void_p(device_ptr), C.byref(n)))
        return n.value

    def item_delta_apply_from(self, device_ptr):
        self._ok(self.lib.svdf_item_delta_apply_from(self.h, C.c_void_p(device_ptr)))

    def set_stream(self, hip_stream):
        self._ok(self.lib.svdf_set_stream(self.h, C.c_void_p(hip_stream)))

    def item_delta_import(self, device_ptr):
        self._ok(self.lib.svdf_item_delta_import(self.h, C.c_void_p(device_ptr)))

    # -- introspection
    def view(self, name):
        rows, cols = C.c_int(), C.c_int()
        self._ok(self.lib.svdf_view_shape(self.h, VIEW[name], C.byref(rows), C.byref(cols)))
        if rows.value < 0:
            return None
        out = np.zeros(max(rows.value * cols.value, 1), dtype=np.float32)
        n = self.lib.svdf_get_view(self.h, VIEW[name], out, out.size)
        if n < 0:
            raise SvdfError(self.lib.svdf_last_error().decode())
        out = out[:n]
        return out.reshape(rows.value, cols.value) if name.startswith("W_") else out

    def set_view(self, name, values):
        v = np.ascontiguousarray(values, np.float32).ravel()
        if self.lib.svdf_set_view(self.h, VIEW[name], _pad(v, np.float32), v.size) < 0:
            raise SvdfError(self.lib.svdf_last_error().decode() or "set_view: shape mismatch")

    def synchronize(self):
        self._ok(self.lib.svdf_synchronize(self.h))

    def stream(self):
        return self.lib.svdf_stream(self.h)

    def counter(self, what):
        return int(self.lib.svdf_counter(self.h, what))

    def set_knob(self, name, value):
        self._ok(self.lib.svdf_set_knob(self.h, name.encode(), int(value)))

    def rank_geometry(self, kind, units, top_n=1, pos_ptr=None):
        """svdf_rank_geometry, a test probe that needs no device: the launch geometry of rank_positions (kind "positions": `units` row tiles, or
        with pos_ptr `units` sections with those positives) or of rank_topn (kind "topn": `units` sections, top_n) on this trainer, from the
        functions the launches use.  A dict: gy, items_per_block, cap, tile_rows, rows, tiles, sections, launches."""
        out = (C.c_long * 8)()
        ptr = None
        if pos_ptr is not None:
            ptr = np.ascontiguousarray(pos_ptr, np.int64)
            if len(ptr) != units + 1:
                raise SvdfError("rank_geometry: pos_ptr must have one entry more than sections")
        self._ok(self.lib.svdf_rank_geometry(self.h, {"positions": 0, "topn": 1}[kind], int(units), int(top_n), _opt_ptr(ptr), out))
        return dict(zip(("gy", "items_per_block", "cap", "tile_rows", "rows", "tiles", "sections", "launches"), (int(v) for v in out)))

    LEVEL_FORMS = (None, "basic_fast", "basic_unit", "basic_values", "basic_slots8", "basic_slots16", "fused", "fused_hot", "fewrow_fast", "fewrow_slots16")
    LEVEL_KNOBS = ("groups_per_wave", "block_threads", "xcd_remap", "load_mode", "store_mode")

    def level_geometry(self, launcher, n, max_nu=1, max_ni=1, unit_values=True, has_globals=False):
        """svdf_level_geometry, a test probe that needs no device: what one conflict-free level of n instances would be launched as on this
        trainer by launch_basicmf (launcher "basic") or launch_fused (launcher "fewrow", with the few-row shape max_nu, max_ni), from the
        functions the launchers use.  A dict: form (a name of LEVEL_FORMS), lane_class, lanes, chunks, full, groups, block, nu, ni, per_set,
        per_block, grid_work, grid, remap, load, store, knobs (the names of the tuning knobs the launch reads), lds, chain, chain_cap."""
        out = (C.c_long * 20)()
        self._ok(self.lib.svdf_level_geometry(self.h, {"basic": 0, "fewrow": 1}[launcher], int(n), int(max_nu), int(max_ni), int(bool(unit_values)),
                                              int(bool(has_globals)), out))
        g = dict(zip(("form", "lane_class", "lanes", "chunks", "full", "groups", "block", "nu", "ni", "per_set", "per_block", "grid_work", "grid", "remap",
                      "load", "store", "knobs", "lds", "chain", "chain_cap"), (int(v) for v in out)))
        g["form"] = self.LEVEL_FORMS[g["form"]]
        g["knobs"] = tuple(name for b, name in enumerate(self.LEVEL_KNOBS) if g["knobs"] >> b & 1)
        return g


_libc.fwrite.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
_libc.fread.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]


class Ranker:
    """ISVDRanker over the HIP engine (apex_svd.h:160-197; SVDFeatureRanker apex_svd_base.h:597-813)."""

    def __init__(self, format_type=0, active_type=0, extend_type=0, variant_type=0, device=-1):
        self.lib = load_library()
        self.h = self.lib.svdf_ranker_create(format_type, active_type, extend_type, variant_type, device)
        if not self.h:
            raise SvdfError(self.lib.svdf_last_error().decode())
        self.cap = 16
        self.top_k = 0

    def close(self):
        if self.h:
            self.lib.svdf_ranker_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ok(self, rc):
        if rc < 0:
            raise SvdfError(self.lib.svdf_last_error().decode())
        return rc

    def set_param(self, name, val):
        self._ok(self.lib.svdf_ranker_set_param(self.h, str(name).encode(), str(val).encode()))
        if str(name) == "top_k":
            self.top_k = int(val)

    def load_model(self, path, with_type_header=True):
        fi = _libc.fopen(str(path).encode(), b"rb")
        if not fi:
            raise SvdfError("cannot open %s" % path)
        try:
            if with_type_header:
                buf = C.create_string_buffer(4)
                _libc.fread(buf, 1, 4, C.c_void_p(fi))
            self._ok(self.lib.svdf_ranker_load_model(self.h, fi))
        finally:
            _libc.fclose(fi)

    def init_ranker(self, num_item_set):
        self.cap = max(16, int(num_item_set) + 16)
        self._ok(self.lib.svdf_ranker_init(self.h, int(num_item_set)))

    @staticmethod
    def _taken(out, n, cap):
        """the native calls return the number of results of the line(s) and write at most `cap` of them: more than the buffer
        holds is an error here, never a silent truncation"""
        if n > cap:
            raise SvdfError("ranker: the call produced %d results, the result buffer holds %d (several PROCESS lines in one call?)" % (n, cap))
        return out[:n].copy()

    def process(self, label, ng, nu, ni, index, value):
        out = np.zeros(self.cap, np.int32)
        n = self._ok(self.lib.svdf_ranker_process_csr(self.h, float(label), ng, nu, ni, _pad(index, np.uint32), _pad(value, np.float32), out, self.cap))
        return self._taken(out, n, self.cap)

    def process_rows(self, d):
        """every row of a CSRData through process() in ONE native call (svdf_ranker_process_rows: sections pipelined on the
        device); returns the concatenated results"""
        lab = np.asarray(d.row_label)
        nproc = int(np.count_nonzero(lab == 4.0))
        rp = np.asarray(d.row_ptr, np.int64)
        npos = int(((rp[2::3] - rp[1:-1:3])[lab == 1.0]).sum()) if d.num_row else 0   # ids listed by the POS_SAMPLE lines
        per = self.top_k if self.top_k > 0 else self.counter(2) + npos
        cap = max(16, nproc * per + 16)
        out = np.zeros(cap, np.int32)
        n = self._ok(self.lib.svdf_ranker_process_rows(self.h, d.num_row, _pad(d.row_label, np.float32), _pad(d.row_ptr, np.int32),
                                                       _pad(d.feat_index, np.uint32), _pad(d.feat_value, np.float32), out, cap))
        return self._taken(out, n, cap)

    def process_block(self, b):
        d = b.data
        cap = self.cap * max(1, d.num_row)
        out = np.zeros(cap, np.int32)
        n = self._ok(self.lib.svdf_ranker_process_block(self.h, b.num_ufeedback, b.extend_tag, _pad(b.index_ufeedback, np.uint32),
                                                        _pad(b.value_ufeedback, np.float32), d.num_row, _pad(d.row_label, np.float32),
                                                        _pad(d.row_ptr, np.int32), _pad(d.feat_index, np.uint32), _pad(d.feat_value, np.float32),
                                                        out, cap))
        return self._taken(out, n, cap)

    def counter(self, what):
        return int(self.lib.svdf_ranker_counter(self.h, what))
