"""The rule that orders the rows of a SHUFFLED pass of rank pairs (include/svdfeature_amd.h), in numpy uint64 -- written from
the published statement, not from the C++ (helper of tests/test_pair_order.py and tests/test_gpu_pair_order.py; not collected).  G and mix are
section 6ab's (rank_negs_rule).

    SALT_ORDER = 0x706169726F726472                                   ("pairordr")
    K_i  = mix((order_seed ^ SALT_ORDER) + (i + 1) * G)               i = 0 .. 3
    b    = the smallest integer >= 2 with 2^b >= n
    E(x): wl = b // 2, wr = b - wl;  L = x >> wr;  R = x & (2^wr - 1)
          for i = 0 .. 3:  f = mix(K_i + (R + 1) * G) >> (64 - wl);   (L, R) = (R, L ^ f);   swap(wl, wr)
          return (L << wr) | R
    sigma(p): x = p;  repeat x = E(x) until x < n                     at least one application, at most WALKS = 128

Position p of a shuffled pass holds source row sigma(p); the pass is the plain / hard / weighted pass on (user[sigma], pos[sigma])."""
import numpy as np

from rank_negs_rule import G, U64, mix

SALT_ORDER = U64(0x706169726F726472)
WALKS = 128


def keys(order_seed):
    """K_0 .. K_3: uint64[4]"""
    with np.errstate(over="ignore"):
        return mix((U64(int(order_seed) & 0xFFFFFFFFFFFFFFFF) ^ SALT_ORDER) + (np.arange(4, dtype=U64) + U64(1)) * G)


def bits(n):
    b = 2
    while (1 << b) < n:
        b += 1
    return b


def E(K, b, x):
    """one application of the network to a uint64 array of values below 2^b"""
    x = np.asarray(x, U64)
    wl = b // 2
    wr = b - wl
    L, R = x >> U64(wr), x & U64((1 << wr) - 1)
    for i in range(4):
        with np.errstate(over="ignore"):
            f = mix(K[i] + (R + U64(1)) * G) >> U64(64 - wl)
        L, R = R, L ^ f
        wl, wr = wr, wl
    return (L << U64(wr)) | R


def sigma(n, order_seed, walks=WALKS, return_steps=False):
    """uint32[n]: what svdf_pair_order returns (and, on request, the applications every position took).  Round t applies E to every
    position still outside [0, n)."""
    K, b = keys(order_seed), bits(n)
    x = np.arange(n, dtype=U64)
    steps = np.zeros(n, np.int64)
    out = np.arange(n)
    for t in range(1, walks + 1):
        x[out] = E(K, b, x[out])
        steps[out] = t
        out = out[x[out] >= U64(n)]
        if len(out) == 0:
            break
    assert len(out) == 0, "order_seed %d needs more than %d steps at position %d" % (order_seed, walks, int(out[0]))
    return (x.astype(np.uint32), steps) if return_steps else x.astype(np.uint32)


def sigma_scalar(n, order_seed):
    """the same in Python integers, position by position: a second statement for the small sizes"""
    M = (1 << 64) - 1
    g = int(G)

    def mix1(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    K = [mix1((((int(order_seed) & M) ^ int(SALT_ORDER)) + (i + 1) * g) & M) for i in range(4)]
    b = bits(n)
    out = []
    for p in range(n):
        x = p
        for _ in range(WALKS):
            wl = b // 2
            wr = b - wl
            L, R = x >> wr, x & ((1 << wr) - 1)
            for i in range(4):
                f = mix1((K[i] + (R + 1) * g) & M) >> (64 - wl)
                L, R = R, L ^ f
                wl, wr = wr, wl
            x = (L << wr) | R
            if x < n:
                break
        else:
            raise AssertionError("position %d" % p)
        out.append(x)
    return np.array(out, np.uint32)


def same(user, order):
    """adjacent positions of the permuted order that share their user"""
    u = np.asarray(user)[np.asarray(order, np.int64)]
    return int((u[1:] == u[:-1]).sum())


NU, NI = 300, 1200


def rows(order, n=3000, seed=5):
    """n positives of 300 users x 1 200 items with repeated (user, item) rows, "grouped" by user or "shuffled"; users 0 and 1 have no row"""
    rng = np.random.default_rng(seed)
    u = rng.integers(2, NU, n)
    p = rng.integers(0, NI, n)
    again = rng.random(n) < 0.15
    again[0] = False
    src = rng.integers(0, np.maximum(np.arange(n), 1))
    u[again], p[again] = u[src[again]], p[src[again]]
    if order == "grouped":
        at = np.argsort(u, kind="stable")
        u, p = u[at], p[at]
    return u.astype(np.uint32), p.astype(np.uint32)


def rows_with_same_at(n, order, positions, seed=9):
    """source rows whose PERMUTED order (user[order], pos[order]) has position p sharing its user with position p - 1 exactly for p in
    `positions`: distinct users everywhere else (n <= NU - 2)"""
    assert n <= NU - 2
    hit = np.zeros(n, bool)
    hit[np.asarray(sorted(positions), np.int64)] = True
    assert not hit[0]
    u_perm = 2 + np.cumsum(~hit) - 1            # a new user wherever the position does not repeat the one before
    p_perm = np.random.default_rng(seed).integers(0, NI, n)
    u, p = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    u[np.asarray(order, np.int64)] = u_perm
    p[np.asarray(order, np.int64)] = p_perm
    return u, p


def grouped_rows(n=4000, num_user=300, num_item=1200, seed=11):
    """n positives grouped by user (ascending user ids, about n / num_user rows each), items at random with repeats"""
    rng = np.random.default_rng(seed)
    user = np.sort(rng.integers(0, num_user, n)).astype(np.uint32)
    pos = rng.integers(0, num_item, n).astype(np.uint32)
    return user, pos
