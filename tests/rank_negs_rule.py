"""The rule that draws a section's negatives for sampled-negative ranking (include/svdfeature_amd.h), in numpy uint64 -- written
from the published statement, not from the C++: splitmix64 seeded per section from a splitmix64 of the seed, mapped onto an id by multiply-high.

    G         = 0x9E3779B97F4A7C15
    mix(z)    : z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
    stream_s  = mix(seed + (s + 1) * G)
    draw(s,t) = (uint32)(((mix(stream_s + (t + 1) * G) >> 32) * num_item) >> 32)

The negatives of section s are the first num_neg ids of draw(s, 0), draw(s, 1), ... that are neither excluded (the section's bans and
positives) nor earlier in the sequence, in the order of the sequence."""
import numpy as np

U64 = np.uint64
G = U64(0x9E3779B97F4A7C15)


def mix(z):
    """splitmix64's output function on a uint64 array (numpy's unsigned arithmetic wraps mod 2^64)"""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def stream(seed, s):
    with np.errstate(over="ignore"):
        return mix(U64(seed) + (np.asarray(s, U64) + U64(1)) * G)


def draws(seed, s, t, num_item):
    """draw(s, t) for an array of t (or an array of s and one t): ids below num_item"""
    with np.errstate(over="ignore"):
        z = mix(stream(seed, s) + (np.asarray(t, U64) + U64(1)) * G)
    return (((z >> U64(32)) * U64(num_item)) >> U64(32)).astype(np.int64)


def section_negatives(seed, s, num_item, num_neg, excluded=()):
    """(the negatives of section s in draw order, the number of draws taken)"""
    seen = set(int(x) for x in excluded)
    out, t0 = [], 0
    while True:
        for j, d in enumerate(draws(seed, s, np.arange(t0, t0 + 256), num_item).tolist()):
            if d in seen:
                continue
            seen.add(d)
            out.append(d)
            if len(out) == num_neg:
                return np.array(out, np.int32), t0 + j + 1
        t0 += 256


def rule_negatives(num_item, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, seed):
    """[S, num_neg] int32: what svdf_rank_negatives returns -- a row of -1 for a section without positives"""
    S = len(pos_ptr) - 1
    out = np.full((S, num_neg), -1, np.int32)
    for s in range(S):
        pos = pos_item[pos_ptr[s]:pos_ptr[s + 1]]
        if len(pos) == 0:
            continue
        ban = ban_item[ban_ptr[s]:ban_ptr[s + 1]] if ban_ptr is not None else ()
        out[s] = section_negatives(seed, s, num_item, num_neg, list(pos) + list(ban))[0]
    return out
