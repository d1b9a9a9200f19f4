"""Seeded soft-NMS inputs shared by tests/golden/make_golden_soft_nms.py (run under python3.9, where the reference's cython_nms.pyx
builds) and by the tests that compare the host loop and the HIP kernel with what the reference's own soft_nms returned for them.

Only RandomState draws cast to float32 at once and float32 IEEE +, -, *, /, floor, minimum, maximum after that: the arrays are
bit-identical under numpy 1.26 and 2.2 (the fixture stores a sha256 of every input, checked before use).

An input: n boxes in clusters of 8 near-duplicates (overlaps are the rule), float or integer coordinates, scores either all different
or quantised to eighths (heavy ties: which of several equal scores is "first" is the rule the compaction order decides), in no
particular order -- soft_nms does not ask for sorted lists."""
import hashlib

import numpy as np

W, H = 1024, 512
f32 = np.float32

# lengths around the kernel's chunk of 64 rows, the evaluation's 300 and the kernel's capacity
SIZES = (1, 2, 3, 63, 64, 65, 128, 129, 300, 2048)
METHODS = (0, 1, 2)                                                  # hard, linear, gaussian
PARAMS = ((0.5, 0.3, 0.001), (0.5, 0.5, 0.05), (0.3, 0.3, 0.3))     # (sigma, Nt, threshold)
# the capacity-sized lists go through ONE (method, parameter set): Gaussian rescoring under the high threshold, where rows die a few
# at a time over the whole sweep (the most compactions over the most chunks); with every method they would be most of the fixture's
# bytes and minutes of the host loop's time
BIG, BIG_AT = 2048, (2, 2)

INPUTS = [(n, integer, tied) for n in SIZES for integer in (False, True) for tied in (False, True)]


def name_of(n, integer, tied):
    return "n%d_%s_%s" % (n, "int" if integer else "flt", "tie" if tied else "uni")


def inputs_of(method, pi):
    """the inputs that the fixture holds results of (method, parameter set pi) for, in the fixture's order"""
    return [c for c in INPUTS if c[0] != BIG or (method, pi) == BIG_AT]


def make(n, integer, tied):
    """-> float32 [n, 5] (x1, y1, x2, y2, score)"""
    rs = np.random.RandomState(int(hashlib.sha256(name_of(n, integer, tied).encode()).hexdigest()[:8], 16))
    k = (n + 7) // 8
    u = lambda lo, hi, size: rs.uniform(lo, hi, size).astype(f32)      # noqa: E731
    x1, y1 = u(0, W - 160, k), u(0, H - 120, k)
    w, h = u(24, 150, k), u(20, 110, k)
    base = np.stack([x1, y1, x1 + w, y1 + h], 1)
    b = np.repeat(base, 8, 0)[:n] + u(-10, 10, (n, 4))
    if integer:
        b = np.floor(b)
    b[:, 0] = np.maximum(b[:, 0], f32(0)); b[:, 1] = np.maximum(b[:, 1], f32(0))
    b[:, 2] = np.minimum(np.maximum(b[:, 2], b[:, 0]), f32(W - 1)); b[:, 3] = np.minimum(np.maximum(b[:, 3], b[:, 1]), f32(H - 1))
    if tied:
        s = rs.randint(1, 9, n).astype(f32) / f32(8)
    else:
        s = (rs.permutation(n) + 1).astype(f32) / f32(n + 1)
        assert len(np.unique(s)) == n
    rows = rs.permutation(n)                                            # the clusters' members are spread over the list
    out = np.ascontiguousarray(np.concatenate([b[rows], s[:, None]], 1), dtype=f32)
    assert out.dtype == f32 and out.shape == (n, 5)
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load(path):
    """the fixture -> {(method, pi): [(name, input [n,5], reference boxes [k,5], reference inds [k])]}; every input's digest is
    checked.  The file stores per (method, pi) the counts, indices and FINAL SCORES of all its cases back to back: the generator
    asserts that the reference's returned coordinates are its input's rows at `inds`, bit for bit, so the returned boxes are
    input[inds] with the score column replaced."""
    g = np.load(path)
    made = {}
    for c, d in zip(INPUTS, g["input_sha256"]):
        a = make(*c)
        assert digest(a) == str(d), "seeded input %s differs from the one the fixture was made with" % name_of(*c)
        made[c] = a
    out = {}
    for method in METHODS:
        for pi in range(len(PARAMS)):
            counts, inds, scores = (g["m%d_p%d_%s" % (method, pi, k)] for k in ("counts", "inds", "scores"))
            cases, o = [], 0
            for c, k in zip(inputs_of(method, pi), counts):
                ii = inds[o:o + k].astype(np.int64)
                boxes = made[c][ii]
                boxes[:, 4] = scores[o:o + k]
                cases.append((name_of(*c), made[c], boxes, ii))
                o += k
            assert o == len(inds) == len(scores)
            out[(method, pi)] = cases
    return out
