"""Hand-built soft-NMS inputs at the structural cases the kernel branches on (scda_amd/csrc/soft_nms.hip), shared by
tests/golden/make_golden_soft_nms_edges.py (run under python3.9, where the reference's cython_nms.pyx builds) and by the tests that
compare the host loop and the HIP kernel with what the reference's own soft_nms returned for them.  tests/soft_nms_cases.py holds the
seeded random lists; these are the ones random draws almost never produce.

Every value is an exactly representable float32 (small integers, k / 8, k / 256, powers of two, NaN, +-inf) written down directly:
no random draw and no rounding (three_rows excepted, see there), so the arrays are the same bytes under every numpy (the fixture
stores a sha256 of each, checked before use).  A case: (name, methods it runs for, (sigma, Nt, threshold), float32 [n, 5] rows (x1, y1, x2, y2, score)).

With t = the row selected in an iteration, N the live length and N' = N - (rows that died in it):
  disjoint_n*          no pair has iw > 0: never a rescore, never a compaction; scores in eighths -- "lowest position first" orders them
  all_dead_n*          n identical boxes, method 0: after iteration 0 N' = 1, nothing survives at or above N'
  tail_k* / head_k*    t, 70 far-away survivors (scores in eighths) and k rows that die in iteration 0, standing AFTER the survivors
                       (every dead place is >= N': no move) or BEFORE them (every death is a move and the moved survivors' order
                       decides the later ties); k = 1, 63, 64, 65 fills the dead / survivor lists across a 64-lane ballot chunk
  ov_eq_nt             10 x 10 against its 10 x 5 (ov = 0.5 = Nt: `>` is strict, not rescored) and its 10 x 6 (ov = 0.6: rescored)
  score_eq_thr / _next 0.25 * (1 - 0.5) = 0.125 against threshold 0.125 (`<` is strict: stays) and against the next float32 (dies)
  touching             iw == 0 exactly: never examined, so a score below the threshold survives; iw == 1: examined, weight 1, dies
  inverted             x2 < x1 or y2 < y1: the reference's arithmetic decides (such a row is never touched, as t or as the other)
  nan_* / inf / three  non-finite scores: the reference selects by `maxscore < boxes[pos, 4]` from maxscore = boxes[i, 4], so a NaN
                       at i is selected and a NaN anywhere else is never greater; +-inf order as numbers
                       (no case multiplies an infinite score by the hard rule's weight 0: that forms a NEW NaN, whose sign bit is
                       the processor's choice, not the algorithm's)
  nan_coord_*          a NaN coordinate, in the row that is selected first (methods 0 and 1) and in rows that are selected last; see
                       nan_coord for what the Gaussian rule is kept away from"""
import hashlib

import numpy as np

f32 = np.float32
NAN, INF = float("nan"), float("inf")
ALL = (0, 1, 2)
DEFAULT = (0.5, 0.3, 0.001)                                           # the reference's defaults (sigma, Nt, threshold)


def _rows(rows):
    a = np.array(rows, dtype=np.float64)
    out = np.ascontiguousarray(a.astype(f32))
    finite = np.isfinite(a)
    assert out.shape == (len(rows), 5) and (out.astype(np.float64)[finite] == a[finite]).all(), "a value that float32 does not hold"
    return out


def _cell(k, y0=0):
    """the k-th 10 x 10 box of a grid with 20-pixel pitch: no two of them touch"""
    x, y = 20 * (k % 32), y0 + 20 * (k // 32)
    return [x, y, x + 9, y + 9]


def _eighths(k):
    return ((k * 5 + 3) % 8 + 1) / 8.0


def disjoint(n):
    return _rows([_cell(k) + [_eighths(k)] for k in range(n)])


def all_dead(n):
    """identical boxes, all different scores (n has no factor 7): the best one discards every other"""
    assert n % 7
    return _rows([[0, 0, 9, 9, ((k * 7) % n + 1) / 256.0] for k in range(n)])


SURVIVORS = 70


def one_region(k, head):
    """t = a 100 x 100 box with score 2, k copies of it with score 0.5 (ov = 1: dead under every method at threshold 0.3) and 70
    disjoint survivors far below it, the copies before the survivors (head) or after them"""
    t = [[0, 0, 99, 99, 2.0]]
    dying = [[0, 0, 99, 99, 0.5]] * k
    alive = [_cell(j, 200) + [_eighths(j)] for j in range(SURVIVORS)]
    return _rows(t + (dying + alive if head else alive + dying))


def ov_eq_nt():
    return _rows([[0, 0, 9, 9, 0.875], [0, 0, 9, 4, 0.75], [0, 0, 9, 5, 0.625], [40, 40, 49, 49, 0.5], [40, 40, 49, 44, 0.25]])


def score_eq_thr():
    return _rows([[0, 0, 9, 9, 0.5], [0, 0, 9, 4, 0.25], [30, 0, 39, 9, 0.125], [30, 0, 39, 4, 0.25]])


def touching():
    return _rows([[0, 0, 9, 9, 0.5],
                  [10, 0, 19, 9, 2.0 ** -11],          # iw == 0 against row 0: never examined, stays although below the threshold
                  [0, 10, 9, 19, 2.0 ** -12],          # ih == 0
                  [50, 50, 59, 59, 2.0 ** -14],        # overlaps nothing
                  [-9, 0, 0, 9, 2.0 ** -11],           # iw == 1: examined, weight 1 (ov is small), dies
                  [10, 10, 19, 19, 2.0 ** -13]])       # a corner: iw == 0 and ih == 0


def inverted():
    return _rows([[0, 0, 9, 9, 0.875], [8, 0, 2, 9, 0.75], [0, 8, 9, 2, 1.0], [9, 9, 0, 0, 0.5], [1, 1, 8, 8, 0.625], [5, 0, 4, 9, 0.25],
                  [3, 3, 3, 3, 0.375], [2, 0, 8, 9, 0.125]])


def cluster(n, scores=None):
    """n 21 x 21 boxes in groups of 10 neighbours 4 pixels apart (heavy overlap inside a group, none between groups), all different
    scores k / 256 in no particular order"""
    s = [((k * 37) % 251 + 1) / 256.0 for k in range(n)] if scores is None else scores
    return _rows([[4 * (k % 10) + 100 * (k // 10), 0, 4 * (k % 10) + 100 * (k // 10) + 20, 20, s[k]] for k in range(n)])


def with_scores(n, at):
    a = cluster(n)
    for k, v in at.items():
        a[k, 4] = v
    return a


def infinities():
    """+inf heads a group (selected first, never rescored); -inf and a second +inf overlap their neighbours only mildly (ov <= Nt:
    weight 1 under methods 0 and 1), so no 0 * inf is formed; 1 * -inf is below every threshold"""
    return _rows([[0, 0, 20, 20, 0.5], [4, 0, 24, 20, INF], [8, 0, 28, 20, 0.75], [22, 0, 42, 20, -INF], [100, 0, 120, 20, -INF],
                  [200, 0, 220, 20, 0.25], [216, 0, 236, 20, INF], [300, 0, 320, 20, 0.375], [302, 0, 322, 20, INF],
                  [318, 0, 338, 20, -INF]])


def nan_coord(as_t):
    """as_t: x1 of the row that is selected first is NaN -- the reference's min / max then return the OTHER row's coordinate, so every
    row of its y-band "overlaps" it with a NaN ov, which is not > Nt: weight 1.  Methods 0 and 1 only: the Gaussian weight of a NaN ov
    is a NaN whose SIGN depends on how a processor subtracts and negates a NaN (x - NaN as x + (-NaN), say), not on the algorithm.
    Otherwise: two rows with a NaN coordinate and the two lowest scores, the last one below the threshold.  The reference's min / max
    return the row's NaN, so no selected row ever touches them: they keep their scores and are selected late, when all
    that is left lies outside their own finite x1 / y2 or has a NaN coordinate itself (no NaN weight is formed -- the rules test
    asserts that no returned score is NaN -- so every method runs).  A kernel that drops the NaN (fminf / fmaxf) rescoring them shows as a NaN
    score under the Gaussian rule and as a death of the row below the threshold under the other two"""
    a = cluster(12)
    if as_t:
        a[3, 0], a[3, 4] = NAN, 254 / 256.0                             # the best score of the list: selected first
    else:
        a[7, 2], a[7, 4] = NAN, 2.0 ** -9
        a[2, 1], a[2, 4] = NAN, 2.0 ** -11
    return a


def three_rows():
    """the smallest list on which lanes of the wave disagreed about the maximum; 0.2 and 0.9 are the float32 nearest to them (the one
    place where a decimal is rounded: correctly, by every numpy)"""
    return np.array([[0, 0, 9, 9, 0.2], [100, 100, 109, 109, NAN], [0, 0, 9, 9, 0.9]], dtype=f32)


NEXT_ABOVE_EIGHTH = float(np.nextafter(f32(0.125), f32(1)))

CASES = (
    [("disjoint_n%d" % n, ALL, DEFAULT, disjoint(n)) for n in (64, 65, 129)]
    + [("all_dead_n%d" % n, (0,), DEFAULT, all_dead(n)) for n in (65, 129)]
    + [("%s_k%d" % ("head" if head else "tail", k), ALL, (0.5, 0.3, 0.3), one_region(k, head)) for head in (False, True)
       for k in (1, 63, 64, 65)]
    + [("ov_eq_nt", (0, 1), (0.5, 0.5, 0.001), ov_eq_nt()),
       ("score_eq_thr", ALL, (0.5, 0.3, 0.125), score_eq_thr()),
       ("score_eq_thr_next", ALL, (0.5, 0.3, NEXT_ABOVE_EIGHTH), score_eq_thr()),
       ("touching", ALL, DEFAULT, touching()),
       ("inverted", ALL, DEFAULT, inverted()),
       ("nan_first", ALL, DEFAULT, with_scores(12, {0: NAN})),
       ("nan_middle", ALL, DEFAULT, with_scores(12, {5: NAN})),
       ("nan_last", ALL, DEFAULT, with_scores(12, {11: NAN})),
       ("nan_three", ALL, DEFAULT, with_scores(23, {0: NAN, 9: NAN, 22: NAN})),
       ("nan_beyond_64", ALL, DEFAULT, with_scores(70, {66: NAN})),
       ("nan_first_and_beyond_64", ALL, DEFAULT, with_scores(131, {0: NAN, 64: NAN, 130: NAN})),
       ("infinities", ALL, DEFAULT, infinities()),
       ("nan_coord_in_t", (0, 1), DEFAULT, nan_coord(True)),
       ("nan_coord_in_other", ALL, DEFAULT, nan_coord(False)),
       ("three_rows", ALL, DEFAULT, three_rows())]
)
KEYS = [(name, m) for name, methods, _, _ in CASES for m in methods]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load(path):
    """the fixture -> [(name, method, (sigma, Nt, threshold), input [n,5], reference boxes [k,5], reference inds [k])] in KEYS' order;
    every input's digest is checked.  The file stores counts, indices and the FINAL SCORES' bits of all (case, method) pairs back to
    back: the generator asserts that the reference's returned coordinates are its input's rows at `inds`, bit for bit, so the
    returned boxes are input[inds] with the score column replaced."""
    g = np.load(path)
    assert [str(s) for s in g["keys"]] == ["%s/m%d" % k for k in KEYS], "the fixture was made for another case list"
    by_name = {}
    for (name, _, params, a), d in zip(CASES, g["input_sha256"]):
        assert digest(a) == str(d), "input %s differs from the one the fixture was made with" % name
        by_name[name] = (params, a)
    out, o = [], 0
    for (name, m), k in zip(KEYS, g["counts"]):
        params, a = by_name[name]
        ii = g["inds"][o:o + k].astype(np.int64)
        boxes = a[ii]
        boxes[:, 4] = g["score_bits"][o:o + k].view(f32)
        out.append((name, m, params, a, boxes, ii))
        o += k
    assert o == len(g["inds"]) == len(g["score_bits"])
    return out
