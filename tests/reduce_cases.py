"""Shared cases of the palette reduction tests (tests/test_palette_reduce_cpu.py, tests/test_gpu_palette_reduce.py): a plain helper
module, not a conftest.

`reduce_reference` is the numpy statement of rhccq_palette_reduce (include/rhccq.h): clusters of weight n, integer sums S and integer
centre c; the pair a < b of least cost n_a n_b D / (n_a + n_b) merges, ties to the smallest a, then the smallest b; the merged centre
is (2 S + n) // (2 n).  Costs are compared with Python integers (cross-multiplied); float64 only picks a shortlist of candidates
within 1e-9 relative of the smallest float cost (the float cost is off by a few 1e-16 relative, and 0.0 exactly when D = 0), among
which the integers decide.  It is written twice: `naive=True` evaluates every live pair in every step, the fast form keeps each row's
nearest partner of higher id and repairs that table after a merge.  `reference` asserts the two equal, merge list included, on every
case of at most 300 rows; larger cases are served by the fast form alone.  Every case's reference is computed once per process and
shared (do not modify what `case` and `reference` return)."""
import functools

import numpy as np

import remap_cases as RM
from roibasedimagecompression_amd import ops

E_ARG, E_LIMIT = RM.E_ARG, RM.E_LIMIT
CAP = ops.palette_reduce_max_rows()   # the largest palette of the device form
BLOCK = 1024                          # lanes of the resident workgroup (kReduceBlock, csrc/palette_reduce.hip): rows per pass of its loops
MAX_SUM = 2 ** 32 - 1
NAIVE_MAX_K = 300
REL = 1e-9
H29 = 2 ** 29


class _State:
    def __init__(self, palette, counts):
        self.n = [int(v) for v in counts]
        self.c = np.array(palette, np.int64).reshape(-1, 3)
        self.S = [[n * int(v) for v in row] for n, row in zip(self.n, self.c)]
        self.nf = np.array(self.n, np.float64)
        self.merges = []

    def exact(self, a, b):
        """(numerator, denominator) of cost(a, b) as Python integers"""
        d = int(((self.c[a] - self.c[b]) ** 2).sum())
        return self.n[a] * self.n[b] * d, self.n[a] + self.n[b]

    def approx(self, a, b):
        """float64 costs of the pairs (a[i], b[i])"""
        d = ((self.c[a] - self.c[b]) ** 2).sum(axis=-1).astype(np.float64)
        return self.nf[a] * self.nf[b] * d / (self.nf[a] + self.nf[b])

    def first_min(self, a, b):
        """the index i of the exactly smallest cost(a[i], b[i]), the first such: the pairs are listed in the order ties go"""
        f = self.approx(a, b)
        lo = f.min()
        if lo == 0.0:                                     # D = 0, exactly
            return int(np.argmax(f == 0.0))
        short = np.nonzero(f <= lo * (1.0 + REL))[0]
        best, key = int(short[0]), self.exact(int(a[short[0]]), int(b[short[0]]))
        for i in short[1:]:
            k = self.exact(int(a[i]), int(b[i]))
            if k[0] * key[1] < key[0] * k[1]:
                best, key = int(i), k
        return best

    def merge(self, a, b):
        assert a < b and self.n[a] > 0 and self.n[b] > 0
        self.n[a] += self.n[b]
        self.S[a] = [x + y for x, y in zip(self.S[a], self.S[b])]
        self.c[a] = [(2 * s + self.n[a]) // (2 * self.n[a]) for s in self.S[a]]
        self.n[b] = 0
        self.nf[a], self.nf[b] = self.n[a], 0.0
        self.merges.append((a, b))


def _run_naive(st, live, steps):
    live = list(live)
    for _ in range(steps):
        ids = np.array(live, np.int64)
        ia, ib = np.triu_indices(len(ids), 1)             # row-major: ascending a, then ascending b
        a, b = ids[ia], ids[ib]
        i = st.first_min(a, b)
        st.merge(int(a[i]), int(b[i]))
        live.remove(int(b[i]))


def _run_fast(st, live, steps):
    K = len(st.n)
    alive = np.zeros(K, bool)
    alive[live] = True
    nn = np.full(K, -1, np.int64)

    def scan(r):
        s = np.nonzero(alive[r + 1:])[0] + r + 1
        nn[r] = s[st.first_min(np.full(len(s), r, np.int64), s)] if len(s) else -1

    for r in live:
        scan(r)
    for _ in range(steps):
        rows = np.nonzero(alive & (nn >= 0))[0]
        a = int(rows[st.first_min(rows, nn[rows])])       # the lowest row among those of least cost to their partner
        b = int(nn[a])
        st.merge(a, b)
        alive[b] = False
        nn[b] = -1
        again = np.nonzero(alive & ((nn == a) | (nn == b)))[0]
        other = np.nonzero(alive[:a] & (nn[:a] != a) & (nn[:a] != b))[0]
        for r in list(again) + [a]:
            scan(int(r))
        if len(other):                                    # the moved a against the partner the row has
            fa, fp = st.approx(other, np.full(len(other), a, np.int64)), st.approx(other, nn[other])
            nn[other[fa < fp * (1.0 - REL)]] = a
            for r in other[(fa >= fp * (1.0 - REL)) & (fa <= fp * (1.0 + REL))]:
                ka, kp = st.exact(int(r), a), st.exact(int(r), int(nn[r]))
                x, y = ka[0] * kp[1], kp[0] * ka[1]
                if x < y or (x == y and a < nn[r]):
                    nn[r] = a


def reduce_reference(palette, counts, k_target, naive=False):
    """-> (palette uint8[k_target, 3], counts int64[k_target], map int32[K], merges int32[K - 1, 2], k_out)"""
    palette = np.asarray(palette, np.uint8).reshape(-1, 3)
    K = len(palette)
    st = _State(palette, counts)
    assert len(st.n) == K and 1 <= k_target <= K and 0 < sum(st.n) <= MAX_SUM and min(st.n) >= 0
    live = [j for j in range(K) if st.n[j] > 0]
    steps = max(0, len(live) - k_target)
    (_run_naive if naive else _run_fast)(st, live, steps)
    parent = np.arange(K)
    for a, b in st.merges:
        parent[b] = a
    out = [j for j in live if st.n[j] > 0]
    row = {j: i for i, j in enumerate(out)}
    map_ = np.full(K, -1, np.int32)
    for j in live:
        r = j
        while parent[r] != r:
            r = parent[r]
        map_[j] = row[r]
    pal_out, cnt_out = np.zeros((k_target, 3), np.uint8), np.zeros(k_target, np.int64)
    pal_out[:len(out)] = st.c[out]
    cnt_out[:len(out)] = [st.n[j] for j in out]
    merges = np.full((K - 1, 2), -1, np.int32)
    merges[:steps] = np.array(st.merges, np.int32).reshape(-1, 2)
    assert len(out) == min(k_target, len(live))
    return pal_out, cnt_out, map_, merges, len(out)


def _case(pal, counts, target, merges=None, palette=None):
    """merges: the expected (a, b) of the steps, literally; palette: the expected live rows of the result"""
    pal = np.asarray(pal, np.uint8)
    if pal.ndim == 1:                                     # one channel, by hand
        pal = np.stack([pal, np.zeros_like(pal), np.zeros_like(pal)], axis=1)
    return {"pal": pal, "counts": np.asarray(counts, np.uint64), "target": int(target), "merges": merges, "palette": palette}


def _build():
    rng = np.random.default_rng(20261019)
    out = {}
    # row counts around the kernel's widths: a wave, the block of the one-pass loops, the workgroup, the cap (cap + 1: host only)
    for K in sorted({1, 2, 3, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, CAP - 1, CAP, CAP + 1}):
        pal = RM._palette(rng, K, levels=256 if K % 2 else 6)           # even K: 216 colours at most, so duplicates and equal costs
        counts = rng.integers(1, 40, K)
        if K >= 8:
            counts[[0, K // 2, K - 1]] = 0                               # three empty rows: K - 3 live ones
        out[f"K{K}"] = _case(pal, counts, 1 if K <= NAIVE_MAX_K else K - 7)     # the large ones: K - 3 live rows to K - 7, 4 steps
    # 200 steps that each move a centre (no duplicate rows to speak of) at the workgroup's width and below the cap
    for K in (BLOCK - 1, BLOCK, BLOCK + 1, CAP - 1):
        out[f"K{K}_distinct"] = _case(RM._palette(rng, K), 1 + rng.integers(0, 1000, K), K - 200)
    out["cap_to_half"] = _case(out[f"K{CAP}"]["pal"], out[f"K{CAP}"]["counts"], CAP // 2)
    # the cap without duplicate-heavy rows: a few hundred steps that each move a centre
    out["cap_distinct"] = _case(RM._palette(rng, CAP), 1 + rng.integers(0, 1000, CAP), CAP - 300)
    # a photograph's palette with its histogram, as encode_with_palette(colours=N) meets it
    out["K300_to_16"] = _case(RM._palette(rng, 300), rng.integers(1, 5000, 300), 16)
    # ties that need exact arithmetic: 1 * 1 * 4 / 2 = 2 * 2 * 2 / 4 = 2, the lower a wins whichever pair it is
    near, far = [[0, 0, 0], [2, 0, 0]], [[100, 0, 0], [101, 1, 0]]
    out["tie_equal_rationals"] = _case(near + far, [1, 1, 2, 2], 2, merges=[(0, 1), (2, 3)])
    out["tie_equal_rationals_swapped"] = _case(far + near, [2, 2, 1, 1], 2, merges=[(0, 1), (2, 3)])
    # 2^29 * 2^29 / 2^30 against (2^29 + 1)(2^29 - 1) / 2^30 = (2^58 - 1) / 2^30: float64 sees a tie, the second is smaller
    h = H29
    out["tie_numerators_differ_by_one"] = _case([0, 1, 100, 101], [h, h, h + 1, h - 1], 3, merges=[(2, 3)])
    out["tie_numerators_differ_by_one_swapped"] = _case([100, 101, 0, 1], [h + 1, h - 1, h, h], 3, merges=[(0, 1)])
    # repair paths, one channel.  (a) row 1's partner 2 dies (into the heavy row 0, which costs row 1 more than row 3 does): it must
    # scan again and find row 3, and that pair is the next merge
    out["repair_partner_dies"] = _case([0, 50, 1, 110], [100, 1, 1, 1], 1, merges=[(0, 2), (1, 3), (0, 1)])
    # (b) row 0 is below a = 1; its partner 2 dies into a, and its best partner becomes the moved a (at 81, weight 2)
    out["repair_partner_becomes_a"] = _case([100, 80, 82, 130], [1, 1, 1, 1], 1, merges=[(1, 2), (0, 1), (0, 3)])
    # (c) row 0's partner is a = 1 at cost 50; a takes the heavy row 2 and then costs 11 * 121 / 12 = 110.9: the old second best,
    # row 3 at 72, wins
    out["repair_cost_to_a_rises"] = _case([100, 90, 89, 112], [1, 1, 10, 1], 1, merges=[(1, 2), (0, 3), (0, 1)])
    # rounding: halves up; sums past 2^32 (2^24 * 509)
    out["round_half_up"] = _case([10, 11], [1, 1], 1, merges=[(0, 1)], palette=[[11, 0, 0]])
    out["round_down"] = _case([10, 10, 11], [1, 1, 1], 1, merges=[(0, 1), (0, 2)], palette=[[10, 0, 0]])
    out["sums_past_2_32"] = _case([[255, 255, 255], [255, 255, 254]], [2 ** 24, 2 ** 24], 1, merges=[(0, 1)], palette=[[255, 255, 255]])
    # edge inputs
    pal9 = RM._palette(rng, 9)
    out["empties_front_middle_end"] = _case(pal9, [0, 0, 5, 1, 0, 0, 7, 2, 0], 2)
    out["all_weight_in_one_row"] = _case(pal9[:5], [0, 0, 7, 0, 0], 1)
    out["target_is_K_only_empties_go"] = _case(pal9, [3, 0, 5, 1, 0, 4, 7, 2, 0], 9)
    out["target_above_non_empty"] = _case(pal9, [3, 0, 5, 1, 0, 4, 7, 2, 0], 8)
    out["one_row_of_three_kept"] = _case(pal9[:5], [0, 0, 7, 0, 0], 3)
    out["largest_sum"] = _case([0, 255, 7], [MAX_SUM - 2, 1, 1], 1, palette=[[0, 0, 0]])
    return out


_CASES = None


def names(device=False):
    """device: only the cases the device form takes (K <= CAP)"""
    global _CASES
    if _CASES is None:
        _CASES = _build()
        for c in _CASES.values():
            c["pal"].setflags(write=False)
            c["counts"].setflags(write=False)
    return [k for k, c in _CASES.items() if not device or len(c["pal"]) <= CAP]


def case(name):
    names()
    return _CASES[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    ref = reduce_reference(c["pal"], c["counts"], c["target"])
    pal, cnt, map_, merges, k = ref
    if len(c["pal"]) <= NAIVE_MAX_K:
        for x, y in zip(ref, reduce_reference(c["pal"], c["counts"], c["target"], naive=True)):
            assert np.array_equal(x, y), name
    if c["merges"] is not None:
        assert merges[:len(c["merges"])].tolist() == [list(m) for m in c["merges"]], (name, merges.tolist())
        assert (merges[len(c["merges"]):] == -1).all(), name
    if c["palette"] is not None:
        assert pal[:k].tolist() == c["palette"], (name, pal.tolist())
    steps = int((merges[:, 0] >= 0).sum())
    if len(c["pal"]) > NAIVE_MAX_K:                       # the large cases do run the merge chain
        assert steps == (4 if name.startswith("K") and "_" not in name else len(c["pal"]) - c["target"]
                         - int((c["counts"] == 0).sum())) and steps >= 4, (name, steps)
    if name == "sums_past_2_32":
        assert 2 ** 24 * 509 > 2 ** 32 and cnt.tolist() == [2 ** 25]
    if name.startswith("tie_numerators"):
        assert float(H29 * H29) == float((H29 + 1) * (H29 - 1)) and H29 * H29 > (H29 + 1) * (H29 - 1)
    if name == "target_above_non_empty":
        assert k == 6 and not pal[6:].any() and not cnt[6:].any()
    for a in ref[:4]:
        a.setflags(write=False)
    return ref


# the argument errors of rhccq_palette_reduce: (what, overrides of a valid call, return code, where).  A valid call: K = 3, counts
# (1, 2, 3), K_target = 2, every buffer given.  A buffer name set to None passes NULL; "misalign": the named buffer is passed one byte
# (8-byte buffers) or two bytes (4-byte buffers) off; "work_short": work_bytes is one less than asked for; "counts": other weights.
# where: "both", "device" (the device form only) or "data": the counts alone show it, so the host form returns the code and the device
# form, which does not read them on the host, returns 0 and writes the code to *k_out.
ERRORS = [
    ("null palette", {"palette": None}, E_ARG, "both"),
    ("null counts", {"counts_buf": None}, E_ARG, "both"),
    ("null palette_out", {"palette_out": None}, E_ARG, "both"),
    ("null counts_out", {"counts_out": None}, E_ARG, "both"),
    ("null map", {"map": None}, E_ARG, "both"),
    ("null k_out", {"k_out": None}, E_ARG, "both"),
    ("null work", {"work": None}, E_ARG, "device"),
    ("K = 0", {"K": 0}, E_ARG, "both"),
    ("K < 0", {"K": -5}, E_ARG, "both"),
    ("K_target = 0", {"K_target": 0}, E_ARG, "both"),
    ("K_target < 0", {"K_target": -1}, E_ARG, "both"),
    ("K_target = K + 1", {"K_target": 4}, E_ARG, "both"),
    ("misaligned counts", {"misalign": "counts_buf"}, E_ARG, "both"),
    ("misaligned counts_out", {"misalign": "counts_out"}, E_ARG, "both"),
    ("misaligned map", {"misalign": "map"}, E_ARG, "both"),
    ("misaligned merges", {"misalign": "merges"}, E_ARG, "both"),
    ("misaligned k_out", {"misalign": "k_out"}, E_ARG, "both"),
    ("misaligned work", {"misalign": "work"}, E_ARG, "device"),
    ("short workspace", {"work_short": True}, E_ARG, "device"),
    ("K = 65537", {"K": 65537, "K_target": 2}, E_LIMIT, "both"),
    ("K = cap + 1", {"K": CAP + 1, "K_target": 2}, E_LIMIT, "device"),
    ("every count zero", {"counts": [0, 0, 0]}, E_ARG, "data"),
    ("counts add up to 2^32", {"counts": [1, MAX_SUM - 1, 1]}, E_LIMIT, "data"),
    ("one count of 2^32", {"counts": [0, 2 ** 32, 0]}, E_LIMIT, "data"),
    ("one count of 2^64 - 1", {"counts": [1, 2 ** 64 - 1, 1]}, E_LIMIT, "data"),
]
# calls that differ from the valid one and succeed
ACCEPTED = [
    ("the valid call", {}),
    ("null merges", {"merges": None}),
    ("counts add up to 2^32 - 1", {"counts": [1, MAX_SUM - 2, 1]}),
    ("K_target = K", {"K_target": 3}),
    ("K_target = 1", {"K_target": 1}),
]
ERROR_K = 3
