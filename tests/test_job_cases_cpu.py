"""tests/job_cases.py checked without a GPU: its reference equals the oracle (O.segment_crop + O.unique_colors) job by job, and the
matrix reaches what tests/test_gpu_job_kernels.py relies on -- every job kind, overlapping and uncovered pixels that the index map
would show, a black fix decided by position, shared first-position entries, the statistics table full and overflowing, the sort
path's n_jobs at a power of two and one above.  Each property is asserted on the reference alone."""
import numpy as np
import pytest

import job_cases as J
from oracle import rhccq_oracle as O

ORACLE_MAX_PIXELS = 20000
BITMAP = J.small_names("bitmap")


def _oracle_cases():
    """every case but the large one: the two 64 x 80 cases, which the device tests run through the statistics only, included"""
    return [n for n in J.names() if J.case(n).H * J.case(n).W <= ORACLE_MAX_PIXELS]


# ---- the reference against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _oracle_cases())
def test_reference_equals_oracle(name):
    cs, ref = J.case(name), J.reference(name)
    r0, _, c0, _ = ref.d.crop
    seen = 0
    for j, c, m in J.job_masks(cs):
        br0, bc0, br1, bc1 = J.class_box(cs, c)
        region = cs.img[br0:br1, bc0:bc1]
        mask = m.reshape(cs.H, cs.W)[br0:br1, bc0:bc1]
        res = O.segment_crop(region, mask)
        assert (res is None) == (not ref.d.present[j]), (name, j)
        if res is None:
            assert len(ref.pal_fix[j]) == 0 and tuple(ref.stats[j]) == (J.INT_MAX, -1, J.INT_MAX, -1, 0, 0)
            continue
        crop, (cr0, cc0) = res
        assert (cr0 + br0, cc0 + bc0) == (r0[j], c0[j]), (name, j)
        assert crop.shape[:2] == (ref.d.crop[1][j] - r0[j] + 1, ref.d.crop[3][j] - c0[j] + 1), (name, j)
        pal, idx = O.unique_colors(crop)
        assert np.array_equal(O.pack_rgb(pal), ref.pal_fix[j]), (name, j)
        full = m.reshape(cs.H, cs.W)[r0[j]:r0[j] + crop.shape[0], c0[j]:c0[j] + crop.shape[1]]
        want = idx.reshape(crop.shape[:2])[full]
        assert np.array_equal(ref.rank_fix[c].reshape(cs.H, cs.W)[m.reshape(cs.H, cs.W)], want), (name, j)
        seen += 1
    assert seen >= 1


@pytest.mark.parametrize("name", [n for n in _oracle_cases() if J.is_whole(J.case(n))])
def test_whole_equals_unique_colors(name):
    cs, ref = J.case(name), J.reference(name)
    pal, idx = O.unique_colors(cs.img)
    assert np.array_equal(O.pack_rgb(pal), ref.pal_plain[0]) and np.array_equal(idx, ref.rank_plain[0])
    assert np.array_equal(ref.sets[1][0], ref.pal_plain[0])


def test_reference_pieces_agree():
    """bitmap words, chunk sums and (word, prefix) pairs restate the same sorted keys"""
    for name in BITMAP:
        ref = J.reference(name)
        for keys in ref.pal_fix + ref.sets[0]:
            idx, val = J.bitmap_words(keys)
            back = np.concatenate([(w << 5) + np.nonzero((int(v) >> np.arange(32)) & 1)[0] for w, v in zip(idx, val)] or [np.zeros(0)])
            assert np.array_equal(back.astype(np.uint32), keys)
            cs_ = J.chunk_sums(keys)
            for ch in np.unique(keys >> 15):
                pairs = J.chunk_pairs(keys, int(ch))
                assert pairs[0, 1] == cs_[ch]
                rank = pairs[(keys >> 5) % J.CHUNK_WORDS, 1][keys >> 15 == ch]
                low = (np.uint32(1) << (keys & 31)) - np.uint32(1)
                word = pairs[(keys >> 5) % J.CHUNK_WORDS, 0][keys >> 15 == ch]
                pop = np.array([bin(int(w & l)).count("1") for w, l in zip(word, low[keys >> 15 == ch])], np.int64)
                assert np.array_equal(rank + pop, np.nonzero(keys >> 15 == ch)[0])


# ---- no failure may hide -----------------------------------------------------------------------------------------------------------
def test_every_job_kind_occurs():
    n = dict.fromkeys(("needs_fix", "all_black", "has_bg", "no_bg", "absent", "no_black"), 0)
    for name in J.names("bitmap"):
        ref = J.reference(name)
        d = ref.d
        n["needs_fix"] += int(d.needs_fix.sum())
        n["all_black"] += int(d.all_black.sum())
        n["has_bg"] += int(d.has_bg.sum())
        n["no_bg"] += int((d.present & ~d.has_bg).sum())
        n["absent"] += int((~d.present).sum())
        n["no_black"] += int((d.present & (ref.stats[:, 5] == 0)).sum())
    assert min(n.values()) >= 3, n


def test_required_colours_present():
    """both ends of a bitmap word, both sides of the chunk boundary, the last bit of the bitmap: placed, not drawn, in every case that has
    six covered pixels outside its all-black job -- every case from 13 pixels up -- and then in some job's palette and colour set"""
    need = set(int(k) for k in J.pack(np.array(J.REQUIRED, np.uint8)))
    for name in J.names():
        cs, ref = J.case(name), J.reference(name)
        if cs.H * cs.W >= 13:
            assert cs.required_placed, name
        if cs.required_placed:
            assert need <= set(int(k) for k in np.concatenate(ref.pal_fix)), name
            assert need <= set(int(k) for k in np.concatenate(ref.sets[0])), name


@pytest.mark.parametrize("name", [n for n in J.names("bitmap") if len(J.case(n).labels) > 1])
def test_multi_class_cases_overlap_and_leave_holes(name):
    cs, ref = J.case(name), J.reference(name)
    cov = np.stack([J.covered(cs, c) for c in range(len(cs.labels))])
    assert int((cov.sum(0) == 0).sum()) >= 2, name
    off = J.pal_offsets(ref.pal_fix)
    for top in (255, 32767, J.INT_MAX):
        for with_lut2 in (False, True):
            lut, lut2 = J.luts(name, int(off[-1]), top, with_lut2)
            want = J.index_map(cs, ref.rank_fix, off, lut, lut2, 0)
            assert want.max() == top, (name, top, with_lut2)
            # the same pixels decided by the classes in the opposite order
            rev = SimpleReversed(cs)
            other = J.index_map(rev, ref.rank_fix[::-1], off, lut, lut2, 0)
            both = cov.sum(0) >= 2
            assert int((want[both] != other[both]).sum()) >= 5, (name, top, with_lut2)
    # and through stored entries
    fpl = J.fp_lut(name, int(off[-1]))
    ent, _ = J.entries(cs, ref.rank_fix, off, fpl)
    a = J.index_map_entries(cs, ent, None, 0)
    b = J.index_map_entries(SimpleReversed(cs), ent[::-1], None, 0)
    assert int((a != b).sum()) >= 5, name


class SimpleReversed:
    """a case with its classes in the opposite order (same job ids)"""

    def __init__(self, cs):
        self.H, self.W, self.n_jobs = cs.H, cs.W, cs.n_jobs
        self.labels, self.job_base, self.n_seg = cs.labels[::-1], cs.job_base[::-1], cs.n_seg[::-1]


def test_black_fix_decided_by_position():
    tied = distinct = 0
    for name in J.names("bitmap"):
        ref = J.reference(name)
        tied += int((ref.ties[:, 0] >= 2).sum())
        distinct += int((ref.ties[:, 1] >= 2).sum())
        assert np.all(ref.best[~ref.d.needs_fix] == J.NO_BEST) and np.all(ref.best[ref.d.needs_fix] != J.NO_BEST)
        assert np.all((ref.fix_key != 0) == ref.d.needs_fix)
    assert tied >= 1 and distinct >= 1, (tied, distinct)


def test_fp_lut_shares_entries():
    shared = 0
    for name in BITMAP:
        ref = J.reference(name)
        off = J.pal_offsets(ref.pal_fix)
        fpl = J.fp_lut(name, int(off[-1]))
        ent, fp = J.entries(ref.case, ref.rank_fix, off, fpl)
        used = np.unique(np.concatenate([off[j] + np.unique(ref.rank_fix[c][m]) for j, c, m in J.job_masks(ref.case) if m.any()]))
        shared += int((np.bincount(fpl[used]) >= 2).sum())
        assert np.array_equal(fp != J.INT_MAX, np.bincount(ent[ent >= 0], minlength=len(fp)) > 0)
    assert shared >= 1


def test_statistics_table_fills_and_overflows():
    over, full = J.case("s64x80_stripes80"), J.case("s64x80_stripes64")
    assert len(J.scan_blocks(64, 80)) == 2
    assert all(n > J.STAT_SLOTS for n in J.jobs_per_block(over)), J.jobs_per_block(over)
    assert all(n == J.STAT_SLOTS for n in J.jobs_per_block(full)), J.jobs_per_block(full)
    assert len(J.scan_blocks(67, 131)) == 3 and all(lo % 131 for lo, _ in J.scan_blocks(67, 131)[1:])
    # every other case stays inside the table
    for name in J.names("bitmap"):
        assert max(J.jobs_per_block(J.case(name))) <= J.STAT_SLOTS, name


def test_sort_path_job_counts():
    n = [J.case(name).n_jobs for name in J.names("bitmap")]
    assert any(v >= 2 and v & (v - 1) == 0 for v in n), n
    assert any(v >= 3 and (v - 1) & (v - 2) == 0 for v in n), n


def test_shapes_and_limits():
    shapes = {(J.case(n).H, J.case(n).W) for n in J.names()}
    assert {(1, 1), (1, 3), (2, 2), (1, 5), (13, 1), (5, 2), (7, 3), (5, 13), (6, 11), (9, 7), (16, 16), (64, 80), (67, 131),
            (1449, 1451)} <= shapes
    assert {(5 * 13) % 4, (6 * 11) % 4, (9 * 7) % 4} == {1, 2, 3}
    assert sorted(len(J.case(n).labels) for n in J.names() if len(J.case(n).labels) > 1).count(4) >= 1
    assert {1, 2, 4} <= {len(J.case(n).labels) for n in J.names()}
    big = J.case(J.BIG)
    assert big.H * big.W > J.GRID_STRIDE_PIXELS and (big.H * big.W) % 4 == 3 and big.n_jobs <= 6 and len(big.labels) == 2
    assert sum(J.case(n).H * J.case(n).W > ORACLE_MAX_PIXELS for n in J.names()) == 1
    for name in J.names("bitmap"):
        assert J.case(name).n_jobs <= 24, name                         # 22 MiB per job with byte flags
    # a job_base with a gap: job ids that no class addresses
    gap = J.case("t6x11_c2_gap")
    assert gap.job_base[1] > gap.n_seg[0] and gap.n_jobs == sum(gap.n_seg) + gap.job_base[1] - gap.n_seg[0]


@pytest.mark.parametrize("name", J.names())
def test_no_case_is_degenerate(name):
    cs, ref = J.case(name), J.reference(name)
    if not J.is_whole(cs):
        assert int(ref.d.present.sum()) >= 2, name
    if cs.H * cs.W > 1:
        assert max(len(s) for s in ref.sets[1]) >= 2, name


def test_generators_are_seeded_and_repeat():
    for name in J.small_names():
        a = J.case(name)
        J.case.cache_clear()
        b = J.case(name)
        assert a is not b and np.array_equal(a.img, b.img) and a.job_base == b.job_base
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a.labels, b.labels))
    assert np.array_equal(J.luts("x", 40, 255, True)[1], J.luts("x", 40, 255, True)[1])
    assert np.array_equal(J.fp_lut("x", 40), J.fp_lut("x", 40))
    for n in J.K2_SIZES:
        for kind in J.K2_KINDS:
            k0, l0 = J.k2_case(n, kind, 5)
            k1, l1 = J.k2_case(n, kind, 5)
            assert np.array_equal(k0, k1) and np.array_equal(l0, l1) and l0.min() >= -1 and l0.max() < 5


def test_k2_cases_reach_their_paths():
    """runs of equal labels inside a thread's 8 points, runs broken by -1, a padded tail, empty clusters"""
    for n in J.K2_SIZES:
        _, lab = J.k2_case(n, "runs", 3)
        assert np.all(np.diff(lab) >= 0)
    assert {n % 8 for n in J.K2_SIZES} >= {0, 1, 7, 3}
    _, lab = J.k2_case(4099, "runs", 3)
    assert (np.diff(lab.reshape(-1)[:4096].reshape(-1, 8), axis=1) != 0).any() and (np.diff(lab[:4096].reshape(-1, 8), axis=1) == 0).all(1).any()
    _, lab = J.k2_case(4099, "broken", 3)
    assert (lab == -1).any() and (lab >= 0).any()
    keys, lab = J.k2_case(9, "runs", 40)
    sums, means = J.k2_reference(keys, lab, 40)
    assert (sums[:, 3] == 0).any() and np.all(means[sums[:, 3] == 0] == 0) and sums[:, 3].sum() == 9
