"""The case matrix and the exact reference of the per-job unique-colour stage (csrc/k1_unique.hip) and of K2 (rhccq_cluster_sums /
rhccq_cluster_means in csrc/k7_kmeans.hip).

numpy only, seeded, no GPU and no import of the package's device code.  The reference works in plain integers, one job at a time, by
boolean mask: it restates what the entry points are documented to produce (include/rhccq.h), not how the kernels get there.
tests/test_job_cases_cpu.py checks it against the oracle (O.segment_crop + O.unique_colors) and proves that the matrix reaches what it
claims to reach; tests/test_gpu_job_kernels.py compares every kernel output with it bit for bit.

A case is: an image uint8[H,W,3], per class a label map int32[H,W] (0 = no job, l > 0 = job job_base[c] + l - 1) or None (every pixel
is job job_base[c]), job_base and n_jobs."""
import functools
from types import SimpleNamespace

import numpy as np

INT_MAX = 2 ** 31 - 1
BITMAP_WORDS = 1 << 19               # 2^24 bits per job
CHUNK_WORDS = 1024                   # words per block of rhccq_bitmap_count / rhccq_bitmap_emit
CHUNKS = BITMAP_WORDS // CHUNK_WORDS
NO_BEST = np.uint64(0xFFFFFFFFFFFFFFFF)
STAT_SLOTS = 64                      # kStatSlots: LDS slots of a block's statistics table
GRID_STRIDE_PIXELS = 2048 * 256 * 4  # above this many pixels the streaming kernels loop

# first and last bit of a bitmap word, both sides of the 1 024-word chunk boundary, the last bit of the bitmap
REQUIRED = [(0, 0, 1), (0, 0, 31), (0, 0, 32), (0, 127, 255), (0, 128, 0), (255, 255, 255)]
# three colours of norm 1: the black fix has to decide between DIFFERENT colours by raster position
NORM1 = [(0, 0, 1), (0, 1, 0), (1, 0, 0)]


def pack(img):
    a = np.asarray(img, np.uint8).reshape(-1, 3).astype(np.uint32)
    return (a[:, 0] << 16) | (a[:, 1] << 8) | a[:, 2]


# ---- label layouts -----------------------------------------------------------------------------------------------------------------
def grid(H, W, rng, ty, tx):
    """synth.grid_labels-style rectangles, ids ascending in tile raster order"""
    th, tw = -(-H // ty), -(-W // tx)
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy // th) * tx + xx // tw + 1).astype(np.int32), ty * tx


def stripes(H, W, rng, J):
    """label = x mod J + 1: the job changes at every pixel"""
    return np.broadcast_to((np.arange(W) % J + 1).astype(np.int32), (H, W)).copy(), J


def blobs(H, W, rng, n, drop=()):
    """nearest of n seeded points (Voronoi cells); the ids in `drop` are removed, so that absent jobs exist"""
    pts = np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2
    lab = (np.argmin(d, axis=2) + 1).astype(np.int32)
    for i in drop:
        lab[lab == i] = 0
    return lab, n


_LAYOUTS = {"grid": grid, "stripes": stripes, "blobs": blobs}


def _holes(lab, rng, frac):
    if frac > 0:
        lab = lab.copy()
        lab[rng.random(lab.shape) < frac] = 0
    return lab


# ---- the matrix --------------------------------------------------------------------------------------------------------------------
# (name, H, W, classes, options).  A class is None (`whole`) or (layout, args, fraction of its pixels set to 0).
# options: gap = job ids between class 0 and class 1 that no class addresses; seed (chosen so that the counts asserted in
# tests/test_job_cases_cpu.py hold: overlapping and uncovered pixels of multi-class cases, job kinds over the matrix);
# paths: "bitmap" (byte-flag and bit-atomics scans, bitmap passes, index and remap kernels, sort path) or "stats" (bit-atomics scan and
# rhccq_job_stats only: 2 MiB of bitmap per job is all such a case allocates).
_SPECS = [
    # H*W of at most one quad plus a tail
    ("q1x1_whole", 1, 1, [None], {}),
    ("q1x3_stripes2", 1, 3, [("stripes", (2,), 0.0)], {}),
    ("q2x2_whole", 2, 2, [None], {}),
    ("q1x5_stripes3", 1, 5, [("stripes", (3,), 0.0)], {}),
    # W < 4: a quad spans 2 to 4 rows
    ("w13x1_c2", 13, 1, [("blobs", (3,), 0.3), ("blobs", (2,), 0.35)], {"seed": 5}),
    ("w5x2_blobs", 5, 2, [("blobs", (3,), 0.1)], {}),
    ("w7x3_c2", 7, 3, [("blobs", (3,), 0.3), ("grid", (2, 1), 0.35)], {"seed": 2}),
    # H*W mod 4 = 1, 2, 3: the scalar tail, and int4 accesses of class c >= 1 that are not 16-byte aligned
    ("t5x13_c4", 5, 13, [("blobs", (3, (2,)), 0.3), ("grid", (1, 2), 0.3), ("stripes", (2,), 0.5), ("blobs", (2,), 0.4)], {"seed": 2}),
    ("t6x11_c2_gap", 6, 11, [("blobs", (4, (3,)), 0.25), ("grid", (2, 2), 0.3)], {"gap": 3, "seed": 0}),
    ("t9x7_c4", 9, 7, [("blobs", (3,), 0.3), ("grid", (2, 1), 0.35), ("blobs", (2,), 0.4), ("stripes", (2,), 0.5)], {"seed": 0}),
    # aligned
    ("a16x16_whole", 16, 16, [None], {}),
    ("a16x16_c2_pow2", 16, 16, [("grid", (2, 2), 0.25), ("blobs", (4,), 0.3)], {"seed": 0}),
    ("a16x16_grid", 16, 16, [("grid", (3, 3), 0.0)], {}),
    # two blocks of the scans: 80 jobs in each overflow the 64-slot statistics table, 64 fill it exactly
    ("s64x80_stripes80", 64, 80, [("stripes", (80,), 0.0)], {"paths": "stats"}),
    ("s64x80_stripes64", 64, 80, [("stripes", (64,), 0.0)], {"paths": "stats"}),
    # three blocks, block boundaries inside rows
    ("b67x131_c2", 67, 131, [("blobs", (12, (5, 9)), 0.2), ("blobs", (7, (2,)), 0.3)], {"seed": 0}),
    # just above the grid-stride limit of the streaming kernels, H*W mod 4 = 3
    ("g1449x1451_c2", 1449, 1451, [("grid", (2, 2), 0.2), ("grid", (1, 2), 0.3)], {"seed": 0}),
]
BIG = "g1449x1451_c2"


def names(paths=None):
    return [s[0] for s in _SPECS if paths is None or s[4].get("paths", "bitmap") == paths]


def is_whole(cs):
    return len(cs.labels) == 1 and cs.labels[0] is None


def small_names(paths=None):
    return [n for n in names(paths) if n != BIG]


def _stable_seed(name, seed):
    return [sum(ord(ch) * (i + 1) for i, ch in enumerate(name)), seed]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace(name, H, W, img uint8[H,W,3], labels [int32[H,W] or None], job_base [int], n_seg [int], n_jobs, paths)"""
    _, H, W, classes, opt = next(s for s in _SPECS if s[0] == name)
    rng = np.random.default_rng(_stable_seed(name, opt.get("seed", 0)))
    labels, n_seg = [], []
    for cl in classes:
        if cl is None:
            labels.append(None)
            n_seg.append(1)
        else:
            lab, n = _LAYOUTS[cl[0]](H, W, rng, *cl[1])
            labels.append(_holes(lab, rng, cl[2]))
            n_seg.append(n)
    job_base, nxt = [], 0
    for c, n in enumerate(n_seg):
        job_base.append(nxt)
        nxt += n + (opt.get("gap", 0) if c == 0 and len(n_seg) > 1 else 0)
    # the image: a palette of a few dozen colours, black scattered at about 15 %
    pal = np.array(REQUIRED + NORM1[1:] + [tuple(v) for v in rng.integers(0, 256, (26, 3))], np.uint8)
    img = pal[rng.integers(0, len(pal), (H, W))]
    img[rng.random((H, W)) < 0.15] = 0
    # one job entirely black, one job cleared of black: both of the class with the most present jobs (its jobs are disjoint), and
    # only where a third job stays as drawn
    present = [np.unique(l[l > 0]) if l is not None else np.array([1]) for l in labels]
    c = int(np.argmax([len(p) for p in present]))
    if len(present[c]) >= 3:
        img[labels[c] == present[c][-1]] = 0
        m = (labels[c] == present[c][0]) & np.all(img == 0, axis=2)
        img[m] = pal[rng.integers(0, len(pal), int(m.sum()))]
    # the six boundary colours, placed (not left to the draw) wherever six pixels are free for them: spread over the pixels that some
    # class covers, outside the all-black job
    free = np.zeros((H, W), bool)
    for l in labels:
        free |= True if l is None else (l > 0)
    if len(present[c]) >= 3:
        free &= labels[c] != present[c][-1]
    spots = np.nonzero(free.reshape(-1))[0]
    placed = len(spots) >= len(REQUIRED)
    if placed:
        pick = spots[np.linspace(0, len(spots) - 1, len(REQUIRED)).round().astype(np.int64)]
        img.reshape(-1, 3)[pick] = np.array(REQUIRED, np.uint8)
    for l in labels:
        if l is not None:
            l.setflags(write=False)
    img.setflags(write=False)
    return SimpleNamespace(name=name, H=H, W=W, img=img, labels=labels, job_base=job_base, n_seg=n_seg, n_jobs=nxt,
                           paths=opt.get("paths", "bitmap"), required_placed=placed)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def job_masks(cs):
    """[(job, class, flat bool mask)] of every job a class addresses, in job order"""
    out = []
    for c, lab in enumerate(cs.labels):
        for l in range(1, cs.n_seg[c] + 1):
            m = np.ones(cs.H * cs.W, bool) if lab is None else (lab.reshape(-1) == l)
            out.append((cs.job_base[c] + l - 1, c, m))
    return out


def class_box(cs, c):
    """(r0, c0, r1 + 1, c1 + 1) of the pixels class c covers: the region a crop is clamped to"""
    lab = cs.labels[c]
    if lab is None:
        return 0, 0, cs.H, cs.W
    rows, cols = np.nonzero(lab > 0)
    if len(rows) == 0:
        return 0, 0, cs.H, cs.W
    return int(rows.min()), int(cols.min()), int(rows.max()) + 1, int(cols.max()) + 1


def stats(cs):
    """int64[n_jobs, 6] = {min_r, max_r, min_c, max_c, count, n_black}; {INT_MAX, -1, INT_MAX, -1, 0, 0} for a job with no pixel"""
    st = np.tile(np.array([INT_MAX, -1, INT_MAX, -1, 0, 0], np.int64), (cs.n_jobs, 1))
    keys = pack(cs.img)
    for j, _, m in job_masks(cs):
        p = np.nonzero(m)[0]
        if len(p):
            r, c = p // cs.W, p % cs.W
            st[j] = [r.min(), r.max(), c.min(), c.max(), len(p), int((keys[p] == 0).sum())]
    return st


def derive(cs, st):
    """present, has_bg, needs_fix, all_black (bool[n_jobs]) and the crops (r0, r1, c0, c1), as FrameEncoder.prepare derives them"""
    job_class = np.zeros(cs.n_jobs, np.int64)
    for j, c, _ in job_masks(cs):
        job_class[j] = c
    rb = np.array([class_box(cs, c) for c in job_class], np.int64)
    count, n_black = st[:, 4], st[:, 5]
    present = count > 0
    r0 = np.maximum(rb[:, 0], st[:, 0] - 2)
    r1 = np.minimum(rb[:, 2] - 1, st[:, 1] + 2)
    c0 = np.maximum(rb[:, 1], st[:, 2] - 2)
    c1 = np.minimum(rb[:, 3] - 1, st[:, 3] + 2)
    area = (r1 - r0 + 1) * (c1 - c0 + 1)
    return SimpleNamespace(present=present, has_bg=present & (area > count), needs_fix=present & (n_black > 0) & (count > n_black),
                           all_black=present & (n_black > 0) & (count == n_black), crop=(r0, r1, c0, c1), job_class=job_class)


def colour_sets(cs, black_is_colour):
    """per job the sorted distinct colours of its pixels (np.unique order), black among them only when black_is_colour"""
    keys = pack(cs.img)
    out = [np.zeros(0, np.uint32) for _ in range(cs.n_jobs)]
    for j, _, m in job_masks(cs):
        k = keys[m]
        out[j] = np.unique(k if black_is_colour else k[k != 0])
    return out


def with_black(sets, jobs):
    """the sets after rhccq_job_set_black on `jobs`"""
    out = list(sets)
    for j in jobs:
        out[j] = np.unique(np.concatenate([np.zeros(1, np.uint32), out[j]]))
    return out


def bitmap_words(keys):
    """sorted keys of ONE job -> (word indices, word values) of the words its bitmap sets"""
    w = (keys >> 5).astype(np.int64)
    idx, inv = np.unique(w, return_inverse=True)
    val = np.zeros(len(idx), np.uint32)
    np.bitwise_or.at(val, inv, np.uint32(1) << (keys & 31).astype(np.uint32))
    return idx, val


def chunk_sums(keys):
    """exclusive sums of the 512 chunk counts of one job (what rhccq_bitmap_count leaves in chunk_sums)"""
    cnt = np.bincount((keys >> 15).astype(np.int64), minlength=CHUNKS)
    return (np.cumsum(cnt) - cnt).astype(np.uint32)


def chunk_pairs(keys, chunk):
    """the 1 024 (bitmap word, exclusive prefix) pairs of one chunk of one job -> uint32[1024, 2]"""
    out = np.zeros((CHUNK_WORDS, 2), np.uint32)
    idx, val = bitmap_words(keys)
    sel = (idx // CHUNK_WORDS) == chunk
    out[idx[sel] % CHUNK_WORDS, 0] = val[sel]
    out[:, 1] = np.searchsorted(keys, (np.arange(CHUNK_WORDS, dtype=np.int64) + chunk * CHUNK_WORDS) * 32, "left")
    return out


def best(cs, needs_fix):
    """uint64[n_jobs]: norm2 << 40 | pixel of the in-mask non-black pixel of smallest R^2+G^2+B^2, the lowest raster position on
    ties; ~0 where the job is not flagged or has no such pixel.  Also the number of candidates of that norm, and of distinct colours
    among them."""
    keys = pack(cs.img)
    px = cs.img.reshape(-1, 3).astype(np.int64)
    n2 = (px * px).sum(1)
    out = np.full(cs.n_jobs, NO_BEST, np.uint64)
    ties = np.zeros((cs.n_jobs, 2), np.int64)
    for j, _, m in job_masks(cs):
        p = np.nonzero(m & (keys != 0))[0]
        if needs_fix[j] and len(p):
            lo = n2[p].min()
            cand = p[n2[p] == lo]
            out[j] = np.uint64((int(lo) << 40) | int(cand.min()))
            ties[j] = [len(cand), len(np.unique(keys[cand]))]
    return out, ties


def fix_keys(cs, bst, needs_fix):
    """uint32[n_jobs]: the colour at the black fix's pixel for a flagged job, else 0 (as FrameEncoder.prepare builds fix_key)"""
    keys = pack(cs.img)
    pos = (bst & np.uint64((1 << 40) - 1)).astype(np.int64)
    return np.where(needs_fix & (bst != NO_BEST), keys[np.where(needs_fix & (bst != NO_BEST), pos, 0)], 0).astype(np.uint32)


def palettes(cs, fix_key=None, black_jobs=()):
    """per job the sorted distinct colours after the black fix (in-mask black shows fix_key[job] where that is non-zero), with colour 0
    added for every job of black_jobs: what the sort path emits, and what the bitmap path holds after scan(black_is_colour = 0 with a
    fix, 1 without) + rhccq_job_set_black"""
    keys = pack(cs.img)
    out = [np.zeros(0, np.uint32) for _ in range(cs.n_jobs)]
    for j, _, m in job_masks(cs):
        k = keys[m].copy()
        if fix_key is not None and fix_key[j] != 0:
            k[k == 0] = fix_key[j]
        out[j] = np.unique(k)
    return with_black(out, black_jobs)


def pal_offsets(pals):
    n = np.array([len(p) for p in pals], np.int64)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)          # [n_jobs + 1]


def ranks(cs, pals, fix_key=None):
    """int32[n_class, H*W]: the rank of every pixel's (fixed) colour in its job's palette, -1 where the label is <= 0"""
    keys = pack(cs.img)
    out = np.full((len(cs.labels), cs.H * cs.W), -1, np.int32)
    for j, c, m in job_masks(cs):
        k = keys[m].copy()
        if fix_key is not None and fix_key[j] != 0:
            k[k == 0] = fix_key[j]
        r = np.searchsorted(pals[j], k)
        assert len(k) == 0 or np.array_equal(pals[j][r], k), "a pixel's colour is missing from its job's palette"
        out[c, m] = r
    return out


def entries(cs, rk, pal_off, fp_lut=None):
    """int32[n_class, H*W]: the table entry every pixel shows (pal_off[job] + rank, through fp_lut when given), -1 where no job;
    and first raster position of every entry (INT_MAX where no pixel shows it) -> (entry map, first_pos int32[n_entries])"""
    n_entries = int(pal_off[-1]) if fp_lut is None else int(fp_lut.max()) + 1
    ent = np.full(rk.shape, -1, np.int32)
    fp = np.full(max(n_entries, 1), INT_MAX, np.int32)
    for j, c, m in job_masks(cs):
        e = pal_off[j] + rk[c, m].astype(np.int64)
        if fp_lut is not None:
            e = fp_lut[e].astype(np.int64)
        ent[c, m] = e
        np.minimum.at(fp, e, np.nonzero(m)[0].astype(np.int32))
    return ent, fp


def index_map(cs, rk, pal_off, lut, lut2, default_index):
    """int64[H*W]: the first class (in the order given) whose label is > 0 decides, through lut then lut2; default_index elsewhere"""
    out = np.full(cs.H * cs.W, default_index, np.int64)
    undecided = np.ones(cs.H * cs.W, bool)
    for c in range(len(cs.labels)):
        for j, cj, m in job_masks(cs):
            if cj != c:
                continue
            sel = m & undecided
            v = lut[pal_off[j] + rk[c, sel].astype(np.int64)].astype(np.int64)
            out[sel] = lut2[v] if lut2 is not None else v
        undecided &= ~covered(cs, c)
    return out


def index_map_entries(cs, ent, lut2, default_index):
    """the same rule from stored entries (rhccq_frame_remap_entries)"""
    out = np.full(cs.H * cs.W, default_index, np.int64)
    undecided = np.ones(cs.H * cs.W, bool)
    for c in range(len(cs.labels)):
        sel = covered(cs, c) & undecided
        v = ent[c, sel].astype(np.int64)
        out[sel] = lut2[v] if lut2 is not None else v
        undecided &= ~sel
    return out


def covered(cs, c):
    lab = cs.labels[c]
    return np.ones(cs.H * cs.W, bool) if lab is None else (lab.reshape(-1) > 0)


def sort_outputs(pals):
    """keys_out, job_start (-1 for a job with no colour), n_unique of rhccq_job_sort_unique"""
    off = pal_offsets(pals)
    n = np.diff(off)
    keys = np.concatenate(pals).astype(np.uint32) if len(pals) else np.zeros(0, np.uint32)
    return keys, np.where(n > 0, off[:-1], -1).astype(np.int32), int(off[-1])


# ---- look-up tables of the remap tests: seeded, and the CPU test proves that they tell the classes apart -----------------------------
# seeds of the look-up tables, chosen like the cases' own: a tiny case shows few entries, and the full-width value has to be among them
LUT_SEEDS = {"w13x1_c2": 1}


def luts(name, n_entries, top, with_lut2, seed=None):
    """lut int32[n_entries] (and lut2): values up to `top` (255, 32 767 or INT_MAX: the full width of the output type), about a quarter
    of them `top` itself.  With lut2, lut indexes a 61-entry table and lut2 carries the wide values."""
    seed = LUT_SEEDS.get(name, 0) if seed is None else seed
    rng = np.random.default_rng(_stable_seed(name, 1000 + seed) + [top % 65521, int(with_lut2)])

    def wide(n):
        v = rng.integers(0, top + 1, n, dtype=np.int64)
        v[rng.random(n) < 0.25] = top
        return v.astype(np.int32)
    if with_lut2:
        return rng.integers(0, 61, max(n_entries, 1)).astype(np.int32), wide(61)
    return wide(max(n_entries, 1)), None


def fp_lut(name, n_entries):
    """(job, rank) entries -> a table a third the size: several entries share one"""
    rng = np.random.default_rng(_stable_seed(name, 2000))
    return rng.integers(0, max(1, n_entries // 3), max(n_entries, 1)).astype(np.int32)


# ---- everything of one case, computed once -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name):
    cs = case(name)
    st = stats(cs)
    d = derive(cs, st)
    bst, ties = best(cs, d.needs_fix)
    fk = fix_keys(cs, bst, d.needs_fix)
    black_jobs = np.nonzero(d.has_bg | d.all_black)[0]
    r = SimpleNamespace(case=cs, stats=st, d=d, best=bst, ties=ties, fix_key=fk, black_jobs=black_jobs)
    # (a "stats" case has the whole reference too: only the device tests leave its bitmap passes out, for their memory)
    r.sets = {b: colour_sets(cs, b) for b in (0, 1)}
    # the frame encoder's state: scan without black, black set where the crop shows background, in-mask black recoloured
    r.pal_fix = palettes(cs, fk, black_jobs)
    r.rank_fix = ranks(cs, r.pal_fix, fk)
    # no fix at all: black is a colour like any other
    r.pal_plain = palettes(cs)
    r.rank_plain = ranks(cs, r.pal_plain)
    return r


# ---- which jobs a block of the scan meets ------------------------------------------------------------------------------------------
def scan_blocks(H, W):
    """pixel ranges [(begin, end)] of the blocks of rhccq_job_scan: ceil(quads / grid) quads each, grid = min(2048, ceil(quads / 1024))"""
    n_px = H * W
    quads = (n_px + 3) // 4
    g = max(1, min(2048, (quads + 1023) // 1024))
    per = (quads + g - 1) // g
    return [(b * per * 4, min((b + 1) * per * 4, n_px)) for b in range(g) if b * per * 4 < n_px]


def jobs_per_block(cs):
    out = []
    for lo, hi in scan_blocks(cs.H, cs.W):
        seen = set()
        for j, _, m in job_masks(cs):
            if m[lo:hi].any():
                seen.add(j)
        out.append(len(seen))
    return out


# ---- K2 ------------------------------------------------------------------------------------------------------------------------------
K2_SIZES = (1, 7, 8, 9, 4099)
K2_KINDS = ("runs", "broken", "none", "random")


def k2_case(n, kind, k, seed=0):
    """keys uint32[n], labels int32[n] in [-1, k): sorted runs of equal labels, runs broken by -1, all -1, or random"""
    rng = np.random.default_rng([n, K2_KINDS.index(kind), k, seed])
    keys = rng.integers(0, 1 << 24, n, dtype=np.int64).astype(np.uint32)
    if kind == "none" or k == 0:
        lab = np.full(n, -1, np.int32)
    elif kind == "random":
        lab = rng.integers(-1, k, n).astype(np.int32)
    else:
        lab = np.sort(rng.integers(0, k, n)).astype(np.int32)
        if kind == "broken":
            lab[rng.random(n) < 0.2] = -1
    return keys, lab


def k2_reference(keys, labels, k):
    """sums int64[k, 4] (r, g, b, count) by np.add.at, floor-mean keys uint32[k] (0 for an empty cluster)"""
    sums = np.zeros((max(k, 0), 4), np.int64)
    sel = labels >= 0
    kk = keys[sel].astype(np.int64)
    rows = np.stack([(kk >> 16) & 255, (kk >> 8) & 255, kk & 255, np.ones_like(kk)], 1)
    np.add.at(sums, labels[sel], rows)
    c = np.maximum(sums[:, 3], 1)
    means = np.where(sums[:, 3] > 0, ((sums[:, 0] // c) << 16) | ((sums[:, 1] // c) << 8) | (sums[:, 2] // c), 0).astype(np.uint32)
    return sums, means
