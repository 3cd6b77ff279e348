"""Thin Python wrappers over the C ABI: torch tensors own device memory, kernels run on torch's
current HIP stream.  Names follow the reference's domain: jobs (segments / crops), palettes, keys
(uint32 R<<16|G<<8|B held in int32 tensors), labels, components.

Reference functions served (paths relative to the reference root):
  unique_colors            encoder/compression/clustering.py:4-103   (get_all_unique_colors)
  clustering_params        encoder/compression/clustering.py:108-135
  eps_components           encoder/compression/clustering.py:233-235 (DBSCAN.fit_predict)
  kmeans_split             encoder/compression/clustering.py:720-775 (KMeans.fit_predict)
  minibatch_kmeans         encoder/compression/clustering.py:207-230 (MiniBatchKMeans.fit_predict)
  cluster_means            encoder/compression/clustering.py:304-310,346-355
  remap / decode           encoder/compression/clustering.py:373-377, decoder/.../uncompression.py:209
  merge_firstpos / paint   encoder/compression/merging.py:52-82
"""
import ctypes as C
import math
import os
import threading

import numpy as np
import torch

from . import _lib
from . import _palette_args as A
from ._lib import MbkDraw, MbkProblem, RhccqError

INT_MAX = 2 ** 31 - 1
BITMAP_WORDS = 524288
MINIBATCH_THRESHOLD = 10000          # clustering.py:205


_DRAW_POOL = None


def host_thread_budget():
    """host threads ONE rank may keep busy: the cores this process may use, shared out over the ranks of the node (LOCAL_WORLD_SIZE under
    torch.distributed.run: 8 ranks on one host must not start 8 x (8 draw + 16 lane + 16 class) workers on each other's cores)"""
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        cores = os.cpu_count() or 1
    ranks = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1))
    return max(2, cores // ranks)


def _draw_pool():
    global _DRAW_POOL
    if _DRAW_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _DRAW_POOL = ThreadPoolExecutor(max_workers=min(8, host_thread_budget()), thread_name_prefix="rhccq-draw")
    return _DRAW_POOL


_LANE_POOLS = {}
_pool_lock = threading.Lock()


def lane_pool(kind):
    """Persistent worker threads for the per-problem / per-class pipelines of a frame (one pool per nesting level, so that a
    class pipeline waiting for its problems never occupies the workers those need): handing a task to a parked worker costs
    tens of microseconds, starting a thread per problem and frame cost 0.3-0.8 ms each in front of the k-means++ chains."""
    pool = _LANE_POOLS.get(kind)
    if pool is None:
        with _pool_lock:
            pool = _LANE_POOLS.get(kind)
            if pool is None:
                from concurrent.futures import ThreadPoolExecutor
                # (the workers mostly wait for the GPU: more of them than cores is fine, but not an unbounded multiple per rank)
                pool = _LANE_POOLS[kind] = ThreadPoolExecutor(max_workers=min(16, 2 * host_thread_budget()), thread_name_prefix=f"rhccq-{kind}")
    return pool


def pack_rgb(rgb):
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3).astype(np.uint32)
    return (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]


def unpack_rgb(keys):
    keys = np.asarray(keys).astype(np.uint32)
    return np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], axis=1).astype(np.uint8)


def morton3(keys):
    """24-bit Z-order code of packed colours: bit i of R, G, B -> bits 3i+2, 3i+1, 3i."""
    def spread(v):
        v = v.astype(np.uint32) & np.uint32(0xFF)
        v = (v | (v << np.uint32(16))) & np.uint32(0xFF0000FF)
        v = (v | (v << np.uint32(8))) & np.uint32(0x0F00F00F)
        v = (v | (v << np.uint32(4))) & np.uint32(0xC30C30C3)
        v = (v | (v << np.uint32(2))) & np.uint32(0x49249249)
        return v
    keys = np.asarray(keys).astype(np.uint32)
    return (spread(keys >> np.uint32(16)) << np.uint32(2)) | (spread(keys >> np.uint32(8)) << np.uint32(1)) | spread(keys)


def clustering_params(n_colors, quality):
    """compute_clustering_params through the C ABI (host-only entry point)."""
    lib = _lib.load()
    if quality == 0:
        raise ZeroDivisionError("float division by zero")     # clustering.py:129 behaviour
    eps, mc = C.c_double(), C.c_int64()
    rc = lib.rhccq_params(int(n_colors), float(quality), C.byref(eps), C.byref(mc))
    if rc:
        raise RhccqError(f"rhccq_params failed ({rc})")
    return eps.value, 1, mc.value


def palette_remap_tile():
    """the palette entries Rhccq.palette_remap's kernel stages at a time (the winner is carried from tile to tile)"""
    return int(_lib.load().rhccq_palette_remap_tile())


def palette_refine_lds_rows():
    """the largest palette whose accumulators Rhccq.palette_refine's kernel keeps in LDS (larger ones add to global memory)"""
    return int(_lib.load().rhccq_palette_refine_lds_rows())


def palette_reduce_max_rows():
    """the largest palette Rhccq.palette_reduce takes: the rows whose state one workgroup's LDS holds"""
    return int(_lib.load().rhccq_palette_reduce_max_rows())


def palette_moments_lds_rows(n_classes=0):
    """the largest palette whose moment tables (n_classes + 1 of them) Rhccq.palette_moments' kernel keeps in LDS"""
    return int(_lib.load().rhccq_palette_moments_lds_rows(int(n_classes)))


def palette_runs_tile():
    """(image rows a workgroup of Rhccq.palette_runs walks by default, columns of the tile it stages through LDS)"""
    lib = _lib.load()
    return int(lib.rhccq_palette_runs_rows()), int(lib.rhccq_palette_runs_tile_cols())


RUN_SLACK_MAX = 3 * 255 ** 2          # the largest slack Rhccq.palette_runs takes: no squared distance is larger
RUN_PENALTY_MAX = (1 << 24) - 1       # the largest penalty Rhccq.palette_segment takes


def palette_segment_max_rows():
    """the largest palette Rhccq.palette_segment takes on the device (a wave holds the K states of an image row in registers)"""
    from . import _lib
    return int(_lib.load().rhccq_palette_segment_max_rows())


def palette_segment_tile():
    """columns of a tile of Rhccq.palette_segment's workspace (a state's stay bits over a tile are one dword)"""
    from . import _lib
    return int(_lib.load().rhccq_palette_segment_tile_cols())


DITHER_MAX = 256                      # the largest strength Rhccq.palette_dither takes: Floyd-Steinberg in full


def palette_dither_max_rows():
    """the largest palette Rhccq.palette_dither takes on the device (the packed palette is 32 KiB of LDS)"""
    return int(_lib.load().rhccq_palette_dither_max_rows())


def palette_dither_rows():
    """image rows of a band of Rhccq.palette_dither's wavefront by default (Rhccq.OPT_DITHER_ROWS)"""
    return int(_lib.load().rhccq_palette_dither_rows())


PATTERN_MAX = 256                     # the largest strength Rhccq.palette_pattern takes: the candidates' mean approaches the pixel in full
PATTERN_SIZES = (2, 4, 8)             # the sides of the threshold matrix Rhccq.palette_pattern takes: 4, 16 or 64 candidates a pixel


def palette_pattern_max_rows():
    """the largest palette Rhccq.palette_pattern takes on the device (the packed palette is 32 KiB of LDS)"""
    return int(_lib.load().rhccq_palette_pattern_max_rows())


def palette_build_max_rows():
    """the most colours Rhccq.palette_build returns on the device: the boxes whose state one workgroup's LDS holds"""
    return int(_lib.load().rhccq_palette_build_max_rows())


def palette_cells_granules():
    """(pixels between two pixels of one lane of Rhccq.palette_cells' kernel, pixels a workgroup takes at a time)"""
    lib = _lib.load()
    return int(lib.rhccq_palette_cells_block()), int(lib.rhccq_palette_cells_chunk())


def png_unfilter_band_rows():
    """rows of a band of Rhccq.png_unfilter's wavefront: a one-wave workgroup, a lane a row"""
    return int(_lib.load().rhccq_png_unfilter_band_rows())


def png_unfilter_tile():
    """steps (filter units of a row) of the tile Rhccq.png_unfilter's kernel stages through LDS"""
    return int(_lib.load().rhccq_png_unfilter_tile())


def png_unfilter_granule():
    """filter units a band of Rhccq.png_unfilter fetches from the band above at a time"""
    return int(_lib.load().rhccq_png_unfilter_granule())


def gif_segment_pixels():
    """pixels of a segment of Rhccq.gif_lzw / gif_encode: every segment is one LZW problem, closed by a Clear code"""
    return int(_lib.load().rhccq_gif_segment_pixels())


PNG_STATUS = ("OK", "BAD_SIGNATURE", "BAD_CHUNK", "BAD_HEADER", "UNSUPPORTED", "LIMIT", "BAD_CRC", "BAD_STREAM", "BAD_LENGTH", "BAD_FILTER", "STALLED")


def png_parse(data):
    """rhccq_png_parse_host (host only, a pure function of the bytes) -> (_lib.PngInfo, the chunk table int64[n_chunks, 4]: offset of the
    type field, data length, first CRC piece, offset in the joined IDAT stream or -1)"""
    a = np.frombuffer(data, dtype=np.uint8)
    cap = a.size // 12 + 1
    table = np.zeros((cap, 4), np.int64)
    info, count = _lib.PngInfo(), C.c_int64()
    rc = _lib.load().rhccq_png_parse_host(C.c_void_p(a.ctypes.data if a.size else 0), a.size, C.byref(info), C.c_void_p(table.ctypes.data), cap, C.byref(count))
    if rc:
        raise RhccqError(f"png_parse: rhccq_png_parse_host failed ({rc})")
    return info, table[:count.value]


GIF_READ_STATUS = ("OK", "BAD_SIGNATURE", "TRUNCATED", "BAD_BLOCK", "BAD_HEADER", "BAD_FRAME", "NO_TABLE", "NO_FRAMES", "LIMIT", "BAD_CODE", "BAD_LENGTH")


def gif_read_tile():
    """codes a step of Rhccq.gif_unlzw's lengths and emit launches: a lane a code"""
    return int(_lib.load().rhccq_gif_read_tile())


def gif_read_scan_step():
    """codes a step of Rhccq.gif_unlzw's scan launch tests for Clear and End: a whole number of tiles, a lane one code of each"""
    return int(_lib.load().rhccq_gif_read_scan_step())


def gif_read_threads():
    """threads of a workgroup of Rhccq.gif_unlzw's launches: also the segments a step of its per-frame prefix sums takes"""
    return int(_lib.load().rhccq_gif_read_threads())


def gif_parse(data):
    """rhccq_gif_parse_host (host only, a pure function of the bytes) -> (_lib.GifInfo, a ctypes array of _lib.GifFrame, one an image, the
    sub-block table int64[n_blocks, 4]: offset of the first data byte, length, frame, place in the joined streams)"""
    a = np.frombuffer(data, dtype=np.uint8)
    lib = _lib.load()
    info, nf, nb = _lib.GifInfo(), C.c_int64(), C.c_int64()
    ptr = C.c_void_p(a.ctypes.data if a.size else 0)
    rc = lib.rhccq_gif_parse_host(ptr, a.size, C.byref(info), None, 0, C.byref(nf), None, 0, C.byref(nb))
    if rc:
        raise RhccqError(f"gif_parse: rhccq_gif_parse_host failed ({rc})")
    frames = (_lib.GifFrame * max(nf.value, 1))()
    blocks = np.zeros((max(nb.value, 1), 4), np.int64)
    if info.status == 0:
        lib.rhccq_gif_parse_host(ptr, a.size, C.byref(info), C.cast(frames, C.c_void_p), nf.value, C.byref(nf), C.c_void_p(blocks.ctypes.data), nb.value, C.byref(nb))
    return info, frames, blocks[:nb.value]


def gif_frames_array(frames, n):
    """the first n rows of a ctypes array of _lib.GifFrame as bytes (uint8, what the device copy holds)"""
    return np.frombuffer(C.string_at(C.addressof(frames), n * C.sizeof(_lib.GifFrame)), np.uint8).copy()


PALETTE_CELLS_SHAPE = (4, 32, 32, 32)  # Rhccq.palette_cells' table: planes {N, Sr, Sg, Sb} over the cells (r >> 3, g >> 3, b >> 3)


def psnr_from_sse(sse, n_pixels):
    """calculate_quality_metrics' PSNR (comparison.py:33-37) from a sum of squared errors over n_pixels RGB pixels:
    10 log10(255^2 / (sse / (3 n_pixels))), inf at sse == 0"""
    if sse == 0:
        return float("inf")
    return 10.0 * math.log10(255.0 ** 2 / (float(sse) / (3.0 * float(n_pixels))))


def eps_threshold(eps):
    lib = _lib.load()
    thr, bnd, r2 = C.c_int32(), C.c_int32(), C.c_double()
    rc = lib.rhccq_eps_threshold(float(eps), C.byref(thr), C.byref(bnd), C.byref(r2))
    if rc:
        raise RhccqError(f"rhccq_eps_threshold({eps}) failed ({rc})")
    return thr.value, bnd.value, r2.value


class _StreamBoundLib:
    """The C ABI as seen by one Rhccq: before every entry point that takes the context, the context is re-bound to
    torch's CURRENT stream when that changed (rhccq_ctx_set_stream) -- every buffer of this module is allocated, zeroed
    and freed by torch on the current stream, so the kernels must run there too (a `with torch.cuda.stream(s):` around
    the mirrored API would otherwise race the memsets against kernels on the stream captured at construction)."""

    def __init__(self, lib, owner):
        self._lib, self._owner = lib, owner

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        args = _lib.PROTOTYPES.get(name, (None, []))[1]
        if not args or args[0] is not _lib.c_void_p or name in ("rhccq_ctx_destroy", "rhccq_last_error", "rhccq_ctx_set_stream", "rhccq_stream"):
            setattr(self, name, fn)
            return fn
        owner = self._owner

        def bound(*a):
            owner._bind_stream()
            return fn(*a)
        bound.__name__ = name
        setattr(self, name, bound)
        return bound


class Rhccq:
    """One context per (process, device).  All methods take / return torch CUDA tensors unless a
    name says numpy."""

    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise RhccqError("no HIP device visible: the RHCCQ product path needs an MI355X (there is no CPU fallback)")
        self._raw = _lib.load()
        self.lib = _StreamBoundLib(self._raw, self)
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self._bound = torch.cuda.current_stream(self.device).cuda_stream
        h = C.c_void_p()
        rc = self._raw.rhccq_ctx_create(device, C.c_void_p(self._bound), C.byref(h))
        if rc:
            raise RhccqError(f"rhccq_ctx_create failed ({rc})")
        self.ctx = h

    OPT_INIT_LDS_BLOCKS, OPT_INIT_MAX_ITEMS, OPT_INIT_KERNEL, OPT_INIT_SHARDS, OPT_INIT_CANDS_PER_WAVE, OPT_REASSIGN_LDS = 1, 2, 3, 4, 5, 6
    OPT_REASSIGN_ORDER = 7           # 1 (default): numpy's scalar-quicksort tie order of the capped reassignment; 0: stable (rounds 1-3)
    OPT_FRAME_CHAINS = 8             # rhccq_encode_frame: 1 (default) one launch for the frame's level-1 k-means++ chains; 0: one per problem lane
    OPT_FRAME_LEVEL2 = 9             # rhccq_encode_frame: 1 (default) the level-2 palettes of all classes as one batch on one lane; 0: one per class lane
    OPT_REFINE_LDS_ROWS = 10         # palette_refine: palettes of more rows accumulate in global memory (0 .. palette_refine_lds_rows(), default that)
    OPT_REFINE_MAX_BLOCKS = 11       # palette_refine: at most this many workgroups (0, default: 8 per CU)
    OPT_RUNS_ROWS = 13               # palette_runs: image rows of a workgroup (0, default: palette_runs_tile()[0]; 2, 4 or 8)
    OPT_CHAIN_RELEASE = 12           # rhccq_encode_frame: 1 (default) a level-1 problem goes on when its own chain of the frame's launch ends; 0: when the launch ends
    OPT_DITHER_ROWS = 14             # palette_dither: image rows of a band (0, default: palette_dither_rows(); 4, 8, 16 or 32)
    OPT_KMEANS_WIDE_PAIRS = 15       # kmeans_split: problems of k <= 1024 and at least this many (point, centre) pairs run their Lloyd iterations as launches on many CUs (0: never, 1: all of them)
    OPT_KMEANS_CHUNK = 16            # kmeans_split: Lloyd iterations of the wide path enqueued between two looks at the state records (1 .. 300)
    OPT_GIF_READ_CHAIN = 17          # gif_unlzw / gif_decode: a segment's len / first chains by pointer doubling (0, default) or by one lane's pass in order (1); same results

    def _bind_stream(self):
        """kernels follow torch's current stream (see _StreamBoundLib)"""
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._bound:
            rc = self._raw.rhccq_ctx_set_stream(self.ctx, C.c_void_p(s))
            if rc:
                raise RhccqError(f"rhccq_ctx_set_stream failed ({rc})")
            self._bound = s

    def set_option(self, option, value):
        """rhccq_ctx_set_int: thresholds between equivalent kernel paths (include/rhccq.h)"""
        self._check(self.lib.rhccq_ctx_set_int(self.ctx, int(option), int(value)), "ctx_set_int")
        # the sibling contexts of pipelined calls (one per lane / per class) follow: an option set on the context a caller holds
        # must reach the kernels wherever they are launched from
        self.__dict__.setdefault("_options", {})[int(option)] = int(value)
        for _, ln in self.__dict__.get("_lanes", {}).values():
            ln.set_option(option, value)

    def _mt_words(self, n):
        """(device address, count >= n) of the first raw MT19937 words of RandomState(42): rhccq_mt_words, the process's one table of
        this device (csrc/mt_replay.h), complete on return; the address stays readable for the life of the process"""
        words, count = C.c_void_p(), C.c_int64()
        self._check(self.lib.rhccq_mt_words(self.ctx, int(n), C.byref(words), C.byref(count)), "mt_words")
        return words, count.value

    def close(self):
        if getattr(self, "ctx", None):
            self._raw.rhccq_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers --------------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc:
            msg = self._raw.rhccq_last_error(self.ctx)
            raise RhccqError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def dev(self, arr, dtype=None):
        t = torch.from_numpy(np.ascontiguousarray(arr))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device, non_blocking=False)

    def to_host(self, *tensors):
        """device tensors -> numpy arrays through page-locked landing buffers (torch's caching host allocator), all copies in flight
        together and ONE synchronisation: a 25 MB frame comes back in ~1 ms instead of ~4 through pageable memory.  The arrays own
        their buffers (freed with them)."""
        outs = []
        for t in tensors:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            outs.append(h)
        torch.cuda.current_stream(self.device).synchronize()
        res = [h.numpy() for h in outs]
        return res[0] if len(res) == 1 else res

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _class_args(self, labels, job_base):
        n = len(job_base)
        ptrs = (C.c_void_p * n)(*[(l.data_ptr() if l is not None else 0) for l in labels])
        bases = (C.c_int32 * n)(*[int(b) for b in job_base])
        return n, ptrs, bases

    # -- K0 / K1 ----------------------------------------------------------------------------------
    def new_job_state(self, n_jobs):
        bitmaps = self.zeros((n_jobs, BITMAP_WORDS), torch.int32)
        stats = torch.tensor([INT_MAX, -1, INT_MAX, -1, 0, 0], dtype=torch.int32, device=self.device).repeat(n_jobs, 1).contiguous()
        return bitmaps, stats

    BYTEMAP_MAX_JOBS = 64        # 16 MiB of byte flags per job: up to 1 GiB of the 288 GB
    scan_events = None           # a list here makes job_scan() bracket its kernel with HIP events (bench.py)

    def job_scan(self, rgb, labels, job_base, bitmaps, stats, black_is_colour, bytemaps=None):
        """K0 + K1a.  With few jobs the colour flags go through byte maps (plain stores) and are packed into
        the bitmaps; with many jobs bits are set directly with atomics."""
        H, W = rgb.shape[0], rgb.shape[1]
        n, ptrs, bases = self._class_args(labels, job_base)
        n_jobs = bitmaps.shape[0]
        if bytemaps is None and n_jobs <= self.BYTEMAP_MAX_JOBS:
            bytemaps = self.zeros((n_jobs, 1 << 24), torch.uint8)
        if bytemaps is not None:
            ev = None
            if self.scan_events is not None:                  # measurement hook (bench.py): HIP events on the launch stream
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            self._check(self.lib.rhccq_job_scan_bytes(self.ctx, self._p(rgb), H, W, n, ptrs, bases, int(black_is_colour),
                                                      self._p(bytemaps), self._p(stats)), "job_scan_bytes")
            if ev is not None:
                ev[1].record()
                self.scan_events.append(ev)
            self._check(self.lib.rhccq_bytemap_pack(self.ctx, self._p(bytemaps), n_jobs, self._p(bitmaps)), "bytemap_pack")
        else:
            self._check(self.lib.rhccq_job_scan(self.ctx, self._p(rgb), H, W, n, ptrs, bases, int(black_is_colour),
                                                self._p(bitmaps), self._p(stats)), "job_scan")

    def job_set_black(self, bitmaps, jobs):
        if len(jobs) == 0:
            return
        j = self.dev(np.asarray(jobs, dtype=np.int32))
        self._check(self.lib.rhccq_job_set_black(self.ctx, self._p(bitmaps), self._p(j), len(jobs)), "job_set_black")

    def bitmap_count(self, bitmaps):
        n_jobs = bitmaps.shape[0]
        chunk = self.empty((n_jobs, 512), torch.int32)
        counts = self.empty((n_jobs,), torch.int32)
        self._check(self.lib.rhccq_bitmap_count(self.ctx, self._p(bitmaps), n_jobs, self._p(chunk), self._p(counts)), "bitmap_count")
        return chunk, counts

    def bitmap_emit(self, bitmaps, chunk, pal_off, total, want_keys=True):
        n_jobs = bitmaps.shape[0]
        prefix = self.empty((n_jobs, BITMAP_WORDS, 2), torch.int32)            # (bitmap word, exclusive prefix) pairs
        keys = self.empty((max(int(total), 1),), torch.int32) if want_keys else None
        self._check(self.lib.rhccq_bitmap_emit(self.ctx, self._p(bitmaps), n_jobs, self._p(chunk), self._p(pal_off),
                                               self._p(prefix), self._p(keys)), "bitmap_emit")
        return prefix, keys

    def job_blackfix(self, rgb, labels, job_base, needs_fix, best):
        H, W = rgb.shape[0], rgb.shape[1]
        n, ptrs, bases = self._class_args(labels, job_base)
        self._check(self.lib.rhccq_job_blackfix(self.ctx, self._p(rgb), H, W, n, ptrs, bases, self._p(needs_fix), self._p(best)),
                    "job_blackfix")

    # -- many-segment frames: unique colours by one device sort (rhccq_job_sort_unique) ------------------------------
    def job_stats(self, rgb, labels, job_base, n_jobs):
        H, W = rgb.shape[0], rgb.shape[1]
        n, ptrs, bases = self._class_args(labels, job_base)
        stats = torch.tensor([INT_MAX, -1, INT_MAX, -1, 0, 0], dtype=torch.int32, device=self.device).repeat(n_jobs, 1).contiguous()
        self._check(self.lib.rhccq_job_stats(self.ctx, self._p(rgb), H, W, n, ptrs, bases, self._p(stats)), "job_stats")
        return stats

    def job_sort_unique(self, rgb, labels, job_base, n_jobs, fix_key, black_jobs):
        """-> (P np.int64[n_jobs] palette sizes, keys int32[sum P] device (sorted per job, job order), rankmap int32[n_class, H*W] device)"""
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        n, ptrs, bases = self._class_args(labels, job_base)
        bj = self.dev(np.asarray(black_jobs, dtype=np.int32)) if len(black_jobs) else None
        total = n * H * W + len(black_jobs)
        tb = int(self.lib.rhccq_job_sort_unique_bytes(total))
        tmp = self.empty((tb,), torch.uint8)
        rankmap = self.empty((n, H * W), torch.int32)
        keys = self.empty((total,), torch.int32)
        start = self.empty((n_jobs,), torch.int32)
        nu = self.empty((1,), torch.int32)
        self._check(self.lib.rhccq_job_sort_unique(self.ctx, self._p(rgb), H, W, n, ptrs, bases, int(n_jobs), self._p(fix_key), self._p(bj), len(black_jobs),
                                                   self._p(tmp), tb, self._p(rankmap), self._p(keys), self._p(start), self._p(nu)), "job_sort_unique")
        st = start.cpu().numpy().astype(np.int64)
        n_unique = int(nu.cpu()[0])
        # palette sizes: the distance to the next job that has colours
        nxt = np.full(n_jobs + 1, n_unique, np.int64)
        for j in range(n_jobs - 1, -1, -1):
            nxt[j] = st[j] if st[j] >= 0 else nxt[j + 1]
        P = np.where(st >= 0, nxt[1:] - st, 0).astype(np.int64)
        return P, keys[:max(n_unique, 1)], rankmap

    def job_index_ranked(self, H, W, labels, job_base, rankmap, pal_off, first_pos, fp_lut):
        n, ptrs, bases = self._class_args(labels, job_base)
        self._check(self.lib.rhccq_job_index_ranked(self.ctx, int(H), int(W), n, ptrs, bases, self._p(rankmap), self._p(pal_off), self._p(first_pos),
                                                    self._p(fp_lut)), "job_index_ranked")

    def frame_remap_ranked(self, H, W, labels, job_base, rankmap, pal_off, lut, default_index, out_dtype, lut2=None):
        n, ptrs, bases = self._class_args(labels, job_base)
        out = self.empty((int(H), int(W)), out_dtype)
        self._check(self.lib.rhccq_frame_remap_ranked(self.ctx, int(H), int(W), n, ptrs, bases, self._p(rankmap), self._p(pal_off), self._p(lut), self._p(lut2),
                                                      int(default_index), self._p(out), out.element_size()), "frame_remap_ranked")
        return out

    def job_index(self, rgb, labels, job_base, bitmaps, prefix, pal_off, fix_key=None, want_idx=True, first_pos=None, fp_lut=None):
        H, W = rgb.shape[0], rgb.shape[1]
        n, ptrs, bases = self._class_args(labels, job_base)
        idx = self.empty((n, H * W), torch.int32) if want_idx else None
        self._check(self.lib.rhccq_job_index(self.ctx, self._p(rgb), H, W, n, ptrs, bases, self._p(bitmaps), self._p(prefix),
                                             self._p(pal_off), self._p(fix_key), self._p(idx), self._p(first_pos), self._p(fp_lut)),
                    "job_index")
        return idx

    def job_index_entries(self, rgb, labels, job_base, bitmaps, prefix, pal_off, fix_key, first_pos, fp_lut, entries_out):
        """first positions as job_index + the table entry every pixel shows, into entries_out (int32[len(labels)][H*W] view)"""
        H, W = rgb.shape[0], rgb.shape[1]
        n, ptrs, bases = self._class_args(labels, job_base)
        assert entries_out.dtype == torch.int32 and entries_out.is_contiguous() and entries_out.numel() == n * H * W
        self._check(self.lib.rhccq_job_index_entries(self.ctx, self._p(rgb), H, W, n, ptrs, bases, self._p(bitmaps), self._p(prefix), self._p(pal_off),
                                                     self._p(fix_key), self._p(first_pos), self._p(fp_lut), self._p(entries_out)), "job_index_entries")

    def frame_remap_entries(self, H, W, labels, job_base, entries, default_index, out_dtype, lut2=None):
        n, ptrs, bases = self._class_args(labels, job_base)
        out = self.empty((int(H), int(W)), out_dtype)
        self._check(self.lib.rhccq_frame_remap_entries(self.ctx, int(H), int(W), n, ptrs, bases, self._p(entries), self._p(lut2), int(default_index),
                                                       self._p(out), out.element_size()), "frame_remap_entries")
        return out

    def frame_remap(self, rgb, labels, job_base, bitmaps, prefix, pal_off, fix_key, lut, default_index, out_dtype, lut2=None):
        H, W = rgb.shape[0], rgb.shape[1]
        n, ptrs, bases = self._class_args(labels, job_base)
        out = self.empty((H, W), out_dtype)
        self._check(self.lib.rhccq_frame_remap(self.ctx, self._p(rgb), H, W, n, ptrs, bases, self._p(bitmaps), self._p(prefix),
                                               self._p(pal_off), self._p(fix_key), self._p(lut), self._p(lut2), int(default_index),
                                               self._p(out), out.element_size()), "frame_remap")
        return out

    def unique_colors(self, rgb):
        """get_all_unique_colors core: rgb uint8[H,W,3] (device) -> (keys int32[P] sorted, idx int32[H*W])."""
        assert rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.shape[-1] == 3
        bitmaps, stats = self.new_job_state(1)
        self.job_scan(rgb, [None], [0], bitmaps, stats, black_is_colour=True)
        chunk, counts = self.bitmap_count(bitmaps)
        total = int(counts.cpu()[0])
        pal_off = self.zeros((1,), torch.int64)
        prefix, keys = self.bitmap_emit(bitmaps, chunk, pal_off, total)
        idx = self.job_index(rgb, [None], [0], bitmaps, prefix, pal_off)
        return keys[:total], idx[0]

    # -- K3 / K4 ----------------------------------------------------------------------------------
    def eps_components(self, key_list, eps_list):
        """Batched DBSCAN(min_samples=1) labels.  key_list: numpy uint32/int arrays; returns
        (list of int32 numpy label arrays, list of component counts)."""
        n_prob = len(key_list)
        if n_prob == 0:
            return [], []
        sizes = [len(k) for k in key_list]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        if offs[-1] == 0:
            return [np.zeros(0, np.int32) for _ in key_list], [0] * n_prob
        desc = np.zeros((n_prob, 4), np.int32)
        r2 = np.zeros(n_prob, np.float64)
        for i, e in enumerate(eps_list):
            thr, bnd, rr = eps_threshold(e)
            desc[i] = (offs[i], sizes[i], thr, bnd)
            r2[i] = rr
        keys = self.dev(np.concatenate(key_list).astype(np.uint32).view(np.int32))
        d_desc, d_r2 = self.dev(desc), self.dev(r2)
        labels = self.empty((int(offs[-1]),), torch.int32)
        ncomp = self.empty((n_prob,), torch.int32)
        self._check(self.lib.rhccq_eps_components(self.ctx, self._p(keys), self._p(d_desc), self._p(d_r2), n_prob, int(max(sizes)),
                                                  self._p(labels), self._p(ncomp)), "eps_components")
        lab = labels.cpu().numpy()
        nc = ncomp.cpu().numpy()
        return [lab[offs[i]:offs[i + 1]] for i in range(n_prob)], [int(v) for v in nc]

    def dbscan_labels(self, keys, eps, min_samples):
        """sklearn DBSCAN(eps / 255, min_samples).fit_predict on one palette (uint32 keys, < 10 000 colours): core points = at least
        min_samples colours within eps (itself included); clusters = eps-components of the core points, numbered by their lowest core
        index; a non-core point takes the smallest label among its core neighbours, -1 (noise) without one.  -> int32 numpy labels"""
        keys = np.ascontiguousarray(keys).astype(np.uint32)
        n = len(keys)
        if n == 0:
            return np.zeros(0, np.int32)
        if min_samples <= 1:
            return self.eps_components([keys], [eps])[0][0]
        thr, bnd, rr = eps_threshold(eps)
        d_keys = self.dev(keys.view(np.int32))
        counts = self.empty((n,), torch.int32)
        self._check(self.lib.rhccq_eps_counts(self.ctx, self._p(d_keys), n, thr, bnd, rr, self._p(counts)), "eps_counts")
        core = counts.cpu().numpy() >= int(min_samples)
        core_label = np.full(n, -1, np.int32)
        if core.any():
            core_label[core] = self.eps_components([keys[core]], [eps])[0][0]
        d_core = self.dev(core_label)
        out = self.empty((n,), torch.int32)
        self._check(self.lib.rhccq_eps_border(self.ctx, self._p(d_keys), n, thr, bnd, rr, self._p(d_core), self._p(out)), "eps_border")
        return out.cpu().numpy()

    # -- K7 -----------------------------------------------------------------------------------------
    def kmeans_split(self, key_list, k_list, return_info=False):
        """Batched KMeans(k, random_state=42).fit_predict labels (KM64).  numpy in / numpy out."""
        n_prob = len(key_list)
        if n_prob == 0:
            return ([], []) if return_info else []
        sizes = [len(k) for k in key_list]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        koff = np.concatenate([[0], np.cumsum(k_list)]).astype(np.int64)
        desc = np.zeros((n_prob, 6), np.int32)
        need = 1
        u0 = self.lib.rhccq_mt_double_host(0)               # RandomState(42).random_sample(): the first centre's draw of every KMeans fit
        for i, (n, k) in enumerate(zip(sizes, k_list)):
            assert 1 <= k <= n
            T = 2 + int(math.log(k))
            desc[i] = (offs[i], n, k, 0, self.lib.rhccq_first_centre_index(n, u0), T)
            need = max(need, (k - 1) * T)
        words, _ = self._mt_words(2 + 2 * need)
        rand = self.empty((need,), torch.float64)
        self._check(self.lib.rhccq_mt_uniforms(self.ctx, words, 2, need, self._p(rand)), "mt_uniforms")     # the doubles behind u0
        keys = self.dev(np.concatenate(key_list).astype(np.uint32).view(np.int32))
        d_desc, d_koff = self.dev(desc), self.dev(koff[:-1].copy())
        work = self.empty((8 * int(koff[-1]) + 8,), torch.float64)
        labels = self.empty((int(offs[-1]),), torch.int32)
        info = self.zeros((n_prob, 4), torch.int32)
        self._check(self.lib.rhccq_kmeans(self.ctx, self._p(keys), self._p(d_desc), self._p(d_koff), self._p(rand), n_prob,
                                          int(max(sizes)), self._p(work), self._p(labels), self._p(info)), "kmeans")
        lab = labels.cpu().numpy()
        out = [lab[offs[i]:offs[i + 1]] for i in range(n_prob)]
        if return_info:
            return out, info.cpu().numpy()
        return out

    # -- K2 -----------------------------------------------------------------------------------------
    def cluster_means(self, keys, labels, k):
        """floor-mean colour per label: keys int32[n] device, labels int32[n] device -> int32[k] keys."""
        sums = self.zeros((max(k, 1), 4), torch.int64)
        self._check(self.lib.rhccq_cluster_sums(self.ctx, self._p(keys), self._p(labels), keys.numel(), max(k, 1), self._p(sums)), "cluster_sums")
        out = self.empty((max(k, 1),), torch.int32)
        self._check(self.lib.rhccq_cluster_means(self.ctx, self._p(sums), k, self._p(out)), "cluster_means")
        return out[:k], sums[:k]

    # -- K8 -----------------------------------------------------------------------------------------
    MBK_LANES = 4        # problems of a small batch run as independent pipelines on this many HIP streams
    MBK_OVERLAP = True   # a lone running problem: E-step of step t + 1 beside the update of step t (bit-identical; k8_overlap.h)
    MBK_OVERLAP_MIN_K = 1024
    MBK_OVERLAP_POLL = 64    # steps per overlapped call (the state is looked at one call behind: no drain between the calls)
    MBK_FIRST_POLL = 16

    def _lane(self, i):
        """a sibling context on its own HIP stream (host thread `i` of a pipelined call)"""
        lanes = self.__dict__.setdefault("_lanes", {})
        if i not in lanes:
            stream = torch.cuda.Stream(self.device)
            with torch.cuda.stream(stream):
                rh = Rhccq(self.device.index)
            for opt, val in self.__dict__.get("_options", {}).items():
                rh.set_option(opt, val)
            lanes[i] = (stream, rh)
        return lanes[i]

    def _minibatch_lanes(self, key_list, k_list, return_info, poll_steps, return_device, estep, estep_split, n_lanes):
        """Independent problems as independent pipelines: init -> steps -> assign of each lane's problems on its own HIP
        stream, driven by its own host thread (the C calls and the state polls release the GIL).  The k-means++ chain of
        one problem and the mini-batch steps of another then overlap instead of queueing behind each other on one
        stream: a single 4K frame's level 1 costs max(init_p + steps_p) rather than max(init) + max(steps)."""
        n_prob = len(key_list)
        # longest chains first, each to the lane with the least work so far
        order = sorted(range(n_prob), key=lambda i: -k_list[i])
        groups, load = [[] for _ in range(n_lanes)], [0] * n_lanes
        for i in order:
            g = load.index(min(load))
            groups[g].append(i)
            load[g] += k_list[i]
        parts = [k if torch.is_tensor(k) else self.dev(np.ascontiguousarray(np.asarray(k)).astype(np.uint32).view(np.int32)) for k in key_list]
        here = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(here)
        results, errors = [None] * n_lanes, []

        def run(g):
            try:
                torch.cuda.set_device(self.device)
                stream, rh = self._lane(g)
                with torch.cuda.stream(stream):
                    stream.wait_event(ready)
                    idx = groups[g]
                    out = rh.minibatch_kmeans([parts[i] for i in idx], [k_list[i] for i in idx], return_info=True, poll_steps=poll_steps,
                                              return_device=True, estep=estep, estep_split=estep_split, lanes=1)
                    done = torch.cuda.Event()
                    done.record(stream)
                    results[g] = (out, done)
            except BaseException as e:                        # surfaced to the caller below
                errors.append(e)

        futs = [lane_pool("mbk").submit(run, g) for g in range(n_lanes) if groups[g]]
        for f in futs:
            f.result()
        if errors:
            raise errors[0]
        labs = [None] * n_prob
        infos = [None] * n_prob
        n_overlapped = 0
        for g in range(n_lanes):
            if not groups[g]:
                continue
            (lg, ig), done = results[g]
            here.wait_event(done)
            n_overlapped += ig["overlapped_launches"]
            for j, i in enumerate(groups[g]):
                lg[j].record_stream(here)
                labs[i] = lg[j]
                a, b = int(ig["koff"][j]), int(ig["koff"][j + 1])
                infos[i] = (ig["state"][j], ig["centres"][a:b], ig["chosen"][a:b], ig["weights"][a:b])
        if not return_device:
            labs = [l.cpu().numpy() for l in labs]
        if return_info:
            koff = np.concatenate([[0], np.cumsum(k_list)]).astype(np.int64)
            return labs, {"state": np.stack([x[0] for x in infos]), "centres": np.concatenate([x[1] for x in infos]),
                          "chosen": np.concatenate([x[2] for x in infos]), "koff": koff, "weights": np.concatenate([x[3] for x in infos]),
                          "overlapped_launches": n_overlapped}
        return labs

    def _overlapped_steps(self, keys, probs, k, n, limit, step, st, cur_max, centres, weights, state, work, wbytes, estep_split, chunk,
                          words_per_step):
        """The remaining steps of ONE problem through rhccq_mbk_steps_overlapped, chunk after chunk WITHOUT draining the stream in
        between: chunk i + 1 is queued before chunk i's state is looked at (an asynchronous copy into pinned memory behind each
        chunk), so the kernels of a ~2000-step problem run back to back.  Everything the host needs for the next chunk it can
        derive itself: which steps reassign follows from "samples since the last reassignment" (+ batch per step, reset at
        10 k), the carry flags come back from the call, and the MT19937 table is sized for all remaining steps up front.  A
        problem that stops inside chunk i leaves chunk i + 1 as launches that return at once.  Returns (steps launched, state,
        launches that went through the overlapped entry)."""
        bs = min(1000, n)
        par = step & 1
        since = int(st[0, 12 if par else 3])
        split = estep_split or next((sp for sp in (1, 2, 4, 8) if ((k + 511) // 512) * 2 * sp >= 1536), 8)
        # MT19937 words for a BOUNDED horizon -- the chunks in flight plus the one being queued, counted from the last cursor the host
        # has seen -- regrown between chunks (a superseded table stays allocated for the kernels already queued on it, rhccq_mt_words):
        # a draw of 1000 rows consumes < 2000 words on average even at the worst acceptance (1/2), a reassigning step (at most one in
        # 10 k / 1000 + the first steps) another ~1400 for its shuffle; twice that plus the kernels' own end-of-table margins.  (Sizing
        # for all 100 n / 1000 possible steps asked for ~2.5 GB per 1.5 M-colour problem that then stopped after tens of steps.)
        cur_known, steps_known = int(cur_max), int(step)
        carry = C.c_int32(0)
        stream = torch.cuda.current_stream(self.device)
        pending = []                                         # (pinned copy of the state, event) per chunk in flight
        n_ov = 0
        # three pinned landing buffers, kept with the context (allocating pinned memory costs ~0.1 ms a time; two chunks are in flight)
        ring = self.__dict__.setdefault("_pinned_state", [torch.empty((1, 16), dtype=torch.float64, pin_memory=True) for _ in range(3)])
        n_chunk = 0
        while True:
            if step < limit:
                ns = int(min(chunk, limit - step))
                words, n_words = self._mt_words(cur_known + (step - steps_known + ns + 4) * 4200 + 8 * words_per_step)
                self._check(self.lib.rhccq_mbk_steps_overlapped(self.ctx, self._p(keys), probs, 1, step, ns, words, n_words,
                                                                self._p(centres), self._p(weights), self._p(state), self._p(work), wbytes,
                                                                split, since, C.byref(carry)), "mbk_steps_overlapped")
                for _ in range(ns):                          # the schedule's own arithmetic (sklearn _random_reassign)
                    since += bs
                    if since >= 10 * k:
                        since = 0
                step += ns
                n_ov += ns
                host = ring[n_chunk % 3]
                n_chunk += 1
                host.copy_(state, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
                pending.append((host, ev))
            if len(pending) >= 2 or step >= limit:
                host, ev = pending.pop(0)
                ev.synchronize()
                st = host.numpy().copy()
                cur_known, steps_known = int(max(st[0, 9], st[0, 14])), int(st[0, 5])
                if st[0, 4] >= 3 or st[0, 11] != 0 or st[0, 5] >= limit:
                    break
                if not pending and step >= limit:
                    break
        if pending:                                          # launches queued behind the stop: they return at once
            pending[-1][1].synchronize()
            st = pending[-1][0].numpy().copy()
        return step, st, n_ov

    def npysort_head(self, w, cap, depth0=-1, use_lds=True):
        """the SET np.argsort(w)[:cap] under numpy's scalar sort kernel (rhccq_npysort_head; w: non-negative integer counts as a
        float64 device tensor or numpy array): bool[k] numpy mask.  The selection inside a capped mini-batch reassignment."""
        w = w if torch.is_tensor(w) else self.dev(np.ascontiguousarray(w, dtype=np.float64))
        k = int(w.numel())
        scratch = self.empty((16 * k,), torch.uint8)
        mask = self.empty(((k + 31) // 32,), torch.int32)
        self._check(self.lib.rhccq_npysort_head(self.ctx, self._p(w), k, int(cap), int(depth0), int(bool(use_lds)), self._p(scratch), self._p(mask)),
                    "npysort_head")
        bits = np.unpackbits(mask.cpu().numpy().view(np.uint8), bitorder="little")[:k]
        return bits.astype(bool)

    def minibatch_kmeans(self, key_list, k_list, return_info=False, poll_steps=64, return_device=False, timing=None, estep="auto", estep_split=0,
                         lanes=None):
        """Batched MiniBatchKMeans(k, batch_size=1000, random_state=42).fit_predict labels: sklearn's fit operation
        for operation (RandomState(42) replayed from its raw MT19937 words, k-means++ in draw order, batch-ordered
        centre updates, the reassignment's np.argsort in the tie order of numpy's scalar quicksort -- csrc/k8_npysort.h;
        OPT_REASSIGN_ORDER = 0 gives the stable order of rounds 1-3).  key_list items are numpy arrays or
        device int32 tensors (kept resident); labels come back as numpy arrays, or as device tensors
        with return_device=True.  `timing` (a dict) receives the HIP-event duration of the k-means++ launch
        (events on the launch stream).  `estep`: "auto" | "tiles" | "grid" -- how the batch E-step searches the
        centres (include/rhccq.h, identical results); "auto" looks at the centres of the problems still running."""
        n_prob = len(key_list)
        if n_prob == 0:
            return ([], []) if return_info else []
        # few problems (a single frame): every problem its own pipeline; many (a batch of frames): one batched launch per
        # phase keeps all CUs busy anyway and costs the host far less
        if lanes is None:
            lanes = min(n_prob, self.MBK_LANES) if (timing is None and 1 < n_prob <= 2 * self.MBK_LANES) else 1
        if lanes > 1 and n_prob > 1:
            return self._minibatch_lanes(key_list, k_list, return_info, poll_steps, return_device, estep, estep_split, min(lanes, n_prob))
        probs = (MbkProblem * n_prob)()
        sizes = [int(k.numel()) if torch.is_tensor(k) else len(k) for k in key_list]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        koff = np.concatenate([[0], np.cumsum(k_list)]).astype(np.int64)
        parts = [k if torch.is_tensor(k) else self.dev(np.ascontiguousarray(np.asarray(k)).astype(np.uint32).view(np.int32)) for k in key_list]
        keys = parts[0] if n_prob == 1 else torch.cat(parts)
        init_list = []
        ioff = roff = 0
        # numpy's RandomState(42) stream of every problem (rhccq_mbk_draws, csrc/mt_replay.h): the sample indices on the host,
        # the k-means++ uniforms on the device
        lib = self.lib

        def draw(args):
            n, k = int(args[0]), int(args[1])
            d = MbkDraw()
            if lib.rhccq_mbk_draws(n, k, C.byref(d), None, 0):
                raise RhccqError(f"rhccq_mbk_draws({n}, {k}): bad argument")
            init_idx = np.empty(d.init_size, np.int32)
            lib.rhccq_mbk_draws(n, k, C.byref(d), init_idx.ctypes.data, init_idx.size)
            return d, init_idx

        todo = list(zip(sizes, k_list))
        # the calls release the GIL: the problems' draws run side by side (the GPU waits for them)
        drawn = list(_draw_pool().map(draw, todo)) if n_prob > 1 else [draw(todo[0])]
        for i, ((n, k), (d, init_idx)) in enumerate(zip(todo, drawn)):
            p = probs[i]
            p.off, p.n, p.k, p.koff = int(offs[i]), n, k, int(koff[i])
            p.init_off, p.init_n, p.rand_off, p.first, p.T = ioff, d.init_size, roff, d.first, d.T
            init_list.append(init_idx)
            ioff += d.init_size
            roff += d.n_uniforms
        words, _ = self._mt_words(max(d.pos + 2 * d.n_uniforms for d, _ in drawn))
        d_rand = self.empty((roff,), torch.float64)
        for p, (d, _) in zip(probs, drawn):
            self._check(self.lib.rhccq_mt_uniforms(self.ctx, words, d.pos, d.n_uniforms, C.c_void_p(d_rand.data_ptr() + 8 * p.rand_off)), "mt_uniforms")
        d_init = self.dev(np.concatenate(init_list))           # sklearn's draw order
        # internal pruning index: the sample positions in Morton order of their colours, on the device: 64 consecutive
        # entries form a compact box, which is what the exact block pruning of mbk_init_kernel relies on
        obytes = int(self.lib.rhccq_mbk_order_bytes(ioff))
        otmp = self.empty((obytes,), torch.uint8)
        d_perm = self.empty((ioff,), torch.int32)
        self._check(self.lib.rhccq_mbk_order(self.ctx, self._p(keys), probs, n_prob, self._p(d_init), self._p(d_perm), self._p(otmp), obytes),
                    "mbk_order")
        K = int(koff[-1])
        centres = self.zeros((K, 4), torch.float64)
        chosen = self.zeros((K,), torch.int32)
        if timing is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        self._check(self.lib.rhccq_mbk_init(self.ctx, self._p(keys), probs, n_prob, self._p(d_init), self._p(d_perm), self._p(d_rand),
                                            self._p(centres), self._p(chosen)), "mbk_init")
        if timing is not None:
            ev[1].record()
            ev[1].synchronize()
            timing["init_ms"] = ev[0].elapsed_time(ev[1])
        weights = self.zeros((K,), torch.float64)
        st0 = np.zeros((n_prob, 16))
        st0[:, 8] = k_list                                   # every centre starts with zero weight
        st0[:, 9] = [d.cursor0 for d, _ in drawn]            # MT19937 words consumed so far: the stream behind the k-means++ uniforms
        state = self.dev(st0)
        cur_max = int(st0[:, 9].max())
        WORDS_PER_STEP = 16384                               # kWordsMargin of mbk_update_kernel
        wbytes = int(self.lib.rhccq_mbk_work_bytes(probs, n_prob))
        work = self.empty((max(wbytes, 8),), torch.uint8)
        k_arr = np.asarray(k_list, np.int64)
        limit = np.array([d.limit for d, _ in drawn], np.int64)
        running = np.ones(n_prob, bool)
        step = 0                                             # launch index = step index of every problem still running
        carry = C.c_int32(0)
        st = st0
        n_overlapped = 0

        def check(st):
            if (st[:, 4] == 3).any():
                raise RhccqError("mini-batch steps ran past the end of the MT19937 word table (internal sizing error)")
            if (st[:, 4] == 4).any():
                raise RhccqError("the sharded k-means++ chain gave up waiting for a partner workgroup (RHCCQ_OPT_INIT_SHARDS = 1 avoids the hand-offs)")
            if (st[:, 4] == 5).any():
                raise RhccqError("the overlapped mini-batch schedule and the device state disagree about a reassignment (internal error)")

        while running.any():
            par = step & 1
            # a lone problem whose centres all carry weight: the next E-step starts beside the update (rhccq_mbk_steps_overlapped)
            tiles_mode = {"tiles": 1, "grid": 2}.get(estep) or (2 if int(k_arr[running].sum()) >= 200000 else 1)
            if (self.MBK_OVERLAP and n_prob == 1 and step > 0 and tiles_mode == 1 and k_list[0] >= self.MBK_OVERLAP_MIN_K
                    and st[0, 13 if par else 8] == 0):
                step, st, n_ov = self._overlapped_steps(keys, probs, k_list[0], sizes[0], int(limit[0]), step, st, cur_max, centres, weights,
                                                        state, work, wbytes, estep_split, max(poll_steps, self.MBK_OVERLAP_POLL), WORDS_PER_STEP)
                n_overlapped += n_ov
                check(st)
                break                                        # (the problem has stopped or used up its steps)
            # most problems converge within a dozen steps: look early once, so that a finished problem does not sit through the
            # launches of a whole poll interval
            ns = int(min(poll_steps if step else min(poll_steps, self.MBK_FIRST_POLL), max(1, limit[running].max() - step)))
            # the grid E-step pays when many centres are in flight; once only stragglers are left the tiled
            # brute force has fewer and shorter launches per step
            mode = tiles_mode
            # few workgroups left (a straggler problem): several threads share a batch point in the tiled E-step
            wgs = int(((k_arr[running] + 511) // 512).sum()) * 2
            split = estep_split or next((sp for sp in (1, 2, 4, 8) if wgs * sp >= 1536), 8)
            words, n_words = self._mt_words(cur_max + (ns + 3) * WORDS_PER_STEP)     # a step consumes at most WORDS_PER_STEP
            if step > 0:
                # no running problem reassigns during these steps (no centre without weight, fewer than 10 k samples since the last
                # reassignment throughout): the second launch of a reassigning step is left out (RHCCQ_STEPS_NO_REASSIGN)
                bs_arr = np.minimum(1000, np.asarray(sizes, np.int64))
                quiet = (st[:, 13 if par else 8] == 0) & (st[:, 12 if par else 3] + ns * bs_arr < 10 * k_arr)
                if quiet[running].all():
                    mode |= 0x100
            self._check(self.lib.rhccq_mbk_steps(self.ctx, self._p(keys), probs, n_prob, step, ns, words, n_words,
                                                 self._p(centres), self._p(weights), self._p(state), self._p(work), wbytes, mode, split),
                        "mbk_steps")
            step += ns
            st = state.cpu().numpy()
            cur_max = int(max(st[:, 9].max(), st[:, 14].max()))
            check(st)
            running = (st[:, 11] == 0) & (st[:, 5] < limit)
        labels = self.empty((int(offs[-1]),), torch.int32)
        self._check(self.lib.rhccq_mbk_assign(self.ctx, self._p(keys), probs, n_prob, self._p(centres), self._p(work), wbytes,
                                              self._p(labels)), "mbk_assign")
        if return_device:
            out = [labels[offs[i]:offs[i + 1]] for i in range(n_prob)]
        else:
            lab = labels.cpu().numpy()
            out = [lab[offs[i]:offs[i + 1]] for i in range(n_prob)]
        if return_info:
            return out, {"state": state.cpu().numpy(), "centres": centres.cpu().numpy(), "chosen": chosen.cpu().numpy(),
                         "koff": koff, "weights": weights.cpu().numpy(), "overlapped_launches": n_overlapped}
        return out

    # -- EXTENSION: pixel-space DBSCAN on (x, y, L, a, b) (no reference counterpart) ------------------------
    @staticmethod
    def px_tables():
        """float32[256 + 2048]: 8-bit sRGB -> linear, then 1024 pairs (f(i/1024), f((i+1)/1024) - f(i/1024)) of the CIE-Lab
        transfer function (cube root above 0.008856, linear toe below); values evaluated in float64 and rounded once,
        differences taken in float32; shared with oracle.px_dbscan"""
        v = np.arange(256, dtype=np.float64) / 255.0
        lin = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4).astype(np.float32)
        t = np.arange(1025, dtype=np.float64) / 1024.0
        f = np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0).astype(np.float32)
        fd = np.stack([f[:-1], f[1:] - f[:-1]], axis=1).reshape(-1)
        return np.concatenate([lin, fd]).astype(np.float32)

    def px_dbscan(self, rgb, radius, eps, spatial_weight, min_pts, want_count=False):
        """rgb uint8[H,W,3] device -> labels int32[H,W] (0 = noise, else 1 + smallest pixel index of the cluster),
        core mask, optional neighbour counts."""
        assert rgb.dtype == torch.uint8 and rgb.is_contiguous()
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        if getattr(self, "_px_lut", None) is None:
            self._px_lut = self.dev(self.px_tables())
        parent = self.empty((H, W), torch.int32)
        count = self.empty((H, W), torch.uint8) if want_count else None
        self._check(self.lib.rhccq_px_neighbours(self.ctx, self._p(rgb), H, W, int(radius), float(eps), float(spatial_weight), int(min_pts),
                                                 self._p(self._px_lut), self._p(parent), self._p(count)), "px_neighbours")
        core = parent >= 0
        labels = self.empty((H, W), torch.int32)
        self._check(self.lib.rhccq_px_expand(self.ctx, self._p(rgb), H, W, int(radius), float(eps), float(spatial_weight), self._p(self._px_lut),
                                             self._p(parent), self._p(labels)), "px_expand")
        return (labels, core, count) if want_count else (labels, core)

    # -- quality metrics (comparison.py:30-80) ------------------------------------------------------
    def error_sums(self, a, b):
        """a, b: uint8[H,W,3] device -> int64[5]: per-channel sum of squared differences, sum |d|, max |d|."""
        assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
        sums = self.empty((5,), torch.int64)
        self._check(self.lib.rhccq_error_sums(self.ctx, self._p(a), self._p(b), a.numel() // 3, self._p(sums)), "error_sums")
        return sums.cpu().numpy()

    def error_tables(self, a, b, want_maxerr=False):
        """a, b: uint8[H,W,3] device -> int64[256][3] rows by worst-channel error (+ uint8[H,W] per-pixel worst error)"""
        assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
        tab = self.empty((256, 3), torch.int64)
        me = self.empty(tuple(a.shape[:2]), torch.uint8) if want_maxerr else None
        self._check(self.lib.rhccq_error_tables(self.ctx, self._p(a), self._p(b), a.numel() // 3, self._p(tab), self._p(me)), "error_tables")
        return tab.cpu().numpy(), me

    def ssim7(self, a, b):
        """mean SSIM per channel (float64[3]) with skimage's defaults for win_size=7, data_range=255."""
        H, W = int(a.shape[0]), int(a.shape[1])
        nb = int(self.lib.rhccq_ssim7_blocks(H, W))
        if nb == 0:
            raise ValueError("win_size exceeds image extent")          # skimage's message
        part = self.empty((nb, 3), torch.float64)
        self._check(self.lib.rhccq_ssim7_sums(self.ctx, self._p(a), self._p(b), H, W, self._p(part), nb), "ssim7")
        return part.cpu().numpy().sum(axis=0) / float((H - 6) * (W - 6))

    # -- per-class quality metrics (EXTENSION: csrc/region_metrics.hip) ------------------------------------
    def _class_map(self, cls, shape):
        if cls.dtype == torch.bool:
            cls = cls.view(torch.uint8)
        assert cls.dtype == torch.uint8 and cls.is_contiguous() and tuple(cls.shape) == tuple(shape), "class map: uint8 / bool [H,W]"
        return cls

    def class_error_sums(self, a, b, cls, n_classes):
        """a, b: uint8[H,W,3] device, cls: uint8 / bool [H,W] device -> int64[n_classes, 6]: per class the sums of squared differences of
        R, G, B, the sum of |d|, max |d| and the pixel count; pixels with cls >= n_classes are in no row."""
        assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
        cls = self._class_map(cls, a.shape[:2])
        sums = self.empty((max(int(n_classes), 1), 6), torch.int64)
        self._check(self.lib.rhccq_class_error_sums(self.ctx, self._p(a), self._p(b), self._p(cls), a.numel() // 3, int(n_classes),
                                                    self._p(sums)), "class_error_sums")
        return sums.cpu().numpy()

    def class_error_sums_indexed(self, a, idx, palette, cls, n_classes):
        """class_error_sums(a, palette[idx], cls, n_classes) without the image palette[idx]: idx uint8 / uint16 (int16 storage) / int32
        device with one element per pixel, palette uint8[K,3] device (Rhccq.decode's arguments)"""
        assert a.dtype == torch.uint8 and a.is_contiguous() and a.shape[-1] == 3 and idx.is_contiguous() and idx.numel() == a.numel() // 3
        assert palette.dtype == torch.uint8 and palette.is_contiguous() and palette.shape[-1] == 3
        cls = self._class_map(cls, a.shape[:2])
        sums = self.empty((max(int(n_classes), 1), 6), torch.int64)
        self._check(self.lib.rhccq_class_error_sums_indexed(self.ctx, self._p(a), self._p(idx), idx.element_size(), self._p(palette),
                                                            palette.shape[0], self._p(cls), a.numel() // 3, int(n_classes), self._p(sums)),
                    "class_error_sums_indexed")
        return sums.cpu().numpy()

    def class_ssim7(self, a, b, cls, n_classes):
        """SSIM (Rhccq.ssim7's definition) by the class of the window's centre pixel -> (float64[n_classes, 3] sums of S per channel,
        int64[n_classes] window centres); an image no 7x7 window fits gives zero centres."""
        assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
        cls = self._class_map(cls, a.shape[:2])
        if not 1 <= int(n_classes) <= 16:
            raise RhccqError("class_ssim7: n_classes must be 1..16")
        H, W = int(a.shape[0]), int(a.shape[1])
        nb = int(self.lib.rhccq_class_ssim7_blocks(H, W))
        if nb == 0:
            return np.zeros((n_classes, 3)), np.zeros(n_classes, np.int64)
        part = self.empty((nb, int(n_classes), 4), torch.float64)
        self._check(self.lib.rhccq_class_ssim7_sums(self.ctx, self._p(a), self._p(b), self._p(cls), H, W, int(n_classes), self._p(part), nb),
                    "class_ssim7")
        tot = part.cpu().numpy().sum(axis=0)                           # tiles in order, as ssim7 adds them
        return tot[:, :3], np.rint(tot[:, 3]).astype(np.int64)

    # -- nearest-colour remap onto a given palette (EXTENSION: csrc/palette_remap.hip) --------------------------
    def palette_remap(self, rgb, palette, class_map=None, n_classes=0):
        """rgb uint8[..., 3], palette uint8[K, 3] (numpy or device), class_map uint8 / bool, one element per pixel, or None ->
        (indices device tensor of rgb's leading shape: uint8 when K <= 256, else int16 holding uint16; sums device int64
        [n_classes + 1, 2]: row c = {pixels, sum of squared errors} of class c, the last row over every pixel).  Each index is the
        nearest palette row in exact integers, ties to the lowest row."""
        rgb, palette = A.pixels(rgb, palette, self.device, "palette_remap")
        n, K = rgb.numel() // 3, int(palette.shape[0])
        cls = A.class_map(class_map, n, n_classes, self.device, "palette_remap")
        idx = self.empty(tuple(rgb.shape[:-1]), A.index_dtype(K))
        sums = self.empty((int(n_classes) + 1, 2), torch.int64)
        if n == 0:                                       # (empty tensors have null pointers: nothing to launch)
            if not 0 <= int(n_classes) <= 16 or K < 1 or K > 65536:
                raise RhccqError("palette_remap: K must be 1..65536 and n_classes 0..16")
            return idx, sums.zero_()
        self._check(self.lib.rhccq_palette_remap(self.ctx, self._p(rgb), n, self._p(palette), K, self._p(cls), int(n_classes), self._p(idx),
                                                 idx.element_size(), self._p(sums)), "palette_remap")
        return idx, sums

    # -- run-carrying remap onto a given palette (EXTENSION: csrc/palette_runs.hip) -------------------------------------
    def palette_runs(self, rgb, palette, slack, class_map=None, n_classes=0):
        """rgb uint8[H, W, 3], palette uint8[K, 3] (numpy or device), slack: one integer 0..RUN_SLACK_MAX for every pixel, or
        n_classes + 1 of them (a pixel of class c < n_classes takes slack[c], every other pixel slack[-1]), class_map uint8 / bool
        [H, W] or None -> (indices device [H, W], uint8 when K <= 256, else int16 holding uint16; sums device int64
        [n_classes + 1, 3]: row c = {pixels, sum of squared errors, carried pixels} of class c, the last row over every pixel).
        Along every image row a pixel keeps its left neighbour's index while that costs at most its slack more squared error
        than its nearest row (palette_remap's); a tie keeps the neighbour's.  Exact integers."""
        rgb, palette = A.pixels(rgb, palette, self.device, "palette_runs", rows=True)
        H, W, K, n_classes = int(rgb.shape[0]), int(rgb.shape[1]), int(palette.shape[0]), int(n_classes)
        _, table = A.class_table(slack, n_classes, RUN_SLACK_MAX, "palette_runs", "slack")
        cls = A.class_map(class_map, H * W, n_classes, self.device, "palette_runs")
        idx = self.empty((H, W), A.index_dtype(K))
        sums = self.empty((n_classes + 1, 3), torch.int64)
        if H * W == 0:                                   # (empty tensors have null pointers: nothing to launch)
            if not 0 <= n_classes <= 16 or K < 1 or K > 65536:
                raise RhccqError("palette_runs: K must be 1..65536 and n_classes 0..16")
            return idx, sums.zero_()
        self._check(self.lib.rhccq_palette_runs(self.ctx, self._p(rgb), H, W, self._p(palette), K, self._p(cls), n_classes, table, self._p(idx),
                                                idx.element_size(), self._p(sums)), "palette_runs")
        return idx, sums

    # -- exact row segmentation onto a given palette (EXTENSION: csrc/palette_segment.hip) ---------------------------------
    def palette_segment(self, rgb, palette, penalty, class_map=None, n_classes=0):
        """rgb uint8[H, W, 3], palette uint8[K, 3] (numpy or device; K <= palette_segment_max_rows(), else RhccqError), penalty: one
        integer 0..RUN_PENALTY_MAX for every pixel, or n_classes + 1 of them (a pixel of class c < n_classes takes penalty[c], every
        other pixel penalty[-1]), class_map uint8 / bool [H, W] or None -> (indices device [H, W], uint8 when K <= 256, else int16
        holding uint16; sums device int64 [n_classes + 1, 4]: row c = {pixels, sum of squared errors, pixels whose index is not the
        nearest row, breaks} of class c, the last row over every pixel).  Per image row the index map minimises the squared error
        plus the penalty of every pixel whose index differs from its left neighbour's (a break), exactly: the 1-D Potts
        segmentation by its K-state dynamic programme in integers (include/rhccq.h pins ties).  The workspace (the full plane of
        decisions, rhccq_palette_segment_bytes) is a torch allocation of this call."""
        rgb, palette = A.pixels(rgb, palette, self.device, "palette_segment", rows=True)
        H, W, K, n_classes = int(rgb.shape[0]), int(rgb.shape[1]), int(palette.shape[0]), int(n_classes)
        _, table = A.class_table(penalty, n_classes, RUN_PENALTY_MAX, "palette_segment", "penalty")
        cls = A.class_map(class_map, H * W, n_classes, self.device, "palette_segment")
        if K < 1 or K > palette_segment_max_rows() or not 0 <= n_classes <= 16:
            raise RhccqError(f"palette_segment: K must be 1..{palette_segment_max_rows()} on the device and n_classes 0..16")
        idx = self.empty((H, W), A.index_dtype(K))
        sums = self.empty((n_classes + 1, 4), torch.int64)
        if H * W == 0:                                   # (empty tensors have null pointers: nothing to launch)
            return idx, sums.zero_()
        nbytes = int(self.lib.rhccq_palette_segment_bytes(H, W, K))
        work = self.empty((nbytes // 8,), torch.int64)
        self._check(self.lib.rhccq_palette_segment(self.ctx, self._p(rgb), H, W, self._p(palette), K, self._p(cls), n_classes, table,
                                                   self._p(work), nbytes, self._p(idx), idx.element_size(), self._p(sums)), "palette_segment")
        return idx, sums

    # -- error-diffusing remap onto a given palette (EXTENSION: csrc/palette_dither.hip) -----------------------------------
    def palette_dither(self, rgb, palette, strength, class_map=None, n_classes=0, with_status=False):
        """rgb uint8[H, W, 3], palette uint8[K, 3] (numpy or device; K <= palette_dither_max_rows(), else RhccqError), strength: one
        integer 0..DITHER_MAX for every pixel, or n_classes + 1 of them (a pixel of class c < n_classes takes strength[c], every other
        pixel strength[-1]), class_map uint8 / bool [H, W] or None -> (indices device [H, W], uint8 when K <= 256, else int16 holding
        uint16; sums device int64 [n_classes + 1, 3]: row c = {pixels, sum of squared errors against the original pixel, pixels whose
        index is not the nearest row} of class c, the last row over every pixel).  Floyd-Steinberg error diffusion in exact integers
        and raster order (include/rhccq.h pins rounding and ties); the strength scales what a pixel receives: 0 gives palette_remap's
        index, 256 the full error.  The workspace (rhccq_palette_dither_bytes) is a torch allocation of this call.
        with_status: -> (indices, sums, status device int32[1]) without waiting for the device; the caller reads status with the sums
        and hands it to check_dither.  Without it the call waits, checks the status itself and returns (indices, sums)."""
        rgb, palette = A.pixels(rgb, palette, self.device, "palette_dither", rows=True)
        H, W, K, n_classes = int(rgb.shape[0]), int(rgb.shape[1]), int(palette.shape[0]), int(n_classes)
        _, table = A.class_table(strength, n_classes, DITHER_MAX, "palette_dither", "strength")
        cls = A.class_map(class_map, H * W, n_classes, self.device, "palette_dither")
        if K < 1 or K > palette_dither_max_rows() or not 0 <= n_classes <= 16:
            raise RhccqError(f"palette_dither: K must be 1..{palette_dither_max_rows()} on the device and n_classes 0..16")
        idx = self.empty((H, W), A.index_dtype(K))
        sums = self.empty((n_classes + 1, 3), torch.int64)
        if H * W == 0:                                   # (empty tensors have null pointers: nothing to launch)
            status = self.zeros((1,), torch.int32)
            return (idx, sums.zero_(), status) if with_status else (idx, sums.zero_())
        status = self.empty((1,), torch.int32)
        nbytes = int(self.lib.rhccq_palette_dither_bytes(H, W))
        work = self.empty((nbytes // 4,), torch.int32)
        self._check(self.lib.rhccq_palette_dither(self.ctx, self._p(rgb), H, W, self._p(palette), K, self._p(cls), n_classes, table, self._p(work),
                                                  nbytes, self._p(idx), idx.element_size(), self._p(sums), self._p(status)), "palette_dither")
        if with_status:
            return idx, sums, status
        self.check_dither(self.to_host(status))
        return idx, sums

    @staticmethod
    def check_dither(status):
        """the status word of palette_dither(with_status=True), read back: non-zero raises RhccqError (the indices and sums mean nothing)"""
        if int(np.asarray(status).reshape(-1)[0]) != 0:
            raise RhccqError("palette_dither: a band gave up waiting for the band above it; the indices are unspecified")

    # -- position-only (pattern) dither onto a given palette (EXTENSION: csrc/palette_pattern.hip) --------------------------------
    @staticmethod
    def _pattern_size(size, fn):
        size = int(size)
        if size not in PATTERN_SIZES:
            raise ValueError(f"{fn}: size must be 2, 4 or 8")
        return size

    def palette_pattern(self, rgb, palette, strength, size=4, class_map=None, n_classes=0):
        """rgb uint8[H, W, 3], palette uint8[K, 3] (numpy or device; K <= palette_pattern_max_rows(), else RhccqError), strength: one
        integer 0..PATTERN_MAX for every pixel, or n_classes + 1 of them (a pixel of class c < n_classes takes strength[c], every other
        pixel strength[-1]), size in PATTERN_SIZES, class_map uint8 / bool [H, W] or None -> (indices device [H, W], uint8 when
        K <= 256, else int16 holding uint16; sums device int64 [n_classes + 1, 3]: row c = {pixels, sum of squared errors against the
        original pixel, pixels whose index is not the nearest row} of class c, the last row over every pixel).  Pattern dithering in
        exact integers (include/rhccq.h pins rounding, order and ties): a pixel builds size x size candidate rows whose mean approaches
        it, orders them by luma, and the Bayer threshold of (y mod size, x mod size) picks one.  The index depends on the pixel and its
        position only; strength 0 gives palette_remap's index.  One launch, no workspace, no status word, no read back."""
        fn = "palette_pattern"
        rgb, palette = A.pixels(rgb, palette, self.device, fn, rows=True)
        H, W, K, n_classes = int(rgb.shape[0]), int(rgb.shape[1]), int(palette.shape[0]), int(n_classes)
        _, table = A.class_table(strength, n_classes, PATTERN_MAX, fn, "strength")
        size = self._pattern_size(size, fn)
        cls = A.class_map(class_map, H * W, n_classes, self.device, fn)
        if K < 1 or K > palette_pattern_max_rows() or not 0 <= n_classes <= 16:
            raise RhccqError(f"{fn}: K must be 1..{palette_pattern_max_rows()} on the device and n_classes 0..16")
        idx = self.empty((H, W), A.index_dtype(K))
        sums = self.empty((n_classes + 1, 3), torch.int64)
        if H * W == 0:                                   # (empty tensors have null pointers: nothing to launch)
            return idx, sums.zero_()
        self._check(self.lib.rhccq_palette_pattern(self.ctx, self._p(rgb), H, W, self._p(palette), K, self._p(cls), n_classes, table, size,
                                                   self._p(idx), idx.element_size(), self._p(sums)), fn)
        return idx, sums

    # -- refinement of a given palette: exact integer Lloyd iterations (EXTENSION: csrc/palette_refine.hip) ----------
    def palette_refine(self, rgb, palette, class_map=None, weights=None, max_iter=8):
        """rgb uint8[..., 3], palette uint8[K, 3] (numpy or device), class_map uint8 / bool, one element per pixel, or None;
        weights: n_classes + 1 ints 0..255 (a pixel of class c < n_classes weighs weights[c], every other pixel weights[-1]),
        None = all ones and no classes -> (palette: a NEW device uint8[K, 3], the argument is not modified; history device int64
        [max_iter, 2]: row i = {weighted sum of squared errors the iteration's assignment found, rows it changed}, zero from
        n_iter on; n_iter device int32[1]).  Each iteration assigns every pixel as palette_remap does and moves every row that
        received pixels to their weighted mean rounded to nearest; it stops after the first iteration that changes no row."""
        rgb, palette = A.pixels(rgb, palette, self.device, "palette_refine")
        n, K, max_iter = rgb.numel() // 3, int(palette.shape[0]), int(max_iter)
        w, warg = A.class_weights(weights, None, "palette_refine")
        n_classes = 0 if w is None else len(w) - 1
        cls = A.class_map(class_map, n, n_classes, self.device, "palette_refine", without="class weights")
        out = palette.clone()
        history = self.empty((max(max_iter, 0), 2), torch.int64)
        n_iter = self.empty((1,), torch.int32)
        if n == 0:                                       # (empty tensors have null pointers: nothing to launch)
            if not 0 <= n_classes <= 16 or K < 1 or K > 65536 or not 1 <= max_iter <= 64 or A.bad_weights(w):
                raise RhccqError("palette_refine: K must be 1..65536, max_iter 1..64, weights 0..255 (n_classes + 1 <= 17 of them, one > 0)")
            return out, history.zero_(), n_iter.zero_()
        wbytes = int(self._raw.rhccq_palette_refine_bytes(K)) if K >= 1 else 0
        work = self.empty((max(wbytes // 8, 1),), torch.int64)
        self._check(self.lib.rhccq_palette_refine(self.ctx, self._p(rgb), n, self._p(out), K, self._p(cls), n_classes, warg, max_iter,
                                                  self._p(work), wbytes, self._p(history), self._p(n_iter)), "palette_refine")
        return out, history, n_iter

    # -- reduction of a given palette to N rows: exact pairwise merging (EXTENSION: csrc/palette_reduce.hip) ------------
    def palette_reduce(self, palette, counts, colours):
        """palette uint8[K, 3], counts [K] non-negative integers (numpy or device; the weight of every row, their sum at most
        2^32 - 1), colours = K_target in 1..K -> (palette device uint8[k_out, 3], counts device int64[k_out], map device int32[K]:
        old row -> new row, -1 for a row of count 0, merges device int32[n_steps, 2]: the (a, b) of every merge in order).
        Pairwise-nearest-neighbour merging by Ward's criterion in exact integers (include/rhccq.h): the two clusters whose union
        costs least merge, ties to the lowest rows, the merged centre is the weighted mean rounded to nearest.  k_out =
        min(colours, rows of non-zero count) is read back once.  K above palette_reduce_max_rows() raises RhccqError."""
        palette = A.as_dtype(palette, torch.uint8, self.device, "palette_reduce", "palette")
        counts = A.as_dtype(counts, torch.int64, self.device, "palette_reduce", "counts")
        K, target = A.counted_rows(palette, counts, "palette_reduce"), int(colours)
        A.rows_cap(K, palette_reduce_max_rows(), "palette_reduce")
        if K < 1 or not 1 <= target <= K:
            raise RhccqError("palette_reduce: K >= 1 and colours in 1..K are required")
        wbytes = int(self._raw.rhccq_palette_reduce_bytes(K))
        work = self.empty((wbytes // 8,), torch.int64)
        pal_out = self.empty((target, 3), torch.uint8)
        cnt_out = self.empty((target,), torch.int64)
        map_ = self.empty((K,), torch.int32)
        merges = self.empty((max(K - 1, 1), 2), torch.int32)
        k_out = self.empty((1,), torch.int32)
        self._check(self.lib.rhccq_palette_reduce(self.ctx, self._p(palette), self._p(counts), K, target, self._p(work), wbytes, self._p(pal_out),
                                                  self._p(cnt_out), self._p(map_), self._p(merges), self._p(k_out)), "palette_reduce")
        k, live = torch.cat([k_out, (counts != 0).sum().to(torch.int32).reshape(1)]).tolist()     # the one read
        n_steps = live - A.k_out_rows(k, "palette_reduce")   # the errors only the counts show come back through k_out
        return pal_out[:k], cnt_out[:k], map_, merges[:max(n_steps, 0)]

    # -- a palette from the image: exact variance splits over a colour histogram (EXTENSION: csrc/palette_build.hip) ---------------
    def palette_cells(self, rgb, cls=None, n_classes=0, weights=None, into=None):
        """rgb uint8[..., 3] (numpy or device), cls uint8 / bool, one element per pixel, or None; weights: n_classes + 1 ints 0..255
        (a pixel of class c < n_classes weighs weights[c], every other pixel weights[-1]; None = all ones) -> the device table
        int64[4, 32, 32, 32]: planes {N, Sr, Sg, Sb} over the cells (r >> 3, g >> 3, b >> 3), N the summed weights, S the summed
        weight x channel value.  into: a table an earlier call returned; this call adds to it and returns it, so the tables of
        several frames sum into one.  One pass over the pixels, no read back."""
        rgb, _ = A.pixels(rgb, None, self.device, "palette_cells")
        n, n_classes = rgb.numel() // 3, int(n_classes)
        w, warg = A.class_weights(weights, n_classes, "palette_cells")
        d_cls = A.class_map(cls, n, n_classes, self.device, "palette_cells", what="cls")
        if not 0 <= n_classes <= 16 or A.bad_weights(w):
            raise RhccqError("palette_cells: n_classes must be 0..16 and weights 0..255 with one > 0")
        if into is not None:
            if not torch.is_tensor(into) or into.dtype != torch.int64 or tuple(into.shape) != PALETTE_CELLS_SHAPE or not into.is_contiguous() \
                    or into.device != torch.device(self.device):
                raise ValueError("palette_cells: into must be a table palette_cells returned (contiguous device int64[4, 32, 32, 32])")
        cells = into if into is not None else self.empty(PALETTE_CELLS_SHAPE, torch.int64)
        if n == 0:                                       # (empty tensors have null pointers: nothing to launch)
            return cells if into is not None else cells.zero_()
        self._check(self.lib.rhccq_palette_cells(self.ctx, self._p(rgb), n, self._p(d_cls), n_classes, warg, 1 if into is not None else 0,
                                                 self._p(cells)), "palette_cells")
        return cells

    def palette_build(self, cells, colours):
        """cells: the table of palette_cells (int64[4, 32, 32, 32], numpy or device; the sum of N at most 2^32 - 1), colours = K_target
        in 1..palette_build_max_rows() -> (palette device uint8[k, 3], counts device int64[k], splits device int32[k - 1, 3]: the
        (box, axis, t) of every split in order, boxes device uint8[k, 6]: lo then hi per box).  Greedy variance-minimising box
        splitting in exact integers (include/rhccq.h): the box whose best cut removes the most squared error is split, ties to the
        lowest box, axis and position; a row is the mean of its box's pixels rounded to nearest.  k <= colours is read back once."""
        cells = A.cells_table(cells, "palette_build")
        if tuple(cells.shape) != PALETTE_CELLS_SHAPE:
            raise ValueError("palette_build: cells [4, 32, 32, 32] is expected")
        cells = cells.to(self.device).contiguous()
        target, cap = int(colours), palette_build_max_rows()
        if target > cap:
            raise RhccqError(f"palette_build: {target} colours, the device form returns at most {cap} (palette_build_max_rows())")
        if target < 1:
            raise RhccqError("palette_build: colours >= 1 is required")
        wbytes = int(self._raw.rhccq_palette_build_bytes())
        work = self.empty((wbytes // 8,), torch.int64)
        pal_out = self.empty((target, 3), torch.uint8)
        cnt_out = self.empty((target,), torch.int64)
        boxes = self.empty((target, 6), torch.uint8)
        splits = self.empty((max(target - 1, 1), 3), torch.int32)
        k_out = self.empty((1,), torch.int32)
        self._check(self.lib.rhccq_palette_build(self.ctx, self._p(cells), target, self._p(work), wbytes, self._p(pal_out), self._p(cnt_out),
                                                 self._p(boxes), self._p(splits), self._p(k_out)), "palette_build")
        # the one read; the errors only the table shows come back through k_out
        k = A.k_out_rows(int(k_out.item()), "palette_build", "the table is empty", "the table's N adds up to more than 2^32 - 1")
        return pal_out[:k], cnt_out[:k], splits[:k - 1], boxes[:k]

    # -- the palette build path for a batch of images (EXTENSION: csrc/palette_batch.hip) ----------------------------------------------
    def _batch_pixels(self, fn, rgb, px_off, px_off_dev, class_map):
        """the arguments the four batched calls share -> (rgb device uint8, px_off host int64[B + 1], its device copy, class map device
        or None, pixels).  px_off_dev: a device int64 copy of px_off an earlier call of the family returned or the caller made (one
        upload for the four calls); None: this call uploads one"""
        rgb, _ = A.pixels(rgb, None, self.device, fn)
        n = rgb.numel() // 3
        off = np.ascontiguousarray(np.asarray(px_off.cpu() if torch.is_tensor(px_off) else px_off), dtype=np.int64).reshape(-1)
        if len(off) < 2 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != n:
            raise ValueError(f"{fn}: px_off must hold B + 1 >= 2 offsets that start at 0, never decrease and end at the number of pixels")
        if px_off_dev is None:
            px_off_dev = self.dev(off)
        elif not torch.is_tensor(px_off_dev) or px_off_dev.dtype != torch.int64 or px_off_dev.numel() != len(off) or not px_off_dev.is_contiguous() \
                or px_off_dev.device != torch.device(self.device):
            raise ValueError(f"{fn}: px_off_dev must be a contiguous device int64 copy of px_off")
        cls = A.class_map(class_map, n, 0, self.device, fn)          # (n_classes: each call tests it where its other arguments are done)
        return rgb, off, px_off_dev, cls, n

    def _batch_palettes(self, fn, palettes, k_rows, B):
        if not torch.is_tensor(palettes):
            palettes = torch.from_numpy(np.ascontiguousarray(palettes))
        if palettes.dtype != torch.uint8 or palettes.ndim != 3 or palettes.shape[0] != B or palettes.shape[2] != 3 or palettes.shape[1] < 1:
            raise ValueError(f"{fn}: palettes uint8[B, K_stride >= 1, 3] is expected")
        if not torch.is_tensor(k_rows):
            k_rows = torch.from_numpy(np.ascontiguousarray(k_rows, dtype=np.int32))
        if k_rows.dtype != torch.int32 or k_rows.numel() != B:
            raise ValueError(f"{fn}: k_rows int32[B] is expected")
        return palettes.to(self.device).contiguous(), k_rows.to(self.device).contiguous().reshape(-1)

    def palette_cells_batch(self, rgb, px_off, cls=None, n_classes=0, weights=None, px_off_dev=None):
        """palette_cells for B images that lie back to back in rgb (uint8[..., 3], numpy or device): image b is the pixels
        px_off[b] .. px_off[b + 1] (B + 1 host integers from 0 to the number of pixels; an image may be empty); cls, n_classes and
        weights as palette_cells takes them, cls over the same concatenation -> the device tables int64[B, 4, 32, 32, 32], table b
        what palette_cells gives for image b alone.  One launch, no read back."""
        rgb, off, off_dev, d_cls, n = self._batch_pixels("palette_cells_batch", rgb, px_off, px_off_dev, cls)
        B, n_classes = len(off) - 1, int(n_classes)
        w, warg = A.class_weights(weights, n_classes, "palette_cells_batch")
        A.class_map(d_cls, n, n_classes, self.device, "palette_cells_batch")
        if not 0 <= n_classes <= 16 or A.bad_weights(w):
            raise RhccqError("palette_cells_batch: n_classes must be 0..16 and weights 0..255 with one > 0")
        cells = self.empty((B,) + PALETTE_CELLS_SHAPE, torch.int64)
        if n == 0:                                       # (empty tensors have null pointers: nothing to launch)
            return cells.zero_()
        self._check(self.lib.rhccq_palette_cells_batch(self.ctx, self._p(rgb), C.c_void_p(off.ctypes.data), self._p(off_dev), B, self._p(d_cls), n_classes,
                                                       warg, self._p(cells)), "palette_cells_batch")
        return cells

    def palette_build_batch(self, cells, colours):
        """cells: the tables of palette_cells_batch (int64[B, 4, 32, 32, 32], numpy or device), colours = one K_target in
        1..palette_build_max_rows() for all of them -> (palettes device uint8[B, colours, 3], counts device int64[B, colours], splits
        device int32[B, colours - 1, 3], boxes device uint8[B, colours, 6], k device int32[B]): per image what palette_build gives,
        NOT trimmed and not read back: k[b] is the rows image b has (zero rows behind them), or the negative code of a table that is
        empty (-1) or adds up to more than 2^32 - 1 (-3), whose rows are all zero.  B chains run as B workgroups of one launch."""
        cells = A.cells_table(cells, "palette_build_batch")
        if cells.ndim != 5 or tuple(cells.shape[1:]) != PALETTE_CELLS_SHAPE or cells.shape[0] < 1:
            raise ValueError("palette_build_batch: cells [B >= 1, 4, 32, 32, 32] is expected")
        cells = cells.to(self.device).contiguous()
        B, target, cap = int(cells.shape[0]), int(colours), palette_build_max_rows()
        if target > cap:
            raise RhccqError(f"palette_build_batch: {target} colours, the device form returns at most {cap} (palette_build_max_rows())")
        if target < 1:
            raise RhccqError("palette_build_batch: colours >= 1 is required")
        wbytes = int(self._raw.rhccq_palette_build_batch_bytes(B))
        work = self.empty((wbytes // 8,), torch.int64)
        pal_out = self.empty((B, target, 3), torch.uint8)
        cnt_out = self.empty((B, target), torch.int64)
        boxes = self.empty((B, target, 6), torch.uint8)
        splits = self.empty((B, target - 1, 3), torch.int32)
        k_out = self.empty((B,), torch.int32)
        self._check(self.lib.rhccq_palette_build_batch(self.ctx, self._p(cells), B, target, self._p(work), wbytes, self._p(pal_out), self._p(cnt_out),
                                                       self._p(boxes), self._p(splits) if target > 1 else C.c_void_p(0), self._p(k_out)),
                    "palette_build_batch")
        return pal_out, cnt_out, splits, boxes, k_out

    def palette_remap_batch(self, rgb, px_off, palettes, k_rows, class_map=None, n_classes=0, px_off_dev=None):
        """palette_remap for B images laid out as palette_cells_batch takes them.  palettes uint8[B, K_stride, 3] and k_rows int32[B]
        (numpy or device; palette_build_batch's palettes and k go in as they are): image b is mapped onto rows 0 .. k_rows[b] - 1 of
        palettes[b], the rows behind them are never read, and an image with k_rows[b] < 1 gets index 0 and zero sums -> (indices
        device [pixels], concatenated like rgb: uint8 when K_stride <= 256, else int16 holding uint16; sums device int64
        [B, n_classes + 1, 2], rows as palette_remap's).  k_rows is read on the device: no read back."""
        rgb, off, off_dev, cls, n = self._batch_pixels("palette_remap_batch", rgb, px_off, px_off_dev, class_map)
        B, n_classes = len(off) - 1, int(n_classes)
        palettes, k_rows = self._batch_palettes("palette_remap_batch", palettes, k_rows, B)
        K = int(palettes.shape[1])
        A.class_map(cls, n, n_classes, self.device, "palette_remap_batch")
        if not 0 <= n_classes <= 16 or K > 65536:
            raise RhccqError("palette_remap_batch: K_stride must be 1..65536 and n_classes 0..16")
        idx = self.empty((n,), A.index_dtype(K))
        sums = self.empty((B, n_classes + 1, 2), torch.int64)
        if n == 0:                                       # (empty tensors have null pointers: nothing to launch)
            return idx, sums.zero_()
        self._check(self.lib.rhccq_palette_remap_batch(self.ctx, self._p(rgb), C.c_void_p(off.ctypes.data), self._p(off_dev), B, self._p(palettes), K,
                                                       self._p(k_rows), self._p(cls), n_classes, self._p(idx), idx.element_size(), self._p(sums)),
                    "palette_remap_batch")
        return idx, sums

    def palette_pattern_batch(self, rgb, px_off, widths, palettes, k_rows, strength, size=4, class_map=None, n_classes=0, px_off_dev=None):
        """palette_pattern for B images laid out as palette_cells_batch takes them; widths: B host integers, the width of every image
        (it divides the image's pixels; its rows and columns give the threshold's position); palettes uint8[B, K_stride, 3] and
        k_rows int32[B] as palette_remap_batch takes them (K_stride <= palette_pattern_max_rows(), else RhccqError); one strength
        (table), size and n_classes for the batch -> (indices device [pixels], concatenated like rgb: uint8 when K_stride <= 256, else
        int16 holding uint16; sums device int64[B, n_classes + 1, 3], rows as palette_pattern's).  Image b's part is bit for bit what
        palette_pattern gives for it alone; an image with k_rows[b] < 1 gets index 0 and zero sums.  One launch, no read back."""
        fn = "palette_pattern_batch"
        rgb, off, off_dev, cls, n = self._batch_pixels(fn, rgb, px_off, px_off_dev, class_map)
        B, n_classes = len(off) - 1, int(n_classes)
        palettes, k_rows = self._batch_palettes(fn, palettes, k_rows, B)
        K = int(palettes.shape[1])
        _, table = A.class_table(strength, n_classes, PATTERN_MAX, fn, "strength")
        size = self._pattern_size(size, fn)
        wid = np.ascontiguousarray(np.asarray(widths), dtype=np.int64).reshape(-1)
        px = np.diff(off)
        if len(wid) != B or (wid < 0).any() or (wid > INT_MAX).any() or ((px > 0) & ((wid < 1) | (px % np.maximum(wid, 1) != 0))).any():
            raise ValueError(f"{fn}: widths must hold one width per image that divides the image's pixels")
        wid = wid.astype(np.int32)
        A.class_map(cls, n, n_classes, self.device, fn)
        if not 0 <= n_classes <= 16 or K > palette_pattern_max_rows():
            raise RhccqError(f"{fn}: K_stride must be 1..{palette_pattern_max_rows()} on the device and n_classes 0..16")
        idx = self.empty((n,), A.index_dtype(K))
        sums = self.empty((B, n_classes + 1, 3), torch.int64)
        if n == 0:                                       # (empty tensors have null pointers: nothing to launch)
            return idx, sums.zero_()
        wid_dev = self.dev(wid)
        self._check(self.lib.rhccq_palette_pattern_batch(self.ctx, self._p(rgb), C.c_void_p(off.ctypes.data), self._p(off_dev), C.c_void_p(wid.ctypes.data),
                                                         self._p(wid_dev), B, self._p(palettes), K, self._p(k_rows), self._p(cls), n_classes, table, size,
                                                         self._p(idx), idx.element_size(), self._p(sums)), fn)
        return idx, sums

    def palette_refine_batch(self, rgb, px_off, palettes, k_rows, class_map=None, weights=None, max_iter=8, px_off_dev=None):
        """palette_refine for B images laid out as palette_cells_batch takes them, palettes and k_rows as palette_remap_batch takes
        them; class_map, weights and max_iter as palette_refine takes them, one table for the batch -> (palettes: a NEW device
        uint8[B, K_stride, 3], rows from k_rows[b] on copied unchanged; history device int64[B, max_iter, 2]; n_iter device int32[B]):
        per image what palette_refine gives for its k_rows[b] rows.  Images stop independently; an empty image, or one with
        k_rows[b] < 1, runs no iteration.  Two launches per iteration for the whole batch, no read back."""
        rgb, off, off_dev, cls, n = self._batch_pixels("palette_refine_batch", rgb, px_off, px_off_dev, class_map)
        B, max_iter = len(off) - 1, int(max_iter)
        palettes, k_rows = self._batch_palettes("palette_refine_batch", palettes, k_rows, B)
        K = int(palettes.shape[1])
        w, warg = A.class_weights(weights, None, "palette_refine_batch")
        n_classes = 0 if w is None else len(w) - 1
        A.class_map(cls, n, n_classes, self.device, "palette_refine_batch", without="class weights")
        if not 0 <= n_classes <= 16 or K > 65536 or not 1 <= max_iter <= 64 or A.bad_weights(w):
            raise RhccqError("palette_refine_batch: K_stride must be 1..65536, max_iter 1..64, weights 0..255 (n_classes + 1 <= 17 of them, one > 0)")
        out = palettes.clone()
        history = self.empty((B, max_iter, 2), torch.int64)
        n_iter = self.empty((B,), torch.int32)
        if n == 0:                                       # (empty tensors have null pointers: nothing to launch)
            return out, history.zero_(), n_iter.zero_()
        wbytes = int(self._raw.rhccq_palette_refine_batch_bytes(B, K))
        work = self.empty((wbytes // 8,), torch.int64)
        self._check(self.lib.rhccq_palette_refine_batch(self.ctx, self._p(rgb), C.c_void_p(off.ctypes.data), self._p(off_dev), B, self._p(out), K,
                                                        self._p(k_rows), self._p(cls), n_classes, warg, max_iter, self._p(work), wbytes,
                                                        self._p(history), self._p(n_iter)), "palette_refine_batch")
        return out, history, n_iter

    # -- the palette ladder: moments, the error curve of every rung, any rung from the log (EXTENSION: csrc/palette_ladder.hip) ----
    def _ladder_log(self, merges, K, fn):
        """the merges of palette_reduce (device int32[n_steps, 2], any n_steps <= K - 1) as the int32[max(K - 1, 1), 2] the C entries read"""
        merges = A.as_dtype(merges, torch.int32, self.device, fn, "merges")
        if merges.ndim != 2 or merges.shape[1] != 2 or merges.shape[0] > max(K - 1, 0):
            raise ValueError(f"{fn}: merges [n_steps <= K - 1, 2] is expected")
        full = torch.full((max(K - 1, 1), 2), -1, dtype=torch.int32, device=self.device)
        full[:merges.shape[0]] = merges
        return full

    def palette_moments(self, rgb, palette, class_map=None, n_classes=0, want_indices=True):
        """rgb uint8[..., 3], palette uint8[K, 3] (numpy or device), class_map uint8 / bool, one element per pixel, or None ->
        (indices as palette_remap returns them, or None with want_indices=False; moments device int64[n_classes + 1, K, 5]: per
        table and palette row {N, Sr, Sg, Sb, Q} of the pixels whose nearest row it is -- their number, their channel sums and
        the sum of r^2 + g^2 + b^2; table c over the pixels of class c, the last table over every pixel).  One pass; unweighted."""
        rgb, palette = A.pixels(rgb, palette, self.device, "palette_moments")
        n, K, n_classes = rgb.numel() // 3, int(palette.shape[0]), int(n_classes)
        cls = A.class_map(class_map, n, n_classes, self.device, "palette_moments")
        if not 0 <= n_classes <= 16 or K < 1 or K > 65536:
            raise RhccqError("palette_moments: K must be 1..65536 and n_classes 0..16")
        idx = self.empty(tuple(rgb.shape[:-1]), A.index_dtype(K)) if want_indices else None
        moments = self.empty((n_classes + 1, K, 5), torch.int64)
        if n == 0:                                       # (empty tensors have null pointers: nothing to launch)
            return idx, moments.zero_()
        self._check(self.lib.rhccq_palette_moments(self.ctx, self._p(rgb), n, self._p(palette), K, self._p(cls), n_classes, self._p(idx),
                                                   idx.element_size() if idx is not None else 0, self._p(moments)), "palette_moments")
        return idx, moments

    def palette_curve(self, palette, counts, merges, moments):
        """palette uint8[K, 3], counts [K] (the weights the chain was run with), merges int32[n_steps, 2] (palette_reduce's), moments
        int64[T, K, 5] (palette_moments') -> curve device int64[T, K]: curve[t, s] = the squared error of table t's pixels shown through
        the clusters after s merges, in exact integers; 0 behind the last step.  It bounds the error of the nearest-row remap onto
        that rung from above.  K above palette_reduce_max_rows() raises RhccqError."""
        palette = A.as_dtype(palette, torch.uint8, self.device, "palette_curve", "palette")
        counts = A.as_dtype(counts, torch.int64, self.device, "palette_curve", "counts")
        moments = A.as_dtype(moments, torch.int64, self.device, "palette_curve", "moments")
        K = A.counted_rows(palette, counts, "palette_curve")
        if moments.ndim != 3 or moments.shape[1] != K or moments.shape[2] != 5 or not 1 <= moments.shape[0] <= 17:
            raise ValueError("palette_curve: moments [1..17, K, 5] are expected")
        A.rows_cap(K, palette_reduce_max_rows(), "palette_curve")
        if K < 1:
            raise RhccqError("palette_curve: K >= 1 is required")
        merges = self._ladder_log(merges, K, "palette_curve")
        T = int(moments.shape[0])
        wbytes = int(self._raw.rhccq_palette_curve_bytes(K, T))
        work = self.empty((wbytes // 8,), torch.int64)
        curve = self.empty((T, K), torch.int64)
        self._check(self.lib.rhccq_palette_curve(self.ctx, self._p(palette), self._p(counts), K, self._p(merges), self._p(moments), T, self._p(work),
                                                 wbytes, self._p(curve)), "palette_curve")
        return curve

    def palette_rung(self, palette, counts, merges, colours):
        """palette uint8[K, 3], counts [K], merges int32[n_steps, 2] (palette_reduce's log of a run to fewer than `colours` rows),
        colours = K_target in 1..K -> (palette device uint8[k_out, 3], counts device int64[k_out], map device int32[K]): what
        palette_reduce(palette, counts, colours) returns, rebuilt from the log without the merge chain.  k_out is read back once.
        A log that ends before `colours` is reached gives the clusters it has (map names them all, the palette has the first
        `colours`).  K above palette_reduce_max_rows() raises RhccqError."""
        palette = A.as_dtype(palette, torch.uint8, self.device, "palette_rung", "palette")
        counts = A.as_dtype(counts, torch.int64, self.device, "palette_rung", "counts")
        K, target = A.counted_rows(palette, counts, "palette_rung"), int(colours)
        A.rows_cap(K, palette_reduce_max_rows(), "palette_rung")
        if K < 1 or not 1 <= target <= K:
            raise RhccqError("palette_rung: K >= 1 and colours in 1..K are required")
        merges = self._ladder_log(merges, K, "palette_rung")
        pal_out = self.empty((target, 3), torch.uint8)
        cnt_out = self.empty((target,), torch.int64)
        map_ = self.empty((K,), torch.int32)
        k_out = self.empty((1,), torch.int32)
        self._check(self.lib.rhccq_palette_rung(self.ctx, self._p(palette), self._p(counts), K, self._p(merges), target, self._p(pal_out),
                                                self._p(cnt_out), self._p(map_), self._p(k_out)), "palette_rung")
        k = min(A.k_out_rows(int(k_out.item()), "palette_rung"), target)       # the one read
        return pal_out[:k], cnt_out[:k], map_

    # -- split score (split_score.py:15-142) ----------------------------------------------------------
    def split_stats(self, rgb, mask=None):
        """rgb uint8[H,W,3] device, mask uint8[H,W] device or None -> (sums float64[12], lbp_hist int64[10], gray_hist int64[32])"""
        assert rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.shape[-1] == 3
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        nb = int(self.lib.rhccq_split_stats_blocks(H, W))
        part = self.empty((nb, 12), torch.float64)
        hist = self.empty((42,), torch.int32)
        self._check(self.lib.rhccq_split_stats(self.ctx, self._p(rgb), H, W, self._p(mask), self._p(part), nb, self._p(hist)), "split_stats")
        h = hist.cpu().numpy().astype(np.int64)
        return part.cpu().numpy().sum(axis=0), h[:10], h[10:]

    # -- ROI stage: connected components, buffer zone ---------------------------------------------------
    def ccl(self, mask, connectivity=8, cap=4096, numbering="opencv", host_stats=True):
        """mask uint8 / bool [H,W] device -> (n, labels int32[H,W] device, stats np.int32[n + 1, 5]) with cv2's conventions:
        label 0 = background, components numbered as cv2.connectedComponentsWithStats numbers them (csrc/ccl.hip), stats
        columns CC_STAT_LEFT, TOP, WIDTH, HEIGHT, AREA.  numbering="raster": components numbered by their first pixel in
        raster order (scipy.ndimage.label, skimage.measure.label); numbering="ids": unordered ids 1..n, no statistics (None)."""
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        assert mask.dtype == torch.uint8 and mask.dim() == 2 and mask.is_contiguous()
        H, W = int(mask.shape[0]), int(mask.shape[1])
        labels = self.empty((H, W), torch.int32)
        count = self.empty((1,), torch.int32)
        while True:
            wb = int(self.lib.rhccq_ccl_work_bytes(H, W, cap))
            work = self.empty((wb,), torch.uint8)
            stats = self.empty((cap + 1, 5), torch.int32)
            self._check(self.lib.rhccq_ccl(self.ctx, self._p(mask), H, W, int(connectivity), {"opencv": 0, "raster": 1, "ids": 2}[numbering], self._p(work),
                                           wb, cap, self._p(labels), self._p(None if numbering == "ids" else stats), self._p(count)), "ccl")
            n = int(count.cpu()[0])
            if n <= cap or numbering == "ids":
                break
            cap = n
        if numbering == "ids":
            return n, labels, None
        return n, labels, (stats[:n + 1].cpu().numpy() if host_stats else stats)   # host_stats=False: the device tensor [cap + 1][5]

    def ccl_keys(self, labels, n, y0, x0, frame_w, connectivity=8, numbering="opencv"):
        """-> np.uint32[n + 1]: the ordering key (frame coordinates) of every component of a tile labelled by ccl(); see rhccq_ccl_keys"""
        H, W = int(labels.shape[0]), int(labels.shape[1])
        keys = self.empty((n + 1,), torch.int32)
        self._check(self.lib.rhccq_ccl_keys(self.ctx, self._p(labels), H, W, int(y0), int(x0), int(frame_w), {"opencv": 0, "raster": 1}[numbering],
                                            int(connectivity), int(n), self._p(keys)), "ccl_keys")
        return keys.cpu().numpy().view(np.uint32)

    def ccl_select(self, labels, lut):
        """labels int32[H,W] device, lut uint8[n + 1] (numpy, or a device tensor) -> uint8[H,W] device = lut[labels]"""
        out = self.empty(tuple(labels.shape), torch.uint8)
        d_lut = lut if torch.is_tensor(lut) else self.dev(np.asarray(lut, np.uint8))   # (named: a temporary would be freed before the launch)
        self._check(self.lib.rhccq_ccl_select(self.ctx, self._p(labels), self._p(d_lut), labels.numel(), self._p(out)), "ccl_select")
        return out

    def roi_buffer(self, region_map, rgb, buffer_size=3):
        """extract_roi_nonroi on the device: -> (roi_image, nonroi_image uint8[H,W,3], roi_mask, nonroi_mask bool[H,W])"""
        assert region_map.dtype == torch.uint8 and rgb.dtype == torch.uint8 and region_map.is_contiguous() and rgb.is_contiguous()
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        assert tuple(region_map.shape) == (H, W) and rgb.shape[-1] == 3
        rm, nm = self.empty((H, W), torch.uint8), self.empty((H, W), torch.uint8)
        ri, ni = torch.empty_like(rgb), torch.empty_like(rgb)
        self._check(self.lib.rhccq_roi_buffer(self.ctx, self._p(region_map), self._p(rgb), H, W, int(buffer_size), self._p(rm), self._p(nm),
                                              self._p(ri), self._p(ni)), "roi_buffer")
        return ri, ni, rm.view(torch.bool), nm.view(torch.bool)

    # -- ROI stage: edge front end (csrc/edges.hip) -------------------------------------------------------
    def edges_gray(self, rgb):
        """rgb uint8[H,W,3] device -> (gray uint8[H,W] device, histogram np.int64[256])"""
        assert rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.shape[-1] == 3
        gray = self.empty(tuple(rgb.shape[:2]), torch.uint8)
        hist = self.empty((256,), torch.int32)
        self._check(self.lib.rhccq_edges_gray(self.ctx, self._p(rgb), gray.numel(), self._p(gray), self._p(hist)), "edges_gray")
        return gray, hist.cpu().numpy().astype(np.int64)

    def edges_grad_hist(self, gray):
        """gray uint8[H,W] device -> (values, counts): the distinct gx^2 + gy^2 of the 3x3 Sobel (BORDER_REFLECT_101), ascending"""
        H, W = int(gray.shape[0]), int(gray.shape[1])
        hist = self.empty((int(self.lib.rhccq_edges_m2_bins()),), torch.int32)
        self._check(self.lib.rhccq_edges_grad_hist(self.ctx, self._p(gray), H, W, self._p(hist)), "edges_grad_hist")
        h = self.to_host(hist)                               # (8 MB of bins: through a page-locked buffer)
        v = np.flatnonzero(h)
        return v.astype(np.int64), h[v].astype(np.int64)

    def canny_nms(self, img):
        """img uint8[H,W] or [H,W,3] device -> uint16[H,W] device (stored as int16): Canny's magnitude at the local maxima, 0 elsewhere"""
        assert img.dtype == torch.uint8 and img.is_contiguous()
        H, W = int(img.shape[0]), int(img.shape[1])
        cn = 1 if img.dim() == 2 else int(img.shape[2])
        mag, nm = self.empty((H, W), torch.int16), self.empty((H, W), torch.int16)
        dxy = self.empty((H, W), torch.int32)
        self._check(self.lib.rhccq_canny_nms(self.ctx, self._p(img), H, W, cn, self._p(mag), self._p(dxy), self._p(nm)), "canny_nms")
        return nm

    def canny_label(self, nm, low, gray=None):
        """first half of Canny's hysteresis on the device: components of {nm > low} (unordered ids: their numbering does not matter here) and
        per label the max of nm, the sums of gray and gray^2, the pixel count.  -> (n, labels int32[H,W] device, red device int64[n + 1][4]);
        only the component count crosses to the host"""
        H, W = int(nm.shape[0]), int(nm.shape[1])
        mask = self.empty((H, W), torch.uint8)
        self._check(self.lib.rhccq_edges_above(self.ctx, self._p(nm), H * W, int(low), self._p(mask)), "edges_above")
        n, labels, _ = self.ccl(mask, 8, cap=0, numbering="ids")
        red = self.empty((n + 1, 4), torch.int64)
        self._check(self.lib.rhccq_label_reduce(self.ctx, self._p(labels), self._p(nm), self._p(gray), labels.numel(), n, self._p(red)), "label_reduce")
        return n, labels, red

    def canny_verdict(self, n, red, high, want_lut=False):
        """second half: a component is an edge when its max exceeds `high`.  -> (lut uint8[n + 1] device or None, (edge components, edge
        pixels, sum gray, sum gray^2) as Python ints): 32 bytes cross to the host"""
        out4 = self.empty((4,), torch.int64)
        lut = self.empty((n + 1,), torch.uint8) if want_lut else None
        self._check(self.lib.rhccq_edge_score(self.ctx, self._p(red), n, int(high), self._p(out4), self._p(lut)), "edge_score")
        return lut, tuple(int(v) for v in out4.cpu().numpy())

    CANNY_SCORES_CAP = 1 << 20      # labels the fused scoring reduces per labelling (32 MB of per-label sums); beyond: the two-step path
    CANNY_SCORES_NESTED = True      # one union-find grown over the descending thresholds (rhccq_canny_scores_nested) instead of a labelling per `low`

    def canny_scores(self, nm, gray, pairs, nested=None):
        """[(edge components, edge pixels, sum gray, sum gray^2)] of several (low, high) pairs (normalised, low <= high) in ONE call and ONE
        read-back: rhccq_canny_scores_nested (every pixel linked once over the whole search), or with nested=False rhccq_canny_scores (pairs
        that share `low` share a labelling of {nm > low} from scratch) -- the same numbers"""
        H, W = int(nm.shape[0]), int(nm.shape[1])
        if self.CANNY_SCORES_NESTED if nested is None else nested:
            lows = (C.c_int32 * len(pairs))(*[int(p[0]) for p in pairs])
            highs = (C.c_int32 * len(pairs))(*[int(p[1]) for p in pairs])
            wb = int(self.lib.rhccq_canny_scores_nested_bytes(H, W))
            work = self.empty((wb,), torch.uint8)
            out = self.empty((len(pairs), 5), torch.int64)
            self._check(self.lib.rhccq_canny_scores_nested(self.ctx, self._p(nm), self._p(gray), H, W, lows, highs, len(pairs), self._p(work), wb, self._p(out)),
                        "canny_scores_nested")
            return [tuple(int(v) for v in row[:4]) for row in out.cpu().numpy()]
        order = sorted(range(len(pairs)), key=lambda i: pairs[i])
        lows = (C.c_int32 * len(pairs))(*[int(pairs[i][0]) for i in order])
        highs = (C.c_int32 * len(pairs))(*[int(pairs[i][1]) for i in order])
        cap = self.CANNY_SCORES_CAP
        wb = int(self.lib.rhccq_canny_scores_bytes(H, W, cap))
        work = self.empty((wb,), torch.uint8)
        out = self.empty((len(pairs), 5), torch.int64)
        self._check(self.lib.rhccq_canny_scores(self.ctx, self._p(nm), self._p(gray), H, W, lows, highs, len(pairs), cap, self._p(work), wb, self._p(out)),
                    "canny_scores")
        res = out.cpu().numpy()
        fours = [None] * len(pairs)
        for j, i in enumerate(order):
            if int(res[j, 4]) > cap:                              # more components than the fused reduction holds: score this pair the long way
                fours[i] = self.canny_components(nm, int(pairs[i][0]), int(pairs[i][1]), gray)[2]
            else:
                fours[i] = tuple(int(v) for v in res[j, :4])
        return fours

    def canny_components(self, nm, low, high, gray=None, want_lut=False):
        """both halves -> (labels, lut or None, the four numbers)"""
        n, labels, red = self.canny_label(nm, low, gray)
        lut, four = self.canny_verdict(n, red, high, want_lut)
        return labels, lut, four

    def label_reduce(self, labels, n, val16=None, val8=None):
        """-> np.uint64[n + 1, 4]: per label {max of val16, sum of val8, sum of val8^2, pixel count}"""
        red = self.empty((n + 1, 4), torch.int64)
        self._check(self.lib.rhccq_label_reduce(self.ctx, self._p(labels), self._p(val16), self._p(val8), labels.numel(), n, self._p(red)), "label_reduce")
        return red.cpu().numpy().view(np.uint64)

    def box_count(self, mask, kernel_size):
        """mask uint8 / bool [H,W] device -> uint16[H,W] device (int16 storage): non-zero pixels per k x k window, BORDER_REFLECT_101"""
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        H, W = int(mask.shape[0]), int(mask.shape[1])
        out = self.empty((H, W), torch.int16)
        self._check(self.lib.rhccq_box_count(self.ctx, self._p(mask), H, W, int(kernel_size), self._p(out)), "box_count")
        return out

    # -- ROI stage: clean-up chain (csrc/morph.hip); masks are uint8[H,W] device planes, set = non-zero, results 0 / 255 ----
    def morph(self, mask, half_widths, erode=False):
        """cv2.dilate / cv2.erode by the symmetric structuring element given as one half-width per row (-1 = empty row)"""
        H, W = int(mask.shape[0]), int(mask.shape[1])
        hw = (C.c_int32 * len(half_widths))(*[int(v) for v in half_widths])
        out = self.empty((H, W), torch.uint8)
        self._check(self.lib.rhccq_morph_dilate(self.ctx, self._p(mask), H, W, len(half_widths) // 2, hw, int(erode), int(erode), self._p(out)), "morph_dilate")
        return out

    def morph_close(self, mask, half_widths):
        return self.morph(self.morph(mask, half_widths), half_widths, erode=True)

    def morph_rect(self, mask, ksize, erode=False):
        """cv2.dilate / cv2.erode by a ksize x ksize rectangle, OpenCV's anchor ksize // 2 (an even element reaches one pixel
        further up / left than down / right)"""
        H, W = int(mask.shape[0]), int(mask.shape[1])
        a, b = int(ksize) // 2, int(ksize) - 1 - int(ksize) // 2
        left = (C.c_int32 * (a + b + 1))(*([a] * (a + b + 1)))
        right = (C.c_int32 * (a + b + 1))(*([b] * (a + b + 1)))
        out = self.empty((H, W), torch.uint8)
        self._check(self.lib.rhccq_morph_dilate_spans(self.ctx, self._p(mask), H, W, a, b, left, right, int(erode), int(erode), self._p(out)), "morph_dilate_spans")
        return out

    def morph_close_rect(self, mask, ksize):
        return self.morph_rect(self.morph_rect(mask, ksize), ksize, erode=True)

    def box_filter_seq(self, plane, kernel_size, scale255):
        """plane uint8[H,W] device -> float32[H,W] device: compute_local_density through OpenCV's direct filter2D path (odd kernels <= 11)"""
        H, W = int(plane.shape[0]), int(plane.shape[1])
        out = self.empty((H, W), torch.float32)
        self._check(self.lib.rhccq_box_filter_seq(self.ctx, self._p(plane), H, W, int(kernel_size), int(bool(scale255)), self._p(out)), "box_filter_seq")
        return out

    def lut_u16(self, values, table_u32):
        """values uint16 (int16 storage) device plane, table np.uint32[n] -> int32 device plane of table[value] (bit copies through rhccq_lut_u16_f32)"""
        t = self.dev(np.ascontiguousarray(table_u32, np.uint32).view(np.float32))
        out = self.empty(tuple(values.shape), torch.int32)
        self._check(self.lib.rhccq_lut_u16_f32(self.ctx, self._p(values), self._p(t), int(t.numel()), values.numel(), self._p(out)), "lut_u16_f32")
        return out

    def mask_op(self, a, b, op):
        """op: 'or', 'and', 'andnot' (a & ~b), 'not' (~a)"""
        out = torch.empty_like(a)
        self._check(self.lib.rhccq_mask_op(self.ctx, self._p(a), self._p(b), a.numel(), ("or", "and", "andnot", "not").index(op), self._p(out)), "mask_op")
        return out

    def gap_bridge(self, mask, counts, min_count, reach):
        out = torch.empty_like(mask)
        self._check(self.lib.rhccq_gap_bridge(self.ctx, self._p(mask), self._p(counts), counts.element_size(), int(mask.shape[0]), int(mask.shape[1]),
                                              int(min_count), int(reach), self._p(out)), "gap_bridge")
        return out

    def dist_chamfer(self, mask):
        """cv2.distanceTransform(mask, DIST_L2, 3) in fixed point (int32[H,W] device, 16 fractional bits)"""
        H, W = int(mask.shape[0]), int(mask.shape[1])
        hz = self.empty((H, W), torch.int16)
        dist = self.empty((H, W), torch.int32)
        self._check(self.lib.rhccq_dist_chamfer(self.ctx, self._p(mask), H, W, self._p(hz), self._p(dist)), "dist_chamfer")
        return dist

    def binary_sobel(self, mask):
        """-> (uint8[H,W] device: gx^2 + gy^2 of the 0/1 image's 3x3 Sobel, its maximum)"""
        H, W = int(mask.shape[0]), int(mask.shape[1])
        m2 = self.empty((H, W), torch.uint8)
        mx = self.empty((1,), torch.int32)
        self._check(self.lib.rhccq_binary_sobel(self.ctx, self._p(mask), H, W, self._p(m2), self._p(mx)), "binary_sobel")
        return m2, int(mx.cpu()[0])

    def lut_u8(self, plane, lut256):
        out = torch.empty_like(plane)
        d_lut = self.dev(np.asarray(lut256, np.uint8))
        self._check(self.lib.rhccq_lut_u8(self.ctx, self._p(plane), self._p(d_lut), plane.numel(), self._p(out)), "lut_u8")
        return out

    def box_sum(self, plane, kernel_size):
        """plane uint8[H,W] device -> int32[H,W] device: sum of the pixel values per k x k window, BORDER_REFLECT_101"""
        H, W = int(plane.shape[0]), int(plane.shape[1])
        out = self.empty((H, W), torch.int32)
        self._check(self.lib.rhccq_box_sum(self.ctx, self._p(plane), H, W, int(kernel_size), self._p(out)), "box_sum")
        return out

    def masked_hist(self, mask, values, n_bins):
        """-> np.int64[n_bins]: histogram of the uint16 plane (int16 storage) over the pixels where mask is set"""
        hist = self.empty((n_bins,), torch.int64)
        self._check(self.lib.rhccq_masked_hist(self.ctx, self._p(mask), self._p(values), values.numel(), int(n_bins), self._p(hist)), "masked_hist")
        return hist.cpu().numpy()

    def value_mask(self, values, min_value, mask=None):
        """-> uint8 plane: 255 where values >= min_value (and mask set, when given)"""
        out = self.empty(tuple(values.shape), torch.uint8)
        self._check(self.lib.rhccq_value_mask(self.ctx, self._p(mask), self._p(values), values.numel(), int(min_value), self._p(out)), "value_mask")
        return out

    def label_sum(self, labels, n, values):
        """-> np.uint64[n + 1]: per label (0 = background included) the sum of a uint16 (int16 storage) or non-negative int32 plane"""
        sums = self.empty((n + 1,), torch.int64)
        self._check(self.lib.rhccq_label_sum(self.ctx, self._p(labels), self._p(values), values.element_size(), labels.numel(), n, self._p(sums)), "label_sum")
        return sums.cpu().numpy().view(np.uint64)

    # -- K6 / decode ------------------------------------------------------------------------------
    def remap(self, idx, lut):
        out = torch.empty_like(idx)
        self._check(self.lib.rhccq_remap(self.ctx, self._p(idx), idx.numel(), self._p(lut), lut.numel(), self._p(out)), "remap")
        return out

    def decode(self, idx, palette):
        """palette uint8[K,3] device, idx uint8/uint16(int16 storage)/int32 device flat -> uint8[n,3]."""
        out = self.empty((idx.numel(), 3), torch.uint8)
        self._check(self.lib.rhccq_decode(self.ctx, self._p(idx), idx.element_size(), idx.numel(), self._p(palette),
                                          palette.shape[0], self._p(out)), "decode")
        return out

    # -- K5 ---------------------------------------------------------------------------------------
    def merge_firstpos(self, idx, h, w, top, left, canvas_h, canvas_w, pal_n):
        fp = torch.full((max(pal_n, 1),), INT_MAX, dtype=torch.int32, device=self.device)
        self._check(self.lib.rhccq_merge_firstpos(self.ctx, self._p(idx), h, w, top, left, canvas_h, canvas_w, pal_n, self._p(fp)),
                    "merge_firstpos")
        return fp[:pal_n]

    def merge_paint(self, idx, h, w, top, left, canvas, lut, pal_n):
        self._check(self.lib.rhccq_merge_paint(self.ctx, self._p(idx), h, w, top, left, canvas.shape[0], canvas.shape[1],
                                               self._p(lut), pal_n, self._p(canvas)), "merge_paint")

    # -- extension ----------------------------------------------------------------------------------
    def luma_qstep(self, rgb, roi_mask, block, q_roi, q_bg):
        H, W = rgb.shape[0], rgb.shape[1]
        luma = self.empty((H, W), torch.float32)
        qstep = self.empty((H // block, W // block), torch.float32)
        self._check(self.lib.rhccq_luma_qstep(self.ctx, self._p(rgb), self._p(roi_mask), H, W, block, float(q_roi), float(q_bg),
                                              self._p(luma), self._p(qstep)), "luma_qstep")
        return luma, qstep

    def dct_quant(self, plane, block, qstep, want_coef=True):
        H, W = plane.shape
        coef = self.empty((H, W), torch.float32) if want_coef else None
        q = self.empty((H, W), torch.int16)
        self._check(self.lib.rhccq_dct_quant(self.ctx, self._p(plane), H, W, block, self._p(qstep), self._p(coef), self._p(q)), "dct_quant")
        return coef, q

    # -- zlib (csrc/zlib_deflate.hip) -------------------------------------------------------------
    def zlib_sizes(self, n, exact=False):
        """-> (workspace bytes, worst-case output bytes) of a zlib stream of n input bytes (host only); exact=True: of the
        byte-exact level-9 encoder (csrc/zlib_deflate9.hip)"""
        ws, bound = C.c_int64(), C.c_int64()
        fn = self._raw.rhccq_zlib9_sizes if exact else self._raw.rhccq_zlib_sizes
        rc = fn(int(n), C.byref(ws), C.byref(bound))
        if rc:
            raise RhccqError(f"rhccq_zlib{'9' if exact else ''}_sizes({n}) failed ({rc})")
        return ws.value, bound.value

    def zlib_compress_async(self, t, out=None, workspace=None, exact=False):
        """contiguous device tensor (its raw bytes) -> (uint8 device buffer, int64 device length): the zlib stream is
        out[:length]; nothing waits for the device.  out / workspace: caller-owned uint8 device buffers (default: allocated
        at the sizes rhccq_zlib_sizes gives; an out smaller than the bound is refused).  exact=True: the stream is byte for
        byte zlib.compress(data, 9) (rhccq_zlib9_compress)"""
        if not t.is_cuda or not t.is_contiguous():
            raise RhccqError("zlib_compress: a contiguous device tensor is required")
        n = t.numel() * t.element_size()
        ws, bound = self.zlib_sizes(n, exact)
        work = self.empty((max(ws, 1),), torch.uint8) if workspace is None else workspace
        if work.numel() < ws:
            raise RhccqError(f"zlib_compress: workspace of {work.numel()} bytes, {ws} needed")
        out = self.empty((bound,), torch.uint8) if out is None else out
        length = self.empty((1,), torch.int64)
        fn = self.lib.rhccq_zlib9_compress if exact else self.lib.rhccq_zlib_compress
        self._check(fn(self.ctx, self._p(t), n, self._p(work), self._p(out), out.numel(), self._p(length)), "zlib_compress")
        return out, length

    def zlib9_stats(self, n, workspace):
        """after zlib_compress_async(exact=True) of n bytes with this workspace: (candidates examined, parse nodes, pointer
        jumping rounds, stored / fixed / dynamic blocks) as a host tuple (waits for the device)"""
        st = self.empty((6,), torch.int64)
        self._check(self.lib.rhccq_zlib9_stats(self.ctx, int(n), self._p(workspace), self._p(st)), "zlib9_stats")
        return tuple(int(v) for v in self.to_host(st))

    def zlib_compress(self, t, exact=False):
        """zlib stream (RFC 1950) of the raw bytes of a contiguous device tensor, as bytes: zlib.decompress() gives
        them back; format-compatible with zlib.compress, not byte-identical to it -- unless exact=True, which gives
        zlib.compress(data, 9) byte for byte"""
        out, length = self.zlib_compress_async(t, exact=exact)
        n = int(length.item())
        return self.to_host(out[:n]).tobytes()

    # -- indexed PNG files (EXTENSION: csrc/png_write.hip; include/rhccq.h pins the file) ----------------------------
    @staticmethod
    def _png_flags(exact=False, depth8=False, filter=True):
        return (1 if exact else 0) | (2 if depth8 else 0) | (0 if filter else 4)

    def _png_args(self, fn, indices, H, W, palette):
        H, W = int(H), int(W)
        palette = A.as_uint8(palette, self.device, fn, "palette")
        if palette.ndim != 2 or palette.shape[1] != 3:
            raise ValueError(f"{fn}: palette [K, 3] is expected")
        K = int(palette.shape[0])
        if H < 1 or W < 1 or not 1 <= K <= 65536:
            raise RhccqError(f"{fn}: H >= 1, W >= 1 and K 1..65536 are expected")
        return A.index_map(indices, H, W, self.device, fn), H, W, palette, K

    def png_sizes(self, H, W, K, exact=False, depth8=False, filter=True):
        """-> (scanline bytes, png_encode's workspace bytes, the file's bound) of an H x W map over K palette rows (host only)"""
        s, ws, bound = C.c_int64(), C.c_int64(), C.c_int64()
        rc = self._raw.rhccq_png_sizes(int(H), int(W), int(K), self._png_flags(exact, depth8, filter), C.byref(s), C.byref(ws), C.byref(bound))
        if rc:
            raise RhccqError(f"png_sizes: rhccq_png_sizes({H}, {W}, {K}) failed ({rc})")
        return s.value, ws.value, bound.value

    def png_scanlines(self, indices, H, W, palette, depth8=False, filter=True):
        """indices (H * W elements: uint8, int16 holding uint16, int32 / int64; numpy or device), palette uint8[K, 3] -> (scan uint8 device:
        the H filtered scanlines of the PNG file, filter_rows int64[5] device: rows per filter type).  K <= 256: packed indices at 1, 2,
        4 or 8 bits (depth8=True: 8), filter type 0; K > 256: palette[idx] as R G B under the row's cheapest filter (filter=False: type
        0).  An index >= K is written as 0.  One launch."""
        fn = "png_scanlines"
        idx, H, W, palette, K = self._png_args(fn, indices, H, W, palette)
        n = self.png_sizes(H, W, K, True, depth8, filter)[0]
        scan = self.empty((n,), torch.uint8)
        rows = self.empty((5,), torch.int64)
        self._check(self.lib.rhccq_png_scanlines(self.ctx, self._p(idx), idx.element_size(), H, W, self._p(palette), K,
                                                 self._png_flags(False, depth8, filter), self._p(scan), self._p(rows)), fn)
        return scan, rows

    def crc32_async(self, t, n=None):
        """contiguous device tensor (its raw bytes) -> the CRC-32 (zlib.crc32) as a device tensor of one int32 element holding the 32
        bits; n: a device int64 tensor with the number of leading bytes to take (clamped to the tensor), or None for all.  Two launches,
        nothing waits for the device."""
        if not t.is_cuda or not t.is_contiguous():
            raise RhccqError("crc32: a contiguous device tensor is required")
        cap = t.numel() * t.element_size()
        if n is not None and (not torch.is_tensor(n) or n.dtype != torch.int64 or not n.is_cuda or n.numel() != 1):
            raise RhccqError("crc32: n must be a device int64 tensor of one element")
        work = self.empty((max(int(self._raw.rhccq_crc32_bytes(cap)), 4),), torch.uint8)
        out = self.empty((1,), torch.int32)
        self._check(self.lib.rhccq_crc32(self.ctx, self._p(t) if cap else C.c_void_p(0), cap, self._p(n), self._p(work), self._p(out)), "crc32")
        return out

    def crc32(self, t, n=None):
        """zlib.crc32 of a contiguous device tensor's bytes (the first n of them: n an int, or a device int64 tensor) as a Python int"""
        if n is not None and not torch.is_tensor(n):
            n = int(n)
            if not 0 <= n <= t.numel() * t.element_size():
                raise ValueError("crc32: n must be 0..the tensor's bytes")
            t, n = t.reshape(-1).view(torch.uint8)[:n], None
        return int(self.to_host(self.crc32_async(t, n))[0]) & 0xFFFFFFFF

    def png_encode_async(self, indices, H, W, palette, exact=False, depth8=False, filter=True):
        """indices and palette as png_scanlines takes them -> (uint8 device buffer, int64 device length): the PNG file is
        out[:length] -- signature, IHDR, PLTE (K <= 256), one IDAT, IEND -- built on the device; nothing waits for it.  exact=True: IDAT
        is zlib.compress(scanlines, 9) byte for byte (the level-9 encoder), so the file is a function of the arguments alone."""
        return self._png_encode(indices, H, W, palette, exact, depth8, filter)[:2]

    def _png_encode(self, indices, H, W, palette, exact, depth8, filter):
        """-> (out, length, filter_rows int64[5] device: a view of the call's workspace)"""
        fn = "png_encode"
        idx, H, W, palette, K = self._png_args(fn, indices, H, W, palette)
        scan, ws, bound = self.png_sizes(H, W, K, exact, depth8, filter)
        work = self.empty((ws,), torch.uint8)
        out = self.empty((bound,), torch.uint8)
        length = self.empty((1,), torch.int64)
        self._check(self.lib.rhccq_png_encode(self.ctx, self._p(idx), idx.element_size(), H, W, self._p(palette), K,
                                              self._png_flags(exact, depth8, filter), self._p(work), self._p(out), bound, self._p(length)), fn)
        at = (scan + 255) // 256 * 256 + 16
        return out, length, work[at:at + 40].view(torch.int64)

    def png_encode(self, indices, H, W, palette, exact=False, depth8=False, filter=True):
        """png_encode_async's file as bytes: one read of the length, one copy of the file"""
        out, length = self.png_encode_async(indices, H, W, palette, exact, depth8, filter)
        return self.to_host(out[:int(length.item())]).tobytes()

    # -- GIF files (EXTENSION: csrc/gif_write.hip; include/rhccq.h pins the file) -------------------------------------
    @staticmethod
    def _gif_flags(local, delta, dictionary="hash"):
        if dictionary not in ("hash", "trie"):
            raise ValueError('gif: dictionary must be "hash" or "trie"')
        return (1 if local else 0) | (2 if delta else 0) | (4 if dictionary == "trie" else 0)

    def _gif_args(self, fn, frames, n, H, W, rows, local, delta, dictionary="hash"):
        """-> (flat device indices, the int32 rows array, flags); every refusal of the definition is a ValueError"""
        n, H, W = int(n), int(H), int(W)
        if n < 1:
            raise ValueError(f"{fn}: at least one frame is expected")
        if not (1 <= H <= 65535 and 1 <= W <= 65535):
            raise ValueError(f"{fn}: H and W must be 1..65535")
        rows = [int(k) for k in rows]
        if len(rows) != (n if local else 1):
            raise ValueError(f"{fn}: one row count per table is expected")
        if min(rows) < 1 or max(rows) > 256:
            raise ValueError(f"{fn}: a table must have 1..256 rows")
        if delta and local:
            raise ValueError(f"{fn}: delta needs a global table")
        if delta and rows[0] > 255:
            raise ValueError(f"{fn}: delta needs a table of at most 255 rows (the transparent index is one more entry)")
        return A.index_map(frames, n * H, W, self.device, fn), (C.c_int32 * len(rows))(*rows), self._gif_flags(local, delta, dictionary)

    def gif_sizes(self, n, H, W, local=False, delta=False):
        """-> (workspace bytes, the bound of one frame's code stream, the bound of the file) of n frames of H x W (host only)"""
        ws, stream, bound = C.c_int64(), C.c_int64(), C.c_int64()
        rc = self._raw.rhccq_gif_sizes(int(n), int(H), int(W), (1 if local else 0) | (2 if delta else 0), C.byref(ws), C.byref(stream), C.byref(bound))
        if rc:
            raise RhccqError(f"gif_sizes: rhccq_gif_sizes({n}, {H}, {W}) failed ({rc})")
        return ws.value, stream.value, bound.value

    def gif_lzw(self, frames, n, H, W, rows, local=False, delta=False, dictionary="hash"):
        """frames: n * H * W indices (uint8, int16 holding uint16, int32 / int64; numpy or device), rows: [K] or, local, one K a frame ->
        (streams uint8[n, bound] device, lengths int64[n] device): frame f's GIF code stream is streams[f, :lengths[f]] (include/rhccq.h:
        segments of gif_segment_pixels() pixels, each an LZW problem of one wave).  delta: a pixel that equals the frame in front is
        written as the transparent index K.  dictionary: "hash" (the open-addressed table, 32 KiB of LDS a segment) or "trie" (sibling-linked,
        16 KiB); the streams are the same.  Nothing waits for the device."""
        fn = "gif_lzw"
        idx, k_rows, flags = self._gif_args(fn, frames, n, H, W, rows, local, delta, dictionary)
        ws, stream, _ = self.gif_sizes(n, H, W, local, delta)
        work = self.empty((ws,), torch.uint8)
        out = self.empty((int(n), stream), torch.uint8)
        lengths = self.empty((int(n),), torch.int64)
        self._check(self.lib.rhccq_gif_lzw(self.ctx, self._p(idx), idx.element_size(), int(n), int(H), int(W), k_rows, flags, self._p(work), self._p(out),
                                           stream, self._p(lengths)), fn)
        return out, lengths

    def gif_encode_async(self, frames, n, H, W, palettes, rows=None, delays=4, loop=0, delta=False, dictionary="hash"):
        """frames as gif_lzw takes them; palettes uint8[K, 3] (ONE global table) or uint8[n, K_stride, 3] with rows = the rows of every
        frame's local table; delays: centiseconds, one number or one a frame -> (uint8 device buffer, int64 device length, int64[n] device
        stream lengths: a view of the call's workspace).  The GIF89a file is out[:length], built on the device; nothing waits for it.
        dictionary: as gif_lzw takes it."""
        fn = "gif_encode"
        palettes = A.as_uint8(palettes, self.device, fn, "palettes")
        local = palettes.ndim == 3
        if palettes.ndim not in (2, 3) or palettes.shape[-1] != 3 or (local and palettes.shape[0] != int(n)):
            raise ValueError(f"{fn}: palettes [K, 3] or [n, K, 3] are expected")
        if local and rows is None:
            rows = [palettes.shape[1]] * int(n)
        if not local:
            rows = [palettes.shape[0]]
        if palettes.shape[-2] > 256 or max(int(k) for k in rows) > palettes.shape[-2]:
            raise ValueError(f"{fn}: a table must have 1..256 rows, all of them in palettes")
        idx, k_rows, flags = self._gif_args(fn, frames, n, H, W, rows, local, delta, dictionary)
        n, H, W = int(n), int(H), int(W)
        delays = [int(delays)] * n if np.ndim(delays) == 0 else [int(d) for d in delays]
        if len(delays) != n or min(delays) < 0 or max(delays) > 65535:
            raise ValueError(f"{fn}: delays must be one number or one a frame, each 0..65535 centiseconds")
        if not 0 <= int(loop) <= 65535:
            raise ValueError(f"{fn}: loop must be 0..65535")
        ws, _, bound = self.gif_sizes(n, H, W, local, delta)
        work = self.empty((ws,), torch.uint8)
        out = self.empty((bound,), torch.uint8)
        length = self.empty((1,), torch.int64)
        self._check(self.lib.rhccq_gif_encode(self.ctx, self._p(idx), idx.element_size(), n, H, W, self._p(palettes), int(palettes.shape[-2]), k_rows,
                                              (C.c_int32 * n)(*delays), int(loop), flags, self._p(work), self._p(out), bound, self._p(length)), fn)
        return out, length, work[:8 * n].view(torch.int64)

    def gif_encode(self, frames, n, H, W, palettes, rows=None, delays=4, loop=0, delta=False):
        """gif_encode_async's file as bytes: one read of the length, one copy of the file"""
        out, length, _ = self.gif_encode_async(frames, n, H, W, palettes, rows, delays, loop, delta)
        return self.to_host(out[:int(length.item())]).tobytes()

    # -- PNG files read on the device (EXTENSION: csrc/png_read.hip; include/rhccq.h pins the definition) ----------------
    def _aligned_bytes(self, t, fn, what):
        """a uint8 tensor or array -> flat, contiguous, on the device and aligned to 16 (a view into a larger buffer is copied)"""
        t = A.as_uint8(t, self.device, fn, what).reshape(-1)
        return t.clone() if t.data_ptr() % 16 else t

    def crc32_segments(self, data, segments, extra=0):
        """data: uint8 (device or numpy); segments: (offset, length) pairs -> a device int32 tensor holding zlib.crc32 of every
        data[offset : offset + length + extra] (its 32 bits), in two launches whatever their number; a range outside data counts as
        empty.  Nothing waits for the device."""
        fn = "crc32_segments"
        data = self._aligned_bytes(data, fn, "data")
        seg = np.ascontiguousarray(segments, dtype=np.int64).reshape(-1, 2)
        table = np.zeros((len(seg), 4), np.int64)
        table[:, :2] = seg
        total = C.c_int64()
        rc = self._raw.rhccq_crc32_segments_plan(C.c_void_p(table.ctypes.data), len(table), int(extra), C.byref(total))
        if rc:
            raise RhccqError(f"{fn}: rhccq_crc32_segments_plan failed ({rc}): extra >= 0 is expected")
        out = self.empty((max(len(table), 1),), torch.int32)
        work = self.empty((max(total.value, 1),), torch.int32)
        table_dev = self.dev(table.reshape(-1))
        self._check(self.lib.rhccq_crc32_segments(self.ctx, self._p(data), data.numel(), self._p(table_dev), len(table), int(extra), total.value,
                                                  self._p(work), self._p(out)), fn)
        return out[:len(table)]

    def png_unfilter(self, scan, H, rowbytes, bpp, out=None):
        """scan: uint8, H scanlines of 1 + rowbytes bytes (a filter type byte and the filtered bytes) -> (raw uint8[H * rowbytes] device,
        status int32[2] device: PNG_STATUS index -- OK, BAD_FILTER (a type byte above 4: that row is copied) or STALLED -- and its
        detail).  bpp: bytes of a filter unit, 1, 2, 3, 4, 6 or 8; rowbytes a multiple of it.  out: a caller's uint8 device buffer."""
        fn = "png_unfilter"
        H, rowbytes, bpp = int(H), int(rowbytes), int(bpp)
        scan = A.as_uint8(scan, self.device, fn, "scan").reshape(-1)
        ws = int(self._raw.rhccq_png_unfilter_bytes(H, rowbytes, bpp)) if 0 < H <= INT_MAX else -1
        if ws < 0:
            raise RhccqError(f"{fn}: H >= 1, rowbytes >= 1 a multiple of bpp, bpp 1, 2, 3, 4, 6 or 8 and scanlines below 2 GiB are expected")
        if scan.numel() != H * (rowbytes + 1):
            raise ValueError(f"{fn}: scan must have H * (rowbytes + 1) bytes")
        raw = self.empty((H * rowbytes,), torch.uint8) if out is None else out
        if raw.dtype != torch.uint8 or not raw.is_cuda or not raw.is_contiguous() or raw.numel() != H * rowbytes:
            raise ValueError(f"{fn}: out must be a contiguous uint8 device tensor of H * rowbytes bytes")
        work = self.empty((ws // 4,), torch.int32)
        status = self.empty((2,), torch.int32)
        self._check(self.lib.rhccq_png_unfilter(self.ctx, self._p(scan), H, rowbytes, bpp, self._p(raw), self._p(work), self._p(status)), fn)
        return raw, status

    def png_expand(self, raw, H, W, colour_type, depth, palette=None, trns=None):
        """raw rows (uint8, H rows of ceil(W channels depth / 8) bytes) -> (rgb uint8[H, W, 3], alpha uint8[H, W], indices uint8[H, W] or
        None unless colour type 3), all on the device.  palette uint8[K, 3] (colour type 3), trns: the bytes of a tRNS chunk or None."""
        fn = "png_expand"
        H, W, ct, depth = int(H), int(W), int(colour_type), int(depth)
        raw = A.as_uint8(raw, self.device, fn, "raw").reshape(-1)
        channels = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}.get(ct)
        if H < 1 or W < 1 or channels is None or depth not in (1, 2, 4, 8, 16):
            raise RhccqError(f"{fn}: H >= 1, W >= 1 and a colour type and depth PNG allows are expected")
        if raw.numel() != H * ((W * channels * depth + 7) // 8):
            raise ValueError(f"{fn}: raw must have H * ceil(W * channels * depth / 8) bytes")
        K = 0
        if ct == 3:
            if palette is None:
                raise ValueError(f"{fn}: colour type 3 needs a palette")
            palette = A.as_uint8(palette, self.device, fn, "palette")
            if palette.ndim != 2 or palette.shape[1] != 3:
                raise ValueError(f"{fn}: palette [K, 3] is expected")
            K = int(palette.shape[0])
        t = None if trns is None or len(trns) == 0 else A.as_uint8(np.frombuffer(bytes(trns), np.uint8) if not torch.is_tensor(trns) else trns, self.device, fn, "trns")
        rgb = self.empty((H, W, 3), torch.uint8)
        alpha = self.empty((H, W), torch.uint8)
        idx = self.empty((H, W), torch.uint8) if ct == 3 else None
        self._check(self.lib.rhccq_png_expand(self.ctx, self._p(raw), H, W, ct, depth, self._p(palette) if ct == 3 else C.c_void_p(0), K,
                                              self._p(t), 0 if t is None else t.numel(), self._p(rgb), self._p(alpha), self._p(idx)), fn)
        return rgb, alpha, idx

    def png_decode(self, file, info=None, table=None, check_crc=True):
        """file: the PNG file's bytes as a uint8 device tensor (or bytes / numpy, uploaded); info, table: png_parse's (parsed from the
        bytes when None, which reads a device tensor back) -> {"rgb" uint8[H, W, 3], "alpha" uint8[H, W] or None, "indices"
        uint8[H, W] or None, "status" int32[2] (PNG_STATUS index, detail), "scan": the inflated scanlines, "file": the bytes on the
        device}, all on the device; nothing waits for it.  With a status the framing shows (info.status) there are no outputs."""
        fn = "png_decode"
        if info is None:
            host = self.to_host(file).tobytes() if torch.is_tensor(file) else bytearray(file)
            info, table = png_parse(host)
            if not torch.is_tensor(file):
                file = np.frombuffer(host, np.uint8)
        status = self.empty((2,), torch.int32)
        if info.status:
            self._check(self.lib.rhccq_png_decode(self.ctx, C.c_void_p(0), 0, C.byref(info), C.c_void_p(0), 0, C.c_void_p(0), C.c_void_p(0),
                                                  C.c_void_p(0), C.c_void_p(0), self._p(status)), fn)
            return {"rgb": None, "alpha": None, "indices": None, "status": status, "scan": None, "file": None}
        file = self._aligned_bytes(file, fn, "file")
        n = file.numel()
        table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 4)
        if len(table) != info.n_chunks:
            raise ValueError(f"{fn}: the table must have info.n_chunks rows")
        ws = C.c_int64()
        rc = self._raw.rhccq_png_read_sizes(C.byref(info), n, C.byref(ws))
        if rc:
            raise RhccqError(f"{fn}: rhccq_png_read_sizes failed ({rc}): info does not describe a file of {n} bytes")
        H, W, ct = info.height, info.width, info.colour_type
        has_alpha = ct in (4, 6) or info.trns_bytes > 0
        work = self.empty((ws.value,), torch.uint8)
        table_dev = self.dev(table.reshape(-1))
        rgb = self.empty((H, W, 3), torch.uint8)
        alpha = self.empty((H, W), torch.uint8) if has_alpha else None
        idx = self.empty((H, W), torch.uint8) if ct == 3 else None
        self._check(self.lib.rhccq_png_decode(self.ctx, self._p(file), n, C.byref(info), self._p(table_dev), 0 if check_crc else 1, self._p(work),
                                              self._p(rgb), self._p(alpha), self._p(idx), self._p(status)), fn)
        at = int(self._raw.rhccq_png_read_scan_offset(C.byref(info)))
        return {"rgb": rgb, "alpha": alpha, "indices": idx, "status": status, "scan": work[at:at + info.scan_bytes], "file": file}

    # -- GIF files read on the device (EXTENSION: csrc/gif_read.hip; include/rhccq.h pins the definition) ----------------
    def _gif_out(self, fn, what, t, shape):
        """a caller's output buffer (a contiguous uint8 device tensor of `shape`'s size), or a new one"""
        if t is None:
            return self.empty(shape, torch.uint8)
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.numel() != int(np.prod(shape)):
            raise ValueError(f"{fn}: {what} must be a contiguous uint8 device tensor of {int(np.prod(shape))} bytes")
        return t

    def _gif_frames(self, fn, frames, n_frames):
        n_frames = int(n_frames)
        if not isinstance(frames, C.Array) or frames._type_ is not _lib.GifFrame or not 1 <= n_frames <= len(frames):
            raise ValueError(f"{fn}: frames must be gif_parse's array and 1 <= n_frames <= its length")
        return n_frames, self.dev(gif_frames_array(frames, n_frames))

    def gif_unlzw(self, streams, frames, n_frames, pixels=None):
        """streams: the joined code streams (uint8, laid out as gif_parse's frames say: every frame's at a 16-byte aligned offset, 16 bytes
        or more behind it); frames: gif_parse's array -> (pixels uint8[sum of w h] device: frame f's strings in stream order from
        frames[f].pixel_offset, counts int64[n_frames] device, status int32[2] device: GIF_READ_STATUS index -- OK, BAD_CODE, BAD_LENGTH --
        and the frame, head int32[4] device: the fault words and the number of segments).  pixels: a caller's buffer.  Nothing waits."""
        fn = "gif_unlzw"
        n_frames, frames_dev = self._gif_frames(fn, frames, n_frames)
        streams = self._aligned_bytes(streams, fn, "streams")
        n_pixels = sum(int(frames[f].w) * int(frames[f].h) for f in range(n_frames))
        ws = int(self._raw.rhccq_gif_unlzw_bytes(C.cast(frames, C.c_void_p), n_frames))
        if ws < 0:
            raise RhccqError(f"{fn}: rhccq_gif_unlzw_bytes failed ({ws}): the frame table is not gif_parse's")
        pixels = self._gif_out(fn, "pixels", pixels, (max(n_pixels, 1),))
        work = self.empty((ws,), torch.uint8)
        counts = self.empty((n_frames,), torch.int64)
        status = self.empty((2,), torch.int32)
        self._check(self.lib.rhccq_gif_unlzw(self.ctx, self._p(streams), streams.numel(), C.cast(frames, C.c_void_p), self._p(frames_dev), n_frames,
                                             self._p(work), self._p(pixels), n_pixels, self._p(counts), self._p(status)), fn)
        return pixels, counts, status, work[:16].view(torch.int32)

    def gif_compose(self, pixels, file, frames, n_frames, H, W, rgb=None, alpha=None, idx=None, want_idx=True):
        """pixels as gif_unlzw leaves them, file: the GIF file's bytes (the colour tables are read from it), frames: gif_parse's array ->
        (rgb uint8[F, H, W, 3], alpha uint8[F, H, W], idx uint8[sum of w h]: every frame's de-interlaced indices from its pixel_offset,
        None with want_idx=False) on the device.  rgb, alpha, idx: a caller's buffers."""
        fn = "gif_compose"
        n_frames, frames_dev = self._gif_frames(fn, frames, n_frames)
        H, W = int(H), int(W)
        if not (1 <= H <= 65535 and 1 <= W <= 65535):
            raise ValueError(f"{fn}: H and W must be 1..65535")
        pixels = A.as_uint8(pixels, self.device, fn, "pixels").reshape(-1)
        file = A.as_uint8(file, self.device, fn, "file").reshape(-1)
        rgb = self._gif_out(fn, "rgb", rgb, (n_frames, H, W, 3))
        alpha = self._gif_out(fn, "alpha", alpha, (n_frames, H, W))
        idx = self._gif_out(fn, "idx", idx, (max(pixels.numel(), 1),)) if want_idx or idx is not None else None
        self._check(self.lib.rhccq_gif_compose(self.ctx, self._p(pixels), pixels.numel(), self._p(file), file.numel(), self._p(frames_dev), n_frames, H, W,
                                               self._p(rgb), self._p(alpha), self._p(idx)), fn)
        return rgb, alpha, idx

    def gif_decode(self, file, parsed=None, rgb=None, alpha=None, idx=None):
        """file: the GIF file's bytes as a uint8 device tensor (or bytes / numpy, uploaded); parsed: gif_parse's triple (parsed from the
        bytes when None, which reads a device tensor back) -> {"rgb" uint8[F, H, W, 3], "alpha" uint8[F, H, W], "indices" uint8[sum of
        w h] (frame f's de-interlaced h x w map from its pixel_offset), "status" int32[2] (GIF_READ_STATUS index, detail), "head" int32[4]
        (the fault words, the segments of all frames), "file": the bytes on the device, "info", "frames"}; nothing waits for the device.
        With a status the framing shows (info.status) there are no outputs.  rgb, alpha, idx: a caller's buffers."""
        fn = "gif_decode"
        if parsed is None:
            host = self.to_host(file).tobytes() if torch.is_tensor(file) else bytearray(file)
            parsed = gif_parse(host)
            if not torch.is_tensor(file):
                file = np.frombuffer(host, np.uint8)
        info, frames, blocks = parsed
        if not torch.is_tensor(file) and not isinstance(file, np.ndarray):
            file = np.frombuffer(bytes(file), np.uint8).copy()
        status = self.empty((2,), torch.int32)
        null = C.c_void_p(0)
        if info.status:
            self._check(self.lib.rhccq_gif_decode(self.ctx, null, 0, C.byref(info), null, null, null, null, null, null, null, self._p(status)), fn)
            return {"rgb": None, "alpha": None, "indices": None, "status": status, "head": None, "file": None, "info": info, "frames": frames}
        file = A.as_uint8(file, self.device, fn, "file").reshape(-1)                 # (any alignment: the kernels read it byte by byte)
        n, F, H, W = file.numel(), info.n_frames, info.height, info.width
        ws = C.c_int64()
        rc = self._raw.rhccq_gif_read_sizes(C.byref(info), n, C.byref(ws))
        if rc:
            raise RhccqError(f"{fn}: rhccq_gif_read_sizes failed ({rc}): info does not describe a file of {n} bytes")
        blocks = np.ascontiguousarray(blocks, dtype=np.int64).reshape(-1, 4)
        if len(blocks) != info.n_blocks:
            raise ValueError(f"{fn}: the sub-block table must have info.n_blocks rows")
        _, frames_dev = self._gif_frames(fn, frames, F)
        blocks_dev = self.dev(blocks.reshape(-1)) if len(blocks) else None
        work = self.empty((ws.value,), torch.uint8)
        rgb = self._gif_out(fn, "rgb", rgb, (F, H, W, 3))
        alpha = self._gif_out(fn, "alpha", alpha, (F, H, W))
        idx = self._gif_out(fn, "idx", idx, (info.pixels,))
        self._check(self.lib.rhccq_gif_decode(self.ctx, self._p(file), n, C.byref(info), C.cast(frames, C.c_void_p), self._p(frames_dev), self._p(blocks_dev),
                                              self._p(work), self._p(rgb), self._p(alpha), self._p(idx), self._p(status)), fn)
        return {"rgb": rgb, "alpha": alpha, "indices": idx, "status": status, "head": work[:16].view(torch.int32), "file": file, "info": info,
                "frames": frames}

    # -- zlib inflate (csrc/zlib_inflate.hip) ------------------------------------------------------------
    ZS_OK, ZS_BAD_HEADER, ZS_BAD_DATA, ZS_TRUNCATED, ZS_ADLER, ZS_CAPACITY = 0, 1, 2, 3, 4, 5
    _ZS_MSG = {1: "incorrect header check", 2: "invalid block type, code lengths, symbol or distance",
               3: "incomplete or truncated stream", 4: "incorrect data check"}

    def zlib_inflate_sizes(self, n, out_cap):
        """-> workspace bytes for decoding n compressed bytes into at most out_cap bytes (host only)"""
        ws = C.c_int64()
        rc = self._raw.rhccq_zlib_inflate_sizes(int(n), int(out_cap), C.byref(ws))
        if rc:
            raise RhccqError(f"rhccq_zlib_inflate_sizes({n}, {out_cap}) failed ({rc})")
        return ws.value

    def _zbuf(self, buf):
        """bytes-like or uint8 device tensor -> contiguous uint8 device tensor"""
        if isinstance(buf, torch.Tensor):
            if not buf.is_cuda or buf.dtype != torch.uint8:
                raise RhccqError("zlib_decompress: a uint8 device tensor or a bytes-like object is required")
            return buf.reshape(-1).contiguous()
        return self.dev(np.frombuffer(bytes(buf), dtype=np.uint8))

    def zlib_decompress_async(self, buf, out_cap, out=None, workspace=None):
        """zlib stream (bytes-like or uint8 device tensor) -> (uint8 device out, int64 device length, int32 device status):
        the decoded bytes are out[:length] when status is ZS_OK; on ZS_CAPACITY length is the size needed.  Nothing waits
        for the device.  out / workspace: caller-owned uint8 device buffers (default: allocated at out_cap and
        zlib_inflate_sizes)."""
        src = self._zbuf(buf)
        n, cap = src.numel(), int(out_cap)
        ws = self.zlib_inflate_sizes(n, cap)
        work = self.empty((max(ws, 1),), torch.uint8) if workspace is None else workspace
        if work.numel() < ws:
            raise RhccqError(f"zlib_decompress: workspace of {work.numel()} bytes, {ws} needed")
        out = self.empty((max(cap, 1),), torch.uint8) if out is None else out
        if out.numel() < cap:
            raise RhccqError(f"zlib_decompress: out of {out.numel()} bytes, out_cap {cap}")
        length = self.empty((1,), torch.int64)
        status = self.empty((1,), torch.int32)
        self._check(self.lib.rhccq_zlib_decompress(self.ctx, self._p(src), n, self._p(work), self._p(out), cap, self._p(length),
                                                   self._p(status)), "zlib_decompress")
        self.__dict__["_zlast"] = (n, cap, work)
        return out, length, status

    def zlib_inflate_stats(self):
        """after zlib_decompress(_async): (candidates, candidates whose decode failed, chained workers, blocks on the chain)"""
        n, cap, work = self._zlast
        st = self.empty((4,), torch.int64)
        self._check(self.lib.rhccq_zlib_inflate_stats(self.ctx, n, cap, self._p(work), self._p(st)), "zlib_inflate_stats")
        return tuple(int(v) for v in self.to_host(st))

    def zlib_decompress(self, buf, out_cap=None):
        """zlib.decompress on the device: -> uint8 device tensor of the exact decoded length.  A bad stream raises RhccqError
        with zlib's wording.  Without out_cap the first try is sized from the input, and a stream that decodes to more is
        decoded once more at the length it reported."""
        src = self._zbuf(buf)
        cap = int(out_cap) if out_cap is not None else min(4 * src.numel() + 65536, (1 << 31) - 1)
        for attempt in range(2):
            out, length, status = self.zlib_decompress_async(src, cap)
            ln, st = (int(v[0]) for v in self.to_host(length, status))
            if st == self.ZS_CAPACITY and out_cap is None and attempt == 0:
                if ln > (1 << 31) - 1:
                    raise RhccqError(f"Error -3 while decompressing data: output of {ln} bytes is beyond the 2 GiB limit")
                cap = ln
                continue
            break
        if st == self.ZS_CAPACITY:
            raise RhccqError(f"Error -5 while decompressing data: output of {ln} bytes exceeds out_cap {cap}")
        if st != self.ZS_OK:
            code = -5 if st == self.ZS_TRUNCATED else -3
            raise RhccqError(f"Error {code} while decompressing data: {self._ZS_MSG.get(st, f'status {st}')}")
        return out[:ln]

    def sync(self):
        self._check(self.lib.rhccq_sync(self.ctx), "sync")


_default = {}


def default_context(device=None):
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    if device not in _default:
        _default[device] = Rhccq(device)
    return _default[device]
