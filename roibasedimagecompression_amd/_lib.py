"""ctypes binding of librhccq_hip.so (C ABI declared in include/rhccq.h).

The product path has NO CPU fallback: if the library is missing or a GPU is not present the
functions below raise.  (The CPU oracle lives in oracle/ and is test infrastructure only.)
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librhccq_hip.so")

_lib = None

c_void_p, c_int32, c_int64, c_double, c_float, c_uint64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_float, C.c_uint64


class MbkProblem(C.Structure):
    """struct rhccq_mbk_problem (include/rhccq.h)."""
    _fields_ = [("off", c_int64), ("n", c_int64), ("k", c_int64), ("koff", c_int64), ("init_off", c_int64),
                ("init_n", c_int64), ("rand_off", c_int64), ("first", c_int32), ("T", c_int32)]


class MbkDraw(C.Structure):
    """struct rhccq_mbk_draw (include/rhccq.h): what a MiniBatchKMeans fit fixes ahead of its k-means++ chain"""
    _fields_ = [("batch", c_int64), ("limit", c_int64), ("init_size", c_int64), ("n_uniforms", c_int64), ("pos", c_int64),
                ("cursor0", c_int64), ("T", c_int32), ("first", c_int32)]


class ClassDesc(C.Structure):
    """struct rhccq_class_desc (include/rhccq.h): one region class of a frame for rhccq_encode_frame"""
    _fields_ = [("labels", c_void_p), ("n_seg", c_int32), ("n_region", c_int32), ("seg_region", c_void_p), ("region_bbox", c_void_p),
                ("quality", c_int32), ("reserved", c_int32)]


class Segment(C.Structure):
    """struct rhccq_segment (include/rhccq.h): a byte range of one buffer; a PNG chunk"""
    _fields_ = [("offset", c_int64), ("length", c_int64), ("first_piece", c_int64), ("dst", c_int64)]


class PngInfo(C.Structure):
    """struct rhccq_png_info (include/rhccq.h): what rhccq_png_parse_host reads from a file's framing"""
    _fields_ = [("status", c_int32), ("detail", c_int32), ("width", c_int32), ("height", c_int32), ("depth", c_int32), ("colour_type", c_int32),
                ("interlace", c_int32), ("channels", c_int32), ("bpp", c_int32), ("palette_rows", c_int32), ("trns_bytes", c_int32),
                ("n_chunks", c_int32), ("first_idat", c_int32), ("n_idat", c_int32), ("rowbytes", c_int64), ("scan_bytes", c_int64),
                ("plte_offset", c_int64), ("trns_offset", c_int64), ("idat_bytes", c_int64), ("crc_pieces", c_int64)]


class GifInfo(C.Structure):
    """struct rhccq_gif_info (include/rhccq.h): what rhccq_gif_parse_host reads from a file's framing"""
    _fields_ = [("status", c_int32), ("detail", c_int32), ("width", c_int32), ("height", c_int32), ("global_rows", c_int32), ("loop", c_int32),
                ("n_frames", c_int32), ("n_blocks", c_int32), ("global_offset", c_int64), ("stream_bytes", c_int64), ("pixels", c_int64),
                ("seg_rows", c_int64)]


class GifFrame(C.Structure):
    """struct rhccq_gif_frame (include/rhccq.h): one image of a GIF file"""
    _fields_ = [("x", c_int32), ("y", c_int32), ("w", c_int32), ("h", c_int32), ("m", c_int32), ("interlace", c_int32), ("table_rows", c_int32),
                ("transparent", c_int32), ("disposal", c_int32), ("delay", c_int32), ("first_block", c_int32), ("n_blocks", c_int32),
                ("table_offset", c_int64), ("stream_offset", c_int64), ("stream_bytes", c_int64), ("pixel_offset", c_int64), ("first_row", c_int64)]


class FrameResult(C.Structure):
    """struct rhccq_frame_result (include/rhccq.h)"""
    _fields_ = [("n_colours", c_int32), ("index_bytes", c_int32), ("shape", c_int32 * 2), ("top_left", c_int32 * 2), ("quality3", c_int32),
                ("n_jobs", c_int32), ("ms", c_double * 8), ("class_ms", (c_double * 4) * 4)]


# name -> (restype, argtypes).  Every symbol include/rhccq.h declares is listed here; the CPU test
# suite checks that the library exports all of them.
PROTOTYPES = {
    "rhccq_abi_version": (c_int32, []),
    "rhccq_ctx_create": (c_int32, [c_int32, c_void_p, C.POINTER(c_void_p)]),
    "rhccq_ctx_destroy": (None, [c_void_p]),
    "rhccq_last_error": (C.c_char_p, [c_void_p]),
    "rhccq_ctx_set_int": (c_int32, [c_void_p, c_int32, c_int64]),
    "rhccq_sync": (c_int32, [c_void_p]),
    "rhccq_stream": (c_void_p, [c_void_p]),
    "rhccq_ctx_set_stream": (c_int32, [c_void_p, c_void_p]),
    "rhccq_params": (c_int32, [c_int64, c_double, C.POINTER(c_double), C.POINTER(c_int64)]),
    "rhccq_eps_threshold": (c_int32, [c_double, C.POINTER(c_int32), C.POINTER(c_int32), C.POINTER(c_double)]),
    "rhccq_job_scan": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32),
                                 c_int32, c_void_p, c_void_p]),
    "rhccq_job_scan_bytes": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32),
                                       c_int32, c_void_p, c_void_p]),
    "rhccq_bytemap_pack": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p]),
    "rhccq_job_set_black": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32]),
    "rhccq_bitmap_count": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "rhccq_bitmap_emit": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_job_blackfix": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32),
                                     c_void_p, c_void_p]),
    "rhccq_job_index": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32),
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_job_index_entries": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32), c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_frame_remap_entries": (c_int32, [c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32), c_void_p, c_void_p, c_int32,
                                            c_void_p, c_int32]),
    "rhccq_job_stats": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32), c_void_p]),
    "rhccq_job_sort_unique_bytes": (c_int64, [c_int64]),
    "rhccq_job_sort_unique": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32), c_int32, c_void_p, c_void_p,
                                        c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_job_index_ranked": (c_int32, [c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32), c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_frame_remap_ranked": (c_int32, [c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32), c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int32, c_void_p, c_int32]),
    "rhccq_eps_components": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "rhccq_cluster_sums": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "rhccq_cluster_means": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_kmeans": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_mbk_init": (c_int32, [c_void_p, c_void_p, C.POINTER(MbkProblem), c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_mbk_init_released": (c_int32, [c_void_p, c_void_p, C.POINTER(MbkProblem), c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, C.c_uint32, C.POINTER(c_int32)]),
    "rhccq_release_flags_alloc": (c_int32, [c_int32, C.POINTER(c_void_p), C.POINTER(c_void_p)]),
    "rhccq_release_flags_free": (None, [c_void_p]),
    "rhccq_encode_frame": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, C.POINTER(ClassDesc), c_int32, c_void_p, c_int32, c_void_p, c_void_p,
                                     C.POINTER(FrameResult)]),
    "rhccq_encode_frame_level2_info": (c_int32, [c_void_p, c_int32, c_void_p]),
    "rhccq_mbk_steps_batch": (c_int32, [c_void_p, c_void_p, C.POINTER(MbkProblem), c_int32, c_int64, c_int32, c_void_p, c_int64, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_int64, c_int32, C.c_uint32, C.c_uint32, c_int32, C.POINTER(c_int64),
                                        C.POINTER(c_int32)]),
    "rhccq_npysort_head": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "rhccq_mbk_steps": (c_int32, [c_void_p, c_void_p, C.POINTER(MbkProblem), c_int32, c_int64, c_int32, c_void_p, c_int64, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32]),
    "rhccq_mbk_steps_overlapped": (c_int32, [c_void_p, c_void_p, C.POINTER(MbkProblem), c_int32, c_int64, c_int32, c_void_p, c_int64, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int64, C.POINTER(c_int32)]),
    "rhccq_mt_randint_host": (c_int64, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p]),
    "rhccq_mt_words_host": (c_int32, [c_int64, c_int64, c_void_p]),
    "rhccq_mt_double_host": (c_double, [c_int64]),
    "rhccq_first_centre_index": (c_int32, [c_int64, c_double]),
    "rhccq_mbk_draws": (c_int32, [c_int64, c_int64, C.POINTER(MbkDraw), c_void_p, c_int64]),
    "rhccq_mt_words": (c_int32, [c_void_p, c_int64, C.POINTER(c_void_p), C.POINTER(c_int64)]),
    "rhccq_scatter_min_host": (c_int32, [c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_cluster_plan_host": (c_int64, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    "rhccq_merge_palettes_host": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_mbk_work_bytes": (c_int64, [C.POINTER(MbkProblem), c_int32]),
    "rhccq_px_neighbours": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.c_float, C.c_float, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_px_expand": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.c_float, C.c_float, c_void_p, c_void_p, c_void_p]),
    "rhccq_error_sums": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_error_tables": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "rhccq_ssim7_blocks": (c_int64, [c_int32, c_int32]),
    "rhccq_ssim7_sums": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64]),
    "rhccq_class_error_sums": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "rhccq_class_error_sums_indexed": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    "rhccq_class_ssim7_blocks": (c_int64, [c_int32, c_int32]),
    "rhccq_class_ssim7_sums": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int64]),
    "rhccq_split_stats_blocks": (c_int64, [c_int32, c_int32]),
    "rhccq_split_stats": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_slic_assign": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double, c_int32, c_void_p]),
    "rhccq_slic_connectivity_host": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "rhccq_ccl_work_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "rhccq_ccl": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_ccl_select": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_ccl_keys": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "rhccq_roi_buffer": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_edges_m2_bins": (c_int64, []),
    "rhccq_edges_gray": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "rhccq_edges_grad_hist": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "rhccq_canny_nms": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_edges_above": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "rhccq_label_reduce": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "rhccq_box_count": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "rhccq_morph_dilate": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_int32), c_int32, c_int32, c_void_p]),
    "rhccq_mask_op": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "rhccq_gap_bridge": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_int32, c_void_p]),
    "rhccq_morph_dilate_spans": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, C.POINTER(c_int32), C.POINTER(c_int32), c_int32, c_int32,
                                           c_void_p]),
    "rhccq_box_filter_seq": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "rhccq_box_sum": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "rhccq_dist_chamfer": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "rhccq_binary_sobel": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "rhccq_lut_u8": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_label_sum": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p]),
    "rhccq_masked_hist": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "rhccq_value_mask": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "rhccq_gauss1d_f64": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int64, c_void_p, c_int32, c_void_p]),
    "rhccq_zoom_linear_f64": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                        c_double, c_double, c_void_p]),
    "rhccq_zoom_nearest": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "rhccq_canny_scores_nested_bytes": (c_int64, [c_int32, c_int32]),
    "rhccq_canny_scores_nested": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    "rhccq_canny_scores_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "rhccq_canny_scores": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    "rhccq_edge_score": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "rhccq_lut_u16_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_void_p]),
    "rhccq_eps_counts": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double, c_void_p]),
    "rhccq_eps_border": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double, c_void_p, c_void_p]),
    "rhccq_mt_uniforms": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "rhccq_mbk_order_bytes": (c_int64, [c_int64]),
    "rhccq_mbk_order": (c_int32, [c_void_p, c_void_p, C.POINTER(MbkProblem), c_int32, c_void_p, c_void_p, c_void_p, c_int64]),
    "rhccq_mbk_assign": (c_int32, [c_void_p, c_void_p, C.POINTER(MbkProblem), c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_remap": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "rhccq_frame_remap": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32),
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32]),
    "rhccq_merge_firstpos": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "rhccq_merge_paint": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "rhccq_decode": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_int64, c_void_p]),
    "rhccq_dct_quant": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_luma_qstep": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p]),
    "rhccq_zlib_sizes": (c_int32, [c_int64, C.POINTER(c_int64), C.POINTER(c_int64)]),
    "rhccq_zlib_compress": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_zlib_inflate_sizes": (c_int32, [c_int64, c_int64, C.POINTER(c_int64)]),
    "rhccq_zlib_decompress": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "rhccq_zlib_inflate_stats": (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "rhccq_zlib_decompress_host": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, C.POINTER(c_int64), C.POINTER(c_int32)]),
    "rhccq_zlib9_sizes": (c_int32, [c_int64, C.POINTER(c_int64), C.POINTER(c_int64)]),
    "rhccq_zlib9_compress": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_zlib9_compress_host": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, C.POINTER(c_int64)]),
    "rhccq_zlib9_stats": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p]),
    "rhccq_split_stats_regions": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int64,
                                            c_void_p, c_void_p]),
    "rhccq_slic_regions_work_bytes": (c_int64, [c_int32, c_int32]),
    "rhccq_slic_sweeps_regions": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64,
                                            c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    "rhccq_image_seg_counts": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                         c_void_p, c_int64]),
    "rhccq_image_overlap": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                      c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_image_paint": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int64, c_void_p]),
    "rhccq_palette_remap": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_remap_host": (c_int32, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_remap_tile": (c_int32, []),
    "rhccq_palette_refine_lds_rows": (c_int32, []),
    "rhccq_palette_refine_bytes": (c_int64, [c_int32]),
    "rhccq_palette_refine": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int64,
                                       c_void_p, c_void_p]),
    "rhccq_palette_refine_host": (c_int32, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "rhccq_palette_reduce_max_rows": (c_int32, []),
    "rhccq_palette_reduce_bytes": (c_int64, [c_int32]),
    "rhccq_palette_reduce": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "rhccq_palette_reduce_host": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_palette_moments_lds_rows": (c_int32, [c_int32]),
    "rhccq_palette_moments": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_moments_host": (c_int32, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_curve_bytes": (c_int64, [c_int32, c_int32]),
    "rhccq_palette_curve": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    "rhccq_palette_curve_host": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_rung": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_palette_rung_host": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_palette_runs_tile_cols": (c_int32, []),
    "rhccq_palette_runs_rows": (c_int32, []),
    "rhccq_palette_runs": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_runs_host": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_segment_max_rows": (c_int32, []),
    "rhccq_palette_segment_tile_cols": (c_int32, []),
    "rhccq_palette_segment_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "rhccq_palette_segment": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int32,
                                        c_void_p]),
    "rhccq_palette_segment_host": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_dither_max_rows": (c_int32, []),
    "rhccq_palette_dither_rows": (c_int32, []),
    "rhccq_palette_dither_bytes": (c_int64, [c_int32, c_int32]),
    "rhccq_palette_dither": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int32,
                                       c_void_p, c_void_p]),
    "rhccq_palette_dither_host": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_cells_block": (c_int32, []),
    "rhccq_palette_cells_chunk": (c_int32, []),
    "rhccq_palette_cells": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_cells_host": (c_int32, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_build_max_rows": (c_int32, []),
    "rhccq_palette_build_bytes": (c_int64, []),
    "rhccq_palette_build": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_palette_build_host": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_palette_build_batch_bytes": (c_int64, [c_int32]),
    "rhccq_palette_refine_batch_bytes": (c_int64, [c_int32, c_int32]),
    "rhccq_palette_cells_batch": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "rhccq_palette_cells_batch_host": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "rhccq_palette_build_batch": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_palette_build_batch_host": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_palette_remap_batch": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                            c_int32, c_void_p]),
    "rhccq_palette_remap_batch_host": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_refine_batch": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                             c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "rhccq_palette_refine_batch_host": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                                                  c_void_p]),
    "rhccq_palette_pattern_max_rows": (c_int32, []),
    "rhccq_palette_pattern": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                        c_void_p]),
    "rhccq_palette_pattern_host": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                             c_void_p]),
    "rhccq_palette_pattern_batch": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p,
                                              c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "rhccq_palette_pattern_batch_host": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32,
                                                   c_void_p, c_int32, c_void_p]),
    "rhccq_png_sizes": (c_int32, [c_int32, c_int32, c_int32, c_int32, C.POINTER(c_int64), C.POINTER(c_int64), C.POINTER(c_int64)]),
    "rhccq_png_scanlines": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "rhccq_crc32_bytes": (c_int64, [c_int64]),
    "rhccq_crc32": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "rhccq_png_encode": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_png_scanlines_host": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "rhccq_crc32_host": (c_int32, [c_void_p, c_int64, c_void_p]),
    "rhccq_png_encode_host": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    "rhccq_png_parse_host": (c_int32, [c_void_p, c_int64, C.POINTER(PngInfo), c_void_p, c_int64, C.POINTER(c_int64)]),
    "rhccq_crc32_segments_plan": (c_int32, [c_void_p, c_int64, c_int64, C.POINTER(c_int64)]),
    "rhccq_crc32_segments": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "rhccq_crc32_segments_host": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p]),
    "rhccq_png_unfilter_band_rows": (c_int32, []),
    "rhccq_png_unfilter_tile": (c_int32, []),
    "rhccq_png_unfilter_granule": (c_int32, []),
    "rhccq_png_unfilter_bytes": (c_int64, [c_int32, c_int64, c_int32]),
    "rhccq_png_unfilter": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_png_unfilter_host": (c_int32, [c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p]),
    "rhccq_png_expand": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_png_expand_host": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_png_join": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int64, c_void_p]),
    "rhccq_png_read_sizes": (c_int32, [C.POINTER(PngInfo), c_int64, C.POINTER(c_int64)]),
    "rhccq_png_read_scan_offset": (c_int64, [C.POINTER(PngInfo)]),
    "rhccq_png_decode": (c_int32, [c_void_p, c_void_p, c_int64, C.POINTER(PngInfo), c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_png_decode_host": (c_int32, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rhccq_gif_segment_pixels": (c_int32, []),
    "rhccq_gif_sizes": (c_int32, [c_int32, c_int32, c_int32, c_int32, C.POINTER(c_int64), C.POINTER(c_int64), C.POINTER(c_int64)]),
    "rhccq_gif_lzw": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "rhccq_gif_encode": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                                   c_void_p, c_int64, c_void_p]),
    "rhccq_gif_lzw_host": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    "rhccq_gif_encode_host": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                                        c_int64, c_void_p, c_void_p]),
    "rhccq_gif_parse_host": (c_int32, [c_void_p, c_int64, C.POINTER(GifInfo), c_void_p, c_int64, C.POINTER(c_int64), c_void_p, c_int64, C.POINTER(c_int64)]),
    "rhccq_gif_read_tile": (c_int32, []),
    "rhccq_gif_read_scan_step": (c_int32, []),
    "rhccq_gif_read_threads": (c_int32, []),
    "rhccq_gif_read_sizes": (c_int32, [C.POINTER(GifInfo), c_int64, C.POINTER(c_int64)]),
    "rhccq_gif_unlzw_bytes": (c_int64, [c_void_p, c_int32]),
    "rhccq_gif_join": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p]),
    "rhccq_gif_unlzw": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "rhccq_gif_compose": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_gif_decode": (c_int32, [c_void_p, c_void_p, c_int64, C.POINTER(GifInfo), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "rhccq_gif_unlzw_host": (c_int32, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p, C.POINTER(c_int64)]),
    "rhccq_gif_compose_host": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "rhccq_gif_decode_host": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
}


class RhccqError(RuntimeError):
    pass


def load():
    """Load the shared library (no GPU needed to load it) and attach prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RhccqError(f"{LIB_PATH} is missing: run `python -m roibasedimagecompression_amd.build` "
                         "(or __graft_entry__.build()); there is no CPU fallback for the product path")
    # torch bundles its own libamdhip64; it must be in the process BEFORE this library is loaded so that
    # both resolve to ONE HIP runtime (torch owns device memory and streams, this library launches on them)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    lib = load()
    return [n for n in PROTOTYPES if hasattr(lib, n)]
