"""clip_cpp_amd — Python host layer over libclip.so (the MI355X-native CLIP encoder).

Mirrors the reference's ctypes binding (`examples/python_bindings/clip_cpp/clip.py:103-424`):
class `Clip` with `tokenize`, `encode_text`, `load_preprocess_encode_image`, `calculate_similarity`,
`compare_text_and_image`, `zero_shot_label_image`, plus MI355X extensions: batched encoders on host
(numpy) or device (raw HBM pointers, e.g. torch tensors) and the data-parallel helpers in
`clip_cpp_amd.parallel`.  Everything heavy happens in the C-ABI library (`include/clip.h`,
`include/clip_amd.h`); this module holds no arithmetic and NO CPU fallback: if the HIP library or a
GPU is missing the encoders raise.
"""
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CLIP_AMD_LIB") or os.path.join(_HERE, "libclip.so")   # CLIP_AMD_LIB: kernel A/B builds (scripts/build_variant.sh)


class ClipTextHparams(C.Structure):  # reference clip.h:14-23
    _fields_ = [("n_vocab", C.c_int32), ("num_positions", C.c_int32), ("hidden_size", C.c_int32),
                ("n_intermediate", C.c_int32), ("projection_dim", C.c_int32), ("n_head", C.c_int32),
                ("n_layer", C.c_int32), ("eps", C.c_float)]


class ClipVisionHparams(C.Structure):  # reference clip.h:25-34
    _fields_ = [("image_size", C.c_int32), ("patch_size", C.c_int32), ("hidden_size", C.c_int32),
                ("n_intermediate", C.c_int32), ("projection_dim", C.c_int32), ("n_head", C.c_int32),
                ("n_layer", C.c_int32), ("eps", C.c_float)]


class ClipTokens(C.Structure):  # reference clip.h:37-40
    _fields_ = [("data", C.POINTER(C.c_int32)), ("size", C.c_size_t)]


class ClipImageU8(C.Structure):  # reference clip.h:50-55
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("data", C.POINTER(C.c_uint8)), ("size", C.c_size_t)]


class ClipImageF32(C.Structure):  # reference clip.h:57-64
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("data", C.POINTER(C.c_float)), ("size", C.c_size_t)]


class ClipImageU8Batch(C.Structure):
    _fields_ = [("data", C.POINTER(ClipImageU8)), ("size", C.c_size_t)]


class ClipImageF32Batch(C.Structure):
    _fields_ = [("data", C.POINTER(ClipImageF32)), ("size", C.c_size_t)]


# every symbol include/clip.h and include/clip_amd.h declare (tests check they are all exported)
API_SYMBOLS = [
    "clip_model_load", "clip_free", "clip_get_text_hparams", "clip_get_vision_hparams", "clip_tokenize",
    "clip_image_u8_make", "clip_image_f32_make", "clip_image_u8_clean", "clip_image_f32_clean", "clip_image_u8_free",
    "clip_image_f32_free", "clip_image_load_from_file", "clip_image_preprocess", "clip_image_batch_preprocess",
    "clip_text_encode", "clip_image_encode", "clip_image_batch_encode", "clip_compare_text_and_image",
    "clip_similarity_score", "softmax_with_sorting", "clip_zero_shot_label_image", "clip_model_quantize",
    "ggml_time_init", "ggml_time_us", "ggml_time_ms",
]
AMD_SYMBOLS = [
    "clip_amd_device_count", "clip_amd_model_load", "clip_amd_model_load_multi", "clip_amd_ctx_device_count", "clip_amd_weights_from_cache", "clip_amd_shard_bounds",
    "clip_amd_gathered_embeddings", "clip_amd_ctx_device", "clip_amd_set_stream", "clip_amd_set_device_shared", "clip_amd_image_batch_encode_device_multi",
    "clip_amd_text_batch_encode_device_multi", "clip_amd_encode_pair_device_multi",
    "clip_amd_image_batch_encode_device", "clip_text_batch_encode", "clip_amd_text_batch_encode_device",
    "clip_amd_image_batch_preprocess_device", "clip_amd_image_batch_encode_u8",
    "clip_amd_zero_shot_score_device", "clip_amd_zero_shot_label_images",
    "clip_amd_synchronize", "clip_amd_profile_enable", "clip_amd_profile_read", "clip_amd_profile_report",
    "clip_amd_test_gemm", "clip_amd_test_gemm_ex", "clip_amd_test_gemm_f32", "clip_amd_test_gemm_tile", "clip_amd_test_gemm_tile_ex", "clip_amd_test_ctx_state", "clip_amd_test_tower_plan", "clip_amd_test_skinny", "clip_amd_test_layernorm", "clip_amd_test_attention", "clip_amd_bench_gemm",
    "clip_amd_test_attention_ex", "clip_amd_bench_attention", "clip_amd_test_attention_ragged",
    "clip_amd_test_layernorm_ex", "clip_amd_test_text_embed", "clip_amd_test_im2col", "clip_amd_test_layernorm_prep", "clip_amd_test_rows",
    "clip_amd_test_gemm_panel", "clip_amd_test_dequant_panels", "clip_amd_test_fold_vectors", "clip_amd_test_fold_producer", "clip_amd_test_fold_consumer",
    "clip_amd_index_create", "clip_amd_index_add", "clip_amd_index_add_device", "clip_amd_index_size", "clip_amd_index_dim",
    "clip_amd_index_search", "clip_amd_index_search_device", "clip_amd_index_save", "clip_amd_index_load", "clip_amd_index_free",
    "clip_amd_bench_search", "clip_amd_index_range_search", "clip_amd_index_pairs", "clip_amd_bench_range",
    "clip_amd_index_remove", "clip_amd_index_live", "clip_amd_index_live_mask", "clip_amd_index_compact", "clip_amd_index_search_subset",
    "clip_amd_index_search_subset_device", "clip_amd_index_range_search_subset", "clip_amd_bench_search_subset",
    "clip_amd_index_search_ids", "clip_amd_index_search_ids_device", "clip_amd_index_knn_graph", "clip_amd_test_index_knn_route", "clip_amd_bench_knn",
    "clip_amd_index_search_index", "clip_amd_index_append", "clip_amd_test_index_cross_route", "clip_amd_bench_cross",
    "clip_amd_image_batch_encode_files", "clip_amd_image_batch_encode_memory", "clip_amd_test_jpeg_plan", "clip_amd_test_jpeg_decode_device",
    "clip_amd_bench_jpeg_kernels", "clip_amd_test_jpeg_device_count",
    "clip_amd_index_search_grouped", "clip_amd_index_search_grouped_device", "clip_amd_bench_search_grouped",
    "clip_amd_image_batch_encode_regions", "clip_amd_image_batch_preprocess_regions_device", "clip_amd_image_batch_encode_files_grid",
    "clip_amd_image_batch_encode_memory_grid",
    "clip_amd_index_search_sets", "clip_amd_index_search_sets_device", "clip_amd_index_search_ids_sets", "clip_amd_test_index_sets_block",
    "clip_amd_bench_search_sets",
    "clip_amd_index_search_distinct", "clip_amd_index_search_distinct_device", "clip_amd_index_search_ids_distinct",
    "clip_amd_test_index_distinct_block", "clip_amd_bench_search_distinct",
    "clip_amd_index_search_compound", "clip_amd_index_search_compound_device", "clip_amd_test_index_compound_block",
    "clip_amd_bench_search_compound",
    "clip_amd_index_components", "clip_amd_index_components_device", "clip_amd_bench_components",
    "clip_amd_index_modes", "clip_amd_index_modes_device", "clip_amd_bench_modes",
    "clip_amd_index_spread", "clip_amd_index_spread_device", "clip_amd_bench_spread",
    "clip_amd_index_linkage", "clip_amd_index_linkage_device", "clip_amd_bench_linkage", "clip_amd_bench_linkage_rounds",
    "clip_amd_test_index_linkage_rounds",
    "clip_amd_index_linkage_core", "clip_amd_index_linkage_core_device", "clip_amd_bench_linkage_core", "clip_amd_bench_linkage_core_parts",
    "clip_amd_index_extents", "clip_amd_index_extents_device", "clip_amd_bench_extents", "clip_amd_test_index_extents_route",
    "clip_amd_index_vote", "clip_amd_index_vote_device", "clip_amd_index_vote_ids", "clip_amd_index_vote_graph", "clip_amd_index_vote_graph_device",
    "clip_amd_test_index_vote_block", "clip_amd_bench_vote_graph",
]

_lib = None


def build_lib(force=False):
    import importlib
    return importlib.import_module(__name__ + ".build").build(force=force)


def lib():
    """Load libclip.so (building it first if the in-tree binary is missing). Raises if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        build_lib()
    L = C.CDLL(LIB_PATH)
    vp, i32, f32p = C.c_void_p, C.c_int, C.POINTER(C.c_float)
    L.clip_model_load.restype = vp
    L.clip_model_load.argtypes = [C.c_char_p, i32]
    L.clip_amd_model_load.restype = vp
    L.clip_amd_model_load.argtypes = [C.c_char_p, i32, i32]
    L.clip_amd_model_load_multi.restype = vp
    L.clip_amd_model_load_multi.argtypes = [C.c_char_p, i32, i32]
    L.clip_amd_ctx_device_count.restype = i32
    L.clip_amd_ctx_device_count.argtypes = [vp]
    L.clip_amd_weights_from_cache.restype = i32
    L.clip_amd_weights_from_cache.argtypes = [vp]
    L.clip_amd_shard_bounds.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.clip_amd_gathered_embeddings.restype = vp
    L.clip_amd_gathered_embeddings.argtypes = [vp, i32]
    L.clip_free.argtypes = [vp]
    L.clip_get_text_hparams.restype = C.POINTER(ClipTextHparams)
    L.clip_get_text_hparams.argtypes = [vp]
    L.clip_get_vision_hparams.restype = C.POINTER(ClipVisionHparams)
    L.clip_get_vision_hparams.argtypes = [vp]
    L.clip_tokenize.restype = C.c_bool
    L.clip_tokenize.argtypes = [vp, C.c_char_p, C.POINTER(ClipTokens)]
    L.clip_image_u8_make.restype = C.POINTER(ClipImageU8)
    L.clip_image_f32_make.restype = C.POINTER(ClipImageF32)
    L.clip_image_u8_clean.argtypes = [C.POINTER(ClipImageU8)]
    L.clip_image_f32_clean.argtypes = [C.POINTER(ClipImageF32)]
    L.clip_image_u8_free.argtypes = [C.POINTER(ClipImageU8)]
    L.clip_image_f32_free.argtypes = [C.POINTER(ClipImageF32)]
    L.clip_image_load_from_file.restype = C.c_bool
    L.clip_image_load_from_file.argtypes = [C.c_char_p, C.POINTER(ClipImageU8)]
    L.clip_image_preprocess.restype = C.c_bool
    L.clip_image_preprocess.argtypes = [vp, C.POINTER(ClipImageU8), C.POINTER(ClipImageF32)]
    L.clip_image_batch_preprocess.argtypes = [vp, i32, C.POINTER(ClipImageU8Batch), C.POINTER(ClipImageF32Batch)]
    L.clip_text_encode.restype = C.c_bool
    L.clip_text_encode.argtypes = [vp, i32, C.POINTER(ClipTokens), f32p, C.c_bool]
    L.clip_text_batch_encode.restype = C.c_bool
    L.clip_text_batch_encode.argtypes = [vp, i32, C.POINTER(ClipTokens), C.c_size_t, f32p, C.c_bool]
    L.clip_image_encode.restype = C.c_bool
    L.clip_image_encode.argtypes = [vp, i32, C.POINTER(ClipImageF32), f32p, C.c_bool]
    L.clip_image_batch_encode.restype = C.c_bool
    L.clip_image_batch_encode.argtypes = [vp, i32, C.POINTER(ClipImageF32Batch), f32p, C.c_bool]
    L.clip_compare_text_and_image.restype = C.c_bool
    L.clip_compare_text_and_image.argtypes = [vp, i32, C.c_char_p, C.POINTER(ClipImageU8), f32p]
    L.clip_similarity_score.restype = C.c_float
    L.clip_similarity_score.argtypes = [f32p, f32p, i32]
    L.softmax_with_sorting.restype = C.c_bool
    L.softmax_with_sorting.argtypes = [f32p, i32, f32p, C.POINTER(C.c_int)]
    L.clip_zero_shot_label_image.restype = C.c_bool
    L.clip_zero_shot_label_image.argtypes = [vp, i32, C.POINTER(ClipImageU8), C.POINTER(C.c_char_p), C.c_size_t, f32p,
                                             C.POINTER(C.c_int)]
    L.clip_model_quantize.restype = C.c_bool
    L.clip_model_quantize.argtypes = [C.c_char_p, C.c_char_p, i32]
    L.clip_amd_device_count.restype = i32
    L.clip_amd_ctx_device.restype = i32
    L.clip_amd_ctx_device.argtypes = [vp]
    L.clip_amd_set_stream.argtypes = [vp, vp]
    L.clip_amd_set_device_shared.restype = None
    L.clip_amd_set_device_shared.argtypes = [vp, i32]
    L.clip_amd_synchronize.argtypes = [vp]
    L.clip_amd_image_batch_encode_device.restype = C.c_bool
    L.clip_amd_image_batch_encode_device.argtypes = [vp, vp, i32, vp, C.c_bool]
    L.clip_amd_image_batch_preprocess_device.restype = C.c_bool
    L.clip_amd_image_batch_preprocess_device.argtypes = [vp, C.POINTER(ClipImageU8), i32, vp]
    L.clip_amd_zero_shot_score_device.restype = C.c_bool
    L.clip_amd_zero_shot_score_device.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp]
    L.clip_amd_zero_shot_label_images.restype = C.c_bool
    L.clip_amd_zero_shot_label_images.argtypes = [vp, C.POINTER(ClipImageU8), i32, C.POINTER(C.c_char_p), C.c_size_t, f32p, C.POINTER(C.c_int)]
    L.clip_amd_image_batch_encode_u8.restype = C.c_bool
    L.clip_amd_image_batch_encode_u8.argtypes = [vp, C.POINTER(ClipImageU8), i32, f32p, C.c_bool]
    L.clip_amd_text_batch_encode_device.restype = C.c_bool
    L.clip_amd_text_batch_encode_device.argtypes = [vp, vp, C.POINTER(C.c_int32), i32, vp, C.c_bool]
    L.clip_amd_image_batch_encode_device_multi.restype = C.c_bool
    L.clip_amd_image_batch_encode_device_multi.argtypes = [vp, C.POINTER(vp), i32, C.c_bool, f32p]
    L.clip_amd_text_batch_encode_device_multi.restype = C.c_bool
    L.clip_amd_text_batch_encode_device_multi.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int32), i32, C.c_bool, f32p]
    L.clip_amd_encode_pair_device_multi.restype = C.c_bool
    L.clip_amd_encode_pair_device_multi.argtypes = [vp, C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(C.c_int32), i32, C.c_bool, f32p, f32p]
    L.clip_amd_profile_enable.argtypes = [vp, C.c_bool]
    L.clip_amd_profile_report.restype = i32
    L.clip_amd_profile_report.argtypes = [vp, C.c_char_p, i32, C.c_bool]
    L.clip_amd_test_gemm.restype = i32
    L.clip_amd_test_gemm.argtypes = [i32, vp, C.c_int64, C.c_int64, f32p, C.c_int64, f32p, f32p, f32p, i32, i32]
    L.clip_amd_test_gemm_ex.restype = i32
    L.clip_amd_test_gemm_ex.argtypes = [i32, vp, C.c_int64, C.c_int64, f32p, C.c_int64, f32p, f32p, f32p, i32, i32, i32, C.c_float, i32, i32, f32p]
    L.clip_amd_test_gemm_panel.restype = i32
    L.clip_amd_test_gemm_panel.argtypes = [i32, vp, vp, C.c_int64, C.c_int64, f32p, C.c_int64, f32p, f32p, f32p, i32, i32, i32, C.c_float, i32, i32]
    L.clip_amd_test_dequant_panels.restype = i32
    L.clip_amd_test_dequant_panels.argtypes = [i32, C.POINTER(i32), C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(vp), C.POINTER(i32)]
    L.clip_amd_test_fold_vectors.restype = i32
    L.clip_amd_test_fold_vectors.argtypes = [i32, vp, C.c_int64, C.c_int64, f32p, f32p, f32p, f32p, f32p]
    L.clip_amd_test_gemm_f32.restype = i32
    L.clip_amd_test_gemm_f32.argtypes = [vp, C.c_int64, C.c_int64, f32p, C.c_int64, f32p, f32p, i32, i32, C.c_float, i32, i32, f32p, i32, i32, f32p]
    L.clip_amd_test_lnfold.restype = i32
    L.clip_amd_test_lnfold.argtypes = [i32, vp, C.c_int64, C.c_int64, vp, C.c_int64, f32p, C.c_int64, f32p, f32p, f32p, f32p, C.c_float, f32p,
                                       i32, i32, i32, i32, i32, C.c_float, f32p, f32p]
    L.clip_amd_test_fold_producer.restype = i32
    L.clip_amd_test_fold_producer.argtypes = [i32, vp, C.c_int64, C.c_int64, f32p, C.c_int64, f32p, f32p, f32p, f32p, i32, C.c_int64, f32p, vp, f32p, C.POINTER(i32)]
    L.clip_amd_test_fold_consumer.restype = i32
    L.clip_amd_test_fold_consumer.argtypes = [i32, vp, C.c_int64, C.c_int64, vp, C.c_int64, f32p, i32, i32, f32p, f32p, f32p, C.c_float, i32, i32, C.c_float,
                                              i32, f32p, f32p]
    L.clip_amd_test_gemm_tile.restype = i32
    L.clip_amd_test_gemm_tile.argtypes = [C.c_int64, C.c_int64, C.c_int64, i32]
    L.clip_amd_test_gemm_tile_ex.restype = i32
    L.clip_amd_test_gemm_tile_ex.argtypes = [C.c_int64, C.c_int64, C.c_int64, i32, i32]
    L.clip_amd_test_ctx_state.restype = i32
    L.clip_amd_test_ctx_state.argtypes = [vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), i32]
    L.clip_amd_test_tower_plan.restype = i32
    L.clip_amd_test_tower_plan.argtypes = [C.c_int64, i32, i32, i32, i32, i32, C.c_int64, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32, C.POINTER(C.c_int64)]
    L.clip_amd_test_skinny.restype = i32
    L.clip_amd_test_skinny.argtypes = [i32, vp, C.c_int64, C.c_int64, f32p, C.c_int64, f32p, f32p, f32p, f32p, C.c_float, f32p, i32, i32, C.c_float, f32p]
    L.clip_amd_bench_gemm.restype = C.c_float
    L.clip_amd_bench_gemm.argtypes = [i32, C.c_int64, C.c_int64, C.c_int64, i32, i32, i32]
    L.clip_amd_test_layernorm.restype = i32
    L.clip_amd_test_layernorm.argtypes = [f32p, f32p, f32p, C.c_float, C.c_int64, C.c_int64, f32p, i32]
    u16p, i32p = C.POINTER(C.c_uint16), C.POINTER(C.c_int32)
    L.clip_amd_test_layernorm_ex.restype = i32
    L.clip_amd_test_layernorm_ex.argtypes = [f32p, C.c_int64, i32, i32p, i32, f32p, f32p, C.c_float, i32, i32, u16p, i32, f32p, i32]
    L.clip_amd_test_text_embed.restype = i32
    L.clip_amd_test_text_embed.argtypes = [i32, vp, C.c_int64, i32, i32p, i32p, i32, i32, f32p, i32, f32p, i32, f32p, u16p, i32, f32p, f32p]
    L.clip_amd_test_im2col.restype = i32
    L.clip_amd_test_im2col.argtypes = [f32p, i32, i32, i32, i32, i32, u16p]
    L.clip_amd_test_layernorm_prep.restype = i32
    L.clip_amd_test_layernorm_prep.argtypes = [f32p, i32, f32p, f32p, C.c_float, i32, i32, f32p, i32, f32p, f32p, i32, i32, f32p, i32, u16p, i32, f32p, f32p]
    L.clip_amd_test_rows.restype = i32
    L.clip_amd_test_rows.argtypes = [i32, vp, vp, i32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp, vp]
    L.clip_amd_test_attention.restype = i32
    L.clip_amd_test_attention.argtypes = [f32p, i32, i32, i32, i32, i32, f32p]
    L.clip_amd_test_attention_ex.restype = i32
    L.clip_amd_test_attention_ex.argtypes = [f32p, i32, i32, i32, i32, i32, f32p, i32]
    L.clip_amd_bench_attention.restype = C.c_float
    L.clip_amd_bench_attention.argtypes = [i32, i32, i32, i32, i32, i32, i32]
    L.clip_amd_test_attention_ragged.restype = i32
    L.clip_amd_test_attention_ragged.argtypes = [f32p, C.c_int64, i32p, i32, i32, i32, i32, i32, f32p, i32]
    i64, i64p = C.c_int64, C.POINTER(C.c_int64)
    L.clip_amd_index_create.restype = vp
    L.clip_amd_index_create.argtypes = [vp, i32, i32]
    L.clip_amd_index_add.restype = C.c_bool
    L.clip_amd_index_add.argtypes = [vp, f32p, i64]
    L.clip_amd_index_add_device.restype = C.c_bool
    L.clip_amd_index_add_device.argtypes = [vp, vp, i64]
    L.clip_amd_index_size.restype = i64
    L.clip_amd_index_size.argtypes = [vp]
    L.clip_amd_index_dim.restype = i32
    L.clip_amd_index_dim.argtypes = [vp]
    L.clip_amd_index_search.restype = C.c_bool
    L.clip_amd_index_search.argtypes = [vp, f32p, i32, i32, f32p, i64p]
    L.clip_amd_index_search_device.restype = C.c_bool
    L.clip_amd_index_search_device.argtypes = [vp, vp, i32, i32, vp, vp]
    L.clip_amd_index_save.restype = C.c_bool
    L.clip_amd_index_save.argtypes = [vp, C.c_char_p]
    L.clip_amd_index_load.restype = vp
    L.clip_amd_index_load.argtypes = [vp, C.c_char_p]
    L.clip_amd_index_free.restype = None
    L.clip_amd_index_free.argtypes = [vp]
    L.clip_amd_bench_search.restype = C.c_float
    L.clip_amd_bench_search.argtypes = [i32, i64, i32, i32, i32, i32]
    L.clip_amd_index_range_search.restype = i64
    L.clip_amd_index_range_search.argtypes = [vp, f32p, i32, C.c_float, i64p, f32p, i64p, i64]
    L.clip_amd_index_pairs.restype = i64
    L.clip_amd_index_pairs.argtypes = [vp, C.c_float, i64p, f32p, i64p, i64]
    L.clip_amd_bench_range.restype = C.c_float
    L.clip_amd_bench_range.argtypes = [i32, i64, i32, i32, C.c_float, i32]
    u64p = C.POINTER(C.c_uint64)
    L.clip_amd_index_remove.restype = i64
    L.clip_amd_index_remove.argtypes = [vp, i64p, i64]
    L.clip_amd_index_live.restype = i64
    L.clip_amd_index_live.argtypes = [vp]
    L.clip_amd_index_live_mask.restype = C.c_bool
    L.clip_amd_index_live_mask.argtypes = [vp, u64p]
    L.clip_amd_index_compact.restype = i64
    L.clip_amd_index_compact.argtypes = [vp, i64p]
    L.clip_amd_index_search_subset.restype = C.c_bool
    L.clip_amd_index_search_subset.argtypes = [vp, f32p, i32, i32, u64p, f32p, i64p]
    L.clip_amd_index_search_subset_device.restype = C.c_bool
    L.clip_amd_index_search_subset_device.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.clip_amd_index_range_search_subset.restype = i64
    L.clip_amd_index_range_search_subset.argtypes = [vp, f32p, i32, C.c_float, u64p, i64p, f32p, i64p, i64]
    L.clip_amd_index_components.restype = i64
    L.clip_amd_index_components.argtypes = [vp, C.c_float, u64p, i64p, f32p, i64p]
    L.clip_amd_index_components_device.restype = C.c_bool
    L.clip_amd_index_components_device.argtypes = [vp, C.c_float, vp, vp, vp, vp]
    L.clip_amd_bench_components.restype = C.c_float
    L.clip_amd_bench_components.argtypes = [i32, i64, i32, C.c_float, i32]
    L.clip_amd_index_modes.restype = i64
    L.clip_amd_index_modes.argtypes = [vp, C.c_float, C.c_float, u64p, i64p, i64p, f32p, C.POINTER(C.c_int32)]
    L.clip_amd_index_modes_device.restype = C.c_bool
    L.clip_amd_index_modes_device.argtypes = [vp, C.c_float, C.c_float, vp, vp, vp, vp, vp]
    L.clip_amd_bench_modes.restype = C.c_float
    L.clip_amd_bench_modes.argtypes = [i32, i64, i32, C.c_float, C.c_float, i32, i32]
    L.clip_amd_index_linkage.restype = i64
    L.clip_amd_index_linkage.argtypes = [vp, C.c_float, u64p, i64p, i64p, f32p]
    L.clip_amd_index_linkage_device.restype = C.c_bool
    L.clip_amd_index_linkage_device.argtypes = [vp, C.c_float, vp, vp, vp, vp, vp]
    L.clip_amd_index_linkage_core.restype = i64
    L.clip_amd_index_linkage_core.argtypes = [vp, i32, C.c_float, u64p, i64p, i64p, f32p, f32p]
    L.clip_amd_index_linkage_core_device.restype = C.c_bool
    L.clip_amd_index_linkage_core_device.argtypes = [vp, i32, C.c_float, vp, vp, vp, vp, vp, vp]
    L.clip_amd_bench_linkage_core.restype = C.c_float
    L.clip_amd_bench_linkage_core.argtypes = [i32, i64, i32, i32, i32, i32]
    L.clip_amd_bench_linkage_core_parts.restype = None
    L.clip_amd_bench_linkage_core_parts.argtypes = [f32p]
    L.clip_amd_bench_linkage.restype = C.c_float
    L.clip_amd_bench_linkage.argtypes = [i32, i64, i32, i32, i32]
    L.clip_amd_bench_linkage_rounds.restype = i32
    L.clip_amd_bench_linkage_rounds.argtypes = []
    L.clip_amd_index_extents.restype = i64
    L.clip_amd_index_extents.argtypes = [vp, i64p, u64p, i64p, f32p, f32p, f32p, i64p]
    L.clip_amd_index_extents_device.restype = C.c_bool
    L.clip_amd_index_extents_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.clip_amd_bench_extents.restype = C.c_float
    L.clip_amd_bench_extents.argtypes = [i32, i64, i32, i32, i32, i32]
    L.clip_amd_test_index_extents_route.restype = i64
    L.clip_amd_test_index_extents_route.argtypes = [vp, i32]
    L.clip_amd_test_index_linkage_rounds.restype = i32
    L.clip_amd_test_index_linkage_rounds.argtypes = [vp]
    L.clip_amd_index_spread.restype = i64
    L.clip_amd_index_spread.argtypes = [vp, i64, C.c_float, i64p, i64, u64p, i64p, f32p, i64p, f32p, f32p]
    L.clip_amd_index_spread_device.restype = C.c_bool
    L.clip_amd_index_spread_device.argtypes = [vp, i64, C.c_float, i64p, i64, vp, vp, vp, vp, vp, vp, vp]
    L.clip_amd_bench_spread.restype = C.c_float
    L.clip_amd_bench_spread.argtypes = [i32, i64, i32, i64, i32, i32]
    L.clip_amd_index_search_grouped.restype = C.c_bool
    L.clip_amd_index_search_grouped.argtypes = [vp, f32p, i32, i32, C.POINTER(C.c_int32), u64p, f32p, i64p]
    L.clip_amd_index_search_grouped_device.restype = C.c_bool
    L.clip_amd_index_search_grouped_device.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
    L.clip_amd_bench_search_grouped.restype = C.c_float
    L.clip_amd_bench_search_grouped.argtypes = [i32, i64, i32, i32, i32, i32, i32]
    L.clip_amd_index_search_sets.restype = C.c_bool
    L.clip_amd_index_search_sets.argtypes = [vp, f32p, i32, i64p, i64, i32, C.POINTER(C.c_int32), u64p, f32p, i64p, C.POINTER(C.c_int32)]
    L.clip_amd_index_search_sets_device.restype = C.c_bool
    L.clip_amd_index_search_sets_device.argtypes = [vp, vp, i32, i64p, i64, i32, vp, vp, vp, vp, vp]
    L.clip_amd_index_search_ids_sets.restype = C.c_bool
    L.clip_amd_index_search_ids_sets.argtypes = [vp, i64p, i64, i64p, i64, i32, i32, C.POINTER(C.c_int32), u64p, f32p, i64p, C.POINTER(C.c_int32)]
    L.clip_amd_test_index_sets_block.restype = i64
    L.clip_amd_test_index_sets_block.argtypes = [vp, i64]
    L.clip_amd_bench_search_sets.restype = C.c_float
    L.clip_amd_bench_search_sets.argtypes = [i32, i64, i32, i32, i32, i32, i32, i32]
    L.clip_amd_index_search_distinct.restype = C.c_bool
    L.clip_amd_index_search_distinct.argtypes = [vp, f32p, i32, i32, C.c_float, i32, u64p, f32p, i64p, C.POINTER(C.c_int32)]
    L.clip_amd_index_search_distinct_device.restype = C.c_bool
    L.clip_amd_index_search_distinct_device.argtypes = [vp, vp, i32, i32, C.c_float, i32, vp, vp, vp, vp]
    L.clip_amd_index_search_ids_distinct.restype = C.c_bool
    L.clip_amd_index_search_ids_distinct.argtypes = [vp, i64p, i32, i32, C.c_float, i32, i32, u64p, f32p, i64p, C.POINTER(C.c_int32)]
    L.clip_amd_test_index_distinct_block.restype = i32
    L.clip_amd_test_index_distinct_block.argtypes = [vp, i32]
    L.clip_amd_bench_search_distinct.restype = C.c_float
    L.clip_amd_bench_search_distinct.argtypes = [i32, i64, i32, i32, i32, i32, C.c_float, i32, i32]
    L.clip_amd_index_search_compound.restype = C.c_bool
    L.clip_amd_index_search_compound.argtypes = [vp, f32p, i64p, C.POINTER(C.c_int32), f32p, i64p, i32, i32, i32, u64p, f32p, i64p]
    L.clip_amd_index_search_compound_device.restype = C.c_bool
    L.clip_amd_index_search_compound_device.argtypes = [vp, vp, i64p, C.POINTER(C.c_int32), f32p, i64p, i32, i32, i32, vp, vp, vp]
    L.clip_amd_test_index_compound_block.restype = i32
    L.clip_amd_test_index_compound_block.argtypes = [vp, i32]
    L.clip_amd_bench_search_compound.restype = C.c_float
    L.clip_amd_bench_search_compound.argtypes = [i32, i64, i32, i32, i32, i32, i32]
    L.clip_amd_bench_search_subset.restype = C.c_float
    L.clip_amd_bench_search_subset.argtypes = [i32, i64, i32, i32, i32, C.c_float, i32, i32]
    L.clip_amd_index_search_ids.restype = C.c_bool
    L.clip_amd_index_search_ids.argtypes = [vp, i64p, i32, i32, i32, u64p, f32p, i64p]
    L.clip_amd_index_search_ids_device.restype = C.c_bool
    L.clip_amd_index_search_ids_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    L.clip_amd_index_knn_graph.restype = C.c_bool
    L.clip_amd_index_knn_graph.argtypes = [vp, i32, f32p, i64p]
    L.clip_amd_test_index_knn_route.restype = i32
    L.clip_amd_test_index_knn_route.argtypes = [vp, i32]
    L.clip_amd_bench_knn.restype = C.c_float
    L.clip_amd_bench_knn.argtypes = [i32, i64, i32, i32, i32, i32]
    L.clip_amd_index_vote.restype = C.c_bool
    L.clip_amd_index_vote.argtypes = [vp, f32p, i32, i32, i32, i32p, u64p, i32p, i32p, f32p, i64p]
    L.clip_amd_index_vote_device.restype = C.c_bool
    L.clip_amd_index_vote_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.clip_amd_index_vote_ids.restype = C.c_bool
    L.clip_amd_index_vote_ids.argtypes = [vp, i64p, i64, i32, i32, i32, i32p, u64p, i32p, i32p, f32p, i64p]
    L.clip_amd_index_vote_graph.restype = C.c_bool
    L.clip_amd_index_vote_graph.argtypes = [vp, i32, i32, i32p, u64p, i32p, i32p, f32p, i64p]
    L.clip_amd_index_vote_graph_device.restype = C.c_bool
    L.clip_amd_index_vote_graph_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.clip_amd_test_index_vote_block.restype = i64
    L.clip_amd_test_index_vote_block.argtypes = [vp, i64]
    L.clip_amd_bench_vote_graph.restype = C.c_float
    L.clip_amd_bench_vote_graph.argtypes = [i32, i64, i32, i32, i32, i32, i32, i32]
    L.clip_amd_index_search_index.restype = C.c_bool
    L.clip_amd_index_search_index.argtypes = [vp, vp, i64p, i64, i32, u64p, f32p, i64p]
    L.clip_amd_index_append.restype = i64
    L.clip_amd_index_append.argtypes = [vp, vp, i64p]
    L.clip_amd_test_index_cross_route.restype = i32
    L.clip_amd_test_index_cross_route.argtypes = [vp, i32]
    L.clip_amd_bench_cross.restype = C.c_float
    L.clip_amd_bench_cross.argtypes = [i32, i64, i64, i32, i32, i32, i32]
    u8p, szp = C.POINTER(C.c_uint8), C.POINTER(C.c_size_t)
    L.clip_amd_image_batch_encode_files.restype = i32
    L.clip_amd_image_batch_encode_files.argtypes = [vp, C.POINTER(C.c_char_p), i32, i32, i32, C.c_bool, f32p, C.POINTER(i32), u8p]
    i32p = C.POINTER(C.c_int32)
    L.clip_amd_image_batch_encode_regions.restype = C.c_bool
    L.clip_amd_image_batch_encode_regions.argtypes = [vp, C.POINTER(ClipImageU8), i32, i32p, i32, f32p, C.c_bool]
    L.clip_amd_image_batch_preprocess_regions_device.restype = C.c_bool
    L.clip_amd_image_batch_preprocess_regions_device.argtypes = [vp, C.POINTER(ClipImageU8), i32, i32p, i32, vp]
    L.clip_amd_image_batch_encode_files_grid.restype = i32
    L.clip_amd_image_batch_encode_files_grid.argtypes = [vp, C.POINTER(C.c_char_p), i32, i32, i32, i32, C.c_bool, f32p, i32p, C.POINTER(i32), u8p]
    L.clip_amd_image_batch_encode_memory_grid.restype = i32
    L.clip_amd_image_batch_encode_memory_grid.argtypes = [vp, C.POINTER(C.c_char_p), szp, i32, i32, i32, i32, C.c_bool, f32p, i32p, C.POINTER(i32), u8p]
    L.clip_amd_image_batch_encode_memory.restype = i32
    L.clip_amd_image_batch_encode_memory.argtypes = [vp, C.POINTER(C.c_char_p), szp, i32, i32, i32, C.c_bool, f32p, C.POINTER(i32), u8p]
    L.clip_amd_test_jpeg_plan.restype = i32
    L.clip_amd_test_jpeg_plan.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(i32)]
    L.clip_amd_test_jpeg_decode_device.restype = i32
    L.clip_amd_test_jpeg_decode_device.argtypes = [C.c_char_p, C.c_size_t, u8p, C.c_size_t, C.POINTER(i32), C.POINTER(i32)]
    L.clip_amd_test_jpeg_device_count.restype = C.c_longlong
    L.clip_amd_test_jpeg_device_count.argtypes = []
    L.clip_amd_bench_jpeg_kernels.restype = i32
    L.clip_amd_bench_jpeg_kernels.argtypes = [C.c_char_p, C.c_size_t, i32, i32, f32p, C.POINTER(C.c_double)]
    _lib = L
    return L


def device_count():
    return lib().clip_amd_device_count()


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _struct_to_dict(s):
    return {f: getattr(s, f) for f, _ in s._fields_}


class Clip:
    """Same surface as the reference binding's `Clip` (clip.py:215-424), minus the HF-hub downloader."""

    def __init__(self, model_path_or_repo_id, verbosity=0, device=None, n_devices=None):
        L = lib()
        path = os.fsencode(model_path_or_repo_id)
        if n_devices is not None:       # single process, replicas on n_devices GPUs, batch sharding + RCCL all-gather behind the C ABI
            self.ctx = L.clip_amd_model_load_multi(path, verbosity, int(n_devices))
        elif device is None:
            self.ctx = L.clip_model_load(path, verbosity)
        else:
            self.ctx = L.clip_amd_model_load(path, verbosity, int(device))
        if not self.ctx:
            raise RuntimeError("clip_model_load failed for %r (no file, malformed GGUF, or no HIP device)" % (model_path_or_repo_id,))
        self.vec_dim = self.vision_config["projection_dim"] or self.text_config["projection_dim"]

    # ---- reference surface ----
    @property
    def vision_config(self):
        return _struct_to_dict(lib().clip_get_vision_hparams(self.ctx).contents)

    @property
    def text_config(self):
        return _struct_to_dict(lib().clip_get_text_hparams(self.ctx).contents)

    @property
    def device(self):
        return lib().clip_amd_ctx_device(self.ctx)

    def tokenize(self, text):
        t = ClipTokens()
        if not lib().clip_tokenize(self.ctx, text.encode("utf-8"), C.byref(t)):
            raise RuntimeError("Could not tokenize text")
        return [t.data[i] for i in range(t.size)]   # (t.data is leaked exactly as in the reference; a few bytes)

    def encode_text(self, tokens, n_threads=os.cpu_count(), normalize=True):
        arr = (C.c_int32 * len(tokens))(*tokens)
        t = ClipTokens(C.cast(arr, C.POINTER(C.c_int32)), len(tokens))
        out = np.empty(self.text_config["projection_dim"], dtype=np.float32)
        if not lib().clip_text_encode(self.ctx, n_threads or 1, C.byref(t), _fp(out), normalize):
            raise RuntimeError("Could not encode text")
        return out.tolist()

    def load_preprocess_encode_image(self, image_path, n_threads=os.cpu_count(), normalize=True):
        L = lib()
        img = L.clip_image_u8_make()
        res = L.clip_image_f32_make()
        try:
            if not L.clip_image_load_from_file(os.fsencode(image_path), img):
                raise RuntimeError("Could not load image '%s'" % image_path)
            if not L.clip_image_preprocess(self.ctx, img, res):
                raise RuntimeError("Could not preprocess image")
            out = np.empty(self.vec_dim, dtype=np.float32)
            if not L.clip_image_encode(self.ctx, n_threads or 1, res, _fp(out), normalize):
                raise RuntimeError("Could not encode image")
            return out.tolist()
        finally:
            L.clip_image_u8_free(img)
            L.clip_image_f32_free(res)

    def calculate_similarity(self, text_embedding, image_embedding):
        a = np.asarray(text_embedding, dtype=np.float32)
        b = np.asarray(image_embedding, dtype=np.float32)
        return float(lib().clip_similarity_score(_fp(a), _fp(b), a.size))

    def compare_text_and_image(self, text, image_path, n_threads=os.cpu_count()):
        L = lib()
        img = L.clip_image_u8_make()
        try:
            if not L.clip_image_load_from_file(os.fsencode(image_path), img):
                raise RuntimeError("Could not load image '%s'" % image_path)
            score = C.c_float()
            if not L.clip_compare_text_and_image(self.ctx, n_threads or 1, text.encode("utf-8"), img, C.byref(score)):
                raise RuntimeError("Could not compare text and image")
            return score.value
        finally:
            L.clip_image_u8_free(img)

    def zero_shot_label_image(self, image_path, labels, n_threads=os.cpu_count()):
        L = lib()
        img = L.clip_image_u8_make()
        try:
            if not L.clip_image_load_from_file(os.fsencode(image_path), img):
                raise RuntimeError("Could not load image '%s'" % image_path)
            return self.zero_shot_label_pixels(img, labels, n_threads)
        finally:
            L.clip_image_u8_free(img)

    # ---- extensions ----
    def zero_shot_label_pixels(self, img_u8_ptr, labels, n_threads=1):
        n = len(labels)
        arr = (C.c_char_p * n)(*[s.encode("utf-8") for s in labels])
        scores = np.empty(n, dtype=np.float32)
        idx = np.empty(n, dtype=np.int32)
        if not lib().clip_zero_shot_label_image(self.ctx, n_threads or 1, img_u8_ptr, arr, n, _fp(scores),
                                                idx.ctypes.data_as(C.POINTER(C.c_int))):
            raise RuntimeError("Could not zero-shot label image")
        return scores.tolist(), idx.tolist()

    def preprocess(self, rgb):
        """uint8 [ny,nx,3] -> float32 [S,S,3] through clip_image_preprocess (host)."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        ny, nx, _ = rgb.shape
        src = ClipImageU8(nx, ny, rgb.ctypes.data_as(C.POINTER(C.c_uint8)), rgb.size)
        res = ClipImageF32()
        if not lib().clip_image_preprocess(self.ctx, C.byref(src), C.byref(res)):
            raise RuntimeError("Could not preprocess image")
        S = self.vision_config["image_size"]
        out = np.ctypeslib.as_array(res.data, shape=(S, S, 3)).copy()
        lib().clip_image_f32_clean(C.byref(res))
        return out

    @staticmethod
    def _u8_array(images):
        if isinstance(images, np.ndarray) and images.ndim == 4 and images.shape[0] > 0:
            # one contiguous [B, ny, nx, 3] block: the clip_image_u8 array without a Python loop (as encode_images; ~7 us per ctypes object)
            blk = np.ascontiguousarray(images, dtype=np.uint8)
            B = blk.shape[0]
            rec = np.empty(B, dtype=np.dtype([("nx", np.int32), ("ny", np.int32), ("data", np.uint64), ("size", np.uint64)], align=True))
            assert rec.dtype.itemsize == C.sizeof(ClipImageU8)
            rec["nx"], rec["ny"], rec["size"] = blk.shape[2], blk.shape[1], blk[0].size
            rec["data"] = blk.ctypes.data + np.arange(B, dtype=np.uint64) * np.uint64(blk.strides[0])
            return (blk, rec), C.cast(rec.ctypes.data, C.POINTER(ClipImageU8)), B
        keep = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        arr = (ClipImageU8 * len(keep))()
        for i, im in enumerate(keep):
            arr[i] = ClipImageU8(im.shape[1], im.shape[0], im.ctypes.data_as(C.POINTER(C.c_uint8)), im.size)
        return keep, arr, len(keep)

    def encode_images_u8(self, images, normalize=True):
        """list of uint8 [ny,nx,3] raw images (any sizes) -> float32 [n,proj]; resize/crop/normalise run on the GPU
        (clip_amd_image_batch_encode_u8), bit-identical to preprocess() + encode_images()."""
        keep, arr, n = self._u8_array(images)
        out = np.empty((n, self.vision_config["projection_dim"]), dtype=np.float32)
        if not lib().clip_amd_image_batch_encode_u8(self.ctx, arr, n, _fp(out), normalize):
            raise RuntimeError("clip_amd_image_batch_encode_u8 failed (see stderr)")
        return out

    @staticmethod
    def _boxes_array(boxes):
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int64).reshape(-1, 5))
        if b.size and (int(b.min()) < -2 ** 31 or int(b.max()) > 2 ** 31 - 1):
            raise ValueError("a box value does not fit 32 bits")
        return np.ascontiguousarray(b, dtype=np.int32)

    def encode_image_regions(self, images, boxes, normalize=True):
        """Boxes of raw images -> float32 [n_boxes, proj]: images is a list of uint8 [ny,nx,3] arrays, boxes an int array [n_boxes, 5] =
        image number, x, y, w, h (inside the image, w, h >= 1, any order, an image any number of times).  Row b is, bit for bit, row b of
        encode_images_u8 over the host crops images[i][y:y+h, x:x+w]; each image is uploaded once per staging piece, not once per box
        (clip_amd_image_batch_encode_regions)."""
        keep, arr, n = self._u8_array(images)
        b = self._boxes_array(boxes)
        out = np.empty((len(b), self.vision_config["projection_dim"]), dtype=np.float32)
        if not lib().clip_amd_image_batch_encode_regions(self.ctx, arr, n, b.ctypes.data_as(C.POINTER(C.c_int32)), len(b), _fp(out), normalize):
            raise RuntimeError("clip_amd_image_batch_encode_regions failed (see stderr)")
        return out

    def preprocess_regions_device(self, images, boxes, d_out_ptr):
        """preprocess_device for boxes of the images (boxes as encode_image_regions): [n_boxes,S,S,3] float32 at device address d_out_ptr"""
        keep, arr, n = self._u8_array(images)
        b = self._boxes_array(boxes)
        if not lib().clip_amd_image_batch_preprocess_regions_device(self.ctx, arr, n, b.ctypes.data_as(C.POINTER(C.c_int32)), len(b), C.c_void_p(d_out_ptr)):
            raise RuntimeError("clip_amd_image_batch_preprocess_regions_device failed (see stderr)")
        self.synchronize()

    class ImageFileList:
        """Paths prepared once for repeated Clip.encode_image_files(..., start=pos) calls over one long list: the encoded names and the
        C arrays are built here, each call then costs what its window costs."""

        def __init__(self, paths):
            self.paths = list(paths)
            self.n = len(self.paths)
            self.arr = (C.c_char_p * max(self.n, 1))(*[os.fsencode(p) for p in self.paths])
            self.ok = np.zeros(max(self.n, 1), dtype=np.uint8)

        def __len__(self):
            return self.n

    def _encode_encoded(self, call, arr, sizes, ok, n, normalize, n_threads, max_images, grid=1, grid_call=None):
        cap = n if max_images is None else max(0, min(int(max_images), n))
        grid = int(grid)
        if grid < 1 or grid > 8:
            raise ValueError("grid must be 1 ... 8, not %d" % grid)
        R = 1 if grid == 1 else 1 + grid * grid
        out = np.empty((cap * R, self.vision_config["projection_dim"]), dtype=np.float32)
        consumed = C.c_int(0)
        if n == 0 or cap == 0:
            return (out[:0], ok[:0].astype(bool), 0) + ((np.zeros((0, 4), dtype=np.int32),) if grid > 1 else ())
        args = (arr,) if sizes is None else (arr, sizes)
        if grid == 1:
            rows = call(self.ctx, *args, n, cap, int(n_threads), normalize, _fp(out), C.byref(consumed), ok.ctypes.data_as(C.POINTER(C.c_uint8)))
            if rows < 0:
                raise RuntimeError("%s failed (see stderr)" % call.__name__)
            return out[:rows], ok[:consumed.value].astype(bool), consumed.value
        boxes = np.zeros((cap * R, 4), dtype=np.int32)
        imgs = grid_call(self.ctx, *args, n, cap, int(n_threads), grid, normalize, _fp(out), boxes.ctypes.data_as(C.POINTER(C.c_int32)),
                         C.byref(consumed), ok.ctypes.data_as(C.POINTER(C.c_uint8)))
        if imgs < 0:
            raise RuntimeError("%s failed (see stderr)" % grid_call.__name__)
        return out[:imgs * R], ok[:consumed.value].astype(bool), consumed.value, boxes[:imgs * R]

    def encode_image_files(self, paths, normalize=True, n_threads=4, max_images=None, start=0, grid=1):
        """Image files -> (embeddings float32 [rows, proj], ok bool [consumed], consumed): the files are read and decoded on n_threads host
        threads, in every format clip_image_load_from_file reads, and the loadable ones encoded as ONE batch, bit-identical to
        clip_image_load_from_file + encode_images_u8.  Only a JPEG's entropy decoding stays on those threads: its IDCT / up-sampling / colour
        conversion run on the GPU (CLIP_AMD_JPEG_DEVICE=0 in the environment: on the host threads as well; same rows).  max_images: stop after that many loadable files; `consumed` paths were looked at, ok[i] says whether path i
        produced a row (clip_amd_image_batch_encode_files).  paths: a list, or a Clip.ImageFileList with `start` = the first path to
        look at, for walking a long list in windows without preparing the rest of it again for every call.
        grid = G > 1 (up to 8): every loadable image gives 1 + G * G consecutive rows, the whole image and then the tiles of grid_boxes(nx,
        ny, G), and a fourth value is returned: boxes int32 [rows, 4] = x, y, w, h of every row.  max_images, ok and consumed keep counting
        images; an image with a side shorter than G counts as not loadable.  Bit-identical to loading each file and one
        encode_image_regions call over those boxes; a JPEG decoded on the GPU is decoded once for all its regions."""
        fl = paths if isinstance(paths, Clip.ImageFileList) else Clip.ImageFileList(paths)
        start = max(0, min(int(start), fl.n))
        arr = C.cast(C.byref(fl.arr, start * C.sizeof(C.c_char_p)), C.POINTER(C.c_char_p))
        return self._encode_encoded(lib().clip_amd_image_batch_encode_files, arr, None, fl.ok[start:], fl.n - start, normalize, n_threads, max_images,
                                    grid, lib().clip_amd_image_batch_encode_files_grid)

    def encode_image_bytes(self, blobs, normalize=True, n_threads=4, max_images=None, grid=1):
        """The same for encoded images held in memory (a list of bytes objects): clip_amd_image_batch_encode_memory[_grid]."""
        blobs = [bytes(b) for b in blobs]
        n = len(blobs)
        arr = (C.c_char_p * max(n, 1))(*blobs)
        sizes = (C.c_size_t * max(n, 1))(*[len(b) for b in blobs])
        return self._encode_encoded(lib().clip_amd_image_batch_encode_memory, arr, sizes, np.zeros(max(n, 1), dtype=np.uint8)[:n], n, normalize, n_threads, max_images,
                                    grid, lib().clip_amd_image_batch_encode_memory_grid)

    def zero_shot_label_images(self, images, labels):
        """Batched clip_zero_shot_label_image on the GPU: list of uint8 [ny,nx,3] images x list of label strings ->
        (scores [B,n] sorted descending, indices [B,n])."""
        keep, arr, B = self._u8_array(images)
        n = len(labels)
        lab = (C.c_char_p * n)(*[l.encode("utf-8") for l in labels])
        scores = np.empty((B, n), dtype=np.float32)
        idx = np.empty((B, n), dtype=np.int32)
        if not lib().clip_amd_zero_shot_label_images(self.ctx, arr, B, lab, n, _fp(scores), idx.ctypes.data_as(C.POINTER(C.c_int))):
            raise RuntimeError("clip_amd_zero_shot_label_images failed (see stderr)")
        return scores, idx

    def preprocess_device(self, images, d_out_ptr):
        """list of uint8 [ny,nx,3] raw images -> [n,S,S,3] float32 at device address d_out_ptr (asynchronous)."""
        keep, arr, B = self._u8_array(images)
        if not lib().clip_amd_image_batch_preprocess_device(self.ctx, arr, B, C.c_void_p(d_out_ptr)):
            raise RuntimeError("clip_amd_image_batch_preprocess_device failed (see stderr)")
        self.synchronize()   # `keep` (the host pixels) must outlive the copy into the pinned blob — it does: the copy is synchronous

    @property
    def weights_from_cache(self):
        """True when this load read the repacked HBM image from CLIP_AMD_WEIGHT_CACHE instead of repacking the GGUF."""
        return bool(lib().clip_amd_weights_from_cache(self.ctx))

    @property
    def n_devices(self):
        return lib().clip_amd_ctx_device_count(self.ctx)

    def encode_images(self, imgs, normalize=True, n_threads=None):
        """float32 [B,S,S,3] preprocessed images (host) -> float32 [B,proj] via clip_image_batch_encode."""
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)
        B, S = imgs.shape[0], imgs.shape[1]
        # the clip_image_f32 array, filled without a Python loop (one ctypes object per image costs ~7 us: 1.8 ms per 256 images,
        # a third of the call); layout = struct clip_image_f32 {int nx, ny; float * data; size_t size;} (clip.h:57-64)
        rec = np.empty(B, dtype=np.dtype([("nx", np.int32), ("ny", np.int32), ("data", np.uint64), ("size", np.uint64)], align=True))
        assert rec.dtype.itemsize == C.sizeof(ClipImageF32)
        rec["nx"], rec["ny"], rec["size"] = S, imgs.shape[2], imgs[0].size if B else 0
        rec["data"] = imgs.ctypes.data + np.arange(B, dtype=np.uint64) * np.uint64(imgs.strides[0] if B else 0)
        batch = ClipImageF32Batch(C.cast(rec.ctypes.data, C.POINTER(ClipImageF32)), B)
        out = np.empty((B, self.vision_config["projection_dim"]), dtype=np.float32)
        if not lib().clip_image_batch_encode(self.ctx, n_threads or min(16, os.cpu_count() or 1), C.byref(batch), _fp(out), normalize):
            raise RuntimeError("clip_image_batch_encode failed (see stderr)")
        return out

    def encode_texts(self, token_lists, normalize=True):
        """list of int token lists -> float32 [n,proj] via clip_text_batch_encode (one ragged batch)."""
        n = len(token_lists)
        keep = [np.ascontiguousarray(t, dtype=np.int32) for t in token_lists]
        arr = (ClipTokens * n)()
        for i, t in enumerate(keep):
            arr[i] = ClipTokens(t.ctypes.data_as(C.POINTER(C.c_int32)), t.size)
        out = np.empty((n, self.text_config["projection_dim"]), dtype=np.float32)
        if not lib().clip_text_batch_encode(self.ctx, 1, C.cast(arr, C.POINTER(ClipTokens)), n, _fp(out), normalize):
            raise RuntimeError("clip_text_batch_encode failed (see stderr)")
        return out

    def set_stream(self, stream_handle):
        lib().clip_amd_set_stream(self.ctx, C.c_void_p(stream_handle))

    def set_device_shared(self, shared=True):
        """the caller runs other work on this device concurrently (clip_amd_set_device_shared: the other tower of a two-tower step)."""
        lib().clip_amd_set_device_shared(self.ctx, 1 if shared else 0)

    def synchronize(self):
        lib().clip_amd_synchronize(self.ctx)

    def encode_images_device(self, d_imgs_ptr, batch, d_out_ptr, normalize=True):
        """Device-resident batch encode: raw HBM pointers (ints), asynchronous on the ctx stream."""
        if not lib().clip_amd_image_batch_encode_device(self.ctx, C.c_void_p(d_imgs_ptr), batch, C.c_void_p(d_out_ptr), normalize):
            raise RuntimeError("clip_amd_image_batch_encode_device failed (see stderr)")

    def encode_texts_device(self, d_ids_ptr, offsets, d_out_ptr, normalize=True):
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        if not lib().clip_amd_text_batch_encode_device(self.ctx, C.c_void_p(d_ids_ptr), off.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       off.size - 1, C.c_void_p(d_out_ptr), normalize):
            raise RuntimeError("clip_amd_text_batch_encode_device failed (see stderr)")

    def encode_images_device_multi(self, d_img_ptrs, total, normalize=True, out=None):
        """Multi-GPU handle (n_devices=...): shard g of `total` preprocessed images already on device g at d_img_ptrs[g] (ints); one
        RCCL all-gather of the embeddings; returns the host copy [total, proj] when out is given (np.float32 array), else None."""
        arr = (C.c_void_p * len(d_img_ptrs))(*[C.c_void_p(p) for p in d_img_ptrs])
        if not lib().clip_amd_image_batch_encode_device_multi(self.ctx, arr, total, normalize, _fp(out) if out is not None else None):
            raise RuntimeError("clip_amd_image_batch_encode_device_multi failed (see stderr)")
        return out

    def encode_texts_device_multi(self, d_ids_ptrs, offsets, normalize=True, out=None):
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        arr = (C.c_void_p * len(d_ids_ptrs))(*[C.c_void_p(p) for p in d_ids_ptrs])
        if not lib().clip_amd_text_batch_encode_device_multi(self.ctx, arr, off.ctypes.data_as(C.POINTER(C.c_int32)), off.size - 1, normalize,
                                                             _fp(out) if out is not None else None):
            raise RuntimeError("clip_amd_text_batch_encode_device_multi failed (see stderr)")
        return out

    def encode_pair_device_multi(self, d_img_ptrs, n_images, d_ids_ptrs, offsets, normalize=True, out_img=None, out_txt=None):
        """Multi-GPU handle: both towers of a step in one call (clip_amd_encode_pair_device_multi) — per device the vision tower on the
        replica's stream and the text tower on a twin context's stream, ONE all-gather of both towers' rows."""
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        ia = (C.c_void_p * len(d_img_ptrs))(*[C.c_void_p(p) for p in d_img_ptrs])
        ta = (C.c_void_p * len(d_ids_ptrs))(*[C.c_void_p(p) for p in d_ids_ptrs])
        if not lib().clip_amd_encode_pair_device_multi(self.ctx, ia, n_images, ta, off.ctypes.data_as(C.POINTER(C.c_int32)), off.size - 1, normalize,
                                                       _fp(out_img) if out_img is not None else None, _fp(out_txt) if out_txt is not None else None):
            raise RuntimeError("clip_amd_encode_pair_device_multi failed (see stderr)")
        return out_img, out_txt

    def gathered_embeddings_ptr(self, device_index=0):
        return lib().clip_amd_gathered_embeddings(self.ctx, device_index)

    def profile(self, on=True):
        lib().clip_amd_profile_enable(self.ctx, on)

    def profile_report(self, reset=True):
        """dict tag -> dict(launches, ms, flops, bytes) from HIP events recorded around each launch."""
        n = lib().clip_amd_profile_report(self.ctx, None, 0, False)
        buf = C.create_string_buffer(n + 16)
        lib().clip_amd_profile_report(self.ctx, buf, n + 16, reset)
        out = {}
        for line in buf.value.decode().splitlines():
            tag, launches, ms, fl, by = line.split()
            out[tag] = dict(launches=int(launches), ms=float(ms), flops=float(fl), bytes=float(by))
        return out

    def close(self):
        if getattr(self, "ctx", None):
            for ix in list(getattr(self, "_indexes", ())):     # an index lives on this context: free it first
                ix.close()
            lib().clip_free(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grid_boxes(nx, ny, G):
    """int32 [R, 4] = x, y, w, h: the regions of an nx x ny image under a grid of G (1 ... 8), as clip_amd_image_batch_encode_files_grid
    makes them: the whole image alone for G = 1, else the whole image and then tile (i, j) = x in [i nx // G, (i + 1) nx // G), y in
    [j ny // G, (j + 1) ny // G), j outer and i inner (R = 1 + G * G).  ValueError for G outside 1 ... 8 or an image with a side shorter
    than G.  Pure arithmetic: needs no device."""
    nx, ny, G = int(nx), int(ny), int(G)
    if G < 1 or G > 8:
        raise ValueError("grid must be 1 ... 8, not %d" % G)
    if nx < 1 or ny < 1 or (G > 1 and min(nx, ny) < G):
        raise ValueError("a %dx%d image is too small for a grid of %d" % (nx, ny, G))
    rows = [(0, 0, nx, ny)]
    if G > 1:
        for j in range(G):
            for i in range(G):
                x, y = i * nx // G, j * ny // G
                rows.append((x, y, (i + 1) * nx // G - x, (j + 1) * ny // G - y))
    return np.array(rows, dtype=np.int32)


def allow_words(allow, n):
    """The uint64 words [(n + 63) // 64] of an allowed set over ids 0 ... n - 1 (the layout of clip_amd_index_search_subset: bit id & 63 of
    word id >> 6): `allow` is a bool array of length n or an integer array of ids (any order, duplicates allowed).  ValueError for a bool
    array of another length or an id outside [0, n).  Pure numpy: needs no device."""
    a = np.asarray(allow)
    if a.dtype == np.bool_:
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError("a bool allow mask must have one entry per id: shape (%d,), not %r" % (n, a.shape))
        bits = a
    else:
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("allow must be a bool mask or an integer array of ids, not %s" % a.dtype)
        ids = a.reshape(-1).astype(np.int64)
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n):
            raise ValueError("allow holds an id outside 0 ... %d" % (n - 1))
        bits = np.zeros(n, dtype=np.bool_)
        bits[ids] = True
    padded = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


class Index:
    """Exact cosine nearest-neighbour index on the GPU of a `Clip` (clip_amd_index_*, include/clip_amd.h): rows are L2-normalised and
    stored in f16 (default) or f32; search returns (distances f32 [nq, k], ids int64 [nq, k]) sorted by ascending 1 - cosine, equal
    distances lower id first, -1 / +inf past the index size.  range_search (every row within a radius of each query) and pairs (every pair
    of rows within a radius: near-duplicates) report the same distances, bit for bit.  Keep the `Clip` alive while the index is in use.
    A row or query with a NaN or an infinity is the zero vector (distance exactly 1 to everything); a finite one is normalised
    independently of its scale (x and x * 2**e store the same bits, from subnormals to values near the f32 maximum), so what the f32 /
    f16 index stores is always finite and within 1 in magnitude; load() refuses a file that holds anything else.

    "i8" (dtype code 3) stores each row as int8, a quarter of f32's bytes: in f32, amax = max |x|, q = rint((x / amax) * 127) (half to
    even; numpy: np.rint((x / amax).astype(np.float32) * np.float32(127))), no L2 normalisation first (the mapping is scale-invariant).
    Queries are quantised the same way at search time.  A vector with amax 0 or any NaN / inf is stored as the zero vector (distance
    exactly 1 to everything).  Distance = 1 - (float)dot * inv_q * inv_r with dot the exact int32 sum q_i r_i and inv = 1 / sqrtf(sum
    v_i^2) (0 for the zero vector): the cosine distance of the stored integer vectors, bit-reproducible like the other dtypes.

    components(radius) groups near-duplicates at any density: the connected components of the pairs graph as one label per row (the
    lowest id of the row's group) and every row's nearest near row, computed on the device; no pair list is ever made.

    modes(radius, link) organises a collection into albums, each with a cover: every row points to its nearest row of higher local density
    (density = its number of rows within `radius`; the parent is looked for within `link`), the roots of that forest are the modes, the
    most typical rows, and every tree is an album.  Exact and deterministic like everything else here.

    spread(n) answers "show me n rows that between them cover everything in here": greedy farthest-first selection (k-center).  From the
    seeds, or the lowest id, the row farthest from everything chosen so far is taken next, until n rows are chosen or nothing is farther
    than `radius` from a chosen one.  It needs no radius, returns exactly n rows (when there are that many), every prefix of them is
    within a factor 2 of the best possible cover, and reach[t] is the coverage radius of the t rows before it.  With `allow` it is the
    diverse-subset step after a search: ids of the 1000 nearest rows in, 20 of them spread apart out (spread(20, allow=ids)).

    linkage() answers for every radius at once: the minimum spanning tree of the rows under the index's distances, the single-linkage
    dendrogram.  cut_linkage(..., radius=R) on its edges gives the labels of components(R), cut_linkage(..., n_groups=N) exactly N
    groups, and the sorted edge distances are the table of radius against number of groups.  The edge order (d, lo, hi) is total, so the
    tree is unique, exact and bit-reproducible.

    extents(labels) measures any of these groupings: how far every row's own group reaches from it, and per group the minimax centre (the
    member whose farthest other member is nearest: a cover for groups that have none), the radius around it and the diameter, the largest
    distance inside the group.  It tells a tight burst of copies from a chain whose ends are far apart.

    remove(ids) marks rows as removed: no search, range_search or pairs returns them again, ids are not renumbered and len() keeps
    counting every id ever given (`live` = len minus the removed rows); compact() drops them from device memory and renumbers the
    survivors.  search and range_search take `allow`, a bool mask of length len(index) or an array of ids: only those rows (and of those
    only the live ones) are eligible.  Either way the result is, bit for bit, that of an index that only ever held the eligible rows.
    save() refuses an index that holds removed rows: compact() first.

    search_ids(ids, k) finds the neighbours of rows that are already stored ("more like this one"): the query is the row's stored values,
    bit for bit, so no vector and no model is needed; with exclude_self (the default) the row itself is not a candidate, and the result is
    what search gives for the added vector with that row's bit cleared in `allow`.  knn_graph(k) is the same for every row at once: its k
    nearest other live rows (an all -1 / +inf row for a removed id), from a tiled kernel on larger indexes.

    search_index(src, k) searches this index with the stored rows of another one of the same Clip, dim and dtype (every row, or `ids` of
    them): row t of the result is what search gives for the vector that was added to `src` as that row, bit for bit.  append(src) copies
    src's rows, bit for bit, to the end of this index.  Neither needs the vectors that were added, or a model; `src` must hold no removed
    rows (compact() it first).

    search_grouped(queries, k, groups) ranks groups of rows instead of rows (several crops of one image, ranked by image): `groups` names
    every row's group and a result holds each group at most once, represented by its best row.  Groups are an argument of the call, not
    state of the index.

    search_sets(queries, set_lims, k, groups) searches with query sets: the rows set_lims[s] ... set_lims[s + 1] - 1 stand for one thing (the
    regions of one image) and the result of a set holds the best stored rows over all of its rows, each group (without groups: each row)
    at most once, with the query row that matched.  search_ids_sets does the same with stored rows as the queries and can leave a set's
    own group out (two gridded images match through their best pair of regions, and no image matches itself); knn_graph_grouped is that
    for every group of the index at once.

    vote(queries, k, labels, m) files queries by example: `labels` gives every row a class (-1: unlabelled), the k nearest labelled rows
    vote, and the m best classes come back by votes, then by their nearest member, each with that member's distance and id; vote_ids takes
    stored rows as the queries and vote_graph every row at once, itself excluded: the audit of a labelling (clip_amd_index_vote*).

    search_distinct(queries, k, radius) folds near-duplicates into one hit: over the query's `pool` nearest rows, walked in search's order,
    a row within `radius` (the distance of pairs) of an earlier kept row is dropped and counted for it; search_ids_distinct does the same
    with stored rows as the queries.  Suppression is over the pool, not the whole index.

    search_compound(queries, k) takes compound queries of 1 ... 8 terms each, a term being a vector or a stored row's id with a kind: "all"
    terms rank (a row's score is its distance to its WORST all-term), "within" / "beyond" terms keep the rows at most / more than a bound
    away, and an "over" term keeps the rows that are farther from it than their score plus a bound ("a beach" but not "people")."""

    DTYPES = {"f32": 0, "f16": 1, "i8": 3}

    def __init__(self, clip, dim, dtype="f16", _handle=None):
        self.clip = clip
        if _handle is None:
            if dtype not in self.DTYPES:
                raise ValueError("dtype must be 'f16', 'f32' or 'i8', not %r" % (dtype,))
            _handle = lib().clip_amd_index_create(clip.ctx, int(dim), self.DTYPES[dtype])
            if not _handle:
                raise RuntimeError("clip_amd_index_create failed (see stderr)")
        self.handle = _handle
        self.dim = lib().clip_amd_index_dim(self.handle)
        if not hasattr(clip, "_indexes"):
            clip._indexes = weakref.WeakSet()
        clip._indexes.add(self)

    @classmethod
    def load(cls, clip, path):
        h = lib().clip_amd_index_load(clip.ctx, os.fsencode(path))
        if not h:
            raise RuntimeError("clip_amd_index_load failed for %r (see stderr)" % (path,))
        return cls(clip, 0, _handle=h)

    def __len__(self):
        return int(lib().clip_amd_index_size(self.handle))

    def len(self):
        return len(self)

    def add(self, vecs):
        """float32 [n, dim] rows (host); they get the next n ids."""
        v = np.ascontiguousarray(vecs, dtype=np.float32).reshape(-1, self.dim)
        if not lib().clip_amd_index_add(self._live(), _fp(v), v.shape[0]):
            raise RuntimeError("clip_amd_index_add failed (see stderr)")

    def add_device(self, ptr, n):
        """n float32 rows of dim values at device address ptr (asynchronous on the context's stream)."""
        if not lib().clip_amd_index_add_device(self._live(), C.c_void_p(ptr), int(n)):
            raise RuntimeError("clip_amd_index_add_device failed (see stderr)")

    def remove(self, ids):
        """Mark the rows `ids` (each in [0, len)) as removed; duplicates and rows removed before are fine.  Returns how many rows this call
        took from live to removed."""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        r = int(lib().clip_amd_index_remove(self._live(), a.ctypes.data_as(C.POINTER(C.c_int64)), a.size))
        if r < 0:
            raise RuntimeError("clip_amd_index_remove failed (see stderr)")
        return r

    @property
    def live(self):
        """rows that are not removed: len(index) minus the removed ones"""
        return int(lib().clip_amd_index_live(self._live()))

    def live_mask(self):
        """bool [len]: True for a live row"""
        n = len(self)
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        if not lib().clip_amd_index_live_mask(self._live(), words.ctypes.data_as(C.POINTER(C.c_uint64))):
            raise RuntimeError("clip_amd_index_live_mask failed (see stderr)")
        return np.unpackbits(words.astype("<u8").view(np.uint8), bitorder="little")[:n].astype(np.bool_)

    def compact(self):
        """Drop the removed rows; the survivors keep their order and become ids 0 ... live - 1.  Returns new_ids int64 [old len]: each old
        id's new id, -1 for a removed row."""
        new_ids = np.empty(len(self), dtype=np.int64)
        if lib().clip_amd_index_compact(self._live(), new_ids.ctypes.data_as(C.POINTER(C.c_int64))) < 0:
            raise RuntimeError("clip_amd_index_compact failed (see stderr)")
        return new_ids

    def _allow(self, allow):
        """(keep-alive array, pointer) of an allowed set; (None, NULL) for None"""
        if allow is None:
            return None, None
        words = allow_words(allow, len(self))
        return words, words.ctypes.data_as(C.POINTER(C.c_uint64))

    def search(self, queries, k, allow=None):
        """(distances f32 [nq, k], ids int64 [nq, k]); `allow` (bool mask [len] or ids): only those rows are eligible"""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        words, wp = self._allow(allow)
        dist = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        if not lib().clip_amd_index_search_subset(self._live(), _fp(q), nq, int(k), wp, _fp(dist), ids.ctypes.data_as(C.POINTER(C.c_int64))):
            raise RuntimeError("clip_amd_index_search%s failed (see stderr)" % ("" if allow is None else "_subset"))
        return dist, ids

    def search_grouped(self, queries, k, groups, allow=None):
        """search with each group at most once in a result: `groups` (int [len], each >= 0) is every row's group, any numbering.  With L the
        eligible rows in search's order, a query's result is the rows of L whose group has not appeared earlier in L, cut to k: (distances
        f32 [nq, k], ids int64 [nq, k]) hold the best row of each of the k best groups and that row's distance, the bits `search` reports
        for it; -1 / +inf where there are fewer groups.  All groups distinct: search's result.  ValueError for a wrong length or a
        negative group."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        if groups is None:
            raise ValueError("groups must be integers, not None")
        g, gp = self._groups(groups)
        words, wp = self._allow(allow)
        dist = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        if not lib().clip_amd_index_search_grouped(self._live(), _fp(q), nq, int(k), gp, wp, _fp(dist),
                                                   ids.ctypes.data_as(C.POINTER(C.c_int64))):
            raise RuntimeError("clip_amd_index_search_grouped failed (see stderr)")
        return dist, ids

    def search_grouped_device(self, d_queries, n_queries, k, d_groups, d_allow, d_distances, d_ids):
        """search_grouped on device pointers (ints): queries [n, dim] f32, groups [len] int32 (trusted: each >= 0), d_allow uint64 words
        (0 / None: every row) -> distances [n, k] f32, ids [n, k] int64; asynchronous on the context's stream."""
        if not lib().clip_amd_index_search_grouped_device(self._live(), C.c_void_p(d_queries), int(n_queries), int(k), C.c_void_p(d_groups or None),
                                                          C.c_void_p(d_allow or None), C.c_void_p(d_distances), C.c_void_p(d_ids)):
            raise RuntimeError("clip_amd_index_search_grouped_device failed (see stderr)")

    @staticmethod
    def _set_lims(set_lims, n_rows):
        """set_lims as a contiguous int64 array after the checks of the library (ValueError): it starts at 0, never decreases and ends at
        n_rows.  Pure numpy: needs no device."""
        a = np.asarray(set_lims)
        if a.ndim != 1 or a.size < 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("set_lims must be a one-dimensional integer array of n_sets + 1 entries")
        a = np.ascontiguousarray(a, dtype=np.int64)
        if int(a[0]) != 0:
            raise ValueError("set_lims must start at 0, not at %d" % int(a[0]))
        if a.size > 1 and bool(np.any(np.diff(a) < 0)):
            raise ValueError("set_lims must not decrease (entry %d)" % (int(np.argmax(np.diff(a) < 0)) + 1))
        if int(a[-1]) != n_rows:
            raise ValueError("set_lims must end at the %d query rows, not at %d" % (n_rows, int(a[-1])))
        return a

    def _groups(self, groups):
        """(keep-alive int32 array, pointer) of one group per row (ValueError for a wrong length, a non-integer or a group outside 0 ...
        2^31 - 1); (None, NULL) for None"""
        if groups is None:
            return None, None
        g = np.asarray(groups)
        if g.size and not np.issubdtype(g.dtype, np.integer):
            raise ValueError("groups must be integers, not %s" % g.dtype)
        g = g.reshape(-1)
        if g.size != len(self):
            raise ValueError("groups must have one entry per row: %d, not %d" % (len(self), g.size))
        if g.size and (int(g.min()) < 0 or int(g.max()) > 2 ** 31 - 1):
            raise ValueError("groups must lie in 0 ... 2^31 - 1")
        g = np.zeros(g.size + 1, dtype=np.int32)[:g.size] if g.size == 0 else np.ascontiguousarray(g, dtype=np.int32)
        return g, g.ctypes.data_as(C.POINTER(C.c_int32))

    def search_sets(self, queries, set_lims, k, groups=None, allow=None):
        """Search with query sets: set s is the query rows set_lims[s] ... set_lims[s + 1] - 1 (set_lims int [n_sets + 1], from 0 to the
        number of rows, non-decreasing; an empty set gives an all-empty result).  Per set, every pair (query row q, eligible stored row r)
        in the order distance ascending, then r, then q, keeping a pair when the group of r (`groups`, int [len]; None: r itself) has not
        appeared earlier, cut to k: (distances f32 [n_sets, k], ids int64 [n_sets, k], qrows int32 [n_sets, k]), the stored row and the
        query row (its index in `queries`) of each kept pair and the distance `search` reports for the two; +inf / -1 / -1 where there
        are fewer.  Sets of one row: search_grouped's result (search's without groups).  ValueError for a malformed set_lims or groups."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        lims = self._set_lims(set_lims, q.shape[0])
        g, gp = self._groups(groups)
        words, wp = self._allow(allow)
        ns = lims.size - 1
        dist = np.empty((ns, k), dtype=np.float32)
        ids = np.empty((ns, k), dtype=np.int64)
        qrows = np.empty((ns, k), dtype=np.int32)
        if not lib().clip_amd_index_search_sets(self._live(), _fp(q), q.shape[0], lims.ctypes.data_as(C.POINTER(C.c_int64)), ns, int(k), gp, wp,
                                                _fp(dist), ids.ctypes.data_as(C.POINTER(C.c_int64)), qrows.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError("clip_amd_index_search_sets failed (see stderr)")
        return dist, ids, qrows

    def search_ids_sets(self, ids, set_lims, k, groups=None, exclude_own=True, allow=None):
        """search_sets with the stored rows `ids` (each a live id; duplicates are fine) as the query rows, bit for bit as search_ids takes
        them (a row is not excluded as itself).  exclude_own (needs `groups`): a stored row of the group of the query row is not eligible
        for that query row, so a group never matches itself.  Returns (distances, ids, qrows) as search_sets, qrows indexing `ids`."""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        lims = self._set_lims(set_lims, a.size)
        g, gp = self._groups(groups)
        if exclude_own and g is None:
            raise ValueError("exclude_own needs groups")
        words, wp = self._allow(allow)
        ns = lims.size - 1
        dist = np.empty((ns, k), dtype=np.float32)
        out = np.empty((ns, k), dtype=np.int64)
        qrows = np.empty((ns, k), dtype=np.int32)
        if not lib().clip_amd_index_search_ids_sets(self._live(), a.ctypes.data_as(C.POINTER(C.c_int64)), a.size, lims.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    ns, int(k), int(bool(exclude_own)), gp, wp, _fp(dist), out.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    qrows.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError("clip_amd_index_search_ids_sets failed (see stderr)")
        return dist, out, qrows

    def search_sets_device(self, d_queries, n_queries, set_lims, k, d_groups, d_allow, d_distances, d_ids, d_qrows):
        """search_sets on device pointers (ints): queries [n, dim] f32, groups [len] int32 (trusted; 0 / None: no groups), d_allow uint64
        words (0 / None: every row) -> distances [n_sets, k] f32, ids [n_sets, k] int64, qrows [n_sets, k] int32; set_lims is a host array
        (it shapes the launches); asynchronous on the context's stream."""
        lims = self._set_lims(set_lims, int(n_queries))
        if not lib().clip_amd_index_search_sets_device(self._live(), C.c_void_p(d_queries or None), int(n_queries), lims.ctypes.data_as(C.POINTER(C.c_int64)),
                                                       lims.size - 1, int(k), C.c_void_p(d_groups or None), C.c_void_p(d_allow or None),
                                                       C.c_void_p(d_distances or None), C.c_void_p(d_ids or None), C.c_void_p(d_qrows or None)):
            raise RuntimeError("clip_amd_index_search_sets_device failed (see stderr)")

    MAX_POOL = 1024

    @classmethod
    def _distinct_args(cls, k, radius, pool):
        """(k, radius, pool) of a distinct search after the checks of the library that need no device (ValueError): 1 <= k <= pool <= 1024
        with pool 0 standing for min(1024, max(64, 8 k)), and a radius that is a number.  The pool returned is what the caller passed."""
        k, pool, radius = int(k), int(pool), float(radius)
        if k < 1 or k > cls.MAX_POOL:
            raise ValueError("k = %d outside 1 ... %d" % (k, cls.MAX_POOL))
        if pool < 0 or pool > cls.MAX_POOL:
            raise ValueError("pool = %d outside 1 ... %d (0: automatic)" % (pool, cls.MAX_POOL))
        if pool and k > pool:
            raise ValueError("k = %d exceeds pool = %d" % (k, pool))
        if radius != radius:
            raise ValueError("radius is NaN")
        return k, radius, pool

    def search_distinct(self, queries, k, radius, pool=0, allow=None):
        """search with near-duplicates folded into one hit.  The pool L is search(query, pool, allow) without its empty tail; two members
        with ids i < j are near when d(i, j) <= radius in f32, d being the distance of pairs (so exactly when pairs(radius) lists them).
        Walking L in order, a member that an earlier kept member is near to is suppressed (and suppresses nothing itself), every other one
        is kept, until k are kept: (distances f32 [nq, k], ids int64 [nq, k], counts int32 [nq, k]), counts[t] the pool members kept
        member t suppressed (each counted once, for the first kept member near it; over the whole pool); +inf / -1 / 0 where fewer are
        kept.  Suppression is over the pool, not the whole index.  1 <= k <= pool <= 1024; pool 0: min(1024, max(64, 8 k)).  radius < 0:
        search's result with counts 0.  ValueError for a wrong shape of queries, k > pool, or a NaN radius."""
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim not in (1, 2) or q.shape[-1] != self.dim:
            raise ValueError("queries must be [n, %d] (or one vector of %d values), not %r" % (self.dim, self.dim, q.shape))
        q = np.ascontiguousarray(q).reshape(-1, self.dim)
        k, radius, pool = self._distinct_args(k, radius, pool)
        nq = q.shape[0]
        words, wp = self._allow(allow)
        dist = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        counts = np.empty((nq, k), dtype=np.int32)
        if not lib().clip_amd_index_search_distinct(self._live(), _fp(q), nq, k, radius, pool, wp, _fp(dist), ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    counts.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError("clip_amd_index_search_distinct failed (see stderr)")
        return dist, ids, counts

    def search_ids_distinct(self, ids, k, radius, pool=0, exclude_self=True, allow=None):
        """search_distinct with the stored rows `ids` (each a live id; duplicates are fine) as the queries, bit for bit as search_ids takes
        them.  exclude_self: the query's own row is not in the pool, so it is neither a hit nor a suppressor.  Returns (distances, ids,
        counts) as search_distinct."""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        k, radius, pool = self._distinct_args(k, radius, pool)
        words, wp = self._allow(allow)
        dist = np.empty((a.size, k), dtype=np.float32)
        out = np.empty((a.size, k), dtype=np.int64)
        counts = np.empty((a.size, k), dtype=np.int32)
        if not lib().clip_amd_index_search_ids_distinct(self._live(), a.ctypes.data_as(C.POINTER(C.c_int64)), a.size, k, radius, pool,
                                                        int(bool(exclude_self)), wp, _fp(dist), out.ctypes.data_as(C.POINTER(C.c_int64)),
                                                        counts.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError("clip_amd_index_search_ids_distinct failed (see stderr)")
        return dist, out, counts

    def search_distinct_device(self, d_queries, n_queries, k, radius, d_distances, d_ids, d_counts, pool=0, d_allow=None):
        """search_distinct on device pointers (ints): queries [n, dim] f32, d_allow uint64 words (0 / None: every row) -> distances [n, k]
        f32, ids [n, k] int64, counts [n, k] int32; asynchronous on the context's stream."""
        k, radius, pool = self._distinct_args(k, radius, pool)
        if not lib().clip_amd_index_search_distinct_device(self._live(), C.c_void_p(d_queries or None), int(n_queries), k, radius, pool,
                                                           C.c_void_p(d_allow or None), C.c_void_p(d_distances or None), C.c_void_p(d_ids or None),
                                                           C.c_void_p(d_counts or None)):
            raise RuntimeError("clip_amd_index_search_distinct_device failed (see stderr)")

    COMPOUND_KINDS = {"all": 0, "within": 1, "beyond": 2, "over": 3}
    MAX_TERMS = 8

    @classmethod
    def _compound_args(cls, queries, dim):
        """The flat arrays of a compound call after the checks of the library that need no device (ValueError): (terms f32 [total, dim],
        term_ids int64 [total] (-1: a vector), kinds int32 [total], bounds f32 [total], term_lims int64 [nq + 1]).  `queries` is a list of
        compound queries, each a list of 1 ... 8 terms (what, kind) or (what, kind, bound): `what` a vector of dim values or an int id,
        `kind` "all" (at least one per query), "within", "beyond" (both need a bound) or "over" (bound 0 unless given)."""
        terms, term_ids, kinds, bounds, lims = [], [], [], [], [0]
        for c, query in enumerate(queries):
            query = list(query)
            if not query:
                raise ValueError("query %d has no terms" % c)
            if len(query) > cls.MAX_TERMS:
                raise ValueError("query %d has %d terms, more than %d" % (c, len(query), cls.MAX_TERMS))
            for term in query:
                if not isinstance(term, (tuple, list)) or len(term) not in (2, 3):
                    raise ValueError("a term of query %d is not (what, kind) or (what, kind, bound): %r" % (c, term))
                what, kind = term[0], term[1]
                if not isinstance(kind, str) or kind not in cls.COMPOUND_KINDS:
                    raise ValueError("query %d: unknown kind %r (known: %s)" % (c, kind, ", ".join(cls.COMPOUND_KINDS)))
                if len(term) == 3 and term[2] is not None:
                    bound = float(term[2])
                elif kind in ("within", "beyond"):
                    raise ValueError("query %d: a %r term needs a bound" % (c, kind))
                else:
                    bound = 0.0
                if bound != bound:
                    raise ValueError("query %d: the bound of a %r term is NaN" % (c, kind))
                if isinstance(what, (int, np.integer)) and not isinstance(what, (bool, np.bool_)):
                    if int(what) < 0:
                        raise ValueError("query %d: the id %d of a term is negative" % (c, int(what)))
                    term_ids.append(int(what))
                    terms.append(np.zeros(dim, dtype=np.float32))
                else:
                    v = np.asarray(what, dtype=np.float32)
                    if v.shape != (dim,):
                        raise ValueError("query %d: a term's vector must have %d values, not the shape %r" % (c, dim, v.shape))
                    term_ids.append(-1)
                    terms.append(v)
                kinds.append(cls.COMPOUND_KINDS[kind])
                bounds.append(bound)
            if cls.COMPOUND_KINDS["all"] not in kinds[lims[-1]:]:
                raise ValueError("query %d has no \"all\" term to rank by" % c)
            lims.append(len(kinds))
        if len(lims) < 2:
            raise ValueError("no queries")
        return (np.ascontiguousarray(np.stack(terms), dtype=np.float32), np.asarray(term_ids, dtype=np.int64), np.asarray(kinds, dtype=np.int32),
                np.asarray(bounds, dtype=np.float32), np.asarray(lims, dtype=np.int64))

    def search_compound(self, queries, k, allow=None, exclude_terms=True):
        """Compound queries: `queries` is a list of queries, each a list of 1 ... 8 terms (what, kind) or (what, kind, bound); `what` is a
        vector or the int id of a stored row (taken bit for bit, as search_ids takes it).  With d_t(row) the distance `search` reports for
        (term t, row): score(row) = the max of d_t over the query's "all" terms (at least one); a "within" term keeps the rows with d_t <=
        bound, a "beyond" term those with d_t > bound, an "over" term those with d_t > score + bound in f32 (bound 0 unless given: the
        row is strictly nearer to what is asked for than to this term).  Eligible rows are live, in `allow` and pass every filter;
        exclude_terms: the stored rows that are terms of a query are not eligible for it.  Returns (distances f32 [nq, k], ids int64 [nq,
        k]): the k best eligible rows by (score, id), the distance being the score; +inf / -1 where there are fewer.  A single "all" term
        is search's result.  ValueError for an empty query, more than 8 terms, no "all" term, a missing or NaN bound, an unknown kind or a
        vector of the wrong length."""
        terms, term_ids, kinds, bounds, lims = self._compound_args(queries, self.dim)
        nq = lims.size - 1
        words, wp = self._allow(allow)
        dist = np.empty((nq, int(k)), dtype=np.float32)
        ids = np.empty((nq, int(k)), dtype=np.int64)
        if not lib().clip_amd_index_search_compound(self._live(), _fp(terms), term_ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    kinds.ctypes.data_as(C.POINTER(C.c_int32)), _fp(bounds), lims.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    nq, int(k), int(bool(exclude_terms)), wp, _fp(dist), ids.ctypes.data_as(C.POINTER(C.c_int64))):
            raise RuntimeError("clip_amd_index_search_compound failed (see stderr)")
        return dist, ids

    def search_compound_device(self, d_terms, term_ids, kinds, bounds, term_lims, k, d_distances, d_ids, exclude_terms=True, d_allow=None):
        """search_compound on device pointers (ints) in the flat form of the library: d_terms [total, dim] f32 in HBM; term_ids int64
        [total] (>= 0: that stored row replaces the vector; None: no id terms), kinds int32 [total] (0 all, 1 within, 2 beyond, 3 over),
        bounds f32 [total] and term_lims int64 [nq + 1] are host arrays, read before the call returns; d_allow uint64 words (0 / None:
        every row) -> distances [nq, k] f32, ids [nq, k] int64; asynchronous on the context's stream.  An id term that is out of range or
        removed gives an all-empty row."""
        kinds = np.ascontiguousarray(kinds, dtype=np.int32).reshape(-1)
        bounds = np.ascontiguousarray(bounds, dtype=np.float32).reshape(-1)
        lims = np.ascontiguousarray(term_lims, dtype=np.int64).reshape(-1)
        tid = None if term_ids is None else np.ascontiguousarray(term_ids, dtype=np.int64).reshape(-1)
        if lims.size < 2 or kinds.size != int(lims[-1]) or bounds.size != kinds.size or (tid is not None and tid.size != kinds.size):
            raise ValueError("term_lims must end at the %d terms that kinds, bounds and term_ids hold" % kinds.size)
        if not lib().clip_amd_index_search_compound_device(self._live(), C.c_void_p(d_terms or None),
                                                           None if tid is None else tid.ctypes.data_as(C.POINTER(C.c_int64)),
                                                           kinds.ctypes.data_as(C.POINTER(C.c_int32)), _fp(bounds), lims.ctypes.data_as(C.POINTER(C.c_int64)),
                                                           lims.size - 1, int(k), int(bool(exclude_terms)), C.c_void_p(d_allow or None),
                                                           C.c_void_p(d_distances or None), C.c_void_p(d_ids or None)):
            raise RuntimeError("clip_amd_index_search_compound_device failed (see stderr)")

    def knn_graph_grouped(self, k, groups):
        """The k-NN graph of the groups (images of a gridded index): (labels, distances, ids, qids).  labels int64 [G]: the distinct groups
        of the live rows, ascending, one result row each; distances f32 / ids int64 / qids int64 [G, k]: the label's k nearest OTHER
        groups by their best pair of rows, ids the other group's row and qids the label's own row of that pair; +inf / -1 / -1 where
        there are fewer other groups.  One search_ids_sets(exclude_own=True) over the live rows stably sorted by group."""
        g, _ = self._groups(groups)
        rows = np.flatnonzero(self.live_mask()).astype(np.int64)
        order = rows[np.argsort(g[rows], kind="stable")]
        labels, counts = np.unique(g[order], return_counts=True)
        lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        dist, ids, qrows = self.search_ids_sets(order, lims, k, groups=g, exclude_own=True)
        qids = np.where(qrows >= 0, order[np.maximum(qrows, 0)] if order.size else -1, -1).astype(np.int64)
        return labels.astype(np.int64), dist, ids, qids

    def range_search(self, queries, radius, allow=None):
        """Every stored row within `radius` of each query (distance <= radius in f32, the distance `search` reports): (lims int64 [nq + 1],
        distances f32 [total], ids int64 [total]); query q's results are [lims[q], lims[q + 1]), nearest first, equal distances lower id
        first.  `allow` (bool mask [len] or ids): only those rows are eligible."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        words, wp = self._allow(allow)
        call = lambda lims, d, i, cap: lib().clip_amd_index_range_search_subset(self._live(), _fp(q), nq, float(radius), wp, lims, d, i, cap)
        return self._join(call, nq + 1, 64 * nq + 1024, "clip_amd_index_range_search" + ("" if allow is None else "_subset"))

    def pairs(self, radius):
        """Every pair of rows i < j at distance <= radius, d(i, j) being what `search` reports for row j when queried with the vector added
        as row i: (i int64 [P], j int64 [P], distances f32 [P]), grouped by ascending i, within one i nearest first, equal distances lower j
        first."""
        n = len(self)
        call = lambda lims, d, i, cap: lib().clip_amd_index_pairs(self._live(), float(radius), lims, d, i, cap)
        lims, dist, j = self._join(call, n + 1, 4 * n + 1024, "clip_amd_index_pairs")
        return np.repeat(np.arange(n, dtype=np.int64), np.diff(lims)), j, dist

    def components(self, radius, allow=None):
        """Connected components of the graph whose edges are the pairs of `pairs(radius)`, without the pairs ever leaving the device:
        (labels int64 [n], nearest_distance f32 [n], nearest_id int64 [n]).  labels[x] is the lowest id of x's component (x itself when no
        row is near it, -1 for a removed or not allowed row); nearest_distance[x] / nearest_id[x] are the smallest distance of a pair x
        is in and the other row of that pair (the lower id among equal distances), +inf / -1 without one.  `allow` (bool mask [len] or
        ids): only those rows are eligible.  The components of two or more rows are the roots (labels[x] == x) with a nearest id."""
        n = len(self)
        words, wp = self._allow(allow)
        labels = np.empty(n, dtype=np.int64)
        dist = np.empty(n, dtype=np.float32)
        ids = np.empty(n, dtype=np.int64)
        if lib().clip_amd_index_components(self._live(), float(radius), wp, labels.ctypes.data_as(C.POINTER(C.c_int64)), _fp(dist),
                                           ids.ctypes.data_as(C.POINTER(C.c_int64))) < 0:
            raise RuntimeError("clip_amd_index_components failed (see stderr)")
        return labels, dist, ids

    def components_device(self, radius, d_labels, d_nearest_distance=None, d_nearest_id=None, d_allow=None):
        """components on device pointers (ints): labels [n] int64, nearest_distance [n] f32 and nearest_id [n] int64 (0 / None: not
        wanted); d_allow: uint64 words on the device (0 / None: every row); asynchronous on the context's stream."""
        if not lib().clip_amd_index_components_device(self._live(), float(radius), C.c_void_p(d_allow or None), C.c_void_p(d_labels),
                                                      C.c_void_p(d_nearest_distance or None), C.c_void_p(d_nearest_id or None)):
            raise RuntimeError("clip_amd_index_components_device failed (see stderr)")

    @staticmethod
    def _modes_scales(radius, link):
        """(radius, link) as the f32 values the library compares with; link None: radius.  ValueError for a NaN, before any call."""
        radius = float(np.float32(radius))
        link = radius if link is None else float(np.float32(link))
        if radius != radius or link != link:
            raise ValueError("radius and link must not be NaN")
        return radius, link

    def modes(self, radius, link=None, allow=None):
        """Density modes: (labels int64 [n], parent int64 [n], parent_distance f32 [n], density int32 [n]).  density[x] is the number of other
        eligible rows within `radius` of x (the distance and the <= of `pairs`).  y outranks x when density[y] > density[x], or the
        densities are equal and y < x.  parent[x] is the nearest row within `link` (default: radius) among those that outrank x, the lower
        id among equal distances, -1 when there is none; parent_distance[x] the distance to it, the bits `pairs` reports, +inf without a
        parent; labels[x] the root reached by following parent: the cover of x's album.  A removed or not allowed row gets -1, -1, +inf,
        -1.  The modes are the rows with labels[x] == x, singletons included.  `allow` (bool mask [len] or ids): only those rows are
        eligible; the result over them is that of an index that only ever held them.  ValueError for a NaN or a malformed allow."""
        radius, link = self._modes_scales(radius, link)
        n = len(self)
        words, wp = self._allow(allow)
        labels = np.empty(n, dtype=np.int64)
        parent = np.empty(n, dtype=np.int64)
        dist = np.empty(n, dtype=np.float32)
        density = np.empty(n, dtype=np.int32)
        if lib().clip_amd_index_modes(self._live(), radius, link, wp, labels.ctypes.data_as(C.POINTER(C.c_int64)),
                                      parent.ctypes.data_as(C.POINTER(C.c_int64)), _fp(dist), density.ctypes.data_as(C.POINTER(C.c_int32))) < 0:
            raise RuntimeError("clip_amd_index_modes failed (see stderr)")
        return labels, parent, dist, density

    def modes_device(self, radius, d_labels, link=None, d_parent=None, d_parent_distance=None, d_density=None, d_allow=None):
        """modes on device pointers (ints): labels [n] int64, parent [n] int64, parent_distance [n] f32 and density [n] int32 (0 / None: not
        wanted); d_allow: uint64 words on the device (0 / None: every row); asynchronous on the context's stream."""
        radius, link = self._modes_scales(radius, link)
        if not lib().clip_amd_index_modes_device(self._live(), radius, link, C.c_void_p(d_allow or None), C.c_void_p(d_labels),
                                                 C.c_void_p(d_parent or None), C.c_void_p(d_parent_distance or None), C.c_void_p(d_density or None)):
            raise RuntimeError("clip_amd_index_modes_device failed (see stderr)")

    @staticmethod
    def _linkage_link(link):
        """link as the f32 the library compares with; None: +inf, the whole tree.  ValueError for a NaN, before any call."""
        link = float("inf") if link is None else float(np.float32(link))
        if link != link:
            raise ValueError("link must not be NaN")
        return link

    def linkage(self, link=None, allow=None):
        """The single-linkage tree: (lo int64 [e], hi int64 [e], d f32 [e]), the edges of the minimum spanning forest of the graph
        "distance <= link" (default: no limit, the whole tree) over the eligible rows, lo < hi, sorted by (d, lo, hi): that is the order
        of the edges, it is total, and an edge is in the forest exactly when strictly smaller edges do not connect its ends.  d are the
        distances and bits of `pairs`.  e = eligible rows - components at link.  cut_linkage turns the edges into labels for any radius
        or any number of groups.  `allow` (bool mask [len] or ids): only those rows are eligible; the result over them is that of an
        index that only ever held them.  ValueError for a NaN or a malformed allow."""
        link = self._linkage_link(link)
        cap = max(len(self) - 1, 1)
        words, wp = self._allow(allow)
        lo = np.empty(cap, dtype=np.int64)
        hi = np.empty(cap, dtype=np.int64)
        dist = np.empty(cap, dtype=np.float32)
        i64 = C.POINTER(C.c_int64)
        m = lib().clip_amd_index_linkage(self._live(), link, wp, lo.ctypes.data_as(i64), hi.ctypes.data_as(i64), _fp(dist))
        if m < 0:
            raise RuntimeError("clip_amd_index_linkage failed (see stderr)")
        return lo[:m].copy(), hi[:m].copy(), dist[:m].copy()

    def linkage_rounds(self):
        """The rounds that did work in the last `linkage` call of this index: sweeps over the pairs that ran (for measurements)"""
        return int(lib().clip_amd_test_index_linkage_rounds(self._live()))

    def linkage_device(self, d_lo, d_hi, d_distances, d_count, link=None, d_allow=None):
        """linkage on device pointers (ints): lo [len - 1] int64, hi [len - 1] int64, distances [len - 1] f32 and count [1] int64, the
        same edges as the host form in an order that is not specified but the same run to run; d_allow: uint64 words on the device
        (0 / None: every row); asynchronous on the context's stream."""
        link = self._linkage_link(link)
        if not lib().clip_amd_index_linkage_device(self._live(), link, C.c_void_p(d_allow or None), C.c_void_p(d_lo or None),
                                                   C.c_void_p(d_hi or None), C.c_void_p(d_distances or None), C.c_void_p(d_count or None)):
            raise RuntimeError("clip_amd_index_linkage_device failed (see stderr)")

    @staticmethod
    def _core_k(k):
        """k of linkage_core as an int; ValueError outside 0 ... 1024, before any call"""
        k = int(k)
        if k < 0 or k > 1024:
            raise ValueError("k = %d outside 0 ... 1024" % k)
        return k

    def linkage_core(self, k, link=None, allow=None):
        """The mutual-reachability tree (robust single linkage): (lo int64 [e], hi int64 [e], w f32 [e], core f32 [len]).  core[x] is the
        distance from x to its k-th nearest other eligible row, the bits search_ids(x, k, exclude_self=True, allow=...) reports (-inf for
        k = 0, inf with fewer than k other rows and for every row that is not eligible); w(x, y) = max(d(x, y), core[x], core[y]); the
        edges are the minimum spanning forest of the graph "w <= link" under the order (w, lo, hi), sorted by it.  A stray row between two
        dense groups has a large core distance, so it no longer chains them together.  k = 0 is `linkage`.  cut_linkage(..., radius=R)
        gives DBSCAN* at R with min_pts = k + 1: the rows with core <= R labelled as components(R, allow=core <= R) labels them, every
        other eligible row on its own; cut_linkage_sized picks the radius from a number of groups.  ValueError for a k outside 0 ... 1024,
        a NaN link or a malformed allow."""
        k = self._core_k(k)
        link = self._linkage_link(link)
        cap = max(len(self) - 1, 1)
        words, wp = self._allow(allow)
        lo = np.empty(cap, dtype=np.int64)
        hi = np.empty(cap, dtype=np.int64)
        w = np.empty(cap, dtype=np.float32)
        core = np.empty(max(len(self), 1), dtype=np.float32)
        i64 = C.POINTER(C.c_int64)
        m = lib().clip_amd_index_linkage_core(self._live(), k, link, wp, lo.ctypes.data_as(i64), hi.ctypes.data_as(i64), _fp(w), _fp(core))
        if m < 0:
            raise RuntimeError("clip_amd_index_linkage_core failed (see stderr)")
        return lo[:m].copy(), hi[:m].copy(), w[:m].copy(), core[:len(self)].copy()

    def linkage_core_device(self, k, d_lo, d_hi, d_weights, d_count, d_core=None, link=None, d_allow=None):
        """linkage_core on device pointers (ints): lo [len - 1] int64, hi [len - 1] int64, weights [len - 1] f32, count [1] int64 and,
        if wanted, core [len] f32; the same edges as the host form in an order that is not specified but the same run to run; d_allow:
        uint64 words on the device (0 / None: every row); asynchronous on the context's stream."""
        k = self._core_k(k)
        link = self._linkage_link(link)
        if not lib().clip_amd_index_linkage_core_device(self._live(), k, link, C.c_void_p(d_allow or None), C.c_void_p(d_lo or None),
                                                        C.c_void_p(d_hi or None), C.c_void_p(d_weights or None), C.c_void_p(d_core or None),
                                                        C.c_void_p(d_count or None)):
            raise RuntimeError("clip_amd_index_linkage_core_device failed (see stderr)")

    def _extents_labels(self, labels, words=None):
        """labels as int64 [len]; ValueError for another length, or a label >= len on a row of the allowed set (words of _allow; None:
        on any row), before the library is reached"""
        size = len(self)
        a = np.asarray(labels)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("labels must be integers, not %s" % a.dtype)
        a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
        if a.size != size:
            raise ValueError("labels holds %d entries, the index %d rows" % (a.size, size))
        checked = a if words is None else a[np.unpackbits(words.astype("<u8").view(np.uint8), bitorder="little")[:size].astype(np.bool_)]
        if checked.size and int(checked.max()) >= size:
            raise ValueError("labels holds %d: a label is negative (not a member) or an id of the index (0 ... %d)" % (int(checked.max()), size - 1))
        return a

    def extents(self, labels, allow=None):
        """Extents of a labelling: (centre int64 [n], radius f32 [n], diameter f32 [n], reach f32 [n], far int64 [n]).  `labels` int64
        [len]: row x is a member when it is eligible and labels[x] >= 0; its group is the members that carry its label (the labels of
        components, modes, cut_linkage and spread's owner all qualify; a label must be < len and need not be a member of its group).
        reach[x] is the largest distance (the distances and bits of `pairs`) from x to a member of its group and far[x] the member that
        attains it, the lowest id among equals; 0 / -1 for the only member of a group.  centre[x] is the member c of x's group that
        minimises (reach[c], c), radius[x] = reach[centre[x]] and diameter[x] the largest reach of the group, its largest pairwise
        distance: equal across a group.  A row that is not a member gets -1 / +inf.  `allow` (bool mask [len] or ids): only those rows
        are eligible; the result over them is that of an index that only ever held them.  ValueError for labels of another length, a
        label >= len (on a row of `allow`, when it is given) or a malformed allow, before the library is reached.  Re-centring a k-centre cover:
        owner = ix.spread(n)[2]; centre, radius = ix.extents(owner)[:2]."""
        words, wp = self._allow(allow)
        lab = self._extents_labels(labels, words)
        n = lab.size
        centre = np.empty(n, dtype=np.int64)
        far = np.empty(n, dtype=np.int64)
        radius = np.empty(n, dtype=np.float32)
        diameter = np.empty(n, dtype=np.float32)
        reach = np.empty(n, dtype=np.float32)
        i64 = C.POINTER(C.c_int64)
        if lib().clip_amd_index_extents(self._live(), lab.ctypes.data_as(i64), wp, centre.ctypes.data_as(i64), _fp(radius), _fp(diameter),
                                        _fp(reach), far.ctypes.data_as(i64)) < 0:
            raise RuntimeError("clip_amd_index_extents failed (see stderr)")
        return centre, radius, diameter, reach, far

    def extents_device(self, d_labels, d_centre, d_radius=None, d_diameter=None, d_reach=None, d_far=None, d_count=None, d_allow=None):
        """extents on device pointers (ints): labels [len] int64 in (trusted: a label >= len makes its row no member); centre [len] int64,
        radius / diameter / reach [len] f32, far [len] int64 and count [1] int64 (the groups with a member) out (0 / None: not wanted);
        d_allow: uint64 words on the device (0 / None: every row); asynchronous on the context's stream."""
        if not lib().clip_amd_index_extents_device(self._live(), C.c_void_p(d_labels or None), C.c_void_p(d_allow or None),
                                                   C.c_void_p(d_centre or None), C.c_void_p(d_radius or None), C.c_void_p(d_diameter or None),
                                                   C.c_void_p(d_reach or None), C.c_void_p(d_far or None), C.c_void_p(d_count or None)):
            raise RuntimeError("clip_amd_index_extents_device failed (see stderr)")

    def extents_route(self, route=0):
        """Test hook: route 0 skips the tile pairs that hold no two rows of one group, route 1 computes them all (the same result);
        returns the tile pairs the last extents call of this index computed"""
        r = int(lib().clip_amd_test_index_extents_route(self._live(), int(route)))
        if r < 0:
            raise ValueError("route must be 0 or 1")
        return r

    @staticmethod
    def _spread_args(n, radius, seeds):
        """(n, stop radius as the f32 the library compares with, seeds int64 [s]); radius None: never stop.  ValueError for a NaN and for
        n < max(1, len(seeds)), before any call."""
        n = int(n)
        stop = float("-inf") if radius is None else float(np.float32(radius))
        if stop != stop:
            raise ValueError("radius must not be NaN")
        seeds = np.ascontiguousarray([] if seeds is None else seeds, dtype=np.int64).reshape(-1)
        if n < max(1, seeds.size):
            raise ValueError("n = %d: at least 1 and at least the %d seeds" % (n, seeds.size))
        return n, stop, seeds

    def _check_seeds(self, seeds, eligible):
        """ValueError for a seed that is out of range, repeated or not eligible (eligible: bool [len])"""
        if seeds.size == 0:
            return
        if seeds.min() < 0 or seeds.max() >= len(self):
            raise ValueError("seeds must be ids of the index (0 ... %d)" % (len(self) - 1))
        if np.unique(seeds).size != seeds.size:
            raise ValueError("a seed is given twice")
        if not eligible[seeds].all():
            raise ValueError("seed %d is removed or not allowed" % int(seeds[~eligible[seeds]][0]))

    def spread(self, n, radius=None, seeds=None, allow=None):
        """Farthest-first selection: (centres int64 [m], reach f32 [m], owner int64 [len], owner_distance f32 [len], cover_radius).  The
        first centres are `seeds` in order (default: the lowest eligible id), with reach +inf; then, while fewer than n are chosen, the
        eligible row with the largest distance to its nearest centre (the distances and bits of `pairs`; the lowest id among equals)
        becomes the next centre and that distance its reach, unless it is <= radius (default: never), which ends the traversal.  m <= n
        is the number chosen.  owner[x] is the centre nearest to x, the earliest chosen among equals, owner_distance[x] the distance to
        it; a centre owns itself at 0.0; a removed or not allowed row gets -1 / +inf.  cover_radius = the largest owner_distance of an
        eligible row.  `allow` (bool mask [len] or ids): only those rows are eligible; the result over them is that of an index that
        only ever held them.  ValueError for a NaN, n < max(1, len(seeds)), a seed that is not eligible or repeated, a malformed allow."""
        n, stop, seeds = self._spread_args(n, radius, seeds)
        size = len(self)
        words, wp = self._allow(allow)
        if seeds.size:
            eligible = self.live_mask()
            if words is not None:
                eligible &= np.unpackbits(words.astype("<u8").view(np.uint8), bitorder="little")[:size].astype(np.bool_)
            self._check_seeds(seeds, eligible)
        cap = min(n, max(size, 1))
        centres = np.empty(cap, dtype=np.int64)
        reach = np.empty(cap, dtype=np.float32)
        owner = np.empty(size, dtype=np.int64)
        dist = np.empty(size, dtype=np.float32)
        cover = C.c_float(0.0)
        i64 = C.POINTER(C.c_int64)
        m = lib().clip_amd_index_spread(self._live(), cap, stop, seeds.ctypes.data_as(i64) if seeds.size else None, seeds.size, wp,
                                        centres.ctypes.data_as(i64), _fp(reach), owner.ctypes.data_as(i64), _fp(dist), C.byref(cover))
        if m < 0:
            raise RuntimeError("clip_amd_index_spread failed (see stderr)")
        return centres[:m].copy(), reach[:m].copy(), owner, dist, float(cover.value)

    def spread_device(self, n, d_centres, radius=None, seeds=None, d_reach=None, d_owner=None, d_owner_distance=None, d_cover_radius=None,
                      d_count=None, d_allow=None):
        """spread on device pointers (ints): centres [n] int64, reach [n] f32, owner [len] int64, owner_distance [len] f32, cover_radius
        [1] f32 and count [1] int64 (0 / None: not wanted, not written); seeds: host ids; d_allow: uint64 words on the device (0 /
        None: every row); asynchronous on the context's stream.  ValueError as for spread, but a seed's eligibility is the library's to
        test (RuntimeError)."""
        n, stop, seeds = self._spread_args(n, radius, seeds)
        if seeds.size and (seeds.min() < 0 or seeds.max() >= len(self) or np.unique(seeds).size != seeds.size):
            raise ValueError("seeds must be distinct ids of the index")
        if not lib().clip_amd_index_spread_device(self._live(), n, stop, seeds.ctypes.data_as(C.POINTER(C.c_int64)) if seeds.size else None,
                                                  seeds.size, C.c_void_p(d_allow or None), C.c_void_p(d_centres), C.c_void_p(d_reach or None),
                                                  C.c_void_p(d_owner or None), C.c_void_p(d_owner_distance or None),
                                                  C.c_void_p(d_cover_radius or None), C.c_void_p(d_count or None)):
            raise RuntimeError("clip_amd_index_spread_device failed (see stderr)")

    @staticmethod
    def _join(call, n_lims, guess, name):
        """(lims, distances, ids) of a range-search / pairs call: a guessed capacity first, the exact total again when it did not fit"""
        lims = np.zeros(n_lims, dtype=np.int64)
        cap = guess
        while True:
            dist = np.empty(cap, dtype=np.float32)
            ids = np.empty(cap, dtype=np.int64)
            total = call(lims.ctypes.data_as(C.POINTER(C.c_int64)), _fp(dist), ids.ctypes.data_as(C.POINTER(C.c_int64)), cap)
            if total < 0:
                raise RuntimeError("%s failed (see stderr)" % name)
            if total <= cap:
                return lims, dist[:total], ids[:total]
            cap = int(total)

    def search_ids(self, ids, k, exclude_self=True, allow=None):
        """Neighbours of the stored rows `ids` (each a live id; duplicates are fine): (distances f32 [n_ids, k], ids int64 [n_ids, k]) as
        `search` gives them for the vectors that were added as those rows; exclude_self: a row is not its own neighbour.  `allow` (bool mask
        [len] or ids) restricts the candidates only."""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        words, wp = self._allow(allow)
        dist = np.empty((a.size, k), dtype=np.float32)
        out = np.empty((a.size, k), dtype=np.int64)
        if not lib().clip_amd_index_search_ids(self._live(), a.ctypes.data_as(C.POINTER(C.c_int64)), a.size, int(k), int(bool(exclude_self)), wp,
                                               _fp(dist), out.ctypes.data_as(C.POINTER(C.c_int64))):
            raise RuntimeError("clip_amd_index_search_ids failed (see stderr)")
        return dist, out

    def search_ids_device(self, d_ids, n_ids, k, d_distances, d_out_ids, exclude_self=True, d_allow=None):
        """search_ids on device pointers (ints): ids [n] int64 -> distances [n, k] f32, ids [n, k] int64; asynchronous on the context's
        stream.  An id out of range or removed gives an all-empty row (-1 / +inf); d_allow: uint64 words on the device (0 / None: every row)."""
        if not lib().clip_amd_index_search_ids_device(self._live(), C.c_void_p(d_ids), int(n_ids), int(k), int(bool(exclude_self)),
                                                      C.c_void_p(d_allow or None), C.c_void_p(d_distances), C.c_void_p(d_out_ids)):
            raise RuntimeError("clip_amd_index_search_ids_device failed (see stderr)")

    def knn_graph(self, k):
        """(distances f32 [n, k], ids int64 [n, k]): for every id its k nearest other live rows, nearest first, equal distances lower id
        first, -1 / +inf where there are fewer (and in the whole row of a removed id); row i equals search_ids([i], k) bit for bit."""
        n = len(self)
        dist = np.empty((n, k), dtype=np.float32)
        ids = np.empty((n, k), dtype=np.int64)
        if not lib().clip_amd_index_knn_graph(self._live(), int(k), _fp(dist), ids.ctypes.data_as(C.POINTER(C.c_int64))):
            raise RuntimeError("clip_amd_index_knn_graph failed (see stderr)")
        return dist, ids

    def _labels(self, labels):
        """(keep-alive int32 array, pointer) of one label per row for the votes: >= 0 a class, -1 unlabelled (ValueError for None, a wrong
        length, a non-integer or a label outside -1 ... 2^31 - 1).  Pure numpy: needs no device."""
        if labels is None:
            raise ValueError("labels must be integers, not None")
        a = np.asarray(labels)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("labels must be integers, not %s" % a.dtype)
        a = a.reshape(-1)
        if a.size != len(self):
            raise ValueError("labels must have one entry per row: %d, not %d" % (len(self), a.size))
        if a.size and (int(a.min()) < -1 or int(a.max()) > 2 ** 31 - 1):
            raise ValueError("labels must lie in -1 ... 2^31 - 1 (-1: unlabelled), not %d ... %d" % (int(a.min()), int(a.max())))
        a = np.zeros(a.size + 1, dtype=np.int32)[:a.size] if a.size == 0 else np.ascontiguousarray(a, dtype=np.int32)
        return a, a.ctypes.data_as(C.POINTER(C.c_int32))

    @staticmethod
    def _vote_km(k, m):
        """(k, m) as ints after the check 1 <= m <= k <= 1024 (ValueError)"""
        k, m = int(k), int(m)
        if not 1 <= m <= k <= 1024:
            raise ValueError("a vote needs 1 <= m <= k <= 1024, not m = %d, k = %d" % (m, k))
        return k, m

    @staticmethod
    def _vote_outputs(n, m):
        out = (np.empty((n, m), dtype=np.int32), np.empty((n, m), dtype=np.int32), np.empty((n, m), dtype=np.float32),
               np.empty((n, m), dtype=np.int64))
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        return out, (out[0].ctypes.data_as(i32p), out[1].ctypes.data_as(i32p), _fp(out[2]), out[3].ctypes.data_as(i64p))

    def vote(self, queries, k, labels, m=1, allow=None):
        """k-NN vote over labelled rows: `labels` (int [len]) is every row's class (>= 0, any numbering) or -1 for an unlabelled row; the
        voters are the live, allowed, labelled rows.  Per query, L = its k nearest voters in search's order (search(..., allow=voters));
        the classes of L by votes (entries in L) descending, then by the rank of the class's nearest entry, cut to m.  Returns (classes
        int32 [nq, m], votes int32 [nq, m], distances f32 [nq, m], ids int64 [nq, m]): per class its number, its votes, and the distance
        (search's bits) and row of its nearest voter; -1 / 0 / +inf / -1 where L holds fewer classes.  k = 1: nearest-neighbour
        classification.  ValueError unless 1 <= m <= k <= 1024 and the labels are right."""
        k, m = self._vote_km(k, m)
        lab, lp = self._labels(labels)
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        words, wp = self._allow(allow)
        out, ptrs = self._vote_outputs(q.shape[0], m)
        if not lib().clip_amd_index_vote(self._live(), _fp(q), q.shape[0], k, m, lp, wp, *ptrs):
            raise RuntimeError("clip_amd_index_vote failed (see stderr)")
        return out

    def vote_ids(self, ids, k, labels, m=1, exclude_self=True, allow=None):
        """vote with the stored rows `ids` (each a live id) as the queries, bit for bit as search_ids takes them; exclude_self: a row does
        not vote for itself.  The query rows need not be labelled or allowed."""
        k, m = self._vote_km(k, m)
        lab, lp = self._labels(labels)
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        words, wp = self._allow(allow)
        out, ptrs = self._vote_outputs(a.size, m)
        if not lib().clip_amd_index_vote_ids(self._live(), a.ctypes.data_as(C.POINTER(C.c_int64)), a.size, k, m, int(bool(exclude_self)), lp, wp, *ptrs):
            raise RuntimeError("clip_amd_index_vote_ids failed (see stderr)")
        return out

    def vote_graph(self, k, labels, m=1, allow=None):
        """vote for every row at once, each row excluded from its own vote (leave-one-out): [len, m] arrays as vote's; row i equals
        vote_ids([i], ...) bit for bit for a live row, and is empty for a removed one.  On the routes of knn_graph."""
        k, m = self._vote_km(k, m)
        lab, lp = self._labels(labels)
        words, wp = self._allow(allow)
        out, ptrs = self._vote_outputs(len(self), m)
        if not lib().clip_amd_index_vote_graph(self._live(), k, m, lp, wp, *ptrs):
            raise RuntimeError("clip_amd_index_vote_graph failed (see stderr)")
        return out

    def vote_device(self, d_queries, n_queries, k, d_labels, d_classes, d_votes, d_distances, d_ids, m=1, d_allow=None):
        """vote on device pointers (ints): queries [n, dim] f32, labels [len] int32 (trusted: any negative value is unlabelled), d_allow
        uint64 words (0 / None: every row) -> classes / votes int32, distances f32, ids int64, [n, m] each; asynchronous on the context's
        stream."""
        k, m = self._vote_km(k, m)
        if not lib().clip_amd_index_vote_device(self._live(), C.c_void_p(d_queries), int(n_queries), k, m, C.c_void_p(d_labels or None),
                                                C.c_void_p(d_allow or None), C.c_void_p(d_classes), C.c_void_p(d_votes), C.c_void_p(d_distances),
                                                C.c_void_p(d_ids)):
            raise RuntimeError("clip_amd_index_vote_device failed (see stderr)")

    def vote_graph_device(self, k, d_labels, d_classes, d_votes, d_distances, d_ids, m=1, d_allow=None):
        """vote_graph on device pointers (ints), outputs [len, m] each: no result visits the host"""
        k, m = self._vote_km(k, m)
        if not lib().clip_amd_index_vote_graph_device(self._live(), k, m, C.c_void_p(d_labels or None), C.c_void_p(d_allow or None),
                                                      C.c_void_p(d_classes), C.c_void_p(d_votes), C.c_void_p(d_distances), C.c_void_p(d_ids)):
            raise RuntimeError("clip_amd_index_vote_graph_device failed (see stderr)")

    def vote_block(self, rows=0):
        """test hook: query rows per block of the votes from now on (0: automatic); returns the value set"""
        r = int(lib().clip_amd_test_index_vote_block(self._live(), int(rows)))
        if r < 0:
            raise ValueError("vote_block: rows must lie in 0 ... 65408, not %d" % int(rows))
        return r

    def search_index(self, src, k, ids=None, allow=None):
        """This index searched with the stored rows of `src` (an Index of the same Clip, dim and dtype without removed rows): every row in
        id order, or the rows `ids` (duplicates and any order are fine).  (distances f32 [n, k], ids int64 [n, k]) as `search` gives them
        for the vectors that were added to `src` as those rows; `allow` (bool mask [len(self)] or ids) restricts the candidates.
        `src is self` equals search_ids(..., exclude_self=False)."""
        a, ap = None, None
        n = len(src)
        if ids is not None:
            a = np.zeros(np.size(ids) + 1, dtype=np.int64)[:np.size(ids)]      # (no ids is still an array, not the NULL of "every row")
            a[:] = np.asarray(ids, dtype=np.int64).reshape(-1)
            ap, n = a.ctypes.data_as(C.POINTER(C.c_int64)), a.size
        words, wp = self._allow(allow)
        dist = np.empty((n, k), dtype=np.float32)
        out = np.empty((n, k), dtype=np.int64)
        if not lib().clip_amd_index_search_index(self._live(), src._live(), ap, n, int(k), wp, _fp(dist), out.ctypes.data_as(C.POINTER(C.c_int64))):
            raise RuntimeError("clip_amd_index_search_index failed (see stderr)")
        return dist, out

    def append(self, src):
        """Append every row of `src` (same Clip, dim and dtype, no removed rows, not this index) bit for bit; `src` is unchanged.  Returns
        new_ids int64 [len(src)]: each src id's id in this index."""
        new_ids = np.empty(len(src), dtype=np.int64)
        if lib().clip_amd_index_append(self._live(), src._live(), new_ids.ctypes.data_as(C.POINTER(C.c_int64))) < 0:
            raise RuntimeError("clip_amd_index_append failed (see stderr)")
        return new_ids

    def search_device(self, d_queries, n_queries, k, d_distances, d_ids):
        """Device pointers (ints): queries [n, dim] f32 -> distances [n, k] f32, ids [n, k] int64; asynchronous on the context's stream."""
        if not lib().clip_amd_index_search_device(self._live(), C.c_void_p(d_queries), int(n_queries), int(k), C.c_void_p(d_distances),
                                                  C.c_void_p(d_ids)):
            raise RuntimeError("clip_amd_index_search_device failed (see stderr)")

    def search_subset_device(self, d_queries, n_queries, k, d_allow, d_distances, d_ids):
        """search_device over the rows allowed by the uint64 words at device address d_allow (0 / None: every row)"""
        if not lib().clip_amd_index_search_subset_device(self._live(), C.c_void_p(d_queries), int(n_queries), int(k), C.c_void_p(d_allow or None),
                                                         C.c_void_p(d_distances), C.c_void_p(d_ids)):
            raise RuntimeError("clip_amd_index_search_subset_device failed (see stderr)")

    def save(self, path):
        if not lib().clip_amd_index_save(self._live(), os.fsencode(path)):
            raise RuntimeError("clip_amd_index_save failed for %r (see stderr)" % (path,))

    def close(self):
        if getattr(self, "handle", None):
            lib().clip_amd_index_free(self.handle)
            self.handle = None

    def _live(self):
        if not getattr(self, "handle", None):
            raise RuntimeError("the index is closed")
        return self.handle

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bench_search(dtype, n, dim, n_queries, k, iters=10):
    """Microseconds per clip_amd_index_search_device on seeded random data (clip_amd_bench_search); < 0 on error."""
    return float(lib().clip_amd_bench_search(Index.DTYPES[dtype], int(n), int(dim), int(n_queries), int(k), int(iters)))


def bench_search_grouped(dtype, n, dim, n_queries, k, group_size, iters=10):
    """Microseconds per clip_amd_index_search_grouped_device on the data of bench_search, row r in group r // group_size
    (clip_amd_bench_search_grouped); < 0 on error."""
    return float(lib().clip_amd_bench_search_grouped(Index.DTYPES[dtype], int(n), int(dim), int(n_queries), int(k), int(group_size), int(iters)))


def bench_search_sets(dtype, n, dim, n_sets, set_size, k, group_size, iters=10):
    """Microseconds per clip_amd_index_search_sets_device of n_sets sets of set_size query rows on the data of bench_search, row r in group
    r // group_size, 0: no groups (clip_amd_bench_search_sets); < 0 on error."""
    return float(lib().clip_amd_bench_search_sets(Index.DTYPES[dtype], int(n), int(dim), int(n_sets), int(set_size), int(k), int(group_size),
                                                  int(iters)))


def bench_search_distinct(dtype, n, dim, n_queries, k, pool, radius, copies=4, iters=10):
    """Microseconds per clip_amd_index_search_distinct_device over n seeded rows in groups of a random row and `copies` noisy copies of it
    (clip_amd_bench_search_distinct); < 0 on error."""
    return float(lib().clip_amd_bench_search_distinct(Index.DTYPES[dtype], int(n), int(dim), int(n_queries), int(k), int(pool), float(radius),
                                                      int(copies), int(iters)))


def bench_search_compound(dtype, n, dim, n_queries, n_terms, k, iters=10):
    """Microseconds per clip_amd_index_search_compound_device of n_queries compound queries of n_terms "all" terms each on the data of
    bench_search (clip_amd_bench_search_compound); < 0 on error."""
    return float(lib().clip_amd_bench_search_compound(Index.DTYPES[dtype], int(n), int(dim), int(n_queries), int(n_terms), int(k), int(iters)))


def bench_search_subset(dtype, n, dim, n_queries, k, allowed_fraction, contiguous, iters=10):
    """Microseconds per clip_amd_index_search_subset_device on the data of bench_search with a seeded allowed set: a random selection of
    `allowed_fraction` of the ids or, `contiguous`, one id range of that size (clip_amd_bench_search_subset); < 0 on error."""
    return float(lib().clip_amd_bench_search_subset(Index.DTYPES[dtype], int(n), int(dim), int(n_queries), int(k), float(allowed_fraction),
                                                    int(bool(contiguous)), int(iters)))


def bench_range(dtype, n, dim, n_queries, radius, iters=10):
    """Microseconds per clip_amd_index_range_search of n_queries queries, or per clip_amd_index_pairs when n_queries == 0, on seeded random
    rows with planted near-duplicates (clip_amd_bench_range); < 0 on error."""
    return float(lib().clip_amd_bench_range(Index.DTYPES[dtype], int(n), int(dim), int(n_queries), float(radius), int(iters)))


def cut_linkage(size, lo, hi, d, radius=None, n_groups=None, eligible=None):
    """Labels from the edges of Index.linkage, with the conventions of Index.components: labels int64 [size], the lowest id of the row's
    group, the row itself for a singleton, -1 for a row outside `eligible` (bool [size]; None: every row).  radius: the edges with
    d <= radius (compared in f32) are kept, which gives exactly the labels of components(radius) when the edges reach that far (link >=
    radius).  n_groups: the longest edges in the order (d, lo, hi) are dropped until exactly n_groups groups are left, singletons
    included.  Neither: every edge is kept.  Host code, a union-find.  ValueError for both at once, a NaN radius, an edge that touches a
    row outside `eligible`, or an n_groups that the edges cannot give (more than the eligible rows, fewer than the trees of the forest)."""
    size = int(size)
    lo = np.ascontiguousarray(lo, dtype=np.int64).reshape(-1)
    hi = np.ascontiguousarray(hi, dtype=np.int64).reshape(-1)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1)
    if not (lo.size == hi.size == d.size):
        raise ValueError("lo, hi and d must have one length")
    if radius is not None and n_groups is not None:
        raise ValueError("radius and n_groups exclude each other")
    if eligible is None:
        eligible = np.ones(size, dtype=np.bool_)
    else:
        eligible = np.ascontiguousarray(eligible, dtype=np.bool_).reshape(-1)
        if eligible.size != size:
            raise ValueError("eligible must have one entry per row")
    if lo.size and (lo.min() < 0 or hi.max() >= size or (lo >= hi).any() or not (eligible[lo].all() and eligible[hi].all())):
        raise ValueError("edges must join two eligible rows lo < hi of the index")
    order = np.lexsort((hi, lo, d))
    if radius is not None:
        r = np.float32(radius)
        if r != r:
            raise ValueError("radius must not be NaN")
        order = order[d[order] <= r]
    if n_groups is not None:
        m = int(eligible.sum())
        keep = m - int(n_groups)
        if int(n_groups) < 1 or keep < 0 or keep > order.size:
            raise ValueError("n_groups = %d with %d eligible rows in %d trees" % (int(n_groups), m, m - order.size))
        order = order[:keep]
    parent = list(range(size))
    for a, b in zip(lo[order].tolist(), hi[order].tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    labels = np.asarray(parent, dtype=np.int64)
    for _ in range(64):                                    # a root is the lowest id of its group: pointer jumping ends at it
        up = labels[labels]
        if (up == labels).all():
            break
        labels = up
    labels[~eligible] = -1
    return labels


def cut_linkage_sized(size, lo, hi, d, n_groups, min_size=2, eligible=None):
    """(labels, radius): the cut of a tree of Index.linkage or Index.linkage_core at the largest of its distances at which it has exactly
    n_groups groups of at least min_size rows; labels as cut_linkage(..., radius=radius) gives them (smaller groups and single rows keep
    their own labels: with a tree of linkage_core those are the rows left unfiled).  One union-find sweep over the sorted edges, the
    count read at the end of every run of equal distances.  ValueError, naming the counts that do occur, when no distance gives exactly
    n_groups; for the rest as cut_linkage."""
    size, n_groups, min_size = int(size), int(n_groups), max(int(min_size), 1)
    labels = cut_linkage(size, lo, hi, d, eligible=eligible)      # (the checks of the edges)
    lo = np.ascontiguousarray(lo, dtype=np.int64).reshape(-1)
    hi = np.ascontiguousarray(hi, dtype=np.int64).reshape(-1)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1)
    order = np.lexsort((hi, lo, d))
    los, his, ds = lo[order].tolist(), hi[order].tolist(), d[order]
    parent, size_of = list(range(size)), [1] * size
    big = int(np.count_nonzero(labels >= 0)) if min_size == 1 else 0
    seen, best = set(), None
    for t in range(len(los)):
        a, b = los[t], his[t]
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            if a > b:
                a, b = b, a
            big += (size_of[a] + size_of[b] >= min_size) - (size_of[a] >= min_size) - (size_of[b] >= min_size)
            parent[b] = a
            size_of[a] += size_of[b]
        if t + 1 == len(los) or ds[t + 1] != ds[t]:
            seen.add(big)
            if big == n_groups:
                best = ds[t]
    if best is None:
        raise ValueError("no distance of the tree gives %d groups of at least %d rows; the counts that occur: %s"
                         % (n_groups, min_size, ", ".join(str(c) for c in sorted(seen)) or "none"))
    return cut_linkage(size, lo, hi, d, radius=best, eligible=eligible), float(best)


def bench_components(dtype, n, dim, radius, iters=3):
    """Microseconds per clip_amd_index_components (host form) over the seeded rows of bench_range (clip_amd_bench_components); < 0 on error."""
    return float(lib().clip_amd_bench_components(Index.DTYPES[dtype], int(n), int(dim), float(radius), int(iters)))


def bench_modes(dtype, n, dim, radius, link=None, copies=0, iters=3):
    """Microseconds per clip_amd_index_modes (host form); copies 0: the seeded rows of bench_range, copies > 0: groups of a row and that
    many noisy copies (clip_amd_bench_modes); < 0 on error."""
    return float(lib().clip_amd_bench_modes(Index.DTYPES[dtype], int(n), int(dim), float(radius), float(radius if link is None else link), int(copies),
                                            int(iters)))


def bench_extents(dtype, n, dim, group_size, sorted=True, iters=3):
    """Microseconds per clip_amd_index_extents (host form) over bursts of group_size rows labelled by burst, the labels following the row
    order (sorted) or scattered over the index (clip_amd_bench_extents); < 0 on error."""
    return float(lib().clip_amd_bench_extents(Index.DTYPES[dtype], int(n), int(dim), int(group_size), int(bool(sorted)), int(iters)))


def bench_linkage(dtype, n, dim, copies=0, iters=3):
    """(microseconds per clip_amd_index_linkage, host form, the whole tree; rounds that did work) over the data of bench_modes
    (clip_amd_bench_linkage); a time < 0 on error."""
    us = float(lib().clip_amd_bench_linkage(Index.DTYPES[dtype], int(n), int(dim), int(copies), int(iters)))
    return us, int(lib().clip_amd_bench_linkage_rounds())


def bench_linkage_core(dtype, n, dim, k, copies=0, iters=3):
    """Microseconds per call, all on one index in one run, interleaved (clip_amd_bench_linkage_core): a dict with linkage_core (host form,
    the whole tree), knn_graph (k), linkage, core_column (the neighbour search with its device-side sink alone), rounds and
    linkage_rounds (the rounds that did work in either tree); linkage_core < 0 on error."""
    us = float(lib().clip_amd_bench_linkage_core(Index.DTYPES[dtype], int(n), int(dim), int(k), int(copies), int(iters)))
    parts = np.zeros(5, dtype=np.float32)
    lib().clip_amd_bench_linkage_core_parts(_fp(parts))
    return dict(linkage_core=us, knn_graph=float(parts[0]), linkage=float(parts[1]), core_column=float(parts[2]), rounds=int(parts[3]),
                linkage_rounds=int(parts[4]))


def bench_spread(dtype, n, dim, n_max, copies=0, iters=3):
    """Microseconds of device time per clip_amd_index_spread_device of n_max centres, no seeds, no stop radius; the data of bench_modes
    (clip_amd_bench_spread); < 0 on error."""
    return float(lib().clip_amd_bench_spread(Index.DTYPES[dtype], int(n), int(dim), int(n_max), int(copies), int(iters)))


def bench_vote_graph(dtype, n, dim, k, m=1, classes=64, route=0, iters=3):
    """Microseconds (wall) per clip_amd_index_vote_graph over the n seeded random rows of bench_knn, a row's label a seeded hash of its
    number modulo `classes`; route as bench_knn (clip_amd_bench_vote_graph); < 0 on error."""
    return float(lib().clip_amd_bench_vote_graph(Index.DTYPES[dtype], int(n), int(dim), int(k), int(m), int(classes), int(route), int(iters)))


def bench_knn(dtype, n, dim, k, route=0, iters=3):
    """Microseconds (wall) per clip_amd_index_knn_graph over n seeded random rows; route 0 automatic, 1 the scan route, 2 the tiled kernel
    (clip_amd_bench_knn); < 0 on error."""
    return float(lib().clip_amd_bench_knn(Index.DTYPES[dtype], int(n), int(dim), int(k), int(route), int(iters)))


def bench_cross(dtype, n_rows, n_queries, dim, k, route=0, iters=3):
    """Microseconds (wall) per clip_amd_index_search_index of an index of n_rows seeded random rows with every one of the n_queries rows of a
    second one; route 0 automatic, 1 the scan route, 2 the tiled kernel (clip_amd_bench_cross); < 0 on error."""
    return float(lib().clip_amd_bench_cross(Index.DTYPES[dtype], int(n_rows), int(n_queries), int(dim), int(k), int(route), int(iters)))


def gguf_inspect(path):
    """(kv dict, [(tensor name, dims, ggml type)]) of a GGUF file (metadata only; see convert_hf_to_gguf.py)."""
    from .convert_hf_to_gguf import gguf_inspect as _gi
    return _gi(path)


def quantize(fname_inp, fname_out, itype):
    return bool(lib().clip_model_quantize(os.fsencode(fname_inp), os.fsencode(fname_out), int(itype)))


def shard_bounds(total, n_devices, device_index):
    """(lo, hi, rows_per_device) of the multi-GPU clip_image_batch_encode (clip_amd_shard_bounds; pure arithmetic)."""
    lo, hi, per = C.c_int(), C.c_int(), C.c_int()
    lib().clip_amd_shard_bounds(total, n_devices, device_index, C.byref(lo), C.byref(hi), C.byref(per))
    return lo.value, hi.value, per.value
