/* clip_amd.h — MI355X-specific extensions of the clip.h C ABI.
 *
 * Everything here is ADDITIVE to the reference API (include/clip.h).  Plain C
 * ABI: pointers + sizes only, no torch / HIP types in signatures (a HIP stream
 * is passed as void*).  Device pointers are raw HBM addresses on the ctx's
 * device (e.g. torch.Tensor.data_ptr()).
 */
#ifndef CLIP_AMD_H
#define CLIP_AMD_H

#include "clip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Number of visible HIP devices (0 when there is no GPU / driver). */
int clip_amd_device_count(void);

/* Like clip_model_load (reference clip.cpp:334) but on an explicit device ordinal.
 * clip_model_load uses $CLIP_AMD_DEVICE, else $LOCAL_RANK, else device 0. */
struct clip_ctx * clip_amd_model_load(const char * fname, int verbosity, int device);

/* Multi-GPU form of clip_model_load (the reference has no multi-device path): ONE process, the weights
 * replicated on the first n_devices HIP devices (n_devices <= 0: all visible), one context + stream + host thread per
 * device behind the returned handle.  clip_image_batch_encode (reference clip.cpp:1247) on such a handle shards a batch
 * of B >= 2 * n_devices images into contiguous runs of ceil(B / n_devices), copies to each device only its shard,
 * runs the identical kernels, and collects the final embeddings with ONE ncclAllGather (RCCL over xGMI) of
 * [ceil(B / n_devices)][projection_dim] f32 rows per device into [n_devices * ceil(B / n_devices)][projection_dim] on
 * every device, then one device-to-host copy from device 0 into `vec`.  Everything else (text encode, small batches)
 * runs on device 0.  RCCL (librccl.so) is bound with dlopen by this call only.  NULL on failure.  clip_free() releases
 * every replica. */
struct clip_ctx * clip_amd_model_load_multi(const char * fname, int verbosity, int n_devices);
/* Number of devices behind a handle (1 for clip_model_load / clip_amd_model_load handles). */
int clip_amd_ctx_device_count(const struct clip_ctx * ctx);

/* Repacked-weight cache (replaces the per-load tensor read + repack of reference clip.cpp:435-461).  Opt-in through the
 * environment: CLIP_AMD_WEIGHT_CACHE=<directory>.  clip_model_load then keeps "<directory>/<file name>.<content key>.hbm" — the exact
 * HBM image of the model — and later loads of the same file content read that image instead of repacking the GGUF tensors.
 * Returns 1 when this context's weights came from the cache, 0 when they were repacked from the GGUF. */
int clip_amd_weights_from_cache(const struct clip_ctx * ctx);
/* The shard clip_image_batch_encode gives device `device_index` of `n_devices` for a batch of `total` images: rows
 * [*lo, *hi), and the padded per-device row count of the all-gather (pure arithmetic, no device needed). */
void clip_amd_shard_bounds(int total, int n_devices, int device_index, int * lo, int * hi, int * rows_per_device);
/* Device address (on device `device_index`) of the gathered [n_devices * rows_per_device][projection_dim] embeddings of
 * the last sharded clip_image_batch_encode: the canonical device-resident result (valid until the next call). */
const float * clip_amd_gathered_embeddings(const struct clip_ctx * ctx, int device_index);

/* Device-resident sharded encodes on a clip_amd_model_load_multi handle (the form bench.py --single-process measures): shard g of the
 * batch — items [lo, hi) of clip_amd_shard_bounds(total, n_devices, g) — already sits ON device g: d_imgs[g] = [hi - lo][S][S][3] f32
 * preprocessed images; d_ids[g] = the token ids of the shard's texts back to back, h_offsets = total + 1 prefix offsets of ALL texts
 * (host).  Each replica runs its tower on its own stream and host thread, then ONE grouped ncclAllGather leaves [n_devices *
 * rows_per_device][projection_dim] on every device (clip_amd_gathered_embeddings); vec (host, [total][projection_dim]) may be NULL.
 * Synchronous: returns when every replica stream has finished.  clip_amd_image_batch_encode_u8 and clip_text_batch_encode shard the
 * same way on such a handle when total >= 2 * n_devices. */
bool clip_amd_image_batch_encode_device_multi(struct clip_ctx * ctx, const float * const * d_imgs, int total, bool normalize, float * vec);
bool clip_amd_text_batch_encode_device_multi(struct clip_ctx * ctx, const int32_t * const * d_ids, const int32_t * h_offsets, int total, bool normalize,
                                             float * vec);
/* Both towers of a step in ONE call: on every device the vision tower (reference clip.cpp:1247) runs on the replica's stream and the text
 * tower (clip.cpp:1016) on the stream of a sibling context of that device (created on the first such call: own activation workspace,
 * the replica's weight image), forked and joined with events, then ONE grouped ncclAllGather of [rows_per_device(n_images) + rows_per_device(n_texts)]
 * rows per device; clip_amd_gathered_embeddings then holds n_devices such blocks (image rows first).  Shards as above; vec_img
 * [n_images][projection_dim] and vec_txt [n_texts][projection_dim] (host) may each be NULL.  Synchronous. */
bool clip_amd_encode_pair_device_multi(struct clip_ctx * ctx, const float * const * d_imgs, int n_images, const int32_t * const * d_ids,
                                       const int32_t * h_offsets, int n_texts, bool normalize, float * vec_img, float * vec_txt);

/* Which device a ctx lives on (-1: host-only ctx, see CLIP_AMD_ALLOW_NO_DEVICE in DESIGN.md). */
int clip_amd_ctx_device(const struct clip_ctx * ctx);

/* Bind all subsequent launches of this ctx to an existing HIP stream (e.g. torch's current
 * stream, as an integer handle).  NULL restores the ctx's own stream.  A context is single-stream and
 * single-thread at any one time (it owns one activation workspace): the switch orders the new stream behind
 * everything still queued on the previous one — by recording an event on the PREVIOUS stream, so that stream must still
 * exist when clip_amd_set_stream (and clip_free, which synchronises the stream in use) is called: switch the context back
 * (or free it) BEFORE destroying a stream it was bound to. */
void clip_amd_set_stream(struct clip_ctx * ctx, void * hip_stream);

/* Tell the context that its device carries other work at the same time (shared != 0) — typically the other tower of a two-tower step
 * on a second context / stream.  The GEMM heuristic then keeps to kernels that share a compute unit (two workgroups per CU); with
 * shared == 0 (the default: one encoder call at a time, as every reference caller does) the wide q/k/v and FFN-up GEMMs of a large batch
 * run on kernels that take a whole CU each (k_gemm32.hip).  Results agree within fp16 output rounding either way.  The two-tower
 * multi-GPU entry point (clip_amd_encode_pair_device_multi) knows by itself.
 *
 * WHAT THE BITS OF AN ENCODE DEPEND ON.  The embeddings a call returns are a function of
 *   - the model file,
 *   - the inputs of the call and how they are batched (which items share a call, in which order: kernels are chosen by row count),
 *   - `normalize`,
 *   - this flag and the sibling state AT THE CALL (the other tower of a pair call running next to it),
 *   - the environment switches the library read when the context was loaded (CLIP_AMD_*),
 * and of nothing else (a call made while clip_amd_profile_enable is on is a different call in this sense: it runs unsplit and uncaptured).  The calls a context has served before — other batch sizes, the other tower, captured and replayed graphs, resident
 * panels built for a larger batch, a workspace that has grown, profiling switched on and off, this flag set and set back — are NOT on the
 * list: a context with a history returns bit for bit what a freshly loaded one returns for the same call (tests/test_gpu_call_history.py). */
void clip_amd_set_device_shared(struct clip_ctx * ctx, int shared);

/* Device-resident form of clip_image_batch_encode (reference clip.cpp:1247-1523):
 * d_imgs  : B x [S,S,3] float32 interleaved RGB, already preprocessed, in HBM
 * d_out   : B x projection_dim float32 in HBM
 * Asynchronous on the ctx stream; no host<->device copies. */
bool clip_amd_image_batch_encode_device(struct clip_ctx * ctx, const float * d_imgs, int batch, float * d_out,
                                        bool normalize);

/* GPU image preprocessing ("next" row §8f-1; reference clip_image_preprocess / clip_image_batch_preprocess,
 * clip.cpp:728-1008): n raw RGB u8 images of any size (HOST pointers, clip_image_u8 as filled by
 * clip_image_load_from_file) -> d_out [n][S][S][3] float32 in HBM, resized (antialiased bicubic, shorter side -> S),
 * centre-cropped and normalised exactly like clip_image_preprocess (bit-identical).  Asynchronous on the ctx stream. */
bool clip_amd_image_batch_preprocess_device(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n, float * d_out);

/* clip_image_batch_preprocess + clip_image_batch_encode in one call with the preprocessing on the GPU.
 * vec: [n][projection_dim] on the host.  Same results as the two-step host path. */
bool clip_amd_image_batch_encode_u8(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n, float * vec, bool normalize);

/* Encoded images in, embeddings out.  The files are read and decoded on n_threads host threads (every format clip_image_load_from_file
 * reads).  Only the entropy decoding of a JPEG stays on those threads: its IDCT, chroma up-sampling and colour conversion run on the GPU,
 * where that provably gives the host decoder's pixels.  CLIP_AMD_JPEG_DEVICE=0 keeps them on the host threads as well (same rows); the
 * comparison that made the device the default: profiles/files_bench.txt.  The rows are bit-identical to
 * clip_image_load_from_file + ONE clip_amd_image_batch_encode_u8 call over the loadable images.
 *
 * Encode the first max_images loadable files of paths[0..n): returns the number of rows written to vec ([rows][proj], in path order),
 * -1 on a device or argument error. *consumed = paths looked at; ok[i] (i < *consumed) = 1 when path i produced a row.  When some of the
 * first max_images paths do not load, as many further paths as are missing are looked at, until max_images have loaded or the list ends:
 * walking a long list with paths + consumed gives max_images consecutive loadable images per call.  vec holds max_images rows, ok n
 * entries; host memory grows with max_images (every decoded image of a call is held until it is encoded).  Not for
 * clip_amd_model_load_multi contexts. */
int clip_amd_image_batch_encode_files(struct clip_ctx * ctx, const char * const * paths, int n, int max_images, int n_threads,
                                      bool normalize, float * vec, int * consumed, uint8_t * ok);
/* the same for encoded images held in memory (uploads, archives): data[i], sizes[i] */
int clip_amd_image_batch_encode_memory(struct clip_ctx * ctx, const uint8_t * const * data, const size_t * sizes, int n, int max_images,
                                       int n_threads, bool normalize, float * vec, int * consumed, uint8_t * ok);

/* Regions: several boxes of uploaded images, one row each (crops per image for a region index; see clip_amd_index_search_grouped).
 * boxes: [n_boxes][5] = image number (0 ... n_imgs - 1), x, y, w, h with w, h >= 1 and the box inside its image; any order, an image may
 * be named any number of times or not at all.  Row b is, bit for bit, row b of ONE clip_amd_image_batch_encode_u8 call over the n_boxes
 * images obtained by copying each box out on the host: the resize treats the box as the whole picture, nothing outside it is read.  An
 * image's pixels are uploaded once per staging piece (at most 128 rows, CLIP_AMD_U8_PIECE) that holds one of its boxes, not once per
 * box.  A bad box (or NULL boxes with n_boxes > 0) returns false before anything is launched, with a message that names the box, and
 * leaves vec untouched.  Not for clip_amd_model_load_multi contexts. */
bool clip_amd_image_batch_encode_regions(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n_imgs, const int32_t * boxes, int n_boxes,
                                         float * vec, bool normalize);
/* the preprocessing half alone, as clip_amd_image_batch_preprocess_device: d_out [n_boxes][S][S][3] float32 in HBM (one staging piece) */
bool clip_amd_image_batch_preprocess_regions_device(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n_imgs, const int32_t * boxes,
                                                    int n_boxes, float * d_out);
/* clip_amd_image_batch_encode_files / _memory with a grid of regions per image, 1 <= grid <= 8.  grid == 1: the same rows as the call
 * without a grid.  grid = G >= 2: every loadable image yields R = 1 + G * G consecutive rows: the whole image, then the tiles row by row,
 * tile (i, j) = x in [i nx / G, (i + 1) nx / G), y in [j ny / G, (j + 1) ny / G) in integer division, j outer and i inner.  max_images,
 * the return value, *consumed and ok keep counting IMAGES; vec holds max_images * R rows and boxes_out [max_images * R][4] receives each
 * row's x, y, w, h.  An image with min(nx, ny) < G counts as not loadable (ok 0, a message on stderr).  The rows are bit-identical to
 * clip_image_load_from_file for each loadable file followed by ONE clip_amd_image_batch_encode_regions call over those boxes.  A JPEG
 * whose pixel half runs on the device is decoded there once per staging piece; all its regions read those pixels, which never exist on
 * the host. */
int clip_amd_image_batch_encode_files_grid(struct clip_ctx * ctx, const char * const * paths, int n, int max_images, int n_threads, int grid,
                                           bool normalize, float * vec, int32_t * boxes_out, int * consumed, uint8_t * ok);
int clip_amd_image_batch_encode_memory_grid(struct clip_ctx * ctx, const uint8_t * const * data, const size_t * sizes, int n, int max_images,
                                            int n_threads, int grid, bool normalize, float * vec, int32_t * boxes_out, int * consumed, uint8_t * ok);

/* Batched text encoding ("next" row §8f-2; per-text semantics identical to
 * clip_text_encode, reference clip.cpp:1016-1233).  Texts are ragged:
 * tokens[i].data holds tokens[i].size ids incl. BOS/EOS.  vec: [n_texts][projection_dim]. */
bool clip_text_batch_encode(const struct clip_ctx * ctx, const int n_threads, const struct clip_tokens * tokens,
                            size_t n_texts, float * vec, const bool normalize);

/* Device-resident batched text encode: d_ids = concatenated ids (int32, HBM),
 * h_offsets = n_texts+1 prefix offsets (HOST memory), d_out [n_texts][proj] in HBM. */
bool clip_amd_text_batch_encode_device(struct clip_ctx * ctx, const int32_t * d_ids, const int32_t * h_offsets,
                                       int n_texts, float * d_out, bool normalize);

/* GPU-side zero-shot scoring ("next" row §8f-2; reference clip_similarity_score + softmax_with_sorting as composed by
 * clip_zero_shot_label_image, clip.cpp:1624-1659, and tests/benchmark.cpp:114-160).  For each of n_images embeddings
 * d_img [n_images][dim]: similarities with d_txt [n_labels][dim] (sequential fp32 dot, same order as the host),
 * exp(x)+1e-9 normalised by the double-precision sum, sorted descending -> d_scores / d_indices [n_images][n_labels].
 * All pointers are HBM addresses; asynchronous on the ctx stream.  n_labels <= 8192, dim <= 4096. */
bool clip_amd_zero_shot_score_device(struct clip_ctx * ctx, const float * d_img, int n_images, const float * d_txt, int n_labels, int dim,
                                     float * d_scores, int * d_indices);

/* Batched clip_zero_shot_label_image: raw u8 images (host) x labels -> scores / indices [n_images][n_labels] (host), per
 * image exactly what clip_zero_shot_label_image returns.  Labels are encoded once (one ragged text batch), images are
 * preprocessed, encoded and scored on the GPU. */
bool clip_amd_zero_shot_label_images(struct clip_ctx * ctx, const struct clip_image_u8 * imgs, int n_images, const char ** labels,
                                     size_t n_labels, float * scores, int * indices);

/* Block until everything queued on the ctx stream has finished. */
void clip_amd_synchronize(struct clip_ctx * ctx);

/* Per-kernel-family accumulated device time (ms) since the last reset, measured with HIP events
 * on the ctx stream when profiling is enabled.  families: 0 gemm, 1 attention, 2 layernorm,
 * 3 other.  launches[] receives launch counts.  Returns number of families written. */
void clip_amd_profile_enable(struct clip_ctx * ctx, bool on);
int clip_amd_profile_read(struct clip_ctx * ctx, float * ms, int64_t * launches, int cap, bool reset);
/* Text report, one line per (kernel family : MxNxK) tag: "tag launches total_ms flops bytes".
 * Returns the number of bytes needed (call with buf == NULL to size the buffer). */
int clip_amd_profile_report(struct clip_ctx * ctx, char * buf, int cap, bool reset);

/* ---- exact nearest-neighbour index (semantic image search; the reference's examples/image-search uses an approximate usearch
 * index for the same job) ----
 * Cosine distance d = 1 - <q/|q|, g/|g|>: rows are L2-normalised in f32 when added, queries when searched (a zero vector stays zero:
 * distance exactly 1), both stored in the index dtype (0 = f32, 1 = f16: the normalised values rounded to fp16), dot products in f32.
 * The f32 / f16 store holds only finite values of magnitude <= 1; every kernel that orders or folds distances relies on it, and add,
 * the query path and load each keep it:
 *   1. a row or query with any NaN or +-inf element is the zero vector (distance exactly 1 to everything, lowest ids first), as for i8;
 *      an add never fails over its values (the device-pointer forms are asynchronous);
 *   2. for finite input the stored vector does not depend on a power-of-two scale of the input: x and x 2^e give the same stored bits
 *      whenever x 2^e is computed exactly (no element overflows or loses bits to underflow), rows of subnormals included.  In f32, in
 *      this order, without FMA contraction: amax = max_i |x_i| = m 2^e with m in [0.5, 1), y_i = x_i 2^-e (exact), ss = sum_i y_i^2
 *      (lane i % 64 adds its values in ascending i, then the xor butterfly 32 ... 1 over the 64 lanes), stored_i = y_i / sqrtf(ss);
 *   3. wherever the sum of squares of the unscaled row neither overflows nor underflows these are the bits of x_i / sqrtf(sum_i x_i^2)
 *      in the same order, which is what every earlier version stored: saved indexes keep searching identically;
 *   4. clip_amd_index_load returns NULL, with a message, for an f32 or f16 file that holds a non-finite value or one of magnitude
 *      above 1 (add cannot write either: sqrtf(fl(ss)) >= |y_i|); rows that are finite and within 1 but not of unit length are not
 *      looked for.  i8 files are unaffected: every byte is a legal value and the inverse norms are recomputed.
 * dtype 3 = i8 (2 is reserved): each row when added and each query when searched is quantised in f32, in this order, without FMA
 * contraction: amax = max_i |x_i|, q_i = (int8) rintf((x_i / amax) * 127.0f) (half to even; |x_i / amax| <= 1, no clamp); no L2
 * normalisation first (the mapping is scale-invariant).  A vector with amax == 0 or any NaN / inf is stored as the zero vector
 * (distance exactly 1).  d = 1 - (float)dot * inv_q * inv_r, dot = sum_i q_i r_i an exact int32 (|dot| <= 127^2 * 4096 < 2^31),
 * inv = 1.0f / sqrtf((float)sum_i v_i^2), 0 for the zero vector: the cosine distance of the stored integer vectors.  1 byte per value
 * (rows padded to 64 values in HBM) + 4 bytes per row for inv_r.
 * Rows get ids 0 ... n-1 in the order they were added; appending after a search is allowed, and so is removal: clip_amd_index_remove marks
 * rows in a device-resident bitmap (one bit per row) that the scan and join kernels honour, so search, search_device, range_search and
 * pairs never return a removed row (pairs neither as i nor as j; its lims keeps size + 1 entries, a removed row's segment is empty) and
 * an aligned group of 16 rows without a live row is not read from HBM.  Removal never reuses or renumbers ids: size still counts every id
 * ever given, live = size minus the removed rows, add after remove appends live rows with the next ids.  clip_amd_index_compact drops the
 * removed rows from device memory and renumbers the survivors 0 ... live - 1 in their old order.  The *_subset forms restrict a search to
 * the rows whose bit is set in a caller's bitmap (one directory, one album, everything not yet dismissed); a row is eligible when it is
 * live and allowed.  Results per query sorted
 * by ascending distance, equal distances lower id first; with k > the number of eligible rows the tail holds id -1 / distance +INFINITY.
 * A result over the eligible rows is, bit for bit, the result of an index to which only those rows were ever added (ids mapped in
 * order).  An index without removed rows searched without a subset runs the unmasked kernels.  1 <= k <= 1024,
 * 4 <= dim <= 4096 with dim % 4 == 0, any number of queries, up to 2^31 - 1 rows.  Results are bit-identical run to run, however queries
 * are split across calls, however rows were split across add calls, and across save / load.
 * The index lives on ctx's device and launches on ctx's stream (clip_amd_set_stream applies); free it before the ctx.  NULL on a
 * host-only ctx.  Bad arguments make a call return false (NULL) with a message on stderr, without launching anything.
 * File format (little-endian): "CLIPIDX1", u32 version (1), u32 dim, u32 dtype, u64 n, then n rows of dim stored values (unpadded;
 * i8: 1-byte values, inv_r is not stored but recomputed on the device at load, so a loaded index searches and re-saves identically).
 * The file has no place for removed rows: save on an index that holds any returns false with a message that says to compact first;
 * after compact, or when nothing was removed, save writes what it always wrote. */
struct clip_amd_index;
struct clip_amd_index * clip_amd_index_create(struct clip_ctx * ctx, int dim, int dtype);
bool clip_amd_index_add(struct clip_amd_index * ix, const float * vecs, int64_t n);            /* host rows [n][dim], synchronous */
bool clip_amd_index_add_device(struct clip_amd_index * ix, const float * d_vecs, int64_t n);   /* HBM rows, asynchronous on the ctx stream */
int64_t clip_amd_index_size(const struct clip_amd_index * ix);
int clip_amd_index_dim(const struct clip_amd_index * ix);
/* queries [n_queries][dim] -> distances [n_queries][k], ids [n_queries][k]; host pointers, synchronous */
bool clip_amd_index_search(struct clip_amd_index * ix, const float * queries, int n_queries, int k, float * distances, int64_t * ids);
/* the same on HBM pointers, asynchronous on the ctx stream */
bool clip_amd_index_search_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, float * d_distances,
                                  int64_t * d_ids);
bool clip_amd_index_save(struct clip_amd_index * ix, const char * path);
struct clip_amd_index * clip_amd_index_load(struct clip_ctx * ctx, const char * path);
void clip_amd_index_free(struct clip_amd_index * ix);
/* Mark rows as removed.  ids: n host values, each in [0, size); duplicates and already-removed ids are allowed.
 * Returns how many rows went from live to removed in this call; -1 (nothing changed) for a NULL index, n < 0, NULL ids with n > 0 or any id
 * outside [0, size).  Ids are never reused or renumbered by removal: clip_amd_index_size still counts every id ever given. */
int64_t clip_amd_index_remove(struct clip_amd_index * ix, const int64_t * ids, int64_t n);
int64_t clip_amd_index_live(const struct clip_amd_index * ix);            /* size minus removed rows */
/* bits: (size + 63) / 64 host words; bit (id & 63) of word id >> 6 is 1 for a live row; bits at positions >= size are written as 0. */
bool clip_amd_index_live_mask(struct clip_amd_index * ix, uint64_t * bits);
/* Drop the removed rows from device memory; survivors keep their order and get ids 0 ... live - 1.  new_ids (host, old size entries, may be
 * NULL) receives each old id's new id, -1 for a removed row.  Returns the new size, -1 on error.  Stored values (i8: and inverse norms) are
 * moved bit for bit: afterwards the index searches and saves exactly like one to which only the survivors were ever added.
 * Device memory at the peak: the old rows, the fresh allocation of the survivors and 8 bytes per old row for the new ids (also with
 * new_ids NULL); the old rows are freed before the call returns.  No removed rows: nothing is allocated or moved. */
int64_t clip_amd_index_compact(struct clip_amd_index * ix, int64_t * new_ids);
/* search / range_search restricted to the rows whose bit is set in allow (layout as live_mask; host words for the host forms, HBM for the
 * _device form; NULL = every row; bits at positions >= size are ignored, whatever they hold).  A removed row is never a result even if allowed. */
bool clip_amd_index_search_subset(struct clip_amd_index * ix, const float * queries, int n_queries, int k, const uint64_t * allow,
                                  float * distances, int64_t * ids);
bool clip_amd_index_search_subset_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, const uint64_t * d_allow,
                                         float * d_distances, int64_t * d_ids);
/* Grouped search: every row belongs to a group and a result holds each group at most once, represented by its best row (several crops or
 * views per image, ranked by image).  groups: size entries, each >= 0, groups[id] = the group of row id; any numbering, rows of a group need
 * not be adjacent.  Groups are an argument of the call, not index state: add, remove, compact, append and save know nothing of them.
 * With L = every eligible row (live and allowed, allow as for search_subset, NULL = every row) in search's order (distance ascending, equal
 * distances lower id first), the result of a query is the rows of L whose group has not appeared earlier in L, cut to k; the tail is -1 /
 * +INFINITY.  ids are row ids and distances the bits clip_amd_index_search reports for the same (query, row) pair, so with all groups
 * distinct the result is search_subset's, bit for bit.  1 <= k <= 1024; the result does not depend on how queries are split across calls.
 * Host form: groups and allow are host arrays (groups is uploaded for the call); a negative group, NULL groups with size > 0 or any bad
 * argument of search returns false with a message and launches nothing.  Device form: d_groups (int32) and d_allow are read from HBM and
 * trusted. */
bool clip_amd_index_search_grouped(struct clip_amd_index * ix, const float * queries, int n_queries, int k, const int32_t * groups,
                                   const uint64_t * allow, float * distances, int64_t * ids);
bool clip_amd_index_search_grouped_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, const int32_t * d_groups,
                                          const uint64_t * d_allow, float * d_distances, int64_t * d_ids);
/* Average device time (microseconds, HIP events) of one clip_amd_index_search_device of n_queries seeded random queries against n seeded
 * random rows on the current device (dtype as clip_amd_index_create: 0, 1 or 3); < 0 on error.  Used by scripts/search_bench.py. */
float clip_amd_bench_search(int dtype, int64_t n, int dim, int n_queries, int k, int iters);
/* The same for clip_amd_index_search_grouped_device over the same seeded rows and queries, row r in group r / group_size (group_size >= 1).
 * Used by scripts/regions_bench.py. */
float clip_amd_bench_search_grouped(int dtype, int64_t n, int dim, int n_queries, int k, int group_size, int iters);
/* Query sets: a set of query rows stands for one thing (the regions of one image) and its result is the best stored rows over all of its
 * rows, each key at most once, with the query row that matched.  set_lims: host int64 [n_sets + 1], starting at 0, non-decreasing and
 * ending at n_queries, in the style of the lims of range_search; set s is the query rows set_lims[s] ... set_lims[s + 1] - 1; an empty set
 * is legal and gives an all-empty result.  groups as for search_grouped, or NULL: every row is its own key.
 * For set s take every pair (query row q of the set, eligible stored row r), eligible as for search_subset, ordered by distance ascending,
 * then r, then q; a pair is kept when the key of r (groups[r]; NULL groups: r) has not been seen earlier in the set's walk; the walk stops
 * at k kept pairs.  Per set: distances [k] f32, ids [k] int64 (the stored row), qrows [k] int32 (the query row's index within the call);
 * the tail is +INFINITY / -1 / -1.  A distance is, bit for bit, what clip_amd_index_search reports for that (query, row) pair: with every
 * set of size one the result is search_grouped's (NULL groups: search_subset's) and qrows counts up.  A set's result does not depend on
 * the other sets of the call or on how the call is cut into passes internally.  1 <= k <= 1024, 0 <= n_sets < 2^31.
 * Host form: host arrays, synchronous; device memory beyond the index is the fixed workspace of knn_graph (query blocks one after
 * another), whatever n_queries and n_sets.  Device form: queries, groups, allow and the three outputs in HBM (groups and allow trusted),
 * asynchronous on the context's stream; set_lims stays a host array because it shapes the launches and is read before the call returns.
 * search_ids_sets: the query rows are the stored rows ids[0 ... n_ids), gathered bit for bit as search_ids does (a row is not excluded as
 * "self"); exclude_own != 0: a pair (q, r) is not eligible when groups[r] == groups[ids[q]], so a group never matches itself through any
 * pair of its own rows; it needs groups.  An id out of range or removed returns false, names the id, launches nothing and leaves the
 * outputs untouched, as for search_ids.
 * Checked before any launch, outputs untouched: set_lims not starting at 0, decreasing or not ending at the number of query rows; a
 * negative group (host forms); exclude_own with NULL groups; k out of range; NULL pointers; everything search refuses. */
bool clip_amd_index_search_sets(struct clip_amd_index * ix, const float * queries, int n_queries, const int64_t * set_lims, int64_t n_sets, int k,
                                const int32_t * groups, const uint64_t * allow, float * distances, int64_t * ids, int32_t * qrows);
bool clip_amd_index_search_sets_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, const int64_t * set_lims, int64_t n_sets,
                                       int k, const int32_t * d_groups, const uint64_t * d_allow, float * d_distances, int64_t * d_ids,
                                       int32_t * d_qrows);
bool clip_amd_index_search_ids_sets(struct clip_amd_index * ix, const int64_t * ids, int64_t n_ids, const int64_t * set_lims, int64_t n_sets, int k,
                                    int exclude_own, const int32_t * groups, const uint64_t * allow, float * distances, int64_t * out_ids,
                                    int32_t * qrows);
/* test hook: the query rows per block of the two host forms above on this index from now on (1 ... 65408; 0: automatic), so that a test
 * can make small sets straddle blocks.  Returns the value set, -1 for a NULL index or another value. */
int64_t clip_amd_test_index_sets_block(struct clip_amd_index * ix, int64_t rows);
/* Average device time (microseconds, HIP events) of one clip_amd_index_search_sets_device of n_sets sets of set_size seeded random query
 * rows each over the seeded rows of clip_amd_bench_search, row r in group r / group_size (0: no groups); < 0 on error.  Used by
 * scripts/sets_bench.py. */
float clip_amd_bench_search_sets(int dtype, int64_t n, int dim, int n_sets, int set_size, int k, int group_size, int iters);
/* Distinct search: near-duplicates fold into one hit (the retrieval form of non-maximum suppression).  Inputs: a query, k, radius R, pool
 * P and allow.
 * Pool: L is the query's result from clip_amd_index_search_subset(ix, q, 1, P, allow): the P nearest eligible rows (live and allowed) in
 * search's order, distance ascending, equal distances lower id first.  Empty tail slots are not members.  SUPPRESSION IS OVER THE POOL,
 * NOT THE WHOLE INDEX: a row outside the P nearest neither suppresses nor is counted.  The pool bounds memory and time, and it makes the
 * result a closed-form function of search's output.
 * Near: two members a != b are near when d(min(a, b), max(a, b)) <= R, compared in f32.  d(i, j) for i < j is exactly the distance
 * clip_amd_index_pairs defines for that pair: what search reports for row j when the query is the vector that was added as row i (row
 * i's stored values are the prepared query; i8: inv_q := inv_r[i]).  So (a, b) are near at R exactly when pairs(R) lists the pair.
 * Walk: walk L in order.  A member that an earlier KEPT member is near to is suppressed: it is skipped, and a suppressed member never
 * suppresses anything.  Every other member is kept.  The walk stops at k kept members.
 * Outputs per query: distances [k] f32 (the query-to-row bits search reports), ids [k] int64, counts [k] int32: counts[t] is the number
 * of pool members that kept member t suppressed, each suppressed member counted once, for the first kept member (in walk order) that is
 * near it; the count runs over the whole pool, including members ranked behind the k-th kept one.  Tail: +INFINITY / -1 / 0.
 * Consequences: R < 0 suppresses nothing (search_subset's first k, bit for bit, all counts 0); a very large R (4, say) keeps only the
 * pool's first member, with count = members - 1; a query's result depends neither on the other queries of the call nor on how the call is
 * cut into blocks; results are bit-identical run to run and across save / load.
 * Limits: 1 <= k <= pool <= 1024; pool == 0 is automatic: min(1024, max(64, 8 k)).  A NaN radius, a pool outside the range, an empty
 * index, n_queries < 1 and everything search_subset refuses return false with a message that names the value; nothing is launched and
 * the outputs are untouched.
 * Host form: host arrays, synchronous; device memory beyond the index is a fixed budget (query blocks one after another: the near bitmap
 * alone is 128 KB per query at pool 1024), whatever n_queries.  Device form: queries, allow (trusted) and the three outputs in HBM,
 * asynchronous on the context's stream.  search_ids_distinct: the queries are the stored rows ids[0 ... n_ids), gathered bit for bit as
 * search_ids does; an id out of range or removed returns false, names the id and leaves the outputs untouched.  exclude_self != 0: the
 * query's own row is not in the pool, so it suppresses nothing either. */
bool clip_amd_index_search_distinct(struct clip_amd_index * ix, const float * queries, int n_queries, int k, float radius, int pool,
                                    const uint64_t * allow, float * distances, int64_t * ids, int32_t * counts);
bool clip_amd_index_search_distinct_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, float radius, int pool,
                                           const uint64_t * d_allow, float * d_distances, int64_t * d_ids, int32_t * d_counts);
bool clip_amd_index_search_ids_distinct(struct clip_amd_index * ix, const int64_t * ids, int n_ids, int k, float radius, int pool, int exclude_self,
                                        const uint64_t * allow, float * distances, int64_t * out_ids, int32_t * counts);
/* test hook: the queries per block of the distinct searches on this index from now on (1 ... 4096; 0: automatic), so that a test can make
 * a call straddle blocks.  Returns the value set, -1 for a NULL index or another value. */
int clip_amd_test_index_distinct_block(struct clip_amd_index * ix, int queries);
/* Average device time (microseconds, HIP events) of one clip_amd_index_search_distinct_device of n_queries seeded random queries over n
 * seeded rows in groups of copies + 1: a seeded random row followed by `copies` noisy copies of it (the row + 0.05 uniform(-1, 1) per
 * value, before normalisation: seeded random rows alone have no near pairs and the walk would never suppress anything); < 0 on error.
 * Used by scripts/distinct_bench.py. */
float clip_amd_bench_search_distinct(int dtype, int64_t n, int dim, int n_queries, int k, int pool, float radius, int copies, int iters);
/* Compound queries: a query is several terms ("a dog" and "on a beach"; like this stored picture and "at night"; "a beach" but not
 * "people"; ranked by A but only within R of image B).  A call holds n_queries compound queries; query c is the terms term_lims[c] ...
 * term_lims[c + 1] - 1 (term_lims: host int64 [n_queries + 1], starting at 0 and increasing, like set_lims), 1 ... 8 of them.
 * A term is a vector and a kind and, for the filter kinds, a bound (f32): terms [total][dim] f32 holds the vectors; term_ids [total] (or
 * NULL) replaces a term's vector by a stored row where term_ids[t] >= 0 (the row's stored values bit for bit, as search_ids gathers them;
 * i8: its inverse norm comes along; the vector is then not used); kinds [total] int32 and bounds [total] f32 (read for kinds 1 ... 3 only).
 * d_t(row) is the distance clip_amd_index_search reports for (term t, row), bit for bit.
 *   kind 0 "all"     scoring term: score(row) = the max over the query's all-terms of d_t(row); at least one per query
 *   kind 1 "within"  the row is eligible only if d_t(row) <= bound (range_search's comparison)
 *   kind 2 "beyond"  the row is eligible only if d_t(row) > bound (its complement)
 *   kind 3 "over"    the row is eligible only if d_t(row) > score(row) + bound, one f32 addition and then the compare; with bound 0 the
 *                    row is strictly nearer to what is asked for than to this term
 * Eligible rows are live, set in allow (as for search_subset; NULL = every row) and pass every filter term; with exclude_terms != 0 the
 * rows named as id terms of that query are not eligible either.  The result is the k best eligible rows by (score ascending, id
 * ascending), search's order; the tail is +INFINITY / -1.  The reported distance is the score: bit for bit one of the all-terms' distances.
 * Consequences: a query of a single all-term is search_subset bit for bit; with exclude_terms and an id term it is search_ids with
 * exclude_self; a result depends neither on the other queries of the call, nor on how terms are padded, nor on how the call is cut into
 * blocks; results are bit-identical run to run, across save / load and however rows were split across add calls.
 * Any-of (the union of the terms' top-k lists) and weighted means (one query vector) compose exactly from the other calls and are not
 * offered here; per-hit term distances are not returned (range_search at radius 4 with allow set to the hits gives them).
 * Limits: 1 <= k <= 1024, 1 <= terms per query <= 8.  A NaN bound of a filter term, an unknown kind, a query without an all-term or with
 * 0 or more than 8 terms, term_lims not starting at 0 or decreasing, an empty index, n_queries < 1 and everything search_subset refuses
 * return false with a message that names the value; nothing is launched and the outputs are untouched.
 * Host form: host arrays, synchronous; an id term out of range or removed returns false, names the id and leaves the outputs untouched,
 * as search_ids does; device memory beyond the index is a fixed budget (query blocks one after another), whatever n_queries.  Device
 * form: terms, allow (trusted) and the two outputs in HBM, the small arrays (term_ids, kinds, bounds, term_lims) on the host and read
 * before the call returns; asynchronous on the context's stream; a bad id term yields an all-empty result row, as search_ids_device does. */
bool clip_amd_index_search_compound(struct clip_amd_index * ix, const float * terms, const int64_t * term_ids, const int32_t * kinds,
                                    const float * bounds, const int64_t * term_lims, int n_queries, int k, int exclude_terms,
                                    const uint64_t * allow, float * distances, int64_t * ids);
bool clip_amd_index_search_compound_device(struct clip_amd_index * ix, const float * d_terms, const int64_t * term_ids, const int32_t * kinds,
                                           const float * bounds, const int64_t * term_lims, int n_queries, int k, int exclude_terms,
                                           const uint64_t * d_allow, float * d_distances, int64_t * d_ids);
/* test hook: the compound queries per block of the two forms above on this index from now on (1 ... 1024; 0: automatic), so that a test
 * can make a call straddle blocks.  Returns the value set, -1 for a NULL index or another value. */
int clip_amd_test_index_compound_block(struct clip_amd_index * ix, int queries);
/* Average device time (microseconds, HIP events) of one clip_amd_index_search_compound_device of n_queries compound queries of n_terms
 * all-terms each (seeded random vectors) over the seeded rows of clip_amd_bench_search; < 0 on error.  Used by scripts/compound_bench.py. */
float clip_amd_bench_search_compound(int dtype, int64_t n, int dim, int n_queries, int n_terms, int k, int iters);
/* The same with an allowed set over the same seeded rows and queries (clip_amd_index_search_subset_device): allowed_fraction in [0, 1] of
 * the ids, a seeded random selection or, contiguous != 0, one id range in the middle of the index.  Used by scripts/subset_bench.py. */
float clip_amd_bench_search_subset(int dtype, int64_t n, int dim, int n_queries, int k, float allowed_fraction, int contiguous, int iters);
/* Neighbours of stored rows and the k-NN graph: searches whose queries are rows of the index itself ("more like this one", the related
 * images of every image), without the vectors that were added and without a model.
 * The query for ids[t] is that row's stored values copied bit for bit (i8: inv_q := inv_r of the row); it is never renormalised or
 * requantised, so with exclude_self == 0 the result for ids[t] is, bit for bit (distances, ids, order, tail), what
 * clip_amd_index_search_subset returns for the vector that was added as that row with the same allow.  With exclude_self != 0 row ids[t]
 * is not eligible for query t (other queries still see it): the result is, bit for bit, search_subset with that row's bit cleared in
 * allow, the result of an index that never held the row; equal distances still come lower id first and the tail holds -1 / +INFINITY.
 * allow (layout as live_mask) restricts the candidates only: the query row itself need not be allowed; NULL = every live row.
 * 1 <= k <= 1024; duplicate ids are fine; n_ids == 0 succeeds and launches nothing.
 * Host form: an id outside [0, size) or a removed id makes the call return false with a message on stderr that names the id; nothing is
 * launched and the outputs are untouched (the discipline of clip_amd_index_remove).  Device form: the ids cannot be checked without a
 * round trip, so an out-of-range or removed id yields an all-empty result row (-1 / +INFINITY); the gather tests the id before it reads
 * anything there, so such an id never causes an out-of-bounds read.
 * knn_graph: for every id in [0, size) its k nearest OTHER live rows; distances / ids are host [size][k].  Row i is search_ids(i, k,
 * exclude_self = 1, allow = NULL) for a live row i, bit for bit; the row of a removed id is all -1 / +INFINITY; size == 0 succeeds and
 * writes nothing.  Small indexes run the self-excluding scan over blocks of gathered rows, larger ones the tiled kernel of k_graph.hip
 * (128 stored rows x 128 stored rows per workgroup step, the top-k selection of the scan behind it); both give the same bits.  Device
 * memory beyond the index is a fixed workspace (candidates <= 512 MB, one query block's results <= 128 MB): query blocks are processed
 * and copied out one after another, nothing grows with size x k.
 * Results are bit-identical run to run, across both graph routes, however rows were split across add calls, across save / load, and
 * across compact (ids mapped through new_ids) as long as no removed row was among a survivor's neighbours. */
bool clip_amd_index_search_ids(struct clip_amd_index * ix, const int64_t * ids, int n_ids, int k, int exclude_self, const uint64_t * allow,
                               float * distances, int64_t * out_ids);                                       /* host, synchronous */
bool clip_amd_index_search_ids_device(struct clip_amd_index * ix, const int64_t * d_ids, int n_ids, int k, int exclude_self,
                                      const uint64_t * d_allow, float * d_distances, int64_t * d_out_ids);  /* HBM, asynchronous */
bool clip_amd_index_knn_graph(struct clip_amd_index * ix, int k, float * distances, int64_t * ids);
/* test hook: the route of clip_amd_index_knn_graph on this index from now on: 0 automatic, 1 the scan route, 2 the tiled kernel.  Returns
 * the route set, -1 for a NULL index or another value. */
int clip_amd_test_index_knn_route(struct clip_amd_index * ix, int route);
/* Average wall time (microseconds) of one clip_amd_index_knn_graph over n seeded random rows on the current device (results copied to the
 * host included), route as above; < 0 on error.  Used by scripts/knn_bench.py. */
float clip_amd_bench_knn(int dtype, int64_t n, int dim, int k, int route, int iters);
/* k-NN voting: "which of MY classes does this belong to?", answered from labelled stored rows.  File a new picture into the folder most
 * of its neighbours sit in (vote), or find the pictures that sit in the wrong folder (vote_graph, the leave-one-out form).
 * labels: one int32 per row id, [size]: >= 0 the class of a labelled row (any numbering up to 2^31 - 1), -1 unlabelled.  Labels are an
 * argument of the call, not index state, like groups.  A row is a VOTER when it is live, allowed (allow as for
 * clip_amd_index_search_subset, NULL = every row) and labelled.  For one query, with 1 <= m <= k <= 1024:
 *   1. L is the first k voters in search's order (distance ascending, equal distances lower id first): bit for bit,
 *      clip_amd_index_search_subset with the voter bitmap as allow;
 *   2. for each class c that occurs in L, votes(c) is the number of its entries in L and first(c) the rank of its nearest entry;
 *   3. the classes are ordered by votes descending, then first ascending (ranks are distinct, so the order is total, and k = 1 is
 *      nearest-neighbour classification);
 *   4. the query's outputs are classes [m] int32, votes [m] int32, distances [m] f32 (the distance of the class's nearest voter, the bits
 *      search reports for that pair) and ids [m] int64 (that voter's row);
 *   5. the tail is -1 / 0 / +INFINITY / -1.
 * With all labels distinct and m == k the result is search_subset's with votes all 1; fewer than k voters make L shorter; no voter at all
 * gives an all-empty row, and so does an empty index.  A query's result does not depend on the other queries, on how queries are split
 * across calls or blocks, or on the route: it is made of integers and of distances search reports, so it is as exact and bit-reproducible
 * as search.  Votes are plain counts: distance-weighted votes are out of scope (a float sum would need an order of its own, and the
 * tie-break on the nearest member already carries most of the benefit).
 * vote: n_queries f32 vectors [n_queries][dim], results [n_queries][m].
 * vote_ids: the stored rows ids[0 ... n_ids) as the queries, each bit for bit as in clip_amd_index_search_ids; with exclude_self != 0 a row
 * is no voter for its own query.  The query row need not be labelled or allowed.  A bad id: as clip_amd_index_search_ids (false, the id
 * named, outputs untouched).
 * vote_graph: every row as the query, itself excluded: results [size][m]; row i is vote_ids(i, exclude_self = 1) for a live row i, bit
 * for bit, the row of a removed id is empty, size == 0 succeeds and writes nothing.  The routes are clip_amd_index_knn_graph's, chosen as
 * there (clip_amd_test_index_knn_route); on the tiled route one 4-byte word is read back before the first block ("is some live row no
 * voter?"): if so every block takes a second tile pass for those rows, if not the pass is knn_graph's own.
 * Host forms refuse, before any launch, with a message that names the value and with the outputs untouched: a label < -1, NULL labels
 * with size > 0, m < 1, m > k, k outside 1 ... 1024, NULL pointers and everything search_subset refuses.  Device forms trust d_labels: any
 * negative value counts as unlabelled.  Device memory beyond the index: the workspaces of the search, the voter bitmap (one bit per row),
 * the labels of a host form and one query block's results; nothing grows with size x k. */
bool clip_amd_index_vote(struct clip_amd_index * ix, const float * queries, int n_queries, int k, int m, const int32_t * labels,
                         const uint64_t * allow, int32_t * classes, int32_t * votes, float * distances, int64_t * ids);   /* host, synchronous */
bool clip_amd_index_vote_device(struct clip_amd_index * ix, const float * d_queries, int n_queries, int k, int m, const int32_t * d_labels,
                                const uint64_t * d_allow, int32_t * d_classes, int32_t * d_votes, float * d_distances,
                                int64_t * d_ids);                                                                        /* HBM, asynchronous */
bool clip_amd_index_vote_ids(struct clip_amd_index * ix, const int64_t * ids, int64_t n_ids, int k, int m, int exclude_self,
                             const int32_t * labels, const uint64_t * allow, int32_t * classes, int32_t * votes, float * distances,
                             int64_t * out_ids);                                                                         /* host, synchronous */
bool clip_amd_index_vote_graph(struct clip_amd_index * ix, int k, int m, const int32_t * labels, const uint64_t * allow, int32_t * classes,
                               int32_t * votes, float * distances, int64_t * ids);                                       /* host, synchronous */
bool clip_amd_index_vote_graph_device(struct clip_amd_index * ix, int k, int m, const int32_t * d_labels, const uint64_t * d_allow,
                                      int32_t * d_classes, int32_t * d_votes, float * d_distances, int64_t * d_ids);    /* results stay in HBM */
/* test hook: query rows per block of the votes on this index from now on (0: automatic), as clip_amd_test_index_sets_block.  Returns the
 * value set, -1 for a NULL index or a value outside 0 ... 65408. */
int64_t clip_amd_test_index_vote_block(struct clip_amd_index * ix, int64_t rows);
/* Average wall time (microseconds) of one clip_amd_index_vote_graph over the n seeded random rows of clip_amd_bench_knn, the label of a row
 * a seeded hash of its number modulo `classes`, route as clip_amd_bench_knn; < 0 on error.  Used by scripts/vote_bench.py. */
float clip_amd_bench_vote_graph(int dtype, int64_t n, int dim, int k, int m, int classes, int route, int iters);
/* One index searched with the rows of another, and one index appended to another: label every image of a database with a small index of
 * captions, find which images of B a database A already holds (k = 1), merge two databases without encoding anything twice.
 * search_index: the queries are stored rows of src: ids[0 ... n_ids) (host), or with ids == NULL every row 0 ... size(src) - 1 (n_ids is
 * then ignored); the candidates are the rows of ix that are live and set in allow (layout as live_mask, (size(ix) + 63) / 64 host words;
 * NULL = every live row).  distances / out_ids are host [n][k], laid out as search lays them out.  Result row t is, bit for bit, what
 * clip_amd_index_search_subset(ix, v, 1, k, allow, ...) returns for the vector v that was added to src as row ids[t]: the stored row is
 * the prepared query (i8: inv_q := its inv_r) and is copied, never renormalised or requantised.  ix == src is allowed and equals
 * search_ids(..., exclude_self = 0, allow).  Requirements, checked before anything is launched: both indexes non-NULL, of the same ctx,
 * dim and dtype; src holds no removed rows (compact it first: a query-side mask stays out of the kernel, and databases on disk never
 * hold removed rows); every id in [0, size(src)); 1 <= k <= 1024; result pointers non-NULL when there is a query.  A failed check returns
 * false with a message on stderr that names the offending value and leaves the outputs untouched.  No queries: succeeds, launches
 * nothing; size(ix) == 0: every row all -1 / +INFINITY.  With ids, and for few queries, the rows are gathered from src's store and
 * scanned like any query; with ids == NULL and many queries the tiled kernel of k_graph.hip reads both stores directly; both give the same
 * bits.  Synchronous on the ctx stream; device memory beyond the two indexes is the fixed workspace of knn_graph (query blocks are
 * processed and copied out one after another).
 * append: copies every row of src, in order and bit for bit (stored values, i8 inverse norms), to the end of ix, where they are live rows
 * with the next ids; new_ids (host, size(src) entries, may be NULL) receives each src id's id in ix.  Returns the number of rows appended
 * (0 for an empty src), or -1 with nothing changed: the requirements above, ix != src and size(ix) + size(src) <= 2^31 - 1.  Afterwards ix
 * searches and saves exactly like an index to which src's vectors had been added with clip_amd_index_add; src is unchanged. */
bool clip_amd_index_search_index(struct clip_amd_index * ix, struct clip_amd_index * src, const int64_t * ids, int64_t n_ids, int k,
                                 const uint64_t * allow, float * distances, int64_t * out_ids);             /* host pointers, synchronous */
int64_t clip_amd_index_append(struct clip_amd_index * ix, struct clip_amd_index * src, int64_t * new_ids);
/* test hook: the route of clip_amd_index_search_index with ids == NULL on this index (as ix) from now on: 0 automatic, 1 the scan route,
 * 2 the tiled kernel.  Returns the route set, -1 for a NULL index or another value. */
int clip_amd_test_index_cross_route(struct clip_amd_index * ix, int route);
/* Average wall time (microseconds) of one clip_amd_index_search_index of an index of n_rows seeded random rows with all n_queries seeded
 * random rows of a second one (results copied to the host included), route as above; < 0 on error.  Used by scripts/cross_bench.py. */
float clip_amd_bench_cross(int dtype, int64_t n_rows, int64_t n_queries, int dim, int k, int route, int iters);
/* Range search and near-duplicate pairs.
 * Distance: exactly what clip_amd_index_search reports for the same (query, row) pair (the same stored values, the same MFMA chain per
 * dtype, the same f32 expression); a row is a result when d <= radius, compared in f32.
 * range_search: for each query every stored (live) row with d <= radius, sorted by ascending distance, equal distances lower id first (search's
 * order: for a query with c <= 1024 results, search with any k >= c begins with exactly those c (id, distance) pairs, bit for bit).
 * pairs: every (i, j) of live rows with i < j < size and d(i, j) <= radius, d(i, j) being the distance search reports for row j when the query is the
 * vector that was added as row i (row i's stored values are exactly that query's normalised / quantised form); grouped by ascending i,
 * within one i in range-search order, so the pairs of row i are range_search(vector of row i) without the ids <= i, bit for bit.
 * Results are bit-identical run to run, however queries are split across calls, however rows were split across add calls, and across
 * save / load.  Zero vectors (i8: also rows with amax 0, NaN or inf) are at distance exactly 1 from everything: results only at radius >= 1.
 * Host pointers, synchronous, on the ctx stream.  lims has n_queries + 1 (range_search) / size + 1 (pairs) entries and is written on every
 * successful call: segment q is [lims[q], lims[q + 1]).  Returns the total lims[last]; distances / ids (capacity entries) are written only
 * when total <= capacity, otherwise only lims (call again with a larger buffer); capacity 0 with NULL outputs is a count-only call.
 * -1 with a message on stderr, nothing launched, for a NULL index or lims, a NaN radius, n_queries < 0, capacity < 0, NULL outputs with
 * capacity > 0 or NULL queries with n_queries > 0.  Device memory: O(size + n_queries + min(total, capacity)) plus a fixed workspace. */
int64_t clip_amd_index_range_search(struct clip_amd_index * ix, const float * queries, int n_queries, float radius,
                                    int64_t * lims, float * distances, int64_t * ids, int64_t capacity);
int64_t clip_amd_index_pairs(struct clip_amd_index * ix, float radius, int64_t * lims, float * distances, int64_t * ids, int64_t capacity);
/* range_search over the allowed rows only (allow as for clip_amd_index_search_subset, host words) */
int64_t clip_amd_index_range_search_subset(struct clip_amd_index * ix, const float * queries, int n_queries, float radius, const uint64_t * allow,
                                           int64_t * lims, float * distances, int64_t * ids, int64_t capacity);
/* Average wall time (microseconds) of one clip_amd_index_range_search of n_queries seeded queries (n_queries == 0: clip_amd_index_pairs)
 * against n seeded random rows of which every 64th is a small perturbation of an earlier one (sparse, non-empty output at small radii), on
 * the current device (dtype as clip_amd_index_create); < 0 on error.  Used by scripts/pairs_bench.py. */
float clip_amd_bench_range(int dtype, int64_t n, int dim, int n_queries, float radius, int iters);
/* Connected components of the graph "distance <= radius": the groups of near-duplicates as one label per row, whatever the number of near
 * pairs (a burst of m copies is m (m - 1) / 2 pairs for clip_amd_index_pairs and m labels here; no pair ever leaves the device).
 * Near pairs: two eligible rows i < j (live and set in allow, layout as live_mask, NULL = every live row) are near when d(i, j) <= radius,
 * compared in f32, d(i, j) being exactly the distance clip_amd_index_pairs defines for that pair: they are near at R exactly when pairs(R)
 * over the eligible rows lists them.
 * labels [size] int64: the lowest id of the row's component; the row itself for a row without a near row; -1 for a removed or not allowed
 * row.  nearest_distance [size] f32: the smallest d over the near pairs the row takes part in, on either side (as i or as j), the bits pairs
 * reports; nearest_id [size] int64: the other row of that pair, the lower id among equal distances; +INFINITY / -1 when the row has no
 * near row (and for a row that is not eligible).  Either of the two, or both, may be NULL.
 * The host form returns the number of components with at least two rows: exactly the roots (labels[x] == x) that have a nearest id; 0 for
 * an empty index (nothing is written); -1 on error.  Results are bit-identical run to run, however rows were split across add calls and
 * across save / load; over the eligible rows they are those of an index to which only those rows were ever added (ids mapped in order).
 * -1 / false with a message on stderr, nothing launched, for a NULL index, NULL labels or a NaN radius.
 * Host form: host arrays, synchronous on the ctx stream.  Device form: allow (trusted) and the outputs in HBM, asynchronous on the ctx
 * stream, synchronises with nothing on the host.  Device memory beyond the index: 16 bytes per row (the host form 20 more for its results). */
int64_t clip_amd_index_components(struct clip_amd_index * ix, float radius, const uint64_t * allow, int64_t * labels, float * nearest_distance,
                                  int64_t * nearest_id);
bool clip_amd_index_components_device(struct clip_amd_index * ix, float radius, const uint64_t * d_allow, int64_t * d_labels,
                                      float * d_nearest_distance, int64_t * d_nearest_id);
/* Average wall time (microseconds) of one clip_amd_index_components (host form, all three outputs) over the seeded rows of
 * clip_amd_bench_range; < 0 on error.  Used by scripts/components_bench.py. */
float clip_amd_bench_components(int dtype, int64_t n, int dim, float radius, int iters);
/* Density modes: the index grouped into albums, each with a cover.  Every row points to its nearest row of higher local density; the roots
 * of that forest are the modes (the most typical rows, not outliers), every tree is an album and its root the cover.
 * E is the set of eligible rows (live and set in allow, layout as live_mask, NULL = every live row); for a pair {x, y} of E, d(x, y) is
 * the distance clip_amd_index_pairs reports for (min, max), the same bits from the same chain.  radius and link are compared in f32.
 * density [size] int32: the number of y in E, y != x, with d(x, y) <= radius.
 * y OUTRANKS x when density[y] > density[x], or the densities are equal and y < x.
 * parent [size] int64: the y that minimises (d(x, y), y) over the rows of E that outrank x and have d(x, y) <= link; -1 when there is none.
 * parent_distance [size] f32: that distance, the bits pairs reports; +INFINITY without a parent.
 * labels [size] int64: the root reached from x by following parent (rank rises strictly along every step: no cycle).
 * A row outside E gets label -1, parent -1, distance +INFINITY and density -1.  parent, parent_distance and density may each be NULL.
 * The host form returns the number of modes: the rows of E without a parent, singletons included; 0 for an empty index (nothing is
 * written); -1 on error.  Among exact copies the lowest id is the root.  Results are bit-identical run to run, however rows were split
 * across add calls and across save / load, and do not depend on the order of any atomic; over E they are those of an index to which only
 * the rows of E were ever added (ids mapped in order).
 * -1 / false with a message on stderr, nothing launched, for a NULL index, NULL labels or a NaN radius or link (pass link = radius for one
 * scale; link = INFINITY leaves only the top-ranked row as a root).
 * Host form: host arrays, synchronous on the ctx stream.  Device form: allow (trusted) and the outputs in HBM, asynchronous on the ctx
 * stream, synchronises with nothing on the host.  Device memory beyond the index: 20 bytes per row (the host form 24 more for its results). */
int64_t clip_amd_index_modes(struct clip_amd_index * ix, float radius, float link, const uint64_t * allow, int64_t * labels, int64_t * parent,
                             float * parent_distance, int32_t * density);
bool clip_amd_index_modes_device(struct clip_amd_index * ix, float radius, float link, const uint64_t * d_allow, int64_t * d_labels,
                                 int64_t * d_parent, float * d_parent_distance, int32_t * d_density);
/* Average wall time (microseconds) of one clip_amd_index_modes (host form, all four outputs); copies == 0: over the seeded rows of
 * clip_amd_bench_range (sparse), copies > 0: over the groups of a row and `copies` noisy copies of clip_amd_bench_search_distinct (dense);
 * < 0 on error.  Used by scripts/modes_bench.py. */
float clip_amd_bench_modes(int dtype, int64_t n, int dim, float radius, float link, int copies, int iters);
/* The single-linkage tree: the minimum spanning tree of the eligible rows under the index's own distances.  Its edges, sorted, are the
 * single-linkage dendrogram: cutting the tree at any R (dropping the edges with d > R) leaves exactly the groups clip_amd_index_components
 * gives at R, dropping its N - 1 longest edges leaves exactly N groups, and the sorted distances are the table of radius against number
 * of groups.  One call answers for every radius.
 * E is the set of eligible rows (live and set in allow, layout as live_mask, NULL = every live row), m its size; for x < y in E, d(x, y) is
 * the distance clip_amd_index_pairs reports for that pair, the same bits from the same chain.  Every comparison is in f32 on those bits.
 * Edges are ordered by (d, lo, hi), lo < hi, lexicographically: a total order.  The result is the minimum spanning forest of the graph
 * "d <= link" under that order: an edge belongs to it exactly when its endpoints are not connected by strictly smaller edges.  So the
 * forest is unique.  link = INFINITY gives the whole tree, m - 1 edges; a finite link gives m - c edges, c being the number of components
 * at link, singletons included, and those edges are the first m - c of the whole tree.
 * Host form: lo, hi [size - 1] int64 and distances [size - 1] f32 receive the edges in ascending edge order; returns their number, 0 when
 * m <= 1 (nothing is written), -1 on error.  Device form: the same set of edges into HBM arrays of the same capacity and their number into
 * d_count (int64); their order is not specified, but it is the same, byte for byte, run to run.
 * Results are bit-identical run to run, however rows were split across add calls and across save / load, and do not depend on the order
 * of any atomic; over E they are those of an index to which only the rows of E were ever added (ids mapped in order).
 * -1 / false with a message on stderr, nothing launched and no output written, for a NULL index, a NULL output or a NaN link.
 * Host form: host arrays, synchronous on the ctx stream.  Device form: allow (trusted) and the outputs in HBM, asynchronous on the ctx
 * stream, synchronises with nothing on the host: it queues ceil(log2 size) rounds, each one sweep over the pairs of E plus O(size) work,
 * and a round after the tree is complete exits at once.  Device memory beyond the index: 32 bytes per row (the host form 20 more for its
 * results). */
int64_t clip_amd_index_linkage(struct clip_amd_index * ix, float link, const uint64_t * allow, int64_t * lo, int64_t * hi, float * distances);
bool clip_amd_index_linkage_device(struct clip_amd_index * ix, float link, const uint64_t * d_allow, int64_t * d_lo, int64_t * d_hi,
                                   float * d_distances, int64_t * d_count);
/* Average wall time (microseconds) of one clip_amd_index_linkage (host form, link = INFINITY) over the rows of clip_amd_bench_modes
 * (copies == 0: sparse, copies > 0: groups of a row and `copies` noisy copies); < 0 on error.  clip_amd_bench_linkage_rounds: the rounds
 * that did work in the last call of it.  Used by scripts/linkage_bench.py. */
float clip_amd_bench_linkage(int dtype, int64_t n, int dim, int copies, int iters);
int clip_amd_bench_linkage_rounds(void);
/* The rounds that did work in the index's last clip_amd_index_linkage (host form): sweeps over the pairs that ran; -1 for a NULL index.
 * Used by scripts/linkage_bench.py and tests/. */
int clip_amd_test_index_linkage_rounds(struct clip_amd_index * ix);
/* The mutual-reachability tree (robust single linkage, the tree of DBSCAN* / HDBSCAN): the single-linkage tree above with every distance
 * replaced by w(x, y) = max(d(x, y), core(x), core(y)).  A row in a sparse region is pushed away from everything, so a bridge of a few
 * stray rows no longer joins two dense groups.  Cut at any R, the tree is DBSCAN* at radius R with min_pts = k + 1: one call answers for
 * every radius.
 * E, m and d(x, y) are exactly those of clip_amd_index_linkage.  0 <= k <= 1024.  core(x) for x in E: -INFINITY when k == 0; else entry
 * k - 1 of the distances clip_amd_index_search_ids(x, k, exclude_self = 1, allow = E) returns, bit for bit: the distance to the row's
 * k-th nearest other eligible row, +INFINITY when E holds fewer than k other rows.  w is the maximum of the three in f32; no operand is
 * ever a NaN, so it is exact and the order of its evaluation does not matter.  Edges are ordered by (w, lo, hi), lo < hi: a total order.
 * The result is the minimum spanning forest of the graph "w <= link" over E under that order: an edge belongs to it exactly when its
 * endpoints are not connected by strictly smaller edges.  weights receives w.  core ([size] f32, may be NULL) receives core(x) for x in
 * E and +INFINITY for every other row; it is written whenever size > 0, also when no edge is.
 * Output forms, capacities (size - 1), order and return values are those of clip_amd_index_linkage: the host form sorted by the edge
 * order, the device form unordered but byte-identical run to run, 0 when m <= 1.  +INFINITY weights are legal: they occur when E holds
 * at most k rows, are in the graph only at link == INFINITY and are then ordered by (lo, hi).
 * Consequences: k == 0 gives, byte for byte, the result of clip_amd_index_linkage.  A finite link gives a prefix of the whole tree.  Cut
 * at R, the rows with core <= R carry exactly the labels of clip_amd_index_components(R, allow = {x in E : core(x) <= R}) and every
 * other eligible row is a group of its own.  Results are bit-identical run to run, however rows were split across add calls, across
 * save / load and on both routes of the neighbour search (clip_amd_index_knn_graph's), and do not depend on the order of any atomic;
 * over E they are those of an index to which only the rows of E were ever added (ids mapped in order).
 * -1 / false with a message on stderr, nothing launched and no output written, for a NULL index, a NULL lo / hi / weights, a NaN link
 * or a k outside 0 ... 1024.
 * Host form: host arrays, synchronous on the ctx stream.  Device form: allow (trusted) and the outputs in HBM, asynchronous on the ctx
 * stream, synchronises with nothing on the host; the core distances never visit the host.  Device memory beyond the index: that of
 * clip_amd_index_linkage plus 4 bytes per row (padded to four rows) and the fixed workspace of clip_amd_index_knn_graph. */
int64_t clip_amd_index_linkage_core(struct clip_amd_index * ix, int k, float link, const uint64_t * allow, int64_t * lo, int64_t * hi,
                                    float * weights, float * core);
bool clip_amd_index_linkage_core_device(struct clip_amd_index * ix, int k, float link, const uint64_t * d_allow, int64_t * d_lo, int64_t * d_hi,
                                        float * d_weights, float * d_core, int64_t * d_count);
/* Average wall times (microseconds) over the rows of clip_amd_bench_modes, taken on one index in one run, the calls of an iteration one
 * after another: returns that of one clip_amd_index_linkage_core (host form, link = INFINITY, core wanted); < 0 on error.
 * clip_amd_bench_linkage_core_parts: parts [5] of the last call of it: clip_amd_index_knn_graph(k), clip_amd_index_linkage, the core
 * column alone (the neighbour search with its device-side sink), the rounds that did work in the mutual-reachability tree and in the
 * single-linkage tree.  clip_amd_test_index_linkage_rounds counts the rounds of clip_amd_index_linkage_core's host form as well.  Used by
 * scripts/linkage_core_bench.py. */
float clip_amd_bench_linkage_core(int dtype, int64_t n, int dim, int k, int copies, int iters);
void clip_amd_bench_linkage_core_parts(float * parts);
/* Extents of a labelling: given one label per row (from clip_amd_index_components, a cut of the linkage tree, clip_amd_index_modes, the
 * owner of clip_amd_index_spread, or anything else), how far every row's own group reaches from it, and for every group its minimax
 * centre, its radius and its diameter.  It tells a tight burst of copies from a chain whose two ends are far apart, and gives every
 * group a cover: the member from which the farthest other member is nearest.
 * E is the set of eligible rows (live and set in allow, layout as live_mask, NULL = every live row); for a pair {x, y} of E, d(x, y) is
 * the distance clip_amd_index_pairs reports for (min, max), the same bits from the same chain for every stored dtype.  A pair whose
 * distance is NaN is not a pair, as in pairs.  Every comparison is in f32 on those bits.
 * labels [size] int64.  Row x is a MEMBER when x is in E and labels[x] >= 0.  Every member's label must be < size (the labels of
 * components, modes, a tree cut and spread's owner are); the label need not be a member of its own group, or eligible.  G(x) is the set
 * of members that carry x's label.
 * reach [size] f32: the maximum of d(x, y) over y in G(x), y != x.  far [size] int64: the y that attains it, the lowest id among equals.
 * The only member of a group (and a member without a pair) gets reach 0 and far -1.
 * centre [size] int64: the member c of G(x) that minimises (reach[c], c).  radius [size] f32: reach[centre[x]].  diameter [size] f32: the
 * maximum of reach over G(x), which is the largest pairwise distance in the group.  These three are equal across a group; they are
 * written per row, so the output is O(size) and needs no table of groups.
 * A row that is not a member gets -1 for the ids and +INFINITY for the floats.  Every output but centre may be NULL.
 * The host form returns the number of groups with at least one member (0 for an empty index: nothing is written; -1 on error); the
 * device form writes it to d_count (int64, may be NULL).  Results are bit-identical run to run, however rows were split across add calls
 * and across save / load, and do not depend on the order of any atomic (every output is a maximum or minimum of integer keys; there is
 * no float sum); over E they are those of an index to which only the rows of E were ever added (ids and labels mapped in order).
 * -1 / false with a message on stderr, nothing launched and no output written, for a NULL index, labels or centre and, in the host form,
 * for a member whose label is >= size.
 * Host form: host arrays, synchronous on the ctx stream.  Device form: labels, allow (both trusted; a row whose label is >= size is
 * treated as not a member) and the outputs in HBM, asynchronous on the ctx stream, synchronises with nothing on the host.
 * Cost: one sweep over the tile pairs (128 x 128 rows) that can hold two rows of one group: a tile pair is skipped when the label ranges
 * of its two tiles do not intersect, so labels that follow the row order cost little more than the diagonal, and shuffled labels one
 * sweep over all pairs of members.  Device memory beyond the index: 24 bytes per row (the host form 36 more for the labels and its
 * results). */
int64_t clip_amd_index_extents(struct clip_amd_index * ix, const int64_t * labels, const uint64_t * allow, int64_t * centre, float * radius,
                               float * diameter, float * reach, int64_t * far);
bool clip_amd_index_extents_device(struct clip_amd_index * ix, const int64_t * d_labels, const uint64_t * d_allow, int64_t * d_centre,
                                   float * d_radius, float * d_diameter, float * d_reach, int64_t * d_far, int64_t * d_count);
/* Average wall time (microseconds) of one clip_amd_index_extents (host form, all five outputs) over n rows in bursts of group_size (a row
 * and group_size - 1 noisy copies, as clip_amd_bench_search_distinct plants them), row r labelled r / group_size; sorted == 0: row r
 * carries the label of row pi(r) instead, pi a fixed permutation, so the groups keep their sizes but lie scattered over the index;
 * < 0 on error.  Used by scripts/extents_bench.py. */
float clip_amd_bench_extents(int dtype, int64_t n, int dim, int group_size, int sorted, int iters);
/* Test hook: route 0 (the default) skips the tile pairs whose label ranges do not intersect, route 1 computes every tile pair of members;
 * the results are the same, bit for bit.  Returns the number of tile pairs the index's last clip_amd_index_extents call (either form; the
 * stream is waited for) computed, 0 before the first; -1 for a NULL index or another route.  Used by tests/. */
int64_t clip_amd_test_index_extents_route(struct clip_amd_index * ix, int route);
/* Farthest-first selection (greedy k-center): n_max rows that between them cover the index, each picked as the row farthest from
 * everything chosen before it.  Every prefix of the result is a 2-approximate k-center solution, and reach[t] is the coverage radius of
 * the prefix before position t, so one call gives the table of "how many rows" against "how far is everything else".
 * E is the set of eligible rows (live and set in allow, layout as live_mask, NULL = every live row); for a pair {x, y} of E, d(x, y) is
 * the distance clip_amd_index_pairs reports for (min, max), the same bits from the same chain.  Every comparison is in f32 on those bits.
 * seeds [n_seeds] (host ids in both forms): the first centres, in order; each must be in E and they must be distinct.  n_seeds == 0: the
 * first centre is the lowest id of E.  Then, while fewer than n_max centres are chosen and E holds a row that is not a centre: with
 * gap(x) = min d(c, x) over the centres so far, take the x of largest gap, the lowest id among equals; if gap(x) <= stop_radius the
 * traversal stops without it (stop_radius = -INFINITY never stops), else x is the next centre, at position t, with reach[t] = gap(x).
 * n_max above the size of E is fine: the traversal ends when every row of E is a centre.
 * centres [n_max] int64: the centres in pick order, -1 past the count.  reach [n_max] f32: +INFINITY for the seeds (and the automatic
 * first centre) and past the count, else the gap at which the centre was picked (non-increasing).  owner [size] int64 / owner_distance
 * [size] f32: the centre that minimises (d(c, x), position of c), so the earliest chosen among equals; a centre owns itself at exactly
 * 0; a row outside E gets -1 / +INFINITY.  cover_radius: one float, the maximum of owner_distance over E (0 when every row of E is a
 * centre).  Every output but centres may be NULL.
 * The host form returns the number of centres m (0: E is empty; only centres, reach and cover_radius are written); the device form writes
 * it to d_count (int64, may be NULL).  Results are bit-identical run to run, however rows were split across add calls and across save /
 * load, and do not depend on the order of any atomic; over E they are those of an index to which only the rows of E were ever added (ids
 * mapped in order).
 * -1 / false with a message on stderr, no output written, for a NULL index, NULL centres, a NaN stop_radius, n_max < 1, n_max < n_seeds, or
 * a seed that is out of range, removed, not allowed or repeated.
 * Host form: host arrays, synchronous on the ctx stream; it reads one slot back every 64 steps and stops queueing once the traversal
 * has ended.  Device form: allow (trusted) and the outputs in HBM, asynchronous on the ctx stream, all min(n_max, size) steps queued (a step
 * after the end exits at once); with seeds and a mask to test them against it waits once for the stream, before anything is written.
 * One launch per 16 seeds and one per further centre, each reading the eligible rows once.  Device memory beyond the index: 8 bytes per
 * row and 8 per centre (the host form 12 more of each for its results). */
int64_t clip_amd_index_spread(struct clip_amd_index * ix, int64_t n_max, float stop_radius, const int64_t * seeds, int64_t n_seeds,
                              const uint64_t * allow, int64_t * centres, float * reach, int64_t * owner, float * owner_distance,
                              float * cover_radius);
bool clip_amd_index_spread_device(struct clip_amd_index * ix, int64_t n_max, float stop_radius, const int64_t * seeds, int64_t n_seeds,
                                  const uint64_t * d_allow, int64_t * d_centres, float * d_reach, int64_t * d_owner,
                                  float * d_owner_distance, float * d_cover_radius, int64_t * d_count);
/* Device time (microseconds, HIP events) of one clip_amd_index_spread_device of n_max centres without seeds or stop radius, all outputs;
 * copies == 0: over the seeded rows of clip_amd_bench_range, copies > 0: over the groups of clip_amd_bench_search_distinct; < 0 on error.
 * Used by scripts/spread_bench.py. */
float clip_amd_bench_spread(int dtype, int64_t n, int dim, int64_t n_max, int copies, int iters);

/* ---- kernel-level test hooks (used by tests/ only; host pointers, synchronous) ----
 * Y[M,N] = X[M,K] . W[N,K]^T (+bias) through the production dequant-GEMM kernel.
 * w_raw is the tensor in its GGUF/ggml block layout (type: ggml type id 0,1,2,3,6,7,8).
 * epilogue: 0 plain f32 out, 1 f16 out (returned widened to f32), 2 gelu->f16, 3 quick-gelu->f16,
 *           4 residual: Y = resid + X.W^T + bias (f32).  tile: 0 auto, else BM*1000+BN.
 * This hook, clip_amd_test_gemm_ex, clip_amd_test_skinny and clip_amd_test_lnfold poison every buffer a kernel stores to before the launch
 * (f32: quiet NaN 0x7fc00000, fp16: 0x7e00; also the split-K workspace and the extra activation row M that clamped or prefetching reads may
 * touch), so an output element that no kernel wrote arrives in y as NaN, never as what an earlier call left in device memory.  Two guard
 * rows lie behind each output (poisoned too; behind the fold's fp16(x gamma) operand they are zero, as rows at and past M must be) and are
 * compared on the host after the launch.
 * Returns 0; -1 no device; -2 repack failed; -3 bad arguments; -4 HIP error; -5 (skinny / lnfold) combination not covered;
 * -6 a guard row changed: a kernel stored past row M - 1 (y is still returned). */
int clip_amd_test_gemm(int type, const void * w_raw, int64_t N, int64_t K, const float * x, int64_t M,
                       const float * bias, const float * resid, float * y, int epilogue, int tile);
/* Same, plus the two epilogue features the plain hook cannot reach: epilogue 1 with qcols / qscale (columns n < qcols
 * are multiplied by qscale AFTER the bias: the 1/sqrt(d_head) Q scale of the fused q/k/v projection, reference
 * clip.cpp:1363) and epilogue 5 = patch embedding (reference clip.cpp:1309-1331): GEMM row m -> output row
 * (m / Np) * T + 1 + m % Np with pos[1 + m % Np] added, no bias; y is [(M / Np) * T][N] and is uploaded first (over the poison, not over
 * the guard rows) so that untouched rows (the class-token rows) keep the caller's fill; pos is [T][N]. */
int clip_amd_test_gemm_ex(int type, const void * w_raw, int64_t N, int64_t K, const float * x, int64_t M,
                          const float * bias, const float * resid, float * y, int epilogue, int tile,
                          int qcols, float qscale, int Np, int T, const float * pos);
/* clip_amd_test_gemm_ex without epilogue 5, with the fp16 panel of a block-quantised weight supplied the way the layer chain supplies it, or withheld.
 * panel_mode = 1 (quantised types only): the panel of w_raw is built by ONE launch_dequant call of lead + 1 jobs, lead in 0..3 — jobs 0 .. lead - 1 are
 * further copies of the weight into panels of their own, the last job feeds the GEMM — and is passed as GemmParams::w16_pre; w16_scratch is NULL.  The
 * DevWeight given to launch_gemm is repacked from w_planes_raw when that is not NULL: a second weight of the same type and shape with other values.
 * By the contract of w16_pre (kernels.h) every kernel multiplies the panel, so y must be the product with w_raw whatever w_planes_raw holds.
 * panel_mode = 0 (lead = 0, w_planes_raw = NULL): neither w16_pre nor w16_scratch; for a panel tile code and a quantised weight launch_gemm must fall
 * back to the fused 4-wave kernel.
 * Checked on the host before the device is looked for: pointers, N, K, M >= 1, epilogue in 0..4 (4 needs resid), tile >= 0, 0 <= qcols <= N, type f16 or
 * block-quantised, panel_mode / lead / type as above.  Poison, guard rows and return codes as for clip_amd_test_gemm. */
int clip_amd_test_gemm_panel(int type, const void * w_raw, const void * w_planes_raw, int64_t N, int64_t K, const float * x, int64_t M,
                             const float * bias, const float * resid, float * y, int epilogue, int tile, int qcols, float qscale,
                             int panel_mode, int lead);
/* launch_dequant (k_gemm8.hip) as dequant_layer of forward.cpp calls it: n <= 8 weights (types[i], w_raw[i], N[i] x K[i]; f16 or block-quantised), each
 * through the production repack; ONE device buffer holds the n fp16 panels [Npad_i][Kpad_i] back to back in the caller's order (Npad = N rounded up to
 * 128, Kpad = K rounded up to 64), with 4096 guard halfs before the first and behind the last; all of it is poisoned with 0x7e00, then ONE
 * launch_dequant(ws, outs, n) runs.  panels_out[i] receives panel i whole (Npad_i * Kpad_i raw fp16 bits).  An f16 entry is legal: launch_dequant
 * skips it and its panel comes back all poison.  *guard_ok (may be NULL) = 1 when the guard halfs still hold the poison, else 0 and the return code
 * is -6.  Returns 0; -1 no device; -2 repack failed; -3 bad arguments (checked before the device is looked for); -4 HIP error; -6. */
int clip_amd_test_dequant_panels(int n, const int * types, const void * const * w_raw, const int64_t * N, const int64_t * K,
                                 uint16_t * const * panels_out, int * guard_ok);
/* ONE launch_fold_vectors (k_fold.hip): c_out[n] = sum_k gamma[k] W[n][k], b_out[n] = sum_k beta[k] W[n][k] + bias[n] (bias may be NULL: no bias),
 * W [N][K] of ggml type `type` (f16 or block-quantised) as the GEMM kernels dequantise it.  c and b' are device buffers of N + 64 floats, poisoned; the
 * 64 floats behind each are compared after the launch (-6).  Return codes as for clip_amd_test_dequant_panels. */
int clip_amd_test_fold_vectors(int type, const void * w_raw, int64_t N, int64_t K, const float * gamma, const float * beta, const float * bias,
                               float * c_out, float * b_out);
/* The GEMM of an f32 file (k_gemm_f32.hip) in the form the layers run it. w is f32 [N][K] (ggml type 0), x f32 [M][K]; bias [N] and resid [M][N] may be
 * NULL (resid is required by epilogue 4); epilogue, qcols / qscale, Np / T / pos as for clip_amd_test_gemm_ex.
 * act_f32 = 1: the activations go up as f32 rows [M][Kpad] (exactly M rows, columns K .. Kpad - 1 zero), GemmParams::act_f32 is set, and epilogues 1-3
 * come back as the f32 values the kernel stores, with no fp16 step.  act_f32 = 0: x is rounded to fp16 and epilogues 1-3 store fp16 (returned widened),
 * as clip_amd_test_gemm_ex does.  Epilogue 4 adds into the residual rows in place (resid and out are one buffer, as in the layers).
 * y is in and out: [M + guard_rows][N], for epilogue 5 [(M / Np) * T + guard_rows][N].  It is uploaded before the launch and all of it is downloaded,
 * so a row the kernel must not write (the guard rows, the class-token rows of epilogue 5) comes back with the caller's fill (with act_f32 = 0 and
 * epilogues 1-3 through fp16: use a fill that fp16 holds exactly).
 * Checked on the host before the device is looked for: N % 4 == 0 and qcols % 4 == 0 (the epilogues work on groups of 4 columns; the loader holds a
 * model to the same multiple and to no coarser one), 0 <= qcols <= N, epilogue in 0..5, act_f32 in {0, 1}, epilogue 5 only with act_f32 = 0 (the patch GEMM
 * always reads fp16 im2col rows) and with Np >= 1, T >= Np + 1, M % Np == 0 and pos, 0 <= guard_rows <= 1024.
 * Returns 0; -1 no device; -2 repack failed; -3 a check failed (nothing launched, y untouched); -4 HIP error. */
int clip_amd_test_gemm_f32(const void * w, int64_t N, int64_t K, const float * x, int64_t M, const float * bias, const float * resid, int epilogue,
                           int qcols, float qscale, int Np, int T, const float * pos, int act_f32, int guard_rows, float * y /* in and out */);
/* LayerNorm fold A/B (the LayerNorm launches of reference clip.cpp:1350-1355,1400-1405 folded into the GEMM epilogues around them):
 *   x1 = resid + a . W1^T + b1                       [M][h]   W1: [h][K1]  (residual epilogue)
 *   y  = epi2( LN(x1; gamma, beta, eps) . W2^T + b2 )  [M][N2]  W2: [N2][h]  (epi2: 1 f16 (+ qcols / qscale), 2 gelu, 3 quick-gelu)
 * fold = 0: three launches (GEMM, LayerNorm kernel, GEMM); fold = 1: two launches — the residual epilogue also writes fp16(x1 gamma) and
 * partial row statistics, the second GEMM's epilogue applies rstd (acc - mean c) + b'.  tile1 / tile2 as `tile` of clip_amd_test_gemm.
 * x1_out [M][h] f32, y_out [M][N2] (fp16 widened).  h % 64 == 0.  tile1 < 0: both GEMMs on the small-M kernels (k_skinny.hip, M <= 128; fold = 0
 * is then the LayerNorm fused on the operand, fold = 1 the folded form).  fold = 2: the folded form with the operand CENTRED (the default of
 * the layer chain since round 4): fp16((x1 - mu) gamma) with mu_m = the mean of row m of `resid` (what the previous LayerNorm's consumer
 * leaves), and rstd (acc - (mean - mu) c) + b' in the consumer.  Poison, guard rows and return codes as for clip_amd_test_gemm; the statistics
 * buffer between the two launches and the consumer's mu_out are poisoned too: a slot that a consumer reads and no producer wrote is a NaN in y. */
int clip_amd_test_lnfold(int type, const void * w1_raw, int64_t h, int64_t K1, const void * w2_raw, int64_t N2, const float * a, int64_t M,
                         const float * b1, const float * resid, const float * gamma, const float * beta, float eps, const float * b2,
                         int epi2, int tile1, int tile2, int fold, int qcols, float qscale, float * x1_out, float * y_out);
/* The two halves of the fold on their own, so that what passes between them — the operand, the partial statistics, the row means — is seen, not only y.
 * Producer: ONE EPI_RESID_F32 launch with xg_out set.  x1 = resid + a . W^T + b1 ([M][h], W [h][K1] of ggml type `type`, f16 or block-quantised),
 * xg = fp16((x1 - xg_mu_m) gamma_next) as raw bits [M][ldxg] (xg_mu NULL: the uncentred form; ldxg >= h, a multiple of 8: the columns past h are
 * never written and come back as the poison 0x7e00), and the WHOLE statistics buffer [h / slotw][st_stride][2] f32, st_stride = M rounded up to 64
 * (rows M .. st_stride - 1 must still hold the poison 0x7fc00000), with *slotw_out = the slot width the launch used: gemm_fold_slotw(tile), 16 for the
 * small-M kernel.  stats_out must hold (h / 16) * st_stride * 2 floats.  tile1: as `tile` of clip_amd_test_gemm (launch_gemm with stats_out /
 * stats_stride), -1 = launch_skinny (fstats_out / fstride_out; M <= 128).  Guard rows: two behind x1 and xg; the device
 * statistics buffer holds h / 16 + 1 slots, and all of it behind the h / slotw slots of this launch is guard.
 * Consumer: ONE launch with ln_c set on an operand and statistics of the caller's making.  y = epi2(q (rstd_m (xg . W^T - (mean_m - ln_mu_m) c) + b_fold))
 * ([M][N2] fp16, widened; W [N2][h]; epi2, qcols / qscale as for clip_amd_test_lnfold; ln_mu may be NULL), (mean_m, rstd_m) merged by the kernel from
 * stats [slots][st_stride][2] (slots * slotw == h; rows >= M are uploaded as given and must not matter).  The operand's rows at and past M are zero.
 * mu_out [st_stride] is poisoned before the launch and comes back whole: rows < M hold the kernel's row means, the rest the poison; 64 guard floats
 * lie behind it.  tile2: as tile1; a panel scratch is provided, so the panel tile codes reach their kernels.
 * Checked on the host before the device is looked for (-3, nothing written): pointers, h % 64 == 0, sizes >= 1, type f16 or block-quantised, tile >= -1,
 * M <= 128 with tile -1, the whole-rounds codes 258 / 260 only where they do not split; producer: ldxg; consumer: N2 % 4 == 0, epi2 in 1..3,
 * 0 <= qcols <= N2 and qcols % 4 == 0, slots * slotw == h, an even slot count with slotw == 32, at most 32 merge units (slots, or pairs of 32-column
 * slots) unless tile2 == -1.  Other return codes as for clip_amd_test_gemm (-5: skinny_supported refuses). */
int clip_amd_test_fold_producer(int type, const void * w_raw, int64_t h, int64_t K1, const float * a, int64_t M, const float * b1, const float * resid,
                                const float * gamma_next, const float * xg_mu, int tile1, int64_t ldxg, float * x1_out, uint16_t * xg_out,
                                float * stats_out, int * slotw_out);
int clip_amd_test_fold_consumer(int type, const void * w_raw, int64_t N2, int64_t h, const uint16_t * xg, int64_t M, const float * stats, int slots,
                                int slotw, const float * ln_mu, const float * c, const float * b_fold, float eps, int epi2, int qcols, float qscale,
                                int tile2, float * y_out, float * mu_out);
/* The tile the heuristic of launch_gemm picks for an [M][K] x [N][K]^T problem (pure host arithmetic, no device needed):
 * BM * 1000 + BN; BM = 65: the mid-M ring kernel on 64-row tiles (k_gemm_ring.hip), BN = 256 / 258-260: the large-M panel kernels,
 * BN = 257: the 256-column tiles of the fused-dequant kernel (128257 / 160257, csrc/gemm_wide.h). */
int clip_amd_test_gemm_tile(int64_t M, int64_t N, int64_t K, int quantised);
int clip_amd_test_gemm_tile_ex(int64_t M, int64_t N, int64_t K, int quantised, int shared_device);   /* ... with clip_amd_set_device_shared's flag */
/* The state a context keeps between calls, read-only (fields are read; no HIP call, so a host-only context answers too).  which: 0 the vision
 * tower, 1 the text tower.  head[5], in this order: the resident-panel mask of that tower (bit i: weight i of every layer has a resident fp16
 * panel; 0 q/k/v, 1 out-projection, 2 FFN-up, 3 FFN-down), the number of entries of its panel table (4 x layers on a context with a device,
 * 0 on a host-only one), the number of vision graph entries that hold an instantiated graph, the same for the text graphs, the bytes of the
 * activation workspace.  panels: the first min(panels_cap, entries) table entries as integers — entry 4 * layer + i is the device address of
 * that panel, 0 where there is none; may be NULL with panels_cap == 0.  Returns the number of table entries, or -3 (nothing written): ctx or
 * head NULL, which outside {0, 1}, panels_cap < 0, panels NULL with panels_cap > 0. */
int clip_amd_test_ctx_state(struct clip_ctx * ctx, int which, int64_t * head, uint64_t * panels, int panels_cap);
/* The layout of a tower pass's activation buffers in the workspace (forward.cpp carve_tower; pure host arithmetic, no context, no device) for rows token
 * rows of nseq sequences, hidden width h, FFN width ff, projection proj, f32 != 0: float activations (f32 file), col_halfs: elements of the vision
 * tower's im2col matrix (0: none), alias: the value of CLIP_AMD_WS_ALIAS.  off / bytes [min(cap, 15)]: byte offset from the 256-byte aligned start
 * and size of, in this order, stats, mu, x, xn, qkv, att, mid, col, pooled, emb, xp, ap, xnp, midp and the region that qkv, att, mid and col
 * share when alias != 0 (size 0 otherwise, as for col when col_halfs == 0).  total, if not NULL: the end of the last buffer.  With CLIP_AMD_GUARD=1
 * in the environment the offsets include the canary blocks.  Returns 15, or -3 (nothing written) on arguments no tower can have. */
int clip_amd_test_tower_plan(int64_t rows, int nseq, int h, int ff, int proj, int f32, int64_t col_halfs, int alias, int64_t * off, int64_t * bytes, int cap,
                             int64_t * total);
/* Average device time (microseconds, HIP events) of one GEMM shape through the production kernel on random
 * weights of ggml type `type`; < 0 on error.  Used by scripts/gemm_bench.py for kernel A/B work. */
float clip_amd_bench_gemm(int type, int64_t N, int64_t K, int64_t M, int epilogue, int tile, int iters);
/* Small-M kernel (one image / one text: the layers use it up to 64 rows, the hook up to 512; k_skinny.hip): y[M][N] = epilogue(A . W^T + bias) with A = fp16(x), or — ln_w
 * != NULL — A = LayerNorm(x) fused into the kernel.  epilogue 0 f32, 1 f16 (+ qcols / qscale), 2 gelu, 3 quick-gelu, 4 residual
 * (stats_out, if not NULL, receives the [128 rows][128 slots][2] partial row statistics the epilogue leaves for the next LayerNorm:
 * slot j of a row = its (sum, sum of squares) over output columns 16 j .. 16 j + 15).
 * Returns -5 when the combination is not covered by this path; poison, guard rows and the other return codes as for clip_amd_test_gemm. */
int clip_amd_test_skinny(int type, const void * w_raw, int64_t N, int64_t K, const float * x, int64_t M, const float * bias,
                         const float * resid, const float * ln_w, const float * ln_b, float eps, float * y, int epilogue,
                         int qcols, float qscale, float * stats_out);
/* y = LayerNorm(x)*w + b, rows x h. out_f16 != 0 rounds the result through fp16. */
int clip_amd_test_layernorm(const float * x, const float * w, const float * b, float eps, int64_t rows, int64_t h,
                            float * y, int out_f16);
/* The general form: row r reads x[in_rows[r]] (in_rows != NULL) or x[r * in_row_mul] of x [x_rows][ldx]; out16 (raw fp16 bits, [rows][ld16]) and
 * out32 ([rows][ld32]), either may be NULL, come out of ONE launch.  Both are filled with a poison pattern first (f32: quiet NaN, fp16: 0x7e00):
 * whatever the kernel does not write, the padding ld > h included, still holds it.  -3: bad arguments. */
int clip_amd_test_layernorm_ex(const float * x, int64_t x_rows, int ldx, const int32_t * in_rows, int in_row_mul, const float * w, const float * b,
                               float eps, int rows, int h, uint16_t * out16, int ld16, float * out32, int ld32);
/* Text embedding (launch_text_embed): x[r] = dequant(tok_raw[ids[r]]) + pos[r - start of r's sequence], tok_raw a table of ggml type `type`
 * (tok_bytes bytes), seq_start [nseq + 1] ascending from 0 to rows, pos [n_pos][h].  gamma_next != NULL: also the fold entry, xg [rows][ldxg] raw fp16
 * bits, stats [rows][2] = (sum, sum of squared deviations), and with centred != 0 mu [rows].  All outputs are poisoned first as above. */
int clip_amd_test_text_embed(int type, const void * tok_raw, int64_t tok_bytes, int h, const int32_t * ids, const int32_t * seq_start, int nseq, int rows,
                             const float * pos, int n_pos, const float * gamma_next, int centred, float * x, uint16_t * xg, int ldxg, float * stats,
                             float * mu);
/* im2col of the patch convolution (launch_im2col): imgs [B][S][S][3] f32 -> col [B (S/P)^2][Kpad] raw fp16 bits (poisoned first).  imgs_f16 != 0: the
 * images are first rounded to fp16 on the device (launch_f32_to_f16) and the fp16-input kernel runs. */
int clip_amd_test_im2col(const float * imgs, int imgs_f16, int B, int S, int P, int Kpad, uint16_t * col);
/* Entry of the folded layer chain with the pre-LayerNorm (launch_layernorm_prep): y = LayerNorm(x) w + b (w == b == NULL: y = x) -> out32 [rows][ld32];
 * xg, stats, mu of y as for clip_amd_test_text_embed (gamma_next required).  class_embd / pos0 != NULL: rows r % T == 0 are class_embd + pos0 and are
 * never read from x.  in_place != 0: out32 aliases x on the device (ld32 := ldx) and returns the x buffer as the launch left it; else out32 is poisoned first. */
int clip_amd_test_layernorm_prep(const float * x, int ldx, const float * w, const float * b, float eps, int rows, int h, const float * gamma_next,
                                 int centred, const float * class_embd, const float * pos0, int T, int in_place, float * out32, int ld32,
                                 uint16_t * xg, int ldxg, float * stats, float * mu);
/* The small row kernels, one launch each; outputs are poisoned first unless stated.
 *   op 0 cls_rows:   in0 class_embd [h], in1 pos [h]; n0 = B, n1 = T, n2 = h; out0 = x [B T][h] f32, uploaded first (in / out)
 *   op 1 gather_rows: in0 x f32 [n3][h], in1 a fp16 [n3][h] or NULL, idx = in_rows [rows] or NULL; n0 = rows, n1 = in_row_mul, n2 = h;
 *                    out0 = xp f32 [rows][h], out1 = ap fp16 [rows][h]
 *   op 2 l2norm:     in0 v [rows][n]; n0 = rows, n1 = n, n2 = normalize; out0 [rows][n] f32
 *   op 3 row_stats:  in0 x [rows][ldx]; n0 = rows, n1 = h, n2 = ldx; out0 [rows][128][2] f32 (slot 0 := (sum, sum of squares))
 *   op 4 f32_to_f16: in0 [rows][lds] f32; n0 = rows, n1 = cols, n2 = cols_pad, n3 = lds, n4 = ldd; out0 [rows][ldd] fp16
 *   op 5 f16_to_f32: in0 [rows][lds] fp16; n0 = rows, n1 = cols, n3 = lds, n4 = ldd; out0 [rows][ldd] f32 */
int clip_amd_test_rows(int op, const void * in0, const void * in1, const int32_t * idx, int64_t n0, int64_t n1, int64_t n2, int64_t n3, int64_t n4,
                       void * out0, void * out1);
/* The JPEG decoder's stages.  plan: runs the entropy stage on the host and says where the pixel stage may run; needs no device.  Returns 1 for a
 * decodable JPEG, else 0.  info[16]: route (0 host, 1 device), width, height, number of components, progressive, colour rule (0 grey,
 * 1 YCbCr, 2 stored RGB, 3 CMYK, 4 YCCK, 5 YCbCr + ignored channel), every scan complete, then (h, v) sampling factors per component. */
int clip_amd_test_jpeg_plan(const uint8_t * data, size_t size, int * info);
/* JPEGs whose pixel half clip_amd_image_batch_encode_files / _memory have run on the device since the process started (the rows do not tell). */
long long clip_amd_test_jpeg_device_count(void);
/* decode_device: the entropy stage, then jpeg_idct_kernel and jpeg_rgb_kernel, then the [ny][nx][3] block copied into rgb (cap bytes).
 * 0 ok; -1 no device; -2 not a JPEG, or one that is planned "host": refused, no kernel runs; -3 bad arguments / cap too small;
 * -4 kernel error; -5 a byte behind the pixels was written. */
int clip_amd_test_jpeg_decode_device(const uint8_t * data, size_t size, uint8_t * rgb, size_t cap, int * nx, int * ny);
/* Median HIP-event times (ms[0] jpeg_idct_kernel, ms[1] jpeg_rgb_kernel) over reps runs on `copies` copies of one device-planned JPEG, and
 * the bytes each kernel must move per run (bytes[0], bytes[1]).  Return codes as above.  Used by scripts/files_bench.py. */
int clip_amd_bench_jpeg_kernels(const uint8_t * data, size_t size, int copies, int reps, float * ms, double * bytes);
/* Multi-head attention over nseq sequences of length T each: qkv [nseq*T][3h] (q pre-scaled), out [nseq*T][h]. */
int clip_amd_test_attention(const float * qkv, int nseq, int T, int h, int n_head, int causal, float * out);
/* ... with the kernel chosen: 0 = automatic (what the layers run), 1 = the whole-row kernel (d_head 64: T <= 592, other head sizes:
 * T <= 288), 2 = the streaming kernel (any T).  Returns -2 when the chosen kernel does not take the shape. */
int clip_amd_test_attention_ex(const float * qkv, int nseq, int T, int h, int n_head, int causal, float * out, int kernel);
/* Ragged batches: qkv [rows_total][3h] (q pre-scaled), seq_start[nseq + 1] row offsets (uploaded to the device as the layers pass them), max_len the
 * launch's key bound (>= every length; it may be larger than the longest sequence).  Rows before seq_start[0] and from seq_start[nseq] on are guard
 * rows no kernel may read or write.  seq_start == NULL: nseq sequences of max_len rows each, from row 0.  kernel: 0 = automatic, 1 = whole-row,
 * 2 = streaming (these three on fp16 copies of qkv and out), 3 = the f32 kernel (qkv and out stay f32 end to end).  out [rows_total][h] is in and
 * out: it is uploaded before the launch and downloaded after it, so a row that no kernel wrote comes back with the caller's value.
 * Checked on the host before anything launches: nseq >= 1, 0 <= seq_start[0], seq_start[nseq] <= rows_total, offsets non-decreasing, every length in
 * [1, max_len] (the kernels clamp to row len - 1: an empty sequence is outside their contract), h % n_head == 0.
 * Returns 0; -1 no device; -2 the chosen kernel does not take the shape; -3 a check failed (nothing launched, out untouched); -4 HIP error. */
int clip_amd_test_attention_ragged(const float * qkv, int64_t rows_total, const int32_t * seq_start, int nseq, int max_len,
                                   int h, int n_head, int causal, float * out /* in and out */, int kernel);
/* Average device time (microseconds, HIP events) of one attention launch on seeded random q / k / v, kernel as
 * clip_amd_test_attention_ex; < 0 on error (-2: the kernel does not take the shape).  Used by scripts/attn_bench.py. */
float clip_amd_bench_attention(int nseq, int T, int h, int n_head, int causal, int kernel, int iters);

#ifdef __cplusplus
}
#endif

#endif /* CLIP_AMD_H */
