/*
 * sr_hip.h -- C ABI of the MI355X-native tile -> blend -> assess engine (libsrhip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / numpy types.  Each entry
 * point names the reference interface it replaces (paths relative to the reference repo).
 * Host-side mirrors of the reference's Python classes (tiling_module.TilingModule,
 * blending_module.BlendingModule, quality_assessment_module.QualityAssessmentModule,
 * main.SuperResolutionPipeline) bind these through ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - every function returns an int status (SR_OK == 0, negative = error); the message of the
 *    last error on the calling thread is sr_last_error().
 *  - "d_" pointers are device (HBM) addresses on the context's GPU, "h_" pointers are host.
 *    Small descriptor arrays (tile rectangles etc.) are always host pointers.
 *  - images are row-major, channel-interleaved (HWC) exactly like the reference's ndarrays;
 *    strides are in BYTES.
 *  - all device work is enqueued on the context's stream (sr_ctx_create makes one;
 *    sr_ctx_create_on_stream adopts the caller's, e.g. torch's current stream).  Functions
 *    that return a value to the host synchronise that stream; the others do not.
 *  - a context may be used from several threads: calls on one context are serialised by an
 *    internal mutex (the reference's ParallelBlender calls laplacian_fusion from a thread
 *    pool on one object, blending_module.py:1668-1701).
 *  - the library never keeps a host pointer after a call returns.
 */
#ifndef SR_HIP_H
#define SR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR_API __attribute__((visibility("default")))

enum sr_status {
    SR_OK = 0,
    SR_ERR_INVALID_ARG = -1, /* -> ValueError in the Python mirror                    */
    SR_ERR_SHAPE = -2,       /* shape / size mismatch (cv2.error in the reference)    */
    SR_ERR_OOM = -3,         /* a failed device allocation, from every entry point    */
    SR_ERR_HIP = -4,         /* any HIP runtime failure, incl. "no device"            */
    SR_ERR_COMM = -5,
    SR_ERR_UNSUPPORTED = -6
};

/* tiling_module.PaddingMode (tiling_module.py:40-45) */
enum sr_pad_mode { SR_PAD_MIRROR = 0, SR_PAD_REPLICATE = 1, SR_PAD_REFLECT = 2, SR_PAD_CONSTANT = 3 };
/* blending_module.WeightType (blending_module.py:52-56) */
enum sr_weight_type { SR_W_LINEAR = 0, SR_W_COSINE = 1, SR_W_SIGMOID = 2,
                      /* every weight 1: what BlendingModule.feather_blend's distance-transform weights evaluate to
                       * (blending_module.py:1313-1337: cv2.distanceTransform of an all-ones mask; see sr_weighted_blend) */
                      SR_W_ONES = 3 };
/* calculate_ssim branches (quality_assessment_module.py:365-417) */
enum sr_ssim_mode { SR_SSIM_UNIFORM7 = 0, SR_SSIM_GAUSS11 = 1, SR_SSIM_SIMPLE = 2 };
enum sr_dtype { SR_U8 = 0, SR_F32 = 1, SR_F64 = 2 };   /* SR_F64: sr_ssim_float only */

typedef struct sr_ctx sr_ctx;
typedef struct sr_blend_plan sr_blend_plan;

/* ---- library / context ------------------------------------------------------------- */
SR_API int sr_version(void);
/* first 16 hex digits of the sha1 over the sources the library was built from (a stale binary shows here) */
SR_API const char *sr_source_digest(void);
SR_API const char *sr_last_error(void);
SR_API int sr_device_count(int *count);
SR_API int sr_ctx_create(int device_id, sr_ctx **out);
SR_API int sr_ctx_create_on_stream(int device_id, void *hip_stream, sr_ctx **out);
SR_API int sr_ctx_destroy(sr_ctx *ctx);
SR_API int sr_ctx_sync(sr_ctx *ctx);
/* compute units of the context's device: what the launch-shape rules (the march's segment length among them) are sized by */
SR_API int sr_ctx_num_cu(sr_ctx *ctx, int *num_cu);

/* device memory helpers, so a host language needs no HIP binding of its own */
SR_API int sr_dev_alloc(sr_ctx *ctx, size_t bytes, void **d_ptr);
SR_API int sr_dev_free(sr_ctx *ctx, void *d_ptr);
SR_API int sr_memcpy_h2d(sr_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
SR_API int sr_memcpy_d2h(sr_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
SR_API int sr_memcpy_d2d(sr_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
SR_API int sr_memset_d(sr_ctx *ctx, void *d_dst, int value, size_t bytes);

/* per-kernel HIP-event timing on the context's stream (bench.py's roofline leg).
 * sr_prof_get: copies up to cap records; name is the kernel family, ms the summed time,
 * launches the number of launches since the last sr_prof_reset. */
typedef struct sr_prof_record {
    char name[48];
    double ms;
    int64_t launches;
} sr_prof_record;
SR_API int sr_prof_enable(sr_ctx *ctx, int on);
/* Restricts the timing to one kernel family (NULL or "": all families).  Every timed family costs two event
 * records per call, which serialise neighbouring kernels: bench.py times only the dominant kernel in its timed
 * region and all families in a separate pass. */
SR_API int sr_prof_select(sr_ctx *ctx, const char *name);
SR_API int sr_prof_reset(sr_ctx *ctx);
SR_API int sr_prof_get(sr_ctx *ctx, sr_prof_record *h_records, int cap, int *n);

/* ---- host-only bookkeeping (bit-exact integer restatements; no GPU needed) ----------- */
/* TilingModule._calculate_tile_positions (tiling_module.py:572-608).
 * h_xywh receives n_tiles x (x, y, w, h), row-major over the grid; *n_tiles is always set,
 * SR_ERR_SHAPE if cap is too small. */
SR_API int sr_tile_plan(int image_w, int image_h, int block_size, int overlap_px, int *n_tiles,
                        int *h_xywh, int cap);
/* TilingModule._calculate_overlap_for_tile (tiling_module.py:610-646): -> top,bottom,left,right */
SR_API int sr_tile_overlaps(int x, int y, int w, int h, int image_w, int image_h, int block_size,
                            int overlap_px, int *h_tblr);
/* TilingModule._build_neighbor_relationships (tiling_module.py:786-823):
 * h_nbr receives n x (top, bottom, left, right) tile indices, -1 where absent. */
SR_API int sr_tile_neighbors(const int *h_xywh, int n, int block_size, int overlap_px, int *h_nbr);
/* SuperResolutionPipeline._calculate_target_size presets (main.py:168-184); preset_mp in
 * {100,150,200}. */
SR_API int sr_target_size(int width, int height, int preset_mp, int *out_w, int *out_h);
/* BlendingModule._create_distance_weight_map (blending_module.py:529-561) tabulated by integer
 * edge distance d = 0..fw: W[y][x] = lut[min(d(y,x), fw)].  h_lut holds fw+1 floats. */
SR_API int sr_weight_lut(int fw, int weight_type, float *h_lut);

/* ---- tile extract (tiling_module.py:713-724 slice + _apply_padding :522-570) ---------- */
/* Copies n tiles out of one HWC u8 image into n contiguous block x block x cn tiles, padding
 * the bottom/right of edge tiles with the reference's border rule. */
SR_API int sr_tile_extract_pad(sr_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, int cn,
                               int64_t img_stride, const int *h_xywh, int n, int block_size,
                               int pad_mode, uint8_t *d_tiles);
/* TilingModule.split_image's complexity_score = np.std(cv2.cvtColor(tile, COLOR_BGR2GRAY)) (tiling_module.py:746-749) for
 * n RGB u8 tiles of h x w that live in HBM, tile i at d_tiles + i * tile_bytes: h_sums[2 i], h_sums[2 i + 1] receive the exact
 * sums of gray and gray^2 (swap_rb != 0: the reference's BGR constants on RGB data).  No pixel leaves the GPU. */
SR_API int sr_gray_moments_u8(sr_ctx *ctx, const uint8_t *d_tiles, int n, int64_t tile_bytes, int64_t stride, int h, int w,
                              int gray_shift, int swap_rb, uint64_t *h_sums);
/* Plain overlap-tile extract (no padding): tile i = img[y:y+h, x:x+w] into d_tiles[i] with row
 * stride tile_strides[i]; used by the benchmark's output-space tile stage. */
SR_API int sr_tile_extract(sr_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, int cn,
                           int64_t img_stride, const int *h_xywh, int n, void *const *h_d_tiles,
                           const int64_t *h_tile_strides);

/* ---- pyramid primitives (BlendingModule.build_gaussian_pyramid :217-269 -> cv2.pyrDown;
 *      build_laplacian_pyramid / collapse :271-363 -> cv2.pyrUp), fp32 HWC, dense ------- */
SR_API int sr_pyr_down(sr_ctx *ctx, const float *d_src, int h, int w, int cn, float *d_dst);
SR_API int sr_pyr_up(sr_ctx *ctx, const float *d_src, int hs, int ws, int cn, float *d_dst, int hd,
                     int wd);
/* d_out = d_a - pyrUp(d_b) (one Laplacian level) and d_out = pyrUp(d_b) + d_a (one collapse step) */
SR_API int sr_pyr_up_sub(sr_ctx *ctx, const float *d_a, int h, int w, int cn, const float *d_b,
                         float *d_out);
SR_API int sr_pyr_up_add(sr_ctx *ctx, const float *d_a, int h, int w, int cn, const float *d_b,
                         float *d_out);

/* ---- blends (BlendingModule.laplacian_fusion :369-506, weighted_average_fusion :661-760) */
typedef struct sr_tile_rect {
    int x, y; /* canvas position of the tile's top-left pixel (TileInfo.x, TileInfo.y) */
    int w, h; /* tile size in pixels                                                   */
} sr_tile_rect;

/* A plan owns the device workspace (per-tile Gaussian / collapsed pyramids, weight pyramids and
 * descriptor tables) for one tile arrangement.  Only canvas rows [row_begin, row_end) are
 * produced (0, canvas_h for the whole image): a strip owner in the multi-GPU blend gets
 * bit-identical rows because every pyramid value it needs is computed from the same inputs in
 * the same order. */
SR_API int sr_blend_plan_create(sr_ctx *ctx, const sr_tile_rect *h_tiles, int n, int cn, int canvas_h,
                                int canvas_w, int levels, int weight_type, int row_begin,
                                int row_end, sr_blend_plan **out);
SR_API int sr_blend_plan_destroy(sr_blend_plan *plan);
/* Host-only form of the window planner (no context, no GPU): for canvas rows [row_begin,row_end)
 * writes n x (r0, r1) = the tile-local input rows each tile must supply (r0 >= r1: tile unused).
 * The multi-GPU exchange plan is built from this on every rank. */
SR_API int sr_strip_tile_rows(const sr_tile_rect *h_tiles, int n, int levels, int canvas_h,
                              int row_begin, int row_end, int *h_rows);
/* Analytic worst case of that back-propagation (host only): a strip reads at most *below input rows before and *above
 * rows after its own rows of a tile (levels of >= 8 rows; 6 levels: 155 / 125). */
SR_API int sr_pyramid_halo(int levels, int *below, int *above);
/* Multi-GPU planning for a non-Python host (host only, deterministic, identical on every rank).
 * sr_strip_bounds: world + 1 even row boundaries of horizontal canvas strips of equal work (assessment + gather of the
 * strip's rows, pyramids of its rows plus the sr_pyramid_halo recompute).  sr_exchange_plan: the same bounds, per rank the
 * canvas rows it blends h_rows[2 r .. 2 r + 1] (strip + metric_halo rows for the SSIM windows), the tile-local rows it
 * needs of every tile h_need[(r * n + t) * 2 ..] (empty: [0, 0)) and an owner per tile.  Rank o sends rank r the rows
 * h_need[r][t] of every tile t it owns (one grouped batch of point-to-point transfers; in the order (r, t) on the sender
 * and (owner, t) on the receiver); the strip owner then calls sr_blend_plan_create(..., row_begin, row_end) with virtual
 * tile base pointers.  Policies: balanced = greedy minimisation of the busiest rank-to-rank link (xGMI is point-to-point). */
enum sr_owner_policy { SR_OWNER_BALANCED = 0, SR_OWNER_ROUNDROBIN = 1, SR_OWNER_LOCALITY = 2 };
SR_API int sr_strip_bounds(const sr_tile_rect *h_tiles, int n, int levels, int canvas_h, int canvas_w, int world,
                           int *h_bounds);
SR_API int sr_exchange_plan(const sr_tile_rect *h_tiles, int n, int cn, int levels, int canvas_h, int canvas_w, int world,
                            int metric_halo, int owner_policy, int *h_bounds, int *h_rows, int *h_need, int *h_owner);
/* The transfers (csrc/sr_comm.cpp).  SURVEY 8(b) planned sr_comm_init + a sharded blend: one process per GPU, RCCL over
 * xGMI.  No reference counterpart.  librccl.so is bound at run time (the copy the process already holds -- PyTorch's --
 * else ROCm's; SR_RCCL_LIB overrides); without it these return SR_ERR_UNSUPPORTED, RCCL failures are SR_ERR_COMM.
 *   rank 0: sr_comm_unique_id(id) -> the host ships the 128 bytes to every rank (MPI, a socket, a file) ->
 *   every rank: sr_comm_init(ctx, id, world, rank, &comm)  [collective: ncclCommInitRank on ctx's device]
 *   per image: sr_exchange_plan(...) once per geometry, then sr_comm_exchange_tile_rows(...) on ctx's stream, then
 *   sr_blend_plan_create(row_begin, row_end) + the blend + metrics on the strip, sr_comm_allreduce_f64 of the 4 partial sums.
 * sr_comm_wrap adopts an ncclComm_t the host created itself (not destroyed by sr_comm_destroy).
 * sr_comm_exchange: ONE ncclGroupStart/End around the sends and receives (u8 bytes), so pairs that send to each other
 * cannot deadlock; asynchronous on ctx's stream.  sr_comm_exchange_tile_rows builds that batch from the plan: rank `me`
 * sends rows h_need[r][t] of every tile t it owns (d_owned[t], DENSE rows of w * cn bytes) to every other rank r that needs
 * them, and receives rows h_need[me][t] of the tiles others own into d_recv[t] (a dense buffer of (r1 - r0) * w * cn bytes;
 * the blend then takes d_recv[t] - r0 * w * cn as the tile's virtual base pointer).  u8 tiles only. */
#define SR_COMM_ID_BYTES 128
typedef struct sr_comm sr_comm;
typedef struct sr_xfer {
    int peer;
    void *d_ptr;
    uint64_t bytes;
} sr_xfer;
SR_API int sr_comm_unique_id(void *id128);
SR_API int sr_comm_init(sr_ctx *ctx, const void *id128, int world, int rank, sr_comm **out);
SR_API int sr_comm_wrap(void *nccl_comm, sr_comm **out);
SR_API int sr_comm_info(const sr_comm *comm, int *world, int *rank);
SR_API int sr_comm_destroy(sr_comm *comm);
SR_API int sr_comm_exchange(sr_ctx *ctx, sr_comm *comm, const sr_xfer *sends, int n_send, const sr_xfer *recvs, int n_recv);
SR_API int sr_comm_exchange_tile_rows(sr_ctx *ctx, sr_comm *comm, const sr_tile_rect *h_tiles, int n, int cn,
                                      const int *h_need, const int *h_owner, const void *const *d_owned,
                                      const int64_t *owned_stride, void *const *d_recv);
/* SURVEY 8(b)'s sr_laplacian_blend_sharded: sr_comm_exchange_tile_rows followed, on the same stream, by sr_laplacian_blend of
 * this rank's rows -- plan = sr_blend_plan_create(..., rows[2 rank], rows[2 rank + 1]) of the exchange plan, the received
 * windows addressed through virtual base pointers.  (A host that wants the exchange of image i + 1 under the blend of image
 * i issues the two calls itself on two streams, as device_pipeline.py does.)  `plan` must have been created on `ctx` (one
 * stream orders the receive before the blend) for the same n tiles and cn channels: SR_ERR_INVALID_ARG / SR_ERR_SHAPE
 * otherwise; the tile arguments are checked by sr_sharded_tile_bases before anything is posted.  If a post inside the RCCL
 * group fails (SR_ERR_COMM) the batch is partial and the communicator must be destroyed: further calls on it fail. */
SR_API int sr_laplacian_blend_sharded(sr_ctx *ctx, sr_comm *comm, sr_blend_plan *plan, const sr_tile_rect *h_tiles, int n, int cn,
                                      const int *h_need, const int *h_owner, const void *const *d_owned,
                                      const int64_t *strides, void *const *d_recv, uint8_t *d_canvas, int64_t canvas_stride);
/* host only: the batch sr_comm_exchange_tile_rows posts, for hosts that move the rows themselves (MPI, hipMemcpyPeer).
 * Sends in (reader, tile) order, receives in (owner, tile) order; *n_send / *n_recv are the counts needed (SR_ERR_SHAPE when
 * the arrays are too small: at most n * (world - 1) sends and n receives). */
SR_API int sr_exchange_xfers(const sr_tile_rect *h_tiles, int n, int cn, int world, int rank, const int *h_need,
                             const int *h_owner, const void *const *d_owned, const int64_t *owned_stride,
                             void *const *d_recv, sr_xfer *sends, int cap_send, int *n_send, sr_xfer *recvs, int cap_recv,
                             int *n_recv);
/* host only: the per-tile base pointers rank `rank` hands to its strip blend -- an owned tile as it is, a received row window
 * moved up to its (virtual) row 0 (d_recv[t] - r0 * w * cn).  Validates what sr_laplacian_blend_sharded relies on: owners
 * inside the world, rows inside the tile, a dense stride (w * cn) for every tile that is received (SR_ERR_SHAPE otherwise),
 * a buffer for every window.  h_base[n] receives the pointers (NULL for tiles this strip does not read). */
SR_API int sr_sharded_tile_bases(const sr_tile_rect *h_tiles, int n, int cn, int world, int rank, const int *h_need,
                                 const int *h_owner, const void *const *d_owned, const int64_t *strides,
                                 void *const *d_recv, void **h_base);
SR_API int sr_comm_allreduce_f64(sr_ctx *ctx, sr_comm *comm, double *d_buf, int count);
/* tile-local rows [*r0, *r1) of tile t that the plan reads (empty if r0 >= r1): what a strip
 * owner must hold / receive for that tile. */
SR_API int sr_blend_plan_tile_rows(const sr_blend_plan *plan, int t, int *r0, int *r1);
SR_API int sr_blend_plan_workspace_bytes(const sr_blend_plan *plan, size_t *bytes);
/* host only: how a blend of tiles of `dtype` (SR_U8 / SR_F32) keeps the level-1 Gaussian planes in the plan's workspace:
 * *fmt = 0 fp32, 1 the exact 16-bit integers 256 * G_1 (three-channel u8 tiles whose levels 1 and 2 all come from the fused
 * down march; SR_G1_U16=0 at plan creation selects fp32).  The canvases are the same bits either way. */
SR_API int sr_blend_plan_g1_format(const sr_blend_plan *plan, int dtype, int *fmt);
/* host only: the work lists of the marched canvas gather as the plan launches them (empty where the plan does not march).
 * nt = 1 .. 4: the items of the `nt`-tile list in launch order, 8 ints each: x0 (canvas x of the left halo cell, a multiple
 * of 4), y0 (first canvas row), ncell (useful cells of 4 pixels: lanes 1 .. ncell), nstep (steps of two canvas rows), tile[4]
 * (the zone's tiles in list order, the first nt valid).  nt = 0: the rectangles that finish what the marched zones leave,
 * 4 ints each: x, y (canvas pixel of the first cell), w, h (cells of 4 x 2 pixels across / down).
 * *count receives the number of items; out (nullable: count only) receives at most `cap` of them. */
SR_API int sr_blend_plan_march_items(const sr_blend_plan *plan, int nt, int32_t *out, int64_t cap, int64_t *count);

/* h_d_tiles[i]: device address of row 0 of tile i (rows outside sr_blend_plan_tile_rows are
 * never touched, so the address may be virtual); h_strides[i]: row stride in bytes.
 * d_canvas: u8 HWC canvas (row stride canvas_stride bytes), only rows [row_begin,row_end)
 * are written.  d_canvas_f32 (nullable): dense fp32 HWC canvas receiving the normalised value
 * before clip / truncation (parity tests).
 * Any stride of at least the row length is addressed: where h_strides[i] * h_i or canvas_stride times the rows of one march
 * segment does not fit the 32-bit byte offsets of the marched canvas gather, the block gather (64-bit row addresses) writes the same bytes. */
SR_API int sr_laplacian_blend(sr_blend_plan *plan, int dtype, void *const *h_d_tiles,
                              const int64_t *h_strides, uint8_t *d_canvas, int64_t canvas_stride,
                              float *d_canvas_f32);
/* The Laplacian blend in two stages, so a strip owner can overlap the row exchange with compute:
 * sr_blend_pyramids builds G_i / R_i for the listed tiles only (first != 0: also the weight pyramids, which depend
 * only on the plan and are built once and kept; call it first with the tiles already resident, then with the tiles
 * that arrived), sr_blend_gather is the canvas gather
 * over all tiles.  sr_laplacian_blend == pyramids(all, first) + gather. */
SR_API int sr_blend_pyramids(sr_blend_plan *plan, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                             const int *h_tile_idx, int n_idx, int first);
SR_API int sr_blend_gather(sr_blend_plan *plan, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                           uint8_t *d_canvas, int64_t canvas_stride, float *d_canvas_f32);
SR_API int sr_weighted_blend(sr_blend_plan *plan, int dtype, void *const *h_d_tiles,
                             const int64_t *h_strides, uint8_t *d_canvas, int64_t canvas_stride,
                             float *d_canvas_f32);

/* weighted_average_fusion with caller-supplied weight maps (blending_module.py:729-751): h_d_weights[i] is an
 * h_i x w_i fp32 map in HBM (row stride in bytes, at least w_i * 4; address and stride multiples of 4).  Same accumulate /
 * normalise / clip / truncate, rows [row_begin, row_end) only; a pixel no tile covers is 0 in both canvases.
 * A tile whose sr_blend_plan_tile_rows window is empty (a row-window plan that does not reach it) is never read: both its
 * tile pointer and its weight pointer may be NULL (its strides are still checked).  A NULL weight pointer for a tile that has
 * rows is SR_ERR_INVALID_ARG.  Every refusal happens before anything is launched: the canvases are untouched. */
SR_API int sr_weighted_blend_custom(sr_blend_plan *plan, int dtype, void *const *h_d_tiles,
                                    const int64_t *h_strides, const float *const *h_d_weights,
                                    const int64_t *h_weight_strides, uint8_t *d_canvas, int64_t canvas_stride,
                                    float *d_canvas_f32);

/* Host-buffer conveniences with the reference's call shape (ndarrays in, ndarray out):
 * stage tiles to HBM, blend, copy the canvas back.  h_tiles[i] is a dense HWC array. */
SR_API int sr_laplacian_fusion_host(sr_ctx *ctx, int dtype, const void *const *h_tiles,
                                    const sr_tile_rect *h_rects, int n, int cn, int canvas_h,
                                    int canvas_w, int levels, int weight_type, uint8_t *h_canvas,
                                    float *h_canvas_f32);
SR_API int sr_weighted_fusion_host(sr_ctx *ctx, int dtype, const void *const *h_tiles,
                                   const sr_tile_rect *h_rects, int n, int cn, int canvas_h,
                                   int canvas_w, int weight_type, uint8_t *h_canvas,
                                   float *h_canvas_f32);

/* ---- BlendingModule.detect_seams window scan (blending_module.py:765-903) -------------
 * For every tile, windows of `window` x `window` pixels every `stride` pixels over the part of the tile inside the
 * canvas; global-statistics SSIM (fp64) between the tile and the canvas window on gray values (the reference's
 * BGR2GRAY-on-RGB quirk included).  Windows scoring below `threshold` are returned unordered (up to cap records;
 * *h_count is the number found -- call again with a larger buffer if it exceeds cap).  Merging adjacent windows into
 * Seam boxes is host bookkeeping (blending_module.py:905-967). */
typedef struct sr_seam_record {
    int tile, x, y, pad;     /* tile index, canvas position of the window */
    double score;
} sr_seam_record;
SR_API int sr_seam_scan(sr_ctx *ctx, const uint8_t *d_canvas, int64_t canvas_stride, int canvas_h, int canvas_w,
                        int cn, const sr_tile_rect *h_rects, void *const *h_d_tiles, const int64_t *h_strides,
                        int n, int window, int stride, int gray_shift, double threshold, sr_seam_record *h_out,
                        int cap, int *h_count);

/* ---- TilingModule.merge_tiles feather path (tiling_module.py:1074-1175) ---------------- */
typedef struct sr_merge_tile {
    int x, y;                 /* int(global_x*scale), int(global_y*scale)                 */
    int src_w, src_h;         /* size of the tile data as handed in                       */
    int out_w, out_h;         /* metadata.output_w/h: data is bilinearly resized to this  */
    int ov_t, ov_b, ov_l, ov_r; /* int(overlap*scale) ramps; 0 = none                     */
} sr_merge_tile;
SR_API int sr_feather_merge(sr_ctx *ctx, const sr_merge_tile *h_tiles, int n, void *const *h_d_tiles,
                            const int64_t *h_strides, int blending, uint8_t *d_canvas,
                            int64_t canvas_stride, int canvas_h, int canvas_w);
/* the same with the tiles' element type given: SR_U8 (as above) or SR_F32 -- float32 tile data is accumulated as it is
 * (the reference's astype(float32), tiling_module.py:1104-1109) or goes through cv2.resize's float INTER_LINEAR arithmetic
 * when its size differs from out_w x out_h.  Strides in bytes. */
SR_API int sr_feather_merge_dt(sr_ctx *ctx, int dtype, const sr_merge_tile *h_tiles, int n, void *const *h_d_tiles,
                               const int64_t *h_strides, int blending, uint8_t *d_canvas, int64_t canvas_stride,
                               int canvas_h, int canvas_w);

/* BlendingModule.gradient_domain_fusion (blending_module.py:1377-1489 with _reconstruct_from_gradients :1491-1523): n tiles
 * of dtype SR_U8 or SR_F32 (the reference's astype(float32) of any other type is the caller's), h x w x cn (cn 1..4) with
 * their canvas rectangles (x, y = the reference's position (y, x); 0 <= x < canvas_w, 0 <= y < canvas_h, min side >= 8).
 * Per channel the float32 Sobel of each tile (reflect-101 at the TILE's borders) times its cosine weight map
 * (feather width min(h, w) // 8) is accumulated in list order, divided by max(sum of weights, 1e-6f), summed along rows
 * (np.cumsum, axis=1) and along columns (axis=0) as sequential fp32 chains, halved, clipped to [0, 255] and truncated into
 * the u8 canvas.  d_work: canvas_h * canvas_w * cn floats of device workspace.  On return d_work holds the row prefix sums
 * (np.cumsum(grad_x / max(W, 1e-6f), axis=1), canvas layout, fp32); tests/test_gpu_gradient_lists.py compares them bit for
 * bit, because the u8 canvas hides most fp32 differences.  Asynchronous. */
SR_API int sr_gradient_fusion(sr_ctx *ctx, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                              const sr_tile_rect *h_rects, int n, int cn, int canvas_h, int canvas_w, uint8_t *d_canvas,
                              int64_t canvas_stride, float *d_work);
/* compute_blend_quality's gradient fields (blending_module.py:1600-1606): over every element of the u8 image (cn 1..4) the
 * float32 Sobel gx, gy (reflect-101 at the image border, exact integers here); *h_sum_sq receives the exact sum of
 * gx^2 + gy^2, *h_sum_mag the fp64 sum of sqrt(gx^2 + gy^2).  mean = sum_mag / N, std = sqrt(sum_sq / N - mean^2). */
SR_API int sr_gradient_stats_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn,
                                uint64_t *h_sum_sq, double *h_sum_mag);
/* compute_blend_quality's per-tile SSIM (blending_module.py:1584-1596 with _compute_ssim :855-903): for tile i (rectangle
 * h_rects[i], u8, cn 1, 3 or 4 like the canvas) the ROI canvas[y:y+h, x:x+w] clipped by the canvas; when the clip changes
 * its size the tile is first resized to the ROI like cv2.resize(INTER_LINEAR).  Gray = cv2.COLOR_BGR2GRAY applied to the
 * RGB data (channel 0 takes the blue weight; cn 1: the value itself).  h_sums[5 i .. 5 i + 4] receive the exact sums of
 * a, b, a^2, b^2, a b over the ROI (a: canvas gray, b: tile gray); the float64 SSIM formula is the caller's. */
SR_API int sr_tile_ssim_sums_u8(sr_ctx *ctx, const uint8_t *d_canvas, int64_t canvas_stride, int canvas_h, int canvas_w,
                                int cn, const sr_tile_rect *h_rects, void *const *h_d_tiles, const int64_t *h_strides, int n,
                                int gray_shift, uint64_t *h_sums);

/* ---- commercial / no-reference metrics (quality_assessment_module.py:611-1193) ---------------------------------------
 * sr_commercial_u8: one u8 image in HBM (cn 1 = gray, 3 = RGB, 4 = RGBA with alpha ignored), gray = the RGB2GRAY rule of
 * gray_shift.  Rectangle 0 is the whole image with the metrics of `flags`; rectangles 1..n_roi are h_rois[i] (inside the
 * image, non-empty) with the metrics of h_roi_flags[i] (only LAPG, TEX, LAB, SKIN, RGB), every stencil taken with
 * reflect-101 at the rectangle's own border.  Flag bits and what lands in h_ints[r * 40 + k] / h_flts[r * 8 + k]:
 *   1 LAPG     k 0..3   exact sum l, l^2 (cv2.Laplacian ksize 1), sum g, g^2
 *   2 NOISE    k 4, 5   exact sum n, n^2, n = 16 (g - GaussianBlur3x3(g)) (an integer)
 *   4 SOBEL    k 6      exact sum gx^2 + gy^2 (3x3 Sobel, reflect-101);   flt 3: fp64 sum sqrt(gx^2 + gy^2)
 *   8 MSCN     flt 0..2 fp64 sums of m, m^2, |m| with m the fp32 MSCN coefficient (7x7 Gaussian sigma 7/6, fixed order)
 *  16 TEX      flt 4    fp64 sum of the fp32 5x5 box local variance
 *  32 LAB      k 7..12  exact sums L, L^2, a, a^2, b, b^2 of cv2's 8-bit RGB2Lab (cn >= 3)
 *  64 SKIN     k 13     count of 133 <= Cr <= 173 and 77 <= Cb <= 127 (8-bit RGB2YCrCb; cn >= 3); LAB sums as well
 * 128 RGB      k 14..16 exact sums R, G, B (cn >= 3)
 * 256 BLOCKS   (rect 0) k 17 sum v, k 18 / 19 low / high 32 bits of sum v^2, v = 64 sum x^2 - (sum x)^2 over the 8x8 blocks
 *              of range(0, h - 8, 8) x range(0, w - 8, 8); k 38 the block count
 * 512 REGIONS  (rect 0) k 20..35 the 16 region sums (h // 4 x w // 4 regions, row-major; zeros when h or w < 4)
 * 1024 CANNY   (rect 0) k 36 cv2.Canny(gray, 50, 150) edge pixel count, k 37 hysteresis sweeps taken
 * 2048 HF      (rect 0) flt 5 / 6: fp64 sum of |F| outside the radius min(h, w) // 4 / over all of the 2-D DFT of the gray
 *              image (centred frequencies; fp32 FFT and magnitude).  SR_ERR_UNSUPPORTED for a side above sr_fft_max_len().
 * Every fp64 sum is per-block partials added in a fixed order: equal inputs give equal bits.  The caller finishes the
 * metrics (means, variances, clips) in fp64. */
SR_API int sr_commercial_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int gray_shift,
                            int flags, const sr_tile_rect *h_rois, const int *h_roi_flags, int n_roi, int64_t *h_ints,
                            double *h_flts);
/* Longest line sr_fft_c2c (and the DFT of sr_commercial_u8) transforms. */
SR_API int sr_fft_max_len(void);
/* Forward DFT (sign -1, unscaled) of `lines` rows of n interleaved fp32 complex values, d_in -> d_out (may alias): the
 * mixed-radix / Bluestein FFT behind the high-frequency ratio.  Synchronous. */
SR_API int sr_fft_c2c(sr_ctx *ctx, const void *d_in, void *d_out, int64_t lines, int n);

/* ---- content analysis (tiling_module.py:174-370, :752-757) ------------------------------------------------------------
 * The u8 image (cn 1 = gray, 3 = RGB, 4 = RGBA with alpha ignored) is in HBM; gray = cv2.COLOR_BGR2GRAY applied to the RGB
 * data as the reference does (channel 0 takes the blue weight, 15-bit rule; cn 1: the value itself).  Every output plane is
 * contiguous (row length w) and stays in HBM.
 *
 * sr_saliency_u8: ContentAnalyzer.compute_saliency_map's spectral-residual branch (:261-289) -> d_sal (h * w bytes).
 * F = fft2(gray), L = log(|F| + 1e-8), the 5x5 mean of L taken on the fftshift-ed array (shift n / 2, reflect-101 at that
 * array's own border), R = L - mean, the inverse 2-D DFT of exp(R) F / |F| (unit phase where F = 0) with its 1 / (h w)
 * scale, its magnitude, the 5x5 Gaussian of sigma 0 ([1 4 6 4 1] / 16, reflect-101), then
 * u8((s - min) / (max - min + 1e-8) * 255) truncated.  fp32 throughout (the FFT of sr_fft_c2c); min and max are taken in a
 * fixed order: equal inputs give equal bytes.  SR_ERR_UNSUPPORTED for a side above sr_fft_max_len().  Asynchronous. */
SR_API int sr_saliency_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, uint8_t *d_sal);
/* compute_local_entropy (:291-321) -> d_out (h * w floats): per window x window cell of the gray image (edge cells
 * partial; 1 <= window <= 32768) the 256-bin histogram with exact counts, p = count / pixels and
 * H = -sum p log2(p + 1e-10) in fp32 (fixed summation order), written to every pixel of the cell.  Asynchronous. */
SR_API int sr_local_entropy_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int window,
                               float *d_out);
/* create_forbidden_zone_map's map (:344-370) -> d_map (h * w bytes, 0 or 1): d_sal[y, x] > threshold (d_sal may be NULL:
 * zeros) OR-ed with the n filled rectangles [y:y+h, x:x+w] of h_rects, clipped to the image (w, h >= 0).  Asynchronous. */
SR_API int sr_forbidden_map(sr_ctx *ctx, const uint8_t *d_sal, int h, int w, int threshold, const sr_tile_rect *h_rects,
                            int n, uint8_t *d_map);
/* Per-tile forbidden counts (:753-757): h_counts[i] = the exact number of non-zero bytes of the u8 plane d_map (h x w, row
 * stride in bytes) inside h_rects[i] clipped to the plane (0 for an empty clip).  One launch for all rectangles (per 32768);
 * synchronous. */
SR_API int sr_rect_counts_u8(sr_ctx *ctx, const uint8_t *d_map, int64_t stride, int h, int w, const sr_tile_rect *h_rects,
                             int n, uint64_t *h_counts);

/* ---- MSER text regions (ContentAnalyzer.detect_text_regions, tiling_module.py:214-237, 358-362; csrc/sr_mser.hip) -------
 * PARITY UNPINNED: cv2 is not available to this repository's tests, so agreement with cv2.MSER_create() is not claimed and
 * not tested.  What is built is Matas' maximally stable extremal regions in component-tree form, with OpenCV's default
 * parameter values and OpenCV's 4-neighbourhood, pinned by a Python restatement, by a brute-force tree through
 * scipy.ndimage.label and by sr_mser_host_u8; every comparison is exact (all records are integers).  Not built: colour
 * MSER (MSCR), 8-connectivity, the regions' pixel lists.
 *
 * Input: a u8 image, cn 1 / 3 / 4 (alpha ignored), row stride in bytes; g = the gray plane of the content section above
 * (cv2.COLOR_BGR2GRAY applied to the RGB data, 15-bit rule; cn 1: the value itself).
 * Polarity: dark regions use g (polarity 0), bright regions 255 - g (polarity 1); each has its own tree.  polarity_mask:
 * bit 0 dark, bit 1 bright; the default of the Python mirror is both, dark first.
 * Component tree: for t = 0 .. 255 take the 4-connected components of {p : g(p) <= t}.  A node is a pair (component C,
 * level t) where C holds at least one pixel with g = t.  The parent of a node is the node of the smallest level t' > t
 * whose component contains C; the component of level max g is the root.  A node carries level, area = |C|, the inclusive
 * box x0, y0, x1, y1 and seed = the smallest row-major pixel index in C; (level, seed) identifies it.
 * Variation: S(n) = the area of the ancestor-or-self of n with the largest level <= level(n) + delta (the walk stops at
 * the root); var(n) = (S(n) - area(n)) / area(n).  Two variations are compared by cross-multiplication in int64,
 * (S_a - A_a) A_b against (S_b - A_b) A_a: nothing rounds.
 * Maximally stable: n is stable iff var(n) <= var(parent(n)) (when it has a parent) and var(n) <= var(c) for every child
 * c.  Ties knock out nobody; the root takes part like any other node.
 * Filters, on stable nodes only: min_area <= area <= max_area, and in float64 (double)(S - area) < max_variation *
 * (double)area (one multiplication, not contracted).
 * Diversity: for a node n that passed the filters let a be its nearest ancestor that also passed them; n is dropped iff, in
 * float64, (double)(area(a) - area(n)) < min_diversity * (double)area(a).  The ancestor's own fate under this rule does not
 * matter.
 * Defaults: delta 5, min_area 60, max_area 14400, max_variation 0.25, min_diversity 0.2.
 * Output order: polarity (dark first), then level, then seed.  Equal inputs give equal bytes.
 * SR_ERR_UNSUPPORTED: more than 2^24 pixels (4096 x 4096: indices stay int32 and the workspace, 53 bytes per pixel + 12 KiB,
 * stays below 1 GiB), delta outside 1 .. 255, min_area < 1, max_area < min_area, a negative or NaN max_variation /
 * min_diversity. */
typedef struct sr_mser_params {
    int delta, min_area, max_area;
    double max_variation, min_diversity;
} sr_mser_params;
typedef struct sr_mser_region {
    int polarity, level, area, x0, y0, x1, y1, seed, S;
} sr_mser_region;
typedef struct sr_mser_node {
    int level, area, x0, y0, x1, y1, seed, parent_level, parent_seed; /* parent_*: -1 for the root */
} sr_mser_node;
SR_API int sr_mser_default_params(sr_mser_params *out);
/* Host only: every refusal above, the bytes of context workspace of one call and the capacity of its node table (either
 * output may be NULL). */
SR_API int sr_mser_plan(int h, int w, const sr_mser_params *params, size_t *workspace_bytes, int64_t *node_cap);
/* The regions of the image in HBM -> h_regions (the first cap of them in output order); *count is the true total even when it
 * exceeds cap.  Level-synchronous union-find; the workspace comes from the context and is never read before it is written.
 * Synchronous. */
SR_API int sr_mser_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, const sr_mser_params *params,
                      int polarity_mask, sr_mser_region *h_regions, int64_t cap, int64_t *count);
/* For inspection: the whole node table of one polarity (0 dark, 1 bright) in (level, seed) order.  *count is the number of
 * nodes; when it exceeds cap nothing else is written.  Synchronous. */
SR_API int sr_mser_tree_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int polarity,
                           sr_mser_node *h_nodes, int64_t cap, int64_t *count);
/* The records of the last sr_mser_u8 call on this context, kept on the host in output order: the first cap of them ->
 * h_regions, *count the total.  No device work: a caller whose buffer was short fetches the rest here instead of running the
 * detection again.  Empty before the first call and after a call that failed. */
SR_API int sr_mser_last_regions(sr_ctx *ctx, sr_mser_region *h_regions, int64_t cap, int64_t *count);
/* For tests: the context's MSER workspace (NULL and 0 before the first call).  A call never reads what it held before. */
SR_API int sr_mser_workspace(sr_ctx *ctx, void **d_ptr, size_t *bytes);
/* The host twins: the same definition on host pointers (sorted-pixel sequential union-find), the restatement the device is
 * held to. */
SR_API int sr_mser_host_u8(const uint8_t *img, int64_t stride, int h, int w, int cn, const sr_mser_params *params,
                           int polarity_mask, sr_mser_region *regions, int64_t cap, int64_t *count);
SR_API int sr_mser_tree_host_u8(const uint8_t *img, int64_t stride, int h, int w, int cn, int polarity, sr_mser_node *nodes,
                                int64_t cap, int64_t *count);
/* Host only: the text boxes of tiling_module.py:231-235 in region order, duplicates kept: (x, y, w, h) = (x0, y0,
 * x1 - x0 + 1, y1 - y0 + 1), kept iff w > 20 and h > 10 and (double)w < image_w * 0.5.  rects needs room for n. */
SR_API int sr_mser_text_boxes(const sr_mser_region *regions, int64_t n, int image_w, sr_tile_rect *rects, int64_t *m);

/* ---- Cascade: Viola-Jones cascade detection (ContentAnalyzer.detect_faces, tiling_module.py:195-212, 346-357;
 * cv2.CascadeClassifier(path).detectMultiScale(gray, 1.1, 4); csrc/sr_cascade.hip) ----------------------------------------
 * PARITY UNPINNED WITH cv2: cv2 is not available to this repository's tests; the OpenCV steps below are recalled from
 * objdetect/src/cascadedetect.cpp and could not be checked.  PARITY PINNED WITH scikit-image 0.18.3 for the LBP stage
 * evaluation: with the OpenCV-trained model scikit-image ships (lbpcascade_frontalface_opencv.xml) the windows that pass
 * every stage on three recorded planes equal those of skimage.feature.Cascade (tests/golden/cascade_skimage.npz).
 * The HAAR path is built and tested on constructed cascades only: the reference's haarcascade_frontalface_default.xml is
 * not available to this repository.  The trained model is the caller's file; the engine is this library.
 *
 * Input: a u8 image, cn 1 / 3 / 4 (alpha ignored), row stride in bytes; g = the gray plane of the content section above
 * (cv2.COLOR_BGR2GRAY applied to the RGB data, 15-bit rule; cn 1: the value itself), the plane MSER uses.
 * Model: a window W0 x H0 and a feature type (SR_CASCADE_LBP / SR_CASCADE_HAAR); stages, each a float32 threshold and a
 * list of depth-1 stumps.  An LBP stump: feature index, eight 32-bit subset words, two float32 leaves.  A HAAR stump:
 * feature index, float32 threshold, two leaves.  An LBP feature: a rectangle (x, y, bw, bh), the top-left block of a 3 x 3
 * grid of bw x bh blocks.  A HAAR feature: 2 or 3 upright rectangles, each with a float32 weight.
 * LBP code: block sums b0 .. b8 in row-major order, centre c = b4; bits 7 .. 0 are b0>=c, b1>=c, b2>=c, b5>=c, b8>=c, b7>=c,
 * b6>=c, b3>=c.  The stump adds leaf[0] when subset[code >> 5] & (1 << (code & 31)) is set, leaf[1] otherwise.  Integers only.
 * HAAR value: val = sum weight_i * boxsum_i in float64, left to right, every product and every sum rounded (no
 * contraction).  With A, s, q the area, sum and sum of squares of the rectangle (1, 1, W0 - 2, H0 - 2) of the window:
 * nf = sqrt((double)(A q - s^2)) when that integer is positive, 1 otherwise.  The stump adds leaf[0] when
 * val < (double)thr * nf, leaf[1] otherwise.
 * Stage: the leaves are added in float32 in stump order, starting from 0 (additions only); the window fails the stage when
 * sum < stageThreshold.  A window is a detection when it passes every stage.
 * Scales: f_0 = 1, f_{k+1} = f_k * scale_factor in double; rnd = round half to even in double;
 * win_k = (rnd(W0 f_k), rnd(H0 f_k)); the scaled plane has sw = rnd(w / f_k), sh = rnd(h / f_k).  The list ends when win_k
 * exceeds max_size on either side (default: the image) or when sw < W0 or sh < H0; scales whose win_k is below min_size on
 * either side are skipped (they still count as steps of the list).
 * Scaled plane: an exact-integer bilinear resize with pixel centres and a replicated border (THIS PROJECT'S CHOICE).  Per
 * axis the position of output sample x is the rational ((2 x + 1) w - sw) / (2 sw); the taps are its floor and floor + 1,
 * both clamped to [0, w - 1]; the weights are the numerators over the common denominator; the value is
 * (sum weight products * pixels + D / 2) // D with D = 4 sw sh, in int64.  f = 1 is the identity.
 * Windows: on scale k every position (x, y) with x = y = 0 modulo step, x <= sw - W0, y <= sh - H0; step = 2 when
 * f_k <= 2, 1 otherwise.  A detection gives the candidate (rnd(x f_k), rnd(y f_k), win_k.w, win_k.h).  Canonical order
 * of candidates: scale, then y, then x.
 * Known distances to OpenCV, no size claimed: (1) OpenCV resizes with INTER_LINEAR_EXACT, whose fixed-point weights are
 * not restated; (2) OpenCV's working size drops the last row and column of positions; (3) OpenCV skips the position after a
 * window that fails stage 0 (a CPU shortcut that depends on scan order).
 * Grouping (host only; groupRectangles(cands, min_neighbors, 0.2)): min_neighbors = 0 returns the candidates as they are.
 * Otherwise classes are the transitive closure of "similar": |dx|, |dy|, |d(x + w)|, |d(y + h)| all <=
 * 0.2 * (min(w1, w2) + min(h1, h2)) * 0.5, evaluated in double in that order.  Classes are ordered by their first member in
 * canonical order.  A class of n members becomes, per field x, y, w, h: the integer sum of the members' fields (held in
 * 64 bits) converted to float32, multiplied in float32 by the float32 quotient 1.f / n, rounded half to even to int.  A
 * class is dropped when
 * n <= min_neighbors; a class r1 is dropped when some other class r2 with n2 > min_neighbors contains it within
 * dx = rnd(r2.w * 0.2), dy = rnd(r2.h * 0.2) (double products) -- r1.x >= r2.x - dx, r1.y >= r2.y - dy,
 * r1.x + r1.w <= r2.x + r2.w + dx, r1.y + r1.h <= r2.y + r2.h + dy -- and (n2 > max(3, n1) or n1 < 3).
 * SR_ERR_UNSUPPORTED, by name, before any device call: the old opencv-haar-classifier XML layout; a stageType other than
 * BOOST; trees deeper than one node; tilted Haar rectangles; more than 3 (or fewer than 2) rectangles per Haar feature; an
 * LBP maxCatCount other than 256; a window side outside 3 .. 255 (3: the LBP grid and the normalisation rectangle need it;
 * 255: coordinates pack into bytes and every box sum of squares stays below 2^32); zero stages; more than 4096 stages or
 * 65536 stumps; a feature index out of range; a rectangle outside the window or empty; NaN thresholds, leaves or weights;
 * scale_factor <= 1 or NaN; more than SR_CASCADE_MAX_SCALES (128) steps of the scale list; a negative min_neighbors; an
 * image above 2^24 pixels; a pyramid whose table elements (the sum of (sw + 1)(sh + 1) over the scales; its samples and
 * window positions are fewer) exceed 2^31 - 1: every index of the kernels is an int32.  The pyramid holds about 5.8 times
 * the image at factor 1.1, far below that; the two caps alone do not bound it (128 scales of nearly 2^24 samples each at
 * a factor close to 1), so the pyramid is measured and refused by name.
 * Not built: tilted features, deep trees, the old XML layout, HOG cascades, detectMultiScale3's weights, a multi-GPU split
 * of one call. */
#define SR_CASCADE_LBP 0
#define SR_CASCADE_HAAR 1
#define SR_CASCADE_MAX_SCALES 128
typedef struct sr_cascade sr_cascade;
typedef struct sr_cascade_info {
    int feature_type, win_w, win_h, n_stages, n_stumps, n_features;
    /* what the file declared, for the refusals: 1 = the old opencv-haar-classifier layout; 0 = BOOST; the deepest tree in
     * nodes; 1 = some Haar rectangle is tilted; the largest rectangle count of a Haar feature (0 for LBP); LBP maxCatCount */
    int old_layout, stage_type, max_tree_nodes, tilted, max_rects, max_cat_count;
} sr_cascade_info;
typedef struct sr_cascade_params {
    double scale_factor;                   /* 1.1 */
    int min_neighbors;                     /* 4; used by the callers of sr_cascade_group */
    int min_w, min_h, max_w, max_h;        /* 0: no minimum / the image */
} sr_cascade_params;
typedef struct sr_cascade_scale {
    double f;
    int win_w, win_h, sw, sh, step, nx, ny; /* nx x ny window positions */
} sr_cascade_scale;
/* Host only: checks and packs a model.  stage_thr[n_stages], stage_count[n_stages] (stumps per stage, in order);
 * stump_feature[n_stumps], stump_leaves[2 n_stumps]; LBP: stump_subsets[8 n_stumps], feat_rects[4 n_features] (x, y, bw, bh);
 * HAAR: stump_thr[n_stumps], feat_nrects[n_features], feat_rects[12 n_features] (three x, y, w, h slots),
 * feat_weights[3 n_features].  Arrays of the other type may be NULL.  Every model refusal above happens here. */
SR_API int sr_cascade_create(const sr_cascade_info *info, const float *stage_thr, const int *stage_count,
                             const int *stump_feature, const float *stump_thr, const float *stump_leaves,
                             const int32_t *stump_subsets, const int *feat_nrects, const int *feat_rects,
                             const float *feat_weights, sr_cascade **out);
SR_API int sr_cascade_destroy(sr_cascade *model);
SR_API int sr_cascade_desc(const sr_cascade *model, sr_cascade_info *out);
SR_API int sr_cascade_default_params(sr_cascade_params *out);
/* Host only: every refusal of the arguments, the scale list (the first cap entries -> scales, *n_scales the total; 0 for an
 * image smaller than the window), the bytes of context workspace of one call and the number of window positions. */
SR_API int sr_cascade_plan(const sr_cascade *model, int h, int w, const sr_cascade_params *params, sr_cascade_scale *scales,
                           int cap, int *n_scales, size_t *workspace_bytes, int64_t *positions);
/* The raw candidates (x, y, w, h) of the image in HBM in canonical order -> h_cands (the first cap of them); *count is the
 * true total.  A fixed number of launches whatever the number of scales; nothing is launched when there is no scale.  The
 * workspace comes from the context and is never read before it is written.  Synchronous. */
SR_API int sr_cascade_u8(sr_ctx *ctx, const sr_cascade *model, const uint8_t *d_img, int64_t stride, int h, int w, int cn,
                         const sr_cascade_params *params, sr_tile_rect *h_cands, int64_t cap, int64_t *count);
/* The candidates of the last sr_cascade_u8 call on this context, kept on the host: no device work.  Empty before the first
 * call and after a call that failed. */
SR_API int sr_cascade_last_candidates(sr_ctx *ctx, sr_tile_rect *h_cands, int64_t cap, int64_t *count);
/* Host only: the grouping above.  rects needs room for n; *m receives the number of boxes. */
SR_API int sr_cascade_group(const sr_tile_rect *cands, int64_t n, int min_neighbors, sr_tile_rect *rects, int64_t *m);
/* For inspection and tests: the scaled plane of scale k of the plan (sw * sh bytes, dense) -> h_plane. */
SR_API int sr_cascade_plane_u8(sr_ctx *ctx, const sr_cascade *model, const uint8_t *d_img, int64_t stride, int h, int w, int cn,
                               const sr_cascade_params *params, int k, uint8_t *h_plane);
/* For inspection and tests: on the scale-0 plane (the gray plane itself) and the given step (1 or 2), per position in
 * row-major order the number of stages passed -> h_map; *count = nx * ny (nothing else is written when it exceeds cap). */
SR_API int sr_cascade_stage_map_u8(sr_ctx *ctx, const sr_cascade *model, const uint8_t *d_img, int64_t stride, int h, int w,
                                   int cn, int step, int32_t *h_map, int64_t cap, int64_t *count);
/* For tests: the context's cascade workspace (NULL and 0 before the first call). */
SR_API int sr_cascade_workspace(sr_ctx *ctx, void **d_ptr, size_t *bytes);
/* The host twins: the same definition on host pointers, the restatement the device is held to. */
SR_API int sr_cascade_host_u8(const sr_cascade *model, const uint8_t *img, int64_t stride, int h, int w, int cn,
                              const sr_cascade_params *params, sr_tile_rect *cands, int64_t cap, int64_t *count);
SR_API int sr_cascade_plane_host_u8(const sr_cascade *model, const uint8_t *img, int64_t stride, int h, int w, int cn,
                                    const sr_cascade_params *params, int k, uint8_t *plane);
SR_API int sr_cascade_stage_map_host_u8(const sr_cascade *model, const uint8_t *img, int64_t stride, int h, int w, int cn,
                                        int step, int32_t *map, int64_t cap, int64_t *count);

/* ---- BlendingModule.poisson_fusion / repair_seams (blending_module.py:563-659, 1148-1240; csrc/sr_poisson.hip) ---------------
 * PARITY UNPINNED: cv2 is not available to this repository's tests, so the OpenCV behaviour below is restated from memory
 * (Cloning::normalClone of photo/src/seamless_cloning_impl.cpp, GaussianBlur's 8-bit fixed-point path) and tested against this
 * repository's own NumPy / SciPy restatement (tests/_poisson_ref.py).
 *
 * sr_poisson_clone_u8: cv2.seamlessClone's solve on ONE rectangle of h x w pixels, 3 channels: d_dest is the destination
 * rectangle, d_patch the source pixels laid over it, d_mask (one byte per pixel) the clone mask.  fp32 throughout:
 *   the mask is (byte != 0) eroded three times by a 3 x 3 element (a 7 x 7 minimum; pixels outside the rectangle do not erode);
 *   forward differences I[x + 1] - I[x], I[y + 1] - I[y] of destination and patch per channel;
 *   mode 1 (NORMAL_CLONE) takes the patch pair where the mask is set, mode 2 (MIXED_CLONE) there takes per pixel and channel the
 *   patch pair where |pgx - pgy| > |dgx - dgy| and else the destination pair, mode 3 (MONOCHROME_TRANSFER) is mode 1 with the
 *   patch replaced by its 8-bit RGB2GRAY value in all three channels; the destination pair where the mask is clear;
 *   backward differences of that field give the Laplacian, the 4-neighbour Laplacian of the destination with its interior
 *   zeroed is subtracted, and the (h - 2) x (w - 2) Dirichlet problem is solved by a DST-I along rows and columns, a division by
 *   (2 cos(pi (x + 1) / (w - 1)) - 2) + (2 cos(pi (y + 1) / (h - 1)) - 2), and the inverse DST-I along both axes;
 *   d_out's interior receives saturate(round-half-even(solution)), its 1-pixel frame the destination's (d_out may be d_dest).
 * (A patch whose pixels outside the mask are zeroed, as seamlessClone prepares it, gives the same bytes: the eroded mask never
 * selects a patch difference that reaches outside the mask.)  h or w below 3: no interior, the output is the destination.  A
 * side above sr_poisson_max_side() (= sr_fft_max_len() / 2 + 1: the DST-I of n values is taken from the DFT of their odd
 * extension to 2 (n + 1)): SR_ERR_UNSUPPORTED.  Fixed summation orders: equal inputs give equal bytes.  Asynchronous. */
SR_API int sr_poisson_max_side(void);
SR_API int sr_poisson_clone_u8(sr_ctx *ctx, const uint8_t *d_dest, int64_t dest_stride, const uint8_t *d_patch,
                               int64_t patch_stride, const uint8_t *d_mask, int64_t mask_stride, int h, int w, int mode,
                               uint8_t *d_out, int64_t out_stride);
/* cv2.GaussianBlur(roi, (15, 15), 0) on u8, cn 1, 3 or 4 (repair_seams' "increase_blend_width", :1191-1193): sigma 2.6,
 * separable, 8.8 fixed-point taps {1 3 6 12 20 29 37 40 37 ...} (side taps rounded, the centre takes what is left of 256), the
 * row pass exact in 16 bits, the column pass rounded once ((s + 2^15) >> 16), REFLECT_101 at the rectangle's own border.
 * d_dst may be d_src (the row pass goes through workspace).  Asynchronous. */
SR_API int sr_gaussian_blur15_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int cn, uint8_t *d_dst,
                                 int64_t dst_stride);
/* _compute_ssim (:855-903) of two u8 rectangles of h x w pixels (cn 1, 3 or 4; gray = cv2.COLOR_BGR2GRAY applied to the RGB
 * data): exact integer moments on the GPU, the float64 global-statistics formula on them -> *h_ssim.  Synchronous. */
SR_API int sr_region_ssim_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
                             int w, int cn, int gray_shift, double *h_ssim);
/* cv2.resize(src, (dw, dh)) with the default INTER_LINEAR on u8 (cn 1..4): the sampling of sr_feather_merge's resize branch
 * (half-pixel centres, 11-bit coefficients).  Asynchronous. */
SR_API int sr_resize_linear_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int cn, uint8_t *d_dst,
                               int64_t dst_stride, int dh, int dw);

/* ---- quality metrics (quality_assessment_module.py:277-417) ---------------------------- */
/* Sum of squared differences over h rows of rowlen u8 elements -> *h_sse (exact integer).
 * PSNR = 10 log10(data_range^2 / (sse / (h*rowlen))) is finished on the host (and partial sums
 * of strips are simply added). */
SR_API int sr_sse_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b,
                     int64_t stride_b, int h, int64_t rowlen, uint64_t *h_sse);
/* Asynchronous form: result left in device memory (8 bytes), no stream sync. */
SR_API int sr_sse_u8_async(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b,
                           int64_t stride_b, int h, int64_t rowlen, uint64_t *d_sse);
SR_API double sr_psnr_from_sse(uint64_t sse, uint64_t count, double data_range);
/* fp32 images (calculate_psnr on float arrays with max > 1, quality_assessment_module.py:191-195 leaves them float):
 * skimage semantics, fp32 difference and square, fp64 sum.  PSNR = 10 log10(data_range^2 / (sse / count)). */
SR_API int sr_sse_f32(sr_ctx *ctx, const float *d_a, int64_t stride_a, const float *d_b, int64_t stride_b,
                      int h, int64_t rowlen, double *h_sse);

/* SSIM between two u8 images of h x w pixels with cn channels (cn == 3: RGB -> gray with the
 * OpenCV fixed-point rule, gray_shift 15 or 14; cn == 1: already gray).  The SSIM map is
 * summed over map rows [row_begin,row_end) intersected with the mode's valid region; the sum
 * and the number of map samples come back so strips can be added.  mean = sum / count. */
SR_API int sr_ssim_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b,
                      int64_t stride_b, int h, int w, int cn, int mode, int gray_shift,
                      double data_range, int row_begin, int row_end, double *h_sum,
                      uint64_t *h_count);
/* The same three SSIM variants on FLOAT images (the reference passes float arrays with max > 1 on unchanged,
 * quality_assessment_module.py:169-195,351-417): dtype SR_F32 or SR_F64, cn 1 (gray as it is) or 3 (float32 only: cv2's
 * float RGB2GRAY, 0.299 R + 0.587 G + 0.114 B in fp32; cv2.cvtColor rejects float64).  float64 arithmetic throughout, like
 * scikit-image 0.18.3 (the version pinned here); a separable reference form, not a tuned kernel.  Strides in bytes.
 * PARITY UNPINNED for SR_F32: scikit-image >= 0.19 (the reference asks for >= 0.21) keeps float32 inputs in float32
 * (_supported_float_type), so its filters and SSIM algebra run in fp32 there and differ from this float64 form by about
 * 1e-6 relative -- inside the north star's 1e-4, outside the 1e-9 the tests hold against this repository's own oracle. */
SR_API int sr_ssim_float(sr_ctx *ctx, int dtype, const void *d_a, int64_t stride_a, const void *d_b, int64_t stride_b,
                         int h, int w, int cn, int mode, double data_range, int row_begin, int row_end, double *h_sum,
                         uint64_t *h_count);
SR_API int sr_ssim_u8_async(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b,
                            int64_t stride_b, int h, int w, int cn, int mode, int gray_shift,
                            double data_range, int row_begin, int row_end, double *d_sum,
                            uint64_t *h_count);
/* Fused assessment: ONE pass over both images (6 bytes / pixel) for the squared-difference sum and
 * the Gaussian SSIM in both variants (cropped "gauss11" and full-frame REFLECT_101 "simple" share all
 * filtered values), plus an all-integer pass for the uniform-7 variant.  Every field is a partial sum over
 * rows [row_begin,row_end) -- additive across strips; divide by sr_ssim_count / (h*w*cn).  The record
 * is all fp64 (the SSE is an exact integer < 2^53) so a strip owner can all-reduce it as is. */
enum sr_assess_flags { SR_ASSESS_SSE = 1, SR_ASSESS_UNIFORM7 = 2, SR_ASSESS_GAUSS11 = 4, SR_ASSESS_SIMPLE = 8, SR_ASSESS_ALL = 15 };
typedef struct sr_assess_sums {
    double sse;
    double ssim_uniform;
    double ssim_gauss;
    double ssim_simple;
} sr_assess_sums;
SR_API int sr_assess_u8_async(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b,
                              int64_t stride_b, int h, int w, int cn, int gray_shift, double data_range,
                              int row_begin, int row_end, int flags, sr_assess_sums *d_out);
SR_API int sr_assess_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b,
                        int64_t stride_b, int h, int w, int cn, int gray_shift, double data_range,
                        int row_begin, int row_end, int flags, sr_assess_sums *h_out);
/* The same sums taken on the cv2.INTER_CUBIC resize of both images to dst_h x dst_w, sampled on the fly -- the
 * resized images are never written to memory.  One call per scale replaces downsample_bicubic x 2 + PSNR + SSIM of
 * QualityAssessmentModule._evaluate_downsample_comparison (quality_assessment_module.py:518-555, 226-253).
 * a, b: h x w x cn u8; divide by sr_ssim_count(dst_h, dst_w, ...) / (dst_h * dst_w * cn). */
SR_API int sr_assess_resized_u8_async(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b,
                                      int64_t stride_b, int h, int w, int cn, int dst_h, int dst_w,
                                      int gray_shift, double data_range, int flags, sr_assess_sums *d_out);
SR_API int sr_assess_resized_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b,
                                int64_t stride_b, int h, int w, int cn, int dst_h, int dst_w, int gray_shift,
                                double data_range, int flags, sr_assess_sums *h_out);
/* number of SSIM-map samples of `mode` inside rows [row_begin,row_end) (host only) */
SR_API int sr_ssim_count(int h, int w, int mode, int row_begin, int row_end, uint64_t *count);
/* Per-cell quality map (csrc/sr_qmap.hip; no reference counterpart: the reference's UI shows a difference heat-map it never
 * computes).  The squared error and the SSIM maps of sr_assess_u8, binned into the cells of a separable grid given as two
 * strictly increasing host edge lists h_xedges[0..gw] (0 .. w) and h_yedges[0..gh] (0 .. h): cell (gy, gx) is rows
 * [ye[gy], ye[gy+1]) x columns [xe[gx], xe[gx+1]).  A cell is a bin for results, not a crop of the input -- the filters read
 * across cell boundaries -- so the cells add up to the global sums: sse exactly, the SSIM sums up to the order of the fp64
 * additions.  h_out: gh * gw records, row-major; sse = the exact sum of (a - b)^2 over the cell's pixels and channels, each
 * ssim_* = the fp64 sum of that variant's SSIM-map samples whose position lies in the cell and in the variant's valid region
 * (uniform-7: cropped by 3, gauss-11: by 5, simple: the whole map); fields not selected by `flags` (sr_assess_flags) are 0,
 * a cell without a valid sample has sum 0.  Divide by sr_quality_map_counts / the cell's pixels * cn.  No floating-point
 * atomics: equal inputs give equal bits.  Synchronous; the workspace (about h / 128 + gh rows of w 8-byte words per selected
 * sum) is allocated and freed inside.  SR_ERR_INVALID_ARG for edges that are not strictly increasing or do not span the side,
 * gw or gh < 1, cn not 1 or 3, unknown flag bits; every argument is checked before any device work. */
typedef struct sr_quality_cell {
    uint64_t sse;
    double ssim_uniform;
    double ssim_gauss;
    double ssim_simple;
} sr_quality_cell;
SR_API int sr_quality_map_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b,
                             int h, int w, int cn, int gray_shift, double data_range, const int *h_xedges, int gw,
                             const int *h_yedges, int gh, int flags, sr_quality_cell *h_out);
/* number of valid SSIM-map samples of `mode` per cell, in closed form (host only): counts[gh * gw], row-major; their total
 * is sr_ssim_count(h, w, mode, 0, h) */
SR_API int sr_quality_map_counts(int h, int w, int mode, const int *h_xedges, int gw, const int *h_yedges, int gh,
                                 uint64_t *counts);
/* ---- multi-scale SSIM (csrc/sr_msssim.hip; Wang, Simoncelli, Bovik 2003) ------------------------------------------------
 * No reference counterpart: the reference's 'ms_ssim' report key is its single-scale Gaussian SSIM under another name
 * (sr_ssim_u8 mode SR_SSIM_GAUSS11), and stays that.  This is the real thing, defined as follows.
 * Inputs: two u8 images of h x w with cn = 1 or 3 (3: grayed with the OpenCV fixed-point rule of sr_ssim_u8, gray_shift 15 or
 * 14).  L levels, 1 <= L <= 5, weights w_0 .. w_{L-1} (default: the first L of 0.0448, 0.2856, 0.3001, 0.2363, 0.1333).
 *   planes   x_0, y_0 = the gray images; x_{j+1} = the 2 x 2 mean of x_j, floor(h_j / 2) x floor(w_j / 2): a last odd row or
 *            column is dropped.  The pooling is EXACT: a level-j value is (sum of 4^j u8 values) / 4^j, the sums (<= 255 * 256
 *            = 65280 at j = 4, which is why L stops at 5) are kept as 16-bit integers and nothing ever rounds.
 *   terms    per level the Gaussian window of 11 taps, sigma 1.5 (the taps of SR_SSIM_GAUSS11), valid region only -- the map
 *            is (h_j - 10) x (w_j - 10) --, population covariance, C1 = (0.01 R)^2, C2 = (0.03 R)^2 with R = data_range,
 *            float64 throughout:  l = (2 ux uy + C1) / (ux^2 + uy^2 + C1),  cs = (2 sxy + C2) / (sx^2 + sy^2 + C2),
 *            S_j = mean(l cs), CS_j = mean(cs).  (The kernels work on the integer sums with C1, C2 scaled by 16^j, which
 *            leaves l and cs unchanged up to rounding at the 1e-16 level.)
 *   value    prod_{j < L-1} max(CS_j, 0)^{w_j} * max(S_{L-1}, 0)^{w_{L-1}}, in float64 on the host with pow(); a negative
 *            mean clamps to 0, so the product is then exactly 0.0.
 *   sizes    every level needs h_j, w_j >= 11, i.e. both sides >= 11 * 2^(L-1) (176 for L = 5); a smaller image is
 *            SR_ERR_SHAPE naming the minimum -- the level count is never silently reduced.
 * Pinned: with L = 1 and w = (1) this is scikit-image's Gaussian SSIM (tests/golden/metrics_skimage.npz), and every S_j equals
 * scikit-image 0.18.3 on the exactly pooled float64 planes (tests/golden/msssim_skimage.npz).  scikit-image does not expose
 * cs, so CS_j rests on the NumPy restatement in tests/_msssim_ref.py alone.  PARITY UNPINNED with pytorch-msssim and
 * TensorFlow's ssim_multiscale: neither is available offline, and they differ from this definition (and from each other) in
 * how they pad odd sides before pooling. */
typedef struct sr_ms_ssim_level {
    double sum_lcs;     /* sum of l * cs over the level's map */
    double sum_cs;      /* sum of cs */
    uint64_t count;     /* map samples, (h_j - 10) * (w_j - 10) */
} sr_ms_ssim_level;
/* Host only, no context: per-level sizes and map sample counts (arrays of `levels` entries, each may be NULL) and the bytes
 * of context scratch a call will hold.  SR_ERR_INVALID_ARG for levels outside 1..5, SR_ERR_SHAPE for a too-small image. */
SR_API int sr_ms_ssim_plan(int h, int w, int levels, int *level_h, int *level_w, uint64_t *counts, size_t *scratch_bytes);
/* One launch per level; level 0 reads both images once (2 * cn bytes / pixel) and writes the level-1 sums (4 bytes per
 * level-1 pixel).  Strides in bytes, arbitrary (>= a row).  h_out: `levels` records.  Per-block partial sums are added in a
 * fixed order, no floating-point atomics: equal inputs give equal bits.  Synchronous.  The level planes and partials are
 * context scratch, grown on demand (about h * w / 3 * 4 bytes).  Refused before any device call: null pointers, a stride
 * shorter than a row (SR_ERR_SHAPE), cn not 1 or 3, gray_shift not 14 or 15, data_range not finite and positive, levels
 * outside 1..5, a too-small image (SR_ERR_SHAPE). */
SR_API int sr_ms_ssim_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                         int cn, int gray_shift, double data_range, int levels, sr_ms_ssim_level *h_out);
/* The value formula above on the records of sr_ms_ssim_u8 (host only); weights: `levels` doubles, or NULL for the default.
 * NaN (and sr_last_error) for a null record list, levels outside 1..5 or a level without samples. */
SR_API double sr_ms_ssim_value(const sr_ms_ssim_level *out, int levels, const double *weights);
/* The pooled planes the context's last completed sr_ms_ssim_u8 call left in its scratch, for inspection: the exact integer
 * sums of 4^level gray values of level 1 <= level < levels of that call, h_x / h_y dense (h >> level) x (w >> level). */
SR_API int sr_ms_ssim_planes(sr_ctx *ctx, int level, uint16_t *h_x, uint16_t *h_y);
/* ---- SR-benchmark PSNR / SSIM (csrc/sr_srbench.hip) -----------------------------------------------------------------------
 * The two numbers the papers and model cards of the SR networks quote: PSNR and SSIM on the BT.601 luma (Y) channel with a
 * border of `scale` pixels cropped -- BasicSR's calculate_psnr / calculate_ssim(crop_border, test_y_channel=True) and the
 * MATLAB evaluation scripts before it.  No reference counterpart.  PARITY UNPINNED with BasicSR: the package is not available
 * offline.  Known distance: BasicSR rounds Y to float32 on the way; measured on the CPU at four sizes, that moves its PSNR
 * by about 1e-6 dB and its SSIM by about 1e-8 against this definition.
 * Inputs: two u8 images of h x w x cn, strides in bytes.  crop_border = cb >= 0: both images are first cropped to rows
 * [cb, h - cb) and columns [cb, w - cb), ch x cw.  Both sides must be at least 11 after the crop, else SR_ERR_SHAPE naming
 * the minimum; nothing is silently reduced.
 *   planes   SR_BENCH_CHANNELS  cn = 1 or 3: the channels as they are (cn planes)
 *            SR_BENCH_Y         cn = 3: one plane Y = 16 + (65.481 R + 128.553 G + 24.966 B) / 255, carried EXACTLY as the
 *                               integer X = 65481 R + 128553 G + 24966 B + 4080000, Y = X / 255000, X <= 59 925 000 < 2^26;
 *                               X X' and X^2 + X'^2 are below 2^53, exact in float64: nothing rounds before the filter
 *            SR_BENCH_Y_ROUND   cn = 3: one u8 plane floor((2 X + 255000) / 510000): MATLAB's uint8 rgb2ycbcr (round half
 *                               up), which the older tables used
 *   PSNR     sse = the sum over planes and pixels of the squared plane difference in gray-level units: an exact integer in
 *            CHANNELS and Y_ROUND, sum (X - X')^2 / 255000^2 in Y (each (X - X')^2 and each thread's sum of them an exact
 *            integer; the fp64 additions of the final tree and the one division round).
 *            psnr = 10 log10(R^2 / (sse / n_elems)), inf for sse == 0; R = data_range.
 *   SSIM     per plane the Gaussian window of 11 taps, sigma 1.5 (the taps of SR_SSIM_GAUSS11), valid region only -- the
 *            map is (ch - 10) x (cw - 10) --, population covariance, C1 = (0.01 R)^2, C2 = (0.03 R)^2, float64 throughout;
 *            the value is the mean over the maps of all planes, ssim_sum / n_map.  Every SSIM term is a ratio homogeneous
 *            of degree 0 in (planes, C1, C2), so in SR_BENCH_Y the kernel filters the integers X with C1, C2 multiplied
 *            by 255000^2 (as sr_ms_ssim_u8 does with 16^j).
 * Pinned: all three modes by scikit-image 0.18.3 (structural_similarity(gaussian_weights=True, sigma=1.5,
 * use_sample_covariance=False, data_range=255) and peak_signal_noise_ratio on the float64 planes;
 * tests/golden/srbench_skimage.npz) and by the NumPy restatement tests/_srbench_ref.py. */
enum sr_bench_mode { SR_BENCH_CHANNELS = 0, SR_BENCH_Y = 1, SR_BENCH_Y_ROUND = 2 };
typedef struct sr_bench_sums {
    double sse;         /* see PSNR above */
    double ssim_sum;    /* sum of the SSIM maps of all planes */
    uint64_t n_elems;   /* ch * cw * planes */
    uint64_t n_map;     /* (ch - 10) * (cw - 10) * planes */
} sr_bench_sums;
/* Host only, no context: the cropped size, both counts and the bytes of context scratch a call will hold (each output may
 * be NULL).  Carries every shape refusal: SR_ERR_INVALID_ARG for cn not 1 or 3, an unknown mode, a Y mode with cn = 1,
 * crop_border < 0, h or w < 1; SR_ERR_SHAPE for a side below 11 after the crop. */
SR_API int sr_bench_plan(int h, int w, int cn, int crop_border, int mode, int *ch, int *cw, uint64_t *n_elems, uint64_t *n_map,
                         size_t *scratch_bytes);
/* One launch, one pass over both images for sse and the SSIM sum.  The crop is pointer arithmetic; pixels are read byte by
 * byte, so no alignment is assumed.  Per-block partial sums are added in a fixed order, no floating-point atomics: equal
 * inputs give equal bits.  Synchronous; the partials are context scratch, grown on demand.  Refused before any device call:
 * null pointers, data_range not finite and positive, everything sr_bench_plan refuses, a stride shorter than a row of the
 * uncropped image (SR_ERR_SHAPE). */
SR_API int sr_bench_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                       int cn, int crop_border, int mode, double data_range, sr_bench_sums *h_out);
/* ---- VIF and GMSD, two classical full-reference metrics (csrc/sr_vif.hip, csrc/sr_gmsd.hip, csrc/sr_vif_host.cpp) -----------
 * VIF: Sheikh and Bovik's visual information fidelity in the pixel-domain multi-scale form of MATLAB's vifp_mscale.m ("VIFp").
 * GMSD: Xue, Zhang, Mou and Bovik's gradient magnitude similarity deviation, the authors' GMSD.m.  No reference counterpart.
 * PARITY UNPINNED for both: MATLAB, piq and pyiqa are not available offline, and both definitions below are recalled from the
 * published scripts; they are pinned by the NumPy / SciPy restatements tests/_vif_ref.py and tests/_gmsd_ref.py alone.  Known
 * distances: piq and pyiqa feed a differently rounded Y; for GMSD they divide by N where GMSD.m's std2 divides by N - 1; the
 * widely copied Python port of vifp_mscale filters with ndimage.gaussian_filter and reflection instead of valid windows,
 * which is a different definition.
 * Inputs and planes (both metrics): two u8 images of h x w x cn, strides in bytes, and crop_border = cb >= 0: rows [cb, h - cb),
 * columns [cb, w - cb), as sr_bench_u8.  One plane per image, in gray-level units 0 .. 255 (both metrics hold absolute
 * constants in those units: unlike SSIM neither is scale-free):
 *   cn = 1, SR_BENCH_CHANNELS   the plane as it is
 *   cn = 3, SR_BENCH_Y          X / 255000 with X = 65481 R + 128553 G + 24966 B + 4080000, an exact integer below 2^26
 *   cn = 3, SR_BENCH_Y_ROUND    floor((2 X + 255000) / 510000)
 * Anything else is SR_ERR_INVALID_ARG, cn = 3 with SR_BENCH_CHANNELS included.
 * VIF.  a is the reference and b the distorted image: the metric is not symmetric.  For scale s = 1 .. 4, N = 2^(5 - s) + 1 =
 * 17, 9, 5, 3 and the window W is fspecial('gaussian', N, N / 5): the outer product of the 1-D taps exp(-(k - c)^2 /
 * (2 sigma^2)), c = (N - 1) / 2, sigma = N / 5, normalised by their sum (fspecial's eps truncation never bites for these four).
 * For s > 1 both planes are first filtered with THAT scale's window over the valid region only and every second sample is
 * kept, from index 0 on both axes.  On the scale's planes x, y, all over the valid region: mu1 = W*x, mu2 = W*y,
 * s1 = W*(x x) - mu1^2, s2 = W*(y y) - mu2^2, s12 = W*(x y) - mu1 mu2; then, in this order: s1, s2 < 0 -> 0;
 * g = s12 / (s1 + 1e-10); sv = s2 - g s12; where s1 < 1e-10: g = 0, sv = s2, s1 = 0; where s2 < 1e-10: g = 0, sv = 0; where
 * g < 0: sv = s2, g = 0; sv <= 1e-10 -> 1e-10.  num_s = sum log10(1 + g^2 s1 / (sv + 2)), den_s = sum log10(1 + s1 / 2)
 * (sigma_nsq = 2); the value is sum_s num_s / sum_s den_s, NaN when the denominators sum to 0 (a flat reference: MATLAB's
 * 0 / 0).  Identical images give a value within 1e-11 of 1, not 1, because of the 1e-10 terms.  Sizes: the scale-1 map is
 * (H - 16) x (W - 16); the scale-2 plane is ceil((H - 8) / 2) on a side and its map 8 less; scale 3: ceil((h2 - 4) / 2), map 4
 * less; scale 4: ceil((h3 - 2) / 2), map 2 less.  Both cropped sides must be at least 41 (one sample at scale 4), else
 * SR_ERR_SHAPE naming the minimum; the scale count is never reduced.  Everything is float64; the filter is evaluated
 * separably, columns first (against the 2-D window that moves num_s by up to 1.9e-12 and den_s by up to 3.5e-12 relative over
 * the shapes of tests/test_gpu_vif.py, measured on an MI355X).
 * GMSD.  avg = conv2(P, ones(2) / 4, 'same'): the mean of P(i .. i + 1, j .. j + 1) with ZERO beyond the last row and column;
 * avg(1:2:end, 1:2:end) is kept, ceil(H / 2) x ceil(W / 2).  Prewitt gradients dx = [1 0 -1; 1 0 -1; 1 0 -1] / 3, dy = dx',
 * conv2(., ., 'same') with a zero border; m = sqrt(Ix^2 + Iy^2); q = (2 m1 m2 + 170) / (m1^2 + m2^2 + 170); the score is
 * std2(q), the standard deviation with the N - 1 divisor.  The record carries d = 1 - q = (m1 - m2)^2 / (m1^2 + m2^2 + 170):
 * the deviation of d is that of q, and summing d avoids the cancellation of a mean near 1.  The 2 x 2 sums and the Prewitt
 * sums are exact integers in every mode; m^2 = (Sx^2 + Sy^2) / 144 rounds once in the plane and Y_ROUND modes and twice in
 * SR_BENCH_Y (the 64-bit integer can pass 2^53 on its way to float64, then the division).  Identical images give exactly 0.  Both cropped sides must be
 * at least 4, else SR_ERR_SHAPE. */
typedef struct sr_vif_scale {
    double num, den;    /* num_s, den_s */
    uint64_t count;     /* samples of the scale's map */
} sr_vif_scale;
typedef struct sr_gmsd_sums {
    double sum_d, sum_d2;   /* sum of d and of d^2 over the half-size map */
    uint64_t count;         /* ceil(ch / 2) * ceil(cw / 2) */
} sr_gmsd_sums;
/* Host only, no context: the plane sizes and map sample counts of the four scales and the bytes of context scratch a call
 * will hold (each output may be NULL; the arrays take 4 entries).  Carries every shape and argument refusal above. */
SR_API int sr_vif_plan(int h, int w, int cn, int crop_border, int mode, int *scale_h, int *scale_w, uint64_t *counts,
                       size_t *scratch_bytes);
/* Host only: the N normalised 1-D taps of scale 1 .. 4 (N = 17, 9, 5, 3). */
SR_API int sr_vif_window(int scale, double *taps);
/* The four scales' sums, h_out[4].  The crop is pointer arithmetic; pixels are read byte by byte, so no alignment is assumed;
 * strides are arbitrary (at least a row).  Per-block partial sums are added in a fixed order, no floating-point atomics: equal
 * inputs give equal bits.  Synchronous; the planes of scales 2 .. 4 and the partials are context scratch, grown on demand.
 * Refused before any device call: null pointers, everything sr_vif_plan refuses, a stride shorter than a row of the uncropped
 * image (SR_ERR_SHAPE). */
SR_API int sr_vif_u8(sr_ctx *ctx, const uint8_t *d_ref, int64_t stride_ref, const uint8_t *d_dist, int64_t stride_dist, int h,
                     int w, int cn, int crop_border, int mode, sr_vif_scale *h_out);
/* sum num_s / sum den_s of the 4 records (host only); NaN for a flat reference, and NaN with sr_last_error for a null list
 * or scales != 4. */
SR_API double sr_vif_value(const sr_vif_scale *out, int scales);
/* Host only: the half-size map, its sample count and the scratch bytes of a GMSD call; every shape and argument refusal. */
SR_API int sr_gmsd_plan(int h, int w, int cn, int crop_border, int mode, int *map_h, int *map_w, uint64_t *count,
                        size_t *scratch_bytes);
/* One launch, one pass over both images; conventions and refusals as sr_vif_u8. */
SR_API int sr_gmsd_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                      int cn, int crop_border, int mode, sr_gmsd_sums *h_out);
/* sqrt((sum_d2 - sum_d^2 / n) / (n - 1)), 0 when rounding takes the variance below 0 (host only); NaN with sr_last_error for
 * a null record or fewer than 2 samples. */
SR_API double sr_gmsd_value(const sr_gmsd_sums *sums);
/* ---- FSIM and FSIMc, the phase-congruency feature similarity (csrc/sr_fsim.hip, csrc/sr_fsim_host.cpp) ------------------------
 * Zhang, Zhang, Mou and Zhang, TIP 2011, in the form of the authors' FeatureSIM.m.  No reference counterpart.
 * PARITY UNPINNED: MATLAB, piq and pyiqa are not available offline; the definition below is recalled from the published
 * scripts and pinned by the NumPy restatement tests/_fsim_ref.py alone.  Known distance, rounding-level: MATLAB forms Y, I, Q
 * and the pooling mean in double with a rounding each, here they are exact integers until one division.
 * Inputs: two u8 images of equal shape h x w x cn, cn = 1, 3 (RGB) or 4 (alpha ignored), strides in bytes.  Both sides must be
 * at least 16 (SR_ERR_SHAPE).  Nothing is cropped.  The metric is symmetric in its two arguments.
 *   planes   carried exactly as integers: Y 1000 = 299 R + 587 G + 114 B, I 1000 = 596 R - 274 G - 322 B, Q 1000 = 211 R -
 *            523 G + 312 B.  cn = 1: Y 1000 = 1000 v and the I and Q records are 0, which gives S_i = S_q = 1 exactly as the
 *            script's I = Q = 1 does: FSIMc = FSIM.
 *   pooling  F = max(1, floor(min(h, w) / 256 + 0.5)); each plane is filtered by the F x F mean as conv2(., 'same') with a
 *            zero border and sampled at 0, F, 2F, ...: rows x cols = ceil(h / F) x ceil(w / F).  0-based, the window of sample
 *            i along an axis covers the source indices i F + floor(F / 2) - F + 1 .. i F + floor(F / 2); indices outside the
 *            image contribute 0 and the divisor is always F^2.  The record is the int64 window sum; the division by 1000 F^2
 *            happens once, in float64.  The pooled long side must be at most 2048 and F at most 256 (SR_ERR_UNSUPPORTED).
 *   PC       Kovesi's phasecong2 as FSIM ships it, of each pooled Y: 4 scales, 4 orientations, minWaveLength 6, mult 2,
 *            sigmaOnf 0.55, dThetaOnSigma 1.2, k 2, epsilon 1e-4.  Grid along an axis of length n: odd n (-(n-1)/2 .. (n-1)/2)
 *            / (n-1), even n (-n/2 .. n/2-1) / n; radius = sqrt(x^2 + y^2), theta = atan2(-y, x), both ifftshifted;
 *            radius[0,0] = 1 for the log-Gabor only.  lp = 1 / (1 + (r / 0.45)^30) on the radius with 0 at DC;
 *            logGabor_s = exp(-ln(radius / fo_s)^2 / (2 ln(0.55)^2)) lp, fo_s = 1 / (6 2^s), s = 0..3, logGabor_s[0,0] = 0;
 *            spread_o = exp(-dtheta^2 / (2 ts^2)), ts = pi / 4 / 1.2, angl = o pi / 4, ds = sin(theta) cos(angl) - cos(theta)
 *            sin(angl), dc = cos(theta) cos(angl) + sin(theta) sin(angl), dtheta = |atan2(ds, dc)|.  Per orientation o:
 *            EO_s = ifft2(fft2(Y) logGabor_s spread_o) = E_s + i O_s, An_s = |EO_s|; sumE, sumO, sumAn over s;
 *            XEnergy = sqrt(sumE^2 + sumO^2) + epsilon, MeanE = sumE / XEnergy, MeanO = sumO / XEnergy;
 *            Energy = sum_s (E_s MeanE + O_s MeanO - |E_s MeanO - O_s MeanE|); medianE2n = MATLAB's median of |EO_0|^2 over
 *            the plane (the mean of the two middle values for an even count); noisePower = (-medianE2n / ln 0.5) / EM_n,
 *            EM_n = sum filter_{0,o}^2; tau = sqrt((2 noisePower S2 + 4 noisePower Sij) / 2); T = (tau sqrt(pi / 2) +
 *            2 sqrt((2 - pi / 2) tau^2)) / 1.7; EnergyAll += max(Energy - T, 0), AnAll += sumAn; PC = EnergyAll / AnAll.
 *            S2 = sum_s sum_px a_s^2, Sij = sum_{s<t} sum_px a_s a_t with a_s = real(ifft2(filter_{s,o})) sqrt(rows cols); by
 *            Parseval sum_px a_s a_t = sum_u g_s(u) g_t(u), g(u) = (f(u) + f(-u)) / 2 with wrap-around, so EM_n, S2 and Sij
 *            depend on (rows, cols) alone and are host work without a transform.
 *            The transform is a float64 dense DFT in two passes (products added in ascending index order with fma, against a
 *            table (cos, sin)(2 pi ((u r) mod n) / n) whose index is reduced in integers); the first sample of the plane is
 *            subtracted from every sample before it (the filters are 0 at DC), so a flat plane gives AnAll = 0 exactly.
 *   G        Scharr dx = [3 0 -3; 10 0 -10; 3 0 -3] / 16, dy = dx', on the pooled Y by conv2(., 'same') with a zero border;
 *            G = sqrt(Ix^2 + Iy^2).
 *   score    S_pc = (2 PC1 PC2 + 0.85) / (PC1^2 + PC2^2 + 0.85), S_g = (2 G1 G2 + 160) / (G1^2 + G2^2 + 160), PCm =
 *            max(PC1, PC2); S_i, S_q the same form on the pooled I, Q with 200.  FSIM = sum(S_g S_pc PCm) / sum PCm;
 *            FSIMc = sum(S_g S_pc Re((S_i S_q)^0.03) PCm) / sum PCm, where a negative S_i S_q = z has the real part
 *            |z|^0.03 cos(0.03 pi).  Identical images give 1 to 1e-12; a flat image has AnAll = 0 and the value is NaN, as
 *            MATLAB's is. */
typedef struct sr_fsim_sums {
    double sum_s;       /* sum S_g S_pc PCm */
    double sum_sc;      /* sum S_g S_pc Re((S_i S_q)^0.03) PCm */
    double sum_pcm;     /* sum PCm */
    uint64_t count;     /* rows * cols */
    int32_t F, rows, cols, reserved;
} sr_fsim_sums;
/* Host only, no context: F, the pooled size and the bytes of context workspace a call will hold (each output may be NULL).
 * Carries every refusal that depends on the shape: SR_ERR_INVALID_ARG for cn not 1, 3 or 4 or h, w < 1; SR_ERR_SHAPE for a
 * side below 16; SR_ERR_UNSUPPORTED, naming the cap, for a pooled side above 2048 or F above 256. */
SR_API int sr_fsim_plan(int h, int w, int cn, int *F, int *rows, int *cols, size_t *workspace_bytes);
/* Host only, for inspection: logGabor_s (log_gabor[4][rows * cols]) and spread_o (spread[4][rows * cols]), both as the
 * transform indexes them (DC first), and EM_n, S2, Sij of the four orientations (em, s2, sij: 4 each).  Each output may be
 * NULL.  rows, cols outside 16 .. 2048: SR_ERR_SHAPE below, SR_ERR_UNSUPPORTED above. */
SR_API int sr_fsim_filters(int rows, int cols, double *log_gabor, double *spread, double *em, double *s2, double *sij);
/* Inspection entry of the pooling with an EXPLICIT F in 1 .. 256 and no minimum side: h_out[2][3][rows * cols] takes the
 * int64 window sums of Y 1000, I 1000, Q 1000 of a, then of b, rows x cols = ceil(h / F) x ceil(w / F).  One pass: every
 * source byte is read at most once.  Synchronous.  Refused before any device call: null pointers, cn not 1, 3 or 4, h or
 * w < 1, F outside 1 .. 256 (SR_ERR_INVALID_ARG), a stride shorter than a row (SR_ERR_SHAPE). */
SR_API int sr_fsim_pool_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                           int cn, int F, int64_t *h_out);
/* PC of one dense float64 device plane of rows x cols into the dense device plane d_pc, plus the four orientations'
 * medianE2n (h_median[4]) and thresholds T (h_T[4]; either may be NULL).  Synchronous; equal inputs give equal bits.
 * Refusals as sr_fsim_filters, and null pointers. */
SR_API int sr_fsim_pc_f64(sr_ctx *ctx, const double *d_plane, int rows, int cols, double *d_pc, double *h_median, double *h_T);
/* The record of the three sums of the pair.  Strides are arbitrary (at least a row); pixels are read byte by byte, so no
 * alignment is assumed.  Integer histograms select the medians and fixed trees add the sums, no floating-point atomics: equal
 * inputs give equal bits.  Synchronous; the workspace belongs to the context and grows on demand.  Refused before any device
 * call: null pointers, everything sr_fsim_plan refuses, a stride shorter than a row (SR_ERR_SHAPE). */
SR_API int sr_fsim_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                      int cn, sr_fsim_sums *h_out);
/* Host only: *fsim = sum_s / sum_pcm, *fsimc = sum_sc / sum_pcm (either may be NULL); NaN for a flat pair (0 / 0) and when a
 * sum is NaN.  SR_ERR_INVALID_ARG for a null record. */
SR_API int sr_fsim_value(const sr_fsim_sums *sums, double *fsim, double *fsimc);
/* Host only: Re((s_i s_q)^0.03), the chroma weight of one sample as the score kernel forms it. */
SR_API double sr_fsim_chroma_weight(double s_i, double s_q);
/* ---- VSI, the visual saliency-induced index with SDSP saliency (csrc/sr_vsi.hip, csrc/sr_vsi_host.cpp, csrc/sr_vsi.h) ---------
 * Zhang, Shen and Li, TIP 2014, in the form of the authors' VSI.m with SDSP.m (Zhang, Gu and Li, ICIP 2013).  No reference
 * counterpart.  PARITY UNPINNED: MATLAB, piq and pyiqa are not available offline; the definition below is recalled from the
 * published scripts (the constants agree with piq's defaults) and pinned by the NumPy restatement tests/_vsi_ref.py alone.
 * Known distances, rounding-level: L, M, N and the pooling mean are exact integers until one division; the pooled saliency is
 * formed from the 256 x 256 map by composite per-axis tables (below) instead of from a stored full-resolution map; the
 * up-resize applies its horizontal pass first whatever the scales.  Where max VS = min VS MATLAB's mat2gray returns the
 * clamped map; here the value is NaN.
 * Inputs: two u8 images of equal shape h x w x cn, cn = 3 (RGB) or 4 (alpha ignored), strides in bytes.  Both sides must be at
 * least 16 (SR_ERR_SHAPE); cn = 1 is SR_ERR_UNSUPPORTED (VSI is defined for colour images: with R = G = B the a and b ranges
 * are rounding residue of the XYZ matrix); F above 256 is SR_ERR_UNSUPPORTED.  Nothing is cropped.  The metric is symmetric.
 *   resize   imresize(., 'bilinear') by the contribution rule of the imresize section above with the triangle t(x) = max(0,
 *            1 - |x|) in place of the cubic and support 2 in place of 4: scale = n_out / n_in; kw = 2 / scale and weights
 *            scale t(scale d) when scale < 1, else kw = 2; P = ceil(kw) + 2 taps, u = (i + 1) / scale + 0.5 (1 - 1 / scale),
 *            left = floor(u - kw / 2); weights normalised by their sum; symmetric reflection at the border; any scale; nothing
 *            is rounded between the passes; the axis with the smaller scale first, a tie vertical first.
 *   SDSP     of each image on a fixed 256 x 256 grid, float64.  R, G, B as double resized to 256 x 256.  Lab by the script's
 *            own RGB2Lab: v = x / 255, v <= 0.04045 ? v / 12.92 : ((v + 0.055) / 1.055)^2.4; X = 0.4124564 R + 0.3575761 G +
 *            0.1804375 B, Y = 0.2126729 R + 0.7151522 G + 0.0721750 B, Z = 0.0193339 R + 0.1191920 G + 0.9503041 B; X / 0.950456,
 *            Z / 1.088754; f(t) = cbrt(t) above 0.008856, else 7.787 t + 16 / 116; L = 116 f_Y - 16, a = 500 (f_X - f_Y), b =
 *            200 (f_Y - f_Z).  (Not sr_delta_e's Lab: another matrix and white point.)  Log-Gabor: u1 = (c - 128) / 256, u2 =
 *            (r - 128) / 256 for 0-based r, c, both 0 where u1^2 + u2^2 > 0.25, ifftshifted; radius = sqrt(u1^2 + u2^2),
 *            radius[0,0] = 1; LG = exp(-ln(radius / 0.021)^2 / (2 1.34^2)), 0 where the radius is 0; LG[0,0] = 0.
 *            SF = sqrt(sum_{p in L,a,b} real(ifft2(fft2(p) LG))^2); SD = exp(-((r + 1 - 128)^2 + (c + 1 - 128)^2) / 145^2);
 *            SC = 1 - exp(-(a_n^2 + b_n^2) / 0.001^2), a_n = (a - min a) / (max a - min a) over the grid, b_n likewise (a flat
 *            a or b is 0 / 0: the value is NaN); VS256 = SF SD SC.  The transform is FSIM's dense float64 DFT (the plane's
 *            first sample subtracted first: LG is 0 at DC).
 *   VS       imresize(VS256, [h w], 'bilinear') by the same rule (a side below 256 is a shrink with its wider kernel), then
 *            mat2gray: (VS - min VS) / (max VS - min VS) over all h w samples; max = min gives NaN.
 *   planes   carried exactly as integers: L 100 = 6 R + 63 G + 27 B, M 100 = 30 R + 4 G - 35 B, N 100 = 34 R - 60 G + 17 B.
 *   pooling  FSIM's: F = max(1, floor(min(h, w) / 256 + 0.5)), the F x F mean as conv2(., 'same') with a zero border sampled
 *            at 0, F, 2F, ...; L, M, N as int64 window sums divided once by 100 F^2; VS with zeros outside the image and the
 *            divisor F^2.  Resize, mat2gray and the mean are linear and separable, so the pooled VS is (C_y VS256 C_x' - min VS
 *            cover) / (max VS - min VS) / F^2, where row i of C_y adds the up-resize rows of the in-image part of window i and
 *            cover counts the in-image samples of a window; only min VS and max VS visit every sample.
 *   score    G = Scharr (FSIM's dx, dy) on the pooled L; sim(u, v, k) = (2 u v + k) / (u^2 + v^2 + k); S_vs = sim(VS1, VS2,
 *            1.27), S_g = sim(G1, G2, 386), S_c = sim(M1, M2, 130) sim(N1, N2, 130), VSm = max(VS1, VS2);
 *            VSI = sum(S_g^0.4 S_vs Re(S_c^0.02) VSm) / sum VSm, a negative S_c = z contributing |z|^0.02 cos(0.02 pi).
 *            Identical images give 1 to 1e-12. */
typedef struct sr_vsi_sums {
    double sum_s;           /* sum S_g^0.4 S_vs Re(S_c^0.02) VSm */
    double sum_w;           /* sum VSm */
    uint64_t count;         /* rows * cols */
    int32_t F, rows, cols, reserved;
    double a_range[2][2];   /* per image: min, max of a on the 256 x 256 grid */
    double b_range[2][2];   /* ... of b */
    double vs_range[2][2];  /* ... of the full-resolution VS before mat2gray */
} sr_vsi_sums;
/* Host only, no context: F, the pooled size and the bytes of context workspace a call will hold (each output may be NULL).
 * Carries every refusal that depends on the shape: SR_ERR_INVALID_ARG for cn not 1, 3 or 4 or h, w < 1; SR_ERR_UNSUPPORTED
 * for cn = 1 and, naming the cap, for F above 256 or more pooled rows than one launch covers; SR_ERR_SHAPE for a side below 16. */
SR_API int sr_vsi_plan(int h, int w, int cn, int *F, int *rows, int *cols, size_t *workspace_bytes);
/* Host only, for inspection: LG (as the transform indexes it, DC first) and SD, 65536 values each; either may be NULL. */
SR_API int sr_vsi_filter(double *lg, double *sd);
/* Host only, for inspection: one axis of the triangle resize n_in -> n_out.  *taps takes the tap count; when w and idx are
 * given (both or neither) they take w[n_out][taps] and the reflected 0-based idx[n_out][taps], cap being the taps there is
 * room for.  SR_ERR_INVALID_ARG for sides below 1, a null taps, one of w and idx alone, or too small a cap. */
SR_API int sr_vsi_resize_weights(int n_in, int n_out, int cap, int *taps, double *w, int32_t *idx);
/* Inspection entry of the pooling with an EXPLICIT F in 1 .. 256 and no minimum side: h_out[2][3][rows * cols] takes the
 * int64 window sums of L 100, M 100, N 100 of a, then of b.  One pass: every source byte is read at most once.  Synchronous.
 * Refused before any device call: null pointers, cn not 1, 3 or 4, h or w < 1, F outside 1 .. 256 (SR_ERR_INVALID_ARG), cn = 1
 * (SR_ERR_UNSUPPORTED), a stride shorter than a row (SR_ERR_SHAPE). */
SR_API int sr_vsi_pool_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                          int cn, int F, int64_t *h_out);
/* Inspection entry of the saliency of ONE image: h_lab[3][65536] (L, a, b on the grid), h_vs256[65536] and h_range[4] (min a,
 * max a, min b, max b); each output may be NULL.  Synchronous.  Refusals as sr_vsi_u8. */
SR_API int sr_vsi_saliency_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, double *h_lab,
                              double *h_vs256, double *h_range);
/* The record of the pair.  Strides are arbitrary (at least a row); pixels are read byte by byte.  Every sum, minimum and maximum
 * goes through a fixed tree, no floating-point atomics: equal inputs give equal bits.  Synchronous; the workspace belongs to
 * the context and grows on demand.  Refused before any device call: null pointers, everything sr_vsi_plan refuses, a stride
 * shorter than a row (SR_ERR_SHAPE). */
SR_API int sr_vsi_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                     int cn, sr_vsi_sums *h_out);
/* Host only: sum_s / sum_w; NaN for 0 / 0, when a sum is NaN, and (with sr_last_error) for a null record. */
SR_API double sr_vsi_value(const sr_vsi_sums *sums);
/* Host only: Re(s_c^0.02), the chroma weight of one sample as the score kernel forms it. */
SR_API double sr_vsi_chroma_weight(double s_c);
/* Host only, no context: the same record from host memory, every stage in the kernels' formulation (sequential sums where the
 * device adds through trees).  Same refusals as sr_vsi_u8. */
SR_API int sr_vsi_host_u8(const uint8_t *a, int64_t stride_a, const uint8_t *b, int64_t stride_b, int h, int w, int cn,
                          sr_vsi_sums *out);
/* ---- colour difference: CIEDE2000 and CIE76 per pixel (csrc/sr_deltae.hip, csrc/sr_deltae_host.cpp, csrc/sr_deltae.h) ---------
 * A full-reference, per-pixel colour difference of two images, in the arithmetic of scikit-image 0.18.3 (rgb2lab of a uint8
 * image, deltaE_ciede2000 / deltaE_cie76, float64).  PARITY PINNED: tests/golden/deltae_skimage.npz holds scikit-image's own
 * Lab and both difference maps.  NOT the private brand-colour number of the commercial metrics (brand_color_delta_e_i), which
 * compares a region MEAN in OpenCV's 8-bit integer Lab with one colour, by CIE76.
 * Inputs: two u8 images of equal shape h x w x cn, strides in bytes.  cn = 1: gray, used as R = G = B; 3: RGB; 4: RGBA, alpha
 * ignored.  crop_border = cb >= 0: rows [cb, h - cb), columns [cb, w - cb); both cropped sides must be >= 1 (SR_ERR_SHAPE).
 * Lab: v = c / 255; linear = ((v + 0.055) / 1.055)^2.4 where v > 0.04045, else v / 12.92 (the 256 values are a table built
 * once on the host in double); XYZ = M rgb with M = [[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169],
 * [0.019334, 0.119193, 0.950227]], each row summed left to right; divided by the D65 / 2 degree white (0.95047, 1, 1.08883);
 * f(t) = cbrt(t) where t > 0.008856, else 7.787 t + 16 / 116; L = 116 f(y) - 16, a = 500 (f(x) - f(y)), b = 200 (f(y) - f(z)).
 * With this matrix only black has a = b = 0 exactly: a gray pixel keeps a small chroma (about 1e-3), as the definition gives it.
 * SR_DELTA_E_76: sqrt(dL^2 + da^2 + db^2).
 * SR_DELTA_E_2000 (kL = kC = kH = 1): Cbar = (hypot(a1, b1) + hypot(a2, b2)) / 2, c7 = Cbar^7,
 * G = (1 - sqrt(c7 / (c7 + 25^7))) / 2; a' = a (1 + G); C' = hypot(a', b); h = atan2(b, a') moved into [0, 2 pi);
 * Lbar = (L1 + L2) / 2, SL = 1 + 0.015 (Lbar - 50)^2 / sqrt(20 + (Lbar - 50)^2), L_term = (L2 - L1) / SL;
 * Cbar' = (C1' + C2') / 2, SC = 1 + 0.045 Cbar', C_term = (C2' - C1') / SC; h_diff = h2 - h1, h_sum = h1 + h2;
 * dH = h_diff, - 2 pi where h_diff > pi, + 2 pi where h_diff < -pi (STRICT comparisons), 0 where C1' C2' == 0;
 * dH_term = 2 sqrt(C1' C2') sin(dH / 2); Hbar = h_sum, + 2 pi (h_sum < 2 pi) or - 2 pi (otherwise) only where C1' C2' != 0 and
 * |h_diff| > pi, then halved -- except where C1' C2' == 0, where Hbar is the SUM of the two hues;
 * T = 1 - 0.17 cos(Hbar - 30 deg) + 0.24 cos(2 Hbar) + 0.32 cos(3 Hbar + 6 deg) - 0.20 cos(4 Hbar - 63 deg);
 * SH = 1 + 0.015 Cbar' T, H_term = dH_term / SH; Rc = 2 sqrt(c7' / (c7' + 25^7)) with c7' = Cbar'^7;
 * dtheta = 30 deg * exp(-((Hbar in degrees - 275) / 25)^2); R = -sin(2 dtheta) Rc C_term H_term;
 * dE = sqrt(max(L_term^2 + C_term^2 + H_term^2 + R, 0)).  Where scikit-image and Sharma, Wu and Dalal's note differ this
 * follows scikit-image: the sum (not the mean) of the hues where a chroma is 0, and the strict comparisons at |h_diff| = pi.
 * hypot is evaluated as sqrt(x^2 + y^2) and the 7th power by multiplication.  A pixel pair with equal bytes gives EXACTLY 0
 * for both formulas (the arithmetic is skipped).  Out of scope: kL / kC / kH other than 1, CIE94 and CMC (any other formula
 * value is SR_ERR_UNSUPPORTED), other illuminants, float and 16-bit inputs.
 * The record over the cropped rectangle: count; sum and sum2 of dE; max; hist: bin min(floor(16 dE), 2047) -- width 1 / 16,
 * the last bin open (sRGB extremes reach dE00 of about 106.7, so 128 covers them).  No floating-point atomics, integer ones
 * only (the histogram); partial sums are combined in a fixed order that depends on the size alone: equal inputs give equal
 * bits. */
#define SR_DELTA_E_BINS 2048
enum sr_delta_e_formula { SR_DELTA_E_2000 = 0, SR_DELTA_E_76 = 1 };
typedef struct sr_delta_e_sums {
    uint64_t count;
    double sum, sum2, max;
    uint64_t hist[SR_DELTA_E_BINS];
} sr_delta_e_sums;
typedef struct sr_delta_e_cell {
    double sum, max;
} sr_delta_e_cell;
/* Host only, no context: the cropped size, the pixel count, the blocks of the sums launch and the bytes of context scratch a
 * call will hold (each output may be NULL).  Carries every refusal that depends on these arguments: SR_ERR_INVALID_ARG for
 * cn not 1, 3 or 4, crop_border < 0, h or w < 1; SR_ERR_UNSUPPORTED for an unknown formula; SR_ERR_SHAPE for a side below 1
 * after the crop. */
SR_API int sr_delta_e_plan(int h, int w, int cn, int crop_border, int formula, int *crop_h, int *crop_w, uint64_t *count,
                           int *blocks, size_t *scratch_bytes);
/* Host only: the 256 linear values of the sRGB bytes, as the kernels index them. */
SR_API int sr_delta_e_table(double *table256);
/* Host only: the Lab of one sRGB pixel, and the difference of two Labs by `formula`, restating the definition in float64 (the
 * same expressions the kernels evaluate; arbitrary Lab values are taken as they are, nothing is skipped). */
SR_API int sr_delta_e_lab_u8(int r, int g, int b, double *lab3);
SR_API int sr_delta_e_pair(const double *lab1, const double *lab2, int formula, double *out);
/* The record of the pair.  d_map (may be NULL): float64, map_stride bytes per row (a multiple of 8, at least 8 cw; the pointer
 * 8-byte aligned), receives the dE of every cropped pixel, ch x cw.  The crop is pointer arithmetic; pixels are read byte by
 * byte; strides are arbitrary (at least a row).  Synchronous; the table, the histogram and the per-block partials are context
 * scratch, grown on demand.  Refused before any device call: null pointers, everything sr_delta_e_plan refuses, a stride
 * shorter than a row of the uncropped image (SR_ERR_SHAPE), a misaligned or short map stride (SR_ERR_INVALID_ARG /
 * SR_ERR_SHAPE). */
SR_API int sr_delta_e_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                         int cn, int crop_border, int formula, double *d_map, int64_t map_stride, sr_delta_e_sums *h_out);
/* Per cell of a separable grid, as sr_quality_map_u8 takes it: strictly increasing host edge lists h_xedges[0..gw] (0 .. cw)
 * and h_yedges[0..gh] (0 .. ch) over the CROPPED rectangle.  h_out: gh * gw records, row-major: the sum and the largest dE of
 * the cell's pixels.  dE is pointwise, so the cell sums add up to the record's sum within the order of fp64 additions and the
 * largest cell max equals the record's max exactly; a cell's pixel count is its area.  Refused before any device call:
 * everything sr_delta_e_u8 refuses, edges that are not strictly increasing or do not span the cropped side
 * (SR_ERR_INVALID_ARG), and what one launch does not cover (SR_ERR_UNSUPPORTED, naming the cap): more than 2^24 - 1 cells, more
 * than 2^24 - 1 row chunks (cell rows in pieces of 64 rows), more than 65535 * 256 columns. */
SR_API int sr_delta_e_cells_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
                               int w, int cn, int crop_border, int formula, const int *h_xedges, int gw, const int *h_yedges,
                               int gh, sr_delta_e_cell *h_out);
/* Host only.  mean = sum / count; rms = sqrt(sum2 / count); NaN with sr_last_error for a null record or count 0. */
SR_API double sr_delta_e_mean(const sr_delta_e_sums *sums);
SR_API double sr_delta_e_rms(const sr_delta_e_sums *sums);
/* Host only: for p in (0, 100], k = max(1, ceil(p count / 100)), j = the first bin whose cumulative count reaches k; the
 * result is the bin's LOWER edge j / 16 (the true percentile lies in [j / 16, (j + 1) / 16); identical images give 0).  NaN
 * with sr_last_error for a null record, count 0, p outside (0, 100] or a histogram that does not add up to count. */
SR_API double sr_delta_e_percentile(const sr_delta_e_sums *sums, double p);
/* Host only: the fraction of pixels with dE >= t, exact from the histogram, for t a multiple of 1 / 16 in [0, 128); any other
 * t is SR_ERR_INVALID_ARG. */
SR_API int sr_delta_e_fraction_at_least(const sr_delta_e_sums *sums, double t, double *fraction);
/* ---- HaarPSI, the Haar wavelet perceptual similarity index (csrc/sr_haarpsi.hip, csrc/sr_haarpsi_host.cpp, csrc/sr_haarpsi.h) --
 * Reisenhofer, Bosse, Kutyniok and Wiegand 2018, a full-reference metric; larger is better, 1 for identical images.  No
 * reference counterpart.  PARITY: the SR_HAARPSI_PYTHON convention is pinned through SciPy's own convolve2d(mode='same'), the
 * call the authors' Python script makes (tests/_haarpsi_ref.py).  The SR_HAARPSI_MATLAB convention and the constants are
 * recalled from the published scripts; MATLAB, piq and pyiqa are not available offline: PARITY UNPINNED.  Known distance,
 * rounding level: the scripts form Y, I and Q in double with a rounding each, here they are exact integers until one division
 * (measured on the CPU against tests/_haarpsi_ref.py: at most 2.6e-14 relative over the sums and the value).
 * Inputs: two u8 images of equal shape h x w x cn (ref, dist), strides in bytes.  cn = 1: gray; 3: RGB; 4: RGBA, alpha ignored.
 * crop_border = cb >= 0: rows [cb, h - cb), columns [cb, w - cb), ch x cw; both cropped sides must be >= 2 (SR_ERR_SHAPE).
 * Constants: C = 30, alpha = 4.2, three scales (nothing else is built).
 * Planes, exact integers x 1000: Y = 299 R + 587 G + 114 B, I = 596 R - 274 G - 322 B, Q = 211 R - 523 G + 312 B; gray: Y = 1000 v
 * and no chroma.
 * Window-centre convention o: SR_HAARPSI_MATLAB (o = 0) is conv2(., k, 'same'), where an even kernel's window looks forward;
 * SR_HAARPSI_PYTHON (o = 1) is scipy.signal.convolve2d(., k, mode='same'), whose centre sits one sample earlier.  The two
 * official scripts differ here and so do their values (1e-3 .. 1e-2 on small images).  Samples outside a plane are ZERO.
 * Subsampling (subsample = 1): every plane P becomes pool[i, j] = sum P[2 i - o + {0, 1}, 2 j - o + {0, 1}], i < ceil(ch / 2),
 * j < ceil(cw / 2), unit div = 4000; subsample = 0: the planes as they are, div = 1000.  mh x mw samples either way.
 * Haar sums of the luma plane, scale s = 1, 2, 3, hf = 2^(s - 1), at sample (i, j):
 *   V_s = sum over columns j - o - hf + 1 .. j - o + hf of (rows i - o - hf + 1 .. i - o) - (rows i - o + 1 .. i - o + hf),
 *   H_s the transposed window; both int32 (below 3.4e7 in magnitude); the coefficient is |.| / (div 2^s), rounded once.
 * Chroma (cn >= 3): c_I = |sum of I over (i - o .. i - o + 1, j - o .. j - o + 1)| / (4 div), c_Q likewise.
 * Per sample and orientation d in {V, H}, a from ref and b from dist: w_d = max(a_3, b_3),
 * LS_d = (sim(a_1, b_1) + sim(a_2, b_2)) / 2 with sim(a, b) = (2 a b + C) / (a^2 + b^2 + C).  Colour adds
 * LS_c = (sim(c_I) + sim(c_Q)) / 2 with w_c = (w_V + w_H) / 2.
 * Per channel (V, H and, for colour, c): num = sum w / (1 + exp(-alpha LS)), den = sum w, float64.  x = sum num / sum den,
 * HaarPSI = (ln(x / (1 - x)) / alpha)^2.  Symmetric; 1 within 1e-12 (not exactly) for identical images; NaN when every weight
 * is 0 (a black pair) -- a flat non-black pair gives 1, the zero border makes the rim coefficients non-zero.
 * No floating-point atomics; partial sums are combined in a fixed order that depends on the size alone: equal inputs give equal
 * bits.  Out of scope, refused or absent by name: other C / alpha / scale counts, float and 16-bit inputs, MDSI. */
enum sr_haarpsi_convention { SR_HAARPSI_MATLAB = 0, SR_HAARPSI_PYTHON = 1 };
typedef struct sr_haarpsi_sums {
    double num[3], den[3];      /* V, H, colour (0 for gray) */
    int32_t channels;           /* 2 (gray) or 3 */
    int32_t reserved;
    uint64_t count;             /* samples: mh * mw */
} sr_haarpsi_sums;
typedef struct sr_haarpsi_cell {
    double num, den;            /* summed over the channels */
} sr_haarpsi_cell;
/* Host only, no context: the sample map, its count, the blocks of the launch and the bytes of context scratch of an
 * sr_haarpsi_u8 call (each output may be NULL).  Carries every refusal that depends on these arguments: SR_ERR_INVALID_ARG for
 * cn not 1, 3 or 4, crop_border < 0, h or w < 1, subsample not 0 or 1, an unknown convention; SR_ERR_SHAPE for a side below 2
 * after the crop (the message names the minimum) and for more samples than one launch covers. */
SR_API int sr_haarpsi_plan(int h, int w, int cn, int crop_border, int subsample, int convention, int *map_h, int *map_w,
                           uint64_t *count, int *blocks, size_t *scratch_bytes);
/* The record of the pair.  The crop is pointer arithmetic; pixels are read byte by byte; strides are arbitrary (at least a
 * row) and 64-bit.  Synchronous; the per-block partials are context scratch, grown on demand.  Refused before any device call:
 * null pointers, everything sr_haarpsi_plan refuses, a stride shorter than a row of the uncropped image (SR_ERR_SHAPE). */
SR_API int sr_haarpsi_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                         int cn, int crop_border, int subsample, int convention, sr_haarpsi_sums *h_out);
/* Per cell of a separable grid with the argument rules of sr_delta_e_cells_u8: strictly increasing host edge lists
 * h_xedges[0..gw] (0 .. cw) and h_yedges[0..gh] (0 .. ch) over the CROPPED rectangle, in pixels.  h_out: gh * gw records,
 * row-major.  A sample belongs to the cell that holds cropped pixel (2 i, 2 j), or (i, j) without subsampling; a cell that
 * holds no sample has den = 0.  The cells add up to the record's sums over the channels within the order of fp64 additions.
 * The per-sample (num, den) pairs (16 bytes a sample) are context scratch.  Refused before any device call: everything
 * sr_haarpsi_u8 refuses, edges that are not strictly increasing or do not span the cropped side (SR_ERR_INVALID_ARG), more than
 * 2^24 - 1 cells (SR_ERR_UNSUPPORTED). */
SR_API int sr_haarpsi_cells_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
                               int w, int cn, int crop_border, int subsample, int convention, const int *h_xedges, int gw,
                               const int *h_yedges, int gh, sr_haarpsi_cell *h_out);
/* Host only: the value of a record, and of one cell's sums; NaN for den == 0 (and, with sr_last_error, for a null record). */
SR_API double sr_haarpsi_value(const sr_haarpsi_sums *sums);
SR_API double sr_haarpsi_cell_value(double num, double den);
/* Host only: the float64 restatement of the definition on HOST memory (direct window sums, the per-sample expressions the
 * kernel evaluates, samples added in row-major order).  Same refusals as sr_haarpsi_u8. */
SR_API int sr_haarpsi_host_u8(const uint8_t *a, int64_t stride_a, const uint8_t *b, int64_t stride_b, int h, int w, int cn,
                              int crop_border, int subsample, int convention, sr_haarpsi_sums *out);
/* ---- NIQE, the no-reference quality model (csrc/sr_niqe.hip, csrc/sr_niqe_host.cpp) -------------------------------------------
 * Mittal, Soundararajan, Bovik 2013, in the arithmetic of MATLAB's computequality / estimatemodelparam and BasicSR's
 * calculate_niqe, made exact wherever it can be.  The reference's calculate_niqe asks pyiqa for this model first; the 'niqe'
 * key of the reports is its MSCN fallback heuristic and is NOT this number.  The model needs a 36-value mean and a 36 x 36
 * covariance of "pristine" features: the caller supplies them (nothing is fetched), or fits them with sr_niqe_fit.
 * PARITY UNPINNED with BasicSR, pyiqa and MATLAB: none of them is available offline, and neither is niqe_pris_params.npz.
 * Known distances, unmeasured here, both rounding-level: BasicSR scales by / 255 ... * 255 around the resize where the plane
 * here is exact, and it convolves with the 2-D window in one scipy.ndimage.convolve where the filter here is separable.
 * All arithmetic is float64 without contraction.
 *   plane    cn = 3 (RGB): MATLAB's u8 luma, SR_BENCH_Y_ROUND's floor((2 X + 255000) / 510000) with X = 65481 R + 128553 G +
 *            24966 B + 4080000 (BasicSR rounds Y before NIQE); cn = 1: the plane as it is.  crop_border pixels per side are
 *            cropped by pointer arithmetic (h' x w'), then the top-left H = 96 floor(h' / 96) by W = 96 floor(w' / 96) is kept:
 *            nby x nbx blocks.  A side below 96 after the crop is SR_ERR_SHAPE.
 *   scale 2  MATLAB imresize(., 0.5): bicubic, a = -0.5, antialiased.  At scale 1/2 every output has the same eight taps
 *            0.5 cubic(0.25, 0.75, 1.25, 1.75) = {-3, -9, 29, 111, 111, 29, -9, -3} / 256 (they sum to 1); output i reads
 *            inputs 2 i - 3 .. 2 i + 4, indices reflect symmetrically (j < 0 -> -j - 1, j >= n -> 2 n - 1 - j), rows first,
 *            then columns.  The input is an integer plane, so 65536 x the result is an exact integer k, |k| < 2^25: the half
 *            plane is kept as int32, nothing rounds and no summation order matters.
 *   MSCN     per scale, window of 7 taps g_i = exp(-i^2 / (2 s^2)), s = 7 / 6, k_i = g_i / sum g (computed on the host),
 *            separable: horizontal pass, then vertical pass, in each the taps added in ascending index order; the border
 *            replicates (scipy.ndimage 'nearest').  mu = G * I, sigma = sqrt(|G * I^2 - mu^2|), m = (I - mu) / (sigma + 1); I in
 *            gray levels at both scales (scale 2: I = k / 65536, I^2 exact in float64).
 *   blocks   96 / scale on a side: both scales have the same nby x nbx blocks.  X_0 = m and X_s = m * roll(m, shift_s) for the
 *            shifts (dy, dx) = (0, 1), (1, 0), (1, 1), (1, -1), roll(b, (dy, dx))[i, j] = b[(i - dy) mod n, (j - dx) mod n]:
 *            circular INSIDE the block, as np.roll on the block is.  A record holds, per X, the counts of X < 0 and X > 0, the
 *            sums of X^2 over each and the sum of |X|; and the block's sum of sigma.  Fixed-order sums, no floating-point
 *            atomics: equal inputs give equal bits.
 *   features AGGD fit of a record's moments: ls = sqrt(ssq_neg / n_neg), rs = sqrt(ssq_pos / n_pos), g = ls / rs,
 *            r = (sabs / n)^2 / ((ssq_neg + ssq_pos) / n), R = r (g^3 + 1)(g + 1) / (g^2 + 1)^2; alpha = the entry of
 *            gam = 0.2 + 0.001 t, t = 0 .. 9800, that minimises (Gamma(2 / gam)^2 / (Gamma(1 / gam) Gamma(3 / gam)) - R)^2
 *            (the first on a tie); beta_l = ls sqrt(Gamma(1 / alpha) / Gamma(3 / alpha)), beta_r likewise.  Per scale 18 values:
 *            [alpha_0, (beta_l0 + beta_r0) / 2], then per shift [alpha, (beta_r - beta_l) Gamma(2 / alpha) / Gamma(1 / alpha),
 *            beta_l, beta_r]; scale 1 then scale 2: 36.  A fit with n_neg = 0 or n_pos = 0 gives NaN.
 *   score    mu_d = the per-feature mean over non-NaN entries, cov_d = the sample covariance (ddof 1) over blocks without a
 *            NaN, S = (cov_pris + cov_d) / 2, S+ = the pseudo-inverse of the symmetric S by eigen-decomposition, eigenvalues
 *            with |l| <= 1e-15 max |l| dropped (numpy pinv's default); NIQE = sqrt((mu_pris - mu_d) S+ (mu_pris - mu_d)^T).
 *   fit      per image sharp_b = sum_sigma_b(scale 1) / 96^2; blocks with sharp_b > T max_b sharp_b are kept (T = 0.75 in
 *            the paper); the kept, NaN-free 36-rows of all images are pooled: mu_pris their mean, cov_pris their sample
 *            covariance.  Fewer than 37 rows is refused. */
typedef struct sr_niqe_moments {
    uint64_t n_neg, n_pos;      /* counts of X < 0, X > 0 */
    double ssq_neg, ssq_pos;    /* sums of X^2 over each */
    double sabs;                /* sum of |X| */
} sr_niqe_moments;
typedef struct sr_niqe_block {
    sr_niqe_moments x[5];       /* X_0 = m, then the four shifted products in the order above */
    double sum_sigma;           /* the block's sum of sigma */
} sr_niqe_block;
/* Host only, no context: the kept size, the block grid and the bytes of context scratch a call will hold (each output may be
 * NULL).  Carries every shape refusal: SR_ERR_INVALID_ARG for cn not 1 or 3, crop_border < 0, h or w < 1; SR_ERR_SHAPE for a
 * side below 96 after the crop. */
SR_API int sr_niqe_plan(int h, int w, int cn, int crop_border, int *H, int *W, int *nby, int *nbx, size_t *scratch_bytes);
/* One read of the image for the half plane, then one workgroup per block and scale.  h_out: 2 nby nbx records, scale-major
 * (scale 1's blocks row-major, then scale 2's).  Strides in bytes, arbitrary (>= a row).  Synchronous; the half plane and the
 * records are context scratch, grown on demand.  Refused before any device call: null pointers, everything sr_niqe_plan
 * refuses, a stride shorter than a row of the uncropped image (SR_ERR_SHAPE). */
SR_API int sr_niqe_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int crop_border,
                      sr_niqe_block *h_out);
/* The half plane (65536 x the scale-2 plane, dense (H / 2) x (W / 2)) the context's last completed sr_niqe_u8 call left in its
 * scratch, for inspection. */
SR_API int sr_niqe_half_plane(sr_ctx *ctx, int32_t *h_out);
/* Host only.  records: 2 nblocks records, scale-major, as sr_niqe_u8 writes them; feat36: nblocks x 36. */
SR_API int sr_niqe_features(const sr_niqe_block *records, int64_t nblocks, double *feat36);
/* Host only.  feat: the pooled rows of n_images images, image i owning rows [image_off[i], image_off[i + 1]); sharp: sharp_b
 * per row.  mu: 36, cov: 36 x 36; *rows_used (may be NULL) is always set once the arguments are valid.  SR_ERR_INVALID_ARG for
 * null pointers, n_images < 1, offsets that do not ascend from 0, T not in [0, 1); SR_ERR_SHAPE, giving the count, for fewer
 * than 37 kept rows. */
SR_API int sr_niqe_fit(const double *feat, const double *sharp, const int64_t *image_off, int n_images, double T, double *mu,
                       double *cov, int64_t *rows_used);
/* Host only.  The score of nblocks feature rows under (mu_pris[36], cov_pris[36 x 36]); NaN (and sr_last_error) for null
 * pointers or fewer than two NaN-free rows. */
SR_API double sr_niqe_score(const double *feat, int64_t nblocks, const double *mu_pris, const double *cov_pris);
/* ---- BRISQUE, the no-reference quality model (csrc/sr_brisque.hip, csrc/sr_brisque_host.cpp) ----------------------------------
 * Mittal, Moorthy, Bovik 2012, in the arithmetic of MATLAB's brisque_feature.m / brisquescore.m and pyiqa's brisque, made
 * exact wherever it can be.  The reference's calculate_brisque asks pyiqa for this model first; the 'brisque' key of the
 * reports is its fallback heuristic and is NOT this number.  The model is an RBF epsilon-SVR over 36 scaled features: the
 * caller supplies it (nothing is fetched and none ships).
 * PARITY UNPINNED with MATLAB, pyiqa and piq: none of them is available offline, and neither are allmodel / allrange.  Known
 * distances, unmeasured here: pyiqa scales by / 255 ... * 255 around the resize where the plane here is exact; the 2-D window
 * is applied in one pass elsewhere and is separable here; an implementation that replicates the border instead of
 * zero-padding differs in a 3-pixel rim.  OpenCV's QualityBRISQUE (non-antialiased bicubic, non-circular shifts) is a
 * different definition and out of scope.  The flat-neighbourhood caveat of NIQE applies unchanged: where a 7 x 7
 * neighbourhood is exactly flat, G * I^2 - mu^2 is rounding noise of either sign and m with it.
 * All arithmetic is float64 without contraction.
 *   plane    cn = 3: NIQE's luma (SR_BENCH_Y_ROUND's formula); cn = 1: the plane as it is.  crop_border pixels per side are
 *            cropped by pointer arithmetic, giving H x W; the whole crop is used (no multiple-of-96 rule).  H < 16 or W < 16
 *            after the crop is SR_ERR_SHAPE: scale 2 (at least 8 x 8) still holds a whole 7-tap window.
 *   scale 2  NIQE's imresize(., 0.5): taps {-3, -9, 29, 111, 111, 29, -9, -3} / 256, output i reads inputs 2 i - 3 .. 2 i + 4,
 *            symmetric reflection (one reflection reaches every index once a side is >= 16), rows first, then columns.  The
 *            output is H2 = ceil(H / 2) by W2 = ceil(W / 2), MATLAB's output size; it is kept as int32 = 65536 x the value,
 *            exact.
 *   MSCN     NIQE's window k_i, separable: horizontal pass, then vertical pass, taps added in ascending index order.  The
 *            border is ZERO, as in MATLAB's filter2(window, I, 'same'): a tap outside the plane contributes an exact 0.
 *            mu, sigma = sqrt(|G * I^2 - mu^2|), m = (I - mu) / (sigma + 1) as for NIQE.
 *   products X_0 = m and X_s = m * roll(m, shift_s) for the shifts (0, 1), (1, 0), (1, 1), (1, -1), NIQE's order and roll
 *            convention, but circular over the WHOLE plane of that scale.  MATLAB's fourth shift is (-1, 1); under a circular
 *            roll m * roll(m, (-1, 1)) is roll(m * roll(m, (1, -1)), (-1, 1)): the same multiset of products, the same moments.
 *   record   per scale n = H_s W_s and five sr_niqe_moments.  Counts are exact.  Sums: per-workgroup partials into context
 *            scratch, then one fixed tree over them whose shape depends on the call shape only.  No floating-point atomics:
 *            equal inputs give equal bits.
 *   features 18 per scale, scale 1 then scale 2.  X_0, a GGD fit: s2 = (ssq_neg + ssq_pos) / n, E = sabs / n, alpha = the
 *            entry of gam = 0.2 + 0.001 t, t = 0 .. 9800, that minimises |Gamma(1 / gam) Gamma(3 / gam) / Gamma(2 / gam)^2 -
 *            s2 / E^2| (the first on a tie): [alpha, s2], NaN for sabs = 0.  Each shift: NIQE's AGGD fit (same table, same
 *            argmin; n counts every element, zeros included; ls, rs as there): [alpha, (rs - ls) (Gamma(2 / alpha) /
 *            Gamma(1 / alpha)) (sqrt(Gamma(1 / alpha)) / sqrt(Gamma(3 / alpha))), ls^2, rs^2], NaN for n_neg = 0 or n_pos = 0.
 *   score    x_k = lower + (upper - lower)(f_k - min_k) / (max_k - min_k), not clamped; x_k = 0 where max_k = min_k (svm-scale
 *            drops such a feature).  score = sum_i coef_i exp(-gamma sum_k (sv_ik - x_k)^2) - rho, support vectors and
 *            features ascending.  NaN for any NaN feature. */
typedef struct sr_brisque_record {
    uint64_t n;                 /* H_s * W_s */
    sr_niqe_moments x[5];       /* X_0 = m, then the four shifted products in the order above */
} sr_brisque_record;
/* Host only, no context: the cropped size, the half plane's size and the bytes of context scratch a call will hold (each
 * output may be NULL).  Carries every shape refusal: SR_ERR_INVALID_ARG for cn not 1 or 3, crop_border < 0, h or w < 1;
 * SR_ERR_SHAPE for a side below 16 after the crop. */
SR_API int sr_brisque_plan(int h, int w, int cn, int crop_border, int *H, int *W, int *H2, int *W2, size_t *scratch_bytes);
/* One read of the image for the half plane, then one launch per scale: a workgroup owns a 64 x 64 tile of m.  h_out: two
 * records, scale 1 then scale 2.  Strides in bytes, arbitrary (>= a row).  Synchronous; the half plane and the partials are
 * context scratch, grown on demand.  Refused before any device call: null pointers, everything sr_brisque_plan refuses, a
 * stride shorter than a row of the uncropped image (SR_ERR_SHAPE). */
SR_API int sr_brisque_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int crop_border,
                         sr_brisque_record *h_out);
/* The half plane (65536 x the scale-2 plane, dense H2 x W2) the context's last completed sr_brisque_u8 call left in its
 * scratch, for inspection. */
SR_API int sr_brisque_half_plane(sr_ctx *ctx, int32_t *h_out);
/* Host only.  records: the two records of sr_brisque_u8; feat36: 36 values. */
SR_API int sr_brisque_features(const sr_brisque_record *records, double *feat36);
/* Host only.  sv: n_sv x 36 row-major, coef: n_sv, fmin / fmax: 36.  NaN (and sr_last_error) for null pointers, n_sv < 1, a
 * gamma that is not finite and positive; NaN for any NaN feature. */
SR_API double sr_brisque_score(const double *feat36, const double *sv, const double *coef, int64_t n_sv, double gamma, double rho,
                               const double *fmin, const double *fmax, double lower, double upper);
/* cv2.cvtColor(RGB2GRAY) on u8 (quality_assessment_module.py:359-360) */
SR_API int sr_rgb2gray_u8(sr_ctx *ctx, const uint8_t *d_rgb, int64_t stride, int h, int w,
                          int gray_shift, uint8_t *d_gray, int64_t gray_stride);
/* cv2.resize(..., INTER_CUBIC) on u8 (downsample_bicubic :226-253; also the benchmark's SR stub) */
SR_API int sr_resize_cubic_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w,
                              int cn, uint8_t *d_dst, int64_t dst_stride, int dh, int dw);
/* Same sampling, but only the dst window [x0,x0+ww) x [y0,y0+wh) of the virtual dh x dw result is
 * produced (dense, stride dst_stride): the SR stub's per-tile form. */
SR_API int sr_resize_cubic_window_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h,
                                     int w, int cn, int dh, int dw, int x0, int y0, int ww, int wh,
                                     uint8_t *d_dst, int64_t dst_stride);
/* ---- MATLAB imresize, bicubic (csrc/sr_imresize.hip, csrc/sr_imresize_host.cpp) -----------------------------------------------
 * imresize(A, scale) / imresize(A, [dh dw]) with the 'bicubic' kernel: MATLAB's imresize.m / contributions, the form BasicSR's
 * matlab_functions.imresize restates -- the degradation every classical SR benchmark is defined on ("HR, downscaled by
 * imresize(hr, 1 / s), run through the network, compared with the HR").  NOT sr_resize_cubic_u8, which is OpenCV's INTER_CUBIC
 * (a = -0.75, four taps whatever the scale, no antialiasing).  No reference counterpart.  PARITY UNPINNED with MATLAB and BasicSR:
 * neither is available offline.  Anchors: at scale 1/2 the definition is NIQE's exact half plane above; away from the border
 * it agrees with torch's F.interpolate(mode='bicubic', antialias=True, align_corners=False) in float64 (torch clamps at the
 * border, MATLAB reflects); tests/_imresize_ref.py restates it in NumPy.  Known distance: BasicSR scales by / 255 ... * 255
 * around the resize where v here is in gray levels, a rounding-level difference.
 * Per axis of input length n and output length m:
 *   sizes    scalar scale: m = ceil(n * scale) evaluated in double exactly as written (MATLAB's answer, its floating-point
 *            trap included: ceil(100 * 0.07) is 8) and both axes use `scale` itself; output size: the axis scale is m / n in
 *            double.
 *   kernel   cubic(x), a = -0.5: 1.5 |x|^3 - 2.5 |x|^2 + 1 for |x| <= 1, -0.5 |x|^3 + 2.5 |x|^2 - 4 |x| + 2 for 1 < |x| <= 2,
 *            else 0.  Kernel width kw = 4 / scale when scale < 1 and antialiasing is on, else 4; P = ceil(kw) + 2 taps.
 *   output i (0-based): u = (i + 1) / scale + 0.5 (1 - 1 / scale), left = floor(u - kw / 2); tap k = 0 .. P - 1 reads the
 *            1-based index left + k with weight scale * cubic(scale * (u - left - k)) when antialiased below 1, else
 *            cubic(u - left - k); the weights of an output are divided by their sum, taken in ascending k, in float64.
 *   border   symmetric reflection as MATLAB writes it: 0-based j = (idx - 1) mod 2 n, then j >= n -> 2 n - 1 - j; an image
 *            shorter than the kernel wraps more than once.
 *   order    the axis with the smaller scale goes first, on a tie the vertical pass (along the height), as in MATLAB and
 *            BasicSR.  Both passes are float64 without contraction, taps added in ascending k; the first pass's result stays
 *            float64 (the im2double -> imresize -> im2uint8 protocol of the dataset scripts: no intermediate u8 rounding).
 *   outputs  v in gray levels.  SR_IMRESIZE_U8: min(255, max(0, floor(v + 0.5))); SR_IMRESIZE_F32: v rounded to float32, not
 *            clamped; SR_IMRESIZE_F64: v itself, not clamped (inspection and tests).
 * Ranges: u8 input, cn 1, 3 or 4, sides >= 1, each axis scale in [1/16, 16] (so P <= 66; outside: SR_ERR_UNSUPPORTED naming
 * the range).  Out of scope: the 'bilinear' / 'lanczos' / 'box' kernels, uint16 / float inputs, and MATLAB's uint8-class path
 * with a rounded intermediate (imresize called on a uint8 array directly), which differs from this by +-1 level in places. */
enum sr_imresize_out { SR_IMRESIZE_U8 = 0, SR_IMRESIZE_F32 = 1, SR_IMRESIZE_F64 = 2 };
/* Host only: ceil(n * scale), or a negative SR_ERR_* (n < 1: SR_ERR_INVALID_ARG; a scale outside [1/16, 16] or not finite:
 * SR_ERR_UNSUPPORTED). */
SR_API int sr_imresize_size(int n, double scale);
/* Host only: the normalised weights and the reflected 0-based indices of one axis.  Leading and trailing taps whose weight is
 * zero for every output are dropped (no value changes): *taps is what is left, and w / idx (both or neither may be NULL) are
 * dense n_out x *taps, room for n_out x cap.  n_out must be ceil(n_in * scale) or scale must be n_out / n_in, else
 * SR_ERR_INVALID_ARG; as is cap < *taps (with *taps set). */
SR_API int sr_imresize_weights(int n_in, int n_out, double scale, int antialias, int cap, int *taps, double *w, int32_t *idx);
/* Host only, no context: the pass order (*order 0: vertical pass first, 1: horizontal first), the tap counts, the output tile
 * of one workgroup (tile_h x tile_w), its LDS bytes and the bytes of context scratch (the tables) a call will hold; each
 * output may be NULL.  Carries every shape refusal of sr_imresize_u8: SR_ERR_INVALID_ARG for h, w, dh or dw < 1, cn not 1, 3
 * or 4, an axis whose (scale, output length) pair is neither form above; SR_ERR_UNSUPPORTED for a scale outside [1/16, 16]. */
SR_API int sr_imresize_plan(int h, int w, int cn, double scale_y, double scale_x, int dh, int dw, int antialias, int *order,
                            int *taps_y, int *taps_x, int *tile_h, int *tile_w, size_t *lds_bytes, size_t *scratch_bytes);
/* One launch: a workgroup owns tile_h x tile_w outputs, runs the first pass for exactly the input span they need into LDS
 * (float64) and the second pass out of LDS; no float64 intermediate goes through HBM.  Every output's sum has a fixed order:
 * the result depends neither on the tile geometry nor on strides.  Strides in bytes, arbitrary (>= a row); pixels are read
 * byte by byte and offsets are 64-bit; nothing outside dh x dw x cn elements of the destination is written.  d_dst holds
 * uint8_t, float or double by out_type.  Synchronous; the tables are context scratch, grown on demand.  Refused before any
 * device call: null pointers, everything sr_imresize_plan refuses, an unknown out_type, a stride shorter than a row
 * (SR_ERR_SHAPE), a float / double destination or stride that is not a multiple of the element size. */
SR_API int sr_imresize_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int cn, double scale_y,
                          double scale_x, int antialias, int out_type, void *d_dst, int64_t dst_stride, int dh, int dw);

/* ---- BlendingModule.color_correction (blending_module.py:969-1146) ---------------------------------
 * sr_histogram_u8: per-channel 256-bin histogram (np.histogram(ch, 256, [0, 256]) of u8 data), h_hist = cn x 256 counts.
 * The matching itself is 256-entry bookkeeping on the host (CDFs in float64, argmin; or the mean / std affine map of
 * _mean_std_matching) and arrives here as a per-channel table h_glut[c][v] = corrected float value of source value v.
 * sr_color_correct_u8: out = astype(u8)(clip(corrected, 0, 255)) with corrected = h_glut[c][img]; with local_filter == 1
 * corrected goes through _simple_guided_filter(guide = corrected, src = img, radius, eps) first (:1110-1146: five
 * cv2.blur((radius, radius)) box means -- anchor radius / 2, REFLECT_101 -- and fp32 element-wise algebra); with
 * local_filter == 2 through the cv2.ximgproc.guidedFilter branch of :1108-1111 instead ((2 radius + 1)^2 window,
 * BORDER_REFLECT, colour guide: per-pixel 3 x 3 covariance inverse; 1 or 3 channels; restated, parity unpinned).
 * radius 1..16.  d_out may be d_img (in place).  At the reference's radius 8 with an integer-valued table both branches run as
 * fused kernels (the a / b coefficient planes of branch 1 never leave the CU); branch 1 also with a float table (mean_std)
 * whose first-stage box sums are exact in fp64 -- sr_color_table_class says which; results do not depend on which kernels run.
 * sr_color_table_class (host only): *cls = 1 when every entry of h_glut[cn][256] is a whole number 0..255 (sums slide as
 * 32-bit integers), 2 when a sum of `terms` values of each of g = T[v], fl32(g * v), fl32(g * g) is exact in fp64 whatever
 * the order (all values multiples of 2^lo and below 2^hi with hi + log2(terms) - lo <= 53: sums slide in fp64), else 0
 * (ordered sums, cv::boxFilter's order).  terms = radius^2 for branch 1. */
SR_API int sr_histogram_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, uint64_t *h_hist);
SR_API int sr_color_table_class(const float *h_glut, int cn, int terms, int *cls);
SR_API int sr_color_correct_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn,
                               const float *h_glut, int local_filter, int radius, float eps, uint8_t *d_out,
                               int64_t out_stride);

/* ---- output writers: stage 5 of SuperResolutionPipeline.process (main.py:399-404) -----------------------
 * Host-only (no context, no GPU), multi-threaded (threads <= 0: every hardware thread).  h_img: h x w x cn u8, row stride in
 * bytes.  TIFF: LZW-compressed strips (Pillow compression='tiff_lzw'; BigTIFF above 4 GB); PNG: deflate level `level`
 * (Pillow compress_level=3), filter None; JPEG: baseline YCbCr 4:2:0 (gray for cn 1) with libjpeg's quality scaling,
 * colour conversion, down-sampling, islow DCT and standard Huffman tables (Pillow quality=95 defaults), restart marker per
 * MCU row.  The lossless files decode to the input bytes; the JPEG decodes to what Pillow's own file decodes to. */
SR_API int sr_encode_tiff_lzw(const uint8_t *h_img, int h, int w, int cn, int64_t stride, const char *path, int threads);
SR_API int sr_encode_png(const uint8_t *h_img, int h, int w, int cn, int64_t stride, int level, const char *path, int threads);
SR_API int sr_encode_jpeg(const uint8_t *h_img, int h, int w, int cn, int64_t stride, int quality, const char *path,
                          int threads);

/* ---- LPIPS (quality_assessment_module.py:419-465 calculate_lpips, :197-224 _to_lpips_tensor, :135-146 model init) -------
 * The reference delegates to the package `lpips` (requirements.txt:16): net 'alex' or 'vgg', version 0.1.  Weights are
 * supplied by the caller (nothing is fetched): h_conv_w[i] = i-th convolution of the backbone, dense OIHW fp32,
 * h_conv_b[i] its bias; h_lin_w[k] = the C_k weights of the k-th 1x1 `lin` layer; h_shift / h_scale = ScalingLayer
 * constants (NULL: the package's).  AlexNet has 5 convolutions, VGG16 13.
 * sr_lpips_u8: a, b are h x w x cn u8 images in HBM (cn 1: gray repeated, 4: alpha dropped).  The image is streamed in
 * `tile` x `tile` input tiles (multiple of 16; <= 0: one tile) so a 200 MP image fits; tiles [tile_begin, tile_end) of the
 * row-major tile grid are processed (tile_end < 0: all) -- ranks of a multi-GPU job take disjoint tile ranges and add the
 * sums.  h_layer_sums[k] receives the sum of the k-th tap's lin map over those tiles; LPIPS = sum_k sums[k] / (H_k W_k)
 * with the map sizes from sr_lpips_layer_sizes (h_hw: 5 x (H, W)).
 * sr_lpips_tile_plan (host only, no context): what sr_lpips_u8 works on for tile `tile_index` of the row-major tile grid --
 * the very function the forward calls.  Activation 0 is the image, activation j the output of the j-th convolution / pooling;
 * *n_act receives their number (at most SR_LPIPS_PLAN_MAX_ACT) and h_plan, n_act x SR_LPIPS_PLAN_FIELDS ints, per activation:
 * needed rows [a, b), owned rows [a, b), needed columns [a, b), owned columns [a, b) (indices of the activation's own
 * grid; a tile adds to a tap's sum over its owned ranges and computes its needed ranges), the buffer pitch in floats,
 * channels, and the activation's full height and width.  *buffer_floats: floats each activation buffer is grown to. */
enum sr_lpips_net { SR_LPIPS_ALEX = 0, SR_LPIPS_VGG = 1 };
#define SR_LPIPS_PLAN_MAX_ACT 18
#define SR_LPIPS_PLAN_FIELDS 12
typedef struct sr_lpips_model sr_lpips_model;
SR_API int sr_lpips_create(sr_ctx *ctx, int net, const float *const *h_conv_w, const float *const *h_conv_b, int n_conv,
                           const float *const *h_lin_w, int n_lin, const float *h_shift, const float *h_scale,
                           sr_lpips_model **out);
SR_API int sr_lpips_destroy(sr_lpips_model *model);
SR_API int sr_lpips_layer_sizes(int net, int h, int w, int *h_hw);
SR_API int sr_lpips_tile_count(int h, int w, int tile, int *n_tiles);
SR_API int sr_lpips_tile_plan(int net, int h, int w, int tile, int tile_index, int *n_act, int *h_plan, int64_t *buffer_floats);
SR_API int sr_lpips_u8(sr_lpips_model *model, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b,
                       int h, int w, int cn, int tile, int tile_begin, int tile_end, double *h_layer_sums);

/* ---- DISTS, deep image structure and texture similarity (csrc/sr_dists.hip, csrc/sr_dists_host.cpp) ---------------------------
 * Ding, Ma, Wang, Simoncelli, "Image Quality Assessment: Unifying Structure and Texture Similarity", 2020, restated.  Not in
 * the reference; SR papers report it beside PSNR / SSIM / LPIPS / NIQE.  PARITY UNPINNED: DISTS_pytorch, piq, pyiqa and
 * torchvision are not available offline, and neither are the published alpha / beta.  Known distance to the package,
 * rounding-level: it forms mean / variance / covariance in fp32 with the two-pass form mean((f - mu)^2); here they come from
 * float64 sums.  Weights are supplied by the caller (nothing is fetched, none ship).
 * Inputs: two u8 images of equal shape, cn 1 (gray repeated), 3, or 4 (alpha dropped).  Any h, w >= 1 is valid.
 *   stage 0   x = u8 / 255, three channels, not normalised.
 *   input     (x - mean_c) / std_c in fp32, in that order, tabulated per channel and u8 value; mean = (0.485, 0.456, 0.406),
 *             std = (0.229, 0.224, 0.225) unless given.  Convolution zero padding acts on this normalised value.
 *   stages    1 .. 5: torchvision VGG16's convolutions, 2, 2, 3, 3, 3 of 3 x 3, pad 1, + bias + ReLU; 64, 128, 256, 512, 512
 *             channels; a stage's feature map is its last ReLU.  Each convolution sums in the order csrc/sr_conv_mfma.h
 *             documents (the first: bias, then channels, then taps ascending, as fmaf).
 *   L2 pool   in front of stages 2 .. 5 in place of the max pooling: y(Y, X) = sqrtf(sum_{j,i} g_j g_i x(2Y - 1 + j,
 *             2X - 1 + i)^2 + 1e-12f), g = (1/4, 1/2, 1/4) (hanning(5)[1:-1], outer product, normalised), stride 2, zero
 *             padding 1: the output side is ceil(n / 2).  All fp32: x * x rounded once, the nine terms g_j g_i (x * x) -- exact
 *             products by powers of two -- added in row-major tap order onto 0, then + 1e-12f, then a correctly rounded sqrtf.
 *   sums      per stage and channel (3 + 64 + 128 + 256 + 512 + 512 = 1475, stage 0 first) five float64 sums over the whole
 *             feature map: a, b, a^2, b^2, a b.  Stage 0: exact integers of the u8 values (the / 255 and / 255^2 happen in
 *             sr_dists_score).  Other stages: fp32 features converted to double, products in double, fixed order (inside a
 *             block, blocks ascending, tiles ascending; no floating-point atomics): equal inputs give equal bits.
 *   score     float64, n_k the pixel count of stage k: mu = sum / n, var = sum_sq / n - mu^2, cov = sum_ab / n - mu_a mu_b,
 *             S1 = (2 mu_a mu_b + c1) / (mu_a^2 + mu_b^2 + c1), S2 = (2 cov + c2) / (var_a + var_b + c2), c1 = c2 = 1e-6;
 *             DISTS = 1 - sum_ch (alpha_ch S1_ch + beta_ch S2_ch) / (sum alpha + sum beta).  For a == b every S1 and S2 is
 *             exactly 1 and the value is 1 minus the rounded sum of the normalised weights: |DISTS(a, a)| <= 1e-12, not
 *             necessarily 0.
 * sr_dists_create: h_conv_w[i] = i-th of the 13 convolutions, dense OIHW fp32, h_conv_b[i] its bias; h_mean / h_std: 3 values
 * or NULL for the defaults.  sr_dists_u8 streams the pair in `tile` x `tile` input tiles (multiple of 16; <= 0: one tile),
 * each recomputing its receptive-field halo, zero padding at the true image border only, over tiles [tile_begin, tile_end)
 * of the row-major tile grid (tile_end < 0: all); h_sums (1475 x 5) receives the sums over the tiles' own disjoint parts of
 * every feature map, additive over disjoint tile ranges.  Synchronous.  Refused before any device call: null pointers, cn not
 * 1, 3 or 4, a side below 1, a tile that is no multiple of 16 (SR_ERR_INVALID_ARG), a stride shorter than a row
 * (SR_ERR_SHAPE), a null or destroyed model.
 * sr_dists_l2pool_f32 (inspection): the pooling kernel on a dense planar [C][H][W] fp32 device tensor -> [C][ceil(H / 2)]
 * [ceil(W / 2)].
 * Host only, no context: sr_dists_layer_sizes gives the six (H, W) (stage 0 = the image, stage 1 the same, then ceil
 * halving) as h_hw[12]; sr_dists_score gives the score from sums, those sizes and alpha / beta (1475 each, stage 0 first;
 * finite with a positive total), and S1 / S2 per channel when s1 / s2 are not NULL. */
typedef struct sr_dists_model sr_dists_model;
SR_API int sr_dists_create(sr_ctx *ctx, const float *const *h_conv_w, const float *const *h_conv_b, const float *h_mean,
                           const float *h_std, sr_dists_model **out);
SR_API int sr_dists_destroy(sr_dists_model *model);
SR_API int sr_dists_tile_count(int h, int w, int tile, int *n_tiles);
/* sr_dists_tile_plan (host only, no context): sr_lpips_tile_plan for the DISTS stack -- the same records
 * (SR_LPIPS_PLAN_FIELDS ints per activation, at most SR_LPIPS_PLAN_MAX_ACT activations), the function sr_dists_u8 calls per tile.
 * Stage 0 is activation 0, the image. */
SR_API int sr_dists_tile_plan(int h, int w, int tile, int tile_index, int *n_act, int *h_plan, int64_t *buffer_floats);
SR_API int sr_dists_u8(sr_dists_model *model, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b,
                       int h, int w, int cn, int tile, int tile_begin, int tile_end, double *h_sums);
SR_API int sr_dists_l2pool_f32(sr_ctx *ctx, const float *d_in, int C, int H, int W, float *d_out);
SR_API int sr_dists_layer_sizes(int h, int w, int *h_hw);
SR_API int sr_dists_score(const double *sums, const int *hw, const float *alpha, const float *beta, double *score, double *s1,
                          double *s2);

/* ---- local SR backend: compact "VGG-style" SR network (csrc/sr_srnet.hip) ------------------------------------------------
 * Stage 2 of the reference is a remote API client (main.py:194-267); this is a local learned upscaler of the family
 * Real-ESRGAN ships as SRVGGNetCompact, restated (parity with that package is unpinned: neither it nor a checkpoint exists
 * offline).  Layers k = 0 .. D + 1 are 3 x 3, stride 1, zero padding 1 at the image border, with bias, all fp32:
 * layer 0 maps x = u8 / 255 (3 channels) to F, layers 1 .. D map F to F, each followed by y >= 0 ? y : slope[c] * y, and
 * layer D + 1 maps F to 3 s^2 without activation.  The output is
 *     o[c, Y, X] = t[c s^2 + (Y % s) s + (X % s), Y / s, X / s] + x[c, Y / s, X / s]
 * (PixelShuffle(s) plus the nearest-upsampled input), written as HWC fp32 unclamped (sr_srnet_f32) or as HWC u8
 * rintf(fminf(fmaxf(o, 0), 1) * 255) (sr_srnet_u8).  F in {64, 128, 192, 256}, 0 <= D <= 64, s in {1, 2, 3, 4}; anything
 * else is SR_ERR_UNSUPPORTED, decided on the host before any device call.
 * sr_srnet_create: h_w[k] = weights of layer k, dense OIHW fp32; h_b[k] its bias (k = 0 .. D + 1); h_slope[k] the F slopes
 * after layer k (k = 0 .. D; ReLU is all zeros, LeakyReLU a constant, PReLU learned).  The arrays are re-laid and uploaded.
 * sr_srnet_plan (host only, no context, no GPU): the image is streamed in tile x tile sub-tiles of the INPUT (tile 0: the
 * library's choice, 2048), each recomputing a halo of *halo = D + 2 input pixels; *n_tiles sub-tiles; *workspace_bytes =
 * the model's two planar F-channel fp32 buffers of one padded sub-tile (side min(tile, side) + 2 halo clipped to the image,
 * rows padded to 4 floats).  Outputs may be NULL.
 * sr_srnet_u8 / sr_srnet_f32: d_src h x w x 3 u8, d_dst (h s) x (w s) x 3; strides in bytes (fp32: a multiple of 4).
 * SR_ERR_INVALID_ARG for null pointers and a tile < 0, SR_ERR_SHAPE for h or w < 1, a stride shorter than a row, an output
 * size beyond int or a sub-tile too large for 32-bit offsets -- all before any launch.  Fixed summation order that does not
 * depend on the sub-tile: every tile size gives the same bits.  Asynchronous. */
typedef struct sr_srnet_model sr_srnet_model;
SR_API int sr_srnet_create(sr_ctx *ctx, int n_feat, int n_body, int scale, const float *const *h_w, const float *const *h_b,
                           const float *const *h_slope, sr_srnet_model **out);
SR_API int sr_srnet_destroy(sr_srnet_model *model);
SR_API int sr_srnet_plan(int h, int w, int n_feat, int n_body, int scale, int tile, int *halo, int *n_tiles,
                         size_t *workspace_bytes);
SR_API int sr_srnet_u8(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                       int64_t dst_stride, int tile);
SR_API int sr_srnet_f32(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                        int64_t dst_stride, int tile);

/* ---- local SR backend: residual family, MSRResNet / EDSR (csrc/sr_resnet.hip) ----------------------------------------------
 * BasicSR's MSRResNet (SRResNet without batch norm) and EDSR (baseline and large), restated (parity with that package is
 * unpinned: neither it nor a checkpoint exists offline).  Everything is fp32 in, fp32 accumulate; every convolution is 3 x 3,
 * stride 1, zero padding 1 at the true image border, with bias.  A model is an sr_resnet_desc:
 *     F = n_feat in {64, 128, 192, 256};  B = n_blocks, 0 <= B <= 64;  s = scale in {1, 2, 3, 4};
 *     flags long_skip, conv_hr, bilinear_base (0 / 1);  slopes a_head, a_up, a_hr (1.0: no activation), where
 *     act(y, a) = y >= 0 ? y : a * y;  res_scale;  mean[3], range.
 *  1. input      x[c] = (u8 / 255 - mean[c]) * range (fp32: one division, one subtraction, one product); zero is padded
 *                after this step.
 *  2. head       h = act(conv 3 -> F (x), a_head).
 *  3. blocks     t_0 = h;  for i = 1 .. B:  t = relu(conv1_i(t_{i-1})),  t_i = fmaf(res_scale, conv2_i(t), t_{i-1}).
 *  4. long skip  if long_skip:  t = conv_after_body(t_B) + h  (one fp32 add).
 *  5. upsampling s = 4: two stages with r = 2;  s in {2, 3}: one stage with r = s;  s = 1: none.  A stage is conv F -> F r^2,
 *                PixelShuffle(r):  u[c, Y, X] = v[c r^2 + (Y % r) r + (X % r), Y / r, X / r],  then act(u, a_up).
 *  6. HR conv    if conv_hr:  t = act(conv F -> F (t), a_hr) at full resolution.
 *  7. last conv  y = conv F -> 3 (t) at full resolution.
 *  8. output     o[c] = y[c] / range + mean[c]  (one division, one add);  with bilinear_base  o[c] = o[c] + base[c, Y, X], the
 *                bilinear upsample of p = u8 / 255 in torch's align_corners=False arithmetic, in fp32 and in this order:
 *                    sy = max((float)(1.0 / s) * (Y + 0.5f) - 0.5f, 0),  y0 = (int)sy,  y1 = y0 + (y0 < h - 1),
 *                    ly1 = sy - y0,  ly0 = 1 - ly1  (x alike),
 *                    base = ly0 * (lx0 * p[y0, x0] + lx1 * p[y0, x1]) + ly1 * (lx0 * p[y1, x0] + lx1 * p[y1, x1]).
 *                Stored as HWC fp32 unclamped (sr_resnet_f32) or as HWC u8 rintf(fminf(fmaxf(o, 0), 1) * 255) (sr_resnet_u8).
 * Presets: MSRResNet = a_head a_up a_hr 0.1, conv_hr, bilinear_base, no long_skip, res_scale 1, mean 0, range 1;
 *          EDSR = slopes 1, long_skip, no conv_hr, no bilinear_base, the caller's res_scale, mean and range.
 * Anything outside the ranges above (non-finite values and range 0 included) is SR_ERR_UNSUPPORTED, decided on the host before
 * any device call.
 * Summation order: body, upsampling, HR and last convolutions: bias, then channel pairs (2p, 2p + 1) ascending, then taps
 * ascending, one two-term MFMA step each (even channel, then odd); head: bias, then channels, then taps, as fmaf; a skip add
 * is one fmaf (or add) after the chain.  The order does not depend on where an output lies in a block or a sub-tile.
 * sr_resnet_create: h_w[k] / h_b[k] = weights (dense OIHW fp32) and bias of convolution k in forward order: head, (conv1,
 * conv2) per block, conv_after_body if long_skip, the upsampling stages, conv_hr if conv_hr, the last convolution; n_conv must
 * be that count.  The arrays are re-laid and uploaded.
 * sr_resnet_plan (host only, no context, no GPU): the image is streamed in tile x tile sub-tiles of the INPUT.  Every layer's
 * extent is derived backwards from the sub-tile's output rectangle: grown by one per convolution, divided by r (rounded
 * outwards) across a shuffle, clipped to the layer's image.  *halo = input pixels a sub-tile reads beyond its edge;
 * *n_tiles sub-tiles; *workspace_bytes = the model's three planar F-channel fp32 buffers, each sized for the largest layer of
 * one sub-tile (rows padded to 4 floats).  tile 0: the largest multiple of 32 up to 2048 (at least 32) with
 * 3 F (s (tile + 2 halo))^2 floats <= 1 GiB.  Outputs may be NULL.
 * sr_resnet_u8 / sr_resnet_f32: d_src h x w x 3 u8, d_dst (h s) x (w s) x 3; strides in bytes (fp32: a multiple of 4).
 * SR_ERR_INVALID_ARG for null pointers, a wrong n_conv and a tile < 0, SR_ERR_SHAPE for h or w < 1, a stride shorter than a
 * row, an output size beyond int or a sub-tile too large for 32-bit offsets -- all before any launch.  Every tile size gives
 * the same bits.  Asynchronous. */
typedef struct sr_resnet_desc {
    int n_feat, n_blocks, scale;
    int long_skip, conv_hr, bilinear_base;
    float a_head, a_up, a_hr, res_scale;
    float mean[3], range;
} sr_resnet_desc;
typedef struct sr_resnet_model sr_resnet_model;
SR_API int sr_resnet_create(sr_ctx *ctx, const sr_resnet_desc *desc, const float *const *h_w, const float *const *h_b, int n_conv,
                            sr_resnet_model **out);
SR_API int sr_resnet_destroy(sr_resnet_model *model);
SR_API int sr_resnet_plan(const sr_resnet_desc *desc, int h, int w, int tile, int *halo, int *n_tiles, size_t *workspace_bytes);
SR_API int sr_resnet_u8(sr_resnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                        int64_t dst_stride, int tile);
SR_API int sr_resnet_f32(sr_resnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                         int64_t dst_stride, int tile);

/* ---- local SR backend: RRDBNet, ESRGAN / Real-ESRGAN x4 (csrc/sr_rrdb.hip) -------------------------------------------------
 * BasicSR's RRDBNet at scale 4 (ESRGAN, RealESRGAN_x4plus with 23 blocks, RealESRGAN_x4plus_anime_6B with 6), restated (parity
 * with the BasicSR / Real-ESRGAN packages is unpinned: neither they nor a checkpoint exist offline).  Everything is fp32 in,
 * fp32 accumulate; every convolution is 3 x 3, stride 1, zero padding 1 at the true image border, with bias.  A model is an
 * sr_rrdb_desc:
 *     F = n_feat in {64, 128, 192, 256};  G = n_grow in {32, 64};  B = n_blocks, 0 <= B <= 32;  scale = 4;
 *     slope a (BasicSR: 0.2), act(y, a) = y >= 0 ? y : a * y;  res_scale beta (BasicSR: 0.2).
 *  1. input      x[c] = u8 / 255 (one fp32 division); zero is padded after this step.
 *  2. head       h = conv_first(x), 3 -> F, no activation.
 *  3. RRDB i = 1 .. B takes r = t_{i-1} (t_0 = h) through three dense blocks, then t_i = fmaf(beta, u, r) with u the third
 *                dense block's output.  A dense block on input x:  x_k = act(conv_k(cat(x, x_1, .., x_{k-1})), a) for
 *                k = 1 .. 4, each F + (k - 1) G -> G;  y = conv_5(cat(x, x_1 .. x_4)), F + 4 G -> F, no activation;  output
 *                fmaf(beta, y, x).  The concatenation's channel order is the weights' cin order: channels [0, F) are x,
 *                channels [F + (j - 1) G, F + j G) are x_j.  The third dense block is two fmafs in this order: first
 *                fmaf(beta, y, x), then fmaf(beta, that, r).
 *  4. trunk end  f = conv_body(t_B) + h  (one fp32 add).
 *  5. upsampling twice:  n[c, Y, X] = f[c, Y >> 1, X >> 1] (nearest), f' = act(conv_up1(n), a) at 2 x; the same again with
 *                conv_up2 at 4 x.
 *  6. HR convs   act(conv_hr(.), a), then conv_last F -> 3, both at 4 x.
 *  7. output     o = conv_last's value, no affine and no base.  Stored as HWC fp32 unclamped (sr_rrdb_f32) or as HWC u8
 *                rintf(fminf(fmaxf(o, 0), 1) * 255) (sr_rrdb_u8).
 * Anything outside the ranges above (non-finite slope / res_scale and scale != 4 included) is SR_ERR_UNSUPPORTED, decided on the
 * host before any device call.  Out of scope: the x2 / x1 variants that put a pixel-unshuffle in front of conv_first (its weight
 * then takes 12 or 48 channels), and fp16 / bf16.
 * Summation order: every F-input convolution: bias, then channel pairs (2p, 2p + 1) of the CONCATENATION ascending, then taps
 * ascending, one two-term MFMA step each (even channel, then odd); head: bias, then channels, then taps, as fmaf.  Nothing
 * depends on the position in a block, a trunk piece or a tail piece.
 * sr_rrdb_create: h_w[k] / h_b[k] = weights (dense OIHW fp32) and bias of convolution k in forward order: head, per RRDB
 * rdb1.conv1 .. conv5, rdb2 .., rdb3 .., then conv_body, conv_up1, conv_up2, conv_hr, conv_last; n_conv must be 1 + 15 B + 5.
 * sr_rrdb_plan (host only, no context, no GPU): two-phase streaming.  Every layer's extent is derived backwards from a piece's
 * output rectangle: divided by r (rounded outwards) across a 2 x 2 replication (r = 2 behind conv_body and conv_up1), grown by
 * one per convolution, clipped to the layer's image; *halo = 15 B + 4 input pixels a piece reads beyond its edge.
 *   trunk phase  tile x tile pieces of the INPUT (*n_tiles): head, RRDBs and conv_body, leaving f replicated to 2 x;
 *   tail phase   each trunk piece in tail x tail sub-pieces of the input (*n_tail_tiles in all): conv_up1 .. conv_last.
 * *workspace_bytes = 4 ((3 (F + 4 G) + F) P0 + F P2 + 2 F P4): three dense buffers of F + 4 G planes and h (F planes) of P0
 * floats, P0 = the largest head extent of a trunk piece (rows x columns padded to 4); f, F planes of P2 = the largest conv_body
 * extent at 2 x; two F-plane tail buffers of P4 = the largest 4 x extent of a tail sub-piece.  tail 0: 256.  tile 0: the
 * largest multiple of 32 up to 2048 (at least 32) whose trunk part 4 ((3 (F + 4 G) + F) P0 + F P2), laid out for this image, is
 * <= SR_RRDB_TRUNK_CAP = 16 GiB -- a policy, chosen so that F 64, G 32 on a 2048 x 2048 input (3.5 KiB per input pixel) runs the
 * trunk in one piece.  Outputs may be NULL.
 * sr_rrdb_u8 / sr_rrdb_f32: d_src h x w x 3 u8, d_dst (4 h) x (4 w) x 3; strides in bytes (fp32: a multiple of 4).
 * SR_ERR_INVALID_ARG for null pointers, a wrong n_conv, a destroyed model and a tile or tail < 0, SR_ERR_SHAPE for h or w < 1, a
 * stride shorter than a row, an output size beyond int or a piece too large for 32-bit offsets -- all before any launch.  Every
 * (tile, tail) gives the same bits.  Asynchronous. */
#define SR_RRDB_TRUNK_CAP ((size_t)16 << 30)
typedef struct sr_rrdb_desc {
    int n_feat, n_grow, n_blocks, scale;
    float slope, res_scale;
} sr_rrdb_desc;
typedef struct sr_rrdb_model sr_rrdb_model;
SR_API int sr_rrdb_create(sr_ctx *ctx, const sr_rrdb_desc *desc, const float *const *h_w, const float *const *h_b, int n_conv,
                          sr_rrdb_model **out);
SR_API int sr_rrdb_destroy(sr_rrdb_model *model);
SR_API int sr_rrdb_plan(const sr_rrdb_desc *desc, int h, int w, int tile, int tail, int *halo, int *n_tiles, int *n_tail_tiles,
                        size_t *workspace_bytes);
SR_API int sr_rrdb_u8(sr_rrdb_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                      int64_t dst_stride, int tile, int tail);
SR_API int sr_rrdb_f32(sr_rrdb_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                       int64_t dst_stride, int tile, int tail);

/* ---- local SR backend: RCAN, residual channel attention (csrc/sr_rcan.hip) --------------------------------------------------
 * BasicSR's RCAN (Zhang et al., ECCV 2018) at scales 1 .. 4, restated (parity with the BasicSR package is unpinned: neither it
 * nor a checkpoint exists offline).  Convolutions are fp32 in, fp32 accumulate, 3 x 3, stride 1, zero padding 1 at the true image
 * border, with bias; the channel attention is float64.  A model is an sr_rcan_desc:
 *     F = n_feat in {64, 128, 192, 256};  R = n_squeeze, 1 <= R <= F (BasicSR: F / 16);  G = n_groups, 1 <= G <= 16;
 *     B = n_blocks per group, 0 <= B <= 32;  s = scale in {1, 2, 3, 4};  res_scale;  mean[3], range.
 *  1. input      x[c] = (u8 / 255 - mean[c]) * range (fp32: one division, one subtraction, one product); zero is padded
 *                after this step.
 *  2. head       h = conv_first(x), 3 -> F, no activation.
 *  3. groups     t_0 = h;  group g = 1 .. G takes u = t_{g-1} through its B blocks (RCABs), then t_g = conv_g(u_B) + u_0 (one
 *                fp32 add, u_0 the group's input).  An RCAB on input u:
 *                    y1 = relu(conv_a(u)), relu(y) = y > 0 ? y : +0;   y2 = conv_b(y1);
 *                    m[c]  = (float)(S[c] / (double)(h w)),  S[c] = the float64 sum of y2[c] over exactly the h w pixels of the
 *                            image, in the order below;
 *                    z1[j] = max(b1[j] + sum_c w1[j][c] m[c], 0),  j < R;     z[c] = b2[c] + sum_j w2[c][j] z1[j]
 *                            (float64 from the fp32 tables and the fp32 m, index ascending, every term one rounded float64
 *                            product and one rounded float64 add; the first layer's products are exact);
 *                    s[c]  = (float)(1 / (1 + exp(-z[c])))  (float64 exp; a restatement's libm may differ from the device's in
 *                            the last place of s);
 *                    out   = fmaf(res_scale, (float)(y2 * s[c]), u)  (the product rounded to fp32, then one fmaf).
 *                The order of S[c]: the rows are cut into chunks of 32.  Inside a chunk, 256 lane sums: lane t adds rows ascending
 *                and, within a row, columns t, t + 256, .. ascending; the lane sums are folded a[t] += a[t + k] for
 *                k = 128, 64, .. 1; the chunks' sums are added in ascending order.  All float64, no atomics: the order depends on
 *                (h, w) alone.
 *  4. long skip  f = conv_after_body(t_G) + h  (one fp32 add).
 *  5. upsampling s = 4: two stages with r = 2;  s in {2, 3}: one stage with r = s;  s = 1: none.  A stage is conv F -> F r^2,
 *                PixelShuffle(r):  u[c, Y, X] = v[c r^2 + (Y % r) r + (X % r), Y / r, X / r]  (no activation).
 *  6. last conv  y = conv_last(.), F -> 3 at full resolution.
 *  7. output     o[c] = y[c] / range + mean[c]  (one division, one add).  Stored as HWC fp32 unclamped (sr_rcan_f32) or as HWC u8
 *                rintf(fminf(fmaxf(o, 0), 1) * 255) (sr_rcan_u8).
 * BasicSR's defaults, which a state dict does not hold: res_scale 1, range 255, mean (0.4488, 0.4371, 0.4040).
 * Anything outside the ranges above (non-finite values, range 0, and x8 with its three shuffle stages included) is
 * SR_ERR_UNSUPPORTED, decided on the host before any device call.  Out of scope: fp16 / bf16, x8, the original repository's key
 * names.
 * Summation order of the 3 x 3 convolutions: bias, then channel pairs (2p, 2p + 1) ascending, then taps ascending, one two-term
 * MFMA step each (even channel, then odd); head: bias, then channels, then taps, as fmaf.  Equal inputs give equal bits.
 * The mean makes an output depend on the whole image: the trunk (steps 2 .. 4) runs on the image in ONE piece, in five planar
 * fp32 buffers of F planes of P0 = h x (w padded to 4) floats (h / f, the group input, t, y1, y2); it is not streamed and there
 * is no tile argument.  After f nothing is global: steps 5 .. 7 run in tail x tail sub-pieces of the input, every layer's extent
 * derived backwards from the sub-piece's output rectangle (divided by r rounded outwards across a shuffle, grown by one per
 * convolution, clipped to the layer's image), in two F-plane buffers of P4 = the largest shuffled extent of a sub-piece.
 * sr_rcan_create: h_w[k] / h_b[k] = the tables in forward order: conv_first; per group, per RCAB conv_a, conv_b (dense OIHW
 * fp32), the first 1 x 1 layer (w1 dense [R][F], b1 [R]), the second (w2 dense [F][R], b2 [F]), then the group's convolution;
 * conv_after_body; the upsampling stages; conv_last.  n_tables must be 1 + G (4 B + 1) + 1 + stages + 1.
 * sr_rcan_plan (host only, no context, no GPU): *halo = input pixels a tail sub-piece reads beyond its edge (1 at s = 1, 2 at
 * every other scale); *n_tail_tiles = ceil(h / tail) ceil(w / tail); *workspace_bytes = 4 (5 F P0 + 2 F P4) + 8 F
 * ceil(h / 32) + 4 F (the buffers, the chunk sums, s).  tail 0: 256.  Outputs may be NULL.
 * sr_rcan_u8 / sr_rcan_f32: d_src h x w x 3 u8, d_dst (h s) x (w s) x 3; strides in bytes (fp32: a multiple of 4).
 * sr_rcan_attention_f32 (for inspection; synchronous): the mean and the attention of step 3 on any planar fp32 tensor on the
 * device, element (c, y, x) at d_x + c plane_stride + y row_stride + 4 x bytes, 1 <= R <= F <= 256; the four tables and the two
 * results h_mean[F], h_s[F] are host arrays.
 * SR_ERR_INVALID_ARG for null pointers, a wrong n_tables, a destroyed model and a tail < 0, SR_ERR_SHAPE for h or w < 1, a stride
 * shorter than a row, an output size beyond int, more than 262140 rows, P0 or P4 above INT_MAX / 8 floats (the convolution's
 * 32-bit offsets), and trunk buffers 20 F P0 bytes above SR_RCAN_TRUNK_CAP = 16 GiB -- a policy, as SR_RRDB_TRUNK_CAP; the
 * message names the largest input that fits (F = 64: 1280 bytes per pixel, about 13.4 MP) -- all before any launch.  Every tail
 * gives the same bits.  Asynchronous, except sr_rcan_attention_f32. */
#define SR_RCAN_TRUNK_CAP ((size_t)16 << 30)
typedef struct sr_rcan_desc {
    int n_feat, n_squeeze, n_groups, n_blocks, scale;
    float res_scale;
    float mean[3], range;
} sr_rcan_desc;
typedef struct sr_rcan_model sr_rcan_model;
SR_API int sr_rcan_create(sr_ctx *ctx, const sr_rcan_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables,
                          sr_rcan_model **out);
SR_API int sr_rcan_destroy(sr_rcan_model *model);
SR_API int sr_rcan_plan(const sr_rcan_desc *desc, int h, int w, int tail, int *halo, int *n_tail_tiles, size_t *workspace_bytes);
SR_API int sr_rcan_u8(sr_rcan_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                      int64_t dst_stride, int tail);
SR_API int sr_rcan_f32(sr_rcan_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                       int64_t dst_stride, int tail);
SR_API int sr_rcan_attention_f32(sr_ctx *ctx, const float *d_x, int64_t plane_stride, int64_t row_stride, int n_feat, int n_squeeze,
                                 int h, int w, const float *h_w1, const float *h_b1, const float *h_w2, const float *h_b2,
                                 float *h_mean, float *h_s);

/* ---- local SR backend: SwinIR, shifted-window attention (csrc/sr_swinir.hip, csrc/sr_swinir_host.cpp) -----------------------
 * BasicSR's SwinIR (Liang et al., ICCVW 2021) with resi_connection '1conv', ape False, patch_norm True, qkv_bias True,
 * patch_size 1, in_chans 3, window 8, restated (parity with BasicSR and the official repository is unpinned: neither package nor
 * a checkpoint exists offline).  Everything is fp32 (fp32 in, fp32 accumulate) except the LayerNorm statistics (float64).  A
 * model is an sr_swinir_desc:
 *     C = n_feat (embed_dim), 4 <= C <= 256, a multiple of 4;  n_heads dividing C with d = C / n_heads <= 32;
 *     n_hidden = the MLP's hidden width (rows of fc1), 1 <= n_hidden <= 4 C;  L = n_groups RSTBs, 1 <= L <= 12;
 *     D = depth, Swin layers per RSTB (the same in every RSTB), 1 <= D <= 12;  s = scale;  upsampler = SR_SWINIR_PIXELSHUFFLE
 *     (s in 2, 3, 4), SR_SWINIR_PIXELSHUFFLEDIRECT (s in 1 .. 4) or SR_SWINIR_NEAREST_CONV (s = 4);  mean[3], range.
 *  1. input      the u8 h x w x 3 image is extended to Hp x Wp, the next multiples of 8, by symmetric reflection: padded index
 *                i reads m = i mod 2 n, m < n ? m : 2 n - 1 - m (np.pad mode 'symmetric': the edge pixel repeated, period 2 n;
 *                the official test script's flip-concatenate whenever the pad is not larger than the side).  Then
 *                x[c] = (u8 / 255 - mean[c]) * range (fp32: one division, one subtraction, one product).
 *  2. head       h = conv_first(x), 3 x 3, 3 -> C, zero padding 1 at the border of the PADDED image (as every 3 x 3 here).
 *  3. deep       r_0 = LN(h) (patch_embed.norm);  RSTB i = 1 .. L:  x = r_{i-1}, D Swin layers, r_i = conv_i(x) + r_{i-1};
 *                then g = LN(r_L) (norm).  Swin layer j = 0 .. D - 1, shift = 0 for even j, 4 for odd j:
 *                    y   = LN1(x);   [q k v] = W y + b  (qkv: rows 0 .. C - 1 are q, then k, then v; head n owns the channels
 *                          n d .. n d + d - 1 of each);   q = q * (float)(1 / sqrtf(d))  (one fp32 multiply after the sum);
 *                    the tokens are the pixels of the image rolled by (-shift, -shift) and cut into 8 x 8 windows: token
 *                          (wy, wx) of window (by, bx) is pixel ((8 by + wy + shift) mod Hp, (8 bx + wx + shift) mod Wp);
 *                    a[i][j] = (sum_dd q_i[dd] k_j[dd]  +  B[rel(i, j)][head])  +  (region(i) != region(j) ? -100 : nothing)
 *                          for the 64 tokens of a window, rel(i, j) = (iy - jy + 7) * 15 + (ix - jx + 7) -- computed, the
 *                          state dict's relative_position_index and attn_mask buffers are ignored -- and, with shift 4 only,
 *                          region = 3 ry + rx of the token's coordinates (v) in the rolled image: 0 for v < L - 8, 1 for
 *                          v < L - 4, else 2 (calculate_mask's slices; L = Hp or Wp);
 *                    p[i][j] = e_j / sum_j e_j,  e_j = expf(a[i][j] - max_j a[i][j]);   o_i[dd] = sum_j p[i][j] v_j[dd];
 *                    x = x + (proj o + b)  at the token's own pixel (the roll back);
 *                    x = x + fc2(gelu(fc1(LN2(x)))),   gelu(t) = 0.5 t (1 + erff(t * 0.70710678f))  (fp32, left to right).
 *                LayerNorm (eps 1e-5, population variance), float64 from the fp32 values, channels ascending, two passes:
 *                    mean = (sum_c x[c]) / C;   var = (sum_c (x[c] - mean)^2) / C  (the square rounded, then added);
 *                    y[c] = (float)((x[c] - mean) * (1 / sqrt(var + 1e-5)) * gamma[c] + beta[c])
 *                every operation one rounded float64 operation, left to right, one rounding to fp32 at the end.
 *  4. long skip  f = conv_after_body(g) + h  (one fp32 add).
 *  5. reconstruction
 *       pixelshuffle        conv_before_upsample C -> 64, LeakyReLU 0.01;  upsample: s = 4 two stages with r = 2, else one with
 *                           r = s, a stage = conv 64 -> 64 r^2 + PixelShuffle(r);  conv_last 64 -> 3.
 *       pixelshuffledirect  upsample.0: conv C -> 3 s^2 + PixelShuffle(s); nothing else.
 *       nearest+conv (x4)   conv_before_upsample (LeakyReLU 0.01);  conv_up1 on the nearest x2 (LeakyReLU 0.2);  conv_up2 on
 *                           the nearest x2 of that (0.2);  conv_hr (0.2);  conv_last.
 *       PixelShuffle(r): u[c, Y, X] = v[c r^2 + (Y % r) r + (X % r), Y / r, X / r];  LeakyReLU: y >= 0 ? y : slope * y.
 *  6. output     o[c] = y[c] / range + mean[c] (one division, one add), cropped to (h s) x (w s).  Stored as HWC fp32 unclamped
 *                (sr_swinir_f32) or as HWC u8 rintf(fminf(fmaxf(o, 0), 1) * 255) (sr_swinir_u8).
 * SwinIR's defaults, which a state dict does not hold: range 1, mean (0.4488, 0.4371, 0.4040).
 * Summation orders.  3 x 3 convolutions and linear layers: bias, then channel pairs (2p, 2p + 1) ascending, then taps ascending,
 * one two-term MFMA step each (even channel, then odd); head: bias, then channels, then taps, as fmaf; a skip is one add after
 * the sum.  Attention: the dot product is an fmaf chain from +0 over dd ascending; then + B, then + the mask (two adds); the sum
 * of e_j runs over the keys j ascending from +0; the division by the sum comes BEFORE the a v sum (p is formed, as torch's
 * softmax does); the a v sum is an fmaf chain from +0 over j ascending.  No atomics.  Equal inputs give equal bits.
 * Anything outside the ranges above (a non-finite mean or range, range 0) is SR_ERR_UNSUPPORTED, decided on the host before any
 * device call.  Out of scope: window sizes other than 8, resi_connection '3conv', the absolute position embedding, the JPEG /
 * denoising variants (no upsampler), fp16 / bf16; Swin2SR is a backend of its own (below).
 * Shifted windows let a pixel see farther with every layer pair, so the trunk (steps 1 .. 4) runs on the padded image in ONE
 * piece: four planar fp32 buffers of Cp = C rounded up to 64 planes of P0 = Hp Wp floats (h / f, the RSTB input, x, LN / attention
 * output) and one of Qp = max(3 C, n_hidden each rounded up to 64) planes (qkv, then the MLP's hidden tensor): 4 (4 Cp + Qp)
 * bytes per pixel, 5376 at C = 180, hidden 360.  There is no tile argument.  After f nothing is global: step 5 runs in tail x tail
 * sub-pieces of the h x w input, every layer's extent derived backwards from the sub-piece's output rectangle (divided by r
 * rounded outwards across a shuffle or a replication, grown by one per convolution, clipped to the padded image), in two 64-plane
 * buffers of P4 = the largest stored extent of a sub-piece (none for pixelshuffledirect).  Every tail gives the same bits.
 * sr_swinir_create: h_w[k] / h_b[k] = the tables in forward order (dense fp32, weight then bias):
 *     conv_first [C][3][3][3];  patch_embed.norm (gamma[C], beta[C]);
 *     per RSTB i, per layer j:  norm1 (gamma, beta);  attn.qkv [3 C][C], [3 C];  attn.relative_position_bias_table [225][heads]
 *         (its h_b entry is ignored and may be NULL);  attn.proj [C][C], [C];  norm2;  mlp.fc1 [hidden][C];  mlp.fc2 [C][hidden];
 *     then the RSTB's conv [C][C][3][3];
 *     norm;  conv_after_body;  then pixelshuffle: conv_before_upsample.0 [64][C][3][3], upsample.0 (and .2) [64 r^2][64][3][3],
 *     conv_last [3][64][3][3];  pixelshuffledirect: upsample.0 [3 s^2][C][3][3];  nearest+conv: conv_before_upsample.0, conv_up1,
 *     conv_up2, conv_hr, conv_last.  n_tables must be 2 + L (7 D + 1) + 2 + (3 or 4 | 1 | 5).
 * sr_swinir_plan (host only, no context, no GPU): *hp, *wp = the padded size;  *halo = input pixels a tail sub-piece reads beyond
 * its edge;  *n_tail_tiles = ceil(h / tail) ceil(w / tail);  *workspace_bytes = 4 (4 Cp + Qp) P0 + 4 * 2 * 64 P4 + 3 P0 (the
 * trunk, the tail buffers, the reflected u8 image).  tail 0: 256.  Outputs may be NULL.
 * sr_swinir_rel_index (host only): rel[i * 64 + j] = rel(i, j); n must be 4096.
 * sr_swinir_u8 / sr_swinir_f32: d_src h x w x 3 u8, d_dst (h s) x (w s) x 3; strides in bytes (fp32: a multiple of 4).
 * sr_swinir_layernorm_f32 (for inspection; synchronous): the LayerNorm above on any planar fp32 tensor on the device, element
 * (c, y, x) at d_x + c plane_stride + y row_stride + 4 x bytes, into d_out likewise; gamma / beta are host arrays; C <= 256.
 * sr_swinir_attention_f32 (for inspection; synchronous): the window attention above (from a[i][j] to o, before proj) on a planar
 * qkv tensor of 3 C planes of hp x wp (multiples of 8) whose q planes are already scaled, h_table the [225][heads] host table,
 * shift 0 or 4, into the C planes of d_out.
 * sr_swinir_fill_workspace (for tests): grows the model's buffers to what an h x w forward needs and fills them with `byte`; a
 * forward must not depend on what its workspace held.
 * SR_ERR_INVALID_ARG for null pointers, a wrong n_tables, a destroyed model and a tail < 0, SR_ERR_SHAPE for h or w < 1, a stride
 * shorter than a row, an output size beyond int, more than 262140 rows, P0 above INT_MAX / 32 or P4 above INT_MAX / 8 floats
 * (the mainloop's 32-bit offsets inside a cin chunk), and trunk buffers above SR_SWINIR_TRUNK_CAP = 32 GiB -- a policy, as
 * SR_RCAN_TRUNK_CAP, so that one 2048 x 2048 pipeline block fits at C = 180; the message names the cap and the largest input
 * that fits -- all before any launch.  Asynchronous, except the two inspection entry points. */
#define SR_SWINIR_TRUNK_CAP ((size_t)32 << 30)
#define SR_SWINIR_PIXELSHUFFLE 0
#define SR_SWINIR_PIXELSHUFFLEDIRECT 1
#define SR_SWINIR_NEAREST_CONV 2
typedef struct sr_swinir_desc {
    int n_feat, n_heads, n_hidden, n_groups, depth, scale, upsampler;
    float mean[3], range;
} sr_swinir_desc;
typedef struct sr_swinir_model sr_swinir_model;
SR_API int sr_swinir_create(sr_ctx *ctx, const sr_swinir_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables,
                            sr_swinir_model **out);
SR_API int sr_swinir_destroy(sr_swinir_model *model);
SR_API int sr_swinir_plan(const sr_swinir_desc *desc, int h, int w, int tail, int *hp, int *wp, int *halo, int *n_tail_tiles,
                          size_t *workspace_bytes);
SR_API int sr_swinir_rel_index(int *rel, int n);
SR_API int sr_swinir_u8(sr_swinir_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                        int64_t dst_stride, int tail);
SR_API int sr_swinir_f32(sr_swinir_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                         int64_t dst_stride, int tail);
SR_API int sr_swinir_fill_workspace(sr_swinir_model *model, int h, int w, int tail, int byte);
SR_API int sr_swinir_layernorm_f32(sr_ctx *ctx, const float *d_x, int64_t plane_stride, int64_t row_stride, int n_feat, int h, int w,
                                   const float *h_gamma, const float *h_beta, float *d_out, int64_t out_plane_stride,
                                   int64_t out_row_stride);
SR_API int sr_swinir_attention_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads,
                                   int hp, int wp, int shift, const float *h_table, float *d_out, int64_t out_plane_stride,
                                   int64_t out_row_stride);

/* ---- local SR backend: HAT, hybrid attention (csrc/sr_hat.hip, csrc/sr_hat_host.cpp) -----------------------------------------
 * HAT (Chen et al., "Activating More Pixels in Image Super-Resolution Transformer", CVPR 2023) with resi_connection '1conv',
 * ape False, patch_norm True, qkv_bias True, patch_size 1, in_chans 3, window_size 16, overlap_ratio 0.5, upsampler
 * pixelshuffle, restated (parity with the official repository is unpinned: neither the package nor a checkpoint exists offline;
 * the forward is written from the published architecture).  Everything is fp32 except the LayerNorm statistics and the CAB's
 * channel attention (float64).  A model is an sr_hat_desc:
 *     C = n_feat (embed_dim), 4 <= C <= 256, a multiple of 4;  n_heads dividing C with d = C / n_heads <= 32;
 *     n_hidden = the MLP's hidden width, 1 <= n_hidden <= 4 C, the same in every HAB and OCAB;  n_mid = the CAB's compressed
 *     width (rows of cab.0), 1 <= n_mid <= C;  n_squeeze = rows of cab.3.attention.1, 1 <= n_squeeze <= C;  L = n_groups RHAGs,
 *     1 <= L <= 12;  D = depth, HABs per RHAG, 1 <= D <= 12;  s = scale in 2, 3, 4;  conv_scale;  mean[3], range.
 *  1. input      the u8 h x w x 3 image is extended to Hp x Wp, the next multiples of 16, by reflection WITHOUT the edge pixel
 *                (F.pad mode 'reflect', which HAT's pre_process uses; not SwinIR's symmetric form): padded index i reads
 *                m = i mod (2 n - 2), m < n ? m : 2 n - 2 - m; for n = 1 the single pixel is repeated.  Then
 *                x[c] = (u8 / 255 - mean[c]) * range, as SwinIR.
 *  2. head, 4. long skip, 5. reconstruction (pixelshuffle only), 6. output: exactly SwinIR's steps of those numbers.
 *  3. deep       r_0 = LN(h) (patch_embed.norm);  RHAG i = 1 .. L:  x = r_{i-1}, D HABs, one OCAB, r_i = conv_i(x) + r_{i-1};
 *                then g = LN(r_L) (norm).  LayerNorm, the linear layers and gelu are SwinIR's.
 *                HAB j = 0 .. D - 1, shift = 0 for even j, 8 for odd j:
 *                    y   = LN1(x);
 *                    window attention on y: SwinIR's with 16 in place of 8 -- 256 tokens per window, token (wy, wx) of window
 *                          (by, bx) is pixel ((16 by + wy + shift) mod Hp, (16 bx + wx + shift) mod Wp);  rel(i, j) =
 *                          (iy - jy + 15) * 31 + (ix - jx + 15), the table is [961][heads];  regions per axis: 0 for v < L - 16,
 *                          1 for v < L - 8, else 2;  the mask is -100;  q = q * (float)(1 / sqrtf(d));  a = proj(o) + b;
 *                    CAB on the same y (unshifted, not windowed; zero padding 1 at the border of the padded image):
 *                          t = gelu(conv3x3 C -> n_mid (y));  u = conv3x3 n_mid -> C (t);  m[c] = the mean of u[c] over the whole
 *                          Hp x Wp PADDED image, float64 in sr_rcan's fixed order (row chunks of 32, no atomics);
 *                          sc = sigmoid(W2 relu(W1 m + b1) + b2) in float64, as sr_rcan_attention_f32;
 *                    x = fmaf(conv_scale, u * sc, x + a):  x + a is one rounded add (proj's skip), u * sc one rounded fp32
 *                          product, and the scaled add ONE fmaf (as RCAN's res_scale) -- not a rounded product and an add;
 *                    x = x + fc2(gelu(fc1(LN2(x)))).
 *                OCAB (no shift, no mask):
 *                    y = LN1(x);  [q k v] = W y + b as above;  q scaled as above;  the queries of window (by, bx) are its 256
 *                    pixels;  the keys are the 576 positions (16 by - 4 + ky, 16 bx - 4 + kx), 0 <= ky, kx < 24;  a key position
 *                    outside the padded image has k = v = 0 EXACTLY (nn.Unfold zero-pads after the projection: the bias does not
 *                    enter) and is NOT masked: its score is 0 + bias, it takes its share of the softmax and adds nothing;
 *                    a[i][j] = q_i . k_j + B_oca[rpi_oca[i][j]][head], B_oca [1521][heads], rpi_oca [256][576];  softmax over the
 *                    576 keys;  x = x + (proj o + b);  x = x + fc2(gelu(fc1(LN2(x)))).
 *                rpi_oca: when the caller supplies an index (HAT's persistent buffer relative_position_index_OCA), THAT index is
 *                used: every value must lie in [-1521, 1520] and a negative one is wrapped once by + 1521 (torch's indexing).
 *                Without one, the default is the formula as recalled from calculate_rpi_oca -- unverified against the official
 *                code: (ky - qy - 7) * 39 + (kx - qx - 7), wrapped the same way.  The window attention's index is computed; a
 *                state's relative_position_index_SA must equal it; attn_mask buffers are ignored.  Where the keys sit: HAT
 *                registers both buffers once, on the top-level module, so a checkpoint holds the bare keys
 *                relative_position_index_SA and relative_position_index_OCA; sr_network.parse_hat_state reads every key that
 *                ends in one of the two names (top level or nested), never ignores one, and wants all OCA copies equal.
 * HAT's defaults, which a state dict does not hold: conv_scale 0.01, range 1, mean (0.4488, 0.4371, 0.4040).
 * Summation orders.  Convolutions, linear layers, head, skips: as SwinIR.  Both attention kernels make three sweeps over the
 * keys and recompute the score in each by the same instruction sequence (equal bits): the dot product is an fmaf chain from +0
 * over dd ascending; then + B, then (window attention, shift 8) + the mask (two adds); sweep 1 takes the exact maximum; sweep 2
 * sums e_j = expf(a_j - max) over the keys j ascending from +0; sweep 3 forms p_j = e_j / sum (the division comes BEFORE the p v
 * sum) and adds p_j v_j[dd] as an fmaf chain from +0 over j ascending.  No atomics.  Nothing depends on tail.  Equal inputs
 * give equal bits.
 * Anything outside the ranges above (a window other than 16, an overlap window other than 24, a non-finite constant, range 0) is
 * SR_ERR_UNSUPPORTED, decided on the host before any device call.  Out of scope: other windows and overlap ratios,
 * resi_connection 'identity', ape, upsamplers other than pixelshuffle, x1 and x8, fp16 / bf16, the ImageNet-pretraining heads.
 * The trunk (steps 1 .. 4) runs on the padded image in ONE piece: five planar fp32 buffers of Cp = C rounded up to 64 planes of
 * P0 = Hp Wp floats (h / f, the RHAG input, x, LN / attention output, the CAB's output), one of Tp = n_mid rounded up to 64 (the
 * CAB's middle tensor) and one of Qp = max(3 C, n_hidden each rounded up to 64) (qkv, then the MLP's hidden tensor):
 * 4 (5 Cp + Tp + Qp) bytes per pixel, 6400 at C = 180, n_mid 60, hidden 360.  The reconstruction runs in tail x tail sub-pieces as
 * SwinIR's.  Every tail gives the same bits.
 * sr_hat_create: h_w[k] / h_b[k] = the tables in forward order (dense fp32, weight then bias):
 *     conv_first [C][3][3][3];  patch_embed.norm (gamma[C], beta[C]);
 *     per RHAG i, per HAB j (residual_group.blocks.j):  norm1;  attn.qkv [3 C][C];  attn.relative_position_bias_table [961][heads]
 *         (its h_b entry is ignored and may be NULL);  attn.proj [C][C];  conv_block.cab.0 [n_mid][C][3][3];  conv_block.cab.2
 *         [C][n_mid][3][3];  conv_block.cab.3.attention.1 [n_squeeze][C];  conv_block.cab.3.attention.3 [C][n_squeeze];  norm2;
 *         mlp.fc1 [hidden][C];  mlp.fc2 [C][hidden];
 *     then the OCAB (residual_group.overlap_attn):  norm1;  qkv [3 C][C];  relative_position_bias_table [1521][heads] (no bias);
 *         proj;  norm2;  mlp.fc1;  mlp.fc2;  then the RHAG's conv [C][C][3][3];
 *     norm;  conv_after_body;  conv_before_upsample.0 [64][C][3][3];  upsample.0 (and .2) [64 r^2][64][3][3];  conv_last.
 *     n_tables must be 2 + L (11 D + 8) + 2 + (3 or 4).  h_rpi_oca: NULL for the default formula, else [256][576] ints.
 * sr_hat_plan (host only): as sr_swinir_plan;  *workspace_bytes = 4 (5 Cp + Tp + Qp) P0 + 4 * 2 * 64 P4 + 3 P0 + 8 C ceil(Hp / 32)
 * + 4 C (the trunk, the tail buffers, the reflected u8 image, the chunk sums and the attention vector).  tail 0: 256.
 * sr_hat_rel_index (host only): rel[i * 256 + j] = rel(i, j); n must be 65536.
 * sr_hat_oca_index (host only): idx[i * 576 + j] = the default rpi_oca, wrapped; n must be 147456.
 * sr_hat_attention_f32 / sr_hat_oca_f32 (for inspection; synchronous): the window attention (shift 0 or 8, h_table [961][heads])
 * and the overlapping cross-attention (h_table [1521][heads], h_index NULL or [256][576]) from a[i][j] to o, before proj, on a
 * planar qkv tensor of 3 C planes of hp x wp (multiples of 16) whose q planes are already scaled, into the C planes of d_out.
 * sr_hat_fill_workspace (for tests): as sr_swinir_fill_workspace.
 * Errors as SwinIR's, the row limit taken on the padded image (Hp above 262140 rows): SR_ERR_SHAPE for P0 above INT_MAX / 32, P4 above INT_MAX / 8 and a trunk above SR_HAT_TRUNK_CAP = 32 GiB
 * (the same policy as SR_SWINIR_TRUNK_CAP; the message names the cap and the largest input that fits), SR_ERR_INVALID_ARG for an
 * index value outside [-1521, 1520] -- all before any launch.  Asynchronous, except the two inspection entry points. */
#define SR_HAT_TRUNK_CAP ((size_t)32 << 30)
typedef struct sr_hat_desc {
    int n_feat, n_heads, n_hidden, n_mid, n_squeeze, n_groups, depth, scale;
    float conv_scale, mean[3], range;
} sr_hat_desc;
typedef struct sr_hat_model sr_hat_model;
SR_API int sr_hat_create(sr_ctx *ctx, const sr_hat_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables,
                         const int *h_rpi_oca, sr_hat_model **out);
SR_API int sr_hat_destroy(sr_hat_model *model);
SR_API int sr_hat_plan(const sr_hat_desc *desc, int h, int w, int tail, int *hp, int *wp, int *halo, int *n_tail_tiles,
                       size_t *workspace_bytes);
SR_API int sr_hat_rel_index(int *rel, int n);
SR_API int sr_hat_oca_index(int *idx, int n);
SR_API int sr_hat_u8(sr_hat_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride,
                     int tail);
SR_API int sr_hat_f32(sr_hat_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride,
                      int tail);
SR_API int sr_hat_fill_workspace(sr_hat_model *model, int h, int w, int tail, int byte);
SR_API int sr_hat_attention_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads,
                                int hp, int wp, int shift, const float *h_table, float *d_out, int64_t out_plane_stride,
                                int64_t out_row_stride);
SR_API int sr_hat_oca_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads, int hp,
                          int wp, const float *h_table, const int *h_index, float *d_out, int64_t out_plane_stride,
                          int64_t out_row_stride);

/* ---- local SR backend: Swin2SR, SwinV2 cosine attention and post-norm (csrc/sr_swin2sr.hip, csrc/sr_swin2sr_host.cpp) ---------
 * Swin2SR (Conde et al., "Swin2SR: SwinV2 Transformer for Compressed Image Super-Resolution and Restoration", ECCVW 2022) with
 * resi_connection '1conv', no absolute position embedding, patch size 1, window 8, shift 4 on odd layers, as the `transformers`
 * package's Swin2SRForImageSuperResolution computes it (modeling_swin2sr.py; the official repository's names in brackets).  The
 * package layout is held against `transformers` 5.15.0 (tests/golden/swin2sr_*.npz); the official layout and its mask value rest
 * on the restatement (tests/_swin2sr_ref.py); no published checkpoint was ever run.  Everything is fp32 except the LayerNorm
 * statistics (float64), as SwinIR.  A model is an sr_swin2sr_desc: SwinIR's fields with SwinIR's ranges (C <= 256 and a multiple
 * of 4, d = C / n_heads <= 32, n_hidden <= 4 C, L <= 12 stages, D <= 12 layers per stage, the three upsamplers
 * SR_SWINIR_PIXELSHUFFLE / _PIXELSHUFFLEDIRECT / _NEAREST_CONV at SwinIR's scales) and mask_value, finite.
 *  1. input      SwinIR's step 1 unchanged: the u8 image extended on the bottom and right to multiples of 8 by SYMMETRIC
 *                reflection (the package's image processor pads 'symmetric', the official test script by flip; the model's own
 *                'reflect' pad is then a no-op), x[c] = (u8 / 255 - mean[c]) * range.  Defaults: the DIV2K mean, range 1.
 *  2. head       h = conv3x3(x)  (first_convolution / conv_first).
 *  3. embedding  e = P_0 h + b, a 1 x 1 convolution C -> C (embeddings.patch_embeddings.projection / patch_embed.proj; SwinIR has
 *                none);  r_0 = LN(e)  (embeddings.patch_embeddings.layernorm / patch_embed.norm).
 *  4. stage i = 1 .. L (RSTB):  x = r_{i-1};  D layers;  r_i = P_i(conv3x3_i(x)) + r_{i-1}, P_i a 1 x 1 convolution with bias
 *                (stages.i.patch_embed.projection / layers.i.patch_embed.proj), the skip one fp32 add after the sum.
 *                Layer j = 0 .. D - 1, shift = 0 for even j, 4 for odd j:
 *                    [q k v] = W x + b on x ITSELF (there is no pre-norm); the k third has no bias (q_bias, 0, v_bias): a k bias
 *                          that is not zero is refused; q is NOT scaled by d^-1/2;
 *                    cosine window attention, per window and head (windows, roll, regions and rel(i, j) as SwinIR's):
 *                          ss = sum_dd q[dd]^2, an fmaf chain over dd ascending from +0;  n = sqrtf(ss);
 *                          qn[dd] = q[dd] / fmaxf(n, 1e-12f)  (a division);  k likewise;
 *                          a[i][j] = ((sum_dd qn_i[dd] kn_j[dd]) * scale_h  +  B[head][rel(i, j)])  +  (region(i) != region(j) ?
 *                          mask_value : nothing)  -- the sum an fmaf chain from +0, the scale one multiply, then two adds;
 *                          exact maximum, e_j = expf(a - max), the sum over keys ascending, p = e / sum, then the p v fmaf
 *                          chain: SwinIR's order;
 *                    x = x + LN1(proj(o) + b)   (layernorm_before / norm1, applied AFTER the attention);
 *                    x = x + LN2(fc2(gelu(fc1(x))))   (layernorm_after / norm2).
 *                LayerNorm as SwinIR's (eps 1e-5, float64);  LN(.) is rounded to fp32, then one fp32 add.
 *  5. long skip  f = conv_after_body(LN(r_L)) + h  (the skip is h, not e).
 *  6. reconstruction and output: SwinIR's steps 5 and 6 unchanged (pixelshuffle with 64 middle features and LeakyReLU 0.01).
 * Host-side tables (sr_swin2sr_cpb_bias; float64 from the fp32 weights, rounded once to fp32):
 *     scale_h = (float)exp(min((double)logit_scale_h, ln 100));
 *     B[t][head], t = (dy + 7) * 15 + dx + 7:  c = (g(8 dy / 7), g(8 dx / 7)), g(v) = sign(v) log2(|v| + 1) / 3;
 *     u = relu(W1 c + b1)  (Linear(2, 512));  z = W2 u  (Linear(512, heads), no bias; sums ascending);  B = 16 / (1 + exp(-z)).
 *     The package evaluates this in fp32; the distance is rounding-level.  The state's relative_coords_table,
 *     relative_position_index and attn_mask buffers are recomputed, never read.
 * mask_value.  The package adds the shifted-window mask twice, so its effective value is -200; the official code adds -100 once.
 * sr_network.parse_swin2sr_state sets -200 for the package's key layout and -100 for the official one (a 0-d `mask_value` entry
 * of a .npz overrides it).  With scale_h up to 100 a masked score can lie 200 + 16 above an unmasked one before the mask, so
 * the two values are not always equivalent.
 * The package's own model fails on a side that is not a multiple of 8 (its patch_unembed is given the unpadded size): at such
 * sizes the result is defined by step 1 alone.
 * Buffers: SwinIR's five (qkv X -> Q; attention -> A; proj A -> Q's first Cp planes; LN + skip -> X; fc1 X -> Q; fc2 Q -> A;
 * LN + skip -> X), the same bytes per pixel, SR_SWIN2SR_TRUNK_CAP = SR_SWINIR_TRUNK_CAP, the same tail phase.
 * sr_swin2sr_create: h_w[k] / h_b[k] = the tables in forward order (dense fp32):
 *     first_convolution [C][3][3][3];  P_0 [C][C], [C];  the embedding LayerNorm (gamma, beta);
 *     per stage, per layer:  qkv [3 C][C], [3 C] (rows q, k, v; bias entries C .. 2 C - 1 zero);  logit_scale [heads] (no bias);
 *         cpb_mlp.0 [512][2], [512];  cpb_mlp.2 [heads][512] (no bias);  proj [C][C], [C];  norm1;  fc1 [hidden][C];  fc2 [C][hidden];
 *         norm2;   then the stage's conv [C][C][3][3] and P_i [C][C], [C];
 *     norm;  conv_after_body;  the reconstruction's tables as sr_swinir_create's.  n_tables = 3 + L (9 D + 2) + 2 + (3 or 4 | 1 | 5).
 * sr_swin2sr_plan: as sr_swinir_plan.  sr_swin2sr_cpb_bias (host only): table [225][heads] and / or scale [heads] (either output
 * may be NULL, and with it the inputs only it needs).  sr_swin2sr_attention_f32 (inspection; synchronous): the attention above
 * on a planar qkv tensor (3 C planes of hp x wp), h_table [225][heads] = B, h_scale [heads], into the C planes of d_out.
 * sr_swin2sr_layernorm_add_f32 (inspection; synchronous): d_out = d_skip + (float)LN(d_x); d_out may be d_skip itself.
 * Errors as SwinIR's; SR_ERR_UNSUPPORTED also for a non-finite mask_value or logit_scale and for a k bias that is not zero.  Out
 * of scope, refused by name: upsampler pixelshuffle_aux, no upsampler (JPEG / denoising), '3conv', the absolute position
 * embedding, windows other than 8, unequal depths or head counts between stages, fp16 / bf16 weights. */
#define SR_SWIN2SR_TRUNK_CAP SR_SWINIR_TRUNK_CAP
typedef struct sr_swin2sr_desc {
    int n_feat, n_heads, n_hidden, n_groups, depth, scale, upsampler;
    float mean[3], range, mask_value;
} sr_swin2sr_desc;
typedef struct sr_swin2sr_model sr_swin2sr_model;
SR_API int sr_swin2sr_create(sr_ctx *ctx, const sr_swin2sr_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables,
                             sr_swin2sr_model **out);
SR_API int sr_swin2sr_destroy(sr_swin2sr_model *model);
SR_API int sr_swin2sr_plan(const sr_swin2sr_desc *desc, int h, int w, int tail, int *hp, int *wp, int *halo, int *n_tail_tiles,
                           size_t *workspace_bytes);
SR_API int sr_swin2sr_cpb_bias(const float *h_w1, const float *h_b1, const float *h_w2, const float *h_logit_scale, int n_heads,
                               float *h_table, float *h_scale);
SR_API int sr_swin2sr_u8(sr_swin2sr_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                         int64_t dst_stride, int tail);
SR_API int sr_swin2sr_f32(sr_swin2sr_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                          int64_t dst_stride, int tail);
SR_API int sr_swin2sr_fill_workspace(sr_swin2sr_model *model, int h, int w, int tail, int byte);
SR_API int sr_swin2sr_attention_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads,
                                    int hp, int wp, int shift, const float *h_table, const float *h_scale, float mask_value,
                                    float *d_out, int64_t out_plane_stride, int64_t out_row_stride);
SR_API int sr_swin2sr_layernorm_add_f32(sr_ctx *ctx, const float *d_x, int64_t plane_stride, int64_t row_stride, int n_feat, int h, int w,
                                        const float *h_gamma, const float *h_beta, const float *d_skip, int64_t skip_plane_stride,
                                        int64_t skip_row_stride, float *d_out, int64_t out_plane_stride, int64_t out_row_stride);

/* ---- geometric self-ensemble of the local SR backends (csrc/sr_ensemble.hip) ------------------------------------------------
 * The "+" results of the SR literature (EDSR+, RCAN+: Timofte et al., Lim et al.): the network runs on the eight flips and
 * rotations of the input, each output is mapped back and the eight are averaged.  No new weights; the forwards are the
 * families' own, unchanged.
 * The eight transforms: for k = 0 .. 7, on an H x W x C image, T_k(x) applies in this order
 *     1. if k & 1, a horizontal flip   x[:, ::-1]
 *     2. if k & 2, a vertical flip     x[::-1]
 *     3. if k & 4, a transpose of the two spatial axes (the result is W x H x C)
 * and T_k^-1 undoes the three steps in reverse order.  The T_k are the dihedral group D4; T_0 is the identity.
 * The members: mask has bits 0 .. 7, 1 <= mask <= 255, bit k = member k in use; n = the number of set bits.
 * The output: with f the family's existing forward (the value sr_<kind>_f32 stores) and y_k = T_k^-1(f(T_k(x))),
 *     s = y_k1;  s = s + y_k2;  ...  (members ascending, every + one IEEE fp32 addition per element)
 *     o = s / (float)n               (a correctly rounded fp32 division, never a reciprocal multiply)
 * *_f32 stores o as HWC fp32 unclamped, *_u8 stores rintf(fminf(fmaxf(o, 0), 1) * 255), the forwards' rule.  So mask 1 gives
 * the plain forward bit for bit, a one-bit mask gives y_k itself, and -- the forwards not depending on the sub-tile -- no
 * result depends on tile / tail.
 * sr_d4_u8: d_dst = T_k(d_src), d_src h x w x 3 u8, d_dst w x h x 3 for k & 4; the two must not overlap.
 * sr_d4_acc_f32: d_acc (H x W x 3 fp32) = T_k^-1(d_y) if first, else d_acc + T_k^-1(d_y); d_y is H x W, or W x H for k & 4.
 * sr_ens_finish_f32 / _u8: d_dst = d_acc / n by the two store rules; n in 1 .. 8.
 * sr_ens_plan (host only, no context, no GPU): *n_members = n; *workspace_bytes = what an ensemble call holds: the
 * accumulator (h scale rows of w scale x 12 bytes), one forward output (the same, and w scale rows of h scale x 12 bytes when
 * a member k >= 4 is in use: the larger) and the transformed u8 input (h rows of 3 w bytes for a member 1 .. 3, w rows of 3 h
 * for a member k >= 4: the larger; nothing for mask 1) -- every row stride rounded up to 16 bytes, every section to 256.
 * Outputs may be NULL.  Refuses an output size beyond int (for k >= 4: of the transposed image too), as the forwards do.
 * sr_<kind>_ens_u8 / _f32: the plain form's arguments, then mask.  The workspace belongs to the model, is grown on demand and
 * is freed with it, like the activation buffers.  Everything runs on the model's stream.  Asynchronous.
 * Refusals, all before any launch: SR_ERR_INVALID_ARG for a null pointer, k outside 0 .. 7, a mask outside 1 .. 255, n
 * outside 1 .. 8, a scale < 1, overlapping buffers, an fp32 pointer that is not a multiple of 4; SR_ERR_SHAPE for a side below
 * 1, a stride shorter than a row, an fp32 stride that is not a multiple of 4, a size beyond int.  Strides in bytes. */
SR_API int sr_d4_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int k, uint8_t *d_dst, int64_t dst_stride);
SR_API int sr_d4_acc_f32(sr_ctx *ctx, const float *d_y, int64_t y_stride, int H, int W, int k, int first, float *d_acc,
                         int64_t acc_stride);
SR_API int sr_ens_finish_f32(sr_ctx *ctx, const float *d_acc, int64_t acc_stride, int H, int W, int n, float *d_dst,
                             int64_t dst_stride);
SR_API int sr_ens_finish_u8(sr_ctx *ctx, const float *d_acc, int64_t acc_stride, int H, int W, int n, uint8_t *d_dst,
                            int64_t dst_stride);
SR_API int sr_ens_plan(int h, int w, int scale, int mask, int *n_members, size_t *workspace_bytes);
SR_API int sr_srnet_ens_u8(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                           int64_t dst_stride, int tile, int mask);
SR_API int sr_srnet_ens_f32(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                            int64_t dst_stride, int tile, int mask);
SR_API int sr_resnet_ens_u8(sr_resnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                            int64_t dst_stride, int tile, int mask);
SR_API int sr_resnet_ens_f32(sr_resnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                             int64_t dst_stride, int tile, int mask);
SR_API int sr_rrdb_ens_u8(sr_rrdb_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                          int64_t dst_stride, int tile, int tail, int mask);
SR_API int sr_rrdb_ens_f32(sr_rrdb_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                           int64_t dst_stride, int tile, int tail, int mask);
/* RCAN+: a flip or a transpose permutes the pixels of every plane, so each member pools over its own planes and nothing else
 * changes. */
SR_API int sr_rcan_ens_u8(sr_rcan_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                          int64_t dst_stride, int tail, int mask);
SR_API int sr_rcan_ens_f32(sr_rcan_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                           int64_t dst_stride, int tail, int mask);
/* SwinIR+: every member is reflected, padded and windowed on its own. */
SR_API int sr_swinir_ens_u8(sr_swinir_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                            int64_t dst_stride, int tail, int mask);
SR_API int sr_swinir_ens_f32(sr_swinir_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                             int64_t dst_stride, int tail, int mask);
/* HAT+: as SwinIR+; each member also pools the CAB's mean over its own padded planes. */
SR_API int sr_hat_ens_u8(sr_hat_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                         int64_t dst_stride, int tail, int mask);
SR_API int sr_hat_ens_f32(sr_hat_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                          int64_t dst_stride, int tail, int mask);
/* Swin2SR+: as SwinIR+. */
SR_API int sr_swin2sr_ens_u8(sr_swin2sr_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst,
                             int64_t dst_stride, int tail, int mask);
SR_API int sr_swin2sr_ens_f32(sr_swin2sr_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst,
                              int64_t dst_stride, int tail, int mask);

#ifdef __cplusplus
}
#endif
#endif /* SR_HIP_H */
