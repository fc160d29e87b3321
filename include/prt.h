/*
 * prt.h — C-ABI of libprt, the MI355X-native path-tracing core behind
 * pyrenderer's Scene / Camera / BSDF API and core.tracing.render().
 *
 * The reference exposes no FFI: its hot path is the Taichi kernel closure
 * `render()` (main_taichi.py:80-99) calling PathTracer.trace
 * (core/tracing.py:116-155) over World.hit_all (mathematics/intersection_taichi.py:238-291),
 * with the scene baked into Taichi fields by World.commit()
 * (mathematics/intersection_taichi.py:220-233) and the camera by
 * Camera.convert_to_taichi_camera() (core/camera.py:27-36).  Each entry point
 * below names the reference interface it replaces; the Python host layer
 * (pyrenderer_amd, ctypes) is the only caller.  INTEGRATION.md shows the
 * binding a pyrenderer maintainer would add.
 *
 * Conventions: all pointers are borrowed for the duration of the call (data is
 * copied to the device); outputs are caller-allocated, C-contiguous float32.
 * Every int-returning function returns PRT_OK (0) or a negative PRT_ERR_*; no
 * C++ exception crosses the ABI; prt_last_error() describes the last failure
 * on the calling thread.  A scene handle is bound to one device and is not
 * re-entrant; distinct handles may be driven from distinct host threads.
 */
#ifndef PRT_H_
#define PRT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.
 * ABI 2: prt_trace_rays, prt_hit_all added; trace-kernel variant ids renumbered to 1..8
 * (PRT_FLAG_VARIANT; 7 / 8 are the pooled-shadow kernel; ids above 8 are rejected with
 * PRT_ERR_ARG, and ABI 1's ids 1..8 named other kernels, so a caller built against ABI 1 must
 * check prt_abi_version()); prt_scene_info's info8[4] is the BVH4 LDS traversal stack depth (0:
 * BVH4 too deep for the LDS-stack variants); watchdog flags are cleared once reported
 * (prt_check_faults).
 * ABI 3 (round 5): prt_render_frames_device (round 4) takes an output pitch between frames
 * (out_pitch, floats; 0 = packed), so a rank whose shard is shorter than its gather slot can render
 * straight into a padded per-frame buffer; prt_scatter_frames and prt_camera_rays added; variant
 * ids 9..14 (three experimental schedules of the pooled kernel) added.
 * ABI 4 (this build, round 6): variant ids 9..14 removed again (none became the default; DESIGN.md
 * §9), ids above 8 are rejected with PRT_ERR_ARG as in ABI 2; prt_scatter_frames rejects a
 * group_pitch too short for n_frames frames at src_frame_pitch; prt_camera_rays zero-fills the rows
 * of slots outside the frame; prt_selftest_guards added.  Added later under the same number (purely
 * additive, no existing entry point changed): the denoiser's four entry points at the end of this
 * header, then the three of its variance-guided mode (prt_denoise_var*), then the four of the
 * sample-moments variance (prt_moments_add*, prt_denoise_var_given*), then the four of the temporal
 * accumulation (prt_temporal_accumulate*, prt_denoise_var_mixed*), then the two of adaptive sampling
 * (prt_adaptive_update*), then the two of temporal accumulation across moving objects
 * (prt_temporal_accumulate_motion*), then the refit of a resident scene (prt_scene_update) and the read-back
 * of a scene's device buffers (prt_scene_download), then the rebuild of a resident scene's trees on the device
 * (prt_scene_rebuild, prt_scene_rebuild_info). */
#define PRT_ABI_VERSION 4

#define PRT_OK 0
#define PRT_ERR_ARG (-1)     /* invalid argument / shape */
#define PRT_ERR_HIP (-2)     /* HIP runtime error (no device, launch failure, ...) */
#define PRT_ERR_OOM (-3)     /* host or device allocation failed */
#define PRT_ERR_RCCL (-4)    /* RCCL communicator / collective failure */
#define PRT_ERR_UNSUP (-5)   /* feature not supported by this build */
#define PRT_ERR_INTERNAL (-6) /* device-side check failed (traversal watchdog); results invalid */

/* render flags */
#define PRT_FLAG_STATS 0x1u  /* count BVH nodes / triangle tests / queries (slower kernel variant) */
#define PRT_FLAG_TIME 0x2u   /* time the trace kernel with HIP events on its stream */
/* ABI 3: rejected with PRT_ERR_UNSUP — camera rays (and, for cameras other than the affine pinhole,
 * their origins) always come from the camera kernel; the trace kernels carry no camera code, whose
 * uniform operands spilled SGPRs in their loops (C2 4.01 -> 3.91 ms per launch without it) */
#define PRT_FLAG_NO_PRIMARY_KERNEL 0x4u
/* estimator variant: direct lighting by the reference's unused MIS function
 * PathTracer.sample_direct_lighting2 (core/tracing.py:57-90, helpers :12-39) in place of
 * sample_direct_lighting — two closest-hit visibility queries per diffuse vertex (light
 * and BRDF strategies, power heuristic, light_area 1.0 as the reference passes it).
 * A different estimator: the image differs from the default one (oracle: or_set_nee_mode).
 * Selects the MIS kernel variants (4, 5); an explicit variant must agree with the flag. */
#define PRT_FLAG_MIS_NEE 0x8u
/* trace-kernel variant in bits 8..15 (0 = automatic; the numbering is the
 * kVar* table of pyrenderer_amd/csrc/prt_kernels.h: 1 LDS-resident scene (>= 7 waves per
 * SIMD), 2 the same without an occupancy target, 3 global scene (quantised nodes, spill
 * stack), 4 / 5 the MIS estimator on an LDS / global scene, 6 the LDS-resident scene built
 * for >= 6 waves per SIMD, 7 / 8 the LDS-resident block-pooled shadow kernel for >= 7 / >= 6
 * waves per SIMD).  Variants of one estimator produce bit-identical images; the selector exists
 * for A/B runs and tests. */
#define PRT_FLAG_VARIANT_SHIFT 8
#define PRT_FLAG_VARIANT(v) (((uint32_t)(v) & 0xFFu) << PRT_FLAG_VARIANT_SHIFT)

/* material row (8 floats): rho.r rho.g rho.b emit sided type ior roughness */
#define PRT_MAT_LAMBERT 0    /* core/bsdf.py:18-42 BSDFLambertian */
#define PRT_MAT_LIGHT 1      /* core/bsdf.py:45-65 BSDFLight (emit=1, sided=1) */
#define PRT_MAT_METAL 2      /* core/bsdf_taichi.py:45-59 */
#define PRT_MAT_DIELECTRIC 3 /* core/bsdf_taichi.py:62-86 */

/* camera record (24 floats) = CameraTaichi state (core/camera_taichi.py:10-39):
 *   [0:16]  iview_c1..iview_c4 (rows of iview.T)
 *   [16:20] sensor_dim = (sensor_width, sensor_height, focus_dist, aperture)
 *   [20:24] reserved, 0 */
#define PRT_CAM_FLOATS 24

int prt_abi_version(void);
const char* prt_last_error(void);
/* number of visible HIP devices (0 when no GPU; returns PRT_OK either way) */
int prt_device_count(int* n);

/* ---------------------------------------------------------------- BVH ----
 * Replaces accelerators/bvh_taichi.py:107-161 (BVH(prims).build(), median
 * split over primitives) with a binned-SAH BVH2 over triangles.  Host only.
 * tri_v: n_tri x 9 (v0 v1 v2).  info[6] = n_nodes, depth, n_leaves, n_tri,
 * bits of the f32 box padding, round(SAH cost * 1000). */
int prt_bvh_build(const float* tri_v, int64_t n_tri, int32_t max_leaf, void** out_bvh);
int prt_bvh_info(void* bvh, int64_t* info6);
/* nodes: n_nodes x 16 f32; tris: n_tri x 12 f32 (BVH order); order: n_tri (BVH slot -> triangle) */
int prt_bvh_export(void* bvh, float* nodes, float* tris, int32_t* order);
/* The wide tree a scene's kernels traverse, collapsed from this BVH2 (same triangle order and leaf
 * references): width 4 (every scene) or 8 (scenes the trace kernels keep in LDS).  info4 = n_nodes,
 * depth (root-to-leaf node count - 1), worst-case traversal stack entries, floats per node (32 / 56).
 * nodes (NULL: sizes only): n_nodes x floats per node; children in groups of four, group g at 24 g floats:
 * lo.x[4] hi.x[4] lo.y[4] hi.y[4] lo.z[4] hi.z[4], then the child refs (int bits) after the last group;
 * empty slots: lo = +inf, hi = -inf, ref = 0x7FFFFFFF. */
int prt_bvh_collapse(void* bvh, int32_t width, int64_t* info4, float* nodes);
void prt_bvh_destroy(void* bvh);

/* -------------------------------------------------------------- scene ----
 * Replaces World.add / World.commit (mathematics/intersection_taichi.py:220-233)
 * plus the Taichi fields of Quad/Cube (mathematics/shapes.py:49-57, 178-186).
 *   tri_v   n_tri x 9 f32   world-space vertices, face order (v0 v1 v2)
 *   tri_n   n_tri x 3 f32   face normal, reference convention (shapes.py:47,176)
 *   tri_mat n_tri i32       material row
 *   sph     n_sph x 4 f32   center.xyz, radius (intersection_taichi.py:15-36); n_sph may be 0
 *   mat     n_mat x 8 f32   material rows (PRT_MAT_*)
 *   light_tri / light_off   triangles of each emitting primitive, grouped per
 *                           light (light_off has n_light+1 prefix offsets):
 *                           World.sample_a_light + Quad.sample_a_point
 *                           (intersection_taichi.py:194-207, shapes.py:62-71)
 *   direct_rgb 3 f32        colour added when a path hits the light (tracing.py:120)
 * Builds the BVH on the host and uploads everything to `device`. */
int prt_scene_create(int device,
                     const float* tri_v, const float* tri_n, const int32_t* tri_mat, int64_t n_tri,
                     const float* sph, const int32_t* sph_mat, int64_t n_sph,
                     const float* mat, int32_t n_mat,
                     const int32_t* light_tri, const int32_t* light_off, int32_t n_light,
                     const float* direct_rgb, void** out_scene);
/* info[8] = device, n_tri, n_nodes, BVH2 depth, BVH4 LDS traversal stack entries (0: the BVH4 is
 * too deep for the LDS-stack variants, only the spill-stack global variant runs), device
 * bytes, blocks/CU of the default variant, CUs */
int prt_scene_info(void* scene, int64_t* info8);
void prt_scene_destroy(void* scene);
/* Added under ABI 4, purely additive: new geometry for a resident scene whose primitives moved (DESIGN.md
 * §13).  tri_v, tri_n and sph are the full arrays with the counts of creation (sph may be NULL when the scene
 * has no spheres); tri_mat, the materials, the light lists and direct_rgb stay those of creation.  The
 * topology of the trees, their leaf references and the triangle order stay too: the device rewrites the
 * BVH-order triangle records, refits the boxes of the four- and eight-wide trees bottom-up (a leaf's box is the
 * bound of its triangles' vertices, padded by the builder's rule taken on the new vertices) and re-quantises
 * the four-wide nodes; the shading data (normals, frames, light vertices, the shade_fast flag) is re-packed on
 * the host and uploaded into the existing buffers.  Every buffer, the handle, its streams and render contexts
 * survive.  Results do not depend on the tree, so every query and render equals that of a scene created from
 * the same arrays, bit for bit; a tree built without reference splits is also word for word the created one.
 * References split at creation get the whole triangle's box, so the tree loosens as objects move far from the
 * pose it was built at (DeviceScene.tree_cost tells).  The first update allocates the device copies it needs
 * (triangle order, level lists, slot bounds, vertices: prt_scene_info's device bytes grow by them).
 * Synchronises the device before it touches the scene and its own stream before it returns.  A NULL scene or
 * array, a vertex, normal or sphere that is not finite, or a radius <= 0 return PRT_ERR_ARG before the device
 * is touched: the scene then renders what it rendered before.  That promise covers argument errors only.  After
 * PRT_ERR_HIP or PRT_ERR_OOM (an allocation of the first update, an upload or a launch failed part-way) some
 * buffers may hold the new geometry and others the old, and the device bytes may count a copy that a later,
 * successful update allocates again: the scene is then good for prt_scene_destroy and for another
 * prt_scene_update that succeeds, which rewrites every buffer, and for nothing else. */
int prt_scene_update(void* scene, const float* tri_v, const float* tri_n, const float* sph);
/* Test and inspection hook, added with prt_scene_update: the scene's device buffer `which` copied to out
 * (host), `bytes` its exact size, else PRT_ERR_ARG.  Layouts: prt_bvh_collapse's nodes for the two trees
 * (NODES8: 0 bytes when the scene has no eight-wide tree), 16 f32 per quantised node, prt_bvh_export's tris,
 * 4 f32 per triangle (normal, material bits), 24 f32 per triangle (frames), 16 f32 per emitter triangle, 4 f32
 * per sphere.  PRT_BUF_UPDATE_MS: 5 f64, the last update's host checks and packing, uploads, triangle records,
 * tree levels and quantiser in ms.  which | PRT_BUF_BYTES: out receives the buffer's size as one int64
 * (bytes = 8).  PRT_BUF_UPDATE_MS and the size queries go beyond the device buffers: they answer from the
 * handle's host state, make no device call and synchronise nothing; every other download synchronises the
 * device first, so it sees the scene as the last render or update left it. */
#define PRT_BUF_NODES4 0
#define PRT_BUF_NODES4Q 1
#define PRT_BUF_NODES8 2
#define PRT_BUF_TRIS 3
#define PRT_BUF_TRI_NM 4
#define PRT_BUF_TRI_FRAME 5
#define PRT_BUF_LIGHT_V 6
#define PRT_BUF_SPH 7
#define PRT_BUF_UPDATE_MS 8
#define PRT_BUF_BYTES 0x100
int prt_scene_download(void* scene, int which, void* out, int64_t bytes);
/* Added under ABI 4, purely additive: the trees of a resident scene built again on the device, for a scene whose
 * refit tree has loosened.  Arguments, checks and the promise about a refused call are
 * prt_scene_update's; a scene of 2^28 triangles or more is refused too (PRT_ERR_ARG).  The tree is a linear BVH
 * (Karras 2012): per triangle the centroid (lo + hi) * 0.5f of its vertex bounds; per axis the 10-bit cell
 * min((int)((c - cmin) / (cmax - cmin) * 1024.0f), 1023) within the centroids' bounds, all in f32, 0 on an axis
 * of zero extent; the 30-bit Morton code with x the most significant bit of each triple; a stable sort by code
 * gives the new slot order, one slot per triangle (no reference is split); the keys code << 32 | slot are
 * distinct, and the binary radix tree over them splits a range at the highest bit in which its first and last
 * key differ.  A wide node over a range takes as children the ranges reached after log2(width) binary splits, a
 * range of at most PRT_MAX_LEAF triangles (as read when the scene was created, default 4) stopping as a leaf;
 * children stand in slot order, empty slots after them; the nodes are numbered breadth-first, level by level.
 * Boxes, padding and the quantised records are prt_scene_update's.  Written: the slot order, the triangle
 * records, the four-wide tree (f32 and quantised) and, for a scene whose new sizes fit LDS, the eight-wide one
 * with the width rule taken again (else the scene has none); the stack needs, the stack variants and the
 * default kernel follow the new trees (a four-wide tree needing more than 32 entries takes the spill variants,
 * as at creation), prt_scene_info's n_nodes and depth become the four-wide tree's node count and levels - 1.
 * A later prt_scene_update refits the new trees.  Buffers grow only when a tree needs more room than they have;
 * the first rebuild allocates the build's work arrays (about 64 bytes per triangle), a second rebuild of the
 * same scene nothing.  Handle, streams and render contexts survive; synchronises as prt_scene_update does. */
int prt_scene_rebuild(void* scene, const float* tri_v, const float* tri_n, const float* sph);
/* The last rebuild's report (PRT_ERR_ARG before the first): info8 = four-wide nodes, depth (levels - 1),
 * worst-case stack entries; eight-wide nodes (0: none), depth, stack entries; the LDS kernels' width; slots.
 * ms8 = host checks and packing, uploads, codes, sort, binary tree, wide emission (both widths, with one count
 * read back per level), triangle records and boxes, quantiser.  Either may be NULL. */
int prt_scene_rebuild_info(void* scene, int64_t* info8, double* ms8);

/* ------------------------------------------------------------- render ----
 * Replaces the render() kernel of main_taichi.py:80-99 run `spp` times
 * (pixels[x,y] += PathTracer.trace(...), samples[x,y] += 1).
 * Work = the pixels of `tile_ids` (tiles of tw x th in a W x H frame, tile id =
 * ty * ceil(W/tw) + tx) times samples 0..spp-1, path depth `depth`.
 * out_sum: n_tiles*tw*th x 3 f32, the per-pixel SUM of radiance over samples
 * taken in sample order (divide by spp for the mean: pixels/samples); slot
 * order = tile-major, then row (ly), then column (lx); pixels outside the
 * frame are 0.  Random numbers are keyed by (seed, y*W+x, sample), so the
 * result does not depend on the tiling or on how tiles are spread over GPUs.
 * stats (optional, 4 x u64, needs PRT_FLAG_STATS): BVH nodes visited,
 * triangle tests, extension queries, shadow queries. */
int prt_render_tiles(void* scene, const float* cam, int W, int H, int tw, int th,
                     const int32_t* tile_ids, int n_tiles, int spp, int depth, uint64_t seed,
                     uint32_t flags, float* out_sum, uint64_t* stats);
/* One rectangular window of the frame, as SURVEY.md §8(b)'s prt_render: samples
 * 0..spp-1 of the pixels [x0, x0+w) x [y0, y0+h) of a W x H frame (random streams
 * keyed by the global pixel, so any window equals the same crop of a full-frame render),
 * path depth `depth`.  out_sum: w x h x 3 f32, the per-pixel radiance SUM over samples
 * in sample order, indexed [x - x0][y - y0] like the reference's pixels.to_numpy()
 * (main_taichi.py:25, the render() kernel of main_taichi.py:80-99 run spp times).
 * Rendered as the 8 x 8 tiles covering the window.  stats as prt_render_tiles. */
int prt_render(void* scene, const float* cam, int W, int H, int x0, int y0, int w, int h, int spp, int depth,
               uint64_t seed, uint32_t flags, float* out_sum, uint64_t* stats);
/* The whole W x H frame over several GPUs of this process (SURVEY.md §8(b)
 * prt_render_multi, §8(e)): scenes[r] is a scene handle on its own device (all
 * distinct; scenes[0] is the root).  Tiles of tile x tile pixels go to rank
 * (tx + s*ty) mod n_scenes (the 'latin' interleave of device_scene.tile_owner), every
 * rank renders its tiles on its device, and ONE RCCL group of ncclSend (each rank,
 * the root included) / ncclRecv (root) moves the packed tile sums to the root over
 * xGMI, where they are scattered into out_frame (host, W x H x 3 f32 sums, [x][y]).
 * Bit-identical to prt_render / prt_render_tiles of the same frame for any n_scenes.
 * The communicator (ncclCommInitAll over the scenes' devices) is created on first use
 * and cached per device list; prt_comm_release() destroys the cached ones.  librccl
 * is loaded at first use: PRT_ERR_RCCL when it is missing.  Synchronous. */
int prt_render_multi(void* const* scenes, int n_scenes, const float* cam, int W, int H, int tile, int spp, int depth,
                     uint64_t seed, uint32_t flags, float* out_frame);
void prt_comm_release(void);
/* Root side of a one-process-per-GPU gather (pyrenderer_amd.distributed): the
 * packed tile sums d_packed (device, n_tiles*tw*th x 3 f32, slot order of prt_render_tiles) of the
 * host tile ids `tile_ids` -> the device frame d_frame (W x H x 3 f32, [x][y]; slots outside the
 * frame are dropped, pixels of other tiles untouched), one kernel enqueued on `stream` (NULL = the
 * scene's stream, whose device is used).  A tile id of -1 marks a padding slot (a rank with fewer
 * tiles than the gather buffer's per-rank stride): its pixels are dropped.  The tile origins are
 * uploaded only when the tile set differs from the previous call's.  Replaces a host-side unpack
 * of the gathered buffers. */
int prt_scatter_tiles(void* scene, const float* d_packed, const int32_t* tile_ids, int n_tiles, int tw, int th,
                      int W, int H, float* d_frame, void* stream);
/* ABI 3: the root's scatter of a whole multi-frame gather in ONE launch.  d_packed holds n_groups
 * blocks (one per rank, rank r's at d_packed + r * group_pitch floats), each with n_frames frames of
 * group_tiles tile slots (frame f at + f * src_frame_pitch floats); tile_ids = n_groups * group_tiles
 * host ids (rank-major, -1 = padding).  Frame f goes to d_frames + f * W*H*3 floats ([x][y]).  The
 * launch covers n_groups * group_tiles slots per frame: the per-rank padding of a ragged shard is
 * one tile list, not (world - 1) * n_frames other frames' slots.  ABI 4: with n_groups
 * > 1, group_pitch >= (n_frames - 1) * src_frame_pitch + group_tiles * tw * th * 3, else PRT_ERR_ARG. */
int prt_scatter_frames(void* scene, const float* d_packed, const int32_t* tile_ids, int n_groups, int group_tiles,
                       int64_t group_pitch, int tw, int th, int W, int H, int n_frames, int64_t src_frame_pitch,
                       float* d_frames, void* stream);
/* Progressive rendering: main_taichi.py:108-127 runs render() once per GUI frame
 * (pixels[x,y] += L, samples[x,y] += 1) and displays the running mean.  This call
 * renders samples first_sample .. first_sample+spp-1 of every pixel (the same
 * (seed, pixel, sample) random streams as prt_render_tiles) and adds them, in
 * sample order, onto io_sum (host, n_tiles*tw*th x 3 f32, same slot order):
 * calls covering samples [0, a), [a, b), ... leave io_sum bit-identical to one
 * prt_render_tiles call of b samples.  Synchronous. */
int prt_render_tiles_accumulate(void* scene, const float* cam, int W, int H, int tw, int th,
                                const int32_t* tile_ids, int n_tiles, int first_sample, int spp, int depth,
                                uint64_t seed, uint32_t flags, float* io_sum);
/* Same work, result left in device memory `d_out_sum` (n_slots x 3 f32) and
 * enqueued on `stream` (a hipStream_t; NULL = the scene's own stream) without
 * a host synchronisation. tile_ids is a host array.  The scene keeps one set of
 * work buffers per stream (up to 8), so renders enqueued on distinct streams may
 * execute concurrently on the device (e.g. frame k's drain overlapping frame
 * k+1's start); renders on one stream are ordered as usual.  PRT_FLAG_STATS
 * counters are shared by all streams. */
int prt_render_tiles_device(void* scene, const float* cam, int W, int H, int tw, int th,
                            const int32_t* tile_ids, int n_tiles, int spp, int depth, uint64_t seed,
                            uint32_t flags, float* d_out_sum, void* stream);
/* Several frames through the same persistent launches (the progressive frame loop of
 * main_taichi.py:108-118, or repeated renders of one frame): frame f = samples
 * f * frame_stride + 0 .. spp - 1 of every pixel of the tile set (frame_stride = spp: consecutive
 * progressive frames; 0: n_frames renders of the same samples), its per-pixel sums written to
 * d_out_sums + f * out_pitch floats (device, slot order of prt_render_tiles; out_pitch 0 = packed
 * frames, n_tiles*tw*th*3; otherwise >= that, e.g. the padded per-frame slot of a gather
 * buffer — the floats between a frame's sums and the next frame are not written).  Every frame is
 * bit-identical to the prt_render_tiles_accumulate call of its samples from zero sums; the
 * launches carry all frames' (pixel, sample) items (as many frames per launch as the per-launch
 * buffer budget holds), so a persistent launch ramps up and drains once per launch instead of
 * once per frame.  Enqueued on `stream` like prt_render_tiles_device. */
int prt_render_frames_device(void* scene, const float* cam, int W, int H, int tw, int th,
                             const int32_t* tile_ids, int n_tiles, int spp, int depth, uint64_t seed,
                             int n_frames, int frame_stride, uint32_t flags, float* d_out_sums, int64_t out_pitch,
                             void* stream);
/* trace-kernel time of every render call made with PRT_FLAG_TIME since the
 * previous prt_kernel_timing() (synchronises on their events, then resets):
 * total ms and number of trace launches.  Also reports PRT_ERR_INTERNAL if the
 * traversal watchdog tripped in the last render of any stream (and clears the flags,
 * like prt_check_faults). */
int prt_kernel_timing(void* scene, double* ms_total, int64_t* launches);

/* Self-test of the kernels' exact-reciprocal fast sequence (prt_device.h rcp_fast_seq: v_rcp_f32, one
 * refinement, two corrections) against the IEEE division 1.0f / b for every one of the 2^32 floats
 * on `device`; mismatches8 = mismatches by the class of |b|: 0 zero, 1 denormal, 2 normal < 2^-40,
 * 3 [2^-40, 2^40] (the range the kernels use the sequence in), 4 (2^40, 2^126], 5 > 2^126 finite,
 * 6 infinite, 7 NaN (both results NaN count as equal).  ABI 3, round 5. */
int prt_selftest_rcp(int device, uint64_t* mismatches8);
/* ABI 4: the guards of the kernels' fast sequences, swept over all 2^32 floats b on `device`
 * (counts16, 10 used): 0 rcp_fast_seq mismatches against 1.0f / b that its guard accepts (the result
 * is a normal float) — the kernels rely on this being 0; 1 operands that guard sends to the division;
 * 2 all rcp mismatches; 3 rcp mismatches for normal |b| <= 2^126; 4 sqrt_fast_seq mismatches against
 * sqrtf that its guard accepts (b >= 2^-96) — must be 0; 5 operands sent to sqrtf; 6 all sqrt
 * mismatches; 7 sqrt mismatches in [2^-96, FLT_MAX]; 8 for +0 and normal b < 2^-96; 9 for denormal b
 * (NaN results count as equal). */
int prt_selftest_guards(int device, uint64_t* counts16);
/* Failure detection for renders whose result stays on the device (prt_render_tiles_device,
 * the torch.distributed path): synchronises the device, then reports PRT_ERR_INTERNAL if
 * the traversal watchdog tripped in the last render enqueued on any of this scene's
 * streams.  PRT_OK otherwise.  A flag is cleared once reported — by this call, by
 * prt_kernel_timing, or by the host-output entry points and prt_closest_hits, which check
 * their own launches — so a fault is never reported against a later, clean render. */
int prt_check_faults(void* scene);
/* World.hit_all for a batch of rays (mathematics/intersection_taichi.py:238-291):
 * rays = n x 8 f32 (o.xyz, t_min, d.xyz, t_max); hit_id = original triangle index,
 * n_tri + k for sphere k, -1 for a miss; hit_t = distance (0 on a miss).  Closest hit
 * among the triangles = minimal (t, id) with the strict t_min < t < t_max test.  The
 * spheres follow in index order against the triangles' result, by hit_sphere's rules
 * (intersection_taichi.py:15-36), which differ: the interval is closed at both ends (a
 * root equal to t_min or to t_max counts; the near root if it lies in the interval, else
 * the far one), so a sphere at the closest triangle's t takes the hit from it, and of
 * spheres with equal roots the highest index wins.  A NaN t_max (the reference's shadow
 * bound when the light sample shares the point's x) accepts no triangle and every
 * sphere root >= t_min.  PRT_HITS_ANY returns some hit in range instead (shadow
 * queries): a triangle if one is in range, else the first sphere in index order.
 * PRT_HITS_QUANTIZED traverses the quantised BVH4 of large scenes instead of the f32
 * one (same results). */
#define PRT_HITS_ANY 0x1u
#define PRT_HITS_QUANTIZED 0x2u
int prt_closest_hits(void* scene, const float* rays, int64_t n, uint32_t flags, int32_t* hit_id, float* hit_t);
/* World.hit_all's full 8-tuple for a batch of rays (mathematics/intersection_taichi.py:238-291,
 * with Quad.hit / Cube.hit's shading at the closest hit, shapes.py:76-110): rays as
 * prt_closest_hits; out = n x 16 f32 per ray:
 *   [0] hit_anything (0/1)  [1] t (closest_so_far: t_max on a miss)  [2:5] p = o + t d
 *   [5:8] normal (flipped toward the ray for two-sided BSDFs, shapes.py:101-102)
 *   [8] emissive (0/1)  [9:12] attenuation = bsdf.evaluate()  [12:15] scattered direction
 *   (cosine-hemisphere draw rotated into the normal frame, bsdf.py:29-34)  [15] pdf = |n.wi|/pi
 * (all zero after [1] on a miss).  The scatter draws 2 numbers from the stream keyed
 * (seed, ray index, 0) — the reference draws them inside hit_all (shapes.py:105) from
 * Taichi's stateful RNG, which cannot be reproduced.  Synchronous. */
int prt_hit_all(void* scene, const float* rays, int64_t n, uint64_t seed, uint32_t flags, float* out16);
/* PathTracer.trace for caller-supplied rays (core/tracing.py:116-155): the radiance of one
 * path per ray, depth `depth`.  rays = n x 8 f32 (o.xyz, unused, d.xyz, unused); out_rgb = n x 3
 * f32.  Ray i draws from the stream keyed (seed, i, 0) — render()'s streams minus the two
 * camera-jitter draws of main_taichi.py:93-94.  flags: PRT_FLAG_MIS_NEE / PRT_FLAG_VARIANT as for
 * the render calls.  Runs the persistent trace kernel of prt_render_tiles.  Synchronous. */
int prt_trace_rays(void* scene, const float* rays, int64_t n, int depth, uint64_t seed, uint32_t flags,
                   float* out_rgb);
/* ABI 3: the primary rays of a render, as camera_kernel generates them for the trace kernels
 * (main_taichi.py:89-95: u = (x + ti.random()) / (W - 1), v likewise, then CameraTaichi.gen_ray
 * core/camera_taichi.py:47-74, the jitter and any lens draws from the stream keyed (seed, pixel,
 * sample)): samples first_sample .. first_sample + spp - 1 of the tile set's pixels, item order
 * [sample][slot] (slot order of prt_render_tiles).  out8 = n x 8 f32: origin.xyz, the RNG state
 * after the camera's draws (u32 bits), direction.xyz, 0.  Parity / inspection entry point (the host
 * gen_ray of PackedCamera is checked against it).  ABI 4: rows of slots whose pixel lies outside
 * the frame (partial edge tiles) are all zeros.  Synchronous. */
int prt_camera_rays(void* scene, const float* cam, int W, int H, int tw, int th, const int32_t* tile_ids,
                    int n_tiles, int first_sample, int spp, uint64_t seed, float* out8);
/* The denoiser's first-hit features (the `feat` of the denoise section below) in one kernel: what
 * prt_camera_rays plus prt_hit_all plus per-pixel sums on the host composed before, without the
 * per-ray buffers and the copies between them.  Added under ABI 4: purely additive.  For every pixel
 * of the W x H frame and samples first_sample .. first_sample + samples - 1 in that order: the
 * render's own primary ray (the stream keyed (seed, pixel, sample), as prt_camera_rays), its closest
 * hit in PathTracer.trace's primary range (t_min 1e-5f, t_max 99999.9f; core/tracing.py:126-127),
 * and at a hit prt_hit_all's normal [5:8] and attenuation [9:12].  Eight f32 sums per pixel start
 * at +0 and take one term per sample in sample order — albedo.rgb, normal.xyz, t, 1 — all 0 at a
 * miss; then channels 0-5 = sum / (float)samples, 6 = t sum / fmaxf(hits, 1), 7 = hits /
 * (float)samples, each one IEEE f32 operation: the result is reproducible bit for bit and equals
 * the host composition (pyrenderer_amd.denoise.features_packed_host).
 *   out   W x H x 8 f32, [x][y]: albedo.rgb, shading normal.xyz, depth, hit fraction
 *   flags 0 or PRT_HITS_QUANTIZED (the quantised BVH4, same results)
 * W and H: 1..65535.  A frame of one row or column has no camera ray the render defines (u = (x + r) /
 * (W - 1)) and no render entry point takes it; it is accepted here for callers that size buffers by
 * it, and its pixels hold whatever IEEE arithmetic makes of the quotient.  NULL scene, cam or out, a
 * size outside that range, samples < 1, first_sample < 0, first_sample + samples > INT32_MAX, other
 * flags, or a BVH4 deeper than the hit queries take return PRT_ERR_ARG before any device call.
 * prt_features: host `out`, synchronous; reports a watchdog trip itself (PRT_ERR_INTERNAL). */
#define PRT_FEATURE_CHANNELS 8
int prt_features(void* scene, const float* cam, int W, int H, int first_sample, int samples, uint64_t seed,
                 uint32_t flags, float* out);
/* The same on the device: d_out (device, 16-byte aligned) is written by one kernel enqueued on
 * `stream` (a hipStream_t of the scene's device; NULL = the null stream) with no host
 * synchronisation, so a frame can go prt_render_tiles_device -> prt_scatter_tiles -> prt_denoise*_device
 * without leaving the device.  PRT_FLAG_TIME does not apply.  A watchdog trip is reported by
 * prt_check_faults, as for the device-output renders. */
int prt_features_device(void* scene, const float* cam, int W, int H, int first_sample, int samples, uint64_t seed,
                        uint32_t flags, float* d_out, void* stream);
/* trace-kernel variant chosen for this scene's large launches when flags select none:
 * out4 = {variant, BVH arity (4, or 8: an LDS reference kernel over the scene's eight-wide tree, env
 *         PRT_LDS_WIDTH), bit 0 scene LDS-resident | bit 1 quantised nodes | bit 2 (4) the scene's
 *         shade_fast: every albedo in [2^-40, 2^40] and every face normal's length in [0.5, 2], so the LDS
 *         kernels' shading quotients run under their cheap guards; clear: under div3's | bit 3 (8) the
 *         scene is plain: no sphere, metal or dielectric (bits 2 and 3 are the uploaded scene's own
 *         flags, the same for every launch),
 *         LDS traversal stack entries per lane: the instantiation set, or for the pooled kernel
 *         (7 / 8) the exact bound of its tree that its stack is sized to} */
int prt_scene_kernel(void* scene, int32_t* out4);
/* the same for one trace launch of n_items (pixel, sample) work items with these render flags: an
 * LDS-resident scene whose pool fits seven blocks per CU takes the block-pooled shadow kernel (7) at
 * every launch size (until round 6: the phase-aligned one (1) below eight items per resident lane) */
int prt_launch_kernel(void* scene, int64_t n_items, uint32_t flags, int32_t* out4);
/* counters of the last render call made with PRT_FLAG_STATS (synchronises) */
int prt_last_stats(void* scene, uint64_t* stats4);
/* Diagnostic words (u64) of the same call, written by the trace kernels' PRT_FLAG_STATS builds.  Words
 * 17.. and 24.. hold different things depending on which kernel ran: the phase-aligned kernel
 * (trace_kernel; variants 1-6) or the pooled one (trace_kernel_pool; variants 7, 8). */
#define PRT_DIAG_NODES 0          /* the four counters of prt_last_stats: BVH node visits, */
#define PRT_DIAG_TRIS 1           /* triangle tests, */
#define PRT_DIAG_EXT 2            /* extension queries, */
#define PRT_DIAG_SHADOW 3         /* shadow queries */
/* 4..10, trace_kernel only: wave-level shader clocks spent in work refill / traversal / shading, wave loop
 * iterations, active lanes summed over iterations, wave-level inner / leaf traversal trips */
#define PRT_DIAG_CLK_REFILL 4
#define PRT_DIAG_CLK_TRAV 5
#define PRT_DIAG_CLK_SHADE 6
#define PRT_DIAG_WAVE_ITERS 7
#define PRT_DIAG_ACTIVE_LANES 8
#define PRT_DIAG_WAVE_INNER 9
#define PRT_DIAG_WAVE_LEAF 10
#define PRT_DIAG_LANE_INNER 11    /* trace_kernel: lane-level inner traversal trips */
#define PRT_DIAG_LANE_LEAF 12     /* ... and leaf trips */
#define PRT_DIAG_MAX_STACK 13     /* deepest traversal stack (both kernels) */
#define PRT_DIAG_NONFINITE 14     /* samples whose radiance came out NaN or infinite (failure detection; 0 for
                                   * a sound scene; both kernels) */
#define PRT_DIAG_WAVE_TRI 15      /* trace_kernel: wave-level triangle-loop trips (max leaf size over the lanes
                                   * of each leaf trip) */
#define PRT_DIAG_MAX_QUERY 16     /* most BVH node visits of one query (both kernels) */
/* 17..21 after trace_kernel's phase-aligned schedule: wave clocks of the extension / shadow iterations,
 * their counts, and the lanes that queried in the shadow ones */
#define PRT_DIAG_PHASE 17
#define PRT_DIAG_PHASE_WORDS 5
/* 17..20 after trace_kernel_pool: wave E iterations, wave S iterations, lanes of the S iterations, shadow
 * rays answered by the light-triangle test */
#define PRT_DIAG_POOL 17
#define PRT_DIAG_POOL_WORDS 4
/* trace_kernel: queries with > 1000 node visits, and from PRT_DIAG_OUTLIER_LOG the first 16 of them in
 * records of 8 words: o.xyz, d.xyz, t_max (f32 bits), query kind << 32 | node visits */
#define PRT_DIAG_OUTLIERS 23
#define PRT_DIAG_OUTLIER_LOG 24
#define PRT_DIAG_OUTLIER_RECORDS 16
#define PRT_DIAG_OUTLIER_WORDS 8
/* trace_kernel_pool built with -DPRT_POOL_CLOCKS (tools/pool_clocks.py) instead: wave-level cycles in E's
 * shading and enqueue, at the barrier, in S, (unused), in the refill, in the extension traversal */
#define PRT_DIAG_POOL_CLOCKS 24
#define PRT_DIAG_POOL_CLOCKS_WORDS 6
/* trace_kernel_pool's lane table (tools/lane_table.py): (wave trips, lane trips) of E inner visits, E
 * triangle tests, S inner visits, S triangle tests, the shading block, the Lambert block, the loop
 * iteration and the resolve of shadow answers */
#define PRT_DIAG_LANE_TABLE 160
#define PRT_DIAG_LANE_TABLE_WORDS 16
#define PRT_DIAG_SUSPENDED 176    /* trace_kernel_pool: extension queries suspended, */
#define PRT_DIAG_RESUMED 177      /* ... and resumed */
#define PRT_DIAG_WORDS 192        /* words kept per scene; prt_diag_words reads 0 past them */
/* the first 16 diagnostic words */
int prt_diag_stats(void* scene, uint64_t* stats16);
/* the first n diagnostic words (words past PRT_DIAG_WORDS read 0) */
int prt_diag_words(void* scene, uint64_t* out, int n);

/* ------------------------------------------------------------ denoise ----
 * Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on albedo-demodulated radiance,
 * guided by first-hit features (the reference has no denoiser).  The entry points
 * below live in units of their own: they take no scene handle and report failures through
 * prt_denoise_last_error, not prt_last_error.
 *   color   W x H x 3 f32   mean radiance, [x][y]
 *   feat    W x H x 8 f32   per pixel: albedo.rgb, shading normal.xyz, depth, hit fraction
 *                           (prt_features / prt_features_device above compute them;
 *                           pyrenderer_amd.denoise.features is their front end)
 *   iterations 0..8         pass i uses the 5 x 5 B3-spline stencil at step 2^i
 *   params4 4 f32           sigma_c (colour), sigma_z (depth), eps_a (albedo floor of the
 *                           demodulation), eps_z (depth floor); all > 0 and finite
 *   out     W x H x 3 f32   filtered radiance
 * A pixel with hit fraction 0, and a pixel whose colour, demodulated colour or any of its eight
 * features is not finite, is returned bit for bit and is never a tap of another pixel; a depth
 * gradient that reaches such a neighbour's depth counts as 0.  Every other output pixel is finite
 * for finite features of magnitude below 2^60.  Every operation is an IEEE f32 add,
 * mul, div, sqrt, min, max or abs in a fixed order: the result is reproducible bit for bit
 * (tests/atrous_ref.py restates it in NumPy).
 * prt_denoise takes host pointers and is synchronous.  Bad arguments (NULL, W or H < 1 or > 32768,
 * iterations outside 0..8, a parameter that is not positive and finite) return PRT_ERR_ARG before
 * any device is touched. */
int prt_denoise(int device, const float* color, const float* feat, int W, int H, int iterations,
                const float* params4, float* out);
/* The same filter on device pointers, enqueued on `stream` (a hipStream_t of `device`; NULL = the
 * null stream) with no host synchronisation: for a progressive preview loop or the root of the
 * torch.distributed path, whose frames stay on the device.  d_work: scratch of at least
 * prt_denoise_work_bytes(W, H) bytes, 16-byte aligned, work_bytes its size; it may be reused by the
 * next call on the same stream.  d_out must not alias d_color. */
int prt_denoise_device(int device, const float* d_color, const float* d_feat, int W, int H, int iterations,
                       const float* params4, float* d_out, void* d_work, int64_t work_bytes, void* stream);
/* scratch bytes prt_denoise_device needs for a W x H frame (56 per pixel, rounded up to 256); 0 for
 * a shape the filter rejects */
int64_t prt_denoise_work_bytes(int W, int H);
/* message of the last failed prt_denoise / prt_denoise_device call on the calling thread */
const char* prt_denoise_last_error(void);

/* Variance-guided mode of the same filter (the spatial half of SVGF, Schied et al. 2017; DESIGN.md
 * §11).  Added under ABI 4 like the four entry points above: purely additive.  The colour
 * edge-stopping width is not a parameter: a 7 x 7 estimate of the per-pixel variance of the
 * demodulated luminance scales it, and the variance is carried through the passes, so the filter
 * widens where the image is noisy and narrows where it has converged.  color, feat, iterations, out,
 * the set-aside rule and the fixed operation order are those of prt_denoise
 * (tests/atrous_var_ref.py restates this mode in NumPy).
 *   params5 5 f32           sigma_l (luminance width in local standard deviations), sigma_z, eps_a,
 *                           eps_z (as above), eps_l (luminance floor, in demodulated radiance); all
 *                           > 0 and finite
 *   out_var W x H f32       optional (may be NULL): the variance estimate of the demodulated
 *                           luminance before any pass, 0 at pixels that are set aside — a noise map
 * The variance is always finite (one that overflows becomes 0).  Every other output pixel is finite
 * for features as above, demodulated radiance |color / max(albedo, eps_a)| <= 2^126 and albedo <= 1.
 * prt_denoise_var takes host pointers and is synchronous; bad arguments return PRT_ERR_ARG before
 * any device is touched, with the text in prt_denoise_last_error. */
int prt_denoise_var(int device, const float* color, const float* feat, int W, int H, int iterations,
                    const float* params5, float* out, float* out_var);
/* prt_denoise_var on device pointers, enqueued on `stream` with no host synchronisation (see
 * prt_denoise_device).  d_out_var may be NULL.  d_work: scratch of at least
 * prt_denoise_var_work_bytes(W, H) bytes, 16-byte aligned.  d_out must not alias d_color; d_out_var
 * must not alias d_out, d_color or d_feat. */
int prt_denoise_var_device(int device, const float* d_color, const float* d_feat, int W, int H, int iterations,
                           const float* params5, float* d_out, float* d_out_var, void* d_work, int64_t work_bytes,
                           void* stream);
/* scratch bytes prt_denoise_var_device needs for a W x H frame (60 per pixel, rounded up to 256); 0
 * for a shape the filter rejects */
int64_t prt_denoise_var_work_bytes(int W, int H);

/* Variance from per-pixel sample moments.  Added under ABI 4, purely additive.  Random
 * streams are keyed by (seed, pixel, sample), so spp samples rendered as K batches from zero sums
 * (prt_render_tiles_accumulate, prt_render_frames_device) give K independent batch means per pixel;
 * the sample variance of those means over K is the variance of the final mean.  It knows nothing of
 * neighbouring pixels, so unlike the 7 x 7 estimate it does not take an edge for noise; its square
 * root is a per-pixel standard-error map.
 *
 * prt_moments_add: a running Welford update over n_frames frames of per-pixel radiance SUMS.
 *   sums      n_frames frames of W x H x 3 f32 [x][y]; frame f starts at + f * frame_pitch floats
 *             (0 = packed, W * H * 3)
 *   n_samples samples per frame (every frame and every call on one state must use the same count)
 *   feat      W x H x 8 f32, as for prt_denoise; eps_a > 0 and finite
 *   io_state  W x H x 4 f32 [x][y], updated in place: k (frames seen, exact below 2^24), mean of the
 *             frames' luminances, M2, var_mean (the variance of that mean).  All zeroes = empty.
 * Per pixel and frame, in frame order, every operation one IEEE f32 operation in this association
 * (tests/moments_ref.py restates it in NumPy):
 *   c = S / n_samples;  I_c = feat[7] > 0 ? c_c / fmax(A_c, eps_a) : c_c;
 *   l = (0.2126 I_r + 0.7152 I_g) + 0.0722 I_b;  a frame whose l is not finite is skipped;
 *   k' = k + 1;  d = l - mean;  mean' = mean + d / k';  M2' = M2 + d * (l - mean')
 * and after the last frame var_mean = k >= 2 ? (M2 / (k - 1)) / k : 0, stored as 0 when not finite.
 * Adding frames in one call or split over several gives the same bits.  Finiteness: with |l| <= B both
 * factors of d * (l - mean') are at most 2B, the product at most 4 B^2, and M2 at most k B^2; the whole
 * state stays finite while k B^2 <= 2^127, i.e. |l| <= 2^62 for up to 8 frames and |l| <= 2^51 for 2^24.
 * Host pointers, synchronous.  Bad arguments (NULL, W or H outside 1..32768, n_frames < 1, a non-zero
 * frame_pitch below W * H * 3, n_samples not finite or < 1, eps_a not positive and finite) return
 * PRT_ERR_ARG before any device is touched, with the text in prt_denoise_last_error. */
int prt_moments_add(int device, const float* sums, int n_frames, int64_t frame_pitch, float n_samples,
                    const float* feat, float eps_a, int W, int H, float* io_state);
/* prt_moments_add on device pointers, enqueued on `stream` with no host synchronisation.  d_io_state
 * must be 16-byte aligned and must not overlap d_sums or d_feat. */
int prt_moments_add_device(int device, const float* d_sums, int n_frames, int64_t frame_pitch, float n_samples,
                           const float* d_feat, float eps_a, int W, int H, float* d_io_state, void* stream);
/* prt_denoise_var with the variance plane in_var (W x H f32 [x][y], e.g. channel 3 of a moments state
 * copied out) in place of the 7 x 7 estimate: at a pixel that is not set aside a value that is finite
 * and >= 0 is used as it is (-0 included), anything else — NaN, inf, a negative value — counts as 0;
 * a pixel that is set aside gets 0.  out_var (may be NULL) receives the variance actually used.
 * Everything else, the finiteness statement included, is prt_denoise_var's. */
int prt_denoise_var_given(int device, const float* color, const float* feat, const float* in_var, int W, int H,
                          int iterations, const float* params5, float* out, float* out_var);
/* prt_denoise_var_given on device pointers, enqueued on `stream` with no host synchronisation.  d_work:
 * prt_denoise_var_work_bytes(W, H) bytes, 16-byte aligned (no more than prt_denoise_var_device needs).
 * The aliasing rules of prt_denoise_var_device hold, and d_in_var must not alias d_out or d_out_var. */
int prt_denoise_var_given_device(int device, const float* d_color, const float* d_feat, const float* d_in_var,
                                 int W, int H, int iterations, const float* params5, float* d_out,
                                 float* d_out_var, void* d_work, int64_t work_bytes, void* stream);

/* Temporal accumulation.  Added under ABI 4, purely additive.  The previous frame's
 * integrated demodulated colour and luminance moments are reprojected through the first-hit features
 * into this frame's camera and blended with this frame: a source of colour and of variance for the
 * variance-guided filter while the camera moves.  Static geometry (prt_temporal_accumulate_motion below takes
 * moving objects), pinhole cameras, one device.
 *
 * State: W x H x PRT_TEMPORAL_CHANNELS f32 [x][y], two float4 per pixel: I.rgb (integrated demodulated
 * colour), h (history length, in frames), m1, m2 (integrated first and second moment of the demodulated
 * luminance), the variance plane value, 0.  No state is "empty": the first frame passes NULL for
 * prev_feat, prev_cam24 and prev_state (all three or none).
 *   color, feat   this frame's mean radiance (W x H x 3) and features (W x H x 8), as for prt_denoise
 *   cam24         this frame's camera record (PRT_CAM_FLOATS floats, a HOST pointer in both forms)
 *   prev_*        the previous frame's features, camera record (host) and state
 *   params8       alpha, alpha_m in [0, 1] (floors of the blend weights of colour and moments; 0 = a
 *                 plain running average), tau_n in [-1, 1], tau_z > 0, tau_a >= 0 (consistency bounds on
 *                 normal, relative depth and albedo), eps_a > 0 (the demodulation's albedo floor),
 *                 min_history >= 1, w_min in (0, 1]; all finite
 *   state         the new state; must not be prev_state (taps read neighbours)
 *   out_color     (may be NULL) W x H x 3, the integrated colour re-modulated
 *   out_var       (may be NULL) W x H, the state's variance plane
 * Per pixel p = (x, y), every operation one IEEE f32 operation in this association
 * (tests/temporal_ref.py restates it in NumPy):
 *  1. hit = F[7] > 0;  a_c = fmax(A_c, eps_a);  I_c = hit ? C_c / a_c : C_c;  l = (0.2126 I_r + 0.7152 I_g)
 *     + 0.0722 I_b.  A pixel with a channel of C, I or F that is not finite takes no part: its state is all
 *     zeroes (h = 0: it donates nothing later), out_color = C, out_var = the marker.
 *  2. Without history (a miss, the first frame, any failure below): state (I, 1, l, l * l, marker, 0).
 *     The marker is the quiet NaN 0x7fc00000: "no trustworthy temporal variance here".
 *  3. u = (x + 0.5) / (W - 1), v = (y + 0.5) / (H - 1);  rx = (u - 0.5) * sw / 0.5, ry likewise with sh;
 *     f_i = (((rx * side_i + ry * up_i) + (-fd) * back_i) + E_i) - E_i;  d = f / sqrt((f0^2 + f1^2) + f2^2);
 *     rel_i = (E_i + Z * d_i) - Eprev_i;  r = sqrt((rel0^2 + rel1^2) + rel2^2);
 *     a, b, c = (rel0 * k_0 + rel1 * k_1) + rel2 * k_2 for k the previous side, up, back;
 *     px = (0.5 + ((0.5 * fd') * a) / (sw' * -c)) * (W - 1) - 0.5, py likewise with b, sh' and H.
 *  4. Only if c < 0 && px > -1 && px < W && py > -1 && py < H (a NaN fails): x0 = floor(px),
 *     fx = px - x0, likewise y; no index is formed before this test and none outside the frame is loaded.
 *  5. Taps q = (x0 + jx, y0 + jy), jx outer, jy inner, weight w = wx[jx] * wy[jy] with wx = (1 - fx, fx).
 *     A tap counts when it is inside the frame, h_q > 0, Fprev_q[7] > 0,
 *     (N_p.x N_q.x + N_p.y N_q.y) + N_p.z N_q.z >= tau_n, |Zprev_q - r| <= tau_z * r and
 *     max_c |Aprev_q,c - A_p,c| <= tau_a.  sum_w += w; acc_k += w * state_q,k for k = I.rgb, h, m1, m2.
 *  6. If sum_w >= w_min: hist = acc / sum_w;  h' = hist.h + 1;  ac = fmax(1 / h', alpha),
 *     am = fmax(1 / h', alpha_m);  I' = hist.I + ac * (I - hist.I);  m1' = hist.m1 + am * (l - hist.m1);
 *     m2' = hist.m2 + am * (l * l - hist.m2).  Otherwise step 2.
 *  7. var = fmax(0, m2' - m1' * m1') * ac if h' >= min_history, else the marker.
 *  8. Two bytewise equal camera records: the one tap q = p with weight 1 and r = Z_p, steps 3 and 4
 *     skipped, the tests of step 5 kept.  With alpha = alpha_m = 0 a static sequence is a running mean.
 * out_color = hit ? I' * a : I'.  A frame with W = 1 or H = 1 divides by zero in step 3; its pixels fail
 * step 4 and come out as step 2 (a static one accumulates).  Finiteness: the state of a pixel that takes
 * part is finite while |I_c| <= 2^62.
 * Host pointers, synchronous.  Bad arguments (NULL, some but not all of prev_* NULL, W or H outside
 * 1..32768, a parameter outside its range or not finite, a camera record that is not finite or has an
 * aperture > 0 — a thin lens has no unique reprojection —, state == prev_state) return PRT_ERR_ARG
 * before any device is touched, with the text in prt_denoise_last_error. */
#define PRT_TEMPORAL_CHANNELS 8
int prt_temporal_accumulate(int device, const float* color, const float* feat, const float* cam24,
                            const float* prev_feat, const float* prev_cam24, const float* prev_state, int W, int H,
                            const float* params8, float* state, float* out_color, float* out_var);
/* prt_temporal_accumulate on device pointers (cam24 and prev_cam24 stay host pointers, read before the
 * call returns), enqueued on `stream` with no host synchronisation.  d_state and d_prev_state must be
 * 16-byte aligned; no output may alias an input or another output. */
int prt_temporal_accumulate_device(int device, const float* d_color, const float* d_feat, const float* cam24,
                                   const float* d_prev_feat, const float* prev_cam24, const float* d_prev_state,
                                   int W, int H, const float* params8, float* d_state, float* d_out_color,
                                   float* d_out_var, void* stream);
/* Temporal accumulation across moving objects (DESIGN.md §11 "Moving objects").  Added under ABI 4, purely
 * additive: prt_temporal_accumulate and its device form are unchanged.  Rigid per-object motion and SVGF's
 * mesh-id test; pinhole cameras, one device.  prt_temporal_accumulate's arguments, plus:
 *   ids        W x H i32 [x][y]: this frame's object id per pixel (any int32; e.g. -1 at a miss)
 *   prev_ids   the previous frame's plane; NULL together with prev_feat, prev_cam24 and prev_state
 *   motion     n_objects x 12 f32: per object a row-major 3 x 4 matrix M that takes a world position of THIS
 *              frame to the same material point's world position in the PREVIOUS frame.  A device pointer in
 *              the device form; the host form copies it.  NULL is allowed only when n_objects == 0
 *   n_objects  0..1048576
 * The contract is prt_temporal_accumulate's steps 1-8 with these changes, every operation one IEEE f32
 * operation in this association (tests/temporal_ref.py restates them as its `ids` clauses):
 *  Id and row.  An id is valid when 0 <= id < n_objects.  Any other id (-1, too large, INT_MIN) has no row: its
 *     pixel reprojects as the static path does and no table entry is read for it.  A valid id whose row holds
 *     an entry that is not finite means "no previous pose": the pixel takes step 2, decided before anything is
 *     projected.
 *  3'. X_i = E_i + Z * d_i as in step 3.  For a valid id Xp_i = ((M[i][0] X_0 + M[i][1] X_1) + M[i][2] X_2) + M[i][3]
 *     and Np_i = (M[i][0] N_0 + M[i][1] N_1) + M[i][2] N_2; otherwise Xp = X and Np = N.  rel_i = Xp_i - Eprev_i;
 *     the rest of steps 3 and 4 is unchanged.
 *  5'. A tap additionally needs prev_ids[q] == ids[p], a plain int32 comparison that also applies to invalid
 *     ids.  The normal test uses Np, the depth test the r obtained from Xp.
 *  8'. The one-tap shortcut (q = p, w = 1, r = Z) is decided per pixel: it applies when the two camera records
 *     are bytewise equal AND the id is invalid or its row is bytewise (1,0,0,0, 0,1,0,0, 0,0,1,0).  A row that
 *     is the identity but for a -0 goes the long way.  A static camera watching one moving object still gives
 *     exact running means everywhere else.
 * Finiteness: prt_temporal_accumulate's statement holds.  A finite row times a finite position may overflow;
 * the resulting inf or NaN fails step 4 (a comparison with a NaN is false) before any index is formed, and the
 * pixel takes step 2.
 * Bad arguments (those of prt_temporal_accumulate; ids NULL; prev_ids not NULL together with the rest of prev_*;
 * n_objects < 0 or > 1048576; motion NULL with n_objects > 0) return PRT_ERR_ARG before any device is touched,
 * with the text in prt_denoise_last_error. */
int prt_temporal_accumulate_motion(int device, const float* color, const float* feat, const float* cam24,
                                   const float* prev_feat, const float* prev_cam24, const float* prev_state,
                                   const int32_t* ids, const int32_t* prev_ids, const float* motion, int n_objects,
                                   int W, int H, const float* params8, float* state, float* out_color, float* out_var);
/* ... on device pointers (cam24 and prev_cam24 stay host pointers), enqueued on `stream` with no host
 * synchronisation.  prt_temporal_accumulate_device's alignment and aliasing rules hold, with d_ids, d_prev_ids
 * and d_motion among the inputs. */
int prt_temporal_accumulate_motion_device(int device, const float* d_color, const float* d_feat, const float* cam24,
                                          const float* d_prev_feat, const float* prev_cam24,
                                          const float* d_prev_state, const int32_t* d_ids, const int32_t* d_prev_ids,
                                          const float* d_motion, int n_objects, int W, int H, const float* params8,
                                          float* d_state, float* d_out_color, float* d_out_var, void* stream);
/* prt_denoise_var_given with a spatial fallback: the 7 x 7 estimate of prt_denoise_var runs first, then
 * in_var replaces it at every pixel that is not set aside where it is finite and >= 0 (-0 included);
 * anywhere else — NaN (the temporal marker), inf, a negative value — the estimate stays.  out_var (may be
 * NULL) receives the variance actually used.  With in_var all NaN it is prt_denoise_var, with in_var all
 * finite and >= 0 prt_denoise_var_given, bit for bit.  Everything else is prt_denoise_var_given's. */
int prt_denoise_var_mixed(int device, const float* color, const float* feat, const float* in_var, int W, int H,
                          int iterations, const float* params5, float* out, float* out_var);
int prt_denoise_var_mixed_device(int device, const float* d_color, const float* d_feat, const float* d_in_var,
                                 int W, int H, int iterations, const float* params5, float* d_out,
                                 float* d_out_var, void* d_work, int64_t work_bytes, void* stream);

/* Adaptive sampling.  Added under ABI 4, purely additive.  Random streams are keyed by
 * (seed, pixel, sample) and every render entry point takes a tile list, so batch b of a subset of tiles
 * holds, for those tiles, exactly the bits a full-frame render of batch b would.  One fused kernel folds
 * such a batch into the frame's radiance sums and its prt_moments_add state and scores every listed tile
 * against a noise target; the caller stops rendering the tiles that have converged.
 *   batch      n_tiles * tw * th x 3 f32: the radiance SUMS of n_samples samples of the tiles tile_ids, in
 *              the slot order of prt_render_tiles (tile-major, then row ly, then column lx); slots outside
 *              the frame hold 0 and are ignored
 *   tile_ids   n_tiles i32, a HOST pointer in both forms (read before the call returns);
 *              id = ty * ceil(W / tw) + tx.  n_tiles == 0 is PRT_OK and does nothing
 *   tw, th     powers of two with tw * th in 64..2^20 (the render calls' rule);  W, H in 1..32768
 *   feat       W x H x 8 f32, as for prt_denoise; eps_a > 0 and finite
 *   n_samples  samples per batch, finite and >= 1 (every call on one state must use the same count)
 *   params2    eps_r > 0 and finite (the floor of the relative error's denominator), target >= 0 (+inf
 *              is allowed: only young pixels then hold a tile)
 *   io_sum     W x H x 3 f32 [x][y], updated in place
 *   io_state   W x H x 4 f32 [x][y], the state of prt_moments_add (k, mean, M2, var_mean), updated in place
 *   records    n_tiles x 4 u32 in the order of tile_ids, written
 * For every pixel of every listed tile that lies inside the frame, every operation one IEEE f32 operation in
 * this association (tests/adaptive_ref.py restates it in NumPy):
 *  1. io_sum_c = io_sum_c + S_c.
 *  2. prt_moments_add's update for the one frame S with its closing step: c = S / n_samples;
 *     I_c = feat[7] > 0 ? c_c / fmax(A_c, eps_a) : c_c;  l = (0.2126 I_r + 0.7152 I_g) + 0.0722 I_b;  a batch whose
 *     l is not finite leaves k, mean and M2 as they are;  k' = k + 1;  d = l - mean;  mean' = mean + d / k';
 *     M2' = M2 + d * (l - mean');  var_mean = k' >= 2 ? (M2' / (k' - 1)) / k' : 0, stored as 0 when not finite.
 *  3. e = sqrt(fmax(var_mean, 0)) / (|mean'| + eps_r), a var_mean of -0 counting as +0: the relative standard
 *     error of the demodulated luminance.
 *  4. The pixel is young if k' < 2, and over if it is young or e > target.
 * The record of a tile: [0] its pixels inside the frame, [1] those that are over, [2] the bits of the
 * greatest e among those that are not young (0 if there is none), [3] those that are young.  The counts are
 * integers and the greatest of non-negative floats is the greatest of their bit patterns as integers, so
 * the four words do not depend on the order in which the pixels are combined: they are reproducible bit for
 * bit.  No sum of e over a tile is offered, because it would not be.  Pixels of tiles that are not listed,
 * and everything outside the frame, are neither read nor written by the kernel (the host form copies the
 * whole planes up and down: such pixels come back with the bits they had).  Finiteness: prt_moments_add's
 * statement holds for the state; with a finite state e is finite and >= +0.
 * Host pointers, synchronous.  Bad arguments (a NULL pointer with n_tiles > 0 or a NULL params2, W or H
 * outside 1..32768, tw or th not a power of two or tw * th outside 64..2^20, n_tiles < 0 or
 * n_tiles * tw * th >= 2^31, a tile id out of range, a tile id listed twice — two blocks would update the
 * same pixels —, n_samples not finite or < 1, eps_a or eps_r not positive and finite, a target that is NaN
 * or negative) return PRT_ERR_ARG before any device is touched, with the text in prt_denoise_last_error. */
int prt_adaptive_update(int device, const float* batch, const int32_t* tile_ids, int n_tiles, int tw, int th, int W,
                        int H, const float* feat, float eps_a, float n_samples, const float* params2, float* io_sum,
                        float* io_state, uint32_t* records);
/* prt_adaptive_update on device pointers (tile_ids and params2 stay host pointers), enqueued on `stream` with
 * no host synchronisation: d_records is zeroed on the stream, then the tile ids travel in the kernel
 * arguments, 896 tiles to a launch.  d_io_state must be 16-byte aligned; d_io_sum, d_io_state and d_records
 * must not overlap each other, d_batch or d_feat. */
int prt_adaptive_update_device(int device, const float* d_batch, const int32_t* tile_ids, int n_tiles, int tw, int th,
                               int W, int H, const float* d_feat, float eps_a, float n_samples, const float* params2,
                               float* d_io_sum, float* d_io_state, uint32_t* d_records, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PRT_H_ */
