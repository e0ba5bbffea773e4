/*
 * icon_amd.h - C ABI of the MI355X-native implicit-surface query engine for ICON.
 *
 * The reference (YuliangXiu/ICON) has no FFI / plugin registry on this path: the seam is two
 * Python call signatures plus module state.  This header is the boundary a
 * maintainer binds with ctypes; every entry point cites the reference
 * code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - all `d_*` pointers are DEVICE pointers (HIP), all `h_*` pointers are HOST pointers;
 *   - float data is float32, indices int64 (as in the reference) unless stated;
 *   - every call that launches work enqueues it on `stream` (a hipStream_t passed as void*) and
 *     returns without synchronising, except where the comment says "synchronises";
 *   - return value: 0 on success, non-zero error code otherwise; icon_last_error() returns a
 *     thread-local human-readable message.  No CPU fallback exists: without a GPU every compute
 *     entry point fails with ICON_ERR_HIP.
 */
#ifndef ICON_AMD_H
#define ICON_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICON_AMD_VERSION 100          /* 0.1.0 */

enum {
    ICON_OK = 0,
    ICON_ERR_ARG = 1,                 /* bad argument (null, shape, range)         */
    ICON_ERR_HIP = 2,                 /* HIP runtime error (message has details)   */
    ICON_ERR_UNSUPPORTED = 3,         /* shape outside what the kernels are built for */
    ICON_ERR_STATE = 4                /* call order violated (e.g. finish before features) */
};

/* prior_type of lib/net/HGPIFuNet.py:63 */
enum { ICON_PRIOR_ICON = 0, ICON_PRIOR_PAMIR = 1, ICON_PRIOR_PIFU = 2 };

/* How clipped ("outlier") points get their cmap channels, lib/net/HGPIFuNet.py:298-305.
 * REFERENCE reproduces the reference bit for bit: smpl_sdf[outlier].repeat(1,1,3) tiles the
 * list of outlier signs of the whole call, so the j-th outlier's channel k receives the sign of
 * outlier (3j+k) mod K.  LOCAL is the per-point rule (cmap := own sign). */
enum { ICON_CMAP_REFERENCE = 0, ICON_CMAP_LOCAL = 1 };

/* MLP arithmetic.  F32: v_mfma_f32_32x32x2_f32, bit-for-bit an f32 fma chain.  F16X3 (the DEFAULT
 * of the host layer): every product as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on v_mfma_f32_16x16x32_f16
 * with f32 accumulation (22-bit operands; ~1e-6 of the f32 result, 5x the rate) - f32-class.
 * Its range is f16's: an input or hidden activation beyond 65504 (a thousand times anything a body mesh produces; a mesh
 * squashed flat reaches it) would make the result NaN - the kernels flag such points and redo them in plain f32
 * (k_rescue_*, mlp_plain_device.h), so F16X3 returns a number wherever F32 does.
 * (Rounds 1-3 carried a third, explicitly NOT f32-equivalent mode - f16 main term + block-scaled fp6 cross terms, value 2 -
 *  that only ever ran the materialising pipeline; removed in round 4: it could never be the headline.) */
enum { ICON_PRECISION_F32 = 0, ICON_PRECISION_F16X3 = 1 };

/* nearest-triangle search strategy (both give identical results; BRUTE is the validation path) */
enum { ICON_SEARCH_BVH = 0, ICON_SEARCH_BRUTE = 1 };

/* Bad data in device buffers never faults: query points whose (projected) coordinates are NaN / Inf / beyond +-64 are
 * evaluated at +-64 - far outside the cube, occupancy 0 (the reference returns 0 * NaN there), an ordinary "outside" entry
 * of the call's outlier list; faces / tetrahedra that name a vertex that does not exist are skipped (icon_visibility,
 * icon_semantic_voxelize) or reported (icon_mesh_components, icon_mesh_create, which also refuses non-finite vertices). */

typedef struct icon_mesh icon_mesh_t;   /* per-image SMPL body: triangles, normals, BVH, ray bins   */
typedef struct icon_feat icon_feat_t;   /* per-image feature planes (and PaMIR volume), repacked    */
typedef struct icon_mlp  icon_mlp_t;    /* if_regressor weights, BatchNorm folded, MFMA operand order */
typedef struct icon_work icon_work_t;   /* reusable device workspace                                  */

const char *icon_last_error(void);
int icon_version(void);
/* number of HIP devices visible; 0 (not an error) when there is none */
int icon_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * Mesh: the per-image half of cal_sdf_batch (lib/dataset/mesh_util.py:357-372):
 *   Meshes(verts, faces).verts_normals_padded()            :367  (pytorch3d leaf)
 *   face_vertices(verts|normals|cmaps|vis, faces)          :369-372, lib/common/render_utils.py:149-163
 * plus the acceleration structures our kernels need (BVH over triangles, (y,z) ray bins).
 * The reference redoes this work on every query() call; here it is once per image.
 * d_verts [V,3] f32, d_faces [F,3] i64, d_cmap [V,3] f32, d_vis [V] f32 (the [1,V,1] tensor).
 * Built ON THE DEVICE (round 4), as the reference's own prologue runs on the device (mesh_util.py:367-372): kernels on
 * `stream`, no copy of the mesh to the host, no synchronisation - the handle is usable by later calls on the same
 * stream as soon as the function returns.  icon_mesh_create allocates the mesh's device memory itself (one hipMalloc;
 * icon_mesh_destroy frees it, which waits for the device); icon_mesh_create_arena builds into memory the CALLER owns
 * (>= icon_mesh_arena_bytes(V, F) bytes, 256-byte aligned, alive and untouched until the last call that uses the
 * handle has run) - with a caching allocator behind it nothing is allocated per image and nothing ever waits.
 * What the build finds wrong with its input (a face naming a missing vertex, a non-finite coordinate) cannot be
 * returned by a call that does not wait: such input is made harmless (vertex 0 / coordinate 0 - no fault) and
 * reported by icon_mesh_status.
 * ------------------------------------------------------------------------------------------- */
int icon_mesh_create(const float *d_verts, int64_t V, const int64_t *d_faces, int64_t F,
                     const float *d_cmap, const float *d_vis, void *stream, icon_mesh_t **out);
int icon_mesh_arena_bytes(int64_t V, int64_t F, int64_t *bytes);
int icon_mesh_create_arena(const float *d_verts, int64_t V, const int64_t *d_faces, int64_t F,
                           const float *d_cmap, const float *d_vis, void *d_arena, int64_t arena_bytes,
                           void *stream, icon_mesh_t **out);
int icon_mesh_destroy(icon_mesh_t *mesh);
/* Input check of the build.  wait != 0: blocks until the build has run; wait == 0: answers from a pinned host word
 * the build's last copy writes - *bits = -1 while it has not run yet (returns ICON_OK), otherwise a bit set:
 * 1 bad face index, 2 bad vertex coordinate (both: ICON_ERR_ARG, the checks the reference's tensors would fail in
 * kaolin), 4 the ray-bin lists did not fit (not an error: inside tests count crossings over all triangles), 8 an
 * internal check of the build failed (ICON_ERR_STATE). */
int icon_mesh_status(const icon_mesh_t *mesh, int wait, int *bits);
/* copy the area-weighted unit vertex normals [V,3] to a device buffer (for tests) */
int icon_mesh_vertex_normals(const icon_mesh_t *mesh, float *d_out, void *stream);
/* BVH statistics (waits for the build): out[0]=nodes, out[1]=max depth, out[2]=ray-bin entries, out[3]=max bin length,
 * out[4]=leaves, out[5]=triangle slots (= F: a slot is a position in the BVH order) */
int icon_mesh_stats(const icon_mesh_t *mesh, int64_t out[6]);

/* ---------------------------------------------------------------------------------------------
 * cal_sdf_batch, per-point half (lib/dataset/mesh_util.py:374-396):
 *   point_to_mesh_distance (kaolin leaf) :374, gathers :375-382,
 *   barycentric_coordinates_of_projection :319-354,383, weighted sums :385-391,
 *   check_sign (kaolin leaf) :393.
 * d_points [N,3]; outputs d_sdf [N], d_norm [N,3], d_cmap [N,3], d_vis [N] (0/1 as float),
 * optional d_face [N] int64 (nearest face index) and d_inside [N] uint8.  Unclipped, as
 * cal_sdf_batch returns them.  The points may come in any order: batches below 98,304 points are
 * searched one wavefront per point, larger ones as 64-point packets over a Morton ordering built on
 * the device (that path synchronises the stream once to free its scratch).
 * ------------------------------------------------------------------------------------------- */
int icon_sdf_query(const icon_mesh_t *mesh, const float *d_points, int64_t N,
                   float *d_sdf, float *d_norm, float *d_cmap, float *d_vis,
                   int64_t *d_face, uint8_t *d_inside, int search, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Feature planes: what index() samples (lib/net/geometry.py:21-43):
 *   d_planes [C,H,W] f32 - features[-1][0] from HGPIFuNet.filter (lib/net/HGPIFuNet.py:204-266);
 *   d_vol [Cv,D,H,W] f32 or NULL - VolumeEncoder output (PaMIR, lib/net/HGPIFuNet.py:321-325).
 * n_select = 2 for the icon prior (front/back halves chosen by feat_select,
 * lib/dataset/mesh_util.py:266-277), 1 otherwise - including the icon prior with smpl_feats that lack 'vis'
 * (configs/train/icon-mvp.yaml:40): every channel is then an MLP input (lib/net/HGPIFuNet.py:345-346).  Repacks to
 * channel-last so one bilinear tap is one to four 16-byte loads.
 * ------------------------------------------------------------------------------------------- */
int icon_feat_create(const float *d_planes, int C, int H, int W, int n_select,
                     const float *d_vol, int Cv, int Dv, int Hv, int Wv,
                     void *stream, icon_feat_t **out);
int icon_feat_destroy(icon_feat_t *feat);
/* icon prior: cfg.net.smpl_feats (lib/net/HGPIFuNet.py:301-309).  The MLP input is [img | sdf | cmap if has_cmap | norm if
 * has_norm]; 'sdf' is always present; 'vis' (it selects the feature half, :334-336) is n_select = 2 above, its absence
 * n_select = 1.  At most 15 input channels in all, or the query entry points return ICON_ERR_UNSUPPORTED.
 * Default: both (every configs/ *.yaml). */
int icon_feat_set_smpl_feats(icon_feat_t *feat, int has_cmap, int has_norm);

/* ---------------------------------------------------------------------------------------------
 * MLP (lib/net/MLP.py:8-72 as built by lib/net/HGPIFuNet.py:128-133): Conv1d(k=1) stack with
 * BatchNorm1d (eval) + LeakyReLU(0.01) after all but the last layer, raw input re-concatenated
 * (after the activations, MLP.py:62) before the layers flagged in is_res, no last_op (test mode).
 * HOST pointers, reference state_dict layout:
 *   h_W[l] [cout[l], cin[l]], h_b[l] [cout[l]],
 *   h_bn_gamma/beta/mean/var[l] [cout[l]] for l < n_layers-1 (NULL arrays => no norm).
 * Supported: n_layers == 4, cin[0] <= 15, cout = {512,256,128,1}, is_res = {0,0,1,1}
 * (every config in configs/ *.yaml).  BatchNorm is folded in float64 on the host.
 * ------------------------------------------------------------------------------------------- */
int icon_mlp_create(int n_layers, const int *cin, const int *cout, const int *is_res,
                    const float *const *h_W, const float *const *h_b,
                    const float *const *h_bn_gamma, const float *const *h_bn_beta,
                    const float *const *h_bn_mean, const float *const *h_bn_var,
                    float bn_eps, void *stream, icon_mlp_t **out);
int icon_mlp_destroy(icon_mlp_t *mlp);
/* MLP.last_op (lib/net/MLP.py:68-70): HGPIFuNet builds the regressor with last_op = nn.Sigmoid() unless cfg.test_mode
 * (lib/net/HGPIFuNet.py:133; every configs/ *.yaml sets test_mode: True, training / validation runs do not).  Applied to the
 * network output before the in_cube mask, in every precision. */
enum { ICON_LASTOP_NONE = 0, ICON_LASTOP_SIGMOID = 1 };
int icon_mlp_set_last_op(icon_mlp_t *mlp, int last_op);
/* MLP.forward on point-major input rows: d_x [N,16] f32 (channels cin[0]..15 ignored),
 * d_out [N].  precision: ICON_PRECISION_*. */
int icon_mlp_forward(const icon_mlp_t *mlp, const float *d_x, int64_t N, float *d_out,
                     int precision, void *stream);

/* workspace: grows on demand, reusable across calls on one stream */
int icon_work_create(icon_work_t **out);
int icon_work_destroy(icon_work_t *work);
/* Stage timing with HIP events recorded on the caller's stream (bench.py's live roofline leg).
 * After enabling, every icon_query_points / icon_grid_* call brackets its stages with events;
 * icon_work_stage_ms synchronises on the last one and returns milliseconds of the most recent
 * call: out_ms[0] = geometry pre-pass (nearest search, sign / outlier codes, count/scan/compact),
 *       out_ms[1] = row materialisation + outlier cmap patch (0 on the fused path),
 *       out_ms[2] = the MLP kernel alone (fused path: k_fused_f16x3, which also assembles the rows). */
int icon_work_profile(icon_work_t *work, int enable);
/* The fused MLP kernel is a persistent grid of one workgroup per CU that takes a CU whole (132 KiB of LDS, every register):
 * the kernels of a collective enqueued on another stream (the all_gather of the first half of a Z-slab, recon.py) cannot run
 * beside it.  n > 0 makes its grid n CUs smaller - the collective gets them; the MLP pays n / CUs.  Default 0. */
int icon_work_set_reserve_cus(icon_work_t *work, int n);
int icon_work_stage_ms(icon_work_t *work, float out_ms[3]);
/* More of the same profiled call: out[0] = the nearest-triangle search kernel ALONE (ms, HIP events around its launch; 0 if
 * the call had none), out[1] = shader cycles and out[2] = wall milliseconds of the fused MLP kernel's workgroup 0 (it brackets
 * its run with s_memtime and the constant-rate s_memrealtime), out[3] = out[1] / out[2] in MHz: the EFFECTIVE clock the
 * kernel ran at under its own load.  cycles = the code's invariant, MHz = the box's: bench.py prints both so that a slower
 * line can be told from a slower build without PMC files.  Synchronises like icon_work_stage_ms. */
int icon_work_profile_detail(icon_work_t *work, double out[4]);
/* ... and what EVERY workgroup of that launch of the fused MLP kernel did (it is a persistent grid of one workgroup per CU;
 * the launch ends with the slowest one).  rec[5 b + 0] = the XCD (HW_REG_XCC_ID) workgroup b ran on, [1] = its start in ms
 * after the earliest start, [2] = its span in ms (constant-rate counter), [3] = its shader cycles, [4] = the tiles of 256
 * lattice points it evaluated (static run + drawn from the pool).  *n = workgroups of the launch; at most cap records are
 * written.  bench.py derives roofline.wg_span_ms / per_xcd_clock_mhz / tail_ms from it. */
int icon_work_profile_workgroups(icon_work_t *work, double *rec, int cap, int *n);
/* The fused MLP kernel's tile partition: the tiles are cut into one contiguous span per workgroup; a workgroup evaluates the first
 * (1000 - permille) / 1000 of its span itself, the rest of every span is drawn in contiguous groups of `group` tiles (1 .. 127) by
 * the workgroups that finish first - from the spans of their own XCD first (one L2 per XCD), then from the others'.
 * permille = 0: all static.  Default 150, 2.  The result does not depend on the setting (bit for bit). */
int icon_work_set_steal(icon_work_t *work, int permille, int group);

/* ---------------------------------------------------------------------------------------------
 * HGPIFuNet.query (lib/net/HGPIFuNet.py:268-367) for explicit points:
 *   xyz = orthogonal(points, calib)                lib/net/geometry.py:46-61  (h_calib: 12 floats,
 *         row-major [3,4] = calibs[0,:3,:4]; NULL = identity as query_func passes,
 *         lib/common/train_util.py:340)
 *   icon : cal_sdf_batch + clipping (:285-305), index + feat_select (:335-336), cat (:343,359)
 *   pamir: index(im_feat, xy) ++ index(vol_feat, xyz)   (:348-354)
 *   pifu : index(im_feat, xy) ++ z                       (:356-357)
 *   preds = in_cube * regressor(point_feat)              (:274-275,361-363)
 * d_points [N,3] (the [1,3,N] tensor transposed), d_occ [N].
 * mesh may be NULL for the pamir / pifu priors.
 * ------------------------------------------------------------------------------------------- */
int icon_query_points(const icon_mesh_t *mesh, const icon_feat_t *feat, const icon_mlp_t *mlp,
                      int prior_type, float sdf_clip, int cmap_mode, const float *h_calib,
                      const float *d_points, int64_t N, float *d_occ,
                      int search, int precision, icon_work_t *work, void *stream);

/* The same with the calibration left on the device: d_calib = 12 floats, calibs[0,:3,:4] row-major
 * (HGPIFuNet.query receives `calibs` as a device tensor, lib/common/train_util.py:340-343); the
 * kernels read it themselves, so query() never synchronises the stream to copy it to the host. */
int icon_query_points_dcalib(const icon_mesh_t *mesh, const icon_feat_t *feat, const icon_mlp_t *mlp,
                             int prior_type, float sdf_clip, int cmap_mode, const float *d_calib,
                             const float *d_points, int64_t N, float *d_occ,
                             int search, int precision, icon_work_t *work, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched HGPIFuNet.query: B subjects per call, as the reference's own query takes them (points [B,3,N],
 * calibs [B,4,4], every feature stack [B,C,H,W], smpl_feat_dict tensors [B,...]; lib/net/HGPIFuNet.py:268-367,
 * lib/dataset/mesh_util.py:357-396).  The call is ONE point-mode call over the B*N points in subject-major order
 * (point i belongs to subject i / N): the outlier sign list of the reference cmap mode is therefore the reference's
 * batch-global list (smpl_sdf[outlier].repeat(1,1,3) flattens all B subjects, HGPIFuNet.py:303-305), and the number of
 * kernel launches does not depend on B.
 *
 * icon_mesh_batch_create: B meshes built by icon_mesh_create(_arena) (one subject each), which must outlive the batch.
 * V and F must agree (ICON_ERR_ARG otherwise).  check_sign(verts, faces[0], points) (mesh_util.py:393) uses subject 0's
 * faces for every subject: the batch compares every subject's faces with subject 0's ON THE DEVICE (no read-back) and
 * reports a difference through icon_mesh_batch_status, as the device mesh build reports bad input.  Enqueued on `stream`.
 * ------------------------------------------------------------------------------------------- */
typedef struct icon_mesh_batch icon_mesh_batch_t;
int icon_mesh_batch_create(const icon_mesh_t *const *meshes, int B, void *stream, icon_mesh_batch_t **out);
int icon_mesh_batch_destroy(icon_mesh_batch_t *mb);
/* bits = 0: the subjects share their faces; -1: the check has not run yet (wait = 0 never blocks); otherwise ICON_ERR_ARG
 * ("faces differ") with bits = ICON_MESH_BATCH_FACES_DIFFER.  wait = 1 synchronises with the check. */
#define ICON_MESH_BATCH_FACES_DIFFER 0x10
int icon_mesh_batch_status(const icon_mesh_batch_t *mb, int wait, int *bits);

/* B feature stacks d_planes [B,C,H,W] in ONE repack launch; the handle holds B plane sets at a fixed stride.  No volume:
 * the pamir prior adds one with icon_feat_batch_set_volume. */
int icon_feat_create_batch(const float *d_planes, int B, int C, int H, int W, int n_select, void *stream, icon_feat_t **out);

/* pamir prior at batch size B: the VolumeEncoder output of every subject, d_vol [B,Cv,D,H,W] f32 - what
 * self.ve(vol, intermediate_output=False) returns for the [B,3,D,H,W] semantic volume (lib/net/HGPIFuNet.py:324-325,
 * lib/net/VE.py:166-183) - packed by ONE launch into the layout icon_feat_create gives a single volume, B volumes at a
 * fixed stride.  Subject b's points sample subject b's volume (index(vol_feat, xyz), HGPIFuNet.py:349-353).
 * ICON_ERR_ARG: B other than the handle's, a handle that already holds a volume, bad sizes; ICON_ERR_UNSUPPORTED: Cv > 8.
 * Enqueued on `stream`; allocates once (the handle's volume), no synchronisation. */
int icon_feat_batch_set_volume(icon_feat_t *feat, const float *d_vol, int B, int Cv, int Dv, int Hv, int Wv, void *stream);

/* d_calibs [B,12] (calibs[:, :3, :4] row-major, DEVICE), d_points [B,N,3] (the [B,3,N] tensor transposed), d_occ [B,N].
 * mb: a batch of B meshes (icon prior), NULL otherwise; feat: a batch of B plane sets (icon_feat_create_batch) - for the
 * pamir prior with B volumes (icon_feat_batch_set_volume; MLP input [img(C) | vol(Cv)], HGPIFuNet.py:346-353).
 * ICON_ERR_UNSUPPORTED: search = ICON_SEARCH_BRUTE, a workspace with a tie rule; ICON_ERR_ARG: batch sizes that
 * disagree, B*N >= 2^31, a pamir call on a handle without a volume.  No synchronisation. */
int icon_query_points_batch(const icon_mesh_batch_t *mb, const icon_feat_t *feat, const icon_mlp_t *mlp,
                            int prior_type, float sdf_clip, int cmap_mode, const float *d_calibs,
                            const float *d_points, int64_t N, int B, float *d_occ,
                            int search, int precision, icon_work_t *work, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Dense lattice evaluation: one rank's Z-slab of reconEngine (lib/common/seg3d_lossless.py).
 * Lattice of `res`^3 points (res odd, :84-86), world mapping of batch_eval (:125-137) with
 * align_corners=True, b_min=[-1,1,-1], b_max=[1,-1,1] (apps/ICON.py:78-90), identity calibration
 * (lib/common/train_util.py:340); output layout [z, y, x] as `occupancys.view(..., D, H, W)`
 * (seg3d_lossless.py:171).  Evaluates planes z0 <= z < z1 into d_occ [(z1-z0), res, res].
 *
 * The result equals ONE query() call over the whole lattice in z,y,x order, i.e. what
 * Seg3dLossless computes with resolutions=[res].
 *
 * Single call (single GPU, or ICON_CMAP_LOCAL on any number of GPUs):
 * ------------------------------------------------------------------------------------------- */
int icon_grid_eval_slab(const icon_mesh_t *mesh, const icon_feat_t *feat, const icon_mlp_t *mlp,
                        int prior_type, float sdf_clip, int cmap_mode,
                        int res, int z0, int z1, float *d_occ,
                        int search, int precision, icon_work_t *work, void *stream);

/* Split form for Z-slab sharding with ICON_CMAP_REFERENCE, where the outlier sign list of the
 * WHOLE lattice is needed before any slab can finish:
 *   1. icon_grid_slab_features: SDF + gather for the slab; writes the slab's outlier signs
 *      (int8, +1/-1/0, lattice order) to d_signs_local (capacity (z1-z0)*res*res) and the
 *      count to *d_count_local (device int64).
 *   2. caller exchanges counts and sign lists between ranks (RCCL all_gather) and builds the
 *      concatenated list d_signs_global [K_total] in rank order;
 *   3. icon_grid_slab_finish: patches the slab's cmap channels from the global list
 *      (rank_offset = number of outliers in lower slabs) and runs the MLP. */
int icon_grid_slab_features(const icon_mesh_t *mesh, const icon_feat_t *feat,
                            int prior_type, float sdf_clip, int cmap_mode,
                            int res, int z0, int z1, int8_t *d_signs_local, int64_t *d_count_local,
                            int search, icon_work_t *work, void *stream);
int icon_grid_slab_finish(const icon_mlp_t *mlp, int res, int z0, int z1,
                          const int8_t *d_signs_global, int64_t k_total, int64_t rank_offset,
                          float *d_occ, int precision, icon_work_t *work, void *stream);
/* The single-collective form of the same protocol (no host read between the exchange and the MLP):
 *   1. icon_grid_slab_features_msg: phase 1, and the slab's message written to d_msg =
 *        [int64 K][K outlier signs in lattice order, 2 bits each (sign + 1), four to a byte, low bits first]
 *      (msg_bytes >= 8 + ceil(points of the slab / 4); every rank uses the same msg_bytes = stride);
 *   2. ONE all_gather of the fixed-size messages: rank r's message at d_gathered + r * stride;
 *   3. icon_grid_slab_finish_gathered: K, this rank's offset and the segment of every index are derived on the
 *      device from the headers.  Evaluates the planes [za, zb) of the slab (z0 <= za < zb <= z1) into the SLAB's
 *      buffer d_occ [(z1-z0), res, res]; it may be called several times for one prepared slab - the multi-GPU driver
 *      gathers the first half of a slab while the second half is computed.  d_gathered == NULL: no exchange
 *      (ICON_CMAP_LOCAL, or a single rank) - the slab's own sign list is the whole list.
 * Shell skip: in_cube is strict (lib/net/HGPIFuNet.py:274-275,363), so every lattice point with a coordinate of
 * exactly +-1 is multiplied by 0.  When the body's bounding box is farther from the cube's boundary than the clip
 * band is wide - then every shell point is an "outside" outlier without looking at the mesh - the search and the MLP
 * cover the interior only and the shell is written as 0 (results identical, 2.3 % less work at 257^3). */
int icon_grid_slab_features_msg(const icon_mesh_t *mesh, const icon_feat_t *feat,
                                int prior_type, float sdf_clip, int cmap_mode,
                                int res, int z0, int z1, void *d_msg, int64_t msg_bytes,
                                int search, icon_work_t *work, void *stream);
int icon_grid_slab_finish_gathered(const icon_mlp_t *mlp, int res, int z0, int z1, int za, int zb,
                                   const void *d_gathered, int64_t stride, int world, int rank,
                                   float *d_occ, int precision, icon_work_t *work, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The reference's own schedule: Seg3dLossless._forward_faster (lib/common/seg3d_lossless.py:152-265, the mode
 * apps/ICON.py:89 selects) - the coarsest lattice dense, every finer level only the voxels near the 0.5 boundary of the
 * trilinearly upsampled field (dilated by a 9^3 / 7^3 / 3^3 box, minus what was evaluated before), the last level
 * interpolated - entirely as kernels on `stream`: boundary test, dilation, compaction in the reference's point order,
 * one query() call per level (own outlier sign list), scatter, upsample; nothing is read back between the levels.
 * resolutions[n_levels]: ascending, odd, each 2 r - 1 of the one before (apps/ICON.py:62-66: 33, 65, 129, 257);
 * standard box / align_corners=True / identity calibration as icon_grid_eval_slab.  d_out [res_last^3] f32, [z][y][x].
 * h_counts [n_levels + 1] (host) or NULL: the points queried per level and, last, 1 when some voxel of the coarsest level
 * exceeds 0.5 (otherwise the reference returns None, :173-177) - filling it synchronises the stream once, at the end;
 * with NULL the call is asynchronous and icon_adaptive_counts reads them later.  ICON_PRECISION_F16X3 + ICON_SEARCH_BVH
 * only (ICON_ERR_UNSUPPORTED otherwise: the host layer drives the schedule itself then).
 * ------------------------------------------------------------------------------------------- */
int icon_adaptive_eval(const icon_mesh_t *mesh, const icon_feat_t *feat, const icon_mlp_t *mlp, int prior_type, float sdf_clip,
                       int cmap_mode, const int *resolutions, int n_levels, float balance, float *d_out, int64_t *h_counts,
                       int search, int precision, icon_work_t *work, void *stream);
int icon_adaptive_counts(icon_work_t *work, int n_levels, int64_t *h_counts, void *stream);
/* With h_counts the call synchronises at its end; the range safety net of the split-precision MLP (operands beyond the f16
 * range are redone in f32, per launch) is then checked ONCE for the whole schedule and a schedule that met such operands is
 * run a second time the per-launch way - same results, three launches fewer in every other case.  *n = how often that
 * happened on this workspace (diagnostics; no shipped checkpoint produces such operands). */
int icon_adaptive_reruns(icon_work_t *work, int *n);

/* ---------------------------------------------------------------------------------------------
 * The MLP input rows of a call, materialised: what HGPIFuNet.query concatenates into point_feat before the regressor
 * (lib/net/HGPIFuNet.py:329-359), point-major d_rows [N,16] f32: slots [0,c0) in the reference's channel order, zeros,
 * slot 15 = integer bits, value 8 set = in_cube (:274-275).  For regressors whose normalisation runs over the points of the call
 * (norm_mlp 'group' / 'instance', lib/net/MLP.py:35-41: the host derives the call's statistics, folds them like
 * BatchNorm and runs icon_mlp_forward on these rows) and for diagnostics.  Exactly one of h_calib / d_calib (or neither:
 * identity); icon_grid_rows: the lattice planes [z0,z1) as one call, shell included.
 * ------------------------------------------------------------------------------------------- */
int icon_query_rows(const icon_mesh_t *mesh, const icon_feat_t *feat, int prior_type, float sdf_clip, int cmap_mode,
                    const float *h_calib, const float *d_calib, const float *d_points, int64_t N, float *d_rows,
                    int search, icon_work_t *work, void *stream);
int icon_grid_rows(const icon_mesh_t *mesh, const icon_feat_t *feat, int prior_type, float sdf_clip, int cmap_mode,
                   int res, int z0, int z1, float *d_rows, int search, icon_work_t *work, void *stream);

/* Diagnostics: with precision F16X3 and the BVH search the query runs FUSED - the MLP input rows are
 * assembled in LDS by the MLP kernel itself and never reach HBM (icon_amd/csrc/fused_f16x3.hip).  on != 0
 * forces the materialising path (rows written by a feature kernel, patched, read back by the MLP kernel) that
 * the other precisions use; both give bit-identical results (tests/test_gpu_parity.py).  Process-wide. */
int icon_debug_set_unfused(int on);
/* Diagnostics, host only (no device is touched): the operand image the F16X3 kernels read, packed from a FOLDED network of
 * input width c0 <= 16.  h_W / h_b: the four layers, [cout][cin] row-major with cin = c0, 512, 256 + c0, 128 + c0.
 * img: 680 KiB of f16 bit patterns (icon_amd/csrc/mlp_f16x3_device.h: lane maps of the 16x16x32 MFMA), side: 1060 floats
 * (biases x weight scale | layer 3 per lane group | zeros), inv[3]: accumulator -> activation factors of layers 0..2,
 * scales[5]: weight scales of layers 0..2 and the activation scales of layers 0, 1 (tests/test_mlp_pack_host.py). */
int icon_debug_mlp_pack_f16x3(int c0, const float *const *h_W, const float *const *h_b, uint16_t *img, float *side,
                              float *inv, float *scales);
/* Diagnostics: host != 0 makes icon_mesh_create* build on the HOST (copy to the host, sequential builder, copy back,
 * synchronises) - the checker of the device build: both emit the same arrays bit for bit.  Process-wide; default device
 * (or ICON_AMD_MESH_BUILD=host in the environment).  icon_debug_mesh_layout: byte offsets of the arena sections
 * [dyn, vnormals, nodes, leaves, tris, attr, slot2face, face2slot, bin_start, bin_slots, end of bin_slots, total]. */
int icon_debug_set_mesh_build(int host);
int icon_debug_mesh_layout(int64_t V, int64_t F, int64_t out[12]);
/* the host builder on HOST buffers, no device involved: fills h_arena (zeroed by the caller) in the arena layout */
int icon_debug_host_mesh_build(const float *h_verts, int64_t V, const int64_t *h_faces, int64_t F,
                               const float *h_cmap, const float *h_vis, void *h_arena, int64_t arena_bytes);
/* Diagnostics: on == 0 evaluates and masks the shell of the lattice like every other point (the reference's own
 * order of operations) instead of skipping it; both give identical results.  Process-wide; default on
 * (or ICON_AMD_SHELL_SKIP=0 in the environment). */
int icon_debug_set_shell_skip(int on);
/* Test / A-B switches by name, process-wide; production leaves them alone.  "lattice_fast" (default 1): 0 makes every packet
 * of the 257^3-class search derive its own tile set-up instead of reading the per-call record.  "share_waves" (-1 = by launch
 * size): wavefronts that share one packet's walk, 1 / 8 / 16 (4: adaptive schedule only).  "share_ring" (0 = 64): forced
 * ring size of the shared walks' hand-over queue; "share_lose_push" (0 = none): ticket of the push that is announced but never
 * stored; "share_spin_log2" (0 = 18): the wait bound, 2^n polls - the torture / fault-injection tests of the error path below.
 * "qc_lanes" (0 = 8, the default mapping): 64 makes icon_query_color's rasteriser sweep a face with one whole wavefront,
 * icon_visibility's mapping - tools/time_query_color.py times the two against each other; the result does not depend on it.
 * "rn_lanes" (0 = the default: chosen from F and the image size): 8 makes icon_render_normal's rasteriser sweep a face's pixel box with eight lanes, 1 with
 * one thread - tools/time_render.py times the two against each other; the result does not depend on it.
 * "tt_chunk" (0 = the default, 32): 1..32 makes icon_render_turntable take that many views per chunk - the tests cross chunk
 * boundaries with a handful of views; the result does not depend on it, icon_render_turntable_bytes does. */
int icon_debug_set_option(const char *key, int value);
/* The searches of coarse lattices and of the adaptive schedule share one packet's BVH walk between the wavefronts of a
 * workgroup through an LDS queue (csrc/geom_device.h nearest_shared).  Every wait in that hand-over is bounded; a wave that
 * gives a wait up records what it waited for in the workspace's host-mapped error record, the walk terminates, and the host
 * reports it: ICON_ERR_STATE (message: code, workgroup, wave, ticket, queue counters) from icon_work_status - or from the
 * next icon_query_points / icon_grid_* / icon_adaptive_* call on the workspace, and from icon_adaptive_eval (with h_counts) /
 * icon_adaptive_counts for the schedule they have just synchronised on.  The record is cleared by the report.  Never
 * synchronises: synchronise the stream first for the verdict on a particular launch. */
int icon_work_status(icon_work_t *work);

/* ---- tie sensitivity of the nearest-triangle choice ---------------------------------------------------
 * lib/dataset/mesh_util.py:374-390: the winner of kaolin's point_to_mesh_distance decides the triangle whose
 * UNCLAMPED barycentric extrapolation gives norm / cmap / vis; around a vertex or an edge several triangles are
 * mathematically equidistant and the last bits of d^2 decide (PARITY UNPINNED: kaolin is not in the tree).
 * icon_sdf_query_ties reports, per point: d_face = the winner (S3: smallest d^2, lowest index on exact ties),
 * d_face2 = the runner-up (next-smallest (d^2, index) key; -1 if none) and d_ulps = how many float32 ulps the
 * runner-up's d^2 lies above the winner's, clipped to 255.  Synchronises the stream.
 * icon_work_set_tie_rule(work, 1, ulps) makes every BVH search issued through `work` pick, among the faces within
 * `ulps` ulps of the minimum d^2, the one with the HIGHEST index (rule 0 = the definition): running the pipeline
 * both ways measures how much of the output depends on the unpinned tie behaviour. */
int icon_sdf_query_ties(const icon_mesh_t *mesh, const float *d_points, int64_t N,
                        int32_t *d_face, int32_t *d_face2, uint8_t *d_ulps, void *stream);
int icon_work_set_tie_rule(icon_work_t *work, int rule, int ulps);

/* Diagnostics (synchronises): BVH work of the lattice traversal over planes [z0,z1):
 * out[0] = wavefronts (point blocks: 4^3 on fine lattices, 2^3 on coarse ones), out[1] = BVH nodes visited, out[2] = triangles
 * tested, both summed over wavefronts (every visit serves all lanes of the wavefront), out[3] = nodes + triangles of the
 * LONGEST walk (what a latency-bound launch - fewer packets than wave slots - waits for).  The walk on pair_box_bound ("box_clamp"
 * off), whatever the mesh was created with; the three calls below read the counters of one kernel. */
int icon_debug_traversal_stats(const icon_mesh_t *mesh, int res, int z0, int z1, uint64_t out[4]);
/* the lattice walk's leaf work: out = [packets, nodes visited, leaf pairs offered to the distance test, leaf pairs tested] */
int icon_debug_pair_stats(const icon_mesh_t *mesh, int res, int z0, int z1, uint64_t out[4]);
/* a superset of icon_debug_pair_stats (same kernel, same walk; out[0..3] are its four values): out = [packets, inner nodes visited (AABB and oriented parents together), leaf pairs offered,
 * leaf pairs tested, leaves visited, oriented parents visited (0 for a mesh created with the "node_box" option off)] */
int icon_debug_walk_stats(const icon_mesh_t *mesh, int res, int z0, int z1, uint64_t out[6]);
/* host only: the oriented-box rule of the leaf pairs (record, kind 0 oriented / 1 AABB / 2 never culled, lower bounds of d^2) */
int icon_debug_pair_box(const float *corners, int64_t n_pairs, const float *pts, int64_t n_pts, int shared_pts,
                        float *rec, int32_t *kind, float *bound);
/* host only: the oriented-box rule of a slot range (the node boxes): rec[15], kind of the n_tris triangles tris[i][3][3]; and the
 * walk's bound on PairBox-shaped records recs[i][16][2]: bound[i][c][j] = component c at point j (pts[j], or pts[i][j]) */
int icon_debug_range_box(const float *tris, int64_t n_tris, float *rec, int32_t *kind);
int icon_debug_box_bound(const float *recs, int64_t n_recs, const float *pts, int64_t n_pts, int shared_pts, float *bound);
/* host only: the same records by the "box_clamp" evaluation (half units, excess clamped to [0, 1]): a quarter of icon_debug_box_bound's
 * value bit for bit while no axis excess passes 2.0, less beyond; same layout */
int icon_debug_box_bound_half(const float *recs, int64_t n_recs, const float *pts, int64_t n_pts, int shared_pts, float *bound);

/* Seg3dLossless._forward_faster's None rule (lib/common/seg3d_lossless.py:173-177: the call returns None when nothing exceeds
 * 0.5 on the COARSEST lattice) for a dense device volume d_occ [res,res,res]: the coarsest lattice is the sub-lattice of strides
 * (sx, sy, sz).  *h_any = 1 when one of its points exceeds `level`, else 0.  One kernel writing a host-mapped word, then the call
 * waits for the stream - the same synchronisation point the reference's `(occupancys > 0.5).sum() == 0` is. */
int icon_volume_any_above(const float *d_occ, int res, int sx, int sy, int sz, float level, icon_work_t *work, void *stream, int *h_any);

/* ---------------------------------------------------------------------------------------------
 * Seg3dLossless.export_mesh (lib/common/seg3d_lossless.py:583-604): marching cubes at 0.5 on
 * occ[1:,1:,1:]; vertices returned as (x,y,z) in voxel units of the cropped grid
 * (verts[:, [2,1,0]]), faces with flipped winding (faces[:, [0,2,1]]).
 * h_occ: HOST [res,res,res] f32.  Two-call protocol: call with h_verts == NULL to get the counts,
 * then with buffers of that size.
 * ------------------------------------------------------------------------------------------- */
int icon_export_mesh(const float *h_occ, int res, float level,
                     float *h_verts, int64_t *n_verts, int64_t *h_faces, int64_t *n_faces);

/* The same on the device (the reference uses a CUDA marching cubes for grids <= 256^3,
 * lib/common/seg3d_lossless.py:597-602): d_occ is the DEVICE volume [res,res,res].
 * icon_mc_count classifies and scans, synchronises and returns the sizes; the caller allocates
 * d_verts [n_verts,3] f32 and d_faces [n_faces,3] i64 and calls icon_mc_emit on the same workspace.
 * Same vertices and triangles as icon_export_mesh (as sets; the order differs). */
int icon_mc_count(const float *d_occ, int res, float level, icon_work_t *work, void *stream,
                  int64_t *n_verts, int64_t *n_faces);
int icon_mc_emit(float *d_verts, int64_t *d_faces, icon_work_t *work, void *stream);
/* One Z-slab's share of the same triangulation (the sharded driver's gather="mesh": meshes instead of the volume cross xGMI).
 * Cell layers [zc0, zc1) only (a layer z reads the planes z + 1 and z + 2 of the volume, export_mesh's occ[1:,1:,1:] view);
 * d_occ is the address plane 0 of the full [res,res,res] volume WOULD have - only the planes the layers read (and, with halo,
 * plane zc1 + 1, the neighbour's first) are dereferenced, so a rank passes slab_ptr - first_plane * res^2.  halo = 1: the x / y
 * edge crossings of plane zc1 + 1 are emitted too (the layer below refers to them; the neighbour emits them as well).
 * icon_mc_emit_keyed also writes d_keys [n_verts] i64 = 3 * cell + edge direction: the vertex's place in the vertex order of the
 * whole-volume call - concatenating the ranks' outputs in rank order and merging equal keys (sorted unique) reproduces
 * icon_mc_count / icon_mc_emit on the whole volume, vertex for vertex and face for face. */
int icon_mc_count_range(const float *d_occ, int res, float level, int zc0, int zc1, int halo, icon_work_t *work, void *stream,
                        int64_t *n_verts, int64_t *n_faces);
int icon_mc_emit_keyed(float *d_verts, int64_t *d_faces, int64_t *d_keys, icon_work_t *work, void *stream);

/* ---- PaMIR semantic voxelisation ---------------------------------------------------------------------
 * replaces voxelize_cuda.forward_semantic_voxelization (external CUDA wheel, requirements.txt:34; call site
 * lib/net/voxelize.py:57-59, arguments of Voxelization.forward :119-137; volume_res 128, sigma 0.05 at
 * lib/net/HGPIFuNet.py:109-118).  PARITY UNPINNED (source and test vectors absent): semantics as defined in
 * oracle/icon_accel.c - voxel centre p = ((x,y,z)+0.5)/res - 0.5, inside = p in some tetrahedron,
 * out = inside * sum_v w_v code_v / (1e-3 + sum_v w_v), w_v = exp(-|p-v|^2 / (2 sigma^2)) over the surface vertices.
 * d_verts [V,3] f32 (the first V_surf are the SMPL surface vertices, the rest the added interior ones,
 * lib/dataset/TestDataset.py:160-163), d_code [V_surf,3] f32, d_tets [T,4] int64 vertex indices,
 * d_out [res,res,res,3] f32 in (z,y,x,c) order - the layout lib/net/voxelize.py:22 documents.  Synchronises. */
int icon_semantic_voxelize(const float *d_verts, int64_t V, int64_t V_surf, const float *d_code,
                           const int64_t *d_tets, int64_t T, int res, float sigma, float *d_out, void *stream);

/* The same for B subjects in one launch of each kernel, as Voxelization.forward takes a batch (lib/net/voxelize.py:119-137,
 * HGPIFuNet.py:316-324): d_verts [B,V,3] (each subject's padding already stripped with subject 0's count, :316-317), ONE
 * tetrahedron table d_tets [T,4] for every subject (update_param(smpl_tetra=voxel_faces[0]) tiles subject 0's, :321-323;
 * vertices_to_tetrahedrons indexes each subject's own vertices with it), ONE code table d_code [V_surf,3]
 * (smpl_vertex_code_batch is the table tiled; its length is the surface vertex count, voxelize.py:84-85,128-129),
 * d_occ a caller-supplied scratch of B*res^3 bytes, d_out [B,res,res,res,3].  Subject b is bit for bit what
 * icon_semantic_voxelize gives for its vertices.  Enqueued on `stream`: no allocation, no synchronisation. */
int icon_semantic_voxelize_batch(const float *d_verts, int B, int64_t V, int64_t V_surf, const float *d_code,
                                 const int64_t *d_tets, int64_t T, int res, float sigma, uint8_t *d_occ, float *d_out, void *stream);

/* ---- connected components of a triangle mesh --------------------------------------------------------
 * the engine of clean_mesh (lib/dataset/mesh_util.py:778-791: trimesh split, keep the component with the
 * most vertices; called on the marching-cubes output at apps/ICON.py:755-756).
 * d_faces [F,3] int64, d_labels [V] int32 out: the smallest vertex index of the vertex's component.
 * Synchronises the stream (reports out-of-range face indices). */
int icon_mesh_components(const int64_t *d_faces, int64_t F, int64_t V, int32_t *d_labels, void *stream);

/* clean_mesh (lib/dataset/mesh_util.py:778-791, called at apps/ICON.py:755-756 on the marching-cubes output) as ONE call:
 * trimesh's split(only_watertight=False) - components over FACE adjacency (two faces are adjacent when they share an edge that
 * exactly two faces use; faces meeting in a vertex only are not) - and the component with the most vertices kept (a pinch
 * vertex counts for every component it touches; ties: the component holding the lowest-index face); vertices and faces keep
 * their relative order, vertex indices are renumbered.  d_verts [V,3] f32, d_faces [F,3] i64 -> d_out_verts [V,3] f32,
 * d_out_faces [F,3] i32 (caller-allocated at the INPUT sizes; the first h_counts[0] vertices / h_counts[1] faces are
 * valid).  All device pointers; synchronises the stream once, for the two counts.  ICON_ERR_ARG for a face naming a vertex
 * that does not exist.  Scratch lives in `work`. */
int icon_clean_mesh(const float *d_verts, int64_t V, const int64_t *d_faces, int64_t F, float *d_out_verts, int32_t *d_out_faces,
                    int64_t *h_counts, icon_work_t *work, void *stream);

/* ---- SMPL vertex visibility ----------------------------------------------------------------------
 * replaces get_visibility (lib/dataset/mesh_util.py:280-316: pytorch3d rasterisation at 2^12 squared,
 * cull_backfaces, 1 face per pixel; vis[faces[unique(pix_to_face)]] = 1, faces[-1] included).
 * d_xy [V,2], d_z [V] exactly as the reference passes them (TestDataset.py:136-137 passes -z),
 * d_faces [F,3] int64, d_vis [V] float32 out in {0,1}.  Synchronises the stream (frees its z-buffer). */
int icon_visibility(const float *d_xy, const float *d_z, int64_t V, const int64_t *d_faces, int64_t F,
                    int image_size, float *d_vis, void *stream);

/* ---- vertex colours of the reconstructed mesh --------------------------------------------------------
 * replaces query_color (lib/common/render.py:60-84; called at apps/infer.py:531 on the cleaned marching-cubes mesh):
 *   vis = get_visibility(xy, z, faces[:, [0,2,1]]) - icon_visibility's rule on the corner-swapped faces, z as it is;
 *   colour = ((grid_sample(image, (x, -y), bilinear, zeros, align_corners=True) + 1) * 0.5) * 255 where vis == 1,
 *            ((n + 1) * 0.5) * 255 with n the S1 vertex normal of the faces as given where vis == 0.
 * d_verts [V,3] f32; d_faces [F,3], int64 when faces_int64 != 0 (icon_mc_emit), else int32 (icon_clean_mesh) - read in place;
 * d_image [3,H,W] f32; d_colors [V,3] f32 out; d_vis [V] f32 out in {0,1}, or NULL.  A face that names a vertex that
 * does not exist is skipped (it neither covers pixels nor adds to a normal) and counted: after the stream has been waited
 * for, the first int32 of the scratch holds the number of such faces.  d_scratch: device memory of at least
 * icon_query_color_bytes(V, F, image_size) bytes, 256-byte aligned, owned by the caller; its contents need not survive
 * between calls.  Enqueued on `stream`: no allocation, no synchronisation, nothing read back; results are bit-identical from
 * run to run. */
int icon_query_color_bytes(int64_t V, int64_t F, int image_size, int64_t *bytes);
int icon_query_color(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                     const float *d_image, int H, int W, int image_size, float *d_colors, float *d_vis,
                     void *d_scratch, int64_t scratch_bytes, void *stream);

/* ---- normal maps and depth maps of a mesh (the forward renderer) -------------------------------------
 * replaces Render.get_rgb_image / get_depth_map (lib/common/render.py:289-325: pytorch3d MeshRasterizer with
 * blur_radius = log(1/1e-4) * 1e-7 and 30 faces per pixel, vertex-normal textures, softmax blend with gamma = 1e-8) for the
 * four orthographic cameras of Render.load_meshes: cam 0 looks from +z, 1 from +x, 2 from -z, 3 from -x, +y is up, the
 * [-1,1] cube fills the image.  The blend is replaced by its limit, the nearest candidate (PARITY UNPINNED).
 * d_verts [V,3] f32; d_faces [F,3], int64 when faces_int64 != 0, else int32 - read in place; cam_ids: n_views (1..4) HOST
 * values 0..3; size: 8..2048.  d_images [n_views,3,size,size] f32 out in [-1,1], background 0; d_depth [n_views,size,size]
 * f32 out (view depth 100 -+ coordinate, background -1) or NULL; d_pix_to_face [n_views,size,size] int32 out (background -1)
 * or NULL.  With exactly two views the planes of cam 2 are mirrored left-right, as the reference does.  A face that names a
 * vertex that does not exist is skipped and counted: after the stream has been waited for, the first int32 of the scratch
 * holds the number of such faces.  d_scratch: device memory of at least icon_render_bytes(V, F, size, n_views) bytes,
 * 256-byte aligned, owned by the caller.  Enqueued on `stream`: no allocation, no synchronisation, nothing read back;
 * results are bit-identical from run to run. */
int icon_render_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes);
int icon_render_normal(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                       const int *cam_ids, int n_views, int size, float *d_images, float *d_depth, int32_t *d_pix_to_face,
                       void *d_scratch, int64_t scratch_bytes, void *stream);

/* ---- the soft silhouette of a mesh, forwards and backwards --------------------------------------------
 * replaces Render.get_silhouette_image (lib/common/render.py:200-213, 376-386: pytorch3d MeshRasterizer with
 * blur_radius = log(1/1e-4 - 1) * 5e-5, faces_per_pixel = 50, cull_backfaces, SoftSilhouetteShader with sigma = 1e-4) for the
 * cameras of icon_render_normal, and its gradient with respect to the vertices (the SMPL fit loop, apps/infer.py:163-273).
 * The rule is DESIGN.md 4.14 (PARITY UNPINNED); ALL candidates of a pixel enter the product, not the 50 nearest.
 * d_verts [V,3] f32; d_faces [F,3], int64 when faces_int64 != 0, else int32 - read in place; cam_ids: n_views (1..4) HOST
 * values 0..3; size: 8..2048.  forward: d_alpha [n_views,size,size] f32 out in [0,1], background 0.  backward: d_alpha as the
 * forward call wrote it, d_grad_alpha [n_views,size,size] f32, d_grad_verts [V,3] f32 out (every entry is written): the
 * gradient of sum(alpha * grad_alpha), summed over the views; candidate set and culling carry no gradient.  With exactly two
 * views the plane of cam 2 is mirrored left-right (alpha and grad_alpha alike).  A face that names a vertex that does not exist
 * is skipped and counted: after the stream has been waited for, the first int32 of the scratch holds the number of such faces.
 * d_scratch: device memory of at least icon_silhouette_bytes(V, F, size, n_views) bytes, 256-byte aligned, owned by the caller;
 * the backward call does not need what the forward call left there.  Enqueued on `stream`: no allocation, no synchronisation,
 * nothing read back; no floating-point atomics: both directions are bit-identical from run to run. */
int icon_silhouette_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes);
int icon_silhouette_forward(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                            const int *cam_ids, int n_views, int size, float *d_alpha,
                            void *d_scratch, int64_t scratch_bytes, void *stream);
int icon_silhouette_backward(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                             const int *cam_ids, int n_views, int size, const float *d_alpha, const float *d_grad_alpha,
                             float *d_grad_verts, void *d_scratch, int64_t scratch_bytes, void *stream);

/* ---- the gradient of the normal maps with respect to the vertices --------------------------------------
 * what Render.get_rgb_image back-propagates in the two optimisation loops of apps/infer.py (:200-217 losses["normal"],
 * :448-456 losses["cloth"]; pytorch3d: TexturesVertex(verts_normals_padded()) interpolated by differentiable barycentrics),
 * for the images icon_render_normal wrote.  The rule is DESIGN.md 4.15 (PARITY UNPINNED): the winner per pixel, the candidate
 * set and the clamp pattern of the barycentrics carry no gradient; the gradient flows through the clamped, renormalised
 * barycentrics of the winner into the NDC corners of its face, and through the S1 vertex normals (the normalisation, the sum
 * over the incident faces, the cross product) into the world coordinates - the latter summed over the views.  Depth maps and
 * pix_to_face are not differentiable.
 * d_verts, d_faces, faces_int64, cam_ids, n_views, size: as given to icon_render_normal.  d_pix_to_face [n_views,size,size]
 * int32: as that call wrote it, the left-right mirror of cam 2 in a two-view call included; it is only compared with face ids,
 * never used as an address: ids that name no face select nothing.  d_grad_images [n_views,3,size,size] f32 (mirrored alike);
 * d_grad_verts [V,3] f32 out (every entry is written; a vertex of no face gets 0): the gradient of sum(images * grad_images).
 * A face that names a vertex that does not exist is skipped and counted: after the stream has been waited for, the first int32
 * of the scratch holds the number of such faces.  d_scratch: device memory of at least
 * icon_render_normal_backward_bytes(V, F, size, n_views) bytes, 256-byte aligned, owned by the caller; the call does not need
 * what icon_render_normal left in ITS scratch.  Enqueued on `stream`: no allocation, no synchronisation, nothing read back;
 * no floating-point atomics: bit-identical from run to run and from int32 and int64 faces.  The debug option "rn_lanes"
 * chooses the mapping of the per-face sweep as it does for icon_render_normal. */
int icon_render_normal_backward_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes);
int icon_render_normal_backward(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                                const int *cam_ids, int n_views, int size, const int32_t *d_pix_to_face,
                                const float *d_grad_images, float *d_grad_verts,
                                void *d_scratch, int64_t scratch_bytes, void *stream);

/* ---- the frames of the turntable video ------------------------------------------------------------------
 * replaces the renders of Render.get_rendered_video (lib/common/render.py:327-374: one pytorch3d render per camera and mesh,
 * 360 cameras on a circle around the y axis, each frame copied to the host) by ONE call for all views of a mesh.  The rule is
 * DESIGN.md 4.18 (PARITY UNPINNED): the camera of azimuth a has its eye at (100 cos a, 0, 100 sin a) and looks at the origin, +y
 * up, under the orthographic projection of icon_render_normal; X = z c - x s, Y = y, D = (100 - x c) - z s with (c, s) the float32
 * pair of a.  Everything after the projection is icon_render_normal's rule; no view is mirrored.  At (1,0) / (0,1) / (-1,0) /
 * (0,-1) the float planes are those of cam 1 / 0 / 3 / 2.
 * d_verts [V,3] f32; d_faces [F,3], int64 when faces_int64 != 0, else int32 - read in place; d_cos_sin: DEVICE [n_views,2] f32,
 * the pairs (c, s) as icon_amd.render.turntable_cos_sin makes them; n_views: 1..1024; size: 8..2048.
 * d_canvas: uint8 [n_views,size,canvas_width,3] or NULL - view k's frame; the mesh's panel is columns x0 .. x0 + size - 1
 * (0 <= x0, x0 + size <= canvas_width) and NO byte outside the panel is written: several meshes and the input images share a
 * frame side by side.  A byte is (uint8) min(max(t * 255, 0), 255) of t = (b0 t0 + b1 t1) + b2 t2, t_k = (n_k + 1) * 0.5, channels in
 * the normal's x, y, z order; background 127.  d_images [n_views,3,size,size] f32 ((t - 0.5) * 2, background 0), d_depth
 * [n_views,size,size] f32 (background -1), d_pix_to_face [n_views,size,size] int32 (background -1): as icon_render_normal's, each
 * may be NULL; at least one of d_canvas / d_images is not.  A face that names a vertex that does not exist is skipped and
 * counted: after the stream has been waited for, the first int32 of the scratch holds the number of such faces.
 * The S1 normals are computed once per call; the views are rasterised in chunks (32 views, "tt_chunk"), so d_scratch - device
 * memory of at least icon_render_turntable_bytes(V, F, size, n_views) bytes, 256-byte aligned, owned by the caller - holds the
 * z-buffers of one chunk and does not grow with n_views beyond it.  Enqueued on `stream` as kernel launches only: no allocation,
 * no synchronisation, nothing read back, no floating-point atomics; results are bit-identical from run to run and from int32 and
 * int64 faces, whatever the chunk. */
int icon_render_turntable_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes);
int icon_render_turntable(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                          const float *d_cos_sin, int n_views, int size, uint8_t *d_canvas, int64_t canvas_width, int64_t x0,
                          float *d_images, float *d_depth, int32_t *d_pix_to_face,
                          void *d_scratch, int64_t scratch_bytes, void *stream);

/* ---- the cloth refinement step without the renderer, forwards and backwards ------------------------------
 * what one iteration of the cloth loop of apps/infer.py:405-476 computes besides its normal maps: the LocalAffine deformation
 * y = A x + b with the stiffness and rigidity means (lib/net/local_affine.py) and the mesh shape priors of
 * update_mesh_shape_prior_losses (lib/dataset/mesh_util.py:168-176: mesh_edge_loss, pytorch3d's mesh_normal_consistency and
 * mesh_laplacian_smoothing(method="uniform")).  The rule is DESIGN.md 4.16 (PARITY UNPINNED); every expression is evaluated in
 * float64 from the float32 inputs and rounded once.
 * Topology (icon_amd/cloth.py: ClothTopology builds it once per mesh): d_edges [E,2]; the neighbour lists d_nbr_off [V+1] /
 * d_nbr [2E] (row v: the other end of every edge at v, multiplicity kept); d_pairs [P,4] = (v0, v1, a, c), the face pairs over
 * an edge (v0, v1) with their third vertices; d_inc_off [V+1] / d_inc [4P] (row v: pair * 4 + slot for every slot of d_pairs
 * that holds v).  All of them int64 when index_int64 != 0, else int32 - read in place; an entry that names nothing is skipped.
 * B meshes share the lists: d_x [B,V,3], d_A [B,V,3,3], d_b [B,V,3,1], d_y [B,V,3] f32.  The scalars (d_stiffness, d_rigid,
 * d_edge, d_nc, d_laplacian) and their incoming gradients are DEVICE pointers to one f32 each; E = 0 gives stiffness 0 and
 * edge 0, P = 0 gives nc 0.  local_affine_backward: d_grad_A / d_grad_b of sum(y grad_y) + stiffness grad_stiffness + rigid
 * grad_rigid; x gets no gradient.  mesh_priors: d_verts [V,3] of ONE mesh; `terms` is a mask of ICON_PRIOR_*: a term left out
 * is not computed, its output is 0 and its incoming gradient is not read; d_grad_verts [V,3] out, every entry written.
 * d_scratch: device memory of at least icon_local_affine_bytes(B, V, E) / icon_mesh_priors_bytes(V, E, P) bytes, 256-byte
 * aligned, owned by the caller; a backward call does not need what the forward call left there, and
 * icon_local_affine_backward - a single gather - takes none.  Enqueued on `stream` (two
 * launches per call, one for icon_local_affine_backward, whatever the sizes): no allocation, no synchronisation, nothing read
 * back; no floating-point atomics: bit-identical from run to run and from int32 and int64 indices. */
enum { ICON_PRIOR_EDGE = 1, ICON_PRIOR_NC = 2, ICON_PRIOR_LAPLACIAN = 4 };
int icon_local_affine_bytes(int64_t B, int64_t V, int64_t E, int64_t *bytes);
int icon_local_affine_forward(const float *d_x, const float *d_A, const float *d_b, int64_t B, int64_t V,
                              const void *d_edges, int64_t E, int index_int64, float *d_y, float *d_stiffness,
                              float *d_rigid, void *d_scratch, int64_t scratch_bytes, void *stream);
int icon_local_affine_backward(const float *d_x, const float *d_A, const float *d_b, int64_t B, int64_t V,
                               const void *d_nbr_off, const void *d_nbr, int64_t E, int index_int64,
                               const float *d_grad_y, const float *d_grad_stiffness, const float *d_grad_rigid,
                               float *d_grad_A, float *d_grad_b, void *stream);
int icon_mesh_priors_bytes(int64_t V, int64_t E, int64_t P, int64_t *bytes);
int icon_mesh_priors_forward(const float *d_verts, int64_t V, const void *d_edges, const void *d_nbr_off, const void *d_nbr, int64_t E,
                             const void *d_pairs, int64_t P, int index_int64, float target_length, int terms,
                             float *d_edge, float *d_nc, float *d_laplacian, void *d_scratch, int64_t scratch_bytes, void *stream);
int icon_mesh_priors_backward(const float *d_verts, int64_t V, const void *d_edges, const void *d_nbr_off, const void *d_nbr, int64_t E,
                              const void *d_pairs, const void *d_inc_off, const void *d_inc, int64_t P, int index_int64,
                              float target_length, int terms, const float *d_grad_edge, const float *d_grad_nc,
                              const float *d_grad_laplacian, float *d_grad_verts, void *d_scratch, int64_t scratch_bytes, void *stream);

/* ---- SMPL linear blend skinning, forwards and backwards ---------------------------------------------------
 * lbs(betas, pose, ..., pose2rot=False) of lib/smplx/lbs.py:152-252 - what dataset.smpl_model computes per step of the body-fit
 * loop (apps/infer.py:163-273).  The rule is DESIGN.md 4.17, pinned to the reference's own lbs(); every expression is evaluated
 * in float64 from the float32 inputs and rounded once.  The rotation matrices need not be orthonormal: plain linear algebra.
 * Per subject b:  J = J_template + J_shapedirs betas;  rel_0 = J_0, rel_j = J_j - J_parent(j);  G_0 = [R_0 | rel_0],
 * G_j = G_parent(j) o [R_j | rel_j];  joints_j = G_j^t;  A_j = [G_j^R | G_j^t - G_j^R J_j];
 * v_posed = v_template + shapedirs betas + sum_p f_p posedirs[p], f = vec(R_j - I) over j >= 1 (joint-major, then row-major);
 * T_v = sum_k skin_w[v,k] A_skin_idx[v,k];  verts_v = T_v^R v_posed + T_v^t.
 * Tables (icon_amd/smpl.py: SmplModel builds them once per model; all device pointers, float32 / int32):
 *   v_template [3][V], shapedirs [NB][3][V], posedirs [P][3][V] - COMPONENT-MAJOR, vertex last: lane v of a wave reads the
 *   float next to lane v - 1's (the module's buffers are [V,3], [V,3,NB] and [P,3V]);
 *   J_template [J][3] = J_regressor v_template and J_shapedirs [J][3][NB] = J_regressor shapedirs, formed in float64 and rounded
 *   once (the joints are linear in betas: no call reduces over vertices for them);  parents [J], parents[j] < j for j >= 1;
 *   skin_idx / skin_w [V][K]: the non-zero weights of vertex v, joints ascending, rows padded with (0, 0.0).
 * A joint index outside 0..J-1 is skipped and a parent outside 0..j-1 is read as 0, so no entry is used as an address unchecked.
 * Limits: 1 <= J <= 64, 0 <= NB <= 512, B V < 2^31 (ICON_ERR_UNSUPPORTED); 1 <= K <= J, P == 9 (J - 1) (ICON_ERR_ARG).
 * icon_smpl_forward: d_betas [B,NB], d_rot_mats [B,J,3,3] -> d_verts [B,V,3], d_joints [B,J,3], and d_A [B,J,3,4], which the
 * caller keeps for the backward call of the same inputs.  Two launches.
 * icon_smpl_backward: d_grad_verts [B,V,3] / d_grad_joints [B,J,3], either may be NULL (a zero that is not read) -> d_grad_betas
 * [B,NB], d_grad_rot_mats [B,J,3,3], every entry written.  v_posed and T_v are recomputed; the 12 J + P + NB sums over vertices
 * go through per-workgroup partials in d_scratch (icon_smpl_bytes, 256-byte aligned, the caller's) and are added in a fixed
 * order by the launch that walks the chain backwards.  Two launches, one when d_grad_verts is NULL.
 * Enqueued on `stream`: no allocation, no synchronisation, nothing read back; no floating-point atomics: equal bytes from run
 * to run. */
typedef struct icon_smpl_tables {
    const float *v_template, *shapedirs, *posedirs, *J_template, *J_shapedirs;
    const int32_t *parents, *skin_idx;
    const float *skin_w;
    int64_t V;
    int32_t J, NB, K, P;
} icon_smpl_tables;
int icon_smpl_bytes(int64_t B, int64_t V, int J, int NB, int K, int64_t *bytes);
int icon_smpl_forward(const icon_smpl_tables *tables, const float *d_betas, const float *d_rot_mats, int64_t B,
                      float *d_verts, float *d_joints, float *d_A, void *stream);
int icon_smpl_backward(const icon_smpl_tables *tables, const float *d_betas, const float *d_rot_mats, int64_t B,
                       const float *d_A, const float *d_grad_verts, const float *d_grad_joints,
                       float *d_grad_betas, float *d_grad_rot_mats, void *d_scratch, int64_t scratch_bytes, void *stream);

/* ---- garment extraction: the submesh inside 2-D polygons, less the body parts a garment type excludes -------
 * replaces extract_cloth (lib/common/cloth_extraction.py:75-170, called at apps/infer.py:565-605) and the classifier of
 * smpl_to_recon_labels (:45-72).  The rule is DESIGN.md 4.19; every decision is an exact comparison in float64 on the float32
 * coordinates widened exactly, pinned to matplotlib's Path.contains_points and sklearn's KNeighborsClassifier(n_neighbors=1).
 * icon_nearest_vertex: d_verts [V,3] f32, d_src [Vs,3] f32 -> d_out_idx [V] int32: the LOWEST j minimising
 *   ((dx*dx + dy*dy) + dz*dz), d = verts[i] - src[j] (numpy's ((q - s)**2).sum(-1).argmin()).  d_only: uint8 [V] or NULL - a
 *   vertex whose byte is 0 is skipped and gets -1.  One launch; no allocation, no synchronisation.
 * icon_extract_cloth: d_verts [V,3] f32; d_faces [F,3], int64 when faces_int64 != 0, else int32 - read in place; d_poly_xy
 *   float64 [total_poly_verts,2], the polygons' vertices in the model's xy plane, polygon p being rows d_poly_off[p] ..
 *   d_poly_off[p+1] - 1 (d_poly_off: int32 [P+1], DEVICE; a range that leaves [0, total_poly_verts) or holds fewer than 3
 *   vertices selects nothing); d_src [Vs,3] f32 with d_src_remove uint8 [Vs], or all three NULL / 0: no source mesh.
 *     selected(i): (x, y) of vertex i lies inside ANY polygon - the crossings test, each polygon closed from its last vertex
 *                  to its first;  keep_v(i) = selected(i) and not src_remove[nearest source vertex of i] (no source mesh:
 *                  selected(i));  a face is kept when any of its corners has keep_v - a face that names a vertex outside [0, V)
 *                  never is;  out: the kept faces in order, the vertices they name in ascending order, faces renumbered.
 *   d_out_verts [V,3] f32, d_out_faces [F,3] int32, d_out_vert_ids [V] int32 (the input index of every output vertex):
 *   caller-allocated at the INPUT sizes; the first h_counts[0] vertices / h_counts[1] faces are valid (HOST int64 [2]).
 *   d_scratch: device memory of at least icon_extract_cloth_bytes(V, F, total_poly_verts, P) bytes, 256-byte aligned, owned by
 *   the caller; its contents need not survive between calls.  Enqueued on `stream`: one memset and seven launches (six without a
 *   source mesh) whatever V, F and P are, no allocation; then the stream is synchronised ONCE, to hand the two counts back, as
 *   icon_clean_mesh does.  No atomics: equal bytes from run to run and from int32 and int64 faces.  Coordinates are taken as
 *   finite. */
int icon_nearest_vertex(const float *d_verts, int64_t V, const float *d_src, int64_t Vs, const uint8_t *d_only,
                        int32_t *d_out_idx, void *stream);
int icon_extract_cloth_bytes(int64_t V, int64_t F, int64_t total_poly_verts, int64_t P, int64_t *bytes);
int icon_extract_cloth(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                       const double *d_poly_xy, const int32_t *d_poly_off, int64_t total_poly_verts, int64_t P,
                       const float *d_src, int64_t Vs, const uint8_t *d_src_remove,
                       float *d_out_verts, int32_t *d_out_faces, int32_t *d_out_vert_ids, int64_t *h_counts,
                       void *d_scratch, int64_t scratch_bytes, void *stream);

/* ---- the evaluator's normal maps and normal consistency ------------------------------------------------------
 * replaces Evaluator._render_normal / _get_reproj_normal_error / calculate_normal_consist / render_normal
 * (lib/dataset/Evaluator.py:58-177; an OpenGL renderer and trimesh's vertex_normals; call sites apps/ICON.py:556 and :639).
 * The rule is DESIGN.md 4.20 (PARITY UNPINNED): coverage at the pixel centres in exact integers on vertices snapped to 1/256
 * pixel, the top-left fill rule, near / far clipping at clip z = -1 / +1, the smallest (z, face id) wins, the interpolated
 * camera normal normalised per fragment, background (1, 1, 1, 0); a face with a |clip x| or |clip y| above 64 is not drawn.
 * Mesh a, and optionally mesh b (all of d_verts_b, d_faces_b, Vb, Fb null / 0: the single-mesh form, which only renders -
 * d_err, d_normals_b, d_rgba_b and d_pix_b must be null then): d_verts [V,3] f32; d_faces [F,3], int64 when faces_int64 != 0,
 * else int32 - read in place, a face that names a missing vertex is skipped; d_normals [V,3] f32 vertex normals, or NULL: the
 * call computes angle-weighted ones in float64 (trimesh's vertex_normals restated, rounded once to float32).
 * Views: d_view_mats [n_views,3,4] f32 - the affine model matrix of each view, row-major; d_view_muls [n_views,3] f32 - what
 * the camera normal's components are multiplied by.  DEVICE pointers, 1 <= n_views <= 32; 8 <= size <= 2048.
 * Outputs: d_err [n_views] float64 - per view the mean over the size^2 pixels of the squared RGB difference of the two meshes'
 * maps, each pixel's in float32, summed in float64 in a fixed tree; d_rgba_a / d_rgba_b [n_views,size,size,4] f32, 16-byte aligned, and
 * d_pix_a / d_pix_b [n_views,size,size] int32 (the winning face, -1: background): each written only when not NULL;
 * d_normals_out_a / d_normals_out_b [V,3] f32: where the call computes a mesh's vertex normals and this is not NULL, they are
 * left here (a mesh's normals are given or asked for, not both).
 * d_scratch: device memory of at least icon_normal_consistency_bytes bytes (same sizes), 256-byte aligned, owned by the caller;
 * its contents need not survive between calls.  Enqueued on `stream`, launches only (at most 19 whatever the sizes): no
 * allocation, no synchronisation, nothing read back; no floating-point atomics: equal bytes from run to run and from int32
 * and int64 faces. */
int icon_normal_consistency_bytes(int64_t Va, int64_t Fa, int64_t Vb, int64_t Fb, int size, int n_views, int64_t *bytes);
int icon_normal_consistency(const float *d_verts_a, int64_t Va, const void *d_faces_a, int64_t Fa, int faces_a_int64,
                            const float *d_normals_a, const float *d_verts_b, int64_t Vb, const void *d_faces_b, int64_t Fb,
                            int faces_b_int64, const float *d_normals_b, const float *d_view_mats, const float *d_view_muls,
                            int n_views, int size, double *d_err, float *d_rgba_a, float *d_rgba_b, int32_t *d_pix_a,
                            int32_t *d_pix_b, float *d_normals_out_a, float *d_normals_out_b, void *d_scratch,
                            int64_t scratch_bytes, void *stream);

/* ---- training samples: the points and labels of get_sampling_geo ---------------------------------------------
 * replaces PIFuDataset.get_sampling_geo (lib/dataset/PIFuDataset.py:483-607, is_sdf=False; called per item at :226-229).
 * The rule is DESIGN.md 4.21: nS = 4 N surface samples verts[id] + vert_normals[id] * (sigma_geo * normal), nU = N / 4 space
 * samples calib_inv (2 u - 1) and, when zray != 0, nS R z-ray samples (surface sample k / R through calib, its z moved by
 * 0.5 * (0.40 * normal), back through calib_inv), n = nS + nU + nS R in that order; slot i of the shuffled list holds source
 * perm(i).  Every draw is Philox4x32-10 of (seed, stream, index); float64 arithmetic in the stated order, rounded once to
 * float32.  Labels: the inside test of `scan` (the rule of icon_sdf_query's `inside`) on the float32 samples - trimesh's
 * `contains` in the reference, UNPINNED.  Balancing: more than N / 2 inside -> the first N / 2 inside and N / 2 outside samples
 * of the shuffled list, else every inside and the first N - n_in outside ones; inside rows first, labels 1 then 0.
 * scan: the scan's mesh handle, built on `stream` or finished; d_verts [V,3] f32, the vertices it was built from (V is the
 * handle's); d_vert_normals [V,3] f32, or NULL: the handle's own vertex normals (S1).  calib / calib_inv: HOST float64 [12],
 * rows of the affine [3][4] and of its inverse.  1 <= N < 2^24, 1 <= R <= 64, n < 2^31.
 * Outputs (device): d_samples [N,3] f32, d_labels [N] f32, d_counts int32 [2] = (inside rows, outside rows); rows past their
 * sum - only when the outside samples run short - are zero with label 0.  Optional, each NULL or [n]: d_all_samples [n,3] f32
 * and d_all_inside uint8, the shuffled list before balancing; d_all_source int32, perm(i); d_all_vertex int32, the vertex drawn
 * for the slot (-1 for a space sample).
 * d_scratch: device memory of at least icon_sample_geo_bytes(n) bytes, 256-byte aligned, owned by the caller; its contents
 * need not survive between calls.  Enqueued on `stream`, three launches whatever the sizes: no allocation, no synchronisation,
 * nothing read back; no atomics: equal bytes from run to run. */
int icon_sample_geo_bytes(int64_t n, int64_t *bytes);
int icon_sample_geo(const icon_mesh_t *scan, const float *d_verts, const float *d_vert_normals,
                    const double *calib, const double *calib_inv, int64_t N, double sigma_geo, int zray, int R,
                    uint64_t seed, float *d_samples, float *d_labels, int32_t *d_counts,
                    float *d_all_samples, uint8_t *d_all_inside, int32_t *d_all_source, int32_t *d_all_vertex,
                    void *d_scratch, int64_t scratch_bytes, void *stream);

/* ---- training: the regressor's input rows of every feature stack, and their gradient into the planes ----------
 * HGPIFuNet.query in training mode up to the regressor (lib/net/HGPIFuNet.py:268-359) for the icon and pifu priors; the rule
 * is DESIGN.md 4.22.  The B*N points are taken in subject-major order as icon_query_points_batch takes them (d_points [B,N,3]
 * world points, d_calibs [B,12] device); d_stacks: HOST array of S device pointers to float32 [B,C,H,W] planes (the caller's own
 * tensors, not repacked), stack_shapes: HOST int32 [S][4] = B, C, H, W of every stack - all must agree.  has_vis / has_cmap /
 * has_norm: cfg.net.smpl_feats (icon; ignored for pifu).  mb: the subjects' mesh batch (icon) or NULL (pifu).
 * Forward outputs (device): d_rows float32 [S,B,Cin,N] = point_feat of every stack, channels [img | sdf | cmap | norm] (icon,
 * the subsets of icon_feat_set_smpl_feats; img = the half smpl_vis selects when has_vis, else all C) or [img | z] (pifu);
 * d_in_cube float32 [B,1,N], the strict test of :274-275; d_taps [B*N] records of 16 bytes (16-byte aligned) for the backward.
 * The search, the SMPL channels, the sdf clip and the batch-global outlier cmap list run once per call, not per stack: the
 * launches of icon_query_points_batch's geometry half plus three, whatever B, N and S.  The workspace grows as for any other
 * call; otherwise no allocation, no synchronisation.  ICON_ERR_UNSUPPORTED: the pamir prior, search 'brute', a tie rule on the
 * workspace, S > 8; ICON_ERR_ARG: stacks of differing shapes, B * N >= 2^31.
 * Backward: d_grad_rows [S,B,Cin,N] -> d_grad_planes [S,B,C,H,W], every element of every stack whose bit of stack_mask is set
 * written (the others are left alone): texel (s,b,c,y,x) = sum over the points whose four taps include it of weight *
 * grad_rows[s,b,c',p], c' = c - half * (C / n_select) for the points of that feature half; products in float32, the sum in
 * float64 in a fixed order (cells nw, ne, sw, se; ascending point index inside a cell, dealt to four lanes and combined by a
 * fixed tree), rounded once; taps outside the image contribute nothing.  No floating-point atomics: equal bytes from run to
 * run.  n_select: 2 when has_vis (icon), else 1.  d_scratch: icon_train_rows_bytes bytes, 256-byte aligned, the caller's;
 * launches only (key kernel, one radix sort, gather kernel), no allocation, no synchronisation. */
int icon_train_rows_bytes(int B, int64_t N, int S, int C, int H, int W, int64_t *bytes);
int icon_train_rows_forward(const icon_mesh_batch_t *mb, int prior_type, float sdf_clip, int cmap_mode, int has_vis,
                            int has_cmap, int has_norm, const float *const *d_stacks, const int32_t *stack_shapes, int S,
                            const float *d_calibs, const float *d_points, int64_t N, float *d_rows, float *d_in_cube,
                            void *d_taps, int search, icon_work_t *work, void *stream);
int icon_train_rows_backward(const float *d_grad_rows, const void *d_taps, int S, uint32_t stack_mask, int B, int Cin, int C,
                             int H, int W, int n_select, int64_t N, float *d_grad_planes, void *d_scratch,
                             int64_t scratch_bytes, void *stream);

/* ---- training, pamir prior: rows [img | vol] of every stack, and their gradient into the volumes ----------
 * HGPIFuNet.query in training mode (lib/net/HGPIFuNet.py:348-359): point_feat = cat(index(im_feat, xy), index(vol_feat, xyz)) per
 * pair of (feature stack, volume of that stack).  d_stacks / stack_shapes as above; d_vols: HOST array of S device pointers to
 * float32 [B,Cv,D,H,W] volumes (VolumeEncoder's outputs, read in place, channel first), vol_shapes: HOST int32 [S][5] - all must
 * agree, and hold the planes' B.  d_rows float32 [S,B,C+Cv,N]: channels 0 .. C-1 the bilinear tap of the planes, C .. C+Cv-1 the
 * trilinear tap of the volume: grid_sample's statement in float32 (x -> W, y -> H, z -> D; corners z0 before z1, inside a z y0x0,
 * y0x1, y1x0, y1x1; weight (x-term * y-term) * z-term; the eight products added left to right; zeros padding, align_corners).
 * d_in_cube, d_taps as above (the record's fourth word carries the projected z).  Two launches, no workspace, no allocation, no
 * synchronisation.  The gradient into the PLANES is icon_train_rows_backward with Cin = C + Cv, n_select = 1.
 * icon_train_vol_backward: d_grad_rows [S,B,Cin,N] -> d_grad_vols [S,B,Cv,D,H,W], every element of every stack whose bit of
 * stack_mask is set written (+0 where no tap reaches): voxel (s,b,c,z,y,x) = sum over the points of subject b that have it among
 * their eight taps of weight * grad_rows[s,b,C+c,p]; weight and product in float32 (the forward's statement), the sum in float64
 * in a fixed order - the eight source cells in corner order, ascending point index inside a cell, dealt to four lanes (term j of
 * a cell to lane j mod 4, each lane running through all eight cells) and combined as (l0 + l1) + (l2 + l3) - rounded once.  No
 * floating-point atomics: equal bytes from run to run.  d_scratch: icon_train_vol_bytes bytes, 256-byte aligned, the caller's;
 * launches only (key kernel, one radix sort, cell-start table, gather kernel).  ICON_ERR_UNSUPPORTED: S > 8, B (D+1) (H+1) (W+1)
 * >= 2^32 - 1; ICON_ERR_ARG: null pointers, differing shapes, another B in the volumes than in the planes, B * N >= 2^31. */
int icon_train_pamir_forward(const float *const *d_stacks, const int32_t *stack_shapes, const float *const *d_vols,
                             const int32_t *vol_shapes, int S, const float *d_calibs, const float *d_points, int64_t N,
                             float *d_rows, float *d_in_cube, void *d_taps, void *stream);
int icon_train_vol_bytes(int B, int64_t N, int S, int Cv, int D, int H, int W, int64_t *bytes);
int icon_train_vol_backward(const float *d_grad_rows, const void *d_taps, int S, uint32_t stack_mask, int B, int Cin, int C,
                            int Cv, int D, int H, int W, int64_t N, float *d_grad_vols, void *d_scratch,
                            int64_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ICON_AMD_H */
