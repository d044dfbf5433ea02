/*
 * f3dg.h -- C ABI of libf3dg_hip.so: the MI355X (gfx950) implementation of F3D-Gaus's GOF rasterization +
 * cycle-aggregative projection hot path.
 *
 * Plain pointers and sizes only (no torch / no C++ types). Every pointer is a DEVICE pointer unless the
 * parameter name starts with `h_`. Nothing in this library synchronises the host with the device except
 * the functions documented as blocking. `stream` is a hipStream_t passed as void* (NULL = default stream).
 *
 * What each entry point replaces in the reference (paths relative to /root/reference; RAST =
 * src/gaussian-splatting/submodules/diff-gof-rasterization):
 *
 *   f3dg_forward / f3dg_forward_batched
 *       CudaRasterizer::Rasterizer::forward      RAST/cuda_rasterizer/rasterizer.h:31-55,
 *                                                RAST/cuda_rasterizer/rasterizer_impl.cu:247-405
 *       reached from pybind `rasterize_gaussians` RAST/ext.cpp:16, RAST/rasterize_points.cu:36-122
 *   f3dg_backward
 *       CudaRasterizer::Rasterizer::backward     RAST/cuda_rasterizer/rasterizer.h:57-90,
 *                                                RAST/cuda_rasterizer/rasterizer_impl.cu:409-526
 *       reached from pybind `rasterize_gaussians_backward` RAST/ext.cpp:18, RAST/rasterize_points.cu:124-211
 *   f3dg_backward_sets
 *       the same for the n_sets Gaussian sets x views_per_set views of one f3dg_forward_sets call (the reference runs
 *       n_sets * views_per_set separate backward calls)
 *   f3dg_mark_visible
 *       CudaRasterizer::Rasterizer::markVisible  RAST/cuda_rasterizer/rasterizer.h:23-29,
 *                                                RAST/cuda_rasterizer/rasterizer_impl.cu:172-186 (pybind `mark_visible`)
 *   f3dg_workspace_bytes / f3dg_read_status
 *       the std::function<char*(size_t)> resize callbacks + the blocking 4-byte D2H of num_rendered
 *       RAST/rasterize_points.cu:28-34, RAST/cuda_rasterizer/rasterizer_impl.cu:277-279,290-292,336-340
 *   f3dg_splat_head
 *       the post-network half of GaussianSplatPredictor_gtunet.forward   src/gaussian_predictor.py:857-881, 961-1007
 *       (python-only in the reference; there is no native FFI for it -- this is the build's fused kernel)
 *   f3dg_splat_head_backward
 *       what torch.autograd derives from those same lines                src/gaussian_predictor.py:857-881, 961-1002
 *   f3dg_render_epilogue
 *       the torch post-processing of render_predicted_more_v2_gof  src/gaussian_renderer/__init__.py:881-909, 1043-1053
 *   f3dg_render_epilogue_backward
 *       what torch.autograd derives from those same lines (they are plain torch ops on the raster in the reference)
 *   f3dg_cycle_inputs_backward
 *       what torch.autograd derives from the hand-off of the cycle aggregation   visualize.py:311, 331-333
 *   f3dg_marching_tets_count / f3dg_marching_tets_emit
 *       the integer topology of _unbatched_marching_tetrahedra     src/utils_tetmesh.py:47-138 (torch.unique + mask indexing there)
 *   f3dg_ssim_forward / f3dg_ssim_backward
 *       ssim / _ssim, l1_loss, l2_loss and what torch.autograd derives from them   src/gaussian-splatting/utils/loss_utils.py:17-63
 *       (the objective of src/gaussian-splatting/train.py:92) and psnr's mean squared error, utils/image_utils.py:17-19
 *   f3dg_geometry_loss_forward / f3dg_geometry_loss_backward
 *       the terms the settings file weighs besides RGB   config/imagenetgs_256x256_v1.yaml:50-66 (the reference ships the weights, not
 *       the trainer: the terms are defined below, on the maps of src/gaussian_renderer/__init__.py:881-909, 1043-1053)
 *   f3dg_forward_warp / f3dg_masked_l1_forward / f3dg_masked_l1_backward
 *       the depth-based forward warp behind the settings' w_warping / w_prop (threshold, erode_kernel_size, erode_pad_size:
 *       config/imagenetgs_256x256_v1.yaml:50-66) and the masked L1 against it. The reference ships the settings, no trainer and no
 *       warp: the semantics are this build's, defined below
 *   f3dg_tsdf_integrate / f3dg_tsdf_cells_count / f3dg_tsdf_cells_emit / f3dg_tsdf_vertices
 *       the TSDF mesh route (depth maps fused into a volume, its surface cells as tetrahedra for f3dg_marching_tets_*): the reference
 *       meshes through an external Delaunay tetrahedralisation (visualize.py:440-548) and holds no TSDF code: the semantics are this
 *       build's, defined below
 *   f3dg_contribution / f3dg_gaussian_compact_count / f3dg_gaussian_compact_emit
 *       per-Gaussian contribution statistics of rendered views and the pruning of a set by them: not in the reference, the
 *       semantics are this build's, defined below
 *   f3dg_mesh_components / f3dg_mesh_compact_count / f3dg_mesh_compact_emit
 *       what follows either mesh route: connected components of the triangles and the removal of the small ones. The reference's
 *       script leaves that to trimesh on the host (update_vertices / update_faces, visualize.py:545-546) and labels no components:
 *       the semantics are this build's, defined below
 *   f3dg_mesh_adjacency / f3dg_mesh_smooth / f3dg_mesh_vertex_normals
 *       vertex adjacency of a triangle mesh, Taubin smoothing and area-weighted vertex normals: not in the reference (its script
 *       exports what trimesh makes of the raw mesh): the semantics are this build's, defined below
 *   f3dg_mesh_simplify_count / f3dg_mesh_simplify_emit
 *       mesh reduction by uniform-grid vertex clustering with root, mean or quadric placement (grid welding at a small cell): not in
 *       the reference: the semantics are this build's, defined below
 *   f3dg_mesh_raster
 *       an exact z-buffered triangle rasteriser over the renderer's cameras (face id, depth, barycentric weights, interpolated vertex
 *       attributes per pixel): not in the reference (the texturing branch of visualize.py:520-537 is dead code and the mesh is never
 *       drawn): the semantics are this build's, defined below
 *   f3dg_mesh_bake_colors / f3dg_mesh_bake_workspace_bytes
 *       the views' colour put back on the mesh's vertices, each (view, vertex) sample tested against f3dg_mesh_raster's own z-buffer:
 *       what the dead texturing branch of visualize.py:520-537 never did; the semantics are this build's, defined below
 *
 * Memory ownership mirrors the reference: outputs and the workspace are allocated and owned by the caller
 * (torch tensors on the Python side). Instead of growing buffers through callbacks in the middle of the call
 * (which forces the reference's host sync, rasterizer_impl.cu:336), the caller passes ONE workspace sized by
 * f3dg_workspace_bytes() for a chosen instance capacity `max_rendered`; if the (Gaussian, tile) instance count
 * of a call exceeds that capacity the device sets an overflow flag, the compositing stage is skipped, and
 * f3dg_read_status()/f3dg_forward() report F3DG_ERR_OVERFLOW together with the capacity that would have
 * sufficed, so the caller can grow the workspace and retry -- the same contract as the resize callback, moved
 * outside the launch sequence. The workspace layout is the forward<->backward contract (as the three byte
 * buffers are in the reference, rasterizer_impl.cu:444-446) and is private to the library.
 */
#ifndef F3DG_H_INCLUDED
#define F3DG_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F3DG_OK              0
#define F3DG_ERR_BAD_ARG    -1   /* NULL where data is required, non-positive sizes, both/neither of sh & colours ... */
#define F3DG_ERR_WORKSPACE  -2   /* workspace_bytes smaller than f3dg_workspace_bytes(...) */
#define F3DG_ERR_OVERFLOW   -3   /* more (Gaussian, tile) instances than max_rendered; see f3dg_read_status */
#define F3DG_ERR_HIP        -4   /* a HIP runtime call failed; f3dg_last_error() has the text */
#define F3DG_ERR_UNSUPPORTED -5  /* NUM_CHANNELS != 3 etc. (rasterizer_impl.cu:294-297) */
#define F3DG_ERR_STATE      -6   /* f3dg_backward on a workspace whose last forward was not a F3DG_FLAG_SAVE_AUX call: nothing was
                                    walked, every gradient is zero (reported by f3dg_backward_pairs / f3dg_read_status) */

/* flags for f3dg_forward_batched */
#define F3DG_FLAG_SAVE_AUX   1u  /* keep final_T / n_contrib / conic / clamped for f3dg_backward (training mode).
                                    Without it the compositing kernel writes only the 9 output channels. */
#define F3DG_FLAG_BG_PER_VIEW 2u /* background is [n_views,3] instead of [3] */
/* Output-channel mask of inference calls (not part of the reference's API: visualize.py:304-306, 400-402 consume only `render`,
 * `rendered_depth` and `rendered_alpha`, and the build's own batched loops -- cycle aggregation, orbit frames -- ask for just those).
 * With BOTH flags the compositing kernel neither accumulates nor writes the view-space normal (channels 3..5) and the distortion
 * (channel 8): those planes of out_color are left untouched, every other channel is bit-identical to the 9-channel call. Ignored
 * with F3DG_FLAG_SAVE_AUX and by the kernels of one- or two-view launches (which then write all nine). */
#define F3DG_FLAG_SKIP_NORMAL 4u
#define F3DG_FLAG_SKIP_DISTORTION 8u
/* Per-call selection of what f3dg_set_option sets as process-wide DEFAULTS (round 5). The reference hands every knob of a call through
 * GaussianRasterizationSettings_GOF (RAST/diff_gof_rasterization/__init__.py:168-182); these bits do the same for the knobs this build
 * adds, so that two streams / threads can render with different settings at the same time:
 *   F3DG_FLAG_EXACT          the compositing of this call runs the reference's float32 / float64 operation order, whatever "render_fast" says
 *                            (a consumer of the distortion channel -- 3-17 % relative off in fast arithmetic -- asks for it per call);
 *   F3DG_FLAG_FAST           ... runs the fast arithmetic, also with F3DG_FLAG_SAVE_AUX (the backward repeats the forward's alpha from the
 *                            workspace header, so the pair stays consistent); EXACT wins when both are given;
 *   F3DG_FLAG_NO_TILE_CULL   the reference's tile lists (every tile of the 3-sigma square, forward.cu:364-374) instead of the culled ones;
 *   F3DG_FLAG_NO_SMALL_PATH  the general launch sequence also for the shapes the three-launch small-call path serves;
 *   F3DG_FLAG_SCAN           (inference calls in the fast arithmetic, general launch sequence) the split-pixel compositing schedule of
 *                            csrc/f3dg_render5.hip: the entries of the pixels that hold a quadrant back are blended by helper lanes and
 *                            combined by a segmented wave scan. The set of blended entries per pixel is unchanged, the sums are associated
 *                            differently: every channel within the 1e-4 of the fast arithmetic against the reference, NOT bit-identical
 *                            to a call without the flag. Ignored with F3DG_FLAG_EXACT / F3DG_FLAG_SAVE_AUX (option "render_scan" sets the
 *                            process default: -1 flag only, 1 every eligible call, 0 never). */
#define F3DG_FLAG_EXACT 16u
#define F3DG_FLAG_FAST 32u
#define F3DG_FLAG_NO_TILE_CULL 64u
#define F3DG_FLAG_NO_SMALL_PATH 128u
#define F3DG_FLAG_SCAN 256u
/* f3dg_forward_sets with n_sets > 1 keeps the auxiliary planes only with F3DG_FLAG_SAVE_AUX | F3DG_FLAG_SETS_AUX: the caller's promise that
 * f3dg_backward_sets (not f3dg_backward, which indexes the Gaussian inputs of one set) follows on that workspace. Without F3DG_FLAG_SAVE_AUX
 * the flag is F3DG_ERR_BAD_ARG; with n_sets == 1 it changes nothing. */
#define F3DG_FLAG_SETS_AUX 512u

#define F3DG_TILE 16             /* BLOCK_X = BLOCK_Y = 16, RAST/cuda_rasterizer/config.h:16-17 */
#define F3DG_OUT_CHANNELS 9      /* RGB, normal xyz, median depth, alpha, distortion: auxiliary.h:21-24 */
#define F3DG_DEPTH_OFFSET 6      /* auxiliary.h:21 */
#define F3DG_ALPHA_OFFSET 7      /* auxiliary.h:22 */
#define F3DG_DISTORTION_OFFSET 8 /* auxiliary.h:23 */

/* Library / build identification: "f3dg-hip gfx950 <version>" */
const char* f3dg_version(void);
/* Text of the last HIP error seen by this thread's calls (empty string if none). */
const char* f3dg_last_error(void);

/* Bytes of workspace needed for n_views views of P Gaussians at W x H with room for max_rendered
 * (Gaussian, tile) instances summed over all views of the call. Pure host arithmetic. */
size_t f3dg_workspace_bytes(int P, int W, int H, int n_views, long long max_rendered);

/* Batched forward: renders n_views views of the SAME P Gaussians in one launch sequence, no host sync.
 *   viewmatrix, projmatrix : [n_views,16]  (row-vector convention, i.e. already transposed; auxiliary.h:86-115)
 *   cam_pos                : [n_views,3]
 *   background             : [3] or [n_views,3] with F3DG_FLAG_BG_PER_VIEW
 *   shs [P,M,3] xor colors_precomp [P,3]; (scales [P,3] and rotations [P,4]) xor cov3D_precomp [P,6];
 *   view2gaussian_precomp  : NULL or [n_views,P,10]
 *   out_color              : [n_views,9,H,W]   radii: [n_views,P] int32 or NULL
 * Returns F3DG_OK or a negative error for host-detectable problems. Instance overflow is reported by
 * f3dg_read_status(). P == 0 is legal: outputs are filled with background / zeros (rasterize_points.cu:85). */
int f3dg_forward_batched(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                         int n_views, int P, int D, int M,
                         const float* background, int W, int H,
                         const float* means3D, const float* shs, const float* colors_precomp,
                         const float* opacities, const float* scales, float scale_modifier,
                         const float* rotations, const float* cov3D_precomp,
                         const float* view2gaussian_precomp,
                         const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                         float tan_fovx, float tan_fovy, float kernel_size,
                         float* out_color, int* radii, unsigned flags);

/* The same for n_sets DIFFERENT Gaussian sets of equal size in one launch sequence -- the image-batched form of the cycle
 * aggregation loop (reference visualize.py:293-314 renders 8 views of each of B images with B x 8 separate rasterizer calls):
 * means3D ... rotations are [n_sets, P, ...], the cameras [n_sets * views_per_set, ...] (set-major), out_color
 * [n_sets * views_per_set, 9, H, W], radii [n_sets * views_per_set, P]; view i renders set i / views_per_set.
 * f3dg_forward_batched is the n_sets = 1 case. Workspace: f3dg_workspace_bytes(P, W, H, n_sets * views_per_set, max_rendered).
 * n_sets > 1 with view2gaussian_precomp, or with F3DG_FLAG_SAVE_AUX alone, returns F3DG_ERR_BAD_ARG (f3dg_backward indexes the
 * Gaussian inputs of ONE set); F3DG_FLAG_SAVE_AUX | F3DG_FLAG_SETS_AUX keeps the auxiliary planes for f3dg_backward_sets. Calls of
 * several sets always take the general launch sequence. */
int f3dg_forward_sets(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                      int n_sets, int views_per_set, int P, int D, int M,
                      const float* background, int W, int H,
                      const float* means3D, const float* shs, const float* colors_precomp,
                      const float* opacities, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp,
                      const float* view2gaussian_precomp,
                      const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                      float tan_fovx, float tan_fovy, float kernel_size,
                      float* out_color, int* radii, unsigned flags);

/* BLOCKING. Waits for `stream`, then reads the workspace header written by the last forward on it.
 * h_num_rendered: total instances the call needed; returns F3DG_OK, or F3DG_ERR_OVERFLOW if that exceeded
 * the capacity the workspace was sized for (outputs of that call are then undefined). */
int f3dg_read_status(void* stream, const void* workspace, long long* h_num_rendered);

/* The same status WITHOUT blocking the caller -- what is left of the reference's blocking copy (rasterizer_impl.cu:336) once a loop
 * renders one view per call and never looks at num_rendered (visualize.py:293-314, 387-416).
 * f3dg_status_post: enqueues on `stream`, behind the forward just issued on it, a copy of the workspace header into pinned host
 *   memory owned by the library, and an event. Returns a ticket >= 0 (or a negative error). The workspace may be reused by the next
 *   call on the same stream at once: the copy is ordered before it.
 * f3dg_status_poll: F3DG_PENDING while the copy has not landed (wait == 0); otherwise -- after waiting for it if wait != 0 --
 *   F3DG_OK / F3DG_ERR_OVERFLOW as f3dg_read_status, *h_num_rendered as there, and the ticket is released. A caller that defers the
 *   check this way must be able to re-issue the call it belongs to (outputs of an overflowed call are undefined). */
#define F3DG_PENDING 1
int f3dg_status_post(void* stream, const void* workspace);
int f3dg_status_poll(int ticket, int wait, long long* h_num_rendered);

/* Reference-shaped single-view forward (Rasterizer::forward): f3dg_forward_batched(n_views = 1) followed by
 * f3dg_read_status(). BLOCKING, like the reference (rasterizer_impl.cu:336). Returns num_rendered >= 0 or a
 * negative error; on F3DG_ERR_OVERFLOW *h_needed (if not NULL) receives the required capacity. */
long long f3dg_forward(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                       int P, int D, int M, const float* background, int W, int H,
                       const float* means3D, const float* shs, const float* colors_precomp,
                       const float* opacities, const float* scales, float scale_modifier,
                       const float* rotations, const float* cov3D_precomp, const float* view2gaussian_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                       float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
                       float* out_color, int* radii, unsigned flags, long long* h_needed);

/* Backward of a forward made with F3DG_FLAG_SAVE_AUX on the same workspace (same P, W, H, n_views,
 * max_rendered). Argument meaning follows Rasterizer::backward (rasterizer.h:57-90). The reference's binding zero-fills every
 * dL_* tensor (rasterize_points.cu:160-170); here the PER-GAUSSIAN sums (dL_dopacity, dL_dmean3D, dL_dsh, dL_dscale, dL_drot) are
 * added into and must be zero-filled (or hold running sums) by the caller, the PER-VIEW outputs (dL_dmean2D, dL_dcolor,
 * dL_dview2gaussian: 64 floats per (view, Gaussian), 2 GB at BASELINE C5) are written in full by the call and may be handed over
 * uninitialised; dL_dconic and dL_dcov3D are never touched (the reference leaves them zero). Sizes per view v:
 *   dL_dpix [n_views,9,H,W] in;  dL_dmean2D [n_views,P,3], dL_dconic [n_views,P,4] (stays 0), dL_dopacity [P],
 *   dL_dcolor [n_views,P,3], dL_dmean3D [P,3], dL_dcov3D [P,6] (stays 0), dL_dsh [P,M,3], dL_dscale [P,3],
 *   dL_drot [P,4], dL_dview2gaussian [n_views,P,10].
 * Per-Gaussian parameter gradients (opacity, mean3D, sh, scale, rot) are summed over the views of the call. */
int f3dg_backward(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                  int n_views, int P, int D, int M, const float* background, int W, int H,
                  const float* means3D, const float* shs, const float* colors_precomp,
                  const float* scales, float scale_modifier, const float* rotations,
                  const float* cov3D_precomp, const float* view2gaussian_precomp,
                  const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                  float tan_fovx, float tan_fovy, float kernel_size,
                  const int* radii, const float* dL_dpix,
                  float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                  float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                  float* dL_dview2gaussian, unsigned flags /* F3DG_FLAG_BG_PER_VIEW as in the forward */);

/* The same for a f3dg_forward_sets call made with F3DG_FLAG_SAVE_AUX | F3DG_FLAG_SETS_AUX (same n_sets, views_per_set, P, W, H, max_rendered):
 * ONE compositing backward over all n_sets * views_per_set views and ONE per-Gaussian stage. means3D, shs, scales, rotations are
 * [n_sets, P, ...]; the cameras, radii and dL_dpix are set-major [n_sets * views_per_set, ...]; the per-view outputs (dL_dmean2D,
 * dL_dcolor, dL_dview2gaussian) are [n_sets * views_per_set, P, ...] and written in full; the per-Gaussian sums (dL_dopacity,
 * dL_dmean3D, dL_dsh, dL_dscale, dL_drot) are [n_sets, P, ...], added into as in f3dg_backward, each summed over the views of its OWN
 * set only, by one writer per Gaussian in a fixed view order. view2gaussian_precomp with n_sets > 1 is F3DG_ERR_BAD_ARG.
 * f3dg_backward is the n_sets = 1 case of the same code. */
int f3dg_backward_sets(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                       int n_sets, int views_per_set, int P, int D, int M, const float* background, int W, int H,
                       const float* means3D, const float* shs, const float* colors_precomp,
                       const float* scales, float scale_modifier, const float* rotations,
                       const float* cov3D_precomp, const float* view2gaussian_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                       float tan_fovx, float tan_fovy, float kernel_size,
                       const int* radii, const float* dL_dpix,
                       float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                       float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                       float* dL_dview2gaussian, unsigned flags /* F3DG_FLAG_BG_PER_VIEW as in the forward */);

/* Gaussians -> points integration: Rasterizer::integrate (rasterizer.h:92-123, rasterizer_impl.cu:530-792) as bound by
 * IntegrateGaussiansToPointsCUDA (rasterize_points.cu:233-343, `_C.integrate_gaussians_to_points`). One view.
 *   points3D [PN,3]; the Gaussian arguments as in f3dg_forward; subpixel_offset [H,W,2] is accepted and ignored (the
 *   reference only loads it into an unused variable, forward.cu:838).
 *   out_color [9,H,W]: 0..2 colour + T * background of the centre ray, 3..5 zero, 6 maximal ray depth, 7 alpha,
 *       8 the number of points that fell into the pixel (forward.cu:984-996, 1194-1196)
 *   out_alpha_integrated [PN] (1 for points outside the frustum / image), out_color_integrated [PN,3] (0 for those)
 * The library writes every output element itself (the reference relies on the caller's torch.full fills). P == 0 or
 * PN == 0: out_color = 0, alpha = 1, colour = 0, returns 0 (rasterize_points.cu:300).
 * BLOCKING like f3dg_forward; returns num_rendered >= 0 or a negative error; on F3DG_ERR_OVERFLOW *h_needed (if not
 * NULL) receives the required instance capacity. The workspace must hold f3dg_integrate_workspace_bytes(). */
size_t f3dg_integrate_workspace_bytes(int P, int PN, int W, int H, long long max_rendered);
long long f3dg_integrate(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                         int PN, int P, int D, int M, const float* background, int W, int H,
                         const float* points3D, const float* means3D, const float* shs, const float* colors_precomp,
                         const float* opacities, const float* scales, float scale_modifier,
                         const float* rotations, const float* cov3D_precomp, const float* view2gaussian_precomp,
                         const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                         float tan_fovx, float tan_fovy, float kernel_size, const float* subpixel_offset,
                         int prefiltered, float* out_color, int* radii, float* out_alpha_integrated,
                         float* out_color_integrated, long long* h_needed);

/* The two halves of f3dg_integrate, for callers that integrate MANY point sets against the same Gaussians and camera
 * (the mesh-extraction sweep of visualize.py:449-505 runs 9 point sets through each of 129 cameras): everything that does
 * not depend on the points -- projection, binning and the five-ray per-pixel pass with its contributor table -- is done
 * once by f3dg_integrate_prepare and stays in the workspace (sized with PN_max = the largest point set that will follow);
 * f3dg_integrate_points then costs one lane per point. out_color is written by prepare (channels 0..7) and read by
 * points (which also writes channel 8). out_alpha_integrated / out_color_integrated may be NULL; alpha_min, if not NULL,
 * is updated as alpha_min[i] = min(alpha_min[i], alpha_integrated[i]) (torch.min semantics, visualize.py:463: NaN propagates) for
 * EVERY point -- alpha_integrated is 1 for a point outside the frustum / image, so a value above 1 comes down to 1 there. */
long long f3dg_integrate_prepare(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                                 int PN_max, int P, int D, int M, const float* background, int W, int H,
                                 const float* means3D, const float* shs, const float* colors_precomp,
                                 const float* opacities, const float* scales, float scale_modifier,
                                 const float* rotations, const float* cov3D_precomp, const float* view2gaussian_precomp,
                                 const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                 float tan_fovx, float tan_fovy, float kernel_size, float* out_color, int* radii,
                                 long long* h_needed);
int f3dg_integrate_points(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                          int PN, int P, int W, int H, const float* points3D, const float* viewmatrix,
                          float tan_fovx, float tan_fovy, float* out_color, float* out_alpha_integrated,
                          float* out_color_integrated, float* alpha_min);

/* The mesh extraction integrates its point sets through 129 cameras of the SAME Gaussians (visualize.py:449-505): n_views cameras
 * prepared in ONE launch sequence (projection, binning and the per-pixel pass with grid = n_views x tiles: a single 256^2 camera is
 * 256 workgroups, one wave per SIMD of an MI355X). viewmatrix / projmatrix [n_views,16], cam_pos [n_views,3], out_color
 * [n_views,9,H,W], radii [n_views,P] or NULL; max_rendered is the capacity for the instances of all cameras together.
 * Workspace: f3dg_integrate_workspace_bytes_batched. Every per-camera result is bit-identical to f3dg_integrate_prepare of that
 * camera. Returns the total instance count or a negative error (BLOCKING, as f3dg_integrate_prepare). */
size_t f3dg_integrate_workspace_bytes_batched(int P, int PN, int W, int H, int n_views, long long max_rendered);
long long f3dg_integrate_prepare_batched(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                                         int n_views, int PN_max, int P, int D, int M, const float* background, int W, int H,
                                         const float* means3D, const float* shs, const float* colors_precomp,
                                         const float* opacities, const float* scales, float scale_modifier,
                                         const float* rotations, const float* cov3D_precomp,
                                         const float* view2gaussian_precomp, const float* viewmatrix,
                                         const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                         float kernel_size, float* out_color, int* radii, long long* h_needed);
/* One point set against camera `view` of a batched preparation (viewmatrix [16] and out_color [9,H,W] of THAT camera). */
int f3dg_integrate_points_view(void* stream, void* workspace, size_t workspace_bytes, long long max_rendered,
                               int n_views, int view, int PN, int P, int W, int H, const float* points3D,
                               const float* viewmatrix, float tan_fovx, float tan_fovy, float* out_color,
                               float* out_alpha_integrated, float* out_color_integrated, float* alpha_min);

/* Diagnostic, BLOCKING: how many (camera, tile) pairs of the last preparation on this workspace reached the reference's limit of 1,024
 * contributors in some pixel (forward.cu:972-976) and were therefore computed again, one pixel per lane, by the plain transcription
 * (f3dg_integrate.hip: integrate_pass1_kernel, launched behind integrate_pass1_rays_kernel on the flagged tiles only). Same shape
 * arguments as the preparation. */
int f3dg_debug_integrate_redo(void* stream, const void* workspace, int P, int PN_max, int W, int H, int n_views, long long max_rendered,
                              int* h_tiles);

/* Inspection: what the per-pixel pass of the last preparation on this workspace left for camera `view`, copied to device buffers of the
 * caller (any pointer may be NULL): contrib_n [H*W] (contributors per pixel), contrib_ids [H*W*1024] (their 1-based positions in the
 * tile's list as the 16-bit values the reference stores, forward.cu:969; only the first contrib_n of a pixel's 1,024 are defined),
 * last_contributor [H*W] (the full position of the last one) and final_T [H*W] (transmittance of the centre ray). Same shape arguments
 * as the preparation; asynchronous on `stream`. Records, list and ranges of the workspace come from f3dg_debug_export. */
int f3dg_debug_integrate_export(void* stream, const void* workspace, int P, int PN_max, int W, int H, int n_views, long long max_rendered,
                                int view, unsigned* contrib_n, unsigned short* contrib_ids, unsigned* last_contributor, float* final_T);

/* present[i] = (view-space z of means3D[i] > 0.2), auxiliary.h:177-202. present is uint8 [P]. */
int f3dg_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix,
                      const float* projmatrix, uint8_t* present);

/* Marching tetrahedra, the integer topology of _unbatched_marching_tetrahedra (src/utils_tetmesh.py:47-138) in two calls on one
 * caller-owned workspace (the output sizes depend on the data; the caller allocates them between the calls):
 *   sdf [N] float32; tets [F,4] point ids, int64 (tets_int32 == 0) or int32 (!= 0). A point is occupied when sdf > 0 (NaN and 0 are
 *   outside); a tetrahedron is on the surface when 1..3 of its corners are; its case index is sum occ_i 2^i over its corners as given.
 *   interp_v [E,2] int64: the unique edges with exactly one occupied end as (lo, hi), lo < hi, in ascending lexicographic order.
 *   faces [n_one + 2 n_two, 3] int64: rows of interp_v; first the triangle of every one-triangle surface tetrahedron in tetrahedron
 *   order, then the two triangles of every two-triangle one in tetrahedron order (triangle_table, utils_tetmesh.py:23-43). A duplicate
 *   tetrahedron gives duplicate faces. All of F is worked in one piece: above 32 Mi tetrahedra the reference recurses over chunks and
 *   returns another permutation of the same faces.
 * max_edges: capacity for the crossing edges of all surface tetrahedra, duplicates included (3 or 4 per surface tetrahedron; 4 F always
 *   suffices and is the largest value accepted).
 * f3dg_marching_tets_count: BLOCKING, two host reads (the counts after the classification, then E; one if nothing crosses, none if
 *   F == 0). h_counts[0..3] = E, n_one, n_two, crossing edges counted. F3DG_ERR_OVERFLOW: more crossing edges than max_edges;
 *   h_counts[3] is the capacity to retry with. F3DG_ERR_BAD_ARG: NULL pointers, N <= 0, F < 0, N or F >= 2^31, or a tetrahedron with an
 *   id outside [0, N) -- every id is range-checked on the device before anything is indexed with it. F3DG_ERR_UNSUPPORTED: 2^31 or more
 *   crossing edges. F == 0 is legal (all counts 0, tets may be NULL).
 * f3dg_marching_tets_emit: after a f3dg_marching_tets_count that returned F3DG_OK with E > 0, same workspace, sizes and tets; n_one is
 *   h_counts[1]. Writes every element of interp_v [E,2] and faces [n_one + 2 n_two, 3]. No host read. Bit-reproducible. */
size_t f3dg_marching_tets_workspace_bytes(long long N, long long F, long long max_edges);
int f3dg_marching_tets_count(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, long long max_edges,
                             const float* sdf, const void* tets, int tets_int32, long long* h_counts);
int f3dg_marching_tets_emit(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, long long max_edges,
                            const void* tets, int tets_int32, long long n_one, long long* interp_v, long long* faces);

/* Cycle-aggregative projection ("splat head", src/gaussian_predictor.py:857-881, 961-1007) for B images:
 *   net_out [B,23,H,W] planar: offset 0:3, opacity 3, scaling 4:7, rotation 7:11, features_dc 11:14, features_rest 14:23
 *   depth [B,1,H,W], ray_dirs [3,H,W] (predictor buffer), view_to_world [B,16] (row-vector convention), cam_quat [B,4]
 * Outputs are written for image b at Gaussian offset `n_offset` of destination tensors whose per-image length is
 * `n_total` (>= n_offset + H*W): this is what lets the cycle loop aggregate the 9 passes in place instead of the
 * reference's torch.cat chain (visualize.py:336-340):
 *   xyz [B,n_total,3], opacity [B,n_total,1], scaling [B,n_total,3], rotation [B,n_total,4],
 *   features_dc [B,n_total,1,3], features_rest [B,n_total,3,3], unet_depth [B,n_total,1]
 * squre_clip: clamp |x|,|y| only when < 10 (gaussian_predictor.py:972-974). */
int f3dg_splat_head(void* stream, int B, int H, int W, const float* net_out, const float* depth,
                    const float* ray_dirs, const float* view_to_world, const float* cam_quat, float squre_clip,
                    long long n_total, long long n_offset,
                    float* xyz, float* opacity, float* scaling, float* rotation,
                    float* features_dc, float* features_rest, float* unet_depth);

/* Backward of f3dg_splat_head with respect to net_out and depth: the vector-Jacobian product that torch.autograd derives from the
 * reference's differentiable lines (src/gaussian_predictor.py:857-881 back-projection, :961-970 bmm / perspective divide / clamp_,
 * :975-979 sigmoid / exp / F.normalize / flatten, :839-855 with :45-64 quaternion product, :821-837 transform_SHs, :991-994).
 * The first twelve arguments are those of f3dg_splat_head. Nothing is saved by the forward: the kernel recomputes its intermediates
 * from net_out / depth with the forward's own float32 expressions (one thread per (image, pixel), no atomics: bit-reproducible).
 *   g_xyz, g_opacity, g_scaling, g_rotation, g_features_dc, g_features_rest, g_unet_depth: upstream gradients in the layout of the
 *       forward's outputs, [B,n_total,...] with image b's rows at n_offset .. n_offset + H*W; rows outside that window are never
 *       read. Each may be NULL = "this output was not used": all of its entries count as zero.
 *   d_net_out [B,23,H,W]: every element is written (no accumulation, the caller need not zero it).
 *   d_depth   [B,1,H,W]:  every element is written; NULL skips it.
 * squre_clip < 10: x / y receive no gradient where the forward clamped them (clamp_ passes it where -c <= x <= c).
 * view_to_world, cam_quat and ray_dirs are data: no gradients are produced for them.
 * F3DG_ERR_BAD_ARG: a NULL required pointer (the five inputs, d_net_out), non-positive sizes, n_offset < 0 or n_total < n_offset + H*W. */
int f3dg_splat_head_backward(void* stream, int B, int H, int W, const float* net_out, const float* depth,
                             const float* ray_dirs, const float* view_to_world, const float* cam_quat, float squre_clip,
                             long long n_total, long long n_offset,
                             const float* g_xyz, const float* g_opacity, const float* g_scaling, const float* g_rotation,
                             const float* g_features_dc, const float* g_features_rest, const float* g_unet_depth,
                             float* d_net_out, float* d_depth);

/* Fused epilogue of render_predicted_more_v2_gof (gaussian_renderer/__init__.py:881-909, 1043-1053) for n_views
 * rendered frames raster [n_views,9,H,W]:
 *   normal_world [n_views,3,H,W] = c2w[:3,:3] @ normalize(raster[3:6]);  c2w = inverse(world_view^T), given as
 *       c2w_rot [n_views,9] row-major 3x3 (host-computed, it is a 4x4 inverse)
 *   depth_normal [n_views,3,H,W]: central-difference normal of the back-projected median depth, border = 0;
 *       needs c2w [n_views,16] row-major 4x4 and fx, fy.
 * Either output pointer may be NULL to skip it. */
int f3dg_render_epilogue(void* stream, int n_views, int H, int W, const float* raster,
                         const float* c2w, float fx, float fy,
                         float* normal_world, float* depth_normal);
/* The same from the world_view matrices themselves ([n_views,16], row-vector convention, as render_predicted_more_v2_gof receives
 * them): every workgroup inverts world_view^T in float64 (cofactors), so the caller needs no matrix inverse per call. */
int f3dg_render_epilogue_view(void* stream, int n_views, int H, int W, const float* raster,
                              const float* world_view, float fx, float fy,
                              float* normal_world, float* depth_normal);
/* Vector-Jacobian product of f3dg_render_epilogue_view with respect to raster: the cotangents dL_dnormal_world and dL_ddepth_normal
 * ([n_views,3,H,W]; either may be NULL = all zero) are ADDED into channels 3..5 and 6 of dL_dpix [n_views,9,H,W]; no other channel
 * is touched. One thread per (view, pixel); the depth channel is a gather over the up to four interior axial neighbours whose
 * depth normal reads this pixel, summed in a fixed order: no atomics, bit-reproducible. F.normalize's backward, with g / 1e-12
 * where its clamp is active. */
int f3dg_render_epilogue_backward(void* stream, int n_views, int H, int W, const float* raster,
                                  const float* world_view, float fx, float fy,
                                  const float* dL_dnormal_world, const float* dL_ddepth_normal, float* dL_dpix);

/* 8-bit RGB frames for the video writer and the multi-GPU gather: dst [n_frames,H,W,3] uint8 =
 * (uint8)(255 * clamp(src[:, 0:3], 0, 1)) with src [n_frames,src_channels,H,W] float32 planar (src_channels = 9 for the
 * rasterizer output), i.e. what visualize.py:407,416 computes on the host per frame. */
int f3dg_pack_frames(void* stream, int n_frames, int H, int W, int src_channels, const float* src, unsigned char* dst);
/* The same frames written directly into PINNED HOST memory (hipHostMalloc / torch pin_memory; 16-byte aligned; anything else is
 * F3DG_ERR_BAD_ARG): the frames of visualize.py:407,416 arrive in host memory with one kernel and no copy command. HIP executes a
 * device -> pinned-host hipMemcpyAsync as a whole-chip shader copy, which competes with whatever renders next; this kernel uses at most
 * max_workgroups workgroups (0: 64) -- the transfer is PCIe-bound either way. Visible to the host after the stream (or an event
 * recorded behind the call) is synchronised. */
int f3dg_pack_frames_host(void* stream, int n_frames, int H, int W, int src_channels, const float* src, unsigned char* dst_host,
                          int max_workgroups);

/* The frames of the reference's orbit video (visualize.py:403-416), composed in one kernel from the float32 planes where they lie:
 * per frame, every image of the batch is a strip of n_panels panels of H x W pixels, left to right, and the strips are laid out as
 * torchvision's make_grid(tensor[n_images,3,H,n_panels*W], nrow, padding, pad_value = 0) lays them out:
 *   xmaps = min(nrow, n_images), ymaps = ceil(n_images / xmaps); a frame is [ymaps*(H+pad)+pad, xmaps*(n_panels*W+pad)+pad, 3] uint8
 *   (HWC); image k has its top-left corner at (k / xmaps * (H+pad) + pad, k % xmaps * (n_panels*W+pad) + pad); padding and cells
 *   without an image are 0. n_images == 1: the bare H x n_panels*W strip, no padding (what make_grid returns for one image).
 * A panel is described by f3dg_panel: pixel (y, x) of plane c of image k in frame f is
 *   src[k * image_stride + f * frame_stride + c * plane_stride + y * W + x]   (strides in floats; rows contiguous)
 * so [B,V,C,H,W] tensors, a channel slice of a [B*V,9,H,W] raster, and a static [B,C,H,W] input (frame_stride = 0: the same on
 * every frame) are all read in place. `kind` decides the bytes:
 *   F3DG_PANEL_RGB      3 planes: byte = (unsigned)(255.0f * fminf(fmaxf(v, 0), 1)), the rule of f3dg_pack_frames (NaN -> 0);
 *   F3DG_PANEL_SIGNED   3 planes, or 1 plane repeated: v' = (v + 1.0f) / 2.0f in float32, then the RGB rule (depth_normal, :412);
 *   F3DG_PANEL_COLORMAP 1 plane d: the reference's colorize() (src/utils.py:94-150) with its defaults. vmin, vmax =
 *       ranges[range_index][0..1]; t = (d - vmin) / (vmax - vmin) in float32 (IEEE divide), t = d * 0 when vmin == vmax;
 *       d == invalid_val -> (128,128,128); NaN t -> (0,0,0); t < 0 -> lut[0]; t >= 1 -> lut[255]; else lut[(int)(t * 256)].
 *       The bytes written are the table's own (the reference's / 255 ... 255 * round trip is the identity on them).
 * lut [256][3] uint8 and ranges [.][2] float32 are DEVICE arrays, read only when a COLORMAP panel exists (NULL otherwise); the
 * call carries no row count of `ranges`: the CALLER guarantees 0 <= range_index < its rows (a negative one is F3DG_ERR_BAD_ARG);
 * `panels` is a HOST array of n_panels (1 .. F3DG_MAX_PANELS) descriptors, passed to the kernel by value.
 * dst: n_frames frames, 16-byte aligned, every byte written. dst_is_host != 0: dst is PINNED host memory (anything else is
 * F3DG_ERR_BAD_ARG), written by the kernel as f3dg_pack_frames_host does. A lane produces 16 consecutive bytes of the stream and
 * stores them at once; the kernel is grid-stride with at most max_workgroups workgroups (0: 64 for host memory, 2048 otherwise).
 * Offsets into src and dst are 64-bit; one frame must stay below 4 GB.
 * F3DG_ERR_BAD_ARG before any launch: NULL dst / panels / panel src, n_panels outside 1..8, nrow < 1, non-positive sizes, negative
 * padding, a COLORMAP panel with NULL lut or ranges, planes not matching kind, an unknown kind, a misaligned dst. */
#define F3DG_MAX_PANELS 8
#define F3DG_PANEL_RGB 0
#define F3DG_PANEL_SIGNED 1
#define F3DG_PANEL_COLORMAP 2
typedef struct f3dg_panel {
    const float* src;
    size_t image_stride, frame_stride, plane_stride;
    int kind, planes, range_index;
} f3dg_panel;
int f3dg_compose_frames(void* stream, int n_frames, int n_images, int H, int W, int nrow, int padding, int n_panels,
                        const f3dg_panel* panels, const unsigned char* lut, const float* ranges, float invalid_val,
                        unsigned char* dst, int dst_is_host, int max_workgroups);
/* Height, width and total byte count (n_frames frames) of what f3dg_compose_frames writes; any output pointer may be NULL. */
int f3dg_compose_frames_size(int n_frames, int n_images, int H, int W, int nrow, int padding, int n_panels,
                             int* frame_h, int* frame_w, size_t* n_bytes);

/* Hand-off of the cycle aggregation (reference visualize.py:311, 331-333): from the rendered rasters [B * V, 9, H, W] (frame
 * b * V + v) to the next predictor inputs, view-major: xin [V, B, 4, H, W] = cat(clamp(rgb, 0, 1), alpha) and
 * depth [V, B, 1, H, W] = the median depth. One kernel; H * W must be a multiple of 4 and the pointers 16-byte aligned. */
int f3dg_cycle_inputs(void* stream, int B, int V, int H, int W, const float* raster, float* xin, float* depth);

/* Adjoint of f3dg_cycle_inputs: the vector-Jacobian product that torch.autograd derives from the hand-off's torch lines
 * (clamp, two slices, cat). The same launch shape as the forward: one thread per four pixels, 16-byte loads and stores, grid.y = B * V.
 *   raster   [B * V, 9, H, W]: the forward's input, read for the clamp mask only (channels 0..2).
 *   g_xin    [V, B, 4, H, W], g_depth [V, B, 1, H, W]: the cotangents, view-major as the forward wrote its outputs. Either may be
 *            NULL = "this output was not used": all of its entries count as zero.
 *   d_raster [B * V, 9, H, W], image-major: frame n = b * V + v takes its cotangents from slot v * B + b. Every element is written
 *            (no accumulation, the caller need not zero it):
 *     channels 0..2   g_xin[slot, c] where 0 <= raster <= 1 (0, 1 and -0.0 pass; NaN and +-Inf do not), else +0.0. The masked value is
 *                     SELECTED, never g * 0: a masked position is +0.0 even under a NaN or Inf cotangent;
 *     channel  7      g_xin[slot, 3];      channel 6      g_depth[slot];      channels 3, 4, 5, 8      0.
 * F3DG_ERR_BAD_ARG before any HIP call: NULL raster or d_raster, non-positive V, H or W, B < 0, H * W not a multiple of 4, a pointer
 * that is not 16-byte aligned, B * V > 65,535. B == 0: F3DG_OK at once. */
int f3dg_cycle_inputs_backward(void* stream, int B, int V, int H, int W, const float* raster,
                               const float* g_xin, const float* g_depth, float* d_raster);

/* The SongUNet backbone's kernels between the convolutions. `dtype` names the activations' type -- F3DG_BF16 and F3DG_F16 are the bf16 /
 * fp16 options of the backbone, 16-bit values in and out; parameters, statistics and all arithmetic are float32 / float64 whatever it is.
 * `nhwc` their layout: 0 = [N,C,HW] contiguous (NCHW), 1 = [N,HW,C] (channels-last, the backbone's "nhwc" layout option: MIOpen's NHWC
 * convolution kernels without the layout transposes around them). */
enum { F3DG_F32 = 0, F3DG_BF16 = 1, F3DG_F16 = 2 };

/* Fused GroupNorm (+ SiLU when apply_silu != 0; src/gaussian_predictor.py:250-262 and the `silu(norm(x))` of the residual blocks,
 * :318-323): x, y as `dtype` and `nhwc` say, weight / bias [C] float32, statistics per (sample, group) over C/groups x HW
 * values, biased variance, y = (v - mean) / sqrt(var + eps) * weight + bias with v = x + pre_bias[c]. pre_bias ([C] float32, may be NULL)
 * is the bias of the convolution that produced x, which PyTorch-ROCm would apply as a separate elementwise pass behind MIOpen's kernel
 * (src/gaussian_predictor.py:163-178); the residual blocks hand it to the GroupNorm that follows. x == y (in place) is allowed.
 * Both layouts sum (v - K) and (v - K)^2, K the first value of the (sample, group), so that the variance keeps torch's float32 accuracy
 * when a group's mean is far from zero (measured up to |mean| / std = 100 and on constant groups: tests/test_backbone_kernels_gpu.py).
 * `stats` (may be NULL; F3DG_F32 only, 8-byte aligned): [N, groups, 2] float32 = (mean, 1 / sqrt(var + eps)) per (sample, group), kept
 * for f3dg_group_norm_silu_backward; y is the same with and without it. (f3dg_group_norm_silu_forward_stats keeps them in every dtype.)
 * `scratch` / `scratch_bytes`: channels-last only (NULL / 0 with nhwc = 0), f3dg_group_norm_nhwc_scratch_bytes(N, HW, groups) bytes: one
 * (sum, sum of squares) pair per workgroup, sample and group, added up in workgroup order by a second-stage kernel -- no atomics, the
 * statistics are bit-reproducible from run to run. `scratch_bytes` is the size of the buffer behind `scratch`: the scratch has grown with
 * the kernels, and a buffer sized by an older header is refused with F3DG_ERR_WORKSPACE instead of being written past its end.
 * F3DG_ERR_BAD_ARG before any HIP call, nothing written: a dtype outside 0..2, stats with a 16-bit dtype or off the 8-byte grid, a NULL
 * x / weight / bias / y (channels-last: scratch), non-positive C / HW / groups, N < 0, groups that do not divide C, x or y not 16-byte
 * aligned, channels-last C that is no multiple of 4 (float32) / 8 (16-bit) or above 1024. N == 0: F3DG_OK and no work. */
size_t f3dg_group_norm_nhwc_scratch_bytes(int N, int HW, int groups);
int f3dg_group_norm_silu_forward(void* stream, int dtype, int nhwc, int N, int C, int HW, int groups,
                                 const void* x, const float* pre_bias, const float* weight, const float* bias,
                                 float eps, int apply_silu, void* y, float* stats, void* scratch, size_t scratch_bytes);
/* f3dg_group_norm_silu_forward keeping its statistics in EVERY dtype, for f3dg_group_norm_silu_backward_dtype: the same launch, y the same
 * bit for bit as f3dg_group_norm_silu_forward writes with the same arguments, and `stats` ([N, groups, 2] float32, 8-byte aligned,
 * REQUIRED) = (mean, 1 / sqrt(var + eps)) per (sample, group) -- float32 whatever the activations are. Refused as the call above refuses
 * (F3DG_ERR_BAD_ARG / F3DG_ERR_WORKSPACE before any HIP call, nothing written), and with F3DG_ERR_BAD_ARG for a NULL stats; a 16-bit dtype
 * is no refusal here. N == 0: F3DG_OK and no work. */
int f3dg_group_norm_silu_forward_stats(void* stream, int dtype, int nhwc, int N, int C, int HW, int groups,
                                       const void* x, const float* pre_bias, const float* weight, const float* bias,
                                       float eps, int apply_silu, void* y, float* stats, void* scratch, size_t scratch_bytes);
/* The residual join of a backbone block (src/gaussian_predictor.py:325-327: the second convolution's bias, `x = x + skip(orig)` with the
 * skip convolution's bias, `x = x * skip_scale`) as ONE elementwise pass: y = ((a + bias_a[c]) + (b + bias_b[c])) * scale in float32,
 * the reference's order. a, b, y as `dtype` and `nhwc` say, 16-byte aligned, N*C*HW a multiple of 4 (float32) / 8 (16-bit) -- and C as
 * well when nhwc = 1; either bias may be null; y may alias a or b. Anything else, and a dtype outside 0..2, is F3DG_ERR_BAD_ARG. */
int f3dg_residual_join_forward(void* stream, int dtype, int nhwc, int N, int C, int HW,
                               const void* a, const float* bias_a, const void* b, const float* bias_b, float scale, void* y);
/* Training through the backbone: the adjoints of the kernels above, both layouts (nhwc = 0: [N,C,HW]; nhwc = 1: [N,HW,C]). The two
 * float32 entry points came first; the *_dtype forms behind them take every activation type, and the float32 ones are calls of those
 * with F3DG_F32.
 *
 * f3dg_group_norm_silu_backward takes `stats` from f3dg_group_norm_silu_forward and recomputes everything else from x. With v = x + pre_bias, xh = (v - mean) * rstd, z = weight * xh + bias
 * (formed as the forward forms it: the mean taken off before the scale), m = (C / groups) * HW:
 *   dz = grad_y * s * (1 + z * (1 - s)), s = sigmoid(z)   (apply_silu != 0; dz = grad_y otherwise)
 *   A[n, c] = sum_hw dz,  B[n, c] = sum_hw dz * xh,  s1[n, g] = sum_c weight[c] A / m,  s2[n, g] = sum_c weight[c] B / m
 *   grad_x = rstd * (dz * weight - s1 - xh * s2)             [as x]
 *   grad_weight[c] = sum_n B,  grad_bias[c] = sum_n A,  grad_pre_bias[c] = sum_{n, hw} grad_x      [C] each
 * Any of the four outputs may be NULL (not wanted); the others are overwritten, not accumulated into. Every sum is taken in float32 over
 * short runs and combined in float64 in a fixed order, without atomics: the gradients are bit-identical from run to run. pre_bias may be
 * NULL. `scratch`: f3dg_group_norm_silu_backward_scratch_bytes(N, C, HW, groups, nhwc) bytes, 8-byte aligned (the per-(sample, channel)
 * sums, the (s1, s2) pairs and, channels-last, a triple per workgroup and channel).
 * Refused as the forward refuses, before anything is written: F3DG_ERR_BAD_ARG for a NULL x / weight / bias / stats / grad_y / scratch,
 * groups that do not divide C, x / grad_y / grad_x not 16-byte aligned, channels-last C that is no multiple of 4 or above 1024;
 * F3DG_ERR_WORKSPACE for scratch_bytes below the size above. N == 0: F3DG_OK and no work. */
size_t f3dg_group_norm_silu_backward_scratch_bytes(int N, int C, int HW, int groups, int nhwc);
int f3dg_group_norm_silu_backward(void* stream, int N, int C, int HW, int groups, int nhwc, const float* x, const float* pre_bias,
                                  const float* weight, const float* bias, const float* stats, int apply_silu, const float* grad_y,
                                  float* grad_x, float* grad_weight, float* grad_bias, float* grad_pre_bias, void* scratch,
                                  size_t scratch_bytes);
/* The same in the activation type `dtype` names: x, grad_y and grad_x are float32, bfloat16 or float16 (16-byte packets of 4 / 8 values);
 * pre_bias, weight, bias, `stats` (from f3dg_group_norm_silu_forward_stats) and the three parameter gradients stay float32. A 16-bit
 * value is widened exactly, all arithmetic and every sum is the float32 call's (nothing is rounded before it enters a sum), and grad_x is
 * rounded to the type ONCE, to nearest even; a float16 grad_x beyond the type's range is +-Inf, never a clamped value (a loss scaler
 * detects overflow by that). No atomics: bit-identical from run to run; a non-finite grad_y stays inside its (sample, group). The scratch
 * is f3dg_group_norm_silu_backward_scratch_bytes whatever the dtype. NCHW takes whole packets where HW is a multiple of 4 / 8 and single
 * values otherwise. Refused as above, and with F3DG_ERR_BAD_ARG for a dtype outside 0..2 and for a channels-last C that is no multiple
 * of 4 (float32) / 8 (16-bit) or above 1024. N == 0: F3DG_OK and no work. */
int f3dg_group_norm_silu_backward_dtype(void* stream, int dtype, int N, int C, int HW, int groups, int nhwc, const void* x,
                                        const float* pre_bias, const float* weight, const float* bias, const float* stats, int apply_silu,
                                        const void* grad_y, void* grad_x, float* grad_weight, float* grad_bias, float* grad_pre_bias,
                                        void* scratch, size_t scratch_bytes);
/* The adjoint of f3dg_residual_join_forward in ONE pass over grad_y: grad_ab = grad_y * scale [as grad_y], which is the gradient of a and of b
 * alike, and grad_bias[c] = the sum of grad_ab over channel c ([C], the gradient of either bias; NULL = not wanted), summed in float64 in
 * a fixed order without atomics. grad_ab may be grad_y. `scratch` (needed only with grad_bias): f3dg_residual_join_backward_scratch_bytes
 * bytes, 8-byte aligned; less is F3DG_ERR_WORKSPACE. F3DG_ERR_BAD_ARG as the forward: N*C*HW no multiple of 4, pointers not 16-byte
 * aligned, channels-last C no multiple of 4 (or above 1024). N == 0: F3DG_OK and no work. */
size_t f3dg_residual_join_backward_scratch_bytes(int N, int C, int HW, int nhwc);
int f3dg_residual_join_backward(void* stream, int N, int C, int HW, int nhwc, const float* grad_y, float scale, float* grad_ab,
                                float* grad_bias, void* scratch, size_t scratch_bytes);
/* The same in the activation type `dtype` names: grad_y and grad_ab are float32, bfloat16 or float16, grad_bias float32. grad_ab is the
 * float32 product grad_y * scale rounded to the type once (to nearest even; float16 overflow is +-Inf); grad_bias sums the float32
 * products themselves, not their rounded copies. The scratch is f3dg_residual_join_backward_scratch_bytes whatever the dtype.
 * F3DG_ERR_BAD_ARG as above with the packet of the type -- N*C*HW, and channels-last C, a multiple of 4 (float32) / 8 (16-bit) -- and for a
 * dtype outside 0..2. N == 0: F3DG_OK and no work. */
int f3dg_residual_join_backward_dtype(void* stream, int dtype, int N, int C, int HW, int nhwc, const void* grad_y, float scale,
                                      void* grad_ab, float* grad_bias, void* scratch, size_t scratch_bytes);

/* Fused differentiable image loss: SSIM (+ L1, L2) of n_planes pairs of H x W planes -- a plane is one channel of one frame; img1, img2
 * and every plane set below are float32, planar and contiguous, [n_planes, H, W].
 * Definition (utils/loss_utils.py:23-63 with window_size 11):
 *   g[i] = float32(exp(-(i - 5)^2 / 4.5)) divided by their float32 sum, i = 0..10 (six distinct values); G*x is the windowed sum of x,
 *   zero-padded by 5 on every side, with the window g (x) g. The library evaluates it separably (11 + 11 taps, horizontal first); the
 *   reference uses one 121-tap window whose entries are the float32-rounded products.
 *   C1 = float32(0.01^2), C2 = float32(0.03^2); a = img1, b = img2; per pixel
 *     mu1 = G*a, mu2 = G*b, sigma1^2 = G*(a a) - mu1^2, sigma2^2 = G*(b b) - mu2^2, sigma12 = G*(a b) - mu1 mu2
 *     m = (2 mu1 mu2 + C1)(2 sigma12 + C2) / ((mu1^2 + mu2^2 + C1)(sigma1^2 + sigma2^2 + C2))
 *   every operation one float32 rounding (no contraction).
 * f3dg_ssim_forward writes, each optional (NULL = skip):
 *   map            m
 *   dm_dmu1, dm_dsigma1_sq, dm_dsigma12   the partial derivatives of m that f3dg_ssim_backward reads (dm_dmu1 with G*(a a) and G*(a b)
 *                  held fixed, i.e. including the mu1 inside sigma1^2 and sigma12)
 *   plane_sums     [n_planes,3]: the sums over the plane of m, of |a - b| and of (a - b)^2. Needs `partials`, a scratch buffer of
 *                  f3dg_ssim_partials_bytes(n_planes, W, H) bytes (partials_bytes = its size): every tile writes its own slot, a second
 *                  kernel adds the slots of a plane in a fixed order. No float atomics: the sums are bit-reproducible from run to run,
 *                  and the sums of one plane do not depend on any other plane's data.
 * f3dg_ssim_backward writes dL/dimg1 (every element) for
 *   L = sum_q dL_dmap(q) m(q)  +  sum_planes ( w[0] sum m + w[1] sum |a - b| + w[2] sum (a - b)^2 ),   w = plane_weights [n_planes,3]
 * from either cotangent or both (dL_dmap [n_planes,H,W]; NULL = absent). With plane_weights alone -- the case of a mean -- no gradient
 * plane exists in memory.
 *   dL/da(p) = sum_q g(q - p) [ w(q) dm_dmu1(q) + 2 a(p) w(q) dm_dsigma1_sq(q) + b(p) w(q) dm_dsigma12(q) ]
 *              + w[1] sign(a - b)(p) + 2 w[2] (a - b)(p),     w(q) = dL_dmap(q) + w[0],  sign(0) = 0 (torch.abs's gradient)
 * The three derivative planes are those a f3dg_ssim_forward on the same img1, img2 wrote; they are required (this library saves them
 * rather than recompute them from a 10-pixel halo). img2 gets no gradient: m is symmetric, a caller who needs it swaps the arguments.
 * F3DG_ERR_BAD_ARG: a NULL required pointer, non-positive sizes, plane_sums without partials, a backward with neither cotangent.
 * F3DG_ERR_WORKSPACE: partials_bytes too small. F3DG_ERR_UNSUPPORTED: more than 2^31 - 1 tiles (32 x 16 pixels) in the call.
 * f3dg_ssim_partials_bytes returns 0 for non-positive sizes. All checks happen before any HIP call. */
size_t f3dg_ssim_partials_bytes(int n_planes, int W, int H);
int f3dg_ssim_forward(void* stream, int n_planes, int W, int H, const float* img1, const float* img2, float* map,
                      float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, float* partials, size_t partials_bytes,
                      float* plane_sums);
int f3dg_ssim_backward(void* stream, int n_planes, int W, int H, const float* img1, const float* img2, const float* dL_dmap,
                       const float* plane_weights, const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                       float* dL_dimg1);

/* Fused geometry losses: the terms the reference's trainer weighs besides RGB (config/imagenetgs_256x256_v1.yaml:50-66: w_depth_normal,
 * w_distortion, w_depth, w_normal, w_alpha) on raster [n_frames,9,H,W], summed per frame -- one forward kernel that never writes the
 * two derived maps, one backward kernel that writes dL/draster directly. Everything is float32, planar and contiguous.
 * Per pixel: N = normal_world and D = depth_normal EXACTLY as f3dg_render_epilogue_view defines them (world_view [n_frames,16] in the
 * row-vector convention, c2w = inverse(world_view^T) by float64 cofactors per frame, the same fx, fy, D = 0 on the border, F.normalize's
 * 1e-12 clamp on both normalisations); n^ = normalize(raster[3:6]) in the camera frame; d = raster[6], alpha = raster[7]; m = mask
 * ([n_frames,H,W]; NULL = 1).
 *   term 0  depth-normal consistency  w (1 - <N, D>),  w = 1, or alpha with F3DG_GEOM_ALPHA_WEIGHT (w is data: it gets no gradient)
 *   term 1  distortion                raster[8]
 *   term 2  depth                     m |d - depth_target|                 depth_target [n_frames,H,W]
 *   term 3  normal                    m (1 - <n^, normal_target>)          normal_target [n_frames,3,H,W], used as given
 *   term 4  alpha                     |alpha - alpha_target|               alpha_target [n_frames,H,W]
 * f3dg_geometry_loss_forward writes frame_sums [n_frames,5]: the sum of every term over the frame's pixels. A NULL target skips its term:
 * the sum is written as 0. `partials` is a scratch buffer of f3dg_geometry_loss_partials_bytes(n_frames, W, H) bytes (partials_bytes =
 * its size): every 32 x 16 tile writes its own slot, a second kernel adds one frame's slots in a fixed order. No float atomics: the sums
 * are bit-reproducible, and the sums of one frame depend on no other frame's data.
 * f3dg_geometry_loss_backward ASSIGNS every element of dL_draster [n_frames,9,H,W] for L = sum_f sum_k frame_weights[f,k] frame_sums[f,k]
 * (frame_weights [n_frames,5] = W0..W4 of a frame), one thread per (frame, pixel), no atomics:
 *   channels 0..2  0
 *   channels 3..5  F.normalize's backward (g / 1e-12 where its clamp is active) of  -W0 w c2w[:3,:3]^T D - W3 m normal_target
 *   channel 6      W2 m sign(d - depth_target) + the gather of term 0 over the up to four interior axial neighbours q whose depth normal
 *                  reads this pixel, in the order of f3dg_render_epilogue_backward, each with the cotangent -W0 w(q) N(q) on D(q)
 *   channel 7      W4 sign(alpha - alpha_target)
 *   channel 8      W1
 * sign(0) = 0. A term with a NULL target contributes nothing, and neither does a term whose weight is exactly 0: it is not evaluated.
 * F3DG_ERR_BAD_ARG: NULL raster, world_view, frame_sums or partials (forward), frame_weights or dL_draster (backward); non-positive
 * sizes; flag bits other than F3DG_GEOM_ALPHA_WEIGHT. F3DG_ERR_WORKSPACE: partials_bytes too small. F3DG_ERR_UNSUPPORTED: 9 H W or the
 * number of tiles beyond 2^31 - 1. f3dg_geometry_loss_partials_bytes returns 0 for non-positive sizes. All checks happen before any
 * HIP call. */
#define F3DG_GEOM_ALPHA_WEIGHT 1
size_t f3dg_geometry_loss_partials_bytes(int n_frames, int W, int H);
int f3dg_geometry_loss_forward(void* stream, int n_frames, int H, int W, const float* raster, const float* world_view, float fx, float fy,
                               int flags, const float* depth_target, const float* normal_target, const float* alpha_target,
                               const float* mask, float* partials, size_t partials_bytes, float* frame_sums);
int f3dg_geometry_loss_backward(void* stream, int n_frames, int H, int W, const float* raster, const float* world_view, float fx, float fy,
                                int flags, const float* depth_target, const float* normal_target, const float* alpha_target,
                                const float* mask, const float* frame_weights, float* dL_draster);

/* Forward warp: source frames splatted into new cameras by their depth, with a z-buffer -- the masked pseudo-target of the settings'
 * w_warping / w_prop. THE SEMANTICS ARE THIS PROJECT'S (the reference holds no warp); tests/warp_truth.py restates them in float64.
 * Everything is float32, planar and contiguous. n_src source frames, n_views target cameras each: pair p = b * n_views + v.
 *   image [n_src,C,H,W], 1 <= C <= 16; depth [n_src,H,W] z-depth; valid [n_src,H,W] or NULL (a source pixel takes part iff valid > 0);
 *   rel [n_src,n_views,16]: row-major 4 x 4, rel[b,v] = inverse(src_world_view[b]) dst_world_view[b,v] in the row-vector convention.
 * Projection. Source pixel (column i, row j) with d = depth[b,j,i] is live iff it is valid, d is finite and d > 0. Its camera point is
 *   X = (i + 0.5 - W/2) / fx * d, Y = (j + 0.5 - H/2) / fy * d, Z = d (the rasterizer's pixel centre), in the target camera
 *   (x,y,z) = X rel[0,:3] + Y rel[1,:3] + Z rel[2,:3] + rel[3,:3]; it stays live iff z > z_near. u = fx x / z + W/2 - 0.5,
 *   v = fy y / z + H/2 - 0.5. The library evaluates this in float64 on the float32 arguments.
 * Footprint. x0 = floor(u), y0 = floor(v), a = u - x0, b = v - y0; the four neighbours (x0 + dx, y0 + dy) have the bilinear weights
 *   w = (dx ? a : 1 - a)(dy ? b : 1 - b); a neighbour is a candidate iff it lies inside the image and w > 0. u and v are range-checked
 *   as floating-point numbers before any conversion to int: +-huge, +-Inf and NaN coordinates touch nothing.
 * Pass 1. zmin[t] = the least z (rounded to float32) over the candidates of target pixel t with w >= occlusion_min_weight; +inf
 *   without one. The floor keeps a point whose u lies 1e-7 past an integer from claiming the neighbouring pixel's z-buffer.
 * Pass 2. A candidate (any w > 0) contributes iff z <= zmin[t] + depth_tolerance: Wsum[t] += w, Csum[t,c] += w image[c], Zsum[t] += w z.
 *   The sums are 64-bit integers in units of q = 2^-24, each term rounded to nearest once: they do not depend on the order of arrival,
 *   and the outputs are bit-identical from run to run. Range: a term |w v| saturates at 2^15 = 32768 (|image| and depth up to there
 *   are exact; a non-finite colour of a live pixel saturates too), and H W <= 2^23 keeps every sum inside 63 bits.
 * Resolve. weight = Wsum; where Wsum > 0 (at least q / 2): warped = Csum / Wsum and warped_depth = Zsum / Wsum, elsewhere both 0;
 *   mask = (Wsum >= threshold) as 0.0 / 1.0.
 * Erode. erode = k odd, 3..15 (0 and 1: off): mask[t] = the minimum of the mask over the k x k window around t, neighbours outside
 *   the image ignored (-max_pool2d(-mask, k, 1, k / 2)).
 * EVERY element of warped [n_src,n_views,C,H,W], mask [n_src,n_views,1,H,W] and, when not NULL, warped_depth and weight
 * [n_src,n_views,1,H,W] is assigned. The colour and depth of a source pixel that is not live never enter arithmetic: a NaN there
 * reaches no output. `workspace` (8-byte aligned, f3dg_forward_warp_workspace_bytes(...) bytes, caller-owned) holds the accumulators
 * [pair][C + 2][H W], the z-buffer and the mask before erosion; the call initialises it. Five launches (four without erosion) for all
 * pairs.
 * F3DG_ERR_BAD_ARG: NULL image, depth, rel, workspace, warped or mask; a workspace off the 8-byte grid; non-positive n_src, n_views, C,
 * H or W; fx or fy not positive and finite; z_near negative or not finite; depth_tolerance negative or NaN; occlusion_min_weight outside
 * [0, 1]; a NaN threshold; erode negative, even or above 15. F3DG_ERR_UNSUPPORTED: C > 16, H W > 2^23, or more than 2^31 - 1 workgroups.
 * F3DG_ERR_WORKSPACE: workspace_bytes too small. f3dg_forward_warp_workspace_bytes returns 0 for every size the call refuses. All checks
 * happen before any HIP call. */
size_t f3dg_forward_warp_workspace_bytes(int n_src, int n_views, int C, int W, int H);
int f3dg_forward_warp(void* stream, int n_src, int n_views, int C, int H, int W, const float* image, const float* depth,
                      const float* valid, const float* rel, float fx, float fy, float z_near, float depth_tolerance,
                      float occlusion_min_weight, float threshold, int erode, void* workspace, size_t workspace_bytes,
                      float* warped, float* mask, float* warped_depth, float* weight);

/* Masked L1 of a [n_frames,C,H,W] against b (the warped frame) under m = mask [n_frames,1,H,W], in the mould of the geometry losses.
 * f3dg_masked_l1_forward writes frame_sums [n_frames,2] = (sum_c sum_pixels m |a - b|, sum_pixels m): a 32 x 16 tile per workgroup
 * writes its own slot of `partials` (f3dg_masked_l1_partials_bytes(n_frames, C, W, H) bytes), a second kernel adds one frame's slots in
 * a fixed order. No atomics: bit-reproducible, and a frame's sums read no other frame's data.
 * f3dg_masked_l1_backward ASSIGNS every element of dL_da = (g[f] m) sign(a - b), g[f] = frame_weights[f,0] (frame_weights [n_frames,2],
 * the cotangent of frame_sums; column 1 is not read: the mask gets no gradient), sign(0) = 0 as torch.abs's gradient.
 * F3DG_ERR_BAD_ARG: a NULL pointer, non-positive sizes. F3DG_ERR_WORKSPACE: partials_bytes too small. F3DG_ERR_UNSUPPORTED: C H W or the
 * number of tiles beyond 2^31 - 1. f3dg_masked_l1_partials_bytes returns 0 for those sizes. All checks happen before any HIP call. */
size_t f3dg_masked_l1_partials_bytes(int n_frames, int C, int W, int H);
int f3dg_masked_l1_forward(void* stream, int n_frames, int C, int H, int W, const float* a, const float* b, const float* mask,
                           float* partials, size_t partials_bytes, float* frame_sums);
int f3dg_masked_l1_backward(void* stream, int n_frames, int C, int H, int W, const float* a, const float* b, const float* mask,
                            const float* frame_weights, float* dL_da);

/* TSDF fusion: rendered depth maps fused into a truncated signed distance volume, the volume's surface cells as tetrahedra for
 * f3dg_marching_tets_count / _emit, and the crossing edges as vertices and vertex colours -- a mesh route that needs no external
 * tetrahedralisation. THE SEMANTICS ARE THIS PROJECT'S (the reference holds no TSDF code); tests/tsdf_truth.py restates them in float64.
 *
 * Volume. Dimensions (nx, ny, nz), `origin` [3] (a HOST array) the world position of the centre of voxel (0,0,0), `voxel` the edge
 *   length. Voxel (x, y, z) has the linear id (z ny + y) nx + x and the centre p = origin + voxel (x, y, z). nx ny nz < 2^31
 *   (F3DG_ERR_UNSUPPORTED beyond). Caller-owned state, float32, plane-major so that x is the fastest axis of every access:
 *   tsdf [nz,ny,nx] a weighted mean in [-1, 1], weight [nz,ny,nx], color [3,nz,ny,nx] a weighted mean, color_weight [nz,ny,nx].
 *   All-zero means empty.
 * One view's sample at a voxel. The conventions are the forward warp's: row-vector world_view [n_views,16] (row-major 4 x 4, a world
 *   point as a row times world_view is the camera point), the rasterizer's pixel centre, depth [n_views,H,W] read as z-depth.
 *   (X, Y, Z) = p world_view[:3,:3] + world_view[3,:3]. The sample is live iff Z > z_near. Pixel i = floor(fx X / Z + W/2),
 *   j = floor(fy Y / Z + H/2) (pixel i has its centre at i + 0.5); the two coordinates are range-checked as floating-point numbers
 *   before any conversion to int, so +-huge, +-Inf and NaN touch nothing; the sample stays live iff 0 <= coordinate < W (H).
 *   d = depth[v,j,i]; the sample stays live iff d is finite and d > 0 and, when `alpha` [n_views,H,W] is given, alpha[v,j,i] >= alpha_min
 *   (a NaN alpha is not live). sdf = d - Z; the sample is dropped iff sdf < -trunc; t = min(1, sdf / trunc). The sample is also a
 *   COLOUR sample iff |sdf| <= trunc: a free-space observation must not tint a voxel with the surface behind it. The colour
 *   (color [n_views,3,H,W]) and depth of a pixel that is not live never enter arithmetic. The library evaluates all of this in float64
 *   on the float32 arguments.
 * One call, n_views views. Per voxel, over the live samples in ascending view order: S = sum t, n = their number; Cs = sum colour,
 *   nc = the number of colour samples (float64 sums). Then, ASSIGNED once per call and rounded to float32 once:
 *   tsdf <- (tsdf weight + S) / (weight + n), weight <- weight + n where n > 0 and weight + n > 0; the same for color / color_weight
 *   with Cs and nc. A voxel with n = 0 (nc = 0) is not written: its tsdf and weight (color and color_weight) keep their bits. Every
 *   voxel has one writer, the views are taken in a fixed order and there are no atomics: the outputs are bit-reproducible. A second call
 *   accumulates further views into the same volume. Weights are float32 counts: exact up to 2^24 samples per voxel.
 *   One launch serves up to F3DG_TSDF_MAX_VIEWS views (the camera table of the kernel); a call with more runs consecutive launches over
 *   consecutive view ranges, which equals consecutive calls with those ranges to the bit. With color == NULL the arrays color_out and
 *   color_weight may be NULL and are untouched.
 * Surface cells. Cell (x, y, z), x < nx - 1, y < ny - 1, z < nz - 1, has the id (z (ny - 1) + y)(nx - 1) + x. It is ACTIVE iff all
 *   eight corners have weight >= min_weight and a finite tsdf, and the corners do not all agree on tsdf < 0. An active cell yields the
 *   six tetrahedra of the Kuhn split along its (0,0,0)-(1,1,1) diagonal, one per order of the axes, vertices as voxel ids: with b the
 *   cell's (0,0,0) corner and X = 1, Y = nx, Z = nx ny, in THIS order
 *       xyz (b, b+X+Y, b+X, b+X+Y+Z)   xzy (b, b+X, b+X+Z, b+X+Y+Z)   yxz (b, b+Y, b+X+Y, b+X+Y+Z)
 *       yzx (b, b+Y+Z, b+Y, b+X+Y+Z)   zxy (b, b+X+Z, b+Z, b+X+Y+Z)   zyx (b, b+Z, b+Y+Z, b+X+Y+Z)
 *   -- the path along the axes in the named order with the two middle vertices of three of the orders swapped, so that all six have
 *   the same orientation, the signed volume (v0 - v3) . ((v1 - v3) x (v2 - v3)) / 6 > 0. That is the orientation for which the triangle
 *   table of f3dg_marching_tets_emit turns every face's normal towards the free side (out of the surface); with the textbook volume
 *   above it is the even orders (xyz, yzx, zxy) whose path is swapped. tets [6 n_active, 4] int32, cells in ascending id.
 *   f3dg_tsdf_cells_count: classification, one bit per cell and the scanned counts into `workspace`
 *   (f3dg_tsdf_cells_workspace_bytes(nx, ny, nz) bytes, 16-byte aligned, caller-owned); BLOCKING, one host read: *h_n_active.
 *   f3dg_tsdf_cells_emit: after a count on the same workspace and volume; writes the tets, at most n_active cells of them (the capacity
 *   of `tets`, 16-byte aligned), and reads nothing back. On a workspace that holds no completed count of this volume it writes nothing.
 * Mesh. f3dg_marching_tets_count / _emit on sdf = -tsdf with these tets: occupied means behind the surface, tsdf == 0 is free.
 *   f3dg_tsdf_vertices, one thread per crossing edge (lo, hi) of interp_v [E,2] int64, in float32 in exactly this order: o = the end with
 *   tsdf < 0 (lo if both), f = the other; w = t_f / (t_f - t_o) where t_f - t_o > 0, else 0; p(id) = origin + voxel * (x, y, z);
 *   vertex = p_f + (p_o - p_f) * w; vertex colour = c_f + (c_o - c_f) * w per channel where both ends have color_weight > 0, the
 *   colour of the one end that has otherwise, 0 where neither has. vertices [E,3], vertex_colors [E,3] or NULL (then color and
 *   color_weight may be NULL). An id outside [0, nx ny nz) indexes nothing: that row is zeros.
 * F3DG_ERR_BAD_ARG, found on the host before any launch: a NULL required pointer (origin, depth, world_view, tsdf, weight; color_out or
 *   color_weight with a color; workspace, h_n_active, tets, interp_v, vertices; color or color_weight with vertex_colors); non-positive
 *   sizes (dimensions, n_views, H, W, E; n_active for emit); voxel, trunc, fx or fy not finite or <= 0; a non-finite origin; z_near
 *   negative or not finite; a NaN alpha_min or min_weight; a dimension below 2 for the cell entries; a workspace or tets off the 16-byte
 *   grid. F3DG_ERR_UNSUPPORTED: nx ny nz >= 2^31, H W >= 2^31. F3DG_ERR_WORKSPACE: workspace_bytes too small.
 *   f3dg_tsdf_cells_workspace_bytes returns 0 for every volume the cell entries refuse. */
#define F3DG_TSDF_MAX_VIEWS 128
int f3dg_tsdf_integrate(void* stream, int nx, int ny, int nz, const float* origin, float voxel, float trunc, float z_near, int n_views,
                        int H, int W, const float* depth, const float* color, const float* alpha, float alpha_min, const float* world_view,
                        float fx, float fy, float* tsdf, float* weight, float* color_out, float* color_weight);
size_t f3dg_tsdf_cells_workspace_bytes(int nx, int ny, int nz);
int f3dg_tsdf_cells_count(void* stream, int nx, int ny, int nz, float min_weight, const float* tsdf, const float* weight, void* workspace,
                          size_t workspace_bytes, long long* h_n_active);
int f3dg_tsdf_cells_emit(void* stream, int nx, int ny, int nz, void* workspace, size_t workspace_bytes, long long n_active, int* tets);
int f3dg_tsdf_vertices(void* stream, int nx, int ny, int nz, const float* origin, float voxel, long long E, const long long* interp_v,
                       const float* tsdf, const float* color, const float* color_weight, float* vertices, float* vertex_colors);

/* Mesh clean-up: the connected components of a triangle mesh, and the compaction that keeps the chosen ones. Integers only: every
 * output is a function of the input alone and bit-reproducible. THE SEMANTICS ARE THIS PROJECT'S; tests/mesh_clean_truth.py restates them.
 *
 * Mesh. faces [F,3] int64 (faces_int32 = 0) or int32 (faces_int32 = 1) over N vertices, 0 < N < 2^31, 0 <= F < 2^31.
 *   A face with an id outside [0, N) makes the call fail with F3DG_ERR_BAD_ARG: every id is range-checked on the device before anything
 *   is indexed with it, and a refused mesh writes none of the outputs.
 *   A face is DEGENERATE when two of its ids are equal. It belongs to no component: its label is -1, it is counted on its own and
 *   compaction always drops it.
 *   Two non-degenerate faces are CONNECTED when they share a VERTEX ID, and components are the classes of the transitive closure. This is
 *   vertex connectivity, not edge adjacency: the coarser relation (two unions per face, no edge table). It is the right one for floater
 *   removal -- a piece that touches the body in a single vertex is not a floater -- and it knows nothing of positions: two vertices at
 *   one place with two ids are two vertices (no welding).
 *   A component's LABEL is the least vertex id among the vertices of its faces (its root). A duplicate face counts as often as it occurs.
 * f3dg_mesh_components: BLOCKING. workspace: f3dg_mesh_components_workspace_bytes(N, F) bytes, 16-byte aligned, caller-owned.
 *   face_component [F] int32, every element written: the root of the face's component, -1 for a degenerate face.
 *   component_faces [N] int32, every element written: the number of faces of the component at its root's index, 0 everywhere else (a
 *   vertex no non-degenerate face uses is the root of nothing).
 *   h_counts[0..3] = number of components, faces of the largest, degenerate faces, rounds used. F == 0 is legal: all counts 0.
 *   Method: a union-find forest over the vertices in the workspace, parent[v] <= v at all times; a round is hook (two unions per face:
 *   roots are hooked by compare-and-swap, the greater root under the lesser, a failed swap continues from the value it returned),
 *   compress (every vertex to its root) and verify (a count of the faces whose corners do not all point at one self-parented root),
 *   followed by one 8-byte host read of that count and the range flag; rounds are repeated while the count is non-zero, at most 32 of
 *   them (F3DG_ERR_UNSUPPORTED beyond; with coherent atomics the first round converges). One more host read returns the counts.
 * f3dg_mesh_compact_count: BLOCKING, one host read. workspace: f3dg_mesh_compact_workspace_bytes(N, F) bytes, 16-byte aligned.
 *   face_component as f3dg_mesh_components wrote it, keep_root [N] uint8. A face is KEPT iff face_component >= 0 and
 *   keep_root[face_component] != 0 (a face_component >= N keeps nothing); a vertex is KEPT iff a kept face uses it. A kept face with an
 *   id outside [0, N) is F3DG_ERR_BAD_ARG as above. h_counts[0..1] = kept faces, kept vertices.
 * f3dg_mesh_compact_emit: after a count that returned F3DG_OK, same workspace, sizes and inputs; no host read.
 *   faces_out [n_faces_kept,3] int64: the kept faces in their input order, in the NEW numbering; vertex_ids [n_vertices_kept] int64: the
 *   old id of each new vertex, ascending (new id = the number of kept vertices with a smaller old id). The two counts are the capacities
 *   of the arrays: rows beyond them are not written. On a workspace that holds no completed count of a mesh of these sizes nothing is
 *   written.
 * Refused before any HIP call, nothing written (h_counts included): F3DG_ERR_BAD_ARG for a NULL workspace, face_component,
 *   component_faces, h_counts, keep_root, faces_out or vertex_ids (faces and face_component may be NULL where F == 0), N <= 0, F < 0,
 *   non-positive n_faces_kept or n_vertices_kept, a workspace off the 16-byte grid, faces_out or vertex_ids off the 8-byte grid; F3DG_ERR_UNSUPPORTED for N or F at or
 *   above 2^31; F3DG_ERR_WORKSPACE for workspace_bytes too small. The two *_workspace_bytes return 0 for every size the calls refuse. */
size_t f3dg_mesh_components_workspace_bytes(long long N, long long F);
int f3dg_mesh_components(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces, int faces_int32,
                         int* face_component, int* component_faces, long long* h_counts);
size_t f3dg_mesh_compact_workspace_bytes(long long N, long long F);
int f3dg_mesh_compact_count(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces,
                            int faces_int32, const int* face_component, const unsigned char* keep_root, long long* h_counts);
int f3dg_mesh_compact_emit(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces,
                           int faces_int32, const int* face_component, const unsigned char* keep_root, long long n_faces_kept,
                           long long n_vertices_kept, long long* faces_out, long long* vertex_ids);

/* Mesh smoothing and vertex normals: the vertex adjacency of a triangle mesh, Taubin lambda|mu smoothing over it, area-weighted vertex
 * normals (f3dg_mesh_smooth.hip). Integer atomics only and no float atomics: every output is a function of
 * the input alone and bit-reproducible. THE SEMANTICS ARE THIS PROJECT'S; tests/mesh_smooth_truth.py restates them in float64 numpy.
 *
 * Mesh. vertices [N,3] float32, faces [F,3] int64 (faces_int32 = 0) or int32 (faces_int32 = 1), 0 < N < 2^31, 0 <= F < 2^31 and
 *   6 F < 2^31 (nbr_start is int32 and the caller's nbr holds 6 F entries). An id outside [0, N) makes the call fail with
 *   F3DG_ERR_BAD_ARG: every id is range-checked on the device before anything is indexed with it, and a refused mesh writes none of the
 *   outputs (as f3dg_mesh_components). A face with two equal ids is DEGENERATE: it contributes nothing anywhere and is counted on its own.
 * Incidence rows. Every non-degenerate face f = (a, b, c) gives each corner two 64-bit entries  nbr << 32 | f << 1 | succ : corner a gets
 *   (b, f, 1) and (c, f, 0), corner b gets (c, f, 1) and (a, f, 0), corner c gets (a, f, 1) and (b, f, 0); succ marks the corner that
 *   follows in the face's winding. A vertex's ROW is its entries SORTED ASCENDING (atomics hand out the slots of the scatter; the sort
 *   erases their arrival order). The rows stay in the workspace for f3dg_mesh_vertex_normals.
 * Neighbours. N(v) = the distinct nbr values of v's row, ascending; deg(v) = |N(v)|. Edge (v, w) is a BOUNDARY edge iff exactly ONE entry
 *   of v's row has nbr == w (three or more entries for one w: non-manifold, not boundary). boundary[v] = 1 iff v has a boundary edge,
 *   else 0. The dense CSR: nbr_start [N+1] int32 (nbr_start[0] = 0, nbr_start[N] = 2E, E the number of undirected edges), nbr int32,
 *   N(v) at [nbr_start[v], nbr_start[v+1]). The caller sizes nbr at 6 F entries (2E <= 6 F), of which the first 2E are written.
 * f3dg_mesh_adjacency: BLOCKING, one host read. workspace: f3dg_mesh_adjacency_workspace_bytes(N, F) bytes, 16-byte aligned,
 *   caller-owned. boundary [N] uint8. h_counts[0..3] = 2E, boundary vertices, degenerate faces, entries of the longest row. F == 0 is
 *   legal: nbr_start and boundary are zeros, all counts 0.
 *   Method: one thread per face counts (range check first), one workgroup scans the counts (f3dg_scan.h), one thread per face scatters
 *   (atomicAdd on a per-vertex fill counter), rows of at most 32 entries are sorted by one thread, longer rows by a 1024-thread workgroup
 *   (a bitonic network in LDS up to 4,096 entries, in place beyond), one thread per vertex counts its distinct neighbours and sets its
 *   boundary flag, one workgroup scans the degrees, one thread per vertex writes its nbr segment. No thread waits on another's write.
 * One smoothing STEP with factor s. For a vertex that is not pinned and has deg > 0, in float64 with no contraction:
 *   S = sum over w in N(v), ascending in w, of (double)p_w (starting from 0.0), per coordinate, and
 *   p'_v = (float)( p_v + (double)s * ( S / (double)deg - p_v ) ).
 *   A pinned vertex (pinned[v] != 0) and a vertex with deg == 0 are copied through; both still count as neighbours of others.
 *   One Taubin ITERATION is a step with lambda followed by a step with mu; mu == 0 is Laplacian smoothing, one step per iteration.
 *   Only IEEE + - * / and one rounding to float32 per step: the kernel is bit-identical to the restatement.
 * f3dg_mesh_smooth: no host read, no workspace. nbr_start, nbr as f3dg_mesh_adjacency wrote them (an entry of nbr outside [0, N) is
 *   skipped: it adds nothing to S); pinned [N] uint8 or NULL (nothing pinned); vertices_in, scratch, vertices_out [N,3] float32, no two
 *   of them the same array (scratch may be NULL where the call takes at most one step). The steps ping-pong between vertices_out and
 *   scratch so that the last one lands in vertices_out; iterations == 0 copies vertices_in. vertices_in is never written.
 *   Valid: 0 < lambda <= 1; mu == 0 or mu < -lambda; iterations >= 0. (The usual choice: lambda 0.5, mu -0.53, 10 iterations.)
 * Vertex normals. For every entry of v's row with succ == 1, IN ROW ORDER (each incident face once, in a canonical order), the face's
 *   cross product (p1 - p0) x (p2 - p0) in the face's own corner order, in float64 from the float32 vertices:
 *   (uy wz - uz wy, uz wx - ux wz, ux wy - uy wx) with u = p1 - p0, w = p2 - p0. The cross products are summed in float64 from 0.0
 *   (area weighting), n = sqrt((sx sx + sy sy) + sz sz), and normals[v] = (float)(s / n) per coordinate; (0, 0, 0) where n is zero or
 *   not finite, and for a vertex with no face.
 * f3dg_mesh_vertex_normals: after an f3dg_mesh_adjacency that returned F3DG_OK, on the same workspace, sizes and faces; no host read.
 *   normals [N,3] float32. On a workspace that holds no completed adjacency build of a mesh of these sizes NOTHING is written (as
 *   f3dg_mesh_compact_emit). F == 0: zeros.
 * Refused before any HIP call, nothing written (h_counts included): F3DG_ERR_BAD_ARG for a NULL workspace, nbr_start, nbr (where F > 0),
 *   boundary, h_counts, faces (where F > 0), vertices_in, vertices_out, scratch (where more than one step is taken), vertices or normals;
 *   N <= 0, F < 0; a workspace off the 16-byte grid; lambda, mu or iterations outside the valid set above (NaN included); two of
 *   vertices_in, scratch, vertices_out equal. F3DG_ERR_UNSUPPORTED for N or F at or above 2^31 or 6 F at or above 2^31;
 *   F3DG_ERR_WORKSPACE for workspace_bytes too small. f3dg_mesh_adjacency_workspace_bytes returns 0 for every size the calls refuse. */
size_t f3dg_mesh_adjacency_workspace_bytes(long long N, long long F);
int f3dg_mesh_adjacency(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces, int faces_int32,
                        int* nbr_start, int* nbr, unsigned char* boundary, long long* h_counts);
int f3dg_mesh_smooth(void* stream, long long N, const int* nbr_start, const int* nbr, const unsigned char* pinned, const float* vertices_in,
                     float lambda, float mu, int iterations, float* scratch, float* vertices_out);
int f3dg_mesh_vertex_normals(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const void* faces,
                             int faces_int32, const float* vertices, float* normals);

/* Mesh simplification: uniform-grid vertex clustering (Rossignac-Borrel) with three placements of the representative vertex, the removal
 * of collapsed and duplicate faces, and the compaction of the result (f3dg_mesh_simplify.hip). Integer
 * atomics only and no float atomics: every output is a function of the input alone and bit-reproducible. THE SEMANTICS ARE THIS
 * PROJECT'S; tests/mesh_simplify_truth.py restates them in float64 numpy and the kernels equal it to the bit. Not edge-collapse
 * decimation: no error bound, no topology or manifold preservation, no tolerance-exact weld across cell boundaries, no gradients.
 *
 * Inputs. vertices [N,3] float32, faces [F,3] int64 (faces_int32 = 0) or int32 (1), 0 < N < 2^31, 0 <= F < 2^31; origin: 3 float64 ON
 *   THE HOST, finite; cell > 0, float64, finite; attrs [N,C] float32, 1 <= C <= F3DG_SIMPLIFY_MAX_ATTRS, or NULL with C = 0; placement =
 *   F3DG_SIMPLIFY_ROOT / _MEAN / _QUADRIC.
 * Cell. Per axis k, c_k = floor(((double)v_k - origin_k) / cell): one IEEE subtraction, one division, floor. 0 <= c_k < 2^21 is required.
 *   The KEY of a vertex is  c_x | c_y << 21 | c_z << 42.
 * Refusals found on the device. A non-finite coordinate, a cell index outside [0, 2^21), a face id outside [0, N): the count fails with
 *   F3DG_ERR_BAD_ARG. All three are found by the FIRST kernel, before anything is indexed with an id, and every later kernel returns on
 *   the flag: a refused mesh writes nothing but the workspace, and nothing to h_counts. One host read in the call.
 * Clusters. Vertices with equal keys form a CLUSTER. Its ROOT is its least vertex id; its MEMBERS are taken in ascending vertex id
 *   wherever an order matters. (Every vertex is in a cluster, whether a face uses it or not.)
 * Faces. A face with two equal input ids is DEGENERATE. Any other face whose three corners do not fall into three distinct clusters is
 *   COLLAPSED. Of the remaining faces those with the same SET of three clusters are DUPLICATES of one another, whatever their winding:
 *   the least face id among them SURVIVES (is KEPT), the others are counted as duplicates. Survivors keep their input order and their
 *   own winding. F = degenerate + collapsed + duplicate + kept, exactly.
 * Output vertices. The clusters that a surviving face uses, numbered by ascending root: n of them. vertex_map [N] int64 maps an old id
 *   to the new id of its cluster, -1 where the cluster is used by no surviving face. cluster_root [n] int64 and cluster_size [n] int64
 *   are the root and the number of members of each output vertex. faces_out [f,3] int64 in the new numbering.
 * Placement. Float64 from the float32 inputs, IEEE + - * / only, no contraction, sums taken one term at a time from 0.0 in the order
 *   named, one rounding to float32 at the end.
 *   ROOT: the root vertex's coordinates, copied bit for bit. With a small cell this is grid welding: positions that are equal to the bit
 *     always share a cell and are merged, while positions within `cell` of each other may straddle a cell boundary and stay apart.
 *   MEAN: pm = (sum of (double)p_m over the members, ascending) / (double)count, per coordinate; the vertex is (float)pm.
 *   QUADRIC: from pm. Walk the members in ascending order; for each member walk the entries of its sorted incidence row (above:
 *     f3dg_mesh_adjacency) with succ == 1, IN ROW ORDER -- the set and order f3dg_mesh_vertex_normals sums, so a face with k corners in
 *     the cluster is taken k times. For each such face, with its corners p0 p1 p2 in the face's own order, u = p1 - p0, w = p2 - p0:
 *       n = (uy wz - uz wy, uz wx - ux wz, ux wy - uy wx)                 (unnormalised: no sqrt anywhere, the weight is area^2)
 *       r = (nx (pmx - p0x) + ny (pmy - p0y)) + nz (pmz - p0z)
 *       Axx += nx nx, Axy += nx ny, Axz += nx nz, Ayy += ny ny, Ayz += ny nz, Azz += nz nz;   gx += r nx, gy += r ny, gz += r nz
 *     Then tr = (Axx + Ayy) + Azz, mu = (0.001 tr) / 3, and (A + mu I) D = -g is solved by the adjugate:
 *       a = Axx + mu, d = Ayy + mu, h = Azz + mu, b = Axy, c = Axz, e = Ayz
 *       c00 = d h - e e, c01 = c e - b h, c02 = b e - c d, c11 = a h - c c, c12 = b c - a e, c22 = a d - b b
 *       det = (a c00 + b c01) + c c02
 *       Dx = -((c00 gx + c01 gy) + c02 gz) / det,  Dy = -((c01 gx + c11 gy) + c12 gz) / det,  Dz = -((c02 gx + c12 gy) + c22 gz) / det
 *     D = 0 (the mean) unless tr > 0 and finite, det > 0 and finite, and every |D_k| <= cell (a D_k that is not finite fails that).
 *     The vertex is (float)(pm + D) per coordinate. The regulariser makes the system positive definite and leaves the unconstrained
 *     directions at the mean: a planar cluster stays at its mean, an edge cluster moves onto the edge, a corner cluster onto the corner.
 * Attributes. attrs_out[row][c] = (float)((sum of (double)attrs[m][c] over the members, ascending) / (double)count), for every placement.
 * f3dg_mesh_simplify_count: BLOCKING, one host read. workspace: f3dg_mesh_simplify_workspace_bytes(N, F) bytes, 16-byte aligned,
 *   caller-owned. h_counts[0..7] = clusters, used clusters (n), degenerate, collapsed, duplicate and kept (f) faces, members of the
 *   largest cluster, 0. F == 0 is legal: the clusters are counted, n = f = 0.
 *   Method: a least-id hash set (an open-addressed table of 32-bit ids, empty = 0xFFFFFFFF, a power of two of at least 16 and at least
 *   twice the items; an empty slot is claimed by compare-and-swap, an occupied one is joined by atomicMin when the OWNER's key,
 *   recomputed from the inputs, is the item's; a slot's key never changes) over the vertices under their cell keys, then a member CSR
 *   by count / scan / scatter / row sort (rows of at most 32 by one thread, longer ones by a 1024-thread workgroup, a bitonic network
 *   in LDS up to 4,096 members and in place beyond), then the same hash set over the faces that are neither degenerate nor collapsed
 *   under the sorted triple of their corners' roots (a face survives iff the lookup returns itself), then the flags, block counts and
 *   scans of the compaction. No thread waits on another's write; every loop is bounded.
 * f3dg_mesh_simplify_emit: after a count that returned F3DG_OK, same workspace, sizes, vertices and faces; no host read. The cell is the
 *   count's. n_vertices_out / n_faces_out are the capacities of the output arrays (the count's n and f): rows beyond them are not
 *   written. vertices_out [n,3] float32, faces_out [f,3] int64, attrs_out [n,C] float32 (NULL with C = 0), vertex_map [N], cluster_root
 *   [n], cluster_size [n] int64. With _QUADRIC, adjacency_workspace is the workspace of an f3dg_mesh_adjacency of these faces that
 *   returned F3DG_OK (NULL and 0 otherwise; 6 F < 2^31 then). On a workspace that holds no completed count of a mesh of these sizes,
 *   or, with _QUADRIC, an adjacency workspace that holds no completed build of them, NOTHING is written (as f3dg_mesh_vertex_normals).
 * Refused before any HIP call, nothing written (h_counts included): F3DG_ERR_BAD_ARG for a NULL workspace, vertices, origin, h_counts,
 *   faces (where F > 0; always for the emit), vertices_out, faces_out, vertex_map, cluster_root or cluster_size, attrs or attrs_out with
 *   C > 0, the adjacency workspace with _QUADRIC; N <= 0, F < 0, F == 0 for the emit; a cell that is not positive and finite, an origin
 *   that is not finite; a placement other than the three; C outside [0, F3DG_SIMPLIFY_MAX_ATTRS]; non-positive n_vertices_out or
 *   n_faces_out; a workspace off the 16-byte grid, an int64 output off the 8-byte grid; an output that is another output, an input or
 *   a workspace. F3DG_ERR_UNSUPPORTED for N or F at or above 2^31 (with _QUADRIC: 6 F at or above 2^31); F3DG_ERR_WORKSPACE for
 *   workspace_bytes or adjacency_workspace_bytes too small. f3dg_mesh_simplify_workspace_bytes returns 0 for every size the calls refuse. */
#define F3DG_SIMPLIFY_ROOT 0
#define F3DG_SIMPLIFY_MEAN 1
#define F3DG_SIMPLIFY_QUADRIC 2
#define F3DG_SIMPLIFY_MAX_ATTRS 64
size_t f3dg_mesh_simplify_workspace_bytes(long long N, long long F);
int f3dg_mesh_simplify_count(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const float* vertices,
                             const void* faces, int faces_int32, const double* origin, double cell, long long* h_counts);
int f3dg_mesh_simplify_emit(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const float* vertices,
                            const void* faces, int faces_int32, int placement, int C, const float* attrs, const void* adjacency_workspace,
                            size_t adjacency_workspace_bytes, long long n_vertices_out, long long n_faces_out, float* vertices_out,
                            long long* faces_out, float* attrs_out, long long* vertex_map, long long* cluster_root, long long* cluster_size);

/* Mesh rasteriser: a triangle mesh drawn from the renderer's cameras with an exact integer coverage test and a 64-bit z-buffer
 * (f3dg_mesh_raster.hip). Integer atomics only: every output is a function of the input alone and
 * bit-reproducible. THE SEMANTICS ARE THIS PROJECT'S; tests/mesh_raster_truth.py restates them in float64 numpy. No clipping, no
 * anti-aliasing, no gradients, no textures.
 *
 * Inputs. vertices [N,3] float32 (world space); faces [F,3] int64 (faces_int32 = 0) or int32 (1); world_views [V,4,4] float32 in the
 *   renderer's row-vector convention (m_rc = world_views[v][r][c]); fx, fy > 0 in pixels (W / (2 tan(fov / 2)), H / (2 tan(fov / 2)) as
 *   TSDFVolume.integrate forms them); z_near > 0; cull = F3DG_RASTER_CULL_NONE / _BACK / _FRONT; attrs [N,C] float32, 1 <= C <= 8, or
 *   NULL with C = 0. An id outside [0, N) makes the call fail with F3DG_ERR_BAD_ARG: every id is range-checked on the device before
 *   anything is indexed with it, and a refused mesh writes none of the outputs and nothing to h_counts.
 * Every (view, face) PAIR falls into exactly one of five classes, tested in this order:
 *   1. DEGENERATE by ids: two of the face's ids are equal. Nothing is projected.
 *   2. Projection of each corner, float64 on the float32 inputs, in this operation order:
 *        x = ((X m00 + Y m10) + Z m20) + m30,  y = ((X m01 + Y m11) + Z m21) + m31,  z = ((X m02 + Y m12) + Z m22) + m32,
 *        u = ((fx x) / z + W / 2) - 0.5,  v = ((fy y) / z + H / 2) - 0.5      (W / 2 = (double)W / 2.0, exact)
 *      so that pixel (i, j) -- column i, row j -- has its centre at u = i, v = j: the forward warp's convention and the renderer's.
 *      NEAR / NON-FINITE: a corner with a non-finite x, y or z, with not (z > z_near), or with a non-finite u or v. No clipping.
 *   3. GUARD BAND: a corner with not (|u| <= 16384 and |v| <= 16384), tested in floating point before anything becomes an integer.
 *   4. Snapping: U = rint(256 u), V = rint(256 v), ties to even (|U|, |V| <= 2^22). Everything about coverage is integer from here.
 *      Signed area A = (U1 - U0)(V2 - V0) - (V1 - V0)(U2 - U0). DEGENERATE (the same count as class 1): A == 0.
 *   5. CULLED. v grows downwards, so a face whose corners run counter-clockwise in world space as seen from outside (its normal
 *      (p1 - p0) x (p2 - p0) points at the camera) has A < 0 under a world_view with a proper rotation: A < 0 is FRONT.
 *      _CULL_BACK drops A > 0, _CULL_FRONT drops A < 0.
 *   What is left is RASTERISED (also when it covers no pixel centre).
 * Coverage. If A < 0, corners 1 and 2 change places FOR THE TEST (o = (0, 2, 1), else o = (0, 1, 2)). For each edge a -> b of the oriented
 *   triangle (o0 -> o1, o1 -> o2, o2 -> o0) and the pixel centre P = (256 i, 256 j):  E = (Ub - Ua)(Py - Va) - (Vb - Va)(Px - Ua)  in
 *   int64. The pixel is covered iff for all three edges  E > 0, or E == 0 and (Vb - Va > 0 or (Vb - Va == 0 and Ub - Ua < 0)):  a centre
 *   on the edge shared by two triangles belongs to exactly one of them, whatever their windings.
 * Depth and weights at a covered pixel, float64 with one rounding to float32 at the end. w_k = the edge value of the oriented edge
 *   opposite the face's OWN corner k (corner o0: edge o1 -> o2; o1: o2 -> o0; o2: o0 -> o1), lambda_k = (double)w_k / (double)|A| (both
 *   integers are exact in a double), q_k = 1 / z_k, and in the face's own corner order
 *        D = (lambda_0 q_0 + lambda_1 q_1) + lambda_2 q_2,   depth = (float)(1 / D),   beta_k = (lambda_k q_k) / D,
 *        bary_k = (float)beta_k,   attr_c = (float)((a_0c beta_0 + a_1c beta_1) + a_2c beta_2)        (a_kc = (double)attrs[id_k][c]).
 *   Only IEEE + - * / and rint: the kernels are bit-identical to the restatement.
 * Visibility. A pixel holds one 64-bit key  bits(depth) << 32 | face  (empty: all ones); keys are combined under an unsigned 64-bit
 *   atomicMin, so the nearest face wins and at equal float32 depth the least face id.
 * Outputs, EVERY element assigned by an accepted call: face_id [V,H,W] int32 (-1 where empty), depth [V,H,W] float32 (0 where empty),
 *   bary [V,3,H,W] float32 (0 where empty), attrs_out [V,C,H,W] float32 where attrs is given (0 where empty).
 *   h_counts[0..6] = pairs rasterised, dropped near / non-finite, dropped by the guard band, degenerate, culled (these five sum to
 *   V F), pairs queued as large (among the rasterised), covered pixels (face_id >= 0, all views).
 * f3dg_mesh_raster: BLOCKING, one host read at the end (the counts and whether an id was out of range). workspace:
 *   f3dg_mesh_raster_workspace_bytes(V, F, H, W) = 256 + align256(8 V H W) + align256(4 V F) bytes (a header, the keys, the queue of
 *   the large pairs), 16-byte aligned, caller-owned. F == 0 is legal: every pixel is empty.
 *   Method: one launch fills the keys; one thread per pair projects, snaps and takes the box of pixel centres i in [ceil(Umin / 256),
 *   floor(Umax / 256)] (and rows likewise) cut to the image: an empty box ends there, a box of at most 64 centres is walked by the
 *   thread, a larger one is queued (one integer atomic hands out the slot; the atomicMin erases the arrival order); a fixed grid reads
 *   the queue's length from device memory and strides the lanes of a wave over every box of at most 512 centres and the 256 threads of a
 *   workgroup over every larger one; one thread per pixel re-derives the winner's weights with the device function the scatter used
 *   and writes every output. No float atomics, no thread waits on another, every loop is bounded by a box or by the queue.
 * Refused before any HIP call, nothing written (h_counts included): F3DG_ERR_BAD_ARG for a NULL workspace, vertices, world_views,
 *   face_id, depth, bary or h_counts, NULL faces where F > 0, attrs without attrs_out or attrs_out without attrs, C outside 0..8 or not
 *   matching attrs (C == 0 iff attrs is NULL), N <= 0, F < 0, non-positive V, H or W, fx, fy or z_near not positive and finite, a cull
 *   outside 0..2, a workspace off the 16-byte grid. F3DG_ERR_UNSUPPORTED for N or F at or above 2^31, H or W above 16384, V H W or V F at
 *   or above 2^31. F3DG_ERR_WORKSPACE for workspace_bytes too small. f3dg_mesh_raster_workspace_bytes returns 0 for every size the call
 *   refuses. */
#define F3DG_RASTER_CULL_NONE 0
#define F3DG_RASTER_CULL_BACK 1
#define F3DG_RASTER_CULL_FRONT 2
size_t f3dg_mesh_raster_workspace_bytes(long long V, long long F, long long H, long long W);
int f3dg_mesh_raster(void* stream, void* workspace, size_t workspace_bytes, long long N, long long F, const float* vertices,
                     const void* faces, int faces_int32, int V, const float* world_views, double fx, double fy, int H, int W,
                     double z_near, int cull, int C, const float* attrs, int* face_id, float* depth, float* bary, float* attrs_out,
                     long long* h_counts);

/* Vertex colour baking: the views' colour put back on a mesh, every (view, vertex) sample tested against the z-buffer f3dg_mesh_raster
 * wrote for this mesh and these cameras (f3dg_mesh_bake.hip). THE SEMANTICS ARE THIS PROJECT'S;
 * tests/mesh_bake_truth.py restates them in float64 numpy. No gradients, no UV atlas or per-face texture, no seam or exposure
 * compensation between views, no clipping.
 *
 * Inputs. vertices [N,3] float32; normals [N,3] float32 or NULL; world_views [V,4,4] float32, row-vector convention as
 *   f3dg_mesh_raster; fx, fy, z_near doubles, formed as for f3dg_mesh_raster; images [V,C,H,W] float32, 1 <= C <= 8; face_id [V,H,W]
 *   int32 and depth [V,H,W] float32 as f3dg_mesh_raster wrote them for this mesh and these cameras; alpha [V,H,W] float32 or NULL;
 *   alpha_min double; depth_tol double, >= 0 and finite; cos_min double in [0,1]; mode F3DG_BAKE_BLEND (0) or F3DG_BAKE_BEST (1).
 * Projection: f3dg_mesh_raster's to the bit (one device function serves both), float64 on the float32 inputs with no contraction:
 *        x = ((X m00 + Y m10) + Z m20) + m30, likewise y and z;  u = ((fx x) / z + W / 2) - 0.5,  v = ((fy y) / z + H / 2) - 0.5;
 *   pixel centres sit at integer u, v.
 * Every (view, vertex) PAIR lands in exactly one of seven counted classes, tested in this order:
 *   1. NEAR: any of x, y, z, u, v is not finite, or not (z > z_near).
 *   2. OUTSIDE: not (0 <= u <= W - 1 and 0 <= v <= H - 1).
 *   3. UNCOVERED: with i = (int)rint(u), j = (int)rint(v) (ties to even), face_id[view][j][i] < 0.
 *   4. OCCLUDED: not (z - (double)depth[view][j][i] <= depth_tol).
 *   5. GRAZING (only with normals): n_c = ((nx m0c + ny m1c) + nz m2c) for c = 0, 1, 2;  g = -((n_0 x + n_1 y) + n_2 z);
 *      nn = (n_0 n_0 + n_1 n_1) + n_2 n_2;  pp = (x x + y y) + z z;  the pair is grazing iff nn is not finite, or not (nn > 0), or
 *      not (g > 0), or not (g g >= cm2 (nn pp)), with cm2 = cos_min cos_min formed on the host. Otherwise w = (g g) / (nn pp), which is
 *      cos^2 of the angle between the normal and the ray to the camera; no square root is taken. Without normals w = 1 and nothing is
 *      grazing.
 *   6. MASKED: the taps are i0 = (int)floor(u), i1 = min(i0 + 1, W - 1), j0 = (int)floor(v), j1 = min(j0 + 1, H - 1); masked iff alpha
 *      is given and not ((double)alpha >= alpha_min) at any of the four taps, or any of the 4 C colour taps is not finite.
 *   7. USED: the sample, float64, with a = u - i0, b = v - j0 and cxy the tap at column ix, row jy:
 *        top = c00 + a (c10 - c00),   bot = c01 + a (c11 - c01),   s_c = top + b (bot - top).
 * Per vertex, over its used samples in ASCENDING VIEW ORDER (the order of the sum is part of the definition):
 *   the best sample is the first used one, replaced by a later one iff that one's w > the best's w (the largest w, the earliest view
 *   at a tie);
 *   BLEND: Sw = Sw + w and S_c = S_c + w s_c from 0, float64, product then sum;  colors[i][c] = (float)(S_c / Sw),  weight[i] = (float)Sw;
 *   BEST:  colors[i][c] = (float)s_c of the best sample,  weight[i] = (float)w of it;
 *   both:  n_used[i] = the number of used samples,  best_view[i] = the view of the best sample.
 *   A vertex with no used sample gets colors = 0, weight = 0, n_used = 0, best_view = -1.
 * Outputs, EVERY element assigned by an accepted call: colors [N,C] float32, weight [N] float32, n_used [N] int32, best_view [N] int32.
 *   h_counts[0..7] = pairs near, outside, uncovered, occluded, grazing, masked, used (these seven sum to V N), then the vertices with
 *   n_used > 0.
 * Only IEEE + - * /, rint and floor in float64 and one rounding to float32 per output; no float atomics: the outputs are a function of
 *   the inputs alone and equal the restatement bit for bit.
 * f3dg_mesh_bake_colors: BLOCKING, one host read at the end (the counts). workspace: f3dg_mesh_bake_workspace_bytes(V, N, H, W) = 256
 *   bytes for every accepted size (the header of counters; the kernel stages its samples in LDS and keeps its sums in registers),
 *   16-byte aligned, caller-owned.
 *   Method: one launch. A wave takes 16 vertices x a slice of 4 consecutive views, one pair per lane; every lane classifies its pair
 *   and leaves (w, s_c) in LDS; one lane per vertex folds the slice in ascending view order into registers, and the same wave walks
 *   the vertex's slices in ascending order, so no partial sum is re-associated. The matrices are widened to double once per workgroup,
 *   128 views at a time, in a table the workgroup refills between two barriers: V is not limited by it. One integer atomicAdd per wave
 *   and class. No thread waits on another wave; every loop is bounded by V.
 * Refused on the host before any launch, nothing written (h_counts included): F3DG_ERR_BAD_ARG for a NULL workspace, vertices,
 *   world_views, images, face_id, depth, colors, weight, n_used, best_view or h_counts (normals and alpha may be NULL), a non-positive
 *   N, V, H or W, C outside 1..8, fx, fy or z_near not finite or <= 0, depth_tol negative or not finite, cos_min outside [0,1] or NaN,
 *   a NaN alpha_min when alpha is given, a mode outside {0, 1}, a workspace off the 16-byte grid. F3DG_ERR_UNSUPPORTED for H or W above
 *   16384, or N, V, V N or V H W at or above 2^31. F3DG_ERR_WORKSPACE for workspace_bytes too small.
 *   f3dg_mesh_bake_workspace_bytes returns 0 for every size the call refuses. */
#define F3DG_BAKE_BLEND 0
#define F3DG_BAKE_BEST 1
size_t f3dg_mesh_bake_workspace_bytes(long long V, long long N, long long H, long long W);
int f3dg_mesh_bake_colors(void* stream, void* workspace, size_t workspace_bytes, long long N, const float* vertices, const float* normals,
                          long long V, const float* world_views, double fx, double fy, long long H, long long W, double z_near,
                          int C, const float* images, const int* face_id, const float* depth, const float* alpha, double alpha_min,
                          double depth_tol, double cos_min, int mode, float* colors, float* weight, int* n_used, int* best_view,
                          long long* h_counts);

/* ---- Which Gaussians matter: contribution statistics and the pruning of a set (f3dg_contribution.hip) -----------
 *
 * For the views of a call and a pair (pixel, entry g of the pixel's tile list), walked in list order from T = 1 exactly as the exact
 * forward walks it, in the REFERENCE's arithmetic whatever the forward ran in:
 *   skipped   the pixel is done, or t <= 0.2, or alpha < 1/255: the pair counts nowhere;
 *   stopper   not skipped and T (1 - alpha) < 0.0001f: the pixel is done, stops[g] += 1. (The entry that ends a pixel's walk is not
 *             blended, but without it the pixel would blend on: "never blended" is not "no effect".)
 *   blended   any other pair: w = alpha T (the float32 number the exact forward adds to its alpha channel), blended[g] += 1,
 *             max_weight[g] = max(., w), sum_weight[g] += w, T = T (1 - alpha).
 * touched = blended + stops. A Gaussian with touched == 0 over a set of views can be removed without changing one bit of an exact
 * render of those views (kept rows in input order: the depth sort is stable by id).
 *
 * The record, F3DG_CONTRIBUTION_BYTES = 32 per Gaussian, 32-byte aligned:
 *   u64 sum_fixed  sum of round(w 2^32), half to even: exact and independent of the order of the pairs;  sum_weight = sum_fixed / 2^32
 *   u64 counts     blended | stops << 32
 *   u32 max_bits   the bits of max_weight (non-negative floats order as their bit patterns);  u32 pad[3]
 * Integer adds and an unsigned maximum only: every byte is bit-reproducible, run to run, culled or unculled lists, general or
 * small-call path, one call of n views or n calls of one.
 * LIMIT: the views x W x H pixels of all the calls that add into one array must stay below 2^31 (each counter then fits 32 bits, the
 * sum 63); f3dg_contribution refuses a call that alone reaches it, the caller watches the total.
 *
 * f3dg_contribution follows a forward (f3dg_forward_batched / f3dg_forward, any arithmetic, with or without F3DG_FLAG_SAVE_AUX, culled
 * lists or not, either path) on the same workspace with the same max_rendered, n_views, P, W, H and fields of view: everything it
 * reads -- the 64-byte records, the sorted lists, the tile ranges -- is still there. It ADDS into stats [P] and never clears it: the
 * caller zero-fills once and accumulates over calls. final_T (may be NULL) [n_views, H, W] receives every pixel's T at the end of its
 * walk -- plane 0 of the exact SAVE_AUX forward's final_T, to the bit. After a forward that overflowed max_rendered the lists are
 * empty: nothing is added, final_T is 1. P == 0 adds nothing.
 * BLOCKING: the workspace header (256 bytes) is read back first. F3DG_ERR_BAD_ARG: null workspace, a size out of range, stats null or off
 * the 32-byte grid with P > 0, a workspace whose forward rendered several Gaussian sets (f3dg_forward_sets with n_sets > 1: not
 * served); F3DG_ERR_WORKSPACE: workspace_bytes below f3dg_workspace_bytes of the shape; F3DG_ERR_STATE: the workspace's last forward had
 * another shape or capacity. One launch.
 *
 * f3dg_gaussian_compact_count / _emit: stream compaction of a Gaussian set, as the mesh routes' (count -> one host read -> emit).
 * Element i of P is kept when   blended + stops >= min_touched  and  max_weight >= min_max_weight  and  sum_weight >= min_sum_weight
 * (stats, may be NULL: no thresholds; sum_weight is (double)sum_fixed / 2^32) and keep[i] != 0 (keep, [P] bytes, may be NULL). At least
 * one of stats and keep must be given. min_touched >= 0; 0, 0.0f and 0.0 switch a threshold off; a NaN threshold is F3DG_ERR_BAD_ARG.
 * BLOCKING: *h_kept = the number of kept elements (the one host read). P == 0 keeps nothing. P above 2^28 - 1 is F3DG_ERR_UNSUPPORTED.
 * _emit: after a count that returned F3DG_OK with *h_kept > 0, same workspace and P; no host read. kept_ids [n_kept] int32: the kept
 * ids ascending; array k of n_arrays <= F3DG_COMPACT_MAX_ARRAYS (host arrays srcs, dsts, row_floats): dsts[k] [n_kept, row_floats[k]]
 * receives the kept rows of srcs[k] [P, row_floats[k]] (float32 rows; any 4-byte type gathers the same way) in input order. n_kept is
 * the capacity of the outputs: rows beyond it are not written. F3DG_ERR_BAD_ARG: n_arrays > F3DG_COMPACT_MAX_ARRAYS, a row width <= 0,
 * a null array, n_kept <= 0 or > P. On a workspace that holds no completed count of P elements nothing is written. */
#define F3DG_CONTRIBUTION_BYTES 32
#define F3DG_COMPACT_MAX_ARRAYS 8
int f3dg_contribution(void* stream, const void* workspace, size_t workspace_bytes, long long max_rendered, int n_views, int P, int W,
                      int H, float tan_fovx, float tan_fovy, void* stats, float* final_T);
size_t f3dg_gaussian_compact_workspace_bytes(long long P);
int f3dg_gaussian_compact_count(void* stream, void* workspace, size_t workspace_bytes, long long P, const void* stats,
                                const unsigned char* keep, long long min_touched, float min_max_weight, double min_sum_weight,
                                long long* h_kept);
int f3dg_gaussian_compact_emit(void* stream, const void* workspace, size_t workspace_bytes, long long P, long long n_kept, int n_arrays,
                               const void* const* srcs, void* const* dsts, const int* row_floats, int* kept_ids);

/* Runtime switches: process-wide DEFAULTS for what a call's own flags do not say (every arithmetic / list / path choice of a call has a
 * flag, above). The library knows sixteen names and one diagnostic pair; everything else returns F3DG_ERR_BAD_ARG.
 *   "render_fast"   (default 1) arithmetic of the compositing forward: 0 = the reference's float32 / float64 operation order, 1 = error-free
 *                   float32 pairs for the float64 island and FMA-contracted accumulations downstream of alpha in inference calls (no
 *                   auxiliary planes; within 3e-7 of mode 0), exact in calls a backward follows, 2 = fast in every call.
 *   "tile_cull"     (default 1) a Gaussian is instantiated only in the tiles that the box of its conservative alpha >= 1/255 ellipse reaches
 *                   instead of every tile of the reference's 3-sigma square (forward.cu:364-374). The dropped (Gaussian, tile) pairs are a
 *                   bare `continue` for every pixel of the tile: outputs and gradients are unchanged (asserted on every scene of the
 *                   tests); num_rendered and the exported lists are SHORTER than the reference's. 0 = the reference's lists, bit for bit.
 *                   f3dg_integrate always uses the reference's lists.
 *   "small_path"    (default 1) calls of one or two views of at most 2^18 Gaussians on at most 1,024 tiles take the three-launch path of
 *                   f3dg_small.hip (2 = on, and forget the shapes an earlier overflow disabled); "small_path_aux" (default 1): forwards
 *                   with F3DG_FLAG_SAVE_AUX too -- f3dg_backward then walks the per-tile slots.
 *   "render_lowocc" (default 1; n > 1: up to n x 1,024 quadrant waves) compositing launches of at most 2,048 quadrant waves (one or two
 *                   256^2 views: every wave alone on its SIMD, its time a chain of latencies) take the multi-wave kernels of
 *                   f3dg_render4.hip, bit-identical to the general kernel; 0 = the general kernel for every launch.
 *   "render_split"  (default -1: by arithmetic) those kernels: 1 = render3p_fwd_kernel, a producer wave scans the list, gathers the records
 *                   and runs phase 1 of the next window while the consumer wave composites (the default in fast arithmetic, and for two
 *                   views); 2 / 3 = render3q_fwd_kernel, consumer + 2 / 3 evaluator waves (the stateless part of every pair, parked in
 *                   LDS) + producer (3: the default for one view in the reference's arithmetic).
 *   "render_unroll" (default -1: 2 in fast arithmetic, else 1) entries per phase-2 trip of render3p (1 or 2).
 *   "render_pack"   (default -1) the rank-packed kernel (f3dg_render4.hip; bit-identical to render3s_fwd_kernel, also its auxiliary planes):
 *                   -1 = launches in the reference's arithmetic (-38 % on pixel-aligned predicted sets, -6 % at C2), 1 = every launch,
 *                   0 = none; "render_pack_th" (default 32; 0: none, 64: all): the trips of a slide in which at most that many pixels take
 *                   part are packed.
 *   "render_scan"   (default -1) the split-pixel schedule (f3dg_render5.hip): -1 = the calls that carry F3DG_FLAG_SCAN, 1 = every fast
 *                   inference launch of the general path, 0 = never; "render_scan_th" (default 12; 64: every pending entry goes through
 *                   dense batches): fused trips while more than that many pixels take part.
 *   "bwd_dense"     (default 1) the compositing backward: 1 = render5_bwd_kernel (f3dg_backward5.hip: entry-major batches of (pixel, entry) pairs,
 *                   segmented scans, one 128-byte accumulation record per (view, Gaussian)), 0 = render3_bwd_kernel (the lock-step walk of
 *                   rounds 2-5); "bwd_occ" (default 5): waves per SIMD the lock-step kernel is compiled for (2..6).
 *   "render_scan_min" (default 4) split-pixel mode: stragglers that hold fewer older-half entries than this finish the slide in fused trips.
 *   diagnostics: "render_count" (default 0) swaps in the counting variants of the compositing kernels (f3dg_debug_render_counts /
 *                   _render4_counts / _render5_counts); "time_launches" (default 0): f3dg_debug_launch_times; "reference_kernels"
 *                   (default 0) 1 = the compositing forward and pass 1 of f3dg_integrate take the plain transcriptions of the reference
 *                   (render_fwd_kernel, integrate_pass1_kernel: every pixel visits every entry of its tile's list, nothing is filtered) in
 *                   the reference's arithmetic whatever the call's flags say, and no call takes the small-call path. The baseline the
 *                   tests hold every other compositing path to, bit for bit; slow. (integrate_pass1_kernel is also what the default path
 *                   runs on the tiles f3dg_debug_integrate_redo counts.)
 * Any other name is F3DG_ERR_BAD_ARG, among them the switches of the kernel generations that were measured and retired (NOTES.md has
 * their measurements). */
int f3dg_set_option(const char* name, int value);

/* Diagnostic: number of kernels this library has launched from this process since the last reset (host-side counter, every
 * launch site counts; memsets / copies do not). bench.py reports launches per call from it. */
long long f3dg_debug_launch_count(int reset);
/* Diagnostic: with option "time_launches" = 1 every launch site measures the host time of its hipLaunchKernelGGL; this prints the
 * per-site averages to stderr (tools/prof_small.py). */
int f3dg_debug_launch_times(int reset);

/* Optional per-stage timing of the forward path with HIP events recorded on the caller's stream (this is what
 * bench.py uses for the live roofline figure). f3dg_profile_enable(1) makes every following
 * f3dg_forward_batched on this host thread record 4 events; f3dg_profile_collect() is BLOCKING, sums the
 * milliseconds of all calls recorded since the last collect into h_stage_ms[3] = {projection (preprocess),
 * binning (scan + key duplication + radix sort + tile ranges), compositing} and returns the call count; h_stage_ms holds FIVE
 * doubles: [3] and [4] are the compositing backward and the per-Gaussian backward of the f3dg_backward calls in between. */
int f3dg_profile_enable(int on);
int f3dg_profile_collect(double* h_stage_ms, int* h_calls);
/* The same, plus the three forward stage times of every recorded call in call order: h_per_call[max_calls][3] (may be NULL). */
int f3dg_profile_collect_calls(double* h_stage_ms, int* h_calls, double* h_per_call, int max_calls);
/* Diagnostics of the compositing forward: the kernel (with its template arguments) the last launch of this process used, and -- with
 * f3dg_set_option("render_count", 1), which swaps in a counting variant of the one-wave kernel -- its work counters summed over the
 * launches since the last reset: h_out8[SIXTEEN] = { list entries staged, list entries scanned, phase-2 trips, slides, lane-trips, waves,
 * trips of slides that began with <= 8 / <= 24 live pixels, those slides, 0 ... }. */
const char* f3dg_debug_last_render_kernel(void);
int f3dg_debug_render_counts(unsigned long long* h_out8, int reset);
/* The counters of the rank-packed kernel's counting variant (render_pack with render_count = 1): h_out[SIXTEEN] = { list entries
 * staged, scanned, fused trips, slides, lane-trips of fused trips, waves, packed batches (= dense trips), blend trips of the batches,
 * pairs evaluated in dense trips, pairs that reached a blend trip, 0 ... }. */
int f3dg_debug_render4_counts(unsigned long long* h_out, int reset);
/* The same for render5_fwd_kernel (F3DG_FLAG_SCAN): h_out[16] = { staged, scanned, fused trips, slides, lane-trips of fused trips, waves,
 * dense batches, pairs in dense batches, pixels compacted, slides with a compaction, 0... }. */
int f3dg_debug_render5_counts(unsigned long long* h_out, int reset);
/* Debug: shader clocks of the roles of the small-launch pipeline kernel (render3q_fwd_kernel, options render_split = 2 / 3 and
 * render_count = 1), summed over the launches since the last reset of f3dg_debug_render4_counts. h_out[4][16]: rows { consumer,
 * evaluators, producer } x { total, waiting at the window barrier, waiting for a round counter, windows, rounds, waves }; row 3 =
 * the longest { consumer, evaluator, producer } wave of any workgroup. */
int f3dg_debug_render3q_clocks(unsigned long long* h_out);

/* BLOCKING: number of contributing (pixel, Gaussian) pairs the last f3dg_backward on this workspace blended back through --
 * "C" of the byte formula 80 R + 60 W H + 68 C of the compositing backward. */
int f3dg_backward_pairs(void* stream, const void* workspace, long long* h_pairs);

/* Test/inspection hook: device-to-device copies of the library's internal per-call state into caller buffers
 * (any pointer may be NULL). Used by the stage-wise parity tests to pin each kernel separately, the way the
 * oracle exposes GeometryState / BinningState / ImageState (rasterizer_impl.cu:188-243).
 *   rec [V*P*16] (view2gaussian[10], opacity*coef, pre-test threshold, rgb[3], culling-ellipse c; after an INFERENCE call only the rows of
 *   (view, Gaussian) pairs that are in a tile list are written -- the others are stale); depths [V*P], means2D [V*P*2], conic [V*P*4],
 *   tiles [V*P], offsets [V*P], clamped [V*P] (bit c = channel c clamped), keys_sorted [cap] u64 (all SAVE_AUX: an inference call does not write them),
 *   point_list [cap], ranges [V*T*2], final_T [V*4*H*W] and n_contrib [V*2*H*W] (SAVE_AUX).
 * Asking for a SAVE_AUX-only plane of a workspace whose last forward was an inference call returns F3DG_ERR_BAD_ARG (BLOCKING then:
 * the header is read back); rec, point_list (Gaussian ids, quadrant masks stripped) and ranges are always available. */
int f3dg_debug_export(void* stream, const void* workspace, int P, int W, int H, int n_views,
                      long long max_rendered, float* rec, float* means2D, float* conic, unsigned* tiles,
                      unsigned* offsets, unsigned char* clamped, unsigned long long* keys_sorted,
                      unsigned* point_list, unsigned* ranges, float* final_T, unsigned* n_contrib, float* depths);

/* Test/inspection hook, BLOCKING: the projection's own conservative culling data of the last forward on this workspace, copied to device
 * buffers of the caller (any pointer may be NULL). Same shape arguments as f3dg_debug_export.
 *   cull [V*P*4]   the conservative alpha >= 1/255 ellipse (cx, cy, a, b) in pixel-index coordinates; its c is slot 15 of `rec`, the
 *                  pre-test constant K slot 11. "everything" is a = b = c = 0; "never" is the centre (-1e9, -1e9) with a = c = 1e30.
 *                  A SAVE_AUX call writes this plane and the record for every pair; an INFERENCE call writes them only for the (view,
 *                  Gaussian) pairs that are in a tile list -- the other rows hold whatever the workspace held before.
 *   rects [V*P*2]  the tile rectangle (min | max << 16 per axis, 15-bit tile coordinates, max exclusive; 0, 0: in no tile) after tile
 *                  culling, with the half-tile hints F3DG_RECT_SKIP_LO (bit 15) / F3DG_RECT_SKIP_HI (bit 31) of each word. ALWAYS written,
 *                  for every pair, by every call.
 *   chunk_boxes [V*ceil(P/64)*2]  small-call path only: the union of the rectangles of each 64 consecutive Gaussians, hint bits
 *                  stripped ("everything", 0 | 0x7FFF << 16, for a view's last partial chunk). Asking for it on a workspace whose last
 *                  forward did not take the small-call path returns F3DG_ERR_STATE. */
int f3dg_debug_export_cull(void* stream, const void* workspace, int P, int W, int H, int n_views, long long max_rendered,
                           float* cull, unsigned* rects, unsigned* chunk_boxes);

/* Kept for callers of earlier versions: h_out8[8] was the phase timing of an instrumented compositing kernel. No kernel is
 * instrumented any more: it returns zeros. */
int f3dg_debug_timing(unsigned long long* h_out8, int reset);

#ifdef __cplusplus
}
#endif
#endif /* F3DG_H_INCLUDED */
