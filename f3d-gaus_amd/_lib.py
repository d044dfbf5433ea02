"""ctypes binding of libf3dg_hip.so (include/f3dg.h). The product path has NO fallback: if the HIP library is
missing or fails to load, importing a function from here raises; nothing under this package touches ``oracle/``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libf3dg_hip.so")

OK, ERR_BAD_ARG, ERR_WORKSPACE, ERR_OVERFLOW, ERR_HIP, ERR_UNSUPPORTED, ERR_STATE = 0, -1, -2, -3, -4, -5, -6
FLAG_SAVE_AUX, FLAG_BG_PER_VIEW, FLAG_SKIP_NORMAL, FLAG_SKIP_DISTORTION = 1, 2, 4, 8
FLAG_EXACT, FLAG_FAST, FLAG_NO_TILE_CULL, FLAG_NO_SMALL_PATH, FLAG_SCAN, FLAG_SETS_AUX = 16, 32, 64, 128, 256, 512
PENDING = 1
GEOM_ALPHA_WEIGHT = 1
MAX_PANELS, PANEL_RGB, PANEL_SIGNED, PANEL_COLORMAP = 8, 0, 1, 2
TSDF_MAX_VIEWS = 128
RASTER_CULL = {"none": 0, "back": 1, "front": 2}
BAKE_MODE = {"blend": 0, "best": 1}
SIMPLIFY_PLACEMENT = {"root": 0, "mean": 1, "quadric": 2}
SIMPLIFY_COUNTS = ("clusters", "used_clusters", "degenerate", "collapsed", "duplicate", "kept", "max_cluster")
SIMPLIFY_MAX_ATTRS = 64
BAKE_COUNTS = ("near", "outside", "uncovered", "occluded", "grazing", "masked", "used", "vertices_seen")


class Panel(C.Structure):
    """f3dg_panel of include/f3dg.h (strides in floats)."""
    _fields_ = [("src", C.c_void_p), ("image_stride", C.c_size_t), ("frame_stride", C.c_size_t), ("plane_stride", C.c_size_t),
                ("kind", C.c_int), ("planes", C.c_int), ("range_index", C.c_int)]


_ERR_TEXT = {
    ERR_BAD_ARG: "bad argument",
    ERR_WORKSPACE: "workspace smaller than f3dg_workspace_bytes()",
    ERR_OVERFLOW: "instance capacity (max_rendered) exceeded",
    ERR_HIP: "HIP runtime error",
    ERR_UNSUPPORTED: "unsupported configuration",
    ERR_STATE: "backward on a workspace whose last forward kept no auxiliary planes (not a save_aux call of the general path)",
}

_p, _i, _f, _ll, _sz, _u = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_size_t, C.c_uint

# name -> (restype, argtypes); must list every symbol include/f3dg.h declares (tests/test_abi.py checks both ways)
SIGNATURES = {
    "f3dg_version": (C.c_char_p, []),
    "f3dg_last_error": (C.c_char_p, []),
    "f3dg_workspace_bytes": (_sz, [_i, _i, _i, _i, _ll]),
    "f3dg_forward_batched": (_i, [_p, _p, _sz, _ll, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p,
                                  _p, _p, _p, _f, _f, _f, _p, _p, _u]),
    "f3dg_forward_sets": (_i, [_p, _p, _sz, _ll, _i, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p,
                               _p, _p, _p, _f, _f, _f, _p, _p, _u]),
    "f3dg_read_status": (_i, [_p, _p, C.POINTER(_ll)]),
    "f3dg_status_post": (_i, [_p, _p]),
    "f3dg_status_poll": (_i, [_i, _i, C.POINTER(_ll)]),
    "f3dg_forward": (_ll, [_p, _p, _sz, _ll, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p,
                           _f, _f, _f, _i, _p, _p, _u, C.POINTER(_ll)]),
    "f3dg_backward": (_i, [_p, _p, _sz, _ll, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p,
                           _f, _f, _f, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _u]),
    # as f3dg_backward with (n_sets, views_per_set) in place of n_views
    "f3dg_backward_sets": (_i, [_p, _p, _sz, _ll, _i, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p,
                                _f, _f, _f, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _u]),
    "f3dg_integrate_workspace_bytes": (_sz, [_i, _i, _i, _i, _ll]),
    # stream, ws, ws_bytes, cap | PN P D M | bg W H | points3D means3D shs colors opac scales | mod | rot cov3D v2g view
    # proj campos | tanx tany ks | subpix | prefiltered | out_color radii alpha_i color_i | h_needed
    "f3dg_integrate": (_ll, [_p, _p, _sz, _ll, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p,
                             _p, _p, _f, _f, _f, _p, _i, _p, _p, _p, _p, C.POINTER(_ll)]),
    "f3dg_integrate_prepare": (_ll, [_p, _p, _sz, _ll, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p,
                                     _p, _f, _f, _f, _p, _p, C.POINTER(_ll)]),
    "f3dg_integrate_points": (_i, [_p, _p, _sz, _ll, _i, _i, _i, _i, _p, _p, _f, _f, _p, _p, _p, _p]),
    "f3dg_integrate_workspace_bytes_batched": (_sz, [_i, _i, _i, _i, _i, _ll]),
    "f3dg_integrate_prepare_batched": (_ll, [_p, _p, _sz, _ll, _i, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p,
                                             _p, _f, _f, _f, _p, _p, C.POINTER(_ll)]),
    "f3dg_integrate_points_view": (_i, [_p, _p, _sz, _ll, _i, _i, _i, _i, _i, _i, _p, _p, _f, _f, _p, _p, _p, _p]),
    "f3dg_debug_integrate_redo": (_i, [_p, _p, _i, _i, _i, _i, _i, _ll, C.POINTER(_i)]),
    "f3dg_debug_integrate_export": (_i, [_p, _p, _i, _i, _i, _i, _i, _ll, _i, _p, _p, _p, _p]),
    "f3dg_mark_visible": (_i, [_p, _i, _p, _p, _p, _p]),
    # stream ws ws_bytes | N F max_edges | sdf tets tets_int32 | h_counts[4]   /   ... | tets tets_int32 n_one | interp_v faces
    "f3dg_marching_tets_workspace_bytes": (_sz, [_ll, _ll, _ll]),
    "f3dg_marching_tets_count": (_i, [_p, _p, _sz, _ll, _ll, _ll, _p, _p, _i, C.POINTER(_ll)]),
    "f3dg_marching_tets_emit": (_i, [_p, _p, _sz, _ll, _ll, _ll, _p, _i, _ll, _p, _p]),
    "f3dg_splat_head": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _f, _ll, _ll, _p, _p, _p, _p, _p, _p, _p]),
    "f3dg_splat_head_backward": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _f, _ll, _ll, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "f3dg_render_epilogue": (_i, [_p, _i, _i, _i, _p, _p, _f, _f, _p, _p]),
    "f3dg_render_epilogue_view": (_i, [_p, _i, _i, _i, _p, _p, _f, _f, _p, _p]),
    "f3dg_render_epilogue_backward": (_i, [_p, _i, _i, _i, _p, _p, _f, _f, _p, _p, _p]),
    "f3dg_cycle_inputs": (_i, [_p, _i, _i, _i, _i, _p, _p, _p]),
    "f3dg_cycle_inputs_backward": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "f3dg_pack_frames": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "f3dg_pack_frames_host": (_i, [_p, _i, _i, _i, _i, _p, _p, _i]),
    # stream | n_frames n_images H W nrow padding n_panels | panels (host, Panel[]) lut ranges invalid_val | dst dst_is_host max_workgroups
    "f3dg_compose_frames": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _f, _p, _i, _i]),
    "f3dg_compose_frames_size": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_sz)]),
    # the backbone between the convolutions: stream dtype nhwc N C HW (groups) | ...
    "f3dg_group_norm_silu_forward": (_i, [_p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _f, _i, _p, _p, _p, _sz]),
    "f3dg_group_norm_silu_forward_stats": (_i, [_p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _f, _i, _p, _p, _p, _sz]),
    "f3dg_residual_join_forward": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _f, _p]),
    "f3dg_group_norm_nhwc_scratch_bytes": (C.c_size_t, [_i, _i, _i]),
    # training through the backbone: the adjoints (stream N C HW groups nhwc | ...)
    "f3dg_group_norm_silu_backward_scratch_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "f3dg_group_norm_silu_backward": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _sz]),
    "f3dg_group_norm_silu_backward_dtype": (_i, [_p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _sz]),
    "f3dg_residual_join_backward_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "f3dg_residual_join_backward": (_i, [_p, _i, _i, _i, _i, _p, _f, _p, _p, _p, _sz]),
    "f3dg_residual_join_backward_dtype": (_i, [_p, _i, _i, _i, _i, _i, _p, _f, _p, _p, _p, _sz]),
    # n_planes W H  /  stream | n_planes W H | img1 img2 | map dm_dmu1 dm_dsigma1_sq dm_dsigma12 | partials partials_bytes plane_sums
    "f3dg_ssim_partials_bytes": (_sz, [_i, _i, _i]),
    "f3dg_ssim_forward": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    # stream | n_planes W H | img1 img2 | dL_dmap plane_weights | dm_dmu1 dm_dsigma1_sq dm_dsigma12 | dL_dimg1
    "f3dg_ssim_backward": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
    # n_frames W H  /  stream | n_frames H W | raster world_view fx fy flags | depth_target normal_target alpha_target mask | ...
    "f3dg_geometry_loss_partials_bytes": (_sz, [_i, _i, _i]),
    "f3dg_geometry_loss_forward": (_i, [_p, _i, _i, _i, _p, _p, _f, _f, _i, _p, _p, _p, _p, _p, _sz, _p]),      # partials partials_bytes frame_sums
    "f3dg_geometry_loss_backward": (_i, [_p, _i, _i, _i, _p, _p, _f, _f, _i, _p, _p, _p, _p, _p, _p]),          # frame_weights dL_draster
    # n_src n_views C W H  /  stream | n_src n_views C H W | image depth valid rel | fx fy z_near depth_tolerance occlusion_min_weight threshold
    # | erode | workspace workspace_bytes | warped mask warped_depth weight
    "f3dg_forward_warp_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "f3dg_forward_warp": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _f, _f, _f, _f, _f, _f, _i, _p, _sz, _p, _p, _p, _p]),
    # n_frames C W H  /  stream | n_frames C H W | a b mask | partials partials_bytes frame_sums  /  ... | frame_weights dL_da
    "f3dg_masked_l1_partials_bytes": (_sz, [_i, _i, _i, _i]),
    "f3dg_masked_l1_forward": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _sz, _p]),
    "f3dg_masked_l1_backward": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    # stream | nx ny nz origin(host [3]) voxel trunc z_near | n_views H W | depth color alpha alpha_min world_view fx fy | tsdf weight color color_weight
    "f3dg_tsdf_integrate": (_i, [_p, _i, _i, _i, C.POINTER(_f), _f, _f, _f, _i, _i, _i, _p, _p, _p, _f, _p, _f, _f, _p, _p, _p, _p]),
    # nx ny nz  /  stream | nx ny nz | min_weight tsdf weight | workspace workspace_bytes h_n_active  /  ... | workspace workspace_bytes n_active tets
    "f3dg_tsdf_cells_workspace_bytes": (_sz, [_i, _i, _i]),
    "f3dg_tsdf_cells_count": (_i, [_p, _i, _i, _i, _f, _p, _p, _p, _sz, C.POINTER(_ll)]),
    "f3dg_tsdf_cells_emit": (_i, [_p, _i, _i, _i, _p, _sz, _ll, _p]),
    # stream | nx ny nz origin(host [3]) voxel | E interp_v | tsdf color color_weight | vertices vertex_colors
    "f3dg_tsdf_vertices": (_i, [_p, _i, _i, _i, C.POINTER(_f), _f, _ll, _p, _p, _p, _p, _p, _p]),
    # N F  /  stream ws ws_bytes | N F faces faces_int32 | face_component component_faces h_counts[4]
    "f3dg_mesh_components_workspace_bytes": (_sz, [_ll, _ll]),
    "f3dg_mesh_components": (_i, [_p, _p, _sz, _ll, _ll, _p, _i, _p, _p, C.POINTER(_ll)]),
    # N F  /  stream ws ws_bytes | N F faces faces_int32 face_component keep_root | h_counts[2]  /  ... | n_faces_kept n_vertices_kept faces_out vertex_ids
    "f3dg_mesh_compact_workspace_bytes": (_sz, [_ll, _ll]),
    "f3dg_mesh_compact_count": (_i, [_p, _p, _sz, _ll, _ll, _p, _i, _p, _p, C.POINTER(_ll)]),
    "f3dg_mesh_compact_emit": (_i, [_p, _p, _sz, _ll, _ll, _p, _i, _p, _p, _ll, _ll, _p, _p]),
    # N F  /  stream ws ws_bytes | N F faces faces_int32 | nbr_start nbr boundary h_counts[4]
    "f3dg_mesh_adjacency_workspace_bytes": (_sz, [_ll, _ll]),
    "f3dg_mesh_adjacency": (_i, [_p, _p, _sz, _ll, _ll, _p, _i, _p, _p, _p, C.POINTER(_ll)]),
    # stream | N nbr_start nbr pinned | vertices_in lambda mu iterations | scratch vertices_out
    "f3dg_mesh_smooth": (_i, [_p, _ll, _p, _p, _p, _p, _f, _f, _i, _p, _p]),
    # stream ws ws_bytes | N F faces faces_int32 | vertices normals
    "f3dg_mesh_vertex_normals": (_i, [_p, _p, _sz, _ll, _ll, _p, _i, _p, _p]),
    # N F  /  stream ws ws_bytes | N F vertices faces faces_int32 | origin(host [3] float64) cell | h_counts[8]
    # /  ... faces_int32 | placement C attrs adj_ws adj_ws_bytes | n_vertices_out n_faces_out | vertices_out faces_out attrs_out vertex_map cluster_root cluster_size
    "f3dg_mesh_simplify_workspace_bytes": (_sz, [_ll, _ll]),
    "f3dg_mesh_simplify_count": (_i, [_p, _p, _sz, _ll, _ll, _p, _p, _i, C.POINTER(C.c_double), C.c_double, C.POINTER(_ll)]),
    "f3dg_mesh_simplify_emit": (_i, [_p, _p, _sz, _ll, _ll, _p, _p, _i, _i, _i, _p, _p, _sz, _ll, _ll, _p, _p, _p, _p, _p, _p]),
    # V F H W  /  stream ws ws_bytes | N F vertices faces faces_int32 | V world_views fx fy H W z_near cull | C attrs | face_id depth bary attrs_out | h_counts[7]
    "f3dg_mesh_raster_workspace_bytes": (_sz, [_ll, _ll, _ll, _ll]),
    "f3dg_mesh_raster": (_i, [_p, _p, _sz, _ll, _ll, _p, _p, _i, _i, _p, C.c_double, C.c_double, _i, _i, C.c_double, _i, _i, _p, _p, _p, _p, _p,
                              C.POINTER(_ll)]),
    # V N H W  /  stream ws ws_bytes | N vertices normals | V world_views fx fy H W z_near | C images face_id depth alpha alpha_min |
    # depth_tol cos_min mode | colors weight n_used best_view | h_counts[8]
    "f3dg_mesh_bake_workspace_bytes": (_sz, [_ll, _ll, _ll, _ll]),
    "f3dg_mesh_bake_colors": (_i, [_p, _p, _sz, _ll, _p, _p, _ll, _p, C.c_double, C.c_double, _ll, _ll, C.c_double, _i, _p, _p, _p, _p,
                                   C.c_double, C.c_double, C.c_double, _i, _p, _p, _p, _p, C.POINTER(_ll)]),
    # stream ws ws_bytes cap | n_views P W H tanx tany | stats final_T
    "f3dg_contribution": (_i, [_p, _p, _sz, _ll, _i, _i, _i, _i, _f, _f, _p, _p]),
    # P  /  stream ws ws_bytes P | stats keep min_touched min_max_weight min_sum_weight | h_kept  /  ... P n_kept | n_arrays srcs dsts row_floats (host) | kept_ids
    "f3dg_gaussian_compact_workspace_bytes": (_sz, [_ll]),
    "f3dg_gaussian_compact_count": (_i, [_p, _p, _sz, _ll, _p, _p, _ll, _f, C.c_double, C.POINTER(_ll)]),
    "f3dg_gaussian_compact_emit": (_i, [_p, _p, _sz, _ll, _ll, _i, C.POINTER(_p), C.POINTER(_p), C.POINTER(_i), _p]),
    "f3dg_set_option": (_i, [C.c_char_p, _i]),
    "f3dg_profile_enable": (_i, [_i]),
    "f3dg_debug_launch_count": (C.c_longlong, [_i]),
    "f3dg_debug_launch_times": (_i, [_i]),
    "f3dg_profile_collect": (_i, [C.POINTER(C.c_double), C.POINTER(_i)]),
    "f3dg_profile_collect_calls": (_i, [C.POINTER(C.c_double), C.POINTER(_i), C.POINTER(C.c_double), _i]),
    "f3dg_debug_last_render_kernel": (C.c_char_p, []),
    "f3dg_debug_render_counts": (_i, [C.POINTER(C.c_ulonglong), _i]),
    "f3dg_debug_render4_counts": (_i, [C.POINTER(C.c_ulonglong), _i]),
    "f3dg_debug_render5_counts": (_i, [C.POINTER(C.c_ulonglong), _i]),
    "f3dg_debug_render3q_clocks": (_i, [C.POINTER(C.c_ulonglong)]),
    "f3dg_backward_pairs": (_i, [_p, _p, C.POINTER(_ll)]),
    "f3dg_debug_timing": (_i, [C.POINTER(C.c_ulonglong), _i]),
    "f3dg_debug_export": (_i, [_p, _p, _i, _i, _i, _i, _ll, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    # stream ws | P W H n_views cap | cull rects chunk_boxes
    "f3dg_debug_export_cull": (_i, [_p, _p, _i, _i, _i, _i, _ll, _p, _p, _p]),
}

_LIB = None


class F3dgError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        detail = ""
        try:
            detail = lib().f3dg_last_error().decode()
        except Exception:
            pass
        super().__init__(f"{where}: {_ERR_TEXT.get(code, 'error')} (code {code})" + (f": {detail}" if detail and code == ERR_HIP else ""))


def lib():
    """Load (once) and return the ctypes handle. Raises if the HIP extension is not built -- loudly, by design."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
                "There is no CPU or PyTorch fallback for the rasterization path.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)       # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(code, where):
    if code < 0:
        raise F3dgError(int(code), where)
    return code


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL; empty tensor -> NULL, as the reference maps empty to nullptr)."""
    if t is None or t.numel() == 0:
        return None
    return C.c_void_p(t.data_ptr())
