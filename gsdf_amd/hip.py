"""ctypes face of libgsdfhip.so (include/gsdf_hip.h): the MI355X HIP backend.

Mirrors the reference seam: `SDF3HIP` stands where `gleval.SDF3Compute` does (gleval/gpu.go:56-103:
Evaluate / Bounds / Evaluations, same error behaviour), `OctreeHIP` where `glrender.Octree` does
(glrender/octreerenderer.go: ReadTriangles iterator + RenderAll), `write_binary_stl` where
`glrender.WriteBinarySTL` does. There is NO CPU fallback: if the HIP library or a GPU is missing,
construction raises.
"""
import ctypes as C
import os
import numpy as np

from ._ctypes_common import GsdfTree

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgsdfhip.so")
_LIB = None

ErrEmptyBuffers = "empty buffers"
ErrMismatchBufferLength = "position and distance buffer length mismatch"

# every symbol include/gsdf_hip.h declares
SYMBOLS = ["gsdf_hip_last_error", "gsdf_hip_init", "gsdf_hip_program_create", "gsdf_hip_program_destroy",
           "gsdf_hip_program_bounds", "gsdf_hip_program_is2d", "gsdf_hip_program_info", "gsdf_hip_evaluations", "gsdf_hip_lower", "gsdf_hip_lower_region", "gsdf_hip_eval3_submit", "gsdf_hip_eval_wait", "gsdf_hip_host_alloc", "gsdf_hip_host_register", "gsdf_hip_host_release", "gsdf_hip_comm_unique_id", "gsdf_hip_comm_create", "gsdf_hip_comm_rank", "gsdf_hip_comm_world", "gsdf_hip_comm_allreduce_sum_u64", "gsdf_hip_mesh_gatherv", "gsdf_hip_mesh_gatherv_start", "gsdf_hip_mesh_gatherv_wait", "gsdf_hip_comm_destroy", "gsdf_hip_selftest_div", "gsdf_hip_selftest_sqrt", "gsdf_hip_selftest_circ", "gsdf_hip_selftest_atan2", "gsdf_hip_selftest_cossin", "gsdf_hip_selftest_math", "gsdf_hip_grid_cus", "gsdf_hip_mesh_minecraft", "gsdf_hip_blockcache_create", "gsdf_hip_blockcache_reset", "gsdf_hip_blockcache_eval3", "gsdf_hip_blockcache_hits", "gsdf_hip_blockcache_evaluations", "gsdf_hip_blockcache_destroy", "gsdf_hip_program_specialize", "gsdf_hip_program_specialize_async", "gsdf_hip_program_specialize_poll", "gsdf_hip_program_is_specialized", "gsdf_hip_program_kernels", "gsdf_hip_specialize_source", "gsdf_hip_specialize_check",
           "gsdf_hip_eval3", "gsdf_hip_eval2", "gsdf_hip_eval3_dev", "gsdf_hip_eval2_dev", "gsdf_hip_normals3", "gsdf_hip_image2", "gsdf_hip_image2_color", "gsdf_hip_picture_size", "gsdf_hip_color_iq", "gsdf_hip_color_gradient", "gsdf_hip_view_orbit", "gsdf_hip_render3",
           "gsdf_hip_mesh_octree", "gsdf_hip_mesh_dualcontour", "gsdf_hip_mesh_flat", "gsdf_hip_mesh_stats_get", "gsdf_hip_mesh_read", "gsdf_hip_mesh_dev_tris",
           "gsdf_hip_mesh_stl", "gsdf_hip_mesh_host_tris", "gsdf_hip_mesh_host_stl", "gsdf_hip_mesh_destroy", "gsdf_hip_brick_owner", "gsdf_hip_slab_range",
           "gsdf_hip_mesh_payload", "gsdf_hip_mesh_march", "gsdf_hip_mesh_stage_ms", "gsdf_hip_mesh_octree_start", "gsdf_hip_mesh_octree_wait", "gsdf_hip_comm_transport", "gsdf_hip_gather_plan",
           "gsdf_hip_mesh_read_records", "gsdf_hip_mesh_weld", "gsdf_hip_indexed_counts", "gsdf_hip_indexed_stats_get", "gsdf_hip_indexed_read",
           "gsdf_hip_indexed_normals", "gsdf_hip_indexed_read_normals", "gsdf_hip_indexed_ply", "gsdf_hip_indexed_host_ply", "gsdf_hip_indexed_destroy",
           "gsdf_hip_indexed_create", "gsdf_hip_indexed_report", "gsdf_hip_indexed_shells", "gsdf_hip_indexed_read_shell_of", "gsdf_hip_indexed_extract",
           "gsdf_hip_indexed_simplify", "gsdf_hip_indexed_simplify_adaptive", "gsdf_hip_indexed_clean", "gsdf_hip_indexed_project", "gsdf_hip_indexed_read_fit", "gsdf_hip_mesh_dualcontour_indexed",
           "gsdf_hip_raycast3", "gsdf_hip_indexed_thickness",
           "gsdf_hip_contour2", "gsdf_hip_slice3", "gsdf_hip_contour_counts", "gsdf_hip_contour_read", "gsdf_hip_contour_stats_get", "gsdf_hip_contour_destroy",
           "gsdf_hip_contour_create", "gsdf_hip_contour_simplify", "gsdf_hip_contour_measures", "gsdf_hip_contour_measures_ms",
           "gsdf_hip_indexed_mass", "gsdf_hip_indexed_mass_ms", "gsdf_hip_inertia_principal", "gsdf_hip_contour_sections", "gsdf_hip_contour_sections_ms",
           "gsdf_hip_contour_hatch", "gsdf_hip_hatch_counts", "gsdf_hip_hatch_read", "gsdf_hip_hatch_rank_ms", "gsdf_hip_hatch_destroy",
           "gsdf_hip_contour_hatch_skin", "gsdf_hip_hatch_read_skin", "gsdf_hip_skin_rank_ms", "gsdf_hip_contour_offset", "gsdf_hip_contour_distance"]


PRUNE_ASSUME_SDF = 1 << 30  # gsdf_hip.h: GSDF_PRUNE_ASSUME_SDF


GATHER_ALL, GATHER_ROOT, GATHER_NONE = 0, 1, 2  # gsdf_hip.h
PAYLOAD_TRIANGLES, PAYLOAD_RECORDS = 0, 1            # gsdf_hip.h: gsdf_mesh_opts.payload
GOP_COPY, GOP_SEND, GOP_RECV = 0, 1, 2               # gsdf_hip.h: gsdf_gather_op.kind


class GatherOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("peer", C.c_int32), ("src_off", C.c_uint64), ("dst_off", C.c_uint64), ("bytes", C.c_uint64)]


class GatherStats(C.Structure):
    _fields_ = [("ms_counts", C.c_double), ("ms_payload", C.c_double), ("bytes_sent", C.c_uint64), ("bytes_received", C.c_uint64),
                ("ms_march", C.c_double)]


class MeshOpts(C.Structure):
    _fields_ = [("prune", C.c_int), ("shard_rank", C.c_int), ("shard_count", C.c_int), ("max_tris", C.c_uint64),
                ("stream", C.c_void_p), ("share_corners", C.c_int), ("host_output", C.c_int), ("payload", C.c_int), ("reserved", C.c_int)]


class GsdfView(C.Structure):
    """gsdf_view (gsdf_hip.h): the camera of one UI frame (gsdfaux/ui.go:276-297) and its sampling."""
    _fields_ = [("ro", C.c_float * 3), ("uu", C.c_float * 3), ("vv", C.c_float * 3), ("ww", C.c_float * 3), ("char_dist", C.c_float),
                ("aa", C.c_int32), ("max_steps", C.c_int32), ("reserved", C.c_int32)]


class GsdfColor2(C.Structure):
    """gsdf_color2 (gsdf_hip.h): one of gsdfaux's colour conversions of a distance (gsdfaux/color.go)."""
    _fields_ = [("kind", C.c_int32), ("length", C.c_float), ("c0", C.c_uint8 * 4), ("c1", C.c_uint8 * 4), ("reserved", C.c_int32 * 4)]


COLOR_DEFAULT, COLOR_IQ, COLOR_GRADIENT, COLOR_BW_SMOOTH = 0, 1, 2, 3


class MeshStats(C.Structure):
    _fields_ = [("n_tris", C.c_uint64), ("evals", C.c_uint64), ("pruned_leaves", C.c_uint64), ("leaf_cubes", C.c_uint64),
                ("active_leaves", C.c_uint64), ("levels", C.c_int), ("origin", C.c_float * 3), ("res", C.c_float),
                ("ms_total", C.c_double), ("ms_prune", C.c_double), ("ms_leaf", C.c_double), ("ms_march", C.c_double),
                ("evals_prune", C.c_uint64), ("evals_leaf", C.c_uint64), ("ms_emit", C.c_double), ("cut_leaves", C.c_uint64)]


class IndexedStats(C.Structure):
    """gsdf_indexed_stats (gsdf_hip.h): device times of a weld's stages and its hash table's figures."""
    _fields_ = [("ms_keys", C.c_double), ("ms_insert", C.c_double), ("ms_number", C.c_double), ("ms_ply", C.c_double),
                ("probes", C.c_uint64), ("table_cells", C.c_uint64), ("attempts", C.c_int32), ("has_normals", C.c_int32)]


class IndexedReport(C.Structure):
    """gsdf_indexed_report (gsdf_hip.h): counts, edge classes, shells and measures of an indexed mesh; bytes 0 .. 159 (RESULT_BYTES)
    are a function of the mesh alone, the rest says what the run cost."""
    _fields_ = [("n_verts", C.c_uint64), ("n_tris", C.c_uint64), ("degenerate", C.c_uint64), ("nonfinite", C.c_uint64), ("used_verts", C.c_uint64),
                ("edges", C.c_uint64), ("boundary_edges", C.c_uint64), ("nonmanifold_edges", C.c_uint64), ("misoriented_edges", C.c_uint64),
                ("n_shells", C.c_uint64), ("euler", C.c_int64), ("area", C.c_double), ("volume", C.c_double), ("centroid", C.c_double * 3),
                ("bbox", C.c_float * 6), ("closed_oriented", C.c_int32), ("exponent", C.c_int32),
                ("ms_edges", C.c_double), ("ms_shells", C.c_double), ("ms_measure", C.c_double), ("probes", C.c_uint64), ("table_cells", C.c_uint64),
                ("attempts", C.c_int32), ("reserved", C.c_int32)]
    RESULT_BYTES = 160

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


class SimplifyOpts(C.Structure):
    """gsdf_simplify_opts (gsdf_hip.h): the clustering grid's cell edge and origin."""
    _fields_ = [("cell", C.c_float), ("origin", C.c_float * 3), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class SimplifyStats(C.Structure):
    """gsdf_simplify_stats (gsdf_hip.h): what a simplification by vertex clustering did; bytes 0 .. 79 (RESULT_BYTES) are a function of
    the mesh and the options alone, the rest says what the run cost."""
    _fields_ = [("n_verts_in", C.c_uint64), ("n_tris_in", C.c_uint64), ("used_verts_in", C.c_uint64), ("degenerate_in", C.c_uint64),
                ("cells", C.c_uint64), ("collapsed", C.c_uint64), ("n_verts", C.c_uint64), ("n_tris", C.c_uint64), ("largest_cell", C.c_uint64),
                ("exponent", C.c_int32), ("reserved", C.c_int32),
                ("ms_cells", C.c_double), ("ms_faces", C.c_double), ("probes", C.c_uint64), ("table_cells", C.c_uint64),
                ("attempts", C.c_int32), ("reserved2", C.c_int32)]
    RESULT_BYTES = 80

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


class AdaptiveOpts(C.Structure):
    """gsdf_adaptive_opts (gsdf_hip.h): the finest cell's edge, the grids' origin, the error a cluster may have, the number of nested grids."""
    _fields_ = [("cell", C.c_float), ("origin", C.c_float * 3), ("tol", C.c_float), ("levels", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class AdaptiveStats(C.Structure):
    """gsdf_adaptive_stats (gsdf_hip.h): what an error-bounded clustering did; bytes 0 .. 223 (RESULT_BYTES) are a function of the mesh
    and the options alone, the rest says what the run cost."""
    _fields_ = [("n_verts_in", C.c_uint64), ("n_tris_in", C.c_uint64), ("used_verts_in", C.c_uint64), ("degenerate_in", C.c_uint64),
                ("cells", C.c_uint64), ("chosen", C.c_uint64 * 16), ("singles", C.c_uint64), ("collapsed", C.c_uint64),
                ("n_verts", C.c_uint64), ("n_tris", C.c_uint64), ("largest_cluster", C.c_uint64), ("max_err", C.c_double),
                ("exponent", C.c_int32), ("reserved", C.c_int32),
                ("ms_cells", C.c_double), ("ms_error", C.c_double), ("ms_faces", C.c_double), ("probes", C.c_uint64), ("table_cells", C.c_uint64),
                ("attempts", C.c_int32), ("reserved2", C.c_int32)]
    RESULT_BYTES = 224

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


CLEAN_MERGE_POSITIONS, CLEAN_FACES = 1, 2  # gsdf_hip.h: GSDF_CLEAN_*


class CleanOpts(C.Structure):
    """gsdf_clean_opts (gsdf_hip.h): which of the two cleaning steps to run."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class CleanStats(C.Structure):
    """gsdf_clean_stats (gsdf_hip.h): what a clean merged and dropped; bytes 0 .. 87 (RESULT_BYTES) are a function of the mesh and the
    flags alone, the rest says what the run cost."""
    _fields_ = [("n_verts_in", C.c_uint64), ("n_tris_in", C.c_uint64), ("merged_verts", C.c_uint64), ("degenerate", C.c_uint64),
                ("face_sets", C.c_uint64), ("cancelled_sets", C.c_uint64), ("duplicate_faces", C.c_uint64), ("opposite_faces", C.c_uint64),
                ("largest_set", C.c_uint64), ("n_verts", C.c_uint64), ("n_tris", C.c_uint64),
                ("ms_merge", C.c_double), ("ms_faces", C.c_double), ("ms_result", C.c_double),
                ("vert_probes", C.c_uint64), ("vert_table_cells", C.c_uint64), ("face_probes", C.c_uint64), ("face_table_cells", C.c_uint64),
                ("vert_attempts", C.c_int32), ("face_attempts", C.c_int32)]
    RESULT_BYTES = 88

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


class ProjectOpts(C.Structure):
    """gsdf_project_opts (gsdf_hip.h): the central-difference step, the on-surface tolerance, the ball no vertex leaves, the trips."""
    _fields_ = [("step", C.c_float), ("tol", C.c_float), ("max_move", C.c_float), ("max_iters", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


PROJECT_STATUS = ["SKIPPED", "ON", "CONVERGED", "ITERS", "FLAT", "CLAMPED", "NONFINITE", "REVERTED"]  # gsdf_hip.h: GSDF_PROJECT_*


class ProjectStats(C.Structure):
    """gsdf_project_stats (gsdf_hip.h): what a projection of a mesh's vertices onto a program's field did; bytes 0 .. 111 (RESULT_BYTES)
    are a function of the mesh, the program and the options alone, ms_device says what the run cost."""
    _fields_ = [("n_verts", C.c_uint64), ("count", C.c_uint64 * 8), ("evals", C.c_uint64), ("over_tol_before", C.c_uint64),
                ("over_tol_after", C.c_uint64), ("max_abs_before", C.c_float), ("max_abs_after", C.c_float), ("steps_max", C.c_uint32),
                ("reserved", C.c_uint32), ("ms_device", C.c_double)]
    RESULT_BYTES = 112

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


class RayOpts(C.Structure):
    """gsdf_ray_opts (gsdf_hip.h, "rays"): where the march starts and ends, the hit tolerance, the shortest step, the march evaluations
    and the bisections of a crossing's bracket."""
    _fields_ = [("t0", C.c_float), ("tmax", C.c_float), ("tol", C.c_float), ("min_step", C.c_float), ("max_steps", C.c_int32),
                ("refine", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ThicknessOpts(C.Structure):
    """gsdf_thickness_opts (gsdf_hip.h): a RayOpts, the central-difference step of the inward normal and the `thin` the stats count below."""
    _fields_ = [("ray", RayOpts), ("step", C.c_float), ("thin", C.c_float), ("reserved", C.c_uint32 * 2)]


RAY_STATUS = ["SKIPPED", "HIT", "CROSSED", "MISS", "STEPS", "NONFINITE", "FLAT"]  # gsdf_hip.h: GSDF_RAY_*


class RayStats(C.Structure):
    """gsdf_ray_stats (gsdf_hip.h): what a batch of rays (the thickness of a mesh) found; bytes 0 .. 103 (RESULT_BYTES) are a function
    of the inputs alone, ms_device says what the run cost."""
    _fields_ = [("n", C.c_uint64), ("count", C.c_uint64 * 8), ("evals", C.c_uint64), ("steps_max", C.c_uint32), ("t_min", C.c_float),
                ("t_max", C.c_float), ("reserved", C.c_uint32), ("below", C.c_uint64), ("ms_device", C.c_double)]
    RESULT_BYTES = 104

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


class ContourOpts(C.Structure):
    """gsdf_contour_opts (gsdf_hip.h): lattice nodes per chunk of whole layers (0: the library's default)."""
    _fields_ = [("max_nodes", C.c_uint64)]


class ContourStats(C.Structure):
    """gsdf_contour_stats (gsdf_hip.h): what a contour / slice call did; bytes 0 .. 63 (RESULT_BYTES) are a function of the program, res
    and the z list alone, the three times say what the run cost (evaluation, tracing, their sum)."""
    _fields_ = [("n_verts", C.c_uint64), ("n_loops", C.c_uint64), ("border_inside", C.c_uint64), ("nonfinite_nodes", C.c_uint64),
                ("saddle_cells", C.c_uint64), ("evals", C.c_uint64), ("nx", C.c_uint32), ("ny", C.c_uint32), ("n_layers", C.c_uint32),
                ("rank_rounds", C.c_uint32), ("ms_device", C.c_double), ("ms_eval", C.c_double), ("ms_trace", C.c_double)]
    RESULT_BYTES = 64

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


class ContourSimplifyOpts(C.Structure):
    """gsdf_contour_simplify_opts (gsdf_hip.h): the deviation a dropped vertex may have, the number of dyadic levels, the passes, dry."""
    _fields_ = [("tol", C.c_float), ("levels", C.c_uint32), ("passes", C.c_uint32), ("dry", C.c_uint32)]


class ContourSimplifyStats(C.Structure):
    """gsdf_contour_simplify_stats (gsdf_hip.h): what a simplification of loops did; bytes 0 .. 183 (RESULT_BYTES) are a function of the
    loops and the options alone, ms_device says what the run cost."""
    _fields_ = [("n_verts_in", C.c_uint64), ("n_verts_out", C.c_uint64), ("n_loops", C.c_uint64), ("loops_changed", C.c_uint64),
                ("spans", C.c_uint64 * 17), ("max_level", C.c_uint32), ("reserved", C.c_uint32), ("max_dev", C.c_double), ("ms_device", C.c_double)]
    RESULT_BYTES = 184

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


# gsdf_loop_measure / gsdf_layer_measure (gsdf_hip.h) as numpy records: one per loop in loop order, one per layer
LOOP_MEASURE_DTYPE = np.dtype([("area", "<f8"), ("length", "<f8"), ("bbox", "<f4", (4,)), ("n_verts", "<u4"), ("layer", "<u4")])
LAYER_MEASURE_DTYPE = np.dtype([("area", "<f8"), ("length", "<f8"), ("bbox", "<f4", (4,)), ("n_loops", "<u4"), ("n_verts", "<u4")])


class Mass(C.Structure):
    """gsdf_mass (gsdf_hip.h, "indexed meshes: mass properties"): volume, first and second moments about the origin (second and
    inertia in the order xx yy zz xy xz yz), centroid and the unit-density inertia tensor about it, of one shell or of the mesh."""
    _fields_ = [("volume", C.c_double), ("first", C.c_double * 3), ("second", C.c_double * 6), ("centroid", C.c_double * 3),
                ("inertia", C.c_double * 6), ("exponent", C.c_int32), ("label", C.c_uint32)]


class Section(C.Structure):
    """gsdf_section (gsdf_hip.h, "contours: section properties"): area, first moments (x, y) and second moments (xx, yy, xy) about
    the origin, centroid and the second moments about it, of one loop or of one layer."""
    _fields_ = [("area", C.c_double), ("first", C.c_double * 2), ("second", C.c_double * 3), ("centroid", C.c_double * 2),
                ("central", C.c_double * 3), ("n_verts", C.c_uint32), ("layer_or_n_loops", C.c_uint32)]


class HatchOpts(C.Structure):
    """gsdf_hatch_opts (gsdf_hip.h, "contours: hatch fill"): the lines' spacing and offset, the directions the layers take in turn, dry."""
    _fields_ = [("spacing", C.c_float), ("offset", C.c_float), ("n_dirs", C.c_uint32), ("dry", C.c_uint32), ("dir", (C.c_float * 2) * 4)]


class HatchLayer(C.Structure):
    """gsdf_hatch_layer (gsdf_hip.h): a layer's hatch length (in units of |dir|), its segments, the smallest and largest line number
    with a crossing (0, -1: none)."""
    _fields_ = [("length", C.c_double), ("n_segments", C.c_uint64), ("k_min", C.c_int32), ("k_max", C.c_int32)]


class HatchStats(C.Structure):
    """gsdf_hatch_stats (gsdf_hip.h): what a hatch produced; bytes 0 .. 55 (RESULT_BYTES) are a function of the loops and the options
    alone, ms_device says what the run cost."""
    _fields_ = [("n_segments", C.c_uint64), ("n_crossings", C.c_uint64), ("n_lines", C.c_uint64), ("max_line_crossings", C.c_uint64),
                ("zero_length", C.c_uint64), ("n_layers", C.c_uint32), ("reserved", C.c_uint32), ("length", C.c_double), ("ms_device", C.c_double)]
    RESULT_BYTES = 56

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


HATCH_LAYER_DTYPE = np.dtype([("length", "<f8"), ("n_segments", "<u8"), ("k_min", "<i4"), ("k_max", "<i4")])


class SkinOpts(C.Structure):
    """gsdf_skin_opts (gsdf_hip.h, "contours: skin classification of the hatch"): the layers under and over a layer that must cover it."""
    _fields_ = [("below", C.c_uint32), ("above", C.c_uint32)]


class SkinLayer(C.Structure):
    """gsdf_skin_layer (gsdf_hip.h): a layer's hatch length and pieces by class (0 inner, 1 bottom, 2 top, 3 both)."""
    _fields_ = [("length", C.c_double * 4), ("n_segments", C.c_uint64 * 4)]


class SkinStats(C.Structure):
    """gsdf_skin_stats (gsdf_hip.h): what a classified hatch produced; bytes 0 .. 127 (RESULT_BYTES) are a function of the loops and
    the options alone, ms_device says what the run cost."""
    _fields_ = [("n_segments", C.c_uint64), ("n_crossings", C.c_uint64), ("n_own_crossings", C.c_uint64), ("n_lines", C.c_uint64),
                ("max_line_crossings", C.c_uint64), ("zero_length", C.c_uint64), ("n_class", C.c_uint64 * 4), ("length", C.c_double * 4),
                ("n_layers", C.c_uint32), ("below", C.c_uint32), ("above", C.c_uint32), ("reserved", C.c_uint32), ("ms_device", C.c_double)]
    RESULT_BYTES = 128

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


SKIN_LAYER_DTYPE = np.dtype([("length", "<f8", (4,)), ("n_segments", "<u8", (4,))])
SKIN_CLASSES = ("inner", "bottom", "top", "both")


class OffsetOpts(C.Structure):
    """gsdf_offset_opts (gsdf_hip.h, "contours: offset"): the lattice spacing, 1 .. 8 insets (> 0 into the material, < 0 outwards), dry,
    lattice nodes per chunk of whole input layers (0: the library's default)."""
    _fields_ = [("res", C.c_float), ("n_insets", C.c_uint32), ("dry", C.c_uint32), ("reserved", C.c_uint32), ("max_nodes", C.c_uint64), ("inset", C.c_float * 8)]


class OffsetStats(C.Structure):
    """gsdf_offset_stats (gsdf_hip.h): what an offset produced and the lattice it used; bytes 0 .. 79 (RESULT_BYTES) are a function of
    the loops and the options alone, the three times say what the run cost (distance field, tracing, their sum)."""
    _fields_ = [("n_verts", C.c_uint64), ("n_loops", C.c_uint64), ("border_inside", C.c_uint64), ("saddle_cells", C.c_uint64), ("inside_nodes", C.c_uint64),
                ("band_nodes", C.c_uint64), ("nx", C.c_uint32), ("ny", C.c_uint32), ("n_layers_in", C.c_uint32), ("n_insets", C.c_uint32), ("x0", C.c_float),
                ("y0", C.c_float), ("band", C.c_float), ("res", C.c_float), ("ms_field", C.c_double), ("ms_trace", C.c_double), ("ms_device", C.c_double)]
    RESULT_BYTES = 80

    def result_bytes(self):
        return bytes(self)[:self.RESULT_BYTES]


# the same two as numpy records (arrays of shells, of loops, of layers)
MASS_DTYPE = np.dtype([("volume", "<f8"), ("first", "<f8", (3,)), ("second", "<f8", (6,)), ("centroid", "<f8", (3,)), ("inertia", "<f8", (6,)),
                       ("exponent", "<i4"), ("label", "<u4")])
SECTION_DTYPE = np.dtype([("area", "<f8"), ("first", "<f8", (2,)), ("second", "<f8", (3,)), ("centroid", "<f8", (2,)), ("central", "<f8", (3,)),
                          ("n_verts", "<u4"), ("layer_or_n_loops", "<u4")])
MASS_TOTAL = 0xffffffff  # Mass.label of a whole mesh


# gsdf_shell (gsdf_hip.h) as a numpy record: one per shell, in increasing order of the label (the shell's smallest vertex number)
SHELL_DTYPE = np.dtype([("n_verts", "<u8"), ("n_tris", "<u8"), ("nonfinite", "<u8"), ("edges", "<u8"), ("boundary_edges", "<u8"),
                        ("nonmanifold_edges", "<u8"), ("misoriented_edges", "<u8"), ("euler", "<i8"), ("area", "<f8"), ("volume", "<f8"),
                        ("centroid", "<f8", (3,)), ("bbox", "<f4", (6,)), ("label", "<u4"), ("reserved", "<u4")])
SHELL_NONE = 0xffffffff  # shell_of(): a vertex no non-degenerate face names / a degenerate face


class HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gsdf_hip error {code}: {msg}")
        self.code = code
        self.msg = msg


def lib():
    """Load libgsdfhip.so. Raises ImportError loudly if it was not built (never falls back)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: the HIP extension must be built "
                              "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.gsdf_hip_last_error.restype = C.c_char_p
        L.gsdf_hip_init.argtypes = [C.c_int]
        L.gsdf_hip_program_create.argtypes = [C.POINTER(GsdfTree), C.POINTER(C.c_void_p)]
        L.gsdf_hip_program_destroy.argtypes = [C.c_void_p]
        L.gsdf_hip_program_destroy.restype = None
        L.gsdf_hip_program_bounds.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.gsdf_hip_program_is2d.argtypes = [C.c_void_p]
        L.gsdf_hip_program_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.gsdf_hip_lower.argtypes = [C.POINTER(GsdfTree), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.gsdf_hip_lower_region.argtypes = [C.POINTER(GsdfTree), C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.gsdf_hip_comm_unique_id.argtypes = [C.c_void_p]
        L.gsdf_hip_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.gsdf_hip_comm_rank.argtypes = [C.c_void_p]
        L.gsdf_hip_comm_world.argtypes = [C.c_void_p]
        L.gsdf_hip_comm_allreduce_sum_u64.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]
        L.gsdf_hip_mesh_gatherv.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.gsdf_hip_mesh_gatherv_start.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.gsdf_hip_mesh_gatherv_wait.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(GatherStats)]
        L.gsdf_hip_comm_destroy.argtypes = [C.c_void_p]
        L.gsdf_hip_comm_transport.restype = C.c_char_p
        L.gsdf_hip_comm_transport.argtypes = [C.c_void_p]
        L.gsdf_hip_gather_plan.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GatherOp), C.c_size_t,
                                           C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
        L.gsdf_hip_mesh_payload.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsdf_hip_mesh_march.argtypes = [C.c_void_p]
        L.gsdf_hip_mesh_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_int)]
        L.gsdf_hip_eval3_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        L.gsdf_hip_eval_wait.argtypes = [C.c_void_p, C.c_int]
        L.gsdf_hip_host_alloc.restype = C.c_void_p
        L.gsdf_hip_host_alloc.argtypes = [C.c_size_t]
        L.gsdf_hip_host_register.argtypes = [C.c_void_p, C.c_size_t]
        L.gsdf_hip_host_release.argtypes = [C.c_void_p]
        L.gsdf_hip_selftest_div.argtypes = [C.c_float, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        L.gsdf_hip_selftest_sqrt.argtypes = [C.POINTER(C.c_uint64)]
        L.gsdf_hip_selftest_circ.argtypes = [C.c_float, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsdf_hip_selftest_atan2.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsdf_hip_selftest_cossin.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsdf_hip_selftest_math.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_float]
        L.gsdf_hip_grid_cus.argtypes = [C.c_int, C.POINTER(C.c_int)]
        L.gsdf_hip_blockcache_create.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_void_p)]
        L.gsdf_hip_blockcache_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float]
        L.gsdf_hip_blockcache_eval3.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]
        L.gsdf_hip_blockcache_hits.restype = C.c_uint64
        L.gsdf_hip_blockcache_hits.argtypes = [C.c_void_p]
        L.gsdf_hip_blockcache_evaluations.restype = C.c_uint64
        L.gsdf_hip_blockcache_evaluations.argtypes = [C.c_void_p]
        L.gsdf_hip_blockcache_destroy.restype = None
        L.gsdf_hip_blockcache_destroy.argtypes = [C.c_void_p]
        L.gsdf_hip_program_specialize.argtypes = [C.c_void_p]
        L.gsdf_hip_program_is_specialized.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.gsdf_hip_program_specialize_async.argtypes = [C.c_void_p]
        L.gsdf_hip_program_specialize_poll.argtypes = [C.c_void_p, C.c_int]
        L.gsdf_hip_program_kernels.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.gsdf_hip_specialize_source.argtypes = [C.POINTER(GsdfTree), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.gsdf_hip_specialize_check.argtypes = [C.POINTER(GsdfTree), C.POINTER(C.c_size_t)]
        L.gsdf_hip_evaluations.restype = C.c_uint64
        L.gsdf_hip_evaluations.argtypes = [C.c_void_p]
        for f in (L.gsdf_hip_eval3, L.gsdf_hip_eval2):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]
        for f in (L.gsdf_hip_eval3_dev, L.gsdf_hip_eval2_dev):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.gsdf_hip_normals3.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float]
        L.gsdf_hip_image2.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.gsdf_hip_image2_color.argtypes = [C.c_void_p, C.POINTER(GsdfColor2), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.gsdf_hip_picture_size.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
        L.gsdf_hip_color_iq.argtypes = [C.POINTER(C.c_float), C.c_float, C.POINTER(GsdfColor2)]
        L.gsdf_hip_color_gradient.argtypes = [C.c_float, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(GsdfColor2)]
        L.gsdf_hip_view_orbit.argtypes = [C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(GsdfView)]
        L.gsdf_hip_render3.argtypes = [C.c_void_p, C.POINTER(GsdfView), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_mesh_octree.argtypes = [C.c_void_p, C.c_float, C.POINTER(MeshOpts), C.POINTER(C.c_void_p)]
        L.gsdf_hip_mesh_octree_start.argtypes = [C.c_void_p, C.c_float, C.POINTER(MeshOpts), C.POINTER(C.c_void_p)]
        L.gsdf_hip_mesh_octree_wait.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.gsdf_hip_mesh_dualcontour.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.gsdf_hip_mesh_flat.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.gsdf_hip_mesh_minecraft.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.POINTER(C.c_void_p)]
        L.gsdf_hip_mesh_stats_get.argtypes = [C.c_void_p, C.POINTER(MeshStats)]
        L.gsdf_hip_mesh_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.gsdf_hip_mesh_dev_tris.restype = C.c_void_p
        L.gsdf_hip_mesh_dev_tris.argtypes = [C.c_void_p]
        L.gsdf_hip_mesh_stl.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.gsdf_hip_mesh_host_tris.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.gsdf_hip_mesh_host_stl.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.gsdf_hip_mesh_destroy.argtypes = [C.c_void_p]
        L.gsdf_hip_mesh_destroy.restype = None
        L.gsdf_hip_mesh_read_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gsdf_hip_mesh_weld.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.gsdf_hip_indexed_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.gsdf_hip_indexed_stats_get.argtypes = [C.c_void_p, C.POINTER(IndexedStats)]
        L.gsdf_hip_indexed_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_indexed_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
        L.gsdf_hip_indexed_read_normals.argtypes = [C.c_void_p, C.c_void_p]
        L.gsdf_hip_indexed_ply.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.gsdf_hip_indexed_host_ply.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.gsdf_hip_indexed_destroy.argtypes = [C.c_void_p]
        L.gsdf_hip_indexed_destroy.restype = None
        L.gsdf_hip_indexed_create.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]
        L.gsdf_hip_indexed_report.argtypes = [C.c_void_p, C.POINTER(IndexedReport)]
        L.gsdf_hip_indexed_shells.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gsdf_hip_indexed_read_shell_of.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_indexed_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.gsdf_hip_indexed_simplify.argtypes = [C.c_void_p, C.POINTER(SimplifyOpts), C.POINTER(C.c_void_p), C.POINTER(SimplifyStats)]
        L.gsdf_hip_indexed_simplify_adaptive.argtypes = [C.c_void_p, C.POINTER(AdaptiveOpts), C.POINTER(C.c_void_p), C.POINTER(AdaptiveStats)]
        L.gsdf_hip_indexed_clean.argtypes = [C.c_void_p, C.POINTER(CleanOpts), C.POINTER(C.c_void_p), C.POINTER(CleanStats)]
        L.gsdf_hip_indexed_project.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ProjectOpts), C.POINTER(C.c_void_p), C.POINTER(ProjectStats)]
        L.gsdf_hip_indexed_read_fit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_raycast3.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayOpts), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(RayStats)]
        L.gsdf_hip_indexed_thickness.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ThicknessOpts), C.c_void_p, C.c_void_p, C.POINTER(RayStats)]
        L.gsdf_hip_mesh_dualcontour_indexed.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(MeshStats)]
        L.gsdf_hip_contour2.argtypes = [C.c_void_p, C.c_float, C.POINTER(ContourOpts), C.POINTER(C.c_void_p)]
        L.gsdf_hip_slice3.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_uint32, C.POINTER(ContourOpts), C.POINTER(C.c_void_p)]
        L.gsdf_hip_contour_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gsdf_hip_contour_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_contour_stats_get.argtypes = [C.c_void_p, C.POINTER(ContourStats)]
        L.gsdf_hip_contour_destroy.argtypes = [C.c_void_p]
        L.gsdf_hip_contour_destroy.restype = None
        L.gsdf_hip_contour_create.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
        L.gsdf_hip_contour_simplify.argtypes = [C.c_void_p, C.POINTER(ContourSimplifyOpts), C.POINTER(C.c_void_p), C.POINTER(ContourSimplifyStats)]
        L.gsdf_hip_contour_measures.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_contour_measures_ms.argtypes = []
        L.gsdf_hip_contour_measures_ms.restype = C.c_double
        L.gsdf_hip_indexed_mass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gsdf_hip_indexed_mass_ms.argtypes = []
        L.gsdf_hip_indexed_mass_ms.restype = C.c_double
        L.gsdf_hip_inertia_principal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_contour_sections.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_contour_sections_ms.argtypes = []
        L.gsdf_hip_contour_sections_ms.restype = C.c_double
        L.gsdf_hip_contour_hatch.argtypes = [C.c_void_p, C.POINTER(HatchOpts), C.POINTER(C.c_void_p), C.POINTER(HatchStats)]
        L.gsdf_hip_hatch_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.gsdf_hip_hatch_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_hatch_rank_ms.argtypes = []
        L.gsdf_hip_hatch_rank_ms.restype = C.c_double
        L.gsdf_hip_hatch_destroy.argtypes = [C.c_void_p]
        L.gsdf_hip_hatch_destroy.restype = None
        L.gsdf_hip_contour_hatch_skin.argtypes = [C.c_void_p, C.POINTER(HatchOpts), C.POINTER(SkinOpts), C.POINTER(C.c_void_p), C.POINTER(SkinStats)]
        L.gsdf_hip_hatch_read_skin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsdf_hip_skin_rank_ms.argtypes = []
        L.gsdf_hip_skin_rank_ms.restype = C.c_double
        L.gsdf_hip_contour_offset.argtypes = [C.c_void_p, C.POINTER(OffsetOpts), C.POINTER(C.c_void_p), C.POINTER(OffsetStats)]
        L.gsdf_hip_contour_distance.argtypes = [C.c_void_p, C.POINTER(OffsetOpts), C.c_uint32, C.c_void_p, C.POINTER(OffsetStats)]
        L.gsdf_hip_brick_owner.restype = C.c_uint32
        L.gsdf_hip_brick_owner.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.gsdf_hip_slab_range.restype = None
        L.gsdf_hip_slab_range.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise HipError(rc, lib().gsdf_hip_last_error().decode())


def lower(shader_or_tree):
    """Host-only lowering of a tree to the device instruction stream: (uint32 code array, lds_slots)."""
    tree = shader_or_tree.tree() if hasattr(shader_or_tree, "tree") else shader_or_tree
    n, sl = C.c_uint32(), C.c_uint32()
    _check(lib().gsdf_hip_lower(C.byref(tree), None, 0, C.byref(n), C.byref(sl)))
    code = np.zeros(n.value, np.uint32)
    _check(lib().gsdf_hip_lower(C.byref(tree), code.ctypes.data, n.value, C.byref(n), C.byref(sl)))
    return code, sl.value


def view_orbit(bounds, yaw=0.0, pitch=0.0, cam_dist=None, target=None, aa=1, max_steps=256):
    """The UI's orbit camera (gsdf_hip_view_orbit; host only, no device needed): a GsdfView looking at `target` (None = the
    origin, as gsdfaux/ui.go) from yaw / pitch (radians) at cam_dist (None = the bounds' diagonal, the UI's default)."""
    bb = (C.c_float * 6)(*[float(v) for v in np.asarray(bounds, np.float32).reshape(6)])
    ta = None if target is None else (C.c_float * 3)(*[float(v) for v in np.asarray(target, np.float32).reshape(3)])
    v = GsdfView()
    _check(lib().gsdf_hip_view_orbit(bb, np.float32(yaw), np.float32(pitch), np.float32(0.0 if cam_dist is None else cam_dist), ta, C.byref(v)))
    v.aa, v.max_steps = int(aa), int(max_steps)
    return v


def _bounds6(bounds):
    return (C.c_float * 6)(*[float(v) for v in np.asarray(bounds, np.float32).reshape(6)])


def picture_size(bounds, pic_height):
    """gsdfaux.RenderPNGFile's picture width for pic_height rows (gsdf_hip_picture_size; host only): the bounds' aspect ratio."""
    w = C.c_int()
    _check(lib().gsdf_hip_picture_size(_bounds6(bounds), int(pic_height), C.byref(w)))
    return w.value


def color_iq(bounds, char_dist=None):
    """ColorConversionInigoQuilez(char_dist) as a GsdfColor2 (gsdf_hip_color_iq; host only); None = RenderPNGFile's default,
    the bounds' Diagonal() / 3."""
    c = GsdfColor2()
    _check(lib().gsdf_hip_color_iq(_bounds6(bounds), np.float32(0.0 if char_dist is None else char_dist), C.byref(c)))
    return c


def color_gradient(length, c0=(0, 0, 0, 255), c1=(255, 255, 255, 255)):
    """ColorConversionLinearGradient(length, c0, c1) as a GsdfColor2 (gsdf_hip_color_gradient; host only): c0 / c1 are 8-bit RGBA as
    image.RGBA stores them; the bytes of black -> white select the black-and-white conversion, as color.Black, color.White do in Go
    (Go's test is an interface comparison: an RGBA black -> white takes the HSV path there, which differs only at length 0, where d
    is 0 or NaN -- gsdf_hip.h). kind=COLOR_GRADIENT afterwards selects that path."""
    a, b = (C.c_uint8 * 4)(*[int(v) for v in c0]), (C.c_uint8 * 4)(*[int(v) for v in c1])
    c = GsdfColor2()
    _check(lib().gsdf_hip_color_gradient(np.float32(length), a, b, C.byref(c)))
    return c


def color_default():
    """ImageRendererSDF2's own default conversion (black, white, red for NaN / Inf) as a GsdfColor2."""
    c = GsdfColor2()
    c.kind = COLOR_DEFAULT
    return c


# gsdf_hip_selftest_math's numbering: 0..12 as oracle/orc_math_export.c, then the evaluator's other routes
MATH_FN = {"hypot": 0, "atan2_ref": 1, "sin": 2, "cos": 3, "acos": 4, "cbrt": 5, "sincos_s": 6, "sincos_c": 7, "min": 8, "max": 9,
           "pow13": 10, "round": 11, "floor": 12, "cossin_c": 13, "cossin_s": 14, "atan2": 15, "sqrt": 16, "div": 17,
           "face2": 18, "face2_legacy": 19, "face3": 20, "face3_legacy": 21}


def math_apply(name, x, y=None, divisor=1.0):
    """One of the device's math routes over x (and y) elementwise, one value per lane (test hook: gsdf_hip_selftest_math)."""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    if y is not None:
        y = np.ascontiguousarray(y, np.float32)
        if y.shape != x.shape:
            raise ValueError("operands differ in shape")
    _check(lib().gsdf_hip_selftest_math(MATH_FN[name], x.ctypes.data, y.ctypes.data if y is not None else None, out.ctypes.data, x.size,
                                        np.float32(divisor)))
    return out


def grid_cus(device=-1, real=False):
    """The CU count a handle created now would size its grids from (test hook: gsdf_hip_grid_cus; GSDF_HIP_GRID_CUS lowers it);
    real=True: (that count, the device's own)."""
    r = C.c_int()
    n = lib().gsdf_hip_grid_cus(int(device), C.byref(r))
    if n <= 0:
        raise HipError(-6, "no HIP device")
    return (n, r.value) if real else n


def init(device=-1):
    """gleval.Init1x1GLFW analogue: make sure a HIP device is usable (raises otherwise)."""
    _check(lib().gsdf_hip_init(device))


class SDFHIP:
    """gleval.SDF3 / SDF2 implemented by the HIP interpreter kernel for one flattened tree."""

    def __init__(self, shader_or_tree, device=-1):
        L = lib()
        tree = shader_or_tree.tree() if hasattr(shader_or_tree, "tree") else shader_or_tree
        self._tree = tree
        if device >= 0:
            _check(L.gsdf_hip_init(device))
        h = C.c_void_p()
        _check(L.gsdf_hip_program_create(C.byref(tree), C.byref(h)))
        self._h = h
        self.is2d = bool(L.gsdf_hip_program_is2d(h))

    def close(self):
        if getattr(self, "_h", None):
            lib().gsdf_hip_program_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Bounds(self):
        bb = (C.c_float * 6)()
        _check(lib().gsdf_hip_program_bounds(self._h, bb))
        return np.array(bb[:], np.float32)

    def Evaluations(self):
        return int(lib().gsdf_hip_evaluations(self._h))

    def info(self):
        a, b = C.c_uint32(), C.c_uint32()
        _check(lib().gsdf_hip_program_info(self._h, C.byref(a), C.byref(b)))
        t = C.c_double()
        sp = lib().gsdf_hip_program_is_specialized(self._h, C.byref(t))
        buf = C.create_string_buffer(512)
        _check(lib().gsdf_hip_program_kernels(self._h, buf, 512))
        kern = dict(kv.split("=") for kv in buf.value.decode().split())
        leaf_k = int(kern["leaf"].split("<")[1].split(",")[0]) if "leaf" in kern else 0  # points per lane of the leaf phase
        # the lowering's division census: divisors with RN(1/d), divisors declined, polygons flagged for the reciprocal form, polygons not
        recip = dict(zip(("recip", "declined", "poly_recip", "poly_plain"), (int(x) for x in kern["recip"].split("/")))) if "recip" in kern else None
        return {"code_words": a.value, "lds_slots": b.value, "specialized": bool(sp), "specialize_s": t.value, "kernels": kern, "leaf_k": leaf_k,
                "recip": recip}

    def specialize(self):
        """Build (hiprtc) and switch to kernels specialised for this tree: same bits, no fetch/decode. Returns self."""
        _check(lib().gsdf_hip_program_specialize(self._h))
        return self

    def specialize_async(self):
        """Start the same build on a thread of the library's own and return: the handle works through the interpreter kernels until
        the specialised ones are ready and switches at its next call (gsdf_hip_program_specialize_async). Returns self."""
        _check(lib().gsdf_hip_program_specialize_async(self._h))
        return self

    def specialize_poll(self, wait=False):
        """True once the handle runs specialised kernels (wait=True: block until the background build has finished)."""
        rc = lib().gsdf_hip_program_specialize_poll(self._h, 1 if wait else 0)
        if rc < 0:
            _check(rc)
        return rc == 1

    def Evaluate(self, pos, dist=None, userData=None):
        """pos: (n,3)|(n,4)|(n,2) float32 host array (row stride = position stride); dist: (n,) float32."""
        pos = np.asarray(pos, np.float32)
        if pos.ndim != 2 or not pos.flags.c_contiguous:
            pos = np.ascontiguousarray(pos.reshape(-1, 2 if self.is2d else 3))
        n = pos.shape[0]
        if dist is None:
            dist = np.empty(n, np.float32)
        elif not (isinstance(dist, np.ndarray) and dist.dtype == np.float32 and dist.ndim == 1 and dist.flags.c_contiguous and dist.flags.writeable):
            # the C side writes n float32 values at dist's address: anything else would be silently corrupted
            raise ValueError("dist must be a writeable, C-contiguous, 1-D float32 array")
        f = lib().gsdf_hip_eval2 if self.is2d else lib().gsdf_hip_eval3
        _check(f(self._h, pos.ctypes.data, pos.strides[0], n, dist.ctypes.data, dist.shape[0]))
        return dist

    def submit(self, pos, dist):
        """Pipelined Evaluate: returns a ticket at once; wait(ticket) blocks until `dist` holds the distances. pos / dist
        must stay alive and untouched until then (C-contiguous float32 arrays)."""
        if pos.dtype != np.float32 or dist.dtype != np.float32 or not pos.flags.c_contiguous or not dist.flags.c_contiguous or dist.ndim != 1:
            raise ValueError("submit needs C-contiguous float32 arrays (pos (n,3|4), dist (n,))")
        t = C.c_int(-1)
        _check(lib().gsdf_hip_eval3_submit(self._h, pos.ctypes.data, pos.strides[0], pos.shape[0], dist.ctypes.data, dist.shape[0], C.byref(t)))
        return t.value

    def wait(self, ticket):
        _check(lib().gsdf_hip_eval_wait(self._h, ticket))

    def evaluate_dev(self, d_pos_ptr, stride_bytes, d_dist_ptr, n, stream=None):
        """Device-resident evaluation on raw device pointers (e.g. torch tensors' data_ptr())."""
        f = lib().gsdf_hip_eval2_dev if self.is2d else lib().gsdf_hip_eval3_dev
        _check(f(self._h, d_pos_ptr, stride_bytes, d_dist_ptr, n, stream))

    def render_image(self, w, h):
        """glrender.ImageRendererSDF2.Render with the default conversion: (dist (h,w) float32, rgba (h,w,4) uint8)."""
        dist = np.empty((h, w), np.float32)
        rgba = np.empty((h, w, 4), np.uint8)
        _check(lib().gsdf_hip_image2(self._h, w, h, dist.ctypes.data, rgba.ctypes.data))
        return dist, rgba

    def render_picture(self, w, h, color=None):
        """The picture of a 2-D part with one of gsdfaux's conversions (a GsdfColor2; None = RenderPNGFile's default, color_iq of
        the bounds; gsdf_hip_image2_color): (rgba (h,w,4) uint8, dist (h,w) float32), row 0 at the top."""
        conv = color_iq(self.Bounds()) if color is None else color
        hh, ww = max(int(h), 0), max(int(w), 0)  # (the library refuses bad sizes with GSDF_ERR_BAD_ARGUMENT)
        rgba = np.empty((hh, ww, 4), np.uint8)
        dist = np.empty((hh, ww), np.float32)
        _check(lib().gsdf_hip_image2_color(self._h, C.byref(conv), int(w), int(h), rgba.ctypes.data, dist.ctypes.data))
        return rgba, dist

    def render_png(self, path, pic_height, color=None):
        """gsdfaux.RenderPNGFile: width from the bounds' aspect ratio, the IQ conversion of Diagonal() / 3 unless `color` is given,
        written as an 8-bit RGBA PNG. Returns the (h, w, 4) pixels."""
        from . import png
        w = picture_size(self.Bounds(), pic_height)
        rgba, _ = self.render_picture(w, pic_height, color)
        png.write_png(path, rgba)
        return rgba

    def render3(self, view, w, h):
        """One UI frame through the camera `view` (a GsdfView; gsdf_hip_render3): (rgba (h,w,4) uint8, depth (h,w) float32, evals
        (h,w) uint32), row 0 at the top."""
        hh, ww = max(int(h), 0), max(int(w), 0)  # (the library refuses bad sizes with GSDF_ERR_BAD_ARGUMENT)
        rgba = np.empty((hh, ww, 4), np.uint8)
        depth = np.empty((hh, ww), np.float32)
        evals = np.empty((hh, ww), np.uint32)
        _check(lib().gsdf_hip_render3(self._h, C.byref(view), int(w), int(h), rgba.ctypes.data, depth.ctypes.data, evals.ctypes.data))
        return rgba, depth, evals

    def render_view(self, w, h, yaw=0.0, pitch=0.0, cam_dist=None, aa=1, target=None, max_steps=256):
        """gsdfaux.UI's view of the part, headless: the orbit camera of view_orbit over this handle's bounds, then render3."""
        return self.render3(view_orbit(self.Bounds(), yaw, pitch, cam_dist, target, aa, max_steps), w, h)

    def normals(self, pos, step):
        pos = np.ascontiguousarray(pos, np.float32)
        out = np.empty_like(pos)
        _check(lib().gsdf_hip_normals3(self._h, pos.ctypes.data, out.ctypes.data, pos.shape[0], step))
        return out

    def raycast(self, origins, dirs, t0=0.0, tmax=float("inf"), tol=1e-4, min_step=0.0, max_steps=256, refine=8, thin=0.0):
        """gsdf_hip_raycast3: the rays origins + t dirs ((n, 3) each; dirs used as given, so t is in units of |dir|) sphere-traced
        through the field from t0, from outside or inside the part: (t (n,) float32, d (n,) float32, status (n,) uint8 -- see
        RAY_STATUS --, steps (n,) uint16, RayStats). A query, not a guarantee: see the header."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != r.shape:
            raise ValueError("origins and dirs differ in shape")
        rays = np.ascontiguousarray(np.concatenate([o, r], axis=1))
        n = len(rays)
        t, d, status, steps = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.uint8), np.empty(n, np.uint16)
        ro = RayOpts(t0=np.float32(t0), tmax=np.float32(tmax), tol=np.float32(tol), min_step=np.float32(min_step), max_steps=int(max_steps), refine=int(refine))
        st = RayStats()
        _check(lib().gsdf_hip_raycast3(self._h, rays.ctypes.data, n, C.byref(ro), np.float32(thin), t.ctypes.data, d.ctypes.data, status.ctypes.data,
                                       steps.ctypes.data, C.byref(st)))
        return t, d, status, steps, st


def host_array(shape, dtype=np.float32):
    """numpy array over pinned, device-mapped host memory (gsdf_hip_host_alloc): Evaluate calls on such arrays make no
    staging copy -- the kernel reads / writes them across PCIe. Freed when the array (and its views) are collected."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = lib().gsdf_hip_host_alloc(max(n, 1))
    if not ptr:
        raise MemoryError("gsdf_hip_host_alloc failed")

    class _Owner:
        def __init__(self, p): self.p = p
        def __del__(self):
            try: lib().gsdf_hip_host_release(self.p)
            except Exception: pass
    raw = (C.c_ubyte * max(n, 1)).from_address(ptr)
    raw._owner = _Owner(ptr)
    return np.frombuffer(raw, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


SDF3HIP = SDFHIP
SDF2HIP = SDFHIP


class BlockCachedSDF3HIP:
    """gleval.BlockCachedSDF3 (gleval/gleval.go:110-218) in front of a HIP evaluator: Reset / Evaluate / CacheHits /
    Evaluations / Bounds with the reference's semantics (lossy per-cell cache, misses evaluated in one batch)."""

    def __init__(self, sdf, resX, resY, resZ):
        self._h = C.c_void_p()
        self.sdf = sdf
        _check(lib().gsdf_hip_blockcache_create(sdf._h, resX, resY, resZ, C.byref(self._h)))

    def Reset(self, sdf, resX, resY, resZ):
        _check(lib().gsdf_hip_blockcache_reset(self._h, sdf._h, resX, resY, resZ))
        self.sdf = sdf

    def Evaluate(self, pos, dist=None, userData=None):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        if dist is None:
            dist = np.empty(pos.shape[0], np.float32)
        _check(lib().gsdf_hip_blockcache_eval3(self._h, pos.ctypes.data, 12, pos.shape[0], dist.ctypes.data, dist.shape[0]))
        return dist

    def CacheHits(self):
        return int(lib().gsdf_hip_blockcache_hits(self._h))

    def Evaluations(self):
        return int(lib().gsdf_hip_blockcache_evaluations(self._h))

    def Bounds(self):
        return self.sdf.Bounds()

    def __del__(self):
        try:
            if self._h:
                lib().gsdf_hip_blockcache_destroy(self._h)
                self._h = None
        except Exception:
            pass


class OctreeHIP:
    """glrender.Octree drop-in: octree pruning + marching cubes on device, triangles drained on demand.

    NewOctreeRenderer(s, cubeResolution, evalBufferSize) -> OctreeHIP(sdf, res) ; the evaluation buffer
    argument has no meaning here (positions are generated on device)."""

    def __init__(self, sdf, res, evalBufferSize=64, prune=True, shard_rank=0, shard_count=1, max_tris=0, stream=None,
                 share_corners=False, host_output=False, assume_sdf=False, payload=PAYLOAD_TRIANGLES):
        if evalBufferSize < 64:
            raise ValueError("bad octree eval buffer size")
        self.sdf = sdf
        self._mesh = None
        self._cursor = 0
        # share_corners: False / 0 every corner of every leaf (the reference's evaluations), True / 1 the distinct lattice points
        # of a brick (leaf_dense_kernel), 2 the distinct z rows of a brick (same kernels, same triangles, fewer evaluations)
        # prune: True / False, or an int bit mask of the octree levels to centre-test (bit L = Level L >= 3);
        # assume_sdf: the reference's predicate verbatim instead of the field's bounds over the cube (gsdf_hip.h)
        self._opts = MeshOpts(int(prune) | (PRUNE_ASSUME_SDF if assume_sdf else 0), shard_rank, shard_count, max_tris, stream, int(share_corners), int(host_output), int(payload), 0)
        self.Reset(sdf, res)

    def Reset(self, sdf, res):
        self._free()
        self.sdf = sdf
        m = C.c_void_p()
        _check(lib().gsdf_hip_mesh_octree(sdf._h, np.float32(res), C.byref(self._opts), C.byref(m)))
        self._adopt(m)

    def _adopt(self, m):
        self._mesh = m
        self._cursor = 0
        st = MeshStats()
        _check(lib().gsdf_hip_mesh_stats_get(m, C.byref(st)))
        self.stats = st

    @classmethod
    def start(cls, sdf, res, **kw):
        """gsdf_hip_mesh_octree_start: enqueue the mesh and return a PendingMesh; .wait() gives the OctreeHIP. Up to three per
        program in flight -- start the next one before waiting for the previous one and the GPU never idles between meshes."""
        self = cls.__new__(cls)
        self.sdf, self._mesh, self._cursor = sdf, None, 0
        kw.setdefault("prune", True)
        self._opts = MeshOpts(int(kw["prune"]) | (PRUNE_ASSUME_SDF if kw.get("assume_sdf") else 0), kw.get("shard_rank", 0), kw.get("shard_count", 1),
                              kw.get("max_tris", 0), kw.get("stream"), int(kw.get("share_corners", False)), int(kw.get("host_output", False)),
                              int(kw.get("payload", PAYLOAD_TRIANGLES)), 0)
        j = C.c_void_p()
        _check(lib().gsdf_hip_mesh_octree_start(sdf._h, np.float32(res), C.byref(self._opts), C.byref(j)))
        return PendingMesh(self, j)

    def _free(self):
        if getattr(self, "_mesh", None):
            lib().gsdf_hip_mesh_destroy(self._mesh)
            self._mesh = None

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    def TotalPruned(self):
        return int(self.stats.pruned_leaves)

    def payload(self):
        """(kind, records, payload bytes): PAYLOAD_TRIANGLES, or PAYLOAD_RECORDS -- packed cut-leaf records, no triangles yet."""
        n, b = C.c_uint64(), C.c_uint64()
        k = lib().gsdf_hip_mesh_payload(self._mesh, C.byref(n), C.byref(b))
        _check(min(k, 0))
        return k, int(n.value), int(b.value)

    def stage_ms(self):
        """{kernel name: device milliseconds} of the mesher's stages, where it records them (dual contouring)."""
        ms, names, n = (C.c_double * 8)(), (C.c_char_p * 8)(), C.c_int()
        _check(lib().gsdf_hip_mesh_stage_ms(self._mesh, ms, names, 8, C.byref(n)))
        return {names[k].decode(): float(ms[k]) for k in range(n.value)}

    def march(self):
        """Marching cubes over a records mesh, in place: afterwards it reads like any mesh (gsdf_hip_mesh_march)."""
        _check(lib().gsdf_hip_mesh_march(self._mesh))
        return self

    def records(self):
        """The cut-leaf records of a records mesh, in the order marching cubes takes them (gsdf_hip_mesh_read_records):
        (dist (n, 8) float32, leaf (n, 3) integer coordinates, case (n,))."""
        n = C.c_uint64()
        _check(lib().gsdf_hip_mesh_read_records(self._mesh, None, 0, C.byref(n)))
        raw = np.zeros((n.value, 10), np.uint32)
        if n.value:
            _check(lib().gsdf_hip_mesh_read_records(self._mesh, raw.ctypes.data, n.value, None))
        leaf = np.stack([raw[:, 8] & 0xffff, raw[:, 8] >> 16, raw[:, 9] & 0xffff], axis=1).astype(np.int64)
        return raw[:, :8].copy().view(np.float32), leaf, (raw[:, 9] >> 16).astype(np.int64)

    def weld(self):
        """The mesh with its marching-cubes vertices welded by lattice edge (gsdf_hip_mesh_weld): an IndexedHIP. For a mesh made
        with payload=PAYLOAD_RECORDS and shard_count 1, marched or not."""
        h = C.c_void_p()
        _check(lib().gsdf_hip_mesh_weld(self._mesh, C.byref(h)))
        return IndexedHIP(h)

    def n_tris(self):
        return int(self.stats.n_tris)

    def dev_ptr(self):
        return lib().gsdf_hip_mesh_dev_tris(self._mesh)

    def ReadTriangles(self, dst, userData=None):
        """dst: (k,3,3) float32. Returns (n, eof) like (n, io.EOF); needs len(dst) >= 5 (io.ErrShortBuffer)."""
        if dst.shape[0] < 5:
            raise BufferError("short buffer")
        remaining = self.n_tris() - self._cursor
        n = min(remaining, dst.shape[0])
        if n:
            _check(lib().gsdf_hip_mesh_read(self._mesh, self._cursor, n, dst.ctypes.data))
        self._cursor += n
        return n, self._cursor >= self.n_tris()

    def RenderAll(self):
        """glrender.RenderAll: all triangles as (n,3,3) float32."""
        n = self.n_tris()
        out = np.empty((n, 3, 3), np.float32)
        if n:
            _check(lib().gsdf_hip_mesh_read(self._mesh, 0, n, out.ctypes.data))
        return out

    def WriteBinarySTL(self):
        """glrender.WriteBinarySTL of the device-resident triangles, records built on device."""
        return self.stl_view().tobytes()

    def _view(self, ptr, nbytes, dtype):
        # numpy array over memory the mesh owns; the ctypes object in its base chain keeps this renderer alive
        raw = (C.c_ubyte * nbytes).from_address(ptr)
        raw._owner = self
        a = np.frombuffer(raw, dtype=dtype)
        a.flags.writeable = False
        return a

    def triangles_view(self):
        """All triangles as a read-only (n,3,3) float32 array over pinned host memory owned by the mesh (one DMA, no
        copy). Valid until this renderer is Reset or freed."""
        n = self.n_tris()
        if n == 0:
            return np.empty((0, 3, 3), np.float32)
        p = C.c_void_p()
        _check(lib().gsdf_hip_mesh_host_tris(self._mesh, C.byref(p)))
        return self._view(p.value, n * 36, np.float32).reshape(n, 3, 3)

    def stl_view(self):
        """The complete binary STL file as a read-only uint8 array over pinned host memory owned by the mesh
        (f.write(view) writes it without another copy). Valid until this renderer is Reset or freed."""
        p, ln = C.c_void_p(), C.c_size_t()
        _check(lib().gsdf_hip_mesh_host_stl(self._mesh, C.byref(p), C.byref(ln)))
        return self._view(p.value, ln.value, np.uint8)


def inertia_principal(inertia):
    """gsdf_hip_inertia_principal (host only): (moments (3,) ascending, axes (3, 3), one unit vector per row, right-handed) of a
    symmetric tensor given as six values xx yy zz xy xz yz or as a (3, 3) array (its upper triangle is read)."""
    a = np.asarray(inertia, np.float64)
    if a.shape == (3, 3):
        a = np.array([a[0, 0], a[1, 1], a[2, 2], a[0, 1], a[0, 2], a[1, 2]])
    a = np.ascontiguousarray(a.reshape(6))
    m, ax = np.empty(3, np.float64), np.empty((3, 3), np.float64)
    _check(lib().gsdf_hip_inertia_principal(a.ctypes.data, m.ctypes.data, ax.ctypes.data))
    return m, ax


def _mass_dict(rec, density):
    i = np.asarray(rec["inertia"], np.float64) * float(density)
    tensor = np.array([[i[0], i[3], i[4]], [i[3], i[1], i[5]], [i[4], i[5], i[2]]])
    if np.isfinite(i).all():
        moments, axes = inertia_principal(i)
    else:
        moments, axes = np.full(3, np.nan), np.full((3, 3), np.nan)
    return {"label": int(rec["label"]), "volume": float(rec["volume"]), "mass": float(density) * float(rec["volume"]),
            "centroid": np.array(rec["centroid"], np.float64), "inertia": tensor, "moments": moments, "axes": axes}


class IndexedHIP:
    """An indexed triangle mesh resident on the device (gsdf_indexed): vertices, faces, the vertices' lattice keys, optional
    normals, and its binary PLY. Independent of the mesh it was welded from."""

    def __init__(self, handle):
        self._h = handle
        nv, nf, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        _check(lib().gsdf_hip_indexed_counts(handle, C.byref(nv), C.byref(nf), C.byref(ms)))
        self.n_verts, self.n_tris, self.ms_device = int(nv.value), int(nf.value), float(ms.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().gsdf_hip_indexed_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stats(self):
        st = IndexedStats()
        _check(lib().gsdf_hip_indexed_stats_get(self._h, C.byref(st)))
        return st

    def read(self):
        """(verts (V, 3) float32, idx (F, 3) uint32, keys (V,) uint64)."""
        v, i, k = np.empty((self.n_verts, 3), np.float32), np.empty((self.n_tris, 3), np.uint32), np.empty(self.n_verts, np.uint64)
        _check(lib().gsdf_hip_indexed_read(self._h, v.ctypes.data, i.ctypes.data, k.ctypes.data))
        return v, i, k

    def normals(self, sdf, step):
        """gleval.NormalsCentralDiff of `sdf` at the vertices, computed and kept on the device; returns them (V, 3) float32."""
        _check(lib().gsdf_hip_indexed_normals(self._h, sdf._h, np.float32(step)))
        n = np.empty((self.n_verts, 3), np.float32)
        _check(lib().gsdf_hip_indexed_read_normals(self._h, n.ctypes.data))
        return n

    @classmethod
    def from_arrays(cls, verts, idx, keys=None):
        """A host mesh on the device (gsdf_hip_indexed_create): verts (V, 3) float32, idx (F, 3) vertex numbers, keys (V,) uint64 or
        None (they then read back as 0). An index >= V raises HipError (GSDF_ERR_BAD_ARGUMENT) with the face and the index."""
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        i = np.asarray(idx)
        if i.size and (i.min() < 0 or i.max() > 0xffffffff):
            raise ValueError("vertex numbers must fit 32 unsigned bits")
        i = np.ascontiguousarray(i, np.uint32).reshape(-1, 3)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64).reshape(-1)
        if k is not None and len(k) != len(v):
            raise ValueError("one key per vertex")
        h = C.c_void_p()
        _check(lib().gsdf_hip_indexed_create(v.ctypes.data, len(v), i.ctypes.data, len(i), None if k is None else k.ctypes.data, C.byref(h)))
        return cls(h)

    @classmethod
    def dual_contour(cls, sdf, res, chiseled=False, stream=None):
        """gsdf_hip_mesh_dualcontour_indexed: the dual-contouring mesh of `sdf` (an SDF3HIP) at cube size `res` as an indexed mesh, one
        vertex per kept cube that a quad names, the faces in lattice order (z, y, x, axis) -- byte for byte the same on every run.
        .mesh_stats: the MeshStats gsdf_hip_mesh_dualcontour reports for the same call."""
        h, st = C.c_void_p(), MeshStats()
        _check(lib().gsdf_hip_mesh_dualcontour_indexed(sdf._h, np.float32(res), int(bool(chiseled)), stream, C.byref(h), C.byref(st)))
        ix = cls(h)
        ix.mesh_stats = st
        return ix

    def report(self):
        """gsdf_hip_indexed_report: an IndexedReport (computed on the device once per handle)."""
        rep = IndexedReport()
        _check(lib().gsdf_hip_indexed_report(self._h, C.byref(rep)))
        return rep

    def shells(self):
        """gsdf_hip_indexed_shells: a structured array (SHELL_DTYPE), one record per shell in increasing order of its label."""
        n = C.c_uint64()
        _check(lib().gsdf_hip_indexed_shells(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, SHELL_DTYPE)
        if n.value:
            _check(lib().gsdf_hip_indexed_shells(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def mass_records(self):
        """gsdf_hip_indexed_mass as it is: (a MASS_DTYPE record of the mesh, a MASS_DTYPE array with one record per shell in shell
        order), unit density; computed on the device once per handle."""
        total, n = np.zeros(1, MASS_DTYPE), C.c_uint64()
        _check(lib().gsdf_hip_indexed_mass(self._h, total.ctypes.data, None, 0, C.byref(n)))
        shells = np.zeros(n.value, MASS_DTYPE)
        if n.value:
            _check(lib().gsdf_hip_indexed_mass(self._h, None, shells.ctypes.data, n.value, C.byref(n)))
        return total[0], shells

    def mass(self, density=1.0):
        """Mass properties of the solid the mesh bounds: (total, shells), each a dict (shells: a list in shell order) with label
        (MASS_TOTAL for the mesh), volume, mass = density * volume, centroid (3,), inertia (3, 3) about the centroid = density * the
        unit-density tensor, and its principal moments (3,) ascending with their axes (3, 3), one unit vector per row
        (inertia_principal). A record with volume 0 has NaN centroid, inertia, moments and axes."""
        total, shells = self.mass_records()
        return _mass_dict(total, density), [_mass_dict(s, density) for s in shells]

    @staticmethod
    def mass_ms():
        """Device milliseconds (HIP events) of the pass behind this thread's last mass() / mass_records()."""
        return float(lib().gsdf_hip_indexed_mass_ms())

    def shell_of(self):
        """(shell number of every vertex (V,), of every face (F,)) uint32; SHELL_NONE for an unused vertex / a degenerate face."""
        sv, sf = np.empty(self.n_verts, np.uint32), np.empty(self.n_tris, np.uint32)
        _check(lib().gsdf_hip_indexed_read_shell_of(self._h, sv.ctypes.data, sf.ctypes.data))
        return sv, sf

    def extract(self, keep=None, drop_degenerate=True):
        """gsdf_hip_indexed_extract: a new IndexedHIP with the faces of the kept shells (keep: one truth value per shell, None = all)
        in their order, vertices renumbered by first appearance; degenerate faces stay only with keep=None, drop_degenerate=False."""
        k = None
        if keep is not None:
            k = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8).reshape(-1)
            if len(k) != int(self.report().n_shells):
                raise ValueError("keep: one entry per shell")
        h = C.c_void_p()
        _check(lib().gsdf_hip_indexed_extract(self._h, None if k is None else k.ctypes.data, 1 if drop_degenerate else 0, C.byref(h)))
        return IndexedHIP(h)

    def simplify(self, cell, origin=(0, 0, 0), dry=False):
        """gsdf_hip_indexed_simplify: the mesh with the used vertices of every grid cell (edge `cell`, cell (0, 0, 0) starting at
        `origin`) merged into one vertex at their mean and the collapsed faces dropped: (a new IndexedHIP, SimplifyStats). dry: the
        stats alone, (None, SimplifyStats), at the cost of the clustering and one pass over the faces."""
        o = SimplifyOpts(cell=np.float32(cell), origin=(C.c_float * 3)(*[np.float32(x) for x in origin]))
        st, h = SimplifyStats(), C.c_void_p()
        _check(lib().gsdf_hip_indexed_simplify(self._h, C.byref(o), None if dry else C.byref(h), C.byref(st)))
        return (None if dry else IndexedHIP(h)), st

    def clean(self, merge=False, faces=True, dry=False):
        """gsdf_hip_indexed_clean: the mesh with vertices of equal position merged (merge), degenerate faces dropped, and of the faces
        over one set of three vertices at most one kept (faces): (a new IndexedHIP, CleanStats). dry: (None, CleanStats)."""
        o = CleanOpts(flags=(CLEAN_MERGE_POSITIONS if merge else 0) | (CLEAN_FACES if faces else 0))
        st, h = CleanStats(), C.c_void_p()
        _check(lib().gsdf_hip_indexed_clean(self._h, C.byref(o), None if dry else C.byref(h), C.byref(st)))
        return (None if dry else IndexedHIP(h)), st

    @classmethod
    def from_soup(cls, tris):
        """A triangle soup (F, 3, 3) float32 -- an STL read back, OctreeHIP.read()'s triangles -- as an indexed mesh: uploaded as 3 F
        vertices with idx = arange, then clean(merge=True, faces=False), which joins the corners with equal positions:
        (IndexedHIP, CleanStats). Corners that are merely close stay apart (gsdf_hip.h, "indexed meshes: clean")."""
        t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
        soup = cls.from_arrays(t.reshape(-1, 3), np.arange(3 * len(t), dtype=np.uint32).reshape(-1, 3))
        try:
            return soup.clean(merge=True, faces=False)
        finally:
            soup.close()

    def read_normals(self):
        """The normals the handle holds (V, 3) float32 -- computed by normals(), or carried by extract / clean; HipError if it has none."""
        n = np.empty((self.n_verts, 3), np.float32)
        _check(lib().gsdf_hip_indexed_read_normals(self._h, n.ctypes.data))
        return n

    def simplify_to(self, max_tris, cell0, origin=(0, 0, 0)):
        """The first of cell0, 2 cell0, 4 cell0, ... (float32 doubling: exact) whose simplification has at most max_tris faces, found by
        dry runs; then that mesh: (IndexedHIP, SimplifyStats, cell). ValueError after 24 doublings, or once nothing would be kept."""
        cell = np.float32(cell0)
        for _ in range(25):
            _, st = self.simplify(cell, origin, dry=True)
            if st.n_tris == 0:
                raise ValueError(f"simplify_to: nothing is kept at cell {float(cell)!r}, and every smaller cell tried keeps more than {max_tris} faces")
            if st.n_tris <= max_tris:
                ix, st = self.simplify(cell, origin)
                return ix, st, cell
            cell = np.float32(cell * np.float32(2))
        raise ValueError(f"simplify_to: more than {max_tris} faces after 24 doublings of the cell {float(np.float32(cell0))!r}")

    def simplify_adaptive(self, cell, tol, levels=8, origin=(0, 0, 0), dry=False):
        """gsdf_hip_indexed_simplify_adaptive: the mesh with the used vertices of every chosen cell merged into one vertex at their mean,
        a vertex's cell being the coarsest of its `levels` nested ones (edges cell, 2 cell, ..) whose mean stays within `tol` of the plane
        of every face touching it: (a new IndexedHIP, AdaptiveStats). dry: the stats alone, (None, AdaptiveStats)."""
        o = AdaptiveOpts(cell=np.float32(cell), origin=(C.c_float * 3)(*[np.float32(x) for x in origin]), tol=np.float32(tol), levels=int(levels))
        st, h = AdaptiveStats(), C.c_void_p()
        _check(lib().gsdf_hip_indexed_simplify_adaptive(self._h, C.byref(o), None if dry else C.byref(h), C.byref(st)))
        return (None if dry else IndexedHIP(h)), st

    def simplify_adaptive_to(self, max_tris, cell, tol0, levels=8, origin=(0, 0, 0)):
        """The first of tol0, 2 tol0, 4 tol0, ... (float32 doubling: exact) whose adaptive simplification has at most max_tris faces, found
        by dry runs (the count does not increase with tol); then that mesh: (IndexedHIP, AdaptiveStats, tol). ValueError for tol0 <= 0,
        after 24 doublings, or once nothing would be kept."""
        tol = np.float32(tol0)
        if not tol > 0:
            raise ValueError(f"simplify_adaptive_to: tol0 must be positive to be doubled, not {float(tol)!r}")
        for _ in range(25):
            _, st = self.simplify_adaptive(cell, tol, levels, origin, dry=True)
            if st.n_tris == 0:
                raise ValueError(f"simplify_adaptive_to: nothing is kept at tol {float(tol)!r}, and every smaller tol tried keeps more than {max_tris} faces")
            if st.n_tris <= max_tris:
                ix, st = self.simplify_adaptive(cell, tol, levels, origin)
                return ix, st, tol
            tol = np.float32(tol * np.float32(2))
        raise ValueError(f"simplify_adaptive_to: more than {max_tris} faces after 24 doublings of tol {float(np.float32(tol0))!r} "
                         f"(cells of at most {1 << (int(levels) - 1)} x {float(np.float32(cell))!r}: raise levels or the cell)")

    def project(self, sdf, step, tol, max_move, max_iters=8, dry=False):
        """gsdf_hip_indexed_project: the mesh with every vertex moved onto the zero set of `sdf` (an SDF3HIP) by up to max_iters Newton
        steps along its central-difference gradient (step: as normals()), never further than max_move from where it started and never
        further from the surface than it was: (a new IndexedHIP with the same faces and keys, ProjectStats). dry: (None, ProjectStats)."""
        o = ProjectOpts(step=np.float32(step), tol=np.float32(tol), max_move=np.float32(max_move), max_iters=int(max_iters))
        st, h = ProjectStats(), C.c_void_p()
        _check(lib().gsdf_hip_indexed_project(self._h, sdf._h, C.byref(o), None if dry else C.byref(h), C.byref(st)))
        return (None if dry else IndexedHIP(h)), st

    def deviation(self, sdf, tol):
        """How far the vertices are from the surface of `sdf`: the dry run of project() with no step, one evaluation per vertex
        (ProjectStats: max_abs_before, over_tol_before, count[ON])."""
        return self.project(sdf, 1.0, tol, 0.0, max_iters=0, dry=True)[1]

    def thickness(self, sdf, step, t0, tmax, tol, min_step=0.0, max_steps=256, refine=8, thin=0.0, dry=False):
        """gsdf_hip_indexed_thickness: per vertex, the distance to the opposite wall of `sdf` (an SDF3HIP) along the inward normal
        (central differences of `step`, as normals()), marched through the field from t0 (pick t0 > tol): (thickness (V,) float32 --
        +Inf where the ray left through tmax, NaN where it has no answer --, status (V,) uint8, see RAY_STATUS, RayStats: t_min,
        t_max, below = the vertices thinner than `thin`). dry: (None, None, RayStats)."""
        ro = RayOpts(t0=np.float32(t0), tmax=np.float32(tmax), tol=np.float32(tol), min_step=np.float32(min_step), max_steps=int(max_steps), refine=int(refine))
        o = ThicknessOpts(ray=ro, step=np.float32(step), thin=np.float32(thin))
        st = RayStats()
        if dry:
            _check(lib().gsdf_hip_indexed_thickness(self._h, sdf._h, C.byref(o), None, None, C.byref(st)))
            return None, None, st
        th, status = np.empty(self.n_verts, np.float32), np.empty(self.n_verts, np.uint8)
        _check(lib().gsdf_hip_indexed_thickness(self._h, sdf._h, C.byref(o), th.ctypes.data, status.ctypes.data, C.byref(st)))
        return th, status, st

    def fit(self):
        """Of a handle project() made: (d_before (V,) float32, d_after (V,) float32, status (V,) uint8, see PROJECT_STATUS)."""
        a, b, s = np.empty(self.n_verts, np.float32), np.empty(self.n_verts, np.float32), np.empty(self.n_verts, np.uint8)
        _check(lib().gsdf_hip_indexed_read_fit(self._h, a.ctypes.data, b.ctypes.data, s.ctypes.data))
        return a, b, s

    def select_shells(self, min_tris=0, drop_cavities=False):
        """A keep mask for extract() from the shell table: shells with at least min_tris faces and, with drop_cavities, a volume
        that is not negative (an enclosed cavity is a shell wound inside out)."""
        sh = self.shells()
        keep = sh["n_tris"] >= min_tris
        if drop_cavities:
            keep &= ~(sh["volume"] < 0)
        return keep

    def ply_size(self):
        ln = C.c_size_t()
        lib().gsdf_hip_indexed_ply(self._h, None, 0, C.byref(ln))
        return int(ln.value)

    def ply(self):
        """The binary PLY file as bytes (gsdf_hip_indexed_ply: packed on the device, copied into a buffer of the caller's)."""
        buf = np.empty(self.ply_size(), np.uint8)
        ln = C.c_size_t()
        _check(lib().gsdf_hip_indexed_ply(self._h, buf.ctypes.data, buf.size, C.byref(ln)))
        return buf[:ln.value].tobytes()

    def ply_view(self):
        """The same file as a read-only uint8 array over pinned host memory the handle owns (one DMA, no copy): valid until
        normals() is called or the handle is freed."""
        p, ln = C.c_void_p(), C.c_size_t()
        _check(lib().gsdf_hip_indexed_host_ply(self._h, C.byref(p), C.byref(ln)))
        raw = (C.c_ubyte * ln.value).from_address(p.value)
        raw._owner = self
        a = np.frombuffer(raw, dtype=np.uint8)
        a.flags.writeable = False
        return a


def layer_heights(bounds, h):
    """The mid-heights of the layers of thickness h that cover the z extent of `bounds` (6 floats): z_k = fl(bb.min.z + fl((k + 0.5) h)),
    float32, for every k whose z_k lies below bb.max.z."""
    bb = np.asarray(bounds, np.float32).reshape(6)
    h = np.float32(h)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("layer height must be finite and positive")
    n = int(np.ceil(float(np.float32(bb[5] - bb[2]) / h))) + 1
    z = (np.float32(bb[2]) + (np.arange(n, dtype=np.float32) + np.float32(0.5)) * h).astype(np.float32)
    return np.ascontiguousarray(z[z < bb[5]])


class ContourHIP:
    """The outline of a 2-D part or the z-slices of a 3-D part as ordered closed loops, traced on the device (gsdf_contour; the
    "contours" section of gsdf_hip.h states the arithmetic). Independent of the program it was traced from."""

    def __init__(self, handle):
        self._h = handle
        nl, nq, nv = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(lib().gsdf_hip_contour_counts(handle, C.byref(nl), C.byref(nq), C.byref(nv)))
        self.n_layers, self.n_loops, self.n_verts = int(nl.value), int(nq.value), int(nv.value)
        self.xy = np.empty((self.n_verts, 2), np.float32)
        self.keys = np.empty(self.n_verts, np.uint32)
        self.loop_start = np.empty(self.n_loops + 1, np.uint32)
        self.loop_layer = np.empty(self.n_loops, np.uint32)
        _check(lib().gsdf_hip_contour_read(handle, self.xy.ctypes.data, self.keys.ctypes.data, self.loop_start.ctypes.data, self.loop_layer.ctypes.data))

    def close(self):
        if getattr(self, "_h", None):
            lib().gsdf_hip_contour_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def outline(cls, sdf2, res, max_nodes=0):
        """gsdf_hip_contour2: the outline of the 2-D part `sdf2` (an SDF2HIP) on a lattice of spacing res, one layer."""
        h, o = C.c_void_p(), ContourOpts(int(max_nodes))
        _check(lib().gsdf_hip_contour2(sdf2._h, np.float32(res), C.byref(o), C.byref(h)))
        return cls(h)

    @classmethod
    def slices(cls, sdf3, res, z, max_nodes=0):
        """gsdf_hip_slice3: the contours of the 3-D part `sdf3` in the planes z[k] (float32), one layer each; max_nodes: lattice nodes
        per chunk of whole layers (0: the default; the result does not depend on it)."""
        z = np.ascontiguousarray(z, np.float32).reshape(-1)
        h, o = C.c_void_p(), ContourOpts(int(max_nodes))
        _check(lib().gsdf_hip_slice3(sdf3._h, np.float32(res), z.ctypes.data if len(z) else None, len(z), C.byref(o), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, xy, loop_start, loop_layer=None, n_layers=1, keys=None):
        """gsdf_hip_contour_create: host loops on the device. xy (n, 2) float32, loop_start n_loops + 1, loop_layer n_loops (None: all 0),
        keys n (None: they read back as 0)."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        loop_start = np.ascontiguousarray(loop_start, np.uint32).reshape(-1)
        n_loops = max(len(loop_start) - 1, 0)
        if loop_layer is not None:
            loop_layer = np.ascontiguousarray(loop_layer, np.uint32).reshape(-1)
            if len(loop_layer) != n_loops:
                raise ValueError(f"from_arrays: {len(loop_layer)} layers for {n_loops} loops")
        if keys is not None:
            keys = np.ascontiguousarray(keys, np.uint32).reshape(-1)
            if len(keys) != len(xy):
                raise ValueError(f"from_arrays: {len(keys)} keys for {len(xy)} vertices")
        h = C.c_void_p()
        _check(lib().gsdf_hip_contour_create(xy.ctypes.data if len(xy) else None, len(xy), loop_start.ctypes.data if len(loop_start) else None, n_loops,
                                             None if loop_layer is None else loop_layer.ctypes.data, int(n_layers),
                                             None if keys is None else keys.ctypes.data, C.byref(h)))
        return cls(h)

    @property
    def stats(self):
        st = ContourStats()
        _check(lib().gsdf_hip_contour_stats_get(self._h, C.byref(st)))
        return st

    def simplify(self, tol, levels=8, passes=1, dry=False):
        """gsdf_hip_contour_simplify: the loops without the vertices that lie within tol of a dyadic chord of their loop (gsdf_hip.h,
        "contours: simplify and measures"): (a new ContourHIP, ContourSimplifyStats). dry: (None, ContourSimplifyStats)."""
        o = ContourSimplifyOpts(np.float32(tol), int(levels), int(passes), int(bool(dry)))
        st, h = ContourSimplifyStats(), C.c_void_p()
        _check(lib().gsdf_hip_contour_simplify(self._h, C.byref(o), None if dry else C.byref(h), C.byref(st)))
        return (None if dry else ContourHIP(h)), st

    def simplify_to(self, max_verts, tol0, levels=8, passes=1):
        """The first of tol0, 2 tol0, 4 tol0, ... (float32 doubling: exact) whose simplification has at most max_verts vertices, found by
        dry runs (one pass never keeps more at a larger tol); then those loops: (ContourHIP, ContourSimplifyStats, tol). ValueError for
        tol0 <= 0, or when +Inf still keeps more (every loop keeps ceil(n / 2^kmax) >= 3 vertices)."""
        tol = np.float32(tol0)
        if not tol > 0:
            raise ValueError(f"simplify_to: tol0 must be positive to be doubled, not {float(tol)!r}")
        _, st = self.simplify(np.inf, levels, passes, dry=True)
        if st.n_verts_out > max_verts:
            raise ValueError(f"simplify_to: {st.n_verts_out} vertices are kept at any tol with levels {int(levels)} and passes {int(passes)}, more than {max_verts}")
        while True:
            _, st = self.simplify(tol, levels, passes, dry=True)
            if st.n_verts_out <= max_verts:
                c, st = self.simplify(tol, levels, passes)
                return c, st, tol
            with np.errstate(over="ignore"):
                tol = np.float32(tol * np.float32(2))

    def measures(self):
        """gsdf_hip_contour_measures: (loops, layers) as numpy records (LOOP_MEASURE_DTYPE per loop, LAYER_MEASURE_DTYPE per layer):
        signed area, length and box, summed on the device as integers (order-independent to the bit)."""
        loops = np.zeros(self.n_loops, LOOP_MEASURE_DTYPE)
        layers = np.zeros(self.n_layers, LAYER_MEASURE_DTYPE)
        _check(lib().gsdf_hip_contour_measures(self._h, loops.ctypes.data if self.n_loops else None, layers.ctypes.data if self.n_layers else None))
        return loops, layers

    @staticmethod
    def measures_ms():
        """Device milliseconds (HIP events) of this thread's last measures()."""
        return float(lib().gsdf_hip_contour_measures_ms())

    def sections(self):
        """gsdf_hip_contour_sections: (loops, layers) as numpy records (SECTION_DTYPE per loop and per layer): area, first and second
        moments of area about the origin, centroid and the second moments about it, summed on the device as integers."""
        loops = np.zeros(self.n_loops, SECTION_DTYPE)
        layers = np.zeros(self.n_layers, SECTION_DTYPE)
        _check(lib().gsdf_hip_contour_sections(self._h, loops.ctypes.data if self.n_loops else None, layers.ctypes.data if self.n_layers else None))
        return loops, layers

    @staticmethod
    def sections_ms():
        """Device milliseconds (HIP events) of this thread's last sections()."""
        return float(lib().gsdf_hip_contour_sections_ms())

    @staticmethod
    def _hatch_opts(spacing, dirs, offset, dry):
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 2)
        o = HatchOpts(np.float32(spacing), np.float32(offset), len(dirs), int(bool(dry)))
        for k, (dx, dy) in enumerate(dirs[:4]):
            o.dir[k][0], o.dir[k][1] = float(dx), float(dy)
        return o

    def hatch_dirs(self, spacing, dirs, offset=0.0, dry=False):
        """gsdf_hip_contour_hatch with raw float32 directions (1 .. 4 pairs (dx, dy); layer l takes dirs[l % len(dirs)]): a HatchHIP;
        dry: (None, HatchStats)."""
        o = self._hatch_opts(spacing, dirs, offset, dry)
        st, h = HatchStats(), C.c_void_p()
        _check(lib().gsdf_hip_contour_hatch(self._h, C.byref(o), None if dry else C.byref(h), C.byref(st)))
        return (None, st) if dry else HatchHIP(h, st)

    def hatch(self, spacing, angles_deg=(45.0,), offset=0.0, dry=False):
        """The segments of parallel lines `spacing` apart inside the loops of every layer (gsdf_hip.h, "contours: hatch fill"); layer l
        takes the direction float32(cos), float32(sin) of angles_deg[l % len(angles_deg)], computed in float64. A HatchHIP; dry: (None,
        HatchStats)."""
        a = np.radians(np.asarray(angles_deg, np.float64).reshape(-1))
        return self.hatch_dirs(spacing, np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32), offset, dry)

    @staticmethod
    def hatch_rank_ms():
        """Device milliseconds (HIP events) of the rank pass of this thread's last hatch."""
        return float(lib().gsdf_hip_hatch_rank_ms())

    def skin_dirs(self, spacing, dirs, below, above, offset=0.0, dry=False):
        """gsdf_hip_contour_hatch_skin with raw float32 directions: the hatch of hatch_dirs cut against the loops of the `below` layers
        under and the `above` layers over each layer, a HatchHIP whose cls gives every piece's class (0 inner, 1 bottom, 2 top, 3 both)
        and whose skin_layers the layers' lengths by class; dry: (None, SkinStats)."""
        o = self._hatch_opts(spacing, dirs, offset, dry)
        k = SkinOpts(int(below), int(above))
        st, h = SkinStats(), C.c_void_p()
        _check(lib().gsdf_hip_contour_hatch_skin(self._h, C.byref(o), C.byref(k), None if dry else C.byref(h), C.byref(st)))
        return (None, st) if dry else HatchHIP(h, st, skin=True)

    def skin(self, spacing, angles_deg, below, above, offset=0.0, dry=False):
        """skin_dirs with the directions float32(cos), float32(sin) of angles_deg, as hatch() makes them."""
        a = np.radians(np.asarray(angles_deg, np.float64).reshape(-1))
        return self.skin_dirs(spacing, np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32), below, above, offset, dry)

    @staticmethod
    def skin_rank_ms():
        """Device milliseconds (HIP events) of the rank and parity pass of this thread's last skin()."""
        return float(lib().gsdf_hip_skin_rank_ms())

    @staticmethod
    def _offset_opts(res, insets, max_nodes, dry):
        insets = np.ascontiguousarray(insets, np.float32).reshape(-1)
        o = OffsetOpts(np.float32(res), len(insets), int(bool(dry)), 0, int(max_nodes))
        for k, v in enumerate(insets[:8]):
            o.inset[k] = float(v)
        return o

    def offset(self, res, insets, max_nodes=0, dry=False):
        """gsdf_hip_contour_offset: the loops moved sideways by the in-plane distances `insets` (1 .. 8 floats; > 0 into the material,
        < 0 outwards, 0 re-traces), traced on a lattice of spacing res from the signed distance to the layer's own edges (gsdf_hip.h,
        "contours: offset"). A new ContourHIP with n_layers x len(insets) layers -- input layer l with inset i is layer
        l len(insets) + i -- and the call's OffsetStats as .offset_stats; dry: (None, OffsetStats)."""
        o = self._offset_opts(res, insets, max_nodes, dry)
        st, h = OffsetStats(), C.c_void_p()
        _check(lib().gsdf_hip_contour_offset(self._h, C.byref(o), None if dry else C.byref(h), C.byref(st)))
        if dry:
            return None, st
        c = ContourHIP(h)
        c.offset_stats = st
        return c

    def distance(self, res, insets, layer):
        """gsdf_hip_contour_distance: the signed in-plane distance of input layer `layer` to its own loops (negative inside, clamped to
        the band of these insets) on exactly the lattice offset(res, insets) uses: an (ny, nx) float32 array. The lattice's origin and
        spacing are in .offset_stats of an offset, or in the OffsetStats of a dry one. Two device passes run: a dry offset (the field
        of every layer and its trace) for nx and ny, as the header has it, then this layer's field again."""
        _, st = self.offset(res, insets, dry=True)
        d = np.empty((int(st.ny), int(st.nx)), np.float32)
        o = self._offset_opts(res, insets, 0, False)
        _check(lib().gsdf_hip_contour_distance(self._h, C.byref(o), int(layer), d.ctypes.data, None))
        return d

    def loops(self, layer=None):
        """The loops (of one layer, or of all) as (n, 2) float32 arrays, in the handle's order."""
        return [self.xy[self.loop_start[q]:self.loop_start[q + 1]] for q in range(self.n_loops) if layer is None or self.loop_layer[q] == layer]

    def areas(self):
        """Signed area of every loop: the float64 shoelace sum over the handle's order, on the host (outer boundaries > 0, holes < 0)."""
        return np.array([loop_area(l) for l in self.loops()], np.float64)


class HatchHIP:
    """The hatch segments of a ContourHIP (gsdf_hatch): seg (n, 4) float32 (x0 y0 x1 y1), line n int32 (the line number k of each),
    layer_start n_layers + 1, layers (HATCH_LAYER_DTYPE records), stats (HatchStats). Independent of the loops it was made from.
    Made by ContourHIP.skin: also cls n uint8 (every segment's class) and skin_layers (SKIN_LAYER_DTYPE records), stats a SkinStats;
    both are None for a plain hatch."""

    def __init__(self, handle, stats, skin=False):
        self._h = handle
        self.stats = stats
        nl, ns = C.c_uint32(), C.c_uint64()
        _check(lib().gsdf_hip_hatch_counts(handle, C.byref(nl), C.byref(ns)))
        self.n_layers, self.n_segments = int(nl.value), int(ns.value)
        self.seg = np.empty((self.n_segments, 4), np.float32)
        self.line = np.empty(self.n_segments, np.int32)
        self.layer_start = np.empty(self.n_layers + 1, np.uint32)
        self.layers = np.zeros(self.n_layers, HATCH_LAYER_DTYPE)
        _check(lib().gsdf_hip_hatch_read(handle, self.seg.ctypes.data, self.line.ctypes.data, self.layer_start.ctypes.data, self.layers.ctypes.data))
        self.cls = self.skin_layers = None
        if skin:
            self.cls = np.empty(self.n_segments, np.uint8)
            self.skin_layers = np.zeros(self.n_layers, SKIN_LAYER_DTYPE)
            _check(lib().gsdf_hip_hatch_read_skin(handle, self.cls.ctypes.data, self.skin_layers.ctypes.data))

    def close(self):
        if getattr(self, "_h", None):
            lib().gsdf_hip_hatch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def segments(self, layer):
        """The segments of one layer, (n, 4) float32, in (k, position) order."""
        return self.seg[self.layer_start[layer]:self.layer_start[layer + 1]]


def loop_area(xy):
    """Float64 shoelace area of one closed loop, (n, 2)."""
    p = np.asarray(xy, np.float64)
    q = np.roll(p, -1, axis=0)
    return 0.5 * float(np.sum(p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]))


class PendingMesh:
    """A mesh whose chain of kernels is enqueued (OctreeHIP.start): wait() returns the finished OctreeHIP."""

    def __init__(self, oc, job):
        self._oc, self._j = oc, job

    def wait(self):
        j, self._j = self._j, None
        m = C.c_void_p()
        _check(lib().gsdf_hip_mesh_octree_wait(j, C.byref(m)))
        self._oc._adopt(m)
        return self._oc

    def __del__(self):
        try:
            if self._j:
                m = C.c_void_p()
                if lib().gsdf_hip_mesh_octree_wait(self._j, C.byref(m)) == 0 and m.value:
                    lib().gsdf_hip_mesh_destroy(m)
                self._j = None
        except Exception:
            pass


class CommHIP:
    """RCCL communicator of the multi-GPU mesher (one process per GPU; gsdf_hip_comm_* in include/gsdf_hip.h).
    Rank 0 draws CommHIP.unique_id() and ships the 128 bytes to the other ranks by any means; every rank then builds
    CommHIP(id, rank, world) after hip.init(device) -- a collective call."""
    ID_BYTES = 128

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * CommHIP.ID_BYTES)()
        _check(lib().gsdf_hip_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, unique_id, rank, world):
        if len(unique_id) != CommHIP.ID_BYTES:
            raise ValueError("unique id must be %d bytes" % CommHIP.ID_BYTES)
        buf = (C.c_ubyte * CommHIP.ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        _check(lib().gsdf_hip_comm_create(buf, rank, world, C.byref(h)))
        self._h, self.rank, self.world = h, rank, world

    def transport(self):
        """"rccl" or "loopback" (GSDF_HIP_COMM=loopback at unique_id() time: ranks are threads of one process)."""
        return lib().gsdf_hip_comm_transport(self._h).decode()

    def allreduce_sum(self, values):
        """Sum of each of `values` (ints) over all ranks. Collective."""
        arr = (C.c_uint64 * len(values))(*[int(v) for v in values])
        _check(lib().gsdf_hip_comm_allreduce_sum_u64(self._h, arr, len(values)))
        return [int(v) for v in arr]

    def close(self):
        if getattr(self, "_h", None):
            lib().gsdf_hip_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GatheredMeshHIP(OctreeHIP):
    """All ranks' triangles, rank-major, device resident on every rank: the result of <renderer>.gatherv(comm)
    (gsdf_hip_mesh_gatherv: RCCL all-gather of the counts + one group of broadcasts, no padding, no staging copies).
    Reads like any renderer: n_tris / RenderAll / ReadTriangles / triangles_view / WriteBinarySTL / dev_ptr."""

    def __init__(self, mesh, counts, stats):
        self.sdf = None
        self._mesh = mesh
        self._cursor = 0
        self.counts = counts
        self.stats = stats

    def Reset(self, sdf, res):
        raise TypeError("a gathered mesh is a result, not a renderer")


def _gatherv(self, comm):
    """RCCL all-gatherv of this rank's triangles with those of the other ranks of `comm`. Collective."""
    out = C.c_void_p()
    counts = (C.c_uint64 * comm.world)()
    _check(lib().gsdf_hip_mesh_gatherv(self._mesh, comm._h, C.byref(out), counts))
    st = MeshStats()
    _check(lib().gsdf_hip_mesh_stats_get(out, C.byref(st)))
    return GatheredMeshHIP(out, [int(c) for c in counts], st)


OctreeHIP.gatherv = _gatherv


class PendingGather:
    """A gather whose payload is moving (gsdf_hip_mesh_gatherv_start): wait() returns (GatheredMeshHIP or None, counts,
    GatherStats). The source renderer may be Reset or freed meanwhile: the library keeps the buffers the gather reads until
    the payload has moved (a destroy in between is deferred)."""

    def __init__(self, src, comm, handle):
        self._src, self._comm, self._h = src, comm, handle

    def wait(self):
        out = C.c_void_p()
        counts = (C.c_uint64 * self._comm.world)()
        gs = GatherStats()
        h, self._h = self._h, None
        _check(lib().gsdf_hip_mesh_gatherv_wait(h, C.byref(out), counts, C.byref(gs)))
        self._src = None
        g = None
        if out.value:
            st = MeshStats()
            _check(lib().gsdf_hip_mesh_stats_get(out, C.byref(st)))
            g = GatheredMeshHIP(out, [int(c) for c in counts], st)
        return g, [int(c) for c in counts], gs

    def __del__(self):
        try:
            if self._h:
                lib().gsdf_hip_mesh_gatherv_wait(self._h, None, None, None)
                self._h = None
        except Exception:
            pass


def _gatherv_start(self, comm, mode=GATHER_ALL, root=0):
    """Collective. Exchanges the counts, enqueues the payload (ALL: everyone gets everything, ROOT: only `root`, NONE: counts
    only) and returns a PendingGather; mesh the next part, then .wait()."""
    h = C.c_void_p()
    _check(lib().gsdf_hip_mesh_gatherv_start(self._mesh, comm._h, int(mode), int(root), C.byref(h)))
    return PendingGather(self, comm, h)


OctreeHIP.gatherv_start = _gatherv_start


class DualContourHIP(OctreeHIP):
    """glrender.DualContourRenderer with DualContourLeastSquares on device (Reset + RenderAll)."""

    def __init__(self, sdf, res, chiseled=False, stream=None, shard_rank=0, shard_count=1):
        self._shard = (shard_rank, shard_count)
        self.sdf = sdf
        self._mesh = None
        self._cursor = 0
        self._chiseled = bool(chiseled)
        self._stream = stream
        self.Reset(sdf, res)

    def Reset(self, sdf, res):
        self._free()
        self.sdf = sdf
        m = C.c_void_p()
        _check(lib().gsdf_hip_mesh_dualcontour(sdf._h, np.float32(res), int(self._chiseled), self._shard[0], self._shard[1],
                                               self._stream, C.byref(m)))
        self._mesh = m
        self._cursor = 0
        st = MeshStats()
        _check(lib().gsdf_hip_mesh_stats_get(m, C.byref(st)))
        self.stats = st


class MinecraftHIP(OctreeHIP):
    """glrender.minecraftRender (dual_contour.go:297-403) on device: the axis-aligned faces between level-1 cubes whose origins lie on
    different sides of the surface."""

    def __init__(self, sdf, res, stream=None):
        self.sdf = sdf
        self._mesh = None
        self._cursor = 0
        m = C.c_void_p()
        _check(lib().gsdf_hip_mesh_minecraft(sdf._h, np.float32(res), stream, C.byref(m)))
        self._mesh = m
        st = MeshStats()
        _check(lib().gsdf_hip_mesh_stats_get(m, C.byref(st)))
        self.stats = st


class FlatHIP(OctreeHIP):
    """glrender.FlatRenderer drop-in (NewFlatRenderer(s, cubeResolution, evalBufferSize, numParallel)): the whole corner
    lattice evaluated into a device-resident grid, then marching cubes of every cube. evalBufferSize / numParallel keep
    the reference's argument checks (flatrenderer.go:37-45) and have no other meaning on the device."""

    def __init__(self, sdf, res, evalBufferSize=4096, numParallel=1, stream=None, shard_rank=0, shard_count=1):
        if evalBufferSize < 8:
            raise ValueError("flat renderer eval buffer size must be at least 8")
        if numParallel < 1:
            raise ValueError("flat renderer numParallel must be at least 1")
        self._shard = (shard_rank, shard_count)
        self.sdf = sdf
        self._mesh = None
        self._cursor = 0
        self._stream = stream
        self.Reset(sdf, res)

    def Reset(self, sdf, res):
        self._free()
        self.sdf = sdf
        m = C.c_void_p()
        _check(lib().gsdf_hip_mesh_flat(sdf._h, np.float32(res), self._shard[0], self._shard[1], self._stream, C.byref(m)))
        self._mesh = m
        self._cursor = 0
        st = MeshStats()
        _check(lib().gsdf_hip_mesh_stats_get(m, C.byref(st)))
        self.stats = st

    def Evaluations(self):
        return int(self.stats.evals)


def gather_plan(bytes_per_rank, rank, mode=GATHER_ALL, root=0):
    """gsdf_hip_gather_plan (host only, pure): ([(kind, peer, src_off, dst_off, bytes), ...], total_bytes) -- the transfers rank
    `rank` performs in a gather of payloads of bytes_per_rank[r] bytes, and the size of its gathered buffer."""
    world = len(bytes_per_rank)
    arr = (C.c_uint64 * world)(*[int(b) for b in bytes_per_rank])
    ops = (GatherOp * (2 * world + 1))()
    n, total = C.c_size_t(), C.c_uint64()
    _check(lib().gsdf_hip_gather_plan(arr, world, int(rank), int(mode), int(root), ops, len(ops), C.byref(n), C.byref(total)))
    return [(o.kind, o.peer, int(o.src_off), int(o.dst_off), int(o.bytes)) for o in ops[:n.value]], int(total.value)
