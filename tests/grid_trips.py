"""Every launch of gsdf_amd/csrc whose grid is smaller than one workgroup per 256 elements, and the case of
tests/test_gpu_grid_trips.py that drives its grid-stride loop through three trips or more.

Such a launch is sized by grid_for(n, num_cu, workgroups per CU) (abi_program.h) or by `num_cu * ...` written out -- then
GSDF_HIP_GRID_CUS=1 (tools/README.md) makes one trip of the loop `workgroups per CU x elements per workgroup and trip` elements long --
or by a constant. tests/test_grid_census.py reads the launches out of the host sources and requires each kernel here; the cases
compute `trip` from this table and assert their own size condition (check_trips below), so a shape that shrinks later fails instead
of passing vacuously.

    kernel -> Row(cap, unit, cases, counts, ragged, bound)

cap     workgroups per CU (an int: the grid is min(work, CUs x cap)), or ("wg", N): N workgroups whatever the device
unit    elements one workgroup takes per trip, in the element `counts` names (a tuple: one per build of the kernel, K = 1, 2, 4
        points per lane; the condition holds for each)
cases   the test functions of tests/test_gpu_grid_trips.py that drive the kernel and assert the condition
ragged  False where n is a power of two by construction (a hash table's size, 8^levels cubes): no partial last trip exists
bound   True where the public statistics give a lower bound of n only: n >= 3 trip + 1 is asserted on the bound, n % trip is not
"""
from collections import namedtuple

Row = namedtuple("Row", "cap unit cases counts ragged bound", defaults=(True, False))
K124 = (256, 512, 1024)   # a lane takes K = 1, 2 or 4 points per trip (gsdf_program::batch_k)

GRID_TABLE = {
    # ---- abi_eval.hip ------------------------------------------------------------------------------------------------------------
    "eval_kernel": Row(64, K124, ("test_evaluate", "test_block_cache"), "points of one call"),
    "normals_kernel": Row(8, 256, ("test_normals",), "points"),
    "image2_kernel": Row(8, K124, ("test_images",), "pixels"),
    "image2_color_kernel": Row(8, K124, ("test_images",), "pixels"),
    # the refilling form (GSDF_HIP_VIEW_REFILL=1): persistent workgroups, at most 4 per CU, whose lanes claim pixels until none is left
    "view_kernel": Row(4, 256, ("test_view_refill",), "claims: pixels rounded up to 8 x 8 tiles"),
    # ---- abi_mesh.hip: octree ----------------------------------------------------------------------------------------------------
    "prune_spec_kernel": Row(8, 256, ("test_octree",), "cubes of the speculative top: (8^S - 1) / 7"),
    "prune_kernel": Row(2, 256, ("test_octree_prune_chain",), "candidates of a level of the chain (>= its survivors: leaf_cubes / 64 at level 3)", True, True),
    "leaf_eval_kernel": Row(32, 256, ("test_octree",), "leaves (stats.leaf_cubes)"),
    "leaf_dense_kernel": Row(32, 256, ("test_octree",), "leaves (stats.leaf_cubes)"),
    "march_records_kernel": Row(4, 256, ("test_octree",), "cut leaves (stats.cut_leaves): a workgroup walks its share 256 at a time"),
    "pack_records_kernel": Row(8, 4096, ("test_octree",), "leaves: a workgroup packs a group of 64 blocks of 64"),
    "march_dense_kernel": Row(4, 256, ("test_octree", "test_gather"), "records: a workgroup walks its share of the chunks of 256"),
    "stl_kernel": Row(8, 256, ("test_octree",), "triangles"),
    # ---- flat ----------------------------------------------------------------------------------------------------------------------
    "flat_grid_kernel": Row(64, 1, ("test_flat",), "workgroup passes: ceil(corners of a plane / 256) x ceil(planes / K) (>= those of K = 4)", True, True),
    "flat_cut_scan_kernel": Row(16, 4, ("test_flat",), "wave passes of 4096 cubes: ceil((nx + 1) ny / 4096) x planes of cubes"),
    "flat_march_list_kernel": Row(6, 256, ("test_flat",), "cut cubes (>= triangles / 5)", True, True),
    # ---- dual contouring -----------------------------------------------------------------------------------------------------------
    "dc_block_test_kernel": Row(8, 256, ("test_dc_grid_clear",), "blocks of 8 x 8 x K origins, four per tile of the swept range (>= the tiles the mesh's bounding box spans)", True, True),
    "dc_grid_clear_kernel": Row(16, 1, ("test_dc_grid_clear",), "blocks of 4 x 4 x 4 tiles of the swept range (>= those the mesh's bounding box spans)", True, True),
    "dc_origin_kernel": Row(32, 1, ("test_dual_contour",), "tiles of 8 x 8 x 4 K origins of the swept range (>= those the mesh's bounding box spans)", True, True),
    "dc_edges_kernel": Row(8, 1, ("test_dual_contour",), "runs of kept cubes (>= kept cubes / 1024)", True, True),
    "dc_normals_kernel": Row(8, 4, ("test_dual_contour",), "runs of active edges, one per wave (>= active edges / 64)", True, True),
    "dc_place_kernel": Row(16, 64, ("test_dual_contour",), "kept cubes (stats.leaf_cubes); workgroups of one wave"),
    "dc_quads_kernel": Row(8, 256, ("test_dual_contour",), "active edges (stats.active_leaves)"),
    "dci_count_kernel": Row(8, 256, ("test_dual_contour_indexed",), "active edges"),
    "dci_scatter_kernel": Row(8, 256, ("test_dual_contour_indexed",), "active edges"),
    # ---- minecraft -----------------------------------------------------------------------------------------------------------------
    "mcr_positions_kernel": Row(16, 256, ("test_minecraft",), "cubes: 8^(levels - 1)", False),
    "mcr_faces_kernel": Row(16, 256, ("test_minecraft",), "cubes: 8^(levels - 1)", False),
    # ---- abi_indexed.hip -----------------------------------------------------------------------------------------------------------
    "weld_keys_kernel": Row(16, 256, ("test_indexed_chain",), "records (cut leaves): a chunk of 256 per workgroup and trip"),
    "weld_insert_kernel": Row(16, 256, ("test_indexed_chain",), "slots: 3 F"),
    "ply_verts_kernel": Row(8, 256, ("test_indexed_chain",), "words of the vertex block: 3 V (6 V with normals)"),
    "ply_faces_kernel": Row(8, 256, ("test_indexed_chain",), "words of the face block: ceil(13 F / 4)"),
    "topo_maxbits_kernel": Row(8, 256, ("test_indexed_chain",), "coordinates: 3 V"),
    "simplify_insert_kernel": Row(16, 256, ("test_indexed_chain",), "vertices"),
    "simplify_place_kernel": Row(8, 256, ("test_indexed_chain",), "cells of the cluster table (stats.table_cells)", False),
    "adaptive_insert_kernel": Row(16, 256, ("test_indexed_chain",), "vertices"),
    "adaptive_place_kernel": Row(8, 256, ("test_indexed_chain",), "cells of the cluster table (stats.table_cells)", False),
    "adaptive_named_kernel": Row(8, 256, ("test_indexed_chain",), "cluster ids (>= the clusters named: stats.n_verts)", True, True),
    "clean_vert_insert_kernel": Row(16, 256, ("test_clean_from_soup",), "vertices"),
    "clean_vert_class_kernel": Row(16, 256, ("test_clean_from_soup",), "vertices"),
    "clean_named_kernel": Row(8, 256, ("test_clean_from_soup",), "vertices"),
    # ---- constant caps: the knob does not reach them, synthetic input does ------------------------------------------------------
    # one workgroup of 1024 threads, ceil(n / 1024) counts each: n > 2048 gives every thread three
    "block_scan_kernel": Row(("wg", 1), 1024, ("test_block_scan_three_counts_per_thread",), "block counts: ceil(3 F / 256) of the faces a clean keeps"),
    "cmeas_maxbits_kernel": Row(("wg", 1024), 256, ("test_contour_measures_past_the_cap",), "coordinates: 2 V"),
}

# Launches on a constant grid that the cases above do not drive, and why.
FIXED_ELSEWHERE = {
    # 4096 (sqrt: 1024) workgroups over all 2^32 floats (atan2: 2^log2n pairs): thousands of trips in every run of their tests
    "div_selftest_kernel": "tests/test_gpu_eval.py::test_exact_division_by_uniform_divisor_exhaustive",
    "sqrt_selftest_kernel": "tests/test_gpu_eval.py::test_sqrt_unit_range_exhaustive",
    "circ_selftest_kernel": "tests/test_gpu_eval.py::test_circular_array_sector_index_without_the_angle",
    "atan2_selftest_kernel": "tests/test_gpu_eval.py::test_atan2_short_route_rounds_like_the_reference",
    "cossin_selftest_kernel": "tests/test_gpu_eval.py::test_cossin_short_route_rounds_like_the_reference_for_every_float",
    # one thread that stores one word: no loop
    "signal_kernel": "tests/test_gpu_eval.py::test_host_buffer_paths_agree_across_the_small_call_threshold",
    # One workgroup of 1024 threads, each with a serial sum over ceil(n / 1024) entries and no collective inside that loop. A
    # second entry per thread takes more than 262 144 records (weld) / 4.2 M leaves (records payload): no mesh a test can hold to
    # a twin in seconds. Same shape of loop as block_scan_kernel, which has its case.
    "weld_chunk_scan_kernel": "NOT DRIVEN past one entry per thread",
    "scan_groups_kernel": "NOT DRIVEN past one entry per thread",
}


# What reading each loop showed before its first run on one CU (uniformity of the trip count where a barrier, block_count, ballot
# or shuffle sits inside; what one trip hands the next; where per-lane sums are flushed; what blockIdx.x is assumed to be).
# No kernel had to change.
READING = {
    "eval_kernel": "base from blockIdx.x: block-uniform; sdf_eval has no barrier (per-lane LDS columns); nothing carried; lanes past n evaluate (0,0,0), store nothing",
    "normals_kernel": "as eval_kernel; three two-point evaluations per trip; nothing carried",
    "image2_kernel": "as eval_kernel; lanes past n repeat pixel n - 1 and store nothing",
    "image2_color_kernel": "as image2_kernel; the conversion's constants are formed once, before the loop",
    "view_kernel": "refilling form: claims by a wave-level append (ballot, wave-uniform exit), no workgroup barrier anywhere; per-lane evaluation count flushed once after the loop (xor-shuffle, one atomic per wave)",
    "prune_spec_kernel": "block-uniform; no collective in the loop; 32-bit base and step: n_spec <= 299 593, no wrap; the clearing loop in front is per lane",
    "prune_kernel": "block-uniform trip count; two barriers per trip guard s_w and the staged queue; `cur` is carried and is block-uniform (from LDS totals); flush() when 1024 staged and once after the loop; my_pass flushed once at the end",
    "leaf_eval_kernel": "column-brick form: the wave's own base, waves of a workgroup make different numbers of trips and the loop body has no workgroup barrier (the one barrier is above it); next cube prefetched one trip ahead (cw_next); leaf-per-lane form: block-uniform",
    "leaf_dense_kernel": "a brick per wave and trip (wave-uniform), no barrier inside",
    "march_records_kernel": "no grid-stride loop: workgroup b takes records [R b / grid, R (b + 1) / grid), a wave a quarter of them, 64 a pass; any grid works",
    "pack_records_kernel": "group g from blockIdx.x: block-uniform; shuffles and ballots only; nothing carried",
    "march_dense_kernel": "contiguous share of the chunks per workgroup (empty share: the whole workgroup returns before any barrier); the running triangle base `out` is carried and reset at a part's first chunk; barriers inside march_chunk_emit under a block-uniform count",
    "stl_kernel": "base from blockIdx.x: block-uniform; barrier after staging and after the copy: LDS is not rewritten under a reader",
    "flat_grid_kernel": "pass w from blockIdx.x: block-uniform; ballots on whole waves; nothing carried",
    "flat_cut_scan_kernel": "wave passes (wave-uniform), barriers outside the loop; early return is wave-uniform with no barrier behind it",
    "flat_march_list_kernel": "contiguous chunks of 64 records per wave; the grid is CUs x 6 whatever the list's length; wave-uniform",
    "dc_block_test_kernel": "block-uniform; no collective; one store per lane",
    "dc_grid_clear_kernel": "block B from blockIdx.x: block-uniform; three barriers per trip, the last one before s_ev / s_list are rewritten",
    "dc_origin_kernel": "tile T from blockIdx.x: block-uniform, also the `continue` of a cleared tile; __syncthreads_or opens every trip (and ends the previous trip's reads of s_w / s_base); part = blockIdx.x % 8 needs a grid that is a multiple of 8: the host rounds it up; my_evals flushed once after the loop",
    "dc_edges_kernel": "run r from blockIdx.x: block-uniform, as are the passes of a run and npend; barrier at the top of every pass; pending edges flushed per run (one atomic); descriptor of the next run prefetched; part = blockIdx.x % 8: grid rounded up to a multiple of 8 by the host",
    "dc_normals_kernel": "run per wave (wave-uniform `continue` on an empty run); no workgroup-level step",
    "dc_place_kernel": "workgroups of one wave; ring of waiting cubes in LDS carried between trips (head, tail wave-uniform); the loop ends when the list is past and the ring empty",
    "dc_quads_kernel": "block-uniform; block_append_n (barriers) once per trip",
    "dci_count_kernel": "per lane; `continue` past the list's end, no collective",
    "dci_scatter_kernel": "per lane; no collective",
    "mcr_positions_kernel": "per lane; nothing carried",
    "mcr_faces_kernel": "per lane; one atomic per cube with a face; no collective",
    "weld_keys_kernel": "chunk c from blockIdx.x: block-uniform; barrier before s_w is rewritten and after; nothing carried",
    "weld_insert_kernel": "per lane; my_probes / my_new / lost accumulate over all trips, table_stats (shuffles, every lane arrives) once after the loop",
    "ply_verts_kernel": "per lane, a word each; nothing carried",
    "ply_faces_kernel": "per lane, a word each; nothing carried",
    "topo_maxbits_kernel": "per lane maximum over all trips, wave reduction and one atomic after the loop",
    "simplify_insert_kernel": "per lane; six per-lane sums over all trips, flushed once after the loop (table_stats, then shuffles: all lanes arrive)",
    "simplify_place_kernel": "per lane; `continue` inside, the wave reduction after the loop",
    "adaptive_insert_kernel": "as simplify_insert_kernel, `levels` claims per vertex",
    "adaptive_place_kernel": "per lane; no collective",
    "adaptive_named_kernel": "per lane count, one wave reduction and atomic after the loop",
    "clean_vert_insert_kernel": "per lane; probes / new / lost over all trips, table_stats once after the loop",
    "clean_vert_class_kernel": "per lane; `merged` summed over all trips, one wave reduction after the loop",
    "clean_named_kernel": "per lane count, one wave reduction after the loop",
    "block_scan_kernel": "one workgroup: a serial sum of ceil(n / 1024) counts per thread, one wave scan, one barrier, a serial write-back; 32-bit totals (3 F < 2^32 checked by the host)",
    "cmeas_maxbits_kernel": "per lane maximum over all trips, one wave reduction and atomic after the loop",
}


def trips_of(kernel, cus):
    """The lengths of one trip of `kernel`'s loop on `cus` CUs, one per build."""
    row = GRID_TABLE[kernel]
    wgs = row.cap[1] if isinstance(row.cap, tuple) else cus * row.cap
    units = row.unit if isinstance(row.unit, tuple) else (row.unit,)
    return [wgs * u for u in units]


def check_trips(case, cus, sizes):
    """The size condition of `case`: `sizes` names exactly the kernels the table gives this case, and every n is three trips and a
    ragged tail at least (n >= 3 trip + 1, n % trip != 0; see ragged / bound above). Returns {kernel: trips}."""
    mine = {k for k, row in GRID_TABLE.items() if case in row.cases}
    assert set(sizes) == mine, (case, sorted(mine - set(sizes)), sorted(set(sizes) - mine))
    out = {}
    for kernel, n in sizes.items():
        row = GRID_TABLE[kernel]
        for trip in trips_of(kernel, cus):
            assert n >= 3 * trip + 1, (case, kernel, "n", n, "trip", trip, "needs", 3 * trip + 1)
            if row.ragged and not row.bound:
                assert n % trip != 0, (case, kernel, "n", n, "is a whole number of trips of", trip)
            out[kernel] = n / trip
    return out
