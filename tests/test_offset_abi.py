"""The offset's C ABI (include/gsdf_hip.h, section "contours: offset") without a GPU: the two symbols in the built library, the ctypes
records with the header's sizes and offsets, the header's own layout asserts."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsdf_hip_contour_offset", "gsdf_hip_contour_distance")


def test_the_library_exports_the_two_symbols():
    lib = os.path.join(ROOT, "gsdf_amd", "csrc", "libgsdfhip.so")
    assert os.path.exists(lib), "build first: python __graft_entry__.py"
    dll = C.CDLL(lib)
    for s in SYMBOLS:
        assert hasattr(dll, s), s


def test_the_python_records_have_the_header_s_layout():
    from gsdf_amd import hip
    o, st = hip.OffsetOpts, hip.OffsetStats
    assert C.sizeof(o) == 56
    assert (o.res.offset, o.n_insets.offset, o.dry.offset, o.reserved.offset, o.max_nodes.offset, o.inset.offset) == (0, 4, 8, 12, 16, 24)
    assert C.sizeof(st) == 104 and st.RESULT_BYTES == 80 == st.ms_field.offset
    assert (st.n_verts.offset, st.n_loops.offset, st.border_inside.offset, st.saddle_cells.offset, st.inside_nodes.offset, st.band_nodes.offset) == (0, 8, 16, 24, 32, 40)
    assert (st.nx.offset, st.ny.offset, st.n_layers_in.offset, st.n_insets.offset, st.x0.offset, st.y0.offset, st.band.offset, st.res.offset) == (48, 52, 56, 60, 64, 68, 72, 76)
    assert (st.ms_trace.offset, st.ms_device.offset) == (88, 96)
    for s in SYMBOLS:
        assert s in hip.SYMBOLS
        getattr(hip.lib(), s)
    hdr = open(os.path.join(ROOT, "include", "gsdf_hip.h")).read()
    for text in ("sizeof(gsdf_offset_opts) == 56", "offsetof(gsdf_offset_opts, inset) == 24", "sizeof(gsdf_offset_stats) == 104", "offsetof(gsdf_offset_stats, ms_field) == 80"):
        assert text in hdr, text
    for s in SYMBOLS:
        assert "int %s(const gsdf_contour* c, const gsdf_offset_opts* o, " % s in hdr


def test_the_twin_packs_the_same_eighty_bytes():
    import offsetref as O
    from gsdf_amd import hip
    assert C.sizeof(hip.OffsetStats) - 24 == 80 == len(O.stats_bytes(dict.fromkeys(("n_verts", "n_loops", "border_inside", "saddle_cells", "inside_nodes", "band_nodes", "nx", "ny",
                                                                                   "n_layers_in", "n_insets", "x0", "y0", "band", "res"), 1)))
