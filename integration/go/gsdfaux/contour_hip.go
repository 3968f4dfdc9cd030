//go:build cgo && hip

package gsdfaux

// contour_hip.go -- goes into github.com/soypat/gsdf/gsdfaux; built with `-tags hip`. ContourHIP traces the outline of a 2-D part
// and SliceHIP the contours of a 3-D part at the given heights, on the device (gsdf_hip_contour2 / gsdf_hip_slice3): closed loops
// in order of travel with the part on the left (outer boundaries counter-clockwise, holes clockwise), ordered by (layer, smallest
// edge key), byte for byte the same on every run. The reference has no counterpart: its only 2-D output is RenderPNGFile's picture.
// Behind the tracer: NewContourHIP takes host loops, Simplify drops vertices within a tolerance of dyadic chords and Measures sums
// the loops' areas, lengths and boxes, all on the device (gsdf_hip_contour_create / _simplify / _measures).

/*
#cgo CFLAGS: -I${SRCDIR}/../third_party/gsdf_amd/include
#cgo LDFLAGS: -L${SRCDIR}/../third_party/gsdf_amd/gsdf_amd/csrc -lgsdfhip
#include <stdlib.h>
#include "gsdf_hip.h"
*/
import "C"

import (
	"errors"
	"math"
	"runtime"

	"github.com/soypat/geometry/ms2"
	"github.com/soypat/gsdf/gleval"
)

// ContoursHIP is the result of ContourHIP / SliceHIP, copied to the host: loop q is Verts[LoopStart[q]:LoopStart[q+1]] and lies in
// layer LoopLayer[q] (an index into the heights given to SliceHIP; 0 for ContourHIP).
type ContoursHIP struct {
	Verts     []ms2.Vec
	Keys      []uint32
	LoopStart []uint32
	LoopLayer []uint32
	Layers    int
	// device time of the two stages, milliseconds
	EvalMillis, TraceMillis float64
}

// Loop returns the vertices of loop q.
func (c *ContoursHIP) Loop(q int) []ms2.Vec { return c.Verts[c.LoopStart[q]:c.LoopStart[q+1]] }

func contoursFromHandle(h *C.gsdf_contour) (*ContoursHIP, error) {
	defer C.gsdf_hip_contour_destroy(h)
	var nLayers C.uint32_t
	var nLoops, nVerts C.uint64_t
	if rc := C.gsdf_hip_contour_counts(h, &nLayers, &nLoops, &nVerts); rc != 0 {
		return nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	var st C.gsdf_contour_stats
	if rc := C.gsdf_hip_contour_stats_get(h, &st); rc != 0 {
		return nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	out := &ContoursHIP{Verts: make([]ms2.Vec, int(nVerts)), Keys: make([]uint32, int(nVerts)), LoopStart: make([]uint32, int(nLoops)+1),
		LoopLayer: make([]uint32, int(nLoops)), Layers: int(nLayers), EvalMillis: float64(st.ms_eval), TraceMillis: float64(st.ms_trace)}
	var xy *C.float
	var keys, layer *C.uint32_t
	if nVerts > 0 {
		xy = (*C.float)(&out.Verts[0].X)
		keys = (*C.uint32_t)(&out.Keys[0])
	}
	if nLoops > 0 {
		layer = (*C.uint32_t)(&out.LoopLayer[0])
	}
	rc := C.gsdf_hip_contour_read(h, xy, keys, (*C.uint32_t)(&out.LoopStart[0]), layer)
	runtime.KeepAlive(out)
	if rc != 0 {
		return nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	return out, nil
}

// ContourHIP traces the outline of the 2-D part held by sdf on a lattice of spacing res.
func ContourHIP(sdf *gleval.SDF2HIP, res float32) (*ContoursHIP, error) {
	var h *C.gsdf_contour
	rc := C.gsdf_hip_contour2((*C.gsdf_program)(sdf.Handle()), C.float(res), nil, &h)
	runtime.KeepAlive(sdf)
	if rc != 0 {
		return nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	return contoursFromHandle(h)
}

// SliceHIP traces the contours of the 3-D part held by sdf in the planes z[k], one layer per height, on an xy lattice of spacing
// res. maxNodes bounds the lattice nodes evaluated at a time (0: the library's default); the result does not depend on it.
func SliceHIP(sdf *gleval.SDF3HIP, res float32, z []float32, maxNodes uint64) (*ContoursHIP, error) {
	if len(z) == 0 {
		return nil, errors.New("gsdfaux: no slice heights")
	}
	opts := C.gsdf_contour_opts{max_nodes: C.uint64_t(maxNodes)}
	var h *C.gsdf_contour
	rc := C.gsdf_hip_slice3((*C.gsdf_program)(sdf.Handle()), C.float(res), (*C.float)(&z[0]), C.uint32_t(len(z)), &opts, &h)
	runtime.KeepAlive(sdf)
	runtime.KeepAlive(z)
	if rc != 0 {
		return nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	return contoursFromHandle(h)
}

// NewContourHIP makes a ContoursHIP of host loops (an SVG read back, or any polygons) after the checks of gsdf_hip_contour_create:
// loopStart has one entry more than there are loops, every loop has 3 vertices or more, loopLayer (nil: all 0) does not decrease
// and stays below layers, every coordinate is finite. keys may be nil (then they are 0).
func NewContourHIP(verts []ms2.Vec, loopStart, loopLayer []uint32, layers int, keys []uint32) (*ContoursHIP, error) {
	c := &ContoursHIP{Verts: verts, Keys: keys, LoopStart: loopStart, LoopLayer: loopLayer, Layers: layers}
	h, err := c.upload()
	if err != nil {
		return nil, err
	}
	return contoursFromHandle(h)
}

// upload puts the loops on the device of the calling thread; the caller destroys the handle.
func (c *ContoursHIP) upload() (*C.gsdf_contour, error) {
	if len(c.Verts) == 0 || len(c.LoopStart) < 2 {
		return nil, errors.New("gsdfaux: no loops")
	}
	nLoops := len(c.LoopStart) - 1
	if (c.Keys != nil && len(c.Keys) != len(c.Verts)) || (c.LoopLayer != nil && len(c.LoopLayer) != nLoops) {
		return nil, errors.New("gsdfaux: keys or loop layers do not match the vertices or loops")
	}
	var keys, layer *C.uint32_t
	if c.Keys != nil {
		keys = (*C.uint32_t)(&c.Keys[0])
	}
	if c.LoopLayer != nil {
		layer = (*C.uint32_t)(&c.LoopLayer[0])
	}
	var h *C.gsdf_contour
	rc := C.gsdf_hip_contour_create((*C.float)(&c.Verts[0].X), C.uint64_t(len(c.Verts)), (*C.uint32_t)(&c.LoopStart[0]), C.uint64_t(nLoops), layer, C.uint32_t(c.Layers), keys, &h)
	runtime.KeepAlive(c)
	if rc != 0 {
		return nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	return h, nil
}

// SimplifyStatsHIP says what Simplify did: everything but DeviceMillis is a function of the loops and the arguments alone.
type SimplifyStatsHIP struct {
	VertsIn, VertsOut, Loops, LoopsChanged uint64
	Spans                                  [17]uint64 // maximal acceptable spans by level, summed over passes
	MaxLevel                               int
	MaxDev                                 float64 // the largest distance of a dropped vertex to the segment that replaces it (per pass)
	DeviceMillis                           float64
}

// Simplify drops, on the device, the vertices that lie within tol of a dyadic chord of their loop (gsdf_hip_contour_simplify: the
// contract is in gsdf_hip.h). levels 1 .. 16 (0: 8), passes 1 .. 8 (0: 1); the result lies within passes x tol of c, both ways, keeps
// every loop, its first vertex and at least 3 vertices of it. c is not changed.
func (c *ContoursHIP) Simplify(tol float32, levels, passes int) (*ContoursHIP, SimplifyStatsHIP, error) {
	var stats SimplifyStatsHIP
	if len(c.LoopStart) < 2 {
		return &ContoursHIP{LoopStart: []uint32{0}, Layers: c.Layers}, stats, nil
	}
	h, err := c.upload()
	if err != nil {
		return nil, stats, err
	}
	defer C.gsdf_hip_contour_destroy(h)
	so := C.gsdf_contour_simplify_opts{tol: C.float(tol), levels: C.uint32_t(levels), passes: C.uint32_t(passes)}
	var sst C.gsdf_contour_simplify_stats
	var out *C.gsdf_contour
	if rc := C.gsdf_hip_contour_simplify(h, &so, &out, &sst); rc != 0 {
		return nil, stats, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	stats = SimplifyStatsHIP{VertsIn: uint64(sst.n_verts_in), VertsOut: uint64(sst.n_verts_out), Loops: uint64(sst.n_loops), LoopsChanged: uint64(sst.loops_changed),
		MaxLevel: int(sst.max_level), MaxDev: float64(sst.max_dev), DeviceMillis: float64(sst.ms_device)}
	for k := range stats.Spans {
		stats.Spans[k] = uint64(sst.spans[k])
	}
	res, err := contoursFromHandle(out)
	return res, stats, err
}

// LoopMeasureHIP is one loop's (one layer's) signed area (outer boundaries > 0, holes < 0), length and box.
type LoopMeasureHIP struct {
	Area, Length float64
	Min, Max     ms2.Vec
	Verts        int
	Layer        int // of a loop; of a layer: its number of loops
}

// Measures sums, on the device, area, length and box of every loop and of every layer (gsdf_hip_contour_measures): integer sums, the
// same bits whatever the order of the threads. In a layer's record Layer holds the number of its loops.
func (c *ContoursHIP) Measures() (loops, layers []LoopMeasureHIP, err error) {
	layers = make([]LoopMeasureHIP, c.Layers)
	inf := float32(math.Inf(1))
	for k := range layers {
		layers[k].Min, layers[k].Max = ms2.Vec{X: inf, Y: inf}, ms2.Vec{X: -inf, Y: -inf}
	}
	if len(c.LoopStart) < 2 {
		return nil, layers, nil
	}
	h, err := c.upload()
	if err != nil {
		return nil, nil, err
	}
	defer C.gsdf_hip_contour_destroy(h)
	lm := make([]C.gsdf_loop_measure, len(c.LoopStart)-1)
	ym := make([]C.gsdf_layer_measure, c.Layers)
	if rc := C.gsdf_hip_contour_measures(h, &lm[0], &ym[0]); rc != 0 {
		return nil, nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	loops = make([]LoopMeasureHIP, len(lm))
	for q := range lm {
		m := &lm[q]
		loops[q] = LoopMeasureHIP{Area: float64(m.area), Length: float64(m.length), Min: ms2.Vec{X: float32(m.bbox[0]), Y: float32(m.bbox[1])},
			Max: ms2.Vec{X: float32(m.bbox[2]), Y: float32(m.bbox[3])}, Verts: int(m.n_verts), Layer: int(m.layer)}
	}
	for k := range ym {
		m := &ym[k]
		layers[k] = LoopMeasureHIP{Area: float64(m.area), Length: float64(m.length), Min: ms2.Vec{X: float32(m.bbox[0]), Y: float32(m.bbox[1])},
			Max: ms2.Vec{X: float32(m.bbox[2]), Y: float32(m.bbox[3])}, Verts: int(m.n_verts), Layer: int(m.n_loops)}
	}
	return loops, layers, nil
}

// SectionHIP is gsdf_section: the section properties of one loop (one layer). First is the integral of (x, y) over the part on the
// left of the loop, Second of (x x, y y, x y), both about the origin; Central is Second about Centroid. Holes are negative, so a
// layer's record is the material's. With Area == 0 Centroid and Central are NaN.
type SectionHIP struct {
	Area     float64
	First    [2]float64
	Second   [3]float64
	Centroid [2]float64
	Central  [3]float64
	Verts    int
	Layer    int // of a loop; of a layer: its number of loops
}

func sectionOf(raw *C.gsdf_section) SectionHIP {
	var gs C.gsdf_section = *raw
	out := SectionHIP{Area: float64(gs.area), Verts: int(gs.n_verts), Layer: int(gs.layer_or_n_loops)}
	for k := 0; k < 2; k++ {
		out.First[k], out.Centroid[k] = float64(gs.first[k]), float64(gs.centroid[k])
	}
	for k := 0; k < 3; k++ {
		out.Second[k], out.Central[k] = float64(gs.second[k]), float64(gs.central[k])
	}
	return out
}

// Sections sums, on the device, the first and second moments of area of every loop and of every layer (gsdf_hip_contour_sections):
// integer sums, the same bits whatever the order of the threads. A layer without loops has Area 0 and NaN Centroid and Central.
func (c *ContoursHIP) Sections() (loops, layers []SectionHIP, err error) {
	layers = make([]SectionHIP, c.Layers)
	for k := range layers {
		layers[k].Centroid = [2]float64{math.NaN(), math.NaN()}
		layers[k].Central = [3]float64{math.NaN(), math.NaN(), math.NaN()}
	}
	if len(c.LoopStart) < 2 || c.Layers == 0 {
		return nil, layers, nil
	}
	h, err := c.upload()
	if err != nil {
		return nil, nil, err
	}
	defer C.gsdf_hip_contour_destroy(h)
	ls := make([]C.gsdf_section, len(c.LoopStart)-1)
	ys := make([]C.gsdf_section, c.Layers)
	if rc := C.gsdf_hip_contour_sections(h, &ls[0], &ys[0]); rc != 0 {
		return nil, nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	loops = make([]SectionHIP, len(ls))
	for q := range ls {
		loops[q] = sectionOf(&ls[q])
	}
	for k := range ys {
		layers[k] = sectionOf(&ys[k])
	}
	return loops, layers, nil
}
