//go:build cgo && hip

package gsdfaux

// contour_hip.go -- goes into github.com/soypat/gsdf/gsdfaux; built with `-tags hip`. ContourHIP traces the outline of a 2-D part
// and SliceHIP the contours of a 3-D part at the given heights, on the device (gsdf_hip_contour2 / gsdf_hip_slice3): closed loops
// in order of travel with the part on the left (outer boundaries counter-clockwise, holes clockwise), ordered by (layer, smallest
// edge key), byte for byte the same on every run. The reference has no counterpart: its only 2-D output is RenderPNGFile's picture.

/*
#cgo CFLAGS: -I${SRCDIR}/../third_party/gsdf_amd/include
#cgo LDFLAGS: -L${SRCDIR}/../third_party/gsdf_amd/gsdf_amd/csrc -lgsdfhip
#include <stdlib.h>
#include "gsdf_hip.h"
*/
import "C"

import (
	"errors"
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
