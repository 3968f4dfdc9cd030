//go:build cgo && hip

package glrender

// hip_indexed.go -- goes into github.com/soypat/gsdf/glrender; built with `-tags hip`. An indexed triangle mesh from the device:
// the octree mesher's marching-cubes vertices welded by the lattice edge they sit on (gsdf_hip_mesh_weld), which a comparison of
// the float corners of a []ms3.Triangle cannot do (the copies of a vertex that neighbouring cubes emit differ in their last bits),
// and its binary PLY. The reference has no counterpart: its meshes are triangle lists (stl.go:15-62).

/*
#cgo CFLAGS: -I${SRCDIR}/../third_party/gsdf_amd/include
#cgo LDFLAGS: -L${SRCDIR}/../third_party/gsdf_amd/gsdf_amd/csrc -lgsdfhip
#include <stdlib.h>
#include "gsdf_hip.h"
*/
import "C"

import (
	"io"
	"unsafe"

	"github.com/soypat/geometry/ms3"
	"github.com/soypat/gsdf/gleval"
)

// IndexedHIP is a welded mesh resident on the device.
type IndexedHIP struct {
	h    *C.gsdf_indexed
	V, F uint64
	// WeldMillis is the device time of the weld.
	WeldMillis float64
}

// RenderIndexedHIP meshes s with the octree renderer at cubeResolution and welds the result on the device.
func RenderIndexedHIP(s *gleval.SDF3HIP, cubeResolution float32) (*IndexedHIP, error) {
	opts := C.gsdf_mesh_opts{prune: 1, shard_rank: 0, shard_count: 1, payload: C.GSDF_PAYLOAD_RECORDS}
	var m *C.gsdf_mesh
	if rc := C.gsdf_hip_mesh_octree(hipProgram(s), C.float(cubeResolution), &opts, &m); rc != 0 {
		return nil, hipErr(rc)
	}
	defer C.gsdf_hip_mesh_destroy(m)
	var h *C.gsdf_indexed
	if rc := C.gsdf_hip_mesh_weld(m, &h); rc != 0 {
		return nil, hipErr(rc)
	}
	ix := &IndexedHIP{h: h}
	var nv, nf C.uint64_t
	var ms C.double
	C.gsdf_hip_indexed_counts(h, &nv, &nf, &ms)
	ix.V, ix.F, ix.WeldMillis = uint64(nv), uint64(nf), float64(ms)
	return ix, nil
}

// Read copies the vertices and the faces' vertex numbers to the host.
func (ix *IndexedHIP) Read() ([]ms3.Vec, [][3]uint32, error) {
	verts := make([]ms3.Vec, ix.V)
	faces := make([][3]uint32, ix.F)
	if rc := C.gsdf_hip_indexed_read(ix.h, (*C.float)(unsafe.Pointer(&verts[0])), (*C.uint32_t)(unsafe.Pointer(&faces[0])), nil); rc != 0 {
		return nil, nil, hipErr(rc)
	}
	return verts, faces, nil
}

// Normals computes gleval.NormalsCentralDiff of s at the vertices on the device; WriteBinaryPLY carries them from then on.
func (ix *IndexedHIP) Normals(s *gleval.SDF3HIP, step float32) error {
	if rc := C.gsdf_hip_indexed_normals(ix.h, hipProgram(s), C.float(step)); rc != 0 {
		return hipErr(rc)
	}
	return nil
}

// WriteBinaryPLY writes the mesh as a binary little-endian PLY: the file is packed on the device and arrives by one DMA in
// pinned host memory the handle owns, so the Go side is one Write.
func (ix *IndexedHIP) WriteBinaryPLY(w io.Writer) (int, error) {
	var p *C.uint8_t
	var n C.size_t
	if rc := C.gsdf_hip_indexed_host_ply(ix.h, &p, &n); rc != 0 {
		return 0, hipErr(rc)
	}
	return w.Write(unsafe.Slice((*byte)(unsafe.Pointer(p)), int(n)))
}

// Close frees the device and pinned host buffers of the mesh.
func (ix *IndexedHIP) Close() {
	if ix.h != nil {
		C.gsdf_hip_indexed_destroy(ix.h)
		ix.h = nil
	}
}
