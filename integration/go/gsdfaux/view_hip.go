//go:build cgo && hip

package gsdfaux

// view_hip.go -- goes into github.com/soypat/gsdf/gsdfaux; built with `-tags hip`. RenderViewHIP is one frame of the UI's
// ray-marched view (ui.go:247-355) without a window: the orbit camera of ui.go:276-297 at the UI's default distance (camDist <= 0)
// or the one given, rendered on the device by gsdf_hip_render3 into an image.RGBA (row 0 at the top).

/*
#cgo CFLAGS: -I${SRCDIR}/../third_party/gsdf_amd/include
#cgo LDFLAGS: -L${SRCDIR}/../third_party/gsdf_amd/gsdf_amd/csrc -lgsdfhip
#include <stdlib.h>
#include "gsdf_hip.h"
*/
import "C"

import (
	"errors"
	"image"
	"runtime"

	"github.com/soypat/gsdf/gleval"
)

// RenderViewHIP renders the part held by sdf as the UI shows it with the mouse at rest after a drag to (yaw, pitch), in radians,
// with one sample per pixel; camDist <= 0 selects the UI's default (the bounds' diagonal).
func RenderViewHIP(sdf *gleval.SDF3HIP, w, h int, yaw, pitch, camDist float32) (*image.RGBA, error) {
	if w <= 0 || h <= 0 {
		return nil, errors.New("gsdfaux: bad image size")
	}
	box := sdf.Bounds()
	bb := [6]C.float{C.float(box.Min.X), C.float(box.Min.Y), C.float(box.Min.Z), C.float(box.Max.X), C.float(box.Max.Y), C.float(box.Max.Z)}
	var view C.gsdf_view
	if rc := C.gsdf_hip_view_orbit(&bb[0], C.float(yaw), C.float(pitch), C.float(camDist), nil, &view); rc != 0 {
		return nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	view.aa = 1
	img := image.NewRGBA(image.Rect(0, 0, w, h))
	rc := C.gsdf_hip_render3((*C.gsdf_program)(sdf.Handle()), &view, C.int(w), C.int(h), (*C.uint8_t)(&img.Pix[0]), nil, nil)
	runtime.KeepAlive(sdf)
	runtime.KeepAlive(img)
	if rc != 0 {
		return nil, errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error()))
	}
	return img, nil
}
