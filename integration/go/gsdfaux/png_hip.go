//go:build cgo && hip

package gsdfaux

// png_hip.go -- goes into github.com/soypat/gsdf/gsdfaux; built with `-tags hip`. RenderPNGFileHIP is RenderPNGFile
// (gsdfaux.go:264-296) with the picture rendered and its colours converted on the device by gsdf_hip_image2_color: the same
// picture size, the same default conversion (ColorConversionInigoQuilez of the bounds' diagonal / 3), the same PNG encoder.
// The conversions are ColorHIP values rather than func(float32) color.Color: an arbitrary Go function cannot run on the device.
// A caller with a conversion of its own takes the distances from gsdf_hip_image2 (dist_out) and converts them on the host.

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
	"image/color"
	"image/png"
	"os"
	"runtime"

	"github.com/soypat/gsdf/gleval"
)

// ColorHIP is one of gsdfaux's colour conversions in the form the device takes (gsdf_color2).
type ColorHIP struct {
	c C.gsdf_color2
}

func hipError() error { return errors.New("gsdf_hip: " + C.GoString(C.gsdf_hip_last_error())) }

// ColorConversionInigoQuilezHIP is ColorConversionInigoQuilez(charDist) (color.go:21-46) on the device.
func ColorConversionInigoQuilezHIP(charDist float32) (*ColorHIP, error) {
	if !(charDist > 0) {
		return nil, errors.New("gsdfaux: characteristic distance must be > 0")
	}
	var conv ColorHIP
	if rc := C.gsdf_hip_color_iq(nil, C.float(charDist), &conv.c); rc != 0 {
		return nil, hipError()
	}
	return &conv, nil
}

// ColorConversionLinearGradientHIP is ColorConversionLinearGradient(length, c0, c1) (color.go:50-71) on the device. The end
// colours go through color.RGBAModel, as image.RGBA stores them; color.Black to color.White selects the black-and-white
// conversion, as the reference's identity test does.
func ColorConversionLinearGradientHIP(length float32, c0, c1 color.Color) (*ColorHIP, error) {
	a := color.RGBAModel.Convert(c0).(color.RGBA)
	b := color.RGBAModel.Convert(c1).(color.RGBA)
	ca := [4]C.uint8_t{C.uint8_t(a.R), C.uint8_t(a.G), C.uint8_t(a.B), C.uint8_t(a.A)}
	cb := [4]C.uint8_t{C.uint8_t(b.R), C.uint8_t(b.G), C.uint8_t(b.B), C.uint8_t(b.A)}
	var conv ColorHIP
	if rc := C.gsdf_hip_color_gradient(C.float(length), &ca[0], &cb[0], &conv.c); rc != 0 {
		return nil, hipError()
	}
	if c0 == color.Black && c1 == color.White {
		conv.c.kind = C.GSDF_COLOR_BW_SMOOTH
	} else {
		conv.c.kind = C.GSDF_COLOR_GRADIENT
	}
	return &conv, nil
}

// RenderPNGFileHIP renders the 2-D part held by sdf as RenderPNGFile does and writes it to filename; a nil conv selects
// RenderPNGFile's default, ColorConversionInigoQuilez(bb.Diagonal() / 3).
func RenderPNGFileHIP(filename string, sdf *gleval.SDF2HIP, picHeight int, conv *ColorHIP) error {
	box := sdf.Bounds()
	bb := [6]C.float{C.float(box.Min.X), C.float(box.Min.Y), 0, C.float(box.Max.X), C.float(box.Max.Y), 0}
	var w C.int
	if rc := C.gsdf_hip_picture_size(&bb[0], C.int(picHeight), &w); rc != 0 {
		return hipError()
	}
	if conv == nil {
		conv = &ColorHIP{}
		if rc := C.gsdf_hip_color_iq(&bb[0], 0, &conv.c); rc != 0 {
			return hipError()
		}
	}
	img := image.NewRGBA(image.Rect(0, 0, int(w), picHeight))
	rc := C.gsdf_hip_image2_color((*C.gsdf_program)(sdf.Handle()), &conv.c, w, C.int(picHeight), (*C.uint8_t)(&img.Pix[0]), nil)
	runtime.KeepAlive(sdf)
	runtime.KeepAlive(img)
	if rc != 0 {
		return hipError()
	}
	fp, err := os.Create(filename)
	if err != nil {
		return err
	}
	defer fp.Close()
	if err = png.Encode(fp, img); err != nil {
		return err
	}
	return fp.Sync()
}
