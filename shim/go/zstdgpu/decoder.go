package zstdgpu

/*
#include <stdlib.h>
#include "kcgpu.h"
*/
import "C"

import (
	"errors"
	"sync"
	"unsafe"

	"github.com/klauspost/compress/zstd"
)

// Decoder routes (*zstd.Decoder).DecodeAll to the device (kc_zstd_decode_all, include/kcgpu.h): one input, or a batch of
// independent inputs in one call (DecodeUnits).  The call goes to the reference decoder when the library answers
// KC_ERR_UNSUPPORTED or there is no device, and below WithDecoderDeviceMinBytes.  Source only, like the rest of the shim.
type Decoder struct {
	device   int
	opts     *C.kc_zstd_dopts
	cpuOpts  []zstd.DOption
	cpu      *zstd.Decoder
	mu       sync.Mutex // one kc_ctx: one device call at a time (the reference path is concurrent)
	ctx      *C.kc_ctx
	noDevice bool
	minBytes int
}

// DOption mirrors zstd.DOption.
type DOption func(d *Decoder) error

// The device's error classes (KC_ZD_*) as the reference's errors.
var errClass = map[C.uint32_t]error{
	C.KC_ZD_MAGIC:           zstd.ErrMagicMismatch,
	C.KC_ZD_EOF:             errors.New("unexpected EOF"),
	C.KC_ZD_UNKNOWN_DICT:    zstd.ErrUnknownDictionary,
	C.KC_ZD_WINDOW_EXCEEDED: zstd.ErrWindowSizeExceeded,
	C.KC_ZD_SIZE_EXCEEDED:   zstd.ErrDecoderSizeExceeded,
	C.KC_ZD_CRC:             zstd.ErrCRCMismatch,
	C.KC_ZD_CORRUPT:         errors.New("zstd: corrupt input"),
}

// WithDecoderMaxMemory mirrors zstd.WithDecoderMaxMemory.
func WithDecoderMaxMemory(n uint64) DOption {
	return func(d *Decoder) error {
		if C.kc_zstd_dopts_max_memory(d.opts, C.uint64_t(n)) != 0 {
			return errors.New("WithDecoderMaxMemory: out of range")
		}
		d.cpuOpts = append(d.cpuOpts, zstd.WithDecoderMaxMemory(n))
		return nil
	}
}

// WithDecoderMaxWindow mirrors zstd.WithDecoderMaxWindow.
func WithDecoderMaxWindow(n uint64) DOption {
	return func(d *Decoder) error {
		if C.kc_zstd_dopts_max_window(d.opts, C.uint64_t(n)) != 0 {
			return errors.New("WithDecoderMaxWindow: out of range")
		}
		d.cpuOpts = append(d.cpuOpts, zstd.WithDecoderMaxWindow(n))
		return nil
	}
}

// IgnoreChecksum mirrors zstd.IgnoreChecksum.
func IgnoreChecksum(b bool) DOption {
	return func(d *Decoder) error {
		C.kc_zstd_dopts_ignore_checksum(d.opts, boolInt(b))
		d.cpuOpts = append(d.cpuOpts, zstd.IgnoreChecksum(b))
		return nil
	}
}

// WithDecoderDicts mirrors zstd.WithDecoderDicts (the library copies the bytes).
func WithDecoderDicts(dicts ...[]byte) DOption {
	return func(d *Decoder) error {
		for _, b := range dicts {
			if len(b) == 0 || C.kc_zstd_dopts_dict(d.opts, (*C.uint8_t)(unsafe.Pointer(&b[0])), C.uint64_t(len(b))) != 0 {
				return errors.New("WithDecoderDicts: dictionary rejected")
			}
		}
		d.cpuOpts = append(d.cpuOpts, zstd.WithDecoderDicts(dicts...))
		return nil
	}
}

// WithDecoderDictRaw mirrors zstd.WithDecoderDictRaw.
func WithDecoderDictRaw(id uint32, content []byte) DOption {
	return func(d *Decoder) error {
		var p *C.uint8_t
		if len(content) > 0 {
			p = (*C.uint8_t)(unsafe.Pointer(&content[0]))
		}
		if C.kc_zstd_dopts_dict_raw(d.opts, C.uint32_t(id), p, C.uint64_t(len(content))) != 0 {
			return errors.New("WithDecoderDictRaw: dictionary rejected")
		}
		d.cpuOpts = append(d.cpuOpts, zstd.WithDecoderDictRaw(id, content))
		return nil
	}
}

// WithDecoderDeviceMinBytes: calls with less input than this go to the reference decoder (default DefaultDeviceMinBytes: one frame
// is decoded by one wave, the device pays with thousands of frames in flight).
func WithDecoderDeviceMinBytes(n int) DOption {
	return func(d *Decoder) error {
		d.minBytes = n
		return nil
	}
}

// NewDecoder == zstd.NewReader(nil, opts...) for DecodeAll use.
func NewDecoder(device int, opts ...DOption) (*Decoder, error) {
	d := &Decoder{device: device, minBytes: DefaultDeviceMinBytes, opts: C.kc_zstd_dopts_default()}
	if d.opts == nil {
		return nil, errors.New("kc_zstd_dopts_default failed")
	}
	for _, o := range opts {
		if err := o(d); err != nil {
			d.Close()
			return nil, err
		}
	}
	cpu, err := zstd.NewReader(nil, d.cpuOpts...)
	if err != nil {
		d.Close()
		return nil, err
	}
	d.cpu = cpu
	return d, nil
}

// Close releases the device context, the options and the reference decoder.
func (d *Decoder) Close() {
	d.mu.Lock()
	defer d.mu.Unlock()
	if d.ctx != nil {
		C.kc_ctx_destroy(d.ctx)
		d.ctx = nil
	}
	if d.opts != nil {
		C.kc_zstd_dopts_free(d.opts)
		d.opts = nil
	}
	if d.cpu != nil {
		d.cpu.Close()
		d.cpu = nil
	}
}

// DecodeAll == (*zstd.Decoder).DecodeAll(input, dst).
func (d *Decoder) DecodeAll(input, dst []byte) ([]byte, error) {
	if len(input) < d.minBytes {
		return d.cpu.DecodeAll(input, dst)
	}
	out, off, errs, served := d.decodeUnits(input, []uint64{0, uint64(len(input))})
	if !served {
		return d.cpu.DecodeAll(input, dst)
	}
	if errs[0] != nil {
		return dst, errs[0]
	}
	return append(dst, out[off[0]:off[1]]...), nil
}

// DecodeUnits == N x DecodeAll(src[off[i]:off[i+1]], nil) in one device batch: the decoded inputs back to back, their offsets, and
// one error per input (nil: decoded).  An input that fails has an empty range.
func (d *Decoder) DecodeUnits(src []byte, off []uint64) ([]byte, []uint64, []error) {
	n := len(off) - 1
	if n > 0 && len(src) >= d.minBytes {
		if out, oo, errs, served := d.decodeUnits(src, off); served {
			return out, oo, errs
		}
	}
	var out []byte
	oo := make([]uint64, n+1)
	errs := make([]error, n)
	for i := 0; i < n; i++ {
		dec, err := d.cpu.DecodeAll(src[off[i]:off[i+1]], nil)
		if err == nil {
			out = append(out, dec...)
		}
		errs[i] = err
		oo[i+1] = uint64(len(out))
	}
	return out, oo, errs
}

// decodeUnits: the device path; served = false when the call has to go to the reference decoder.
func (d *Decoder) decodeUnits(src []byte, off []uint64) ([]byte, []uint64, []error, bool) {
	n := len(off) - 1
	if n <= 0 || len(src) == 0 {
		return nil, nil, nil, false
	}
	d.mu.Lock()
	defer d.mu.Unlock()
	if d.noDevice {
		return nil, nil, nil, false
	}
	if d.ctx == nil {
		if C.kc_ctx_create(&d.ctx, C.int(d.device), nil) != C.KC_OK {
			d.ctx = nil
			d.noDevice = true
			return nil, nil, nil, false
		}
	}
	bound := make([]uint64, n)
	status := make([]uint32, n)
	sp := (*C.uint8_t)(unsafe.Pointer(&src[0]))
	op := (*C.uint64_t)(unsafe.Pointer(&off[0]))
	stp := (*C.uint32_t)(unsafe.Pointer(&status[0]))
	if C.kc_zstd_decode_all_bound(d.ctx, d.opts, sp, op, C.uint32_t(n), (*C.uint64_t)(unsafe.Pointer(&bound[0])), stp) != C.KC_OK {
		return nil, nil, nil, false
	}
	var capBytes uint64
	for i := range bound {
		if status[i] == 0 {
			capBytes += bound[i]
		}
	}
	dst := make([]byte, capBytes+1)
	oo := make([]uint64, n+1)
	st := C.kc_zstd_decode_all(d.ctx, d.opts, sp, op, C.uint32_t(n), (*C.uint8_t)(unsafe.Pointer(&dst[0])), C.uint64_t(capBytes),
		(*C.uint64_t)(unsafe.Pointer(&oo[0])), stp)
	if st != C.KC_OK { // KC_ERR_UNSUPPORTED / KC_ERR_NO_DEVICE and everything else: the reference decoder answers
		return nil, nil, nil, false
	}
	errs := make([]error, n)
	for i := range status {
		if status[i] != 0 {
			errs[i] = errClass[C.uint32_t(status[i])]
		}
	}
	return dst[:oo[n]], oo, errs, true
}
