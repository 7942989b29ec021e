package s2gpu

/*
#include <stdlib.h>
#include "kcgpu.h"
*/
import "C"

import (
	"bytes"
	"errors"
	"io"
	"sync"
	"unsafe"

	"github.com/klauspost/compress/s2"
)

// Decoder routes whole-input reads of s2.Reader and s2.Decode to the device (kc_s2_decode_streams / kc_s2_decode_blocks_all,
// include/kcgpu.h): a batch of independent inputs in one call.  A call goes to the reference when the library answers anything but
// KC_OK or there is no device, and below WithDecoderDeviceMinBytes.  Source only, like the rest of the shim.
type Decoder struct {
	device   int
	opts     *C.kc_s2_ropts
	cpuOpts  []s2.ReaderOption
	mu       sync.Mutex // one kc_ctx: one device call at a time (the reference path is concurrent)
	ctx      *C.kc_ctx
	noDevice bool
	minBytes int
}

// ReaderOption mirrors s2.ReaderOption.
type ReaderOption func(d *Decoder) error

// DefaultDecoderDeviceMinBytes: one chunk is decoded by one wave, the device pays with thousands of chunks in flight.
const DefaultDecoderDeviceMinBytes = 8 << 20

// ErrSizeExceeded: a host-buffer call met an input that does not fit the context's scratch ceiling alone (KC_S2D_SIZE_EXCEEDED).
var ErrSizeExceeded = errors.New("s2gpu: input too large for one device batch")

// The device's error classes (KC_S2D_*) as the reference's errors.
var errClass = map[C.uint32_t]error{
	C.KC_S2D_CORRUPT:       s2.ErrCorrupt,
	C.KC_S2D_CRC:           s2.ErrCRC,
	C.KC_S2D_UNSUPPORTED:   s2.ErrUnsupported,
	C.KC_S2D_SIZE_EXCEEDED: ErrSizeExceeded,
}

func boolInt(b bool) C.int {
	if b {
		return 1
	}
	return 0
}

// ReaderMaxBlockSize mirrors s2.ReaderMaxBlockSize.
func ReaderMaxBlockSize(blockSize int) ReaderOption {
	return func(d *Decoder) error {
		if C.kc_s2_ropts_max_block_size(d.opts, C.int64_t(blockSize)) != 0 {
			return errors.New("s2: block size too large. Must be <= 4MB and > 0")
		}
		d.cpuOpts = append(d.cpuOpts, s2.ReaderMaxBlockSize(blockSize))
		return nil
	}
}

// ReaderIgnoreCRC mirrors s2.ReaderIgnoreCRC.
func ReaderIgnoreCRC() ReaderOption {
	return func(d *Decoder) error {
		C.kc_s2_ropts_ignore_crc(d.opts, 1)
		d.cpuOpts = append(d.cpuOpts, s2.ReaderIgnoreCRC())
		return nil
	}
}

// ReaderIgnoreStreamIdentifier mirrors s2.ReaderIgnoreStreamIdentifier.
func ReaderIgnoreStreamIdentifier() ReaderOption {
	return func(d *Decoder) error {
		C.kc_s2_ropts_ignore_stream_identifier(d.opts, 1)
		d.cpuOpts = append(d.cpuOpts, s2.ReaderIgnoreStreamIdentifier())
		return nil
	}
}

// WithDecoderDeviceMinBytes: calls with less input than this go to the reference.
func WithDecoderDeviceMinBytes(n int) ReaderOption {
	return func(d *Decoder) error {
		d.minBytes = n
		return nil
	}
}

// NewDecoder == s2.NewReader(nil, opts...) for whole-input use.
func NewDecoder(device int, opts ...ReaderOption) (*Decoder, error) {
	d := &Decoder{device: device, minBytes: DefaultDecoderDeviceMinBytes, opts: C.kc_s2_ropts_default()}
	if d.opts == nil {
		return nil, errors.New("kc_s2_ropts_default failed")
	}
	for _, o := range opts {
		if err := o(d); err != nil {
			d.Close()
			return nil, err
		}
	}
	return d, nil
}

// Close releases the device context and the options.
func (d *Decoder) Close() {
	d.mu.Lock()
	defer d.mu.Unlock()
	if d.ctx != nil {
		C.kc_ctx_destroy(d.ctx)
		d.ctx = nil
	}
	if d.opts != nil {
		C.kc_s2_ropts_free(d.opts)
		d.opts = nil
	}
}

// DecodeStreams == N x io.ReadAll(s2.NewReader(src[off[i]:off[i+1]], opts...)) in one device batch: the decoded inputs in their
// planned layout, its offsets, and one error per input (nil: decoded).  An input that fails keeps its planned range, zero-filled:
// unlike the sequential Reader, nothing decoded in front of an error is handed out.
func (d *Decoder) DecodeStreams(src []byte, off []uint64) ([]byte, []uint64, []error) {
	n := len(off) - 1
	if n > 0 && len(src) >= d.minBytes {
		if out, oo, errs, served := d.decode(src, off, false); served {
			return out, oo, errs
		}
	}
	return decodeRef(src, off, func(in []byte) ([]byte, error) {
		return io.ReadAll(s2.NewReader(bytes.NewReader(in), d.cpuOpts...))
	})
}

// DecodeBlocks == N x s2.Decode(nil, src[off[i]:off[i+1]]) in one device batch, with the layout of DecodeStreams.
func (d *Decoder) DecodeBlocks(src []byte, off []uint64) ([]byte, []uint64, []error) {
	n := len(off) - 1
	if n > 0 && len(src) >= d.minBytes {
		if out, oo, errs, served := d.decode(src, off, true); served {
			return out, oo, errs
		}
	}
	return decodeRef(src, off, func(in []byte) ([]byte, error) { return s2.Decode(nil, in) })
}

func decodeRef(src []byte, off []uint64, one func([]byte) ([]byte, error)) ([]byte, []uint64, []error) {
	n := len(off) - 1
	if n < 0 {
		n = 0
	}
	var out []byte
	oo := make([]uint64, n+1)
	errs := make([]error, n)
	for i := 0; i < n; i++ {
		dec, err := one(src[off[i]:off[i+1]])
		if err == nil {
			out = append(out, dec...)
		}
		errs[i] = err
		oo[i+1] = uint64(len(out))
	}
	return out, oo, errs
}

// decode: the device path; served = false when the call has to go to the reference.
func (d *Decoder) decode(src []byte, off []uint64, blocks bool) ([]byte, []uint64, []error, bool) {
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
	bp := (*C.uint64_t)(unsafe.Pointer(&bound[0]))
	stp := (*C.uint32_t)(unsafe.Pointer(&status[0]))
	var st C.kc_status
	if blocks {
		st = C.kc_s2_decode_blocks_all_bound(d.ctx, sp, op, C.uint32_t(n), bp, stp)
	} else {
		st = C.kc_s2_decode_streams_bound(d.ctx, d.opts, sp, op, C.uint32_t(n), bp, stp)
	}
	if st != C.KC_OK {
		return nil, nil, nil, false
	}
	var capBytes uint64
	for _, b := range bound {
		capBytes += b
	}
	dst := make([]byte, capBytes+1)
	oo := make([]uint64, n+1)
	dp := (*C.uint8_t)(unsafe.Pointer(&dst[0]))
	oop := (*C.uint64_t)(unsafe.Pointer(&oo[0]))
	if blocks {
		st = C.kc_s2_decode_blocks_all(d.ctx, sp, op, C.uint32_t(n), dp, C.uint64_t(capBytes), oop, stp)
	} else {
		st = C.kc_s2_decode_streams(d.ctx, d.opts, sp, op, C.uint32_t(n), dp, C.uint64_t(capBytes), oop, stp)
	}
	if st != C.KC_OK { // KC_ERR_UNSUPPORTED / KC_ERR_NO_DEVICE and everything else: the reference answers
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
