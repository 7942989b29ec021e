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
	"runtime"
	"unsafe"

	"github.com/klauspost/compress/s2"
)

// Range is one request of ReadRanges: Len decoded bytes at decoded offset Off of input Stream.
type Range struct {
	Stream uint32
	Off    uint64
	Len    uint64
}

// The ranged reads' own classes (KC_S2D_EOF, KC_S2D_UNEXPECTED_EOF) as the errors ReadAt and Skip return.
func rangeErr(status uint32) error {
	switch C.uint32_t(status) {
	case 0:
		return nil
	case C.KC_S2D_EOF:
		return io.EOF
	case C.KC_S2D_UNEXPECTED_EOF:
		return io.ErrUnexpectedEOF
	}
	return errClass[C.uint32_t(status)]
}

// IndexStream == s2.IndexStream over a stream held in memory (kc_s2_index_stream: host code, no device).
func IndexStream(stream []byte) ([]byte, error) {
	var sp *C.uint8_t
	if len(stream) > 0 {
		sp = (*C.uint8_t)(unsafe.Pointer(&stream[0]))
	}
	out := make([]byte, 64+20*(len(stream)>>20+2))
	for {
		var n C.uint64_t
		var st C.uint32_t
		rc := C.kc_s2_index_stream(sp, C.uint64_t(len(stream)), (*C.uint8_t)(unsafe.Pointer(&out[0])), C.uint64_t(len(out)), &n, &st)
		if rc == C.KC_ERR_DST_TOO_SMALL {
			out = make([]byte, int(n))
			continue
		}
		if rc != C.KC_OK {
			return s2.IndexStream(bytes.NewReader(stream))
		}
		if st != 0 {
			return nil, rangeErr(uint32(st))
		}
		return out[:n], nil
	}
}

// ReadRanges == for every request ReadSeeker.ReadAt(make([]byte, Len), Off) of s2.NewReader(src[off[Stream]:off[Stream+1]], opts...)
// in one device batch (kc_s2_read_ranges).  indexes holds per input the bytes of its index, or nil: that input is walked from its
// start.  Request j owns out[oo[j]:oo[j+1]] (oo: the prefix sum of the lengths), of which got[j] bytes are data; errs[j] is nil,
// io.EOF for a short read, io.ErrUnexpectedEOF or the reference's error.  served = false: the caller uses the reference.
func (d *Decoder) ReadRanges(src []byte, off []uint64, indexes [][]byte, reqs []Range) (out []byte, oo []uint64, got []uint64, errs []error, served bool) {
	n, m := len(off)-1, len(reqs)
	if n <= 0 || m == 0 || len(src) == 0 {
		return nil, nil, nil, nil, false
	}
	d.mu.Lock()
	defer d.mu.Unlock()
	if d.noDevice {
		return nil, nil, nil, nil, false
	}
	if d.ctx == nil {
		if C.kc_ctx_create(&d.ctx, C.int(d.device), nil) != C.KC_OK {
			d.ctx = nil
			d.noDevice = true
			return nil, nil, nil, nil, false
		}
	}
	// the index handles live in C memory: no Go pointer is stored where C keeps it
	hp := (**C.kc_s2_index)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	defer C.free(unsafe.Pointer(hp))
	handles := unsafe.Slice(hp, n)
	defer func() {
		for _, h := range handles {
			if h != nil {
				C.kc_s2_index_free(h)
			}
		}
	}()
	for i := 0; i < n && i < len(indexes); i++ {
		if len(indexes[i]) == 0 {
			continue
		}
		h := C.kc_s2_index_new()
		if h == nil {
			return nil, nil, nil, nil, false
		}
		handles[i] = h
		if C.kc_s2_index_load(h, (*C.uint8_t)(unsafe.Pointer(&indexes[i][0])), C.uint64_t(len(indexes[i])), nil) != C.KC_S2I_OK {
			return nil, nil, nil, nil, false // the reference reports what is wrong with the index
		}
	}
	rs := make([]uint32, m)
	ro := make([]uint64, m)
	rl := make([]uint64, m)
	var total uint64
	for j, r := range reqs {
		rs[j], ro[j], rl[j] = r.Stream, r.Off, r.Len
		total += r.Len
	}
	out = make([]byte, total+1)
	oo = make([]uint64, m+1)
	got = make([]uint64, m)
	status := make([]uint32, m)
	st := C.kc_s2_read_ranges(d.ctx, d.opts, (*C.uint8_t)(unsafe.Pointer(&src[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])), C.uint32_t(n), hp,
		(*C.uint32_t)(unsafe.Pointer(&rs[0])), (*C.uint64_t)(unsafe.Pointer(&ro[0])), (*C.uint64_t)(unsafe.Pointer(&rl[0])), C.uint32_t(m),
		(*C.uint8_t)(unsafe.Pointer(&out[0])), C.uint64_t(total), (*C.uint64_t)(unsafe.Pointer(&oo[0])), (*C.uint64_t)(unsafe.Pointer(&got[0])),
		(*C.uint32_t)(unsafe.Pointer(&status[0])))
	runtime.KeepAlive(indexes)
	if st != C.KC_OK {
		return nil, nil, nil, nil, false
	}
	errs = make([]error, m)
	for j := range status {
		errs[j] = rangeErr(status[j])
	}
	return out[:total], oo, got, errs, true
}

// ReadSeeker == s2.ReadSeeker over a whole input held in memory: ReadAt / Seek / Read through Decoder.ReadRanges, the reference's own
// ReadSeeker behind it when the device does not serve a call.
type ReadSeeker struct {
	d     *Decoder
	src   []byte
	index []byte
	total int64
	pos   int64
	ref   *s2.ReadSeeker
}

// NewReadSeeker == s2.NewReader(bytes.NewReader(src), opts...).ReadSeeker(true, index): a supplied index wins, else the one at the
// end of src is used; without either the reference's ErrCantSeek is returned.
func (d *Decoder) NewReadSeeker(src []byte, index []byte) (*ReadSeeker, error) {
	ref, err := s2.NewReader(bytes.NewReader(src), d.cpuOpts...).ReadSeeker(true, index)
	if err != nil {
		return nil, err
	}
	r := &ReadSeeker{d: d, src: src, index: index, ref: ref}
	var ix s2.Index
	if len(index) != 0 {
		_, err = ix.Load(index)
	} else {
		err = ix.LoadStream(bytes.NewReader(src))
		if err == nil && len(src) >= 10 { // the index chunk at the end of src
			sz := int(src[len(src)-10]) | int(src[len(src)-9])<<8 | int(src[len(src)-8])<<16 | int(src[len(src)-7])<<24
			if sz <= len(src) {
				r.index = src[len(src)-sz:]
			}
		}
	}
	if err != nil {
		return nil, err
	}
	r.total = ix.TotalUncompressed
	return r, nil
}

// ReadAt implements io.ReaderAt; like the reference's, it moves the position Read continues from.
func (r *ReadSeeker) ReadAt(p []byte, off int64) (int, error) {
	if off < 0 {
		return 0, errors.New("seek before start of file")
	}
	if len(p) >= r.d.minBytes || r.d.minBytes == 0 {
		out, _, got, errs, served := r.d.ReadRanges(r.src, []uint64{0, uint64(len(r.src))}, [][]byte{r.index}, []Range{{0, uint64(off), uint64(len(p))}})
		if served {
			if errs[0] != nil && errs[0] != io.EOF {
				return 0, errs[0]
			}
			n := copy(p, out[:got[0]])
			r.pos = off + int64(n)
			return n, errs[0]
		}
	}
	n, err := r.ref.ReadAt(p, off)
	r.pos = off + int64(n)
	return n, err
}

// Seek implements io.Seeker.
func (r *ReadSeeker) Seek(offset int64, whence int) (int64, error) {
	abs := offset
	switch whence {
	case io.SeekStart:
	case io.SeekCurrent:
		abs = r.pos + offset
	case io.SeekEnd:
		abs = r.total + offset
	default:
		return 0, s2.ErrUnsupported
	}
	if abs < 0 {
		return 0, errors.New("seek before start of file")
	}
	if abs > r.total {
		return r.pos, io.ErrUnexpectedEOF
	}
	r.pos = abs
	return abs, nil
}

// Read implements io.Reader from the current position.
func (r *ReadSeeker) Read(p []byte) (int, error) {
	if len(p) == 0 {
		return 0, nil
	}
	n, err := r.ReadAt(p, r.pos)
	if n > 0 && err == io.EOF {
		err = nil
	}
	return n, err
}
