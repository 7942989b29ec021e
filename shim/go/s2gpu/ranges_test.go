package s2gpu

import (
	"bytes"
	"io"
	"math/rand"
	"testing"

	"github.com/klauspost/compress/kcgpu"
	"github.com/klauspost/compress/s2"
)

// TestReadRanges: ReadSeeker.ReadAt through the device == the reference's ReadSeeker.ReadAt on the same indexed stream, and
// IndexStream == s2.IndexStream.  Written, not run here, like the rest of the shim.
func TestReadRanges(t *testing.T) {
	data, err := kcgpu.CorpusFill('T', kcgpu.Seed('T'), 0, 64, 64<<10)
	if err != nil {
		t.Fatal(err)
	}
	var buf bytes.Buffer
	w := s2.NewWriter(&buf, s2.WriterBlockSize(64<<10), s2.WriterAddIndex())
	if _, err := w.Write(data); err != nil {
		t.Fatal(err)
	}
	if err := w.Close(); err != nil {
		t.Fatal(err)
	}
	stream := buf.Bytes()

	var plain bytes.Buffer
	w = s2.NewWriter(&plain, s2.WriterBlockSize(64<<10))
	w.Write(data)
	w.Close()
	want, err := s2.IndexStream(bytes.NewReader(plain.Bytes()))
	if err != nil {
		t.Fatal(err)
	}
	got, err := IndexStream(plain.Bytes())
	if err != nil || !bytes.Equal(got, want) {
		t.Fatalf("IndexStream differs from s2.IndexStream (%v)", err)
	}

	d, err := NewDecoder(0, WithDecoderDeviceMinBytes(0))
	if err != nil {
		t.Skip(err)
	}
	defer d.Close()
	rs, err := d.NewReadSeeker(stream, nil)
	if err != nil {
		t.Fatal(err)
	}
	ref, err := s2.NewReader(bytes.NewReader(stream)).ReadSeeker(true, nil)
	if err != nil {
		t.Fatal(err)
	}
	rnd := rand.New(rand.NewSource(1))
	for i := 0; i < 200; i++ {
		off := rnd.Int63n(int64(len(data)) + 1)
		n := rnd.Intn(200000)
		a, b := make([]byte, n), make([]byte, n)
		na, ea := rs.ReadAt(a, off)
		nb, eb := ref.ReadAt(b, off)
		if na != nb || (ea == io.EOF) != (eb == io.EOF) || (ea == nil) != (eb == nil) || !bytes.Equal(a[:na], b[:nb]) {
			t.Fatalf("ReadAt(%d bytes, %d): device %d %v, reference %d %v", n, off, na, ea, nb, eb)
		}
	}
	if p, err := rs.Seek(-100, io.SeekEnd); err != nil || p != int64(len(data))-100 {
		t.Fatal(p, err)
	}
	tail, err := io.ReadAll(rs)
	if err != nil || !bytes.Equal(tail, data[len(data)-100:]) {
		t.Fatalf("Read after Seek: %d bytes, %v", len(tail), err)
	}
}
