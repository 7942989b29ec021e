// kc_zip_dir.cpp — zip.NewReader's directory pass on the host: the end record, the zip64 locator and end record, baseOffset and the
// central directory headers of an archive held in memory (kc_zip_dir_* of include/kcgpu.h).  Needs no device and no context.
//
// Restated from zip/reader.go: Reader.init :146-207, readDirectoryHeader :386-564, readDirectoryEnd :605-682, findDirectory64End
// :687-708, readDirectory64End :712-732, findSignatureInBlock :734-750, and detectUTF8 of zip/writer.go:230-248.  The archive is the
// io.ReaderAt: a read that does not fit is io.EOF there.  The input is untrusted: every read below is checked against the buffer's
// end first, and the entry vector is reserved only under the reference's own plausibility check (:153-161).
//
// Not restated: the timestamp extras (FileHeader.Modified), NameDecoder, ErrInsecurePath (off by default in the reference).
#include <string.h>
#include <new>
#include "kc_zip_dir.h"

namespace {

enum { Z_OK = 0, Z_FORMAT, Z_UEOF /* io.ErrUnexpectedEOF */, Z_IOEOF /* io.EOF */, Z_COMMENT };

inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t rd32(const uint8_t* p) { return rd16(p) | rd16(p + 2) << 16; }
inline uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }

// detectUTF8, writer.go:230-248: *require = a rune outside 0x20 .. 0x7d or a backslash; false = not UTF-8 (utf8.DecodeRuneInString's
// rules: no overlong forms, no surrogates, nothing above U+10FFFF)
bool detect_utf8(const uint8_t* s, uint32_t n, bool* require) {
    *require = false;
    for (uint32_t i = 0; i < n;) {
        const uint32_t b = s[i];
        if (b < 0x80) {
            if (b < 0x20 || b > 0x7d || b == 0x5c) *require = true;
            i++;
            continue;
        }
        uint32_t need, lo = 0x80, hi = 0xBF;
        if (b >= 0xC2 && b <= 0xDF) need = 1;
        else if (b >= 0xE0 && b <= 0xEF) { need = 2; if (b == 0xE0) lo = 0xA0; if (b == 0xED) hi = 0x9F; }
        else if (b >= 0xF0 && b <= 0xF4) { need = 3; if (b == 0xF0) lo = 0x90; if (b == 0xF4) hi = 0x8F; }
        else return false;
        if (n - i <= need) return false;
        if (s[i + 1] < lo || s[i + 1] > hi) return false;
        for (uint32_t k = 2; k <= need; k++)
            if (s[i + k] < 0x80 || s[i + k] > 0xBF) return false;
        *require = true;
        i += need + 1;
    }
    return true;
}

// readDirectoryHeader over buf[pos, end): the entry (header offset as the directory states it) and the position behind it
int read_header(const uint8_t* buf, uint64_t pos, uint64_t end, kc_zip_entry* f, uint64_t* next) {
    if (end - pos < 46) return end == pos ? Z_IOEOF : Z_UEOF;                    // io.ReadFull, :388
    const uint8_t* b = buf + pos;
    if (rd32(b) != 0x02014b50u) return Z_FORMAT;                                // :392
    memset(f, 0, sizeof(*f));
    f->creator_version = (uint16_t)rd16(b + 4);
    f->reader_version = (uint16_t)rd16(b + 6);
    f->flags = (uint16_t)rd16(b + 8);
    f->method = (uint16_t)rd16(b + 10);
    f->modified_time = (uint16_t)rd16(b + 12);
    f->modified_date = (uint16_t)rd16(b + 14);
    f->crc32 = rd32(b + 16);
    const uint32_t csize = rd32(b + 20), usize = rd32(b + 24);
    f->compressed_size64 = csize;
    f->uncompressed_size64 = usize;
    const uint32_t nl = rd16(b + 28), el = rd16(b + 30), cl = rd16(b + 32);
    f->external_attrs = rd32(b + 38);
    const uint32_t hoff = rd32(b + 42);
    f->header_offset = (int64_t)hoff;
    const uint64_t var = (uint64_t)nl + el + cl, have = end - (pos + 46);
    if (have < var) return have == 0 ? Z_IOEOF : Z_UEOF;                        // :413
    f->name = b + 46; f->name_len = nl;
    f->extra = b + 46 + nl; f->extra_len = el;
    f->comment = b + 46 + nl + el; f->comment_len = cl;
    *next = pos + 46 + var;
    bool req1, req2;                                                            // :428-444
    const bool val1 = detect_utf8(f->name, nl, &req1), val2 = detect_utf8(f->comment, cl, &req2);
    if (!val1 || !val2) f->non_utf8 = 1;
    else if (!req1 && !req2) f->non_utf8 = 0;
    else f->non_utf8 = (f->flags & 0x800u) == 0;
    bool need_u = usize == 0xFFFFFFFFu, need_c = csize == 0xFFFFFFFFu, need_h = hoff == 0xFFFFFFFFu;  // :446-448
    const uint8_t* x = f->extra;
    uint32_t left = el;
    while (left >= 4) {                                                          // :455-491: every round takes a tag and a size
        const uint32_t tag = rd16(x), size = rd16(x + 2);
        x += 4; left -= 4;
        if (left < size) break;
        const uint8_t* fb = x;
        uint32_t fl = size;
        x += size; left -= size;
        if (tag != 0x0001u) continue;  // zip64ExtraID: only the fields that are maxed out are replaced (golang.org/issue/13367)
        if (need_u) { need_u = false; if (fl < 8) return Z_FORMAT; f->uncompressed_size64 = rd64(fb); fb += 8; fl -= 8; }
        if (need_c) { need_c = false; if (fl < 8) return Z_FORMAT; f->compressed_size64 = rd64(fb); fb += 8; fl -= 8; }
        if (need_h) { need_h = false; if (fl < 8) return Z_FORMAT; f->header_offset = (int64_t)rd64(fb); fb += 8; fl -= 8; }
    }
    // an uncompressed size of 2^32 - 1 without an extra stands (:549-557)
    if (need_c || need_h) return Z_FORMAT;                                       // :559-561
    return Z_OK;
}

struct DirEnd {
    uint64_t records = 0, size = 0, offset = 0;
    const uint8_t* comment = nullptr;
    uint32_t comment_len = 0;
};

// findSignatureInBlock, :734-750; -1: none, or the last one's comment is cut
int64_t find_signature(const uint8_t* b, uint64_t n) {
    if (n < 22) return -1;
    for (int64_t i = (int64_t)n - 22; i >= 0; i--)
        if (b[i] == 'P' && b[i + 1] == 'K' && b[i + 2] == 0x05 && b[i + 3] == 0x06) {
            const uint64_t cl = rd16(b + i + 20);
            if (cl + 22 + (uint64_t)i > n) return -1;
            return i;
        }
    return -1;
}

// readDirectoryEnd, :605-682
int read_directory_end(const uint8_t* buf, uint64_t size, DirEnd* d, int64_t* base_offset) {
    const uint8_t* blk = nullptr;
    uint64_t blen = 0;
    int64_t end_off = 0, p = -1;
    for (int i = 0; i < 2; i++) {                                                // :609-625
        blen = i == 0 ? 1024 : 65 * 1024;
        if (blen > size) blen = size;
        blk = buf + (size - blen);
        p = find_signature(blk, blen);
        if (p >= 0) { end_off = (int64_t)(size - blen) + p; break; }
        if (i == 1 || blen == size) return Z_FORMAT;
    }
    const uint8_t* b = blk + p + 4;                                              // (find_signature: at least 18 bytes follow)
    d->records = rd16(b + 6);
    d->size = rd32(b + 8);
    d->offset = rd32(b + 12);
    d->comment_len = rd16(b + 16);
    if (d->comment_len > blen - (uint64_t)p - 22) return Z_COMMENT;              // :638-641
    d->comment = b + 18;
    if (d->records == 0xffff || d->size == 0xffff || d->offset == 0xffffffffu) {  // :645-654
        const int64_t loc = end_off - 20;                                        // findDirectory64End, :687-708
        int64_t p64 = -1;
        if (loc >= 0) {                                                          // (loc + 20 = end_off <= size: the read fits)
            const uint8_t* l = buf + loc;
            if (rd32(l) == 0x07064b50u && rd32(l + 4) == 0 && rd32(l + 16) == 1) p64 = (int64_t)rd64(l + 8);
        }
        if (p64 >= 0) {
            end_off = p64;
            if (size < 56 || (uint64_t)p64 > size - 56) return Z_IOEOF;         // readDirectory64End, :712-732: the ReaderAt's io.EOF
            const uint8_t* e = buf + p64;
            if (rd32(e) != 0x06064b50u) return Z_FORMAT;
            d->records = rd64(e + 32);
            d->size = rd64(e + 40);
            d->offset = rd64(e + 48);
        }
    }
    const uint64_t max63 = ((uint64_t)1 << 63) - 1;
    if (d->size > max63 || d->offset > max63) return Z_FORMAT;                   // :656-659
    int64_t base = (int64_t)((uint64_t)end_off - d->size - d->offset);           // :661 (wraps as the reference's int64 does)
    const int64_t o = (int64_t)((uint64_t)base + d->offset);
    if (o < 0 || (uint64_t)o >= size) return Z_FORMAT;                           // :664-666
    if (base > 0 && d->offset < size) {                                          // :668-679: a valid header at baseOffset 0 wins
        kc_zip_entry probe;
        uint64_t next;
        if (read_header(buf, d->offset, size, &probe, &next) == Z_OK) base = 0;
    }
    *base_offset = base;
    return Z_OK;
}

int status_of(int z) {
    return z == Z_OK ? KC_ZIP_OK : z == Z_FORMAT ? KC_ZIP_FORMAT : z == Z_COMMENT ? KC_ZIP_COMMENT : KC_ZIP_EOF;
}

}  // namespace

extern "C" {

// zip.NewReader(bytes.NewReader(buf), len): Reader.init, :146-207
int kc_zip_dir_load(const uint8_t* buf, uint64_t len, kc_zip_dir** dir) {
    if (!dir) return KC_ZIP_FORMAT;
    *dir = nullptr;
    if (len && !buf) return KC_ZIP_FORMAT;
    DirEnd end;
    int64_t base = 0;
    int z = read_directory_end(buf, len, &end, &base);
    if (z != Z_OK) return status_of(z);
    kc_zip_dir* d = new (std::nothrow) kc_zip_dir();
    if (!d) return KC_ZIP_FORMAT;
    d->comment = end.comment;
    d->comment_len = end.comment_len;
    d->base_offset = base;
    try {
        if (end.size < len && (len - end.size) / 30 >= end.records) d->files.reserve((size_t)end.records);  // :153-161
        uint64_t pos = (uint64_t)base + end.offset;                              // (0 <= pos < len: read_directory_end)
        // every round reads one header of at least 46 bytes or stops
        for (;;) {                                                               // :176-187
            kc_zip_entry f;
            uint64_t next = pos;
            z = read_header(buf, pos, len, &f, &next);
            if (z == Z_FORMAT || z == Z_UEOF) break;
            if (z != Z_OK) { delete d; return status_of(z); }                    // io.EOF: returned as it is
            f.header_offset = (int64_t)((uint64_t)f.header_offset + (uint64_t)base);
            d->files.push_back(f);
            pos = next;
        }
    } catch (...) {
        delete d;
        return KC_ZIP_FORMAT;
    }
    if ((uint16_t)d->files.size() != (uint16_t)end.records) {                    // :188-192: sixteen bits only
        delete d;
        return status_of(z);
    }
    *dir = d;
    return KC_ZIP_OK;
}

void kc_zip_dir_free(kc_zip_dir* d) { delete d; }
uint64_t kc_zip_dir_count(const kc_zip_dir* d) { return d ? d->files.size() : 0; }
int64_t kc_zip_dir_base_offset(const kc_zip_dir* d) { return d ? d->base_offset : 0; }
const uint8_t* kc_zip_dir_comment(const kc_zip_dir* d, uint32_t* len) {
    if (len) *len = d ? d->comment_len : 0;
    return d ? d->comment : nullptr;
}
int kc_zip_dir_entry(const kc_zip_dir* d, uint64_t i, kc_zip_entry* out) {
    if (!d || !out || i >= d->files.size()) return -1;
    *out = d->files[(size_t)i];
    return 0;
}
// the member table of kc_zip_read for the entries [first, first + n): what File.Open reads of a File (:247-286)
int kc_zip_dir_members(const kc_zip_dir* d, uint64_t first, uint64_t n, kc_zip_member* out) {
    if (!d || (n && !out) || first > d->files.size() || n > d->files.size() - first) return -1;
    for (uint64_t k = 0; k < n; k++) {
        const kc_zip_entry& f = d->files[(size_t)(first + k)];
        kc_zip_member& m = out[k];
        memset(&m, 0, sizeof(m));
        m.header_offset = f.header_offset;
        m.compressed_size = f.compressed_size64;
        m.uncompressed_size = f.uncompressed_size64;
        m.crc32 = f.crc32;
        m.method = f.method;
        m.flags = f.flags;
        m.is_dir = f.name_len && f.name[f.name_len - 1] == '/';               // strings.HasSuffix(f.Name, "/"), :252
    }
    return 0;
}

}  // extern "C"
