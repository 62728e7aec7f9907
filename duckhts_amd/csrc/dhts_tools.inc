// dhts_tools.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// bgzip / bgunzip / BGZF wrap.
// ---- bgzip / bgunzip (src/bgzip.c: bgzf_write / bgzf_read loops, htslib bgzf.c) ----------------------------------------------------------
static const uint8_t BGZF_EOF_BLOCK[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
// raw bytes already in z_in (n of them, padded; `in`: where in z_in they start, null for its front) -> packed BGZF blocks in z_out; *out_len = their size
static int bgzf_compress_device(dhts_ctx *c, uint64_t n, int level, uint64_t *out_len, const uint8_t *in = nullptr) {
    const int64_t nblk = (int64_t)((n + DFL_IN - 1) / DFL_IN);
    *out_len = 0;
    if (nblk == 0) return 0;
    ENSURE(c, c->z_slots, (size_t)nblk * DFL_SLOT + 64); ENSURE(c, c->z_sizes, (size_t)(nblk + 1) * 4 + 64); ENSURE(c, c->z_offs, (size_t)(nblk + 2) * 8 + 64);
    if (level != 0) ENSURE(c, c->z_tok, (size_t)nblk * DFL_IN * 4 + 64);                  // the parse of every block: one word per token
    hipLaunchKernelGGL(bgzf_deflate_blocks, dim3((unsigned)nblk), dim3(64), DFL_LDS_BYTES, c->stream, in ? in : (const uint8_t *)c->z_in.p, n, nblk, level, (uint8_t *)c->z_slots.p, (uint32_t *)c->z_sizes.p,
                       (uint32_t *)c->z_tok.p);
    HIPCHK(c, hipGetLastError());
    const uint32_t *in1[1] = {(const uint32_t *)c->z_sizes.p}; uint64_t *o64[1] = {(uint64_t *)c->z_offs.p}; uint64_t total = 0;
    if (run_scan(c, 1, in1, nullptr, o64, nblk, &total)) return -1;
    ENSURE(c, c->z_out, total + 64);
    hipLaunchKernelGGL(bgzf_pack_blocks, dim3((unsigned)nblk), dim3(64), 0, c->stream, (const uint8_t *)c->z_slots.p, (const uint32_t *)c->z_sizes.p, (const uint64_t *)c->z_offs.p, nblk, (uint8_t *)c->z_out.p);
    HIPCHK(c, hipGetLastError());
    *out_len = total;
    return 0;
}
// GPU bgzip of a host buffer: one BGZF block per 0xff00 input bytes + the EOF block.  Returns the file size; with out == NULL or cap too small
// nothing is written and the return value is an upper bound (call twice).  level 0 stores, 1..9 (and -1) compress (one setting).
extern "C" int64_t dhts_bgzf_compress(dhts_ctx *c, const void *raw, uint64_t n, int level, void *out, uint64_t cap) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t nblk = (n + DFL_IN - 1) / DFL_IN, bound = n + nblk * 31 + 28;
    if (!out || cap < bound) return (int64_t)bound;
    if (n >= (1ull << 40)) return fail(c, "input too large");
    uint64_t done = 0, at = 0;
    const uint64_t CH = (uint64_t)DFL_IN * 4096;                                  // 267 MB of input per launch
    while (done < n) {
        const uint64_t m = n - done < CH ? n - done : CH;
        ENSURE(c, c->z_in, m + PAD_BYTES);
        HIPCHK(c, hipMemcpyAsync(c->z_in.p, (const uint8_t *)raw + done, m, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync((uint8_t *)c->z_in.p + m, 0, PAD_BYTES, c->stream));
        uint64_t ol = 0;
        if (bgzf_compress_device(c, m, level, &ol)) return -1;
        if (at + ol + 28 > cap) return fail(c, "internal: compressed size above its bound");
        HIPCHK(c, hipMemcpyAsync((uint8_t *)out + at, c->z_out.p, ol, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        at += ol; done += m;
    }
    memcpy((uint8_t *)out + at, BGZF_EOF_BLOCK, 28);
    return (int64_t)(at + 28);
}
// tests: dfl_build_lengths + dfl_assign_codes of the encoder on ncases count vectors of nsym symbols each (host arrays; one launch, one wave per
// case).  The caller answers for count vectors the builder's loops end on (tests/deflate_code_ref.py carries each through first); what can
// be refused here is: a total that does not fit 32 bits, more symbols than maxbits can code.
extern "C" int dhts_debug_deflate_codes(dhts_ctx *c, const uint32_t *counts, uint32_t nsym, uint32_t maxbits, int64_t ncases, uint8_t *lens_out, uint32_t *codes_out) {
    if (!c) return -1;
    if (!counts || !lens_out || !codes_out || nsym < 2u || nsym > 288u || maxbits < 1u || maxbits > 15u || (uint64_t)nsym > (1ull << maxbits) || ncases < 0 || ncases > (1 << 20))
        return fail(c, "debug_deflate_codes: arguments out of range");
    if (ncases == 0) return 0;
    for (int64_t k = 0; k < ncases; k++) {
        uint64_t t = 0; for (uint32_t s = 0; s < nsym; s++) t += counts[(uint64_t)k * nsym + s];
        if (t >> 32) return fail(c, "debug_deflate_codes: the counts of case %lld do not fit 32 bits", (long long)k);
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nw = (size_t)ncases * nsym;
    ENSURE(c, c->z_in, nw * 4 + 64); ENSURE(c, c->z_out, nw + 64); ENSURE(c, c->z_tok, nw * 4 + 64);
    HIPCHK(c, hipMemcpyAsync(c->z_in.p, counts, nw * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bgzf_deflate_debug_codes, dim3((unsigned)ncases), dim3(64), 0, c->stream, (const uint32_t *)c->z_in.p, nsym, maxbits, ncases, (uint8_t *)c->z_out.p, (uint32_t *)c->z_tok.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(lens_out, c->z_out.p, nw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(codes_out, c->z_tok.p, nw * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// bgzip(path): file -> BGZF file (bgzip.c:231-293).  Returns 0, -2 input cannot be opened, -3 output cannot be opened, -4 read error, -5 write error.
extern "C" int dhts_bgzip_file(dhts_ctx *c, const char *in_path, const char *out_path, int level, int64_t *bytes_in, int64_t *bytes_out) {
    if (!c || !in_path || !out_path) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    const int fd = open(in_path, O_RDONLY);
    if (fd < 0) { fail(c, "bgzip: cannot open input %s: %s", in_path, strerror(errno)); return -2; }
    FILE *fo = fopen(out_path, "wb");
    if (!fo) { close(fd); fail(c, "bgzip: cannot open output %s", out_path); return -3; }
    const uint64_t CH = (uint64_t)DFL_IN * 4096;                                  // 267 MB of input per launch
    uint8_t *pin = (uint8_t *)dhts_host_alloc(CH + CH / 1024 + (1u << 20));
    int rc = 0; int64_t nin = 0, nout = 0;
    if (!pin) { rc = -1; fail(c, "bgzip: out of pinned memory"); }
    if (level < 0 || level > 9) level = -1;
    while (rc == 0) {
        size_t got = 0;
        while (got < CH) { const ssize_t r = read(fd, pin + got, CH - got); if (r < 0) { rc = -4; fail(c, "bgzip: read error"); break; } if (r == 0) break; got += (size_t)r; }
        if (rc || got == 0) break;
        uint64_t ol = 0;
        if (c->z_in.ensure(got + PAD_BYTES)) { rc = -1; fail(c, "hipMalloc failed"); break; }
        if (hipMemcpyAsync(c->z_in.p, pin, got, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipMemsetAsync((uint8_t *)c->z_in.p + got, 0, PAD_BYTES, c->stream) != hipSuccess ||
            bgzf_compress_device(c, got, level == 0 ? 0 : 6, &ol) || hipMemcpyAsync(pin, c->z_out.p, ol, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
            rc = -1; if (!*dhts_error(c)) fail(c, "bgzip: device error"); break;
        }
        if (fwrite(pin, 1, ol, fo) != ol) { rc = -5; fail(c, "bgzip: write error"); break; }
        nin += (int64_t)got; nout += (int64_t)ol;
        if (got < CH) break;
    }
    if (rc == 0 && fwrite(BGZF_EOF_BLOCK, 1, 28, fo) != 28) { rc = -5; fail(c, "bgzip: write error"); }
    if (rc == 0) nout += 28;
    if (pin) dhts_host_free(pin);
    close(fd);
    if (fclose(fo) != 0 && rc == 0) { rc = -5; fail(c, "bgzip: close error"); }
    if (rc) unlink(out_path);
    if (bytes_in) *bytes_in = nin;
    if (bytes_out) *bytes_out = nout;
    return rc;
}
// bgunzip(path): BGZF file -> the bytes it holds (bgzip.c:167-230: bgzf_read until 0).  Blocks are inflated on the device in batches.
// Returns 0, -2 input cannot be opened / is not BGZF, -3 output cannot be opened, -4 a block failed (the reference: "bgunzip: read error"), -5 write error.
extern "C" int dhts_bgunzip_file(dhts_ctx *c, const char *in_path, const char *out_path, int64_t *bytes_in, int64_t *bytes_out) {
    if (!c || !in_path || !out_path) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    {
        // a file that is not gzip at all is handed through as it is (bgzf_open "r" reads such a file transparently, bgzf.c:412-450, so the
        // reference's bgunzip copies it): nothing to inflate, the copy is plain file I/O
        const int fd = open(in_path, O_RDONLY);
        if (fd < 0) { fail(c, "bgunzip: cannot open input %s", in_path); return -2; }
        uint8_t magic[2] = {0, 0}; const ssize_t got = pread(fd, magic, 2, 0);
        if (got >= 0 && !(got == 2 && magic[0] == 0x1f && magic[1] == 0x8b)) {   // (a file shorter than the magic is not gzip either)
            FILE *fo = fopen(out_path, "wb");
            if (!fo) { close(fd); fail(c, "bgunzip: cannot open output %s: %s", out_path, strerror(errno)); return -3; }
            std::vector<uint8_t> buf(1u << 20); int rc = 0; int64_t n = 0;
            for (;;) { const ssize_t r = read(fd, buf.data(), buf.size()); if (r < 0) { rc = -4; fail(c, "bgunzip: read error"); break; } if (r == 0) break;
                       if (fwrite(buf.data(), 1, (size_t)r, fo) != (size_t)r) { rc = -5; fail(c, "bgunzip: write error"); break; } n += r; }
            close(fd);
            if (fclose(fo) != 0 && rc == 0) { rc = -5; fail(c, "bgunzip: write error"); }
            if (rc) unlink(out_path);                        // no partial output behind an error
            if (bytes_in) *bytes_in = n;
            if (bytes_out) *bytes_out = n;
            return rc;
        }
        close(fd);
    }
    if (dhts_open_path(c, in_path) != 0) return -2;
    c->gz_any = true;                                        // plain gzip: bgzf_read inflates it through zlib (bgzf.c:828-893); here the serial device decoder does
    const int64_t nb = dhts_bgzf_index(c);
    c->gz_any = false;
    if (nb < 0 || (nb == 0 && c->comp_len > 0 && !c->gz_plain)) { if (nb == 0) fail(c, "bgunzip: %s is gzip but holds no BGZF block", in_path); return -2; }
    if (c->bgzf_status != 0) { fail(c, "bgunzip: read error"); return -4; }
    FILE *fo = fopen(out_path, "wb");
    if (!fo) { fail(c, "bgunzip: cannot open output %s: %s", out_path, strerror(errno)); return -3; }
    const int64_t B = 4096;
    // (room for B blocks of 64 KiB each, whatever their ISIZE fields say: the block table is corrected from the decoded lengths as phase A
    //  reaches a range, htslib never reads ISIZE)
    const uint64_t cap = (uint64_t)(nb < B ? nb : B) * 65536ull;
    uint8_t *pin = (uint8_t *)dhts_host_alloc(cap + 64);
    std::vector<int32_t> bs(B);
    int rc = pin ? 0 : -1; int64_t nout = 0;
    for (int64_t b = 0; b < nb && rc == 0; b += B) {
        const int64_t k = b + B < nb ? B : nb - b;
        const int64_t got = dhts_bgzf_inflate_to_host(c, b, k, pin, cap, bs.data());
        if (got < 0) { rc = -1; break; }
        for (int64_t i = 0; i < k; i++) if (bs[i] != 0) { rc = -4; fail(c, "bgunzip: read error"); break; }
        if (rc) break;
        if (got > 0 && fwrite(pin, 1, (size_t)got, fo) != (size_t)got) { rc = -5; fail(c, "bgunzip: write error"); break; }
        nout += got;
    }
    if (pin) dhts_host_free(pin);
    if (fclose(fo) != 0 && rc == 0) { rc = -5; fail(c, "bgunzip: write error"); }
    if (rc) unlink(out_path);
    if (bytes_in) *bytes_in = (int64_t)c->file_size;
    if (bytes_out) *bytes_out = nout;
    return rc;
}

// raw bytes -> a valid BGZF file (what hts_idx_save writes a .csi / .tbi through): stored (uncompressed) DEFLATE blocks of up to 65,280
// bytes with CRC-32 and ISIZE, and the 28-byte EOF block.  Host only.  Returns the size (also when out is NULL or too small: call twice).
extern "C" int64_t dhts_bgzf_wrap(const void *raw, uint64_t n, void *out, uint64_t cap) {
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t *src = (const uint8_t *)raw; uint8_t *dst = (uint8_t *)out; uint64_t need = 28, at = 0;
    for (uint64_t p = 0; p < n; p += 65280) need += 18 + 5 + (n - p < 65280 ? n - p : 65280) + 8;
    if (!dst || cap < need) return (int64_t)need;
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; i++) { uint32_t x = i; for (int k = 0; k < 8; k++) x = (x & 1) ? 0xEDB88320u ^ (x >> 1) : x >> 1; tab[i] = x; }
    for (uint64_t p = 0; p < n; p += 65280) {
        const uint32_t l = (uint32_t)(n - p < 65280 ? n - p : 65280), total = 18 + 5 + l + 8;
        const uint8_t hd[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, (uint8_t)((total - 1) & 0xff), (uint8_t)((total - 1) >> 8)};
        memcpy(dst + at, hd, 18); at += 18;
        dst[at++] = 1; dst[at++] = (uint8_t)l; dst[at++] = (uint8_t)(l >> 8); dst[at++] = (uint8_t)~l; dst[at++] = (uint8_t)((~l) >> 8);      // BFINAL = 1, BTYPE = 00, LEN, NLEN
        memcpy(dst + at, src + p, l); at += l;
        uint32_t crc = 0xffffffffu; for (uint32_t i = 0; i < l; i++) crc = tab[(crc ^ src[p + i]) & 0xff] ^ (crc >> 8);
        crc ^= 0xffffffffu;
        for (int k = 0; k < 4; k++) dst[at++] = (uint8_t)(crc >> (8 * k));
        for (int k = 0; k < 4; k++) dst[at++] = (uint8_t)(l >> (8 * k));
    }
    memcpy(dst + at, eof, 28); at += 28;
    return (int64_t)at;
}
