// sim_scan.cpp -- host build of bam_tile_scan_lanes' per-lane function (line loads, prefilter, full filter three deep, light walk) under
// ASAN/UBSAN.  Its text is cut out of bam_records.hip and bam_tiles_lds.hip by run_scan.sh (scan_extract.inc); nothing is duplicated here
// except the plain serial model it is compared with.
//   sim_scan [-r N] [-t] stream.bin ...   (a stream = BAM records one behind the other; -t before a file: it is a non-final batch;
//                                         -r N: the header of the files that follow names N references, default 2)
// Every tile t >= 1 of a stream is scanned on an exact-size copy of it: the buffer ends where the 16-byte padding of the device buffer
// ends, so a read the device code may not make is an ASAN error.  The tables (first, end_next, count, err, recs_first, the record list)
// must equal the model's: the smallest offset of the tile that passes bam_read1's core tests and the speculation filter with its next two
// hops not invalid, then a walk over block_size words.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define __device__
#define __forceinline__ inline
struct uint4 { uint32_t x, y, z, w; };
static inline int __ffs(int v) { return __builtin_ffs(v); }
static inline int __ffsll(unsigned long long v) { return __builtin_ffsll((long long)v); }
#include "scan_extract.inc"

// ---- the plain model (64-bit signed arithmetic, byte-wise reads) ----
static int64_t rd_i32(const std::vector<uint8_t> &u, int64_t o) { int32_t v; memcpy(&v, u.data() + o, 4); return v; }
enum { M_OK = 0, M_INVALID = 1, M_INCOMPLETE = 2 };
static int model_check(const std::vector<uint8_t> &u, int64_t ulen, int64_t n_ref, int64_t o, int64_t &bl) {
    if (ulen - o < 4) return M_INCOMPLETE;
    const int64_t b = rd_i32(u, o);
    if (b < 32) return M_INVALID;
    if (ulen - o - 4 < 32) return M_INCOMPLETE;
    const int64_t tid = rd_i32(u, o + 4), l_qname = u[o + 12], n_cigar = (uint16_t)rd_i32(u, o + 16), l_seq = rd_i32(u, o + 20), mtid = rd_i32(u, o + 24);
    if (l_seq < 0 || l_qname < 1) return M_INVALID;
    const int64_t body = b - 32, core = 4 * n_cigar + l_qname + (l_seq + 1) / 2 + l_seq;
    if (core > body) return M_INVALID;
    if (tid < -1 || tid >= n_ref || mtid < -1 || mtid >= n_ref) return M_INVALID;
    if (body - core > 8 * core + 65536) return M_INVALID;
    if (ulen - o - 36 < body) return M_INCOMPLETE;
    if (u[o + 36 + l_qname - 1] != 0) return M_INVALID;
    bl = b;
    return M_OK;
}
static bool model_spec(const std::vector<uint8_t> &u, int64_t ulen, int64_t n_ref, int64_t o) {
    int64_t bl;
    if (model_check(u, ulen, n_ref, o, bl) != M_OK) return false;
    int64_t o2 = o + 4 + bl;
    for (int k = 0; k < 2; k++) {
        const int rc = model_check(u, ulen, n_ref, o2, bl);
        if (rc == M_INVALID) return false;
        if (rc == M_INCOMPLETE) break;
        o2 += 4 + bl;
    }
    return true;
}

int main(int argc, char **argv) {
    int bad_files = 0; bool final_batch = true; int64_t n_ref = 2;
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "-t")) { final_batch = false; continue; }
        if (!strcmp(argv[a], "-r") && a + 1 < argc) { n_ref = atoll(argv[++a]); continue; }
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> u; uint8_t tmp[65536]; size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) u.insert(u.end(), tmp, tmp + n);
        fclose(f);
        const int64_t ulen = (int64_t)u.size();
        const int64_t ntiles = ulen ? (ulen + TL_TILE - 1) / TL_TILE : 1;
        // the device buffer: the stream, then padding to a multiple of 16 bytes and not a byte more; 16-byte aligned (new[] of a 16-byte type)
        const size_t padded = ((size_t)ulen + 15) & ~(size_t)15;
        uint4 *img4 = new uint4[padded / 16 ? padded / 16 : 1];
        uint8_t *img = (uint8_t *)img4;
        memset(img, 0xA5, padded); if (ulen) memcpy(img, u.data(), (size_t)ulen);
        std::vector<uint8_t> um(u); um.resize(padded + 64, 0xA5);           // the model's own copy (it tests the length before it reads)
        BamStream st; st.u = img; st.ulen = (uint64_t)ulen; st.n_ref = (int32_t)n_ref; st.final_batch = final_batch ? 1 : 0; st.seq_packed = 0; st.want_rg = 1;
        std::vector<uint64_t> first(ntiles, 0xEE), en(ntiles, 0xEE), rf(ntiles, 0xEE); std::vector<uint32_t> cnt(ntiles, 0xEE); std::vector<int32_t> err(ntiles, 0xEE);
        std::vector<uint16_t> recs((size_t)ntiles * TL_RECS, 0xEEEE);
        TileOut out; out.first = first.data(); out.end_next = en.data(); out.count = cnt.data(); out.err = err.data();
        int64_t mism = 0, with_first = 0, without = 0, nrec = 0, nerr = 0;
        for (int64_t t = 1; t < ntiles; t++) {
            tile_scan_lane(st, t, out, recs.data(), rf.data());
            const int64_t tb = t * (int64_t)TL_TILE, te = tb + TL_TILE < ulen ? tb + TL_TILE : ulen;
            int64_t mf = -1;
            for (int64_t o = tb; o < te; o++) if (model_spec(um, ulen, n_ref, o)) { mf = o; break; }
            int64_t men = -1, mcnt = 0, merr = 0; std::vector<uint16_t> ml;
            if (mf >= 0) {
                int64_t o = mf;
                while (o < te) {
                    if (ulen - o < 4) { if (final_batch) merr = 1; break; }
                    const int64_t b = rd_i32(um, o);
                    if (b < 32) { merr = 1; break; }
                    if (ulen - o - 4 < b) { if (final_batch) merr = 1; break; }
                    if (mcnt < (int64_t)TL_RECS) ml.push_back((uint16_t)(o - tb));
                    mcnt++; o += 4 + b;
                }
                men = o;
            }
            bool ok = first[t] == (uint64_t)mf && rf[t] == (uint64_t)mf && en[t] == (uint64_t)men && cnt[t] == (uint32_t)mcnt && err[t] == (int32_t)merr;
            for (size_t k = 0; ok && k < TL_RECS; k++) ok = recs[(size_t)t * TL_RECS + k] == (k < ml.size() ? ml[k] : 0xEEEE);
            if (!ok) {
                mism++;
                printf("MISMATCH %s tile %lld: first %lld / %lld end %lld / %lld count %u / %lld err %d / %lld\n", argv[a], (long long)t, (long long)first[t], (long long)mf,
                       (long long)en[t], (long long)men, cnt[t], (long long)mcnt, err[t], (long long)merr);
            }
            if (mf >= 0) with_first++; else without++;
            nrec += mcnt; nerr += merr;
        }
        delete[] img4;
        printf("tiles %lld mismatching %lld with_first %lld without %lld records %lld err %lld final %d %s\n", (long long)(ntiles - 1), (long long)mism, (long long)with_first,
               (long long)without, (long long)nrec, (long long)nerr, final_batch ? 1 : 0, argv[a]);
        if (mism) bad_files++;
        final_batch = true;
    }
    return bad_files ? 1 : 0;
}
