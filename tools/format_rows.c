/* format_rows.c -- the host side of the route bam_bedgraph_export replaces, for tools/bench_bedgraph_export.py: a page of bam_bedgraph's columns
 * (contig id, start, end, depth) printed as `name \t start \t end \t depth \n` by one host thread, digits written from the last to the first:
 * what a host formats rows with when it is written with care.  Built by the benchmark into a temporary shared object; not part of the library. */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

static char *put_u64(char *p, uint64_t v) {
    char tmp[20]; int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *p++ = tmp[--n];
    return p;
}

/* out has room for n * (longest name + 3 * 20 + 4) bytes; returns the bytes written */
size_t format_rows(const int32_t *tid, const int64_t *start, const int64_t *end, const int32_t *depth, size_t n, const char *names, const uint32_t *name_off, char *out) {
    char *p = out;
    for (size_t i = 0; i < n; i++) {
        const uint32_t o = name_off[tid[i]], l = name_off[tid[i] + 1] - o;
        memcpy(p, names + o, l); p += l;
        *p++ = '\t'; p = put_u64(p, (uint64_t)start[i]);
        *p++ = '\t'; p = put_u64(p, (uint64_t)end[i]);
        *p++ = '\t'; p = put_u64(p, (uint64_t)(uint32_t)depth[i]);
        *p++ = '\n';
    }
    return (size_t)(p - out);
}
