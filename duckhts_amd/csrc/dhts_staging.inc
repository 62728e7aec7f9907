// dhts_staging.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// staging: pinned host pool, file -> HBM (whole file, byte range, shard window, index segments, streaming).
// ---- pinned host memory, pooled for the life of the process ---------------------------------------------------------------------
// Page-locking is slow (a few GB/s), so staging and read-back buffers are kept and handed out again: a long-lived host (DuckDB)
// pays for them once, not per query.  Portable: usable from every device.
namespace {
struct PinBuf { void *p; size_t cap; bool busy; int node; };   // node: NUMA node of the thread that allocated it (-1 unknown)
std::mutex g_pin_mu;
std::vector<PinBuf> g_pin;
thread_local int t_numa_node = -1;        // the node this thread was bound to (dhts_bind_thread_near_device); pinned buffers prefer it
// "0-3,8,10-11" -> cpu_set_t; returns the number of CPUs
int parse_cpulist(const char *s, cpu_set_t *set) {
    CPU_ZERO(set); int n = 0;
    while (*s) {
        char *e; long a = strtol(s, &e, 10); if (e == s) break; long b = a;
        if (*e == '-') { s = e + 1; b = strtol(s, &e, 10); if (e == s) break; }
        for (long k = a; k <= b && k < CPU_SETSIZE; k++) if (k >= 0) { CPU_SET((int)k, set); n++; }
        s = e; while (*s == ',' || *s == ' ' || *s == '\n') s++;
    }
    return n;
}
}
// ---- NUMA placement ------------------------------------------------------------------------------------------------------------------
// A producer and its staging readers move every byte of the file host -> device and every column byte device -> host: on a two-socket
// host the pinned buffers and the threads that fill them belong on the socket the GPU hangs off (hipDeviceGetPCIBusId ->
// /sys/bus/pci/devices/<id>/numa_node -> /sys/devices/system/node/node<N>/cpulist).  The reference leaves placement to the OS: its reader
// threads (hts_set_threads, src/bam_reader.c:584,625) have no device to be near.  DHTS_NUMA=0 turns the binding off.
extern "C" int dhts_device_numa_node(int device) {
    char bus[64] = {0};
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { (void)hipGetLastError(); return -1; }     // (no sticky error left behind for the caller's next check)
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *q = bus; *q; q++) *q = (char)tolower((unsigned char)*q);
    char path[160]; snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r"); if (!f) return -1;
    int node = -1; if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f);
    return node;
}
// binds the CALLING thread (and the threads it creates from now on) to the CPUs of `node`; 0 = bound, 1 = nothing to do, -1 = failed
extern "C" int dhts_bind_thread_to_node(int node) {
    static const bool off = getenv("DHTS_NUMA") && atoi(getenv("DHTS_NUMA")) == 0;
    if (off || node < 0) return 1;
    char path[96]; snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = fopen(path, "r"); if (!f) return 1;
    char line[4096] = {0}; const bool got = fgets(line, sizeof(line), f) != nullptr; fclose(f);
    cpu_set_t want, cur, both; if (!got || parse_cpulist(line, &want) == 0) return 1;
    // (inside a container the process may be confined to a subset of the machine's CPUs: bind to the intersection, never to nothing)
    if (sched_getaffinity(0, sizeof(cur), &cur) != 0) return -1;
    CPU_AND(&both, &want, &cur);
    if (CPU_COUNT(&both) == 0) return 1;
    if (sched_setaffinity(0, sizeof(both), &both) != 0) return -1;
    t_numa_node = node;
    return 0;
}
extern "C" int dhts_bind_thread_near_device(int device) { return dhts_bind_thread_to_node(dhts_device_numa_node(device)); }
// streams of the staging threads (host -> device copies).  DHTS_STAGE_PRIO: 0 normal (default), 1 highest, 2 lowest -- which hardware queue
// class the copies share (see the copy stream of the read-back)
static hipError_t stage_stream_create(hipStream_t *st) {
    static const int prio = getenv("DHTS_STAGE_PRIO") ? atoi(getenv("DHTS_STAGE_PRIO")) : 0;
    if (prio == 0) return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio == 1 ? hi : lo);
}
extern "C" void *dhts_host_alloc(uint64_t n) {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    // a buffer that was allocated from the caller's NUMA node first (smallest that fits), then one of unknown placement; a buffer of
    // another node only for a caller that is not bound to any
    int best = -1;
    for (int pass = 0; pass < 2 && best < 0; pass++)
        for (size_t i = 0; i < g_pin.size(); i++) {
            if (g_pin[i].busy || g_pin[i].cap < n) continue;
            const bool fits = pass == 0 ? g_pin[i].node == t_numa_node : (t_numa_node < 0 || g_pin[i].node < 0);
            if (fits && (best < 0 || g_pin[i].cap < g_pin[best].cap)) best = (int)i;
        }
    if (best >= 0) { g_pin[best].busy = true; return g_pin[best].p; }
    void *p = nullptr; size_t want = (size_t)n + (size_t)n / 8 + 4096;
    if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess) return nullptr;
    // drop idle buffers that are too small to matter any more (keeps the pool from growing without bound)
    for (size_t i = 0; i < g_pin.size();) { if (!g_pin[i].busy && g_pin[i].cap * 2 <= want && g_pin.size() > 16) { (void)hipHostFree(g_pin[i].p); g_pin.erase(g_pin.begin() + i); } else i++; }
    g_pin.push_back({p, want, true, t_numa_node});     // (first touch / the runtime's own policy place the pages: the caller is bound to its device's node)
    return p;
}
// gives the idle pooled buffers (device and pinned host) back to the driver; buffers in use are untouched
extern "C" void dhts_release_pools(void) {
    { std::lock_guard<std::mutex> lk(g_ss_mu); for (auto &x : g_ss) { (void)hipSetDevice(x.dev); (void)hipEventDestroy(x.ev); (void)hipStreamDestroy(x.sb); (void)hipStreamDestroy(x.s); } g_ss.clear(); }
    { std::lock_guard<std::mutex> lk(g_pool_mu); for (auto &b : g_pool) (void)hipFree(b.p); g_pool.clear(); g_pool_bytes = 0; }
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (size_t i = 0; i < g_pin.size();) { if (!g_pin[i].busy) { (void)hipHostFree(g_pin[i].p); g_pin.erase(g_pin.begin() + i); } else i++; }
}
// free / total HBM of a device as the driver reports it (what the leak tests and the pool sizing look at)
extern "C" int dhts_device_mem_info(int device, uint64_t *free_bytes, uint64_t *total_bytes) {
    size_t f = 0, t = 0;
    if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemGetInfo(&f, &t) != hipSuccess) return -1;
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}
extern "C" void dhts_host_free(void *p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (auto &b : g_pin) if (b.p == p) { b.busy = false; return; }
}

// file bytes [off, off+len) -> dst[0, len): reader threads pread 8 MiB pieces into their own pair of pinned buffers and queue the
// H2D copies on their own streams, so the page-cache copy (one core moves ~5-10 GB/s) and the PCIe transfer overlap and scale.
static int stage_file_range(dhts_ctx *c, int fd, uint64_t off, uint64_t len, uint8_t *dst, StageProg *prog = nullptr) {
    const size_t CH = 8u << 20;
    const uint64_t npieces = (len + CH - 1) / CH;
    static const int env_thr = getenv("DHTS_READ_THREADS") ? atoi(getenv("DHTS_READ_THREADS")) : 0;
    // (measured on the MI355X host, per 0.85 GB query: 4 readers 75 ms, 8: 80, 16: 120, 32: 180)
    int nthr = env_thr > 0 ? env_thr : 4; if ((uint64_t)nthr > npieces) nthr = (int)npieces; if (nthr < 1) nthr = 1;
    std::atomic<uint64_t> next(0); std::atomic<int> rc(0);
    const int dev = c->device;
    if (prog) { std::lock_guard<std::mutex> lk(prog->mu); prog->piece_done.assign(npieces, 0); prog->next_piece = 0; prog->frontier = 0; prog->len = len; }
    auto worker = [&]() {
        if (hipSetDevice(dev) != hipSuccess) { rc = -1; return; }
        hipStream_t st = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; void *pin[2] = {dhts_host_alloc(CH), dhts_host_alloc(CH)}; bool used[2] = {false, false};
        uint64_t piece_of[2] = {0, 0};
        if (!pin[0] || !pin[1] || stage_stream_create(&st) != hipSuccess || hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess) rc = -2;
        int k = 0;
        while (rc == 0) {
            if (prog && prog->cancel.load()) { rc = -9; break; }                      // (the caller is closing the context: stop reading)
            const uint64_t pi = next.fetch_add(1);
            if (pi >= npieces) break;
            const uint64_t o = pi * CH; const size_t want = (size_t)(len - o < CH ? len - o : CH);
            if (used[k]) { (void)hipEventSynchronize(ev[k]); if (prog) prog->mark(piece_of[k], CH); used[k] = false; }
            size_t got = 0;
            while (got < want) { ssize_t r = pread(fd, (char *)pin[k] + got, want - got, (off_t)(off + o + got)); if (r <= 0) { rc = -3; break; } got += (size_t)r; }
            if (rc != 0) break;
            if (hipMemcpyAsync(dst + o, pin[k], want, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(ev[k], st) != hipSuccess) { rc = -4; break; }
            used[k] = true; piece_of[k] = pi; k ^= 1;
            // the other buffer's copy was queued a whole pread ago: it has usually landed, report it now rather than a piece later
            if (prog && used[k] && hipEventQuery(ev[k]) == hipSuccess) { prog->mark(piece_of[k], CH); used[k] = false; }
        }
        if (st) (void)hipStreamSynchronize(st);
        for (int q = 0; q < 2; q++) { if (used[q] && prog && rc == 0) prog->mark(piece_of[q], CH); if (ev[q]) (void)hipEventDestroy(ev[q]); dhts_host_free(pin[q]); }
        if (st) (void)hipStreamDestroy(st);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthr; t++) th.emplace_back(worker);
    worker();
    for (auto &t : th) t.join();
    return rc.load();
}

// identity of an unchanged file: what a cached copy of its bytes is valid for
static std::string file_tag(const struct stat &sb) {
    char b[160];
    snprintf(b, sizeof(b), "%llx:%llx:%llu:%lld.%09ld:%lld.%09ld", (unsigned long long)sb.st_dev, (unsigned long long)sb.st_ino, (unsigned long long)sb.st_size,
             (long long)sb.st_mtim.tv_sec, (long)sb.st_mtim.tv_nsec, (long long)sb.st_ctim.tv_sec, (long)sb.st_ctim.tv_nsec);
    return b;
}

// several file ranges in one go (the index windows of a region query): one set of reader threads works through all their pieces
struct StagePiece { uint64_t file_off; size_t len; uint8_t *dst; };
static int stage_file_pieces(dhts_ctx *c, int fd, const std::vector<StagePiece> &ranges) {
    const size_t CH = 8u << 20;
    std::vector<StagePiece> pc;
    for (auto &r : ranges) for (size_t o = 0; o < r.len; o += CH) pc.push_back({r.file_off + o, r.len - o < CH ? r.len - o : CH, r.dst + o});
    if (pc.empty()) return 0;
    static const int env_thr = getenv("DHTS_READ_THREADS") ? atoi(getenv("DHTS_READ_THREADS")) : 0;
    int nthr = env_thr > 0 ? env_thr : 4; if ((size_t)nthr > pc.size()) nthr = (int)pc.size();
    size_t tot = 0; for (auto &x : pc) tot += x.len;
    if (tot <= (1u << 20)) nthr = 1;                            // a sliver: thread start-up would cost more than the copy
    std::atomic<size_t> next(0); std::atomic<int> rc(0);
    const int dev = c->device;
    auto worker = [&]() {
        if (hipSetDevice(dev) != hipSuccess) { rc = -1; return; }
        hipStream_t st = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; void *pin[2] = {dhts_host_alloc(CH), dhts_host_alloc(CH)}; bool used[2] = {false, false};
        if (!pin[0] || !pin[1] || stage_stream_create(&st) != hipSuccess || hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess) rc = -2;
        int k = 0;
        while (rc == 0) {
            const size_t pi = next.fetch_add(1);
            if (pi >= pc.size()) break;
            const StagePiece &x = pc[pi];
            if (used[k]) { (void)hipEventSynchronize(ev[k]); used[k] = false; }
            size_t got = 0;
            while (got < x.len) { ssize_t r = pread(fd, (char *)pin[k] + got, x.len - got, (off_t)(x.file_off + got)); if (r <= 0) { rc = -3; break; } got += (size_t)r; }
            if (rc != 0) break;
            if (hipMemcpyAsync(x.dst, pin[k], x.len, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(ev[k], st) != hipSuccess) { rc = -4; break; }
            used[k] = true; k ^= 1;
        }
        if (st) (void)hipStreamSynchronize(st);
        for (int q = 0; q < 2; q++) { if (ev[q]) (void)hipEventDestroy(ev[q]); dhts_host_free(pin[q]); }
        if (st) (void)hipStreamDestroy(st);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthr; t++) th.emplace_back(worker);
    worker();
    for (auto &t : th) t.join();
    return rc.load();
}

// htslib hts_open + the reads underneath bgzf_read_block, for a BYTE RANGE of the file: [off, off+len) (len = 0: to the end of the
// file) becomes the context's resident bytes.  A rank of a multi-GPU scan stages only its own block range plus the halo.
int dhts_open_path_range(dhts_ctx *c, const char *path, uint64_t off, uint64_t len) {
    if (!c) return -1;
    discard_prefetch(c);
    int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(c, "cannot open %s", path);
    struct stat sb; if (fstat(fd, &sb) != 0) { close(fd); return fail(c, "cannot stat %s", path); }
    const uint64_t fsize = (uint64_t)sb.st_size;
    if (off > fsize) off = fsize;
    uint64_t n = fsize - off; if (len != 0 && len < n) n = len;
    if (hipSetDevice(c->device) != hipSuccess) { close(fd); return fail(c, "hipSetDevice failed"); }
    reset_file_state(c);
    const bool whole = off == 0 && n == fsize && n > 0 && file_cache_on();
    const std::string tag = whole ? file_tag(sb) : std::string();
    if (whole && c->comp.adopt(tag) == (int64_t)n) {            // the unchanged file is still in HBM from an earlier query
        close(fd);
        c->comp_len = n; c->file_off = 0; c->file_size = fsize; c->cache_hit = true;
        return 0;
    }
    if (c->comp.ensure(n + PAD_BYTES) != 0) { close(fd); return fail(c, "hipMalloc of %llu bytes failed", (unsigned long long)(n + PAD_BYTES)); }
    int rc = n ? stage_file_range(c, fd, off, n, (uint8_t *)c->comp.p) : 0;
    close(fd);
    if (rc) return fail(c, rc == -3 ? "read error on %s" : "staging %s failed", path);
    HIPCHK(c, hipMemsetAsync((uint8_t *)c->comp.p + n, 0, PAD_BYTES, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->comp_len = n; c->file_off = off; c->file_size = fsize;
    if (whole) { c->comp.tag = tag; c->comp.tag_len = n; }
    return 0;
}
int dhts_open_path(dhts_ctx *c, const char *path) { return dhts_open_path_range(c, path, 0, 0); }

static bool host_is_bgzf_header(const uint8_t *p);
// Only the parts of a file a region query needs (htslib seeks to each chunk, hts.c:4320-4607; here they are staged): the header blocks
// file[0, header_bytes) and the windows [beg[k], end[k] + length of the BGZF block at end[k]) from dhts_bam_region_segments, merged where
// they touch, laid out one after the other in file order.  dhts_bgzf_index, dhts_bam_open, dhts_bam_set_regions and dhts_bam_load_index
// follow as for a whole file; the block table maps resident blocks back to file offsets, so virtual offsets stay those of the file.
// `raw`: the file is not BGZF and [beg[k], end[k]) are plain byte ranges (the region windows of an uncompressed FASTA: dhts_fasta_index.inc)
static int open_path_ranges(dhts_ctx *c, const char *path, uint64_t header_bytes, const uint64_t *beg, const uint64_t *end, int64_t n, bool raw);
extern "C" int dhts_open_path_segments(dhts_ctx *c, const char *path, uint64_t header_bytes, const uint64_t *beg, const uint64_t *end, int64_t n) {
    return open_path_ranges(c, path, header_bytes, beg, end, n, false);
}
static int open_path_ranges(dhts_ctx *c, const char *path, uint64_t header_bytes, const uint64_t *beg, const uint64_t *end, int64_t n, bool raw) {
    if (!c || n < 0 || (n > 0 && (!beg || !end))) return -1;
    discard_prefetch(c);
    int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(c, "cannot open %s", path);
    struct stat sb; if (fstat(fd, &sb) != 0) { close(fd); return fail(c, "cannot stat %s", path); }
    const uint64_t fsize = (uint64_t)sb.st_size;
    if (header_bytes > fsize) header_bytes = fsize;
    std::vector<std::pair<uint64_t, uint64_t>> rg;              // [first byte, one past the last byte)
    if (header_bytes) rg.push_back({0, header_bytes});
    for (int64_t k = 0; k < n; k++) {
        uint64_t b = beg[k], e = end[k];
        if (b >= fsize) continue;
        if (e == ~0ull || e >= fsize) e = fsize;
        else if (!raw) {
            uint8_t h[18];
            if (e + 18 > fsize || pread(fd, h, 18, (off_t)e) != 18 || !host_is_bgzf_header(h)) { close(fd); return fail(c, "index does not match the file (no BGZF block at offset %llu)", (unsigned long long)e); }
            e += ((uint64_t)h[16] | ((uint64_t)h[17] << 8)) + 1;
            if (e > fsize) e = fsize;
        }
        if (e > b) rg.push_back({b, e});
    }
    std::sort(rg.begin(), rg.end());
    std::vector<std::pair<uint64_t, uint64_t>> mg;
    for (auto &x : rg) { if (!mg.empty() && x.first <= mg.back().second) { if (x.second > mg.back().second) mg.back().second = x.second; } else mg.push_back(x); }
    uint64_t tot = 0; for (auto &x : mg) tot += x.second - x.first;
    if (hipSetDevice(c->device) != hipSuccess) { close(fd); return fail(c, "hipSetDevice failed"); }
    reset_file_state(c);
    if (c->comp.ensure(tot + PAD_BYTES) != 0) { close(fd); return fail(c, "hipMalloc of %llu bytes failed", (unsigned long long)(tot + PAD_BYTES)); }
    uint64_t at = 0;
    std::vector<StagePiece> ranges;
    for (auto &x : mg) {
        ranges.push_back({x.first, (size_t)(x.second - x.first), (uint8_t *)c->comp.p + at});
        c->segs.push_back({at, x.first, x.second - x.first});
        at += x.second - x.first;
    }
    const int rc = stage_file_pieces(c, fd, ranges);
    close(fd);
    if (rc) { c->segs.clear(); return fail(c, rc == -3 ? "read error on %s" : "staging %s failed", path); }
    HIPCHK(c, hipMemsetAsync((uint8_t *)c->comp.p + tot, 0, PAD_BYTES, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->comp_len = tot; c->file_off = 0; c->file_size = fsize; c->hdr_bytes_known = header_bytes;
    c->partial_tail = mg.empty() || mg.back().second < fsize;
    if (c->segs.size() == 1 && c->segs[0].file_off == 0 && c->segs[0].len == fsize) c->segs.clear();      // everything is resident after all
    return 0;
}

// The same for a scan that starts before the file has arrived: staging runs on background threads, dhts_stage_wait reports how many
// contiguous bytes are resident, dhts_bgzf_index_staged (re)builds the block table over that prefix, and dhts_bam_next_batch serves the
// blocks known so far (the stream is not "at its end" while bytes are still arriving).
int dhts_open_path_async(dhts_ctx *c, const char *path) {
    if (!c) return -1;
    discard_prefetch(c);
    int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(c, "cannot open %s", path);
    struct stat sb; if (fstat(fd, &sb) != 0) { close(fd); return fail(c, "cannot stat %s", path); }
    const uint64_t n = (uint64_t)sb.st_size;
    if (hipSetDevice(c->device) != hipSuccess) { close(fd); return fail(c, "hipSetDevice failed"); }
    reset_file_state(c);
    const std::string tag = (n > 0 && file_cache_on()) ? file_tag(sb) : std::string();
    if (!tag.empty() && c->comp.adopt(tag) == (int64_t)n) {     // still in HBM from an earlier query: nothing to stage
        close(fd);
        c->prog = new StageProg(); c->prog->len = n; c->prog->frontier = n; c->prog->finished = true;
        c->stage_total = n; c->file_off = 0; c->file_size = n; c->comp_len = 0; c->growing = true; c->cache_hit = true;
        return 0;
    }
    if (c->comp.ensure(n + PAD_BYTES) != 0) { close(fd); return fail(c, "hipMalloc of %llu bytes failed", (unsigned long long)(n + PAD_BYTES)); }
    HIPCHK(c, hipMemsetAsync((uint8_t *)c->comp.p + n, 0, PAD_BYTES, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->prog = new StageProg(); c->prog->len = n; c->stage_total = n; c->file_off = 0; c->file_size = n; c->comp_len = 0; c->growing = true;
    c->pending_tag = tag;
    StageProg *pg = c->prog; uint8_t *dst = (uint8_t *)c->comp.p;
    c->stager = std::thread([c, fd, n, dst, pg]() {
        int rc = n ? stage_file_range(c, fd, 0, n, dst, pg) : 0;
        close(fd);
        std::lock_guard<std::mutex> lk(pg->mu); pg->rc = rc; pg->finished = true; if (rc == 0) pg->frontier = n; pg->cv.notify_all();
    });
    return 0;
}
int64_t dhts_stage_wait(dhts_ctx *c, uint64_t min_bytes, int *done) {
    if (!c || !c->prog) { if (done) *done = 1; return c ? (int64_t)c->comp_len : -1; }
    StageProg *pg = c->prog;
    std::unique_lock<std::mutex> lk(pg->mu);
    pg->cv.wait(lk, [&] { return pg->finished || pg->frontier >= min_bytes; });
    if (pg->finished && pg->rc != 0) { lk.unlock(); return fail(c, "staging failed (read error)"); }
    if (done) *done = pg->finished ? 1 : 0;
    return (int64_t)pg->frontier;
}
static int64_t index_impl(dhts_ctx *c, bool extend);
int64_t dhts_bgzf_index_staged(dhts_ctx *c) {
    if (!c) return -1;
    if (!c->prog) return dhts_bgzf_index(c);
    int done = 0; const int64_t f = dhts_stage_wait(c, 0, &done);
    if (f < 0) return -1;
    const bool extend = c->comp_len > 0 && c->n_blocks > 0;
    c->comp_len = (uint64_t)f; c->partial_tail = !done; c->growing = !done;
    return index_impl(c, extend);
}
int64_t dhts_blocks_ahead(const dhts_ctx *c) { return c ? c->n_blocks - c->next_block : 0; }

uint64_t dhts_resident_bytes(const dhts_ctx *c) { return c ? c->comp_len : 0; }
extern "C" int dhts_resident_from_cache(const dhts_ctx *c) { return c && c->cache_hit ? 1 : 0; }
