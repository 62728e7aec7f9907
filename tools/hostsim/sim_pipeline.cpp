// sim_pipeline.cpp -- races the batch pipeline of read_bam / read_bcf (duckhts_amd/csrc/duckdb_pipeline.h) on a CPU: fake producer threads
// publish batches of numbered rows into malloc'ed arenas, worker threads consume them through next_rows and the chunk loop.  Built with
// -fsanitize=thread and with -fsanitize=address,undefined by tests/test_hostsim_pipeline.py; every case prints one line, "FAIL" marks a
// broken expectation and the exit status is the number of failed cases.
//   g++ -std=c++17 -pthread -O1 -g -fsanitize=thread tools/hostsim/sim_pipeline.cpp -o sim_pipeline
#include "../../duckhts_amd/csrc/duckdb_pipeline.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>

static const uint64_t VSIZE = 2048;
static const int64_t SIZES[5] = {1, 2047, 2048, 2049, 5000};

struct SimBatch : PipeSlot { bool waited = false, landed = false; int64_t first = 0; };     // waited: the copy of this batch has been waited for
typedef Pipeline<SimBatch> Pipe;

static std::atomic<int> g_arenas{0}, g_ctx_live{0}, g_freed_under_ctx{0}, g_seen_early{0}, g_landed_early{0}, g_take_cancelled{0}, g_take_calls{0}, g_failed_first{0};
static thread_local bool t_producer = false;                       // (a producer frees an arena to grow it; teardown frees them all)
static void *sim_alloc(uint64_t n) { g_arenas++; return malloc(n); }
static void sim_free(void *p) { if (!p) return; if (!t_producer && g_ctx_live.load()) g_freed_under_ctx++; g_arenas--; free(p); }     // a context dies before any arena
static void sim_ctx_destroy(void *c) { g_ctx_live--; delete (int *)c; }

static uint64_t row_id(size_t source, int64_t row) { return ((uint64_t)source << 40) | (uint64_t)row; }

struct Plan {
    int sources = 1, workers = 1, batches = 10; bool serial = false;
    int stop_source = -1, stop_after = 0; bool stop_with_error = false, second_error = false;    // source stop_source ends after stop_after batches: unclean end, or an error
    bool abandon = false;                                                                        // the consumer takes one chunk and tears down
};

// one fake producer: batch j has SIZES[j % 5] rows; a copy "lands" only in fetch_wait (serial: in fetch), as the device's does
static void producer(Pipe &pipe, size_t k, const Plan &pl) {
    Pipe::Source &src = *pipe.src[k];
    t_producer = true; src.ctx = new int(0); g_ctx_live++;
    int64_t row = 0, cur_n = 0; SimBatch *in_flight[2] = {nullptr, nullptr};
    auto write_rows = [&](SimBatch *hb) { uint64_t *a = (uint64_t *)hb->arena; for (int64_t r = 0; r < hb->n; r++) a[r] = row_id(k, hb->first + r); hb->waited = true; };
    auto rb = make_readback(pipe, src, pl.serial,
                            [&](SimBatch *hb) { hb->n = cur_n; hb->first = row; write_rows(hb); return true; },
                            [&](SimBatch *hb, int sl) { hb->n = cur_n; hb->first = row; in_flight[sl] = hb; return true; },
                            [&](int sl) { write_rows(in_flight[sl]); in_flight[sl] = nullptr; return true; },
                            [&](SimBatch *hb) { if (!hb->waited) g_landed_early++; hb->landed = true; });
    for (int j = 0; j < pl.batches; j++) {
        if ((int)k == pl.stop_source && j == pl.stop_after) {
            (void)rb.flush();
            if (pl.stop_with_error) { pipe.finish(src, "error from source " + std::to_string(k)); g_failed_first = 1; }
            else pipe.finish(src);                                                               // clean_end stays false
            return;
        }
        if (pl.second_error && (int)k != pl.stop_source && j == pl.stop_after) {                 // a second failing source, after the first
            while (!g_failed_first.load()) std::this_thread::yield();
            pipe.finish(src, "error from source " + std::to_string(k)); return;
        }
        cur_n = SIZES[j % 5];
        g_take_calls++;
        SimBatch *hb = pipe.take_slot(src);
        if (!hb) { g_take_cancelled++; break; }
        if (!pipe.reserve(hb, (uint64_t)cur_n * 8)) { pipe.finish(src, "out of memory"); return; }
        hb->waited = hb->landed = false;
        if (!rb.begin(hb)) { pipe.finish(src, "fetch failed"); return; }
        hb->status = 0; hb->next = 0; hb->readers = 0; hb->retired = false;
        if (!rb.turn(hb)) { pipe.finish(src, "fetch_wait failed"); return; }
        row += cur_n;
        if (pipe.cancelled()) break;
    }
    if (!rb.flush()) { pipe.finish(src, "fetch_wait failed"); return; }
    src.clean_end = true;
    pipe.finish(src);
}

struct WorkerOut { std::vector<std::vector<uint64_t>> chunks; std::string err; };
static void worker(Pipe &pipe, const Plan &pl, WorkerOut &out) {
    Pipe::Cursor at;
    for (;;) {
        std::vector<uint64_t> chunk(VSIZE);
        const int64_t n = pipe.fill_chunk(at, VSIZE, out.err, [&](const SimBatch &hb, int64_t s, uint64_t take, uint64_t row_count) {
            if (!hb.waited || !hb.landed) g_seen_early++;
            memcpy(chunk.data() + row_count, (const uint64_t *)hb.arena + s, take * 8);
        });
        if (n <= 0) break;
        chunk.resize((size_t)n); out.chunks.push_back(chunk);
        if (pl.abandon) {
            // LIMIT: the first chunk is batch 0 (1 row) and batch 1 (2047 rows), and batch 1's slot is still this worker's.  Batches 2 and 3 fill
            // the other two slots, so the producer's fifth take_slot finds none: wait until it is there, then leave
            while (g_take_calls.load() < 5) std::this_thread::yield();
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
            break;
        }
    }
}

static int64_t rows_of(const Plan &pl, int k) {
    const int nb = k == pl.stop_source ? pl.stop_after : pl.batches;
    int64_t n = 0; for (int j = 0; j < nb; j++) n += SIZES[j % 5];
    return n;
}

// runs one plan; returns 0 when every expectation holds
static int run(const char *name, const Plan &pl) {
    g_take_calls = 0; g_failed_first = 0; g_take_cancelled = 0;
    std::vector<WorkerOut> outs((size_t)pl.workers);
    {
        Pipe pipe;
        pipe.init((size_t)pl.sources, 3, pl.workers, sim_alloc, sim_free, sim_ctx_destroy);
        for (size_t k = 0; k < (size_t)pl.sources; k++) pipe.start(k, [&pipe, k, &pl] { producer(pipe, k, pl); });
        std::vector<std::thread> th;
        for (int w = 1; w < pl.workers; w++) th.emplace_back([&pipe, &pl, &outs, w] { worker(pipe, pl, outs[(size_t)w]); });
        worker(pipe, pl, outs[0]);
        for (auto &t : th) t.join();
        pipe.teardown();                                              // (must return: a producer may be waiting for a free slot)
    }
    std::vector<uint64_t> got; std::string err; size_t n_chunks = 0; bool sizes_ok = true, full_ok = true;
    for (auto &o : outs) {
        if (err.empty()) err = o.err;
        for (size_t i = 0; i < o.chunks.size(); i++) {
            n_chunks++; sizes_ok = sizes_ok && o.chunks[i].size() <= VSIZE;
            if (i + 1 < o.chunks.size() && o.chunks[i].size() != VSIZE) full_ok = false;
            got.insert(got.end(), o.chunks[i].begin(), o.chunks[i].end());
        }
    }
    // what a complete scan delivers: source after source, batch after batch (an unclean end: nothing behind it)
    std::vector<uint64_t> want;
    for (int k = 0; k < pl.sources; k++) {
        for (int64_t r = 0; r < rows_of(pl, k); r++) want.push_back(row_id((size_t)k, r));
        if (k == pl.stop_source && !pl.stop_with_error && pl.workers == 1) break;
    }
    bool ok = sizes_ok && g_arenas.load() == 0 && g_ctx_live.load() == 0 && g_freed_under_ctx.load() == 0 && g_seen_early.load() == 0 && g_landed_early.load() == 0;
    if (pl.abandon) ok = ok && got.size() == VSIZE && std::equal(got.begin(), got.end(), want.begin()) && err.empty() && g_take_cancelled.load() == 1;
    else if (pl.stop_with_error) ok = ok && err == "error from source " + std::to_string(pl.stop_source);      // the first message wins
    else {
        ok = ok && err.empty();
        if (pl.workers == 1) ok = ok && full_ok && got == want;       // in order, full chunks except the last
        else { std::sort(got.begin(), got.end()); std::sort(want.begin(), want.end()); ok = ok && got == want; }
    }
    printf("case %-28s sources %d workers %d %-10s rows %zu of %zu chunks %zu err '%s' cancelled-in-take %d early %d/%d arenas %d contexts %d: %s\n", name, pl.sources, pl.workers,
           pl.serial ? "serial" : "overlapped", got.size(), want.size(), n_chunks, err.c_str(), g_take_cancelled.load(), g_seen_early.load(), g_landed_early.load(), g_arenas.load(), g_ctx_live.load(), ok ? "ok" : "FAIL");
    return ok ? 0 : 1;
}

int main() {
    int bad = 0, n = 0;
    for (int serial = 0; serial < 2; serial++) {
        Plan p; p.serial = serial != 0;
        for (int sources : {1, 3}) {
            p.sources = sources; p.workers = 1; bad += run("complete_ordered", p); n++;
            for (int workers : {3, 4}) { p.workers = workers; bad += run("parallel", p); n++; }
        }
        Plan u; u.serial = p.serial; u.sources = 3; u.stop_source = 0; u.stop_after = 4; bad += run("unclean_end_first_source", u); n++;
        Plan e; e.serial = p.serial; e.stop_source = 0; e.stop_after = 5; e.stop_with_error = true; bad += run("producer_error", e); n++;
        e.sources = 3; e.workers = 3; e.stop_source = 1; e.second_error = true; bad += run("two_errors_first_wins", e); n++;
        Plan a; a.serial = p.serial; a.batches = 40; a.abandon = true; bad += run("cancel_in_take_slot", a); n++;
        a.sources = 3; a.workers = 1; a.abandon = false; a.batches = 8; bad += run("eight_batches_three_sources", a); n++;
    }
    printf("%s: %d cases, %d failed\n", bad ? "FAILED" : "ALL OK", n, bad);
    return bad;
}
