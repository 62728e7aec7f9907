// duckdb_pipeline.h -- the batch pipeline of read_bam and read_bcf: producer threads turn a file into batches in pinned host arenas, the
// engine's worker threads fill DataChunks from them.  One copy of the slot bookkeeping, the read-back overlap, the consumer, the chunk loop
// and the teardown order.  Standard library only (no DuckDB, no dhts_*, no HIP): tools/hostsim/sim_pipeline.cpp races it on a CPU under
// ThreadSanitizer and AddressSanitizer.  static / inline / templates only, like duckdb_surface.h.
//   n_workers == 1: ordered mode -- the sources are drained one after the other, whole batches, rows in file order.
//   n_workers  > 1: parallel mode -- workers claim slices of at most `want` rows of whatever is ready; the row order across workers is unspecified.
#ifndef DUCKHTS_DUCKDB_PIPELINE_H
#define DUCKHTS_DUCKDB_PIPELINE_H
#include <stdint.h>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// what every reader's host batch starts with: one arena and the rows that sit in it
struct PipeSlot {
    void *arena = nullptr; uint64_t cap = 0;
    int64_t n = 0; int status = 0;
    int64_t next = 0; int readers = 0; bool retired = false;      // parallel mode: rows [0, next) are claimed; retired = off the ready queue
};

template <class Batch>                                             // Batch derives from PipeSlot and adds the reader's payload
struct Pipeline {
    // one producer: read_bcf has one, read_bam one per entry of DHTS_DEVICES
    struct Source {
        std::deque<Batch *> ready; std::vector<Batch *> free_slots, all;
        bool done = false, clean_end = false;                      // clean_end: the stream ended at its end, not on a bad block / record
        void *ctx = nullptr;                                       // a context the source still owns: teardown destroys it before any arena is freed
        std::thread th;
    };
    struct Cursor { Batch *cur = nullptr; Source *owner = nullptr; int64_t pos = 0, end = 0; bool done = false; };   // rows [pos, end) of `cur` are this worker's

    std::mutex mu; std::condition_variable cv_ready, cv_free;
    std::vector<Source *> src; size_t cur_src = 0;
    std::string error; bool cancel = false, all_done_seen = false;
    int n_workers = 1;
    void *(*arena_alloc)(uint64_t) = nullptr; void (*arena_free)(void *) = nullptr; void (*ctx_destroy)(void *) = nullptr;
    std::function<void(std::string &)> on_all_done;                // called once, under the lock, when every source is done and drained: may set the error

    void init(size_t n_sources, int n_slots, int workers, void *(*alloc)(uint64_t), void (*release)(void *), void (*destroy)(void *)) {
        n_workers = workers; arena_alloc = alloc; arena_free = release; ctx_destroy = destroy;
        for (size_t k = 0; k < n_sources; k++) {
            Source *s = new Source();
            for (int q = 0; q < n_slots; q++) { Batch *hb = new Batch(); s->free_slots.push_back(hb); s->all.push_back(hb); }
            src.push_back(s);
        }
    }
    template <class Main> void start(size_t k, Main main) { src[k]->th = std::thread(main); }
    // cancel, wake everyone, join every producer, destroy the contexts the sources still own (that waits for their copy streams, whose D2H
    // may still be writing into an arena), and only then free the arenas
    void teardown() {
        { std::lock_guard<std::mutex> lk(mu); cancel = true; }
        cv_free.notify_all(); cv_ready.notify_all();
        for (Source *s : src) if (s->th.joinable()) s->th.join();
        for (Source *s : src) if (s->ctx) { ctx_destroy(s->ctx); s->ctx = nullptr; }
        for (Source *s : src) { for (Batch *hb : s->all) { arena_free(hb->arena); delete hb; } delete s; }
        src.clear();
    }
    ~Pipeline() { teardown(); }

    // ---- producer side -------------------------------------------------------------------------------------------------------------
    Batch *take_slot(Source &s) {                                   // waits for a free slot; nullptr once the scan is cancelled
        std::unique_lock<std::mutex> lk(mu);
        cv_free.wait(lk, [&] { return cancel || !s.free_slots.empty(); });
        if (cancel) return nullptr;
        Batch *hb = s.free_slots.back(); s.free_slots.pop_back();
        return hb;
    }
    bool reserve(Batch *hb, uint64_t need) {                        // exact-size growth; false: out of (pinned) host memory
        if (need > hb->cap) { arena_free(hb->arena); hb->arena = arena_alloc(need); hb->cap = hb->arena ? need : 0; }
        return !need || hb->arena;
    }
    void publish(Source &s, Batch *hb) {
        { std::lock_guard<std::mutex> lk(mu); s.ready.push_back(hb); }
        cv_ready.notify_all();
    }
    void finish(Source &s, const std::string &err = std::string()) {     // the first message wins
        { std::lock_guard<std::mutex> lk(mu); if (!err.empty() && error.empty()) error = err; s.done = true; }
        cv_ready.notify_all();
    }
    bool cancelled() { std::lock_guard<std::mutex> lk(mu); return cancel; }

    // ---- consumer side -------------------------------------------------------------------------------------------------------------
    void give_back(Cursor &l) {                                     // (under the lock) parallel mode: the last reader of a retired batch returns the slot
        if (!l.cur) return;
        Batch *hb = l.cur; hb->readers--;
        if (n_workers == 1 || (hb->retired && hb->readers == 0)) { l.owner->free_slots.push_back(hb); cv_free.notify_all(); }
        l.cur = nullptr;
    }
    // hands the calling worker its next run of rows: a whole batch (ordered mode) or a slice of at most `want` rows of a ready batch.
    // false at the end of the scan, or on a producer error (`error`).
    bool next_rows(Cursor &l, uint64_t want) {
        std::unique_lock<std::mutex> lk(mu);
        give_back(l);
        for (;;) {
            if (!error.empty()) return false;
            for (size_t k = 0; k < src.size(); k++) {
                Source *s = src[n_workers == 1 ? cur_src : (cur_src + k) % src.size()];
                while (!s->ready.empty()) {
                    Batch *hb = s->ready.front();
                    if (n_workers == 1) {
                        s->ready.pop_front(); hb->readers = 1;
                        l.cur = hb; l.owner = s; l.pos = 0; l.end = hb->n;
                        return true;
                    }
                    if (hb->next >= hb->n) {                        // every row is claimed
                        s->ready.pop_front(); hb->retired = true;
                        if (hb->readers == 0) { s->free_slots.push_back(hb); cv_free.notify_all(); }
                        continue;
                    }
                    l.cur = hb; l.owner = s; l.pos = hb->next; l.end = hb->next + (int64_t)want < hb->n ? hb->next + (int64_t)want : hb->n;
                    hb->next = l.end; hb->readers++;
                    return true;
                }
                if (n_workers == 1) {
                    if (s->done) {
                        if (!s->clean_end) return false;            // the stream ended on an error inside this source: the scan ends here, silently
                        if (cur_src + 1 < src.size()) { cur_src++; k = (size_t)-1; continue; }
                    }
                    break;
                }
            }
            bool all_done = true;
            for (Source *s : src) if (!s->done || !s->ready.empty()) all_done = false;
            if (all_done) {
                if (!all_done_seen) { all_done_seen = true; if (on_all_done) on_all_done(error); }
                return false;
            }
            cv_ready.wait(lk);
        }
    }
    // One scan call: up to vector_size rows through fill(batch, s, take, row_count) -- rows [s, s + take) of the batch -> rows [row_count,
    // row_count + take) of the chunk.  Returns the chunk's size (0 = done), or -1 with err = the producer's error.
    template <class Fill>
    int64_t fill_chunk(Cursor &l, uint64_t vector_size, std::string &err, Fill fill) {
        if (l.done) return 0;
        uint64_t row_count = 0;
        while (row_count < vector_size) {
            if (!l.cur || l.pos >= l.end) {
                if (n_workers > 1 && row_count > 0) break;          // parallel mode: one slice per chunk
                if (!next_rows(l, vector_size)) {                   // (it has given the worker's slot back)
                    l.done = true;
                    { std::lock_guard<std::mutex> lk(mu); err = error; }
                    if (!err.empty()) return -1;
                    break;
                }
            }
            uint64_t take = (uint64_t)(l.end - l.pos); if (take > vector_size - row_count) take = vector_size - row_count;
            fill(*l.cur, l.pos, take, row_count);
            row_count += take; l.pos += (int64_t)take;
        }
        return (int64_t)row_count;
    }
};

// ---- read-back overlap: the copy of batch k runs on copy slot k & 1 while batch k + 1 is scanned; batch k is handed to the fill threads one
// turn later, after fetch_wait(slot) and the reader's landed(batch) step.  serial (DHTS_OVERLAP_READBACK=0): copy, landed, hand over.
// Every callable returns true on success (landed returns nothing).
template <class Batch, class Fetch, class FetchBegin, class FetchWait, class Landed>
struct Readback {
    Pipeline<Batch> &pipe; typename Pipeline<Batch>::Source &src; bool serial;
    Fetch fetch; FetchBegin fetch_begin; FetchWait fetch_wait; Landed landed;
    Batch *pending = nullptr; int pending_slot = 0, slot_no = 0;
    bool begin(Batch *hb) { return serial ? fetch(hb) : fetch_begin(hb, slot_no); }       // start (serial: make) the copy of this batch
    bool flush() {                                                   // hand over the batch whose copy was begun one turn ago
        if (!pending) return true;
        Batch *hb = pending; pending = nullptr;
        if (!fetch_wait(pending_slot)) return false;
        landed(hb); pipe.publish(src, hb);
        return true;
    }
    bool turn(Batch *hb) {                                           // after begin(hb) and the reader's own bookkeeping
        if (!flush()) return false;
        if (serial) { landed(hb); pipe.publish(src, hb); }
        else { pending = hb; pending_slot = slot_no; slot_no ^= 1; }
        return true;
    }
};
template <class Batch, class Fetch, class FetchBegin, class FetchWait, class Landed>
static inline Readback<Batch, Fetch, FetchBegin, FetchWait, Landed> make_readback(Pipeline<Batch> &pipe, typename Pipeline<Batch>::Source &src, bool serial, Fetch f, FetchBegin fb, FetchWait fw, Landed ld) {
    return Readback<Batch, Fetch, FetchBegin, FetchWait, Landed>{pipe, src, serial, f, fb, fw, ld};
}
#endif
